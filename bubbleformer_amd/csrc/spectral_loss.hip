// The shell-weighted spectral criterion (utils.losses.SpectralLpLoss; no reference program): the training configuration's
// relative L2 taken in Fourier space with one weight per radial shell and per field.  pred, y are [rows][H][W] fp32, rows = B * T * C, field
// c = row % C; X(ky, kx) = sum x[r][s] exp(-2 pi i (ky r / H + kx s / W)), the shell q(ky, kx) section 18's, by the same text (csrc/fft_lines.h):
//   S_e[row] = sum_k w[c][q(k)] |E_k|^2 / (H W),  S_y the same over Y,  rho = sqrt(S_e / S_y),  loss = sum_c a_c mean_{b,t} rho
//   dpred    = g a_c / (B T) * Re ifft2(w E) / sqrt(S_e S_y)
// The transforms are fft_lines.h's Stockham autosorts in LDS, here in fp32 (float2) on lines an odd stride apart; twiddles are formed in fp64
// by sincospi and rounded once; every sum is fp64 in an order that depends on (H, W) alone (no float atomics): two calls give the same bits,
// a frame the same bits alone and in a batch.
//
// Launches of the forward, all on the caller's stream:
//   tables    exp(-2 pi i j / N) for N = W and N = H, and the shell of every mode (ky, kx <= W/2) as int16 (built in every call, nothing kept);
//   rows      a group of rows of one field: e = pred - y and y, each transformed along x (never both in one complex transform), the Hermitian
//             halves kx <= W/2 stored as complex fp32;
//   columns   up to 16 adjacent columns kx (a 128-byte segment per row of the group): y, then e, transformed along y; m w |.|^2 and m |.|^2
//             added in fp64 (m = 2 for a mirrored column); for e the column is multiplied by w, conjugated and transformed again (the inverse
//             is the forward transform under conjugation) and stored back in place: what the backward reads;
//   finish    one workgroup: column groups in order, ratios, means over the frames, field terms, loss; leaves {S_e, S_y}.
// The backward is one launch: a group of rows of the saved half-spectrum, the Hermitian line rebuilt in LDS, transformed along x, the real part
// times the row coefficient written to every element of dpred.
#include "fft_lines.h"
#include <algorithm>
#include <string>

namespace {
constexpr int NT = 256;
constexpr int MAX_SIDE = 1024;
constexpr int LINE_ELEMS = 3104;                   // complex fp32 per ping-pong buffer (16 lines of stride 193, 2 of 1025): 2 x 24.25 KiB, plus 8 KiB of twiddles
constexpr int MAX_LINES = 16;                      // 16 fp32-complex columns are a 128-byte segment
constexpr int SLP_MAX_C = 16;
constexpr int PART = 4;                            // {sum w |E|^2, sum w |Y|^2, sum |E|^2, sum |Y|^2} per (row, column group)

typedef float2 cplx;
static_assert(NT == FFT_NT, "the transform's stage loops stride by the workgroup size");
int line_stride(int n) { return n | 1; }           // odd: the lines of a transposed load fall into different LDS banks
int lines_for(int n, int fields) { return std::max(1, std::min(MAX_LINES / fields, LINE_ELEMS / (fields * line_stride(n)))); }

struct SlpFields { double a[SLP_MAX_C]; };
struct SlpLayout {                                 // byte offsets into the workspace, each 16-byte aligned
    long tw_w, tw_h, shell, spec_y, part, rho, total;
    int Wh, rows_per, rgroups, cols_per, cgroups, back_per, bgroups;
    SlpLayout() = default;
    SlpLayout(long rows, int H, int W) {
        Wh = W / 2 + 1;
        rows_per = lines_for(W, 2); rgroups = (H + rows_per - 1) / rows_per;
        cols_per = lines_for(H, 1); cgroups = (Wh + cols_per - 1) / cols_per;
        back_per = lines_for(W, 1); bgroups = (H + back_per - 1) / back_per;
        auto up = [](long b) { return (b + 15) / 16 * 16; };
        tw_w = 0; tw_h = tw_w + up(8L * W); shell = tw_h + up(8L * H);
        spec_y = shell + up(2L * H * Wh);
        part = spec_y + up(rows * H * Wh * 8);
        rho = part + up(rows * cgroups * PART * 8);
        total = rho + up(rows * 2 * 8);
    }
};
struct SlpArgs {
    const float* pred; const float* y;
    long rows; int C, H, W, K;
    Plan pw, ph;
    SlpLayout lay;
    char* ws; const double* wtab; cplx* spec;
};
struct SlpColsArgs {                               // what the column kernel reads, and no more: it is the one that is short of scalar registers
    const cplx* tw; const short* shell; const double* wtab;
    cplx* spec_e; cplx* spec_y; double* part;
    int C, H, W, K, per, groups;
    Plan ph;
};

// ---------------------------------------------------------------------------- the transform (fft_lines.h), lines an odd stride apart
struct FftLds { cplx tw[MAX_SIDE]; cplx a[LINE_ELEMS]; cplx b[LINE_ELEMS]; };

__global__ void __launch_bounds__(NT) slp_tables_kernel(cplx* tw_w, cplx* tw_h, short* shell, int H, int W) {
    const int Wh = W / 2 + 1;
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i < W) tw_w[i] = twiddle<cplx>((int)i, W);
    else if (i < W + H) tw_h[i - W] = twiddle<cplx>((int)(i - W), H);
    else if (i < W + H + (long)H * Wh) {
        const long m = i - W - H;
        const int ky = (int)(m / Wh), kx = (int)(m - (long)ky * Wh);
        shell[m] = (short)shell_of(ky <= H / 2 ? ky : ky - H, kx, H, W);
    }
}

// rows: workgroup = (row, group of rows_per lines y).  spec_e / spec_y [row][y][kx] complex fp32, kx in [0, W/2]
__global__ void __launch_bounds__(NT) slp_rows_kernel(SlpArgs a) {
    __shared__ FftLds L;
    const int H = a.H, W = a.W, Wh = a.lay.Wh, per = a.lay.rows_per, groups = a.lay.rgroups, ls = W | 1;
    const int g = blockIdx.x % groups;
    const long r = blockIdx.x / groups;
    const int y0 = g * per, n = min(per, H - y0);
    const cplx* tw = (const cplx*)(a.ws + a.lay.tw_w);
    for (int i = threadIdx.x; i < W; i += NT) L.tw[i] = tw[i];
    const long base = (r * H + y0) * W;
    for (int i = threadIdx.x; i < n * W; i += NT) {
        const int l = i / W, x = i - l * W;
        const float p = a.pred[base + i], t = a.y[base + i];
        L.a[l * ls + x] = make_float2(p - t, 0.f);
        L.a[(n + l) * ls + x] = make_float2(t, 0.f);
    }
    __syncthreads();
    const cplx* out = fft_lines(L.a, L.b, L.tw, a.pw, 2 * n, ls);
    cplx* se = a.spec + (r * H + y0) * Wh;
    cplx* sy = (cplx*)(a.ws + a.lay.spec_y) + (r * H + y0) * Wh;
    for (int i = threadIdx.x; i < n * Wh; i += NT) {
        const int l = i / Wh, kx = i - l * Wh;
        se[i] = out[l * ls + kx];
        sy[i] = out[(n + l) * ls + kx];
    }
}

// columns: workgroup = (row, group of cols_per columns kx).  part[row][group] = the four sums of the group, every thread's fp64 sum over its
// modes in a set order, the lanes by butterfly, the waves in order.
__global__ void __launch_bounds__(NT) slp_cols_kernel(SlpColsArgs a) {
    __shared__ FftLds L;
    __shared__ double red[NT / 64][PART];      // several values at once in this kernel's own order, which its restatement's bits pin: not bf_common.h's block_reduce
    const int H = a.H, W = a.W, Wh = W / 2 + 1, per = a.per, groups = a.groups, ls = H | 1;
    const int g = blockIdx.x % groups;
    const long r = blockIdx.x / groups;
    const int kx0 = g * per, n = min(per, Wh - kx0);
    for (int i = threadIdx.x; i < H; i += NT) L.tw[i] = a.tw[i];
    const short* shell = a.shell + kx0;
    const double* wrow = a.wtab + (r % a.C) * a.K;
    double e_w = 0.0, y_w = 0.0, e_1 = 0.0, y_1 = 0.0;
    cplx *in = L.a, *out = L.b;
#pragma unroll 1
    for (int t = 0; t < 3; ++t) {                                          // y forward, e forward, w e inverse: one transform each
        cplx* plane = (t == 0 ? a.spec_y : a.spec_e) + r * H * Wh + kx0;
        __syncthreads();                                                   // the previous transform's result has been read (or rewritten)
        if (t < 2) {
            in = L.a; out = L.b;
            for (int i = threadIdx.x; i < n * H; i += NT) {
                const int yy = i / n, l = i - yy * n;
                in[l * ls + yy] = plane[(long)yy * Wh + l];
            }
            __syncthreads();
        }
        cplx* X = fft_lines(in, out, L.tw, a.ph, n, ls);
        if (t == 2) {                                                      // fft(conj(w E)) = conj of the unnormalised inverse
            for (int i = threadIdx.x; i < n * H; i += NT) {
                const int yy = i / n, l = i - yy * n;
                plane[(long)yy * Wh + l] = X[l * ls + yy];
            }
            break;
        }
        double sw = 0.0, s1 = 0.0;
        for (int i = threadIdx.x; i < n * H; i += NT) {
            const int ky = i / n, l = i - ky * n, kx = kx0 + l;
            const cplx u = X[l * ls + ky];
            const double w = wrow[shell[(long)ky * Wh + l]];
            const double m = (kx == 0 || 2 * kx == W) ? 1.0 : 2.0;
            const double pw = m * ((double)u.x * (double)u.x + (double)u.y * (double)u.y);
            s1 += pw; sw += w * pw;
            if (t == 1) { const float wf = (float)w; X[l * ls + ky] = make_float2(wf * u.x, -(wf * u.y)); }        // conj(w E): every thread its own modes
        }
        if (t == 0) { y_w = sw; y_1 = s1; } else { e_w = sw; e_1 = s1; in = X; out = X == L.a ? L.b : L.a; }
    }
    e_w = wave_sum(e_w); y_w = wave_sum(y_w); e_1 = wave_sum(e_1); y_1 = wave_sum(y_1);
    if ((threadIdx.x & 63) == 0) { double* t = red[threadIdx.x >> 6]; t[0] = e_w; t[1] = y_w; t[2] = e_1; t[3] = y_1; }
    __syncthreads();
    if (threadIdx.x < PART) {
        double t = red[0][threadIdx.x];
        for (int w = 1; w < NT / 64; ++w) t += red[w][threadIdx.x];
        a.part[(r * groups + g) * PART + threadIdx.x] = t;
    }
}

// One workgroup: sums[row] = {S_e, S_y}, the column groups in order, over H W; rho = sqrt(S_e / S_y) and the same at w = 1; terms[c] = a_c * mean
// over the frames of rho, terms[C + c] the same at w = 1, added in a fixed order; loss = sum_c terms[c].  All fp64, each output rounded once.
__global__ void __launch_bounds__(NT) slp_finish_kernel(SlpArgs a, SlpFields fa, double* __restrict__ sums, float* __restrict__ loss, float* __restrict__ terms) {
    __shared__ double red[NT / 64];
    const int C = a.C, groups = a.lay.cgroups;
    const long frames = a.rows / C;
    const double* part = (const double*)(a.ws + a.lay.part);
    double* rho = (double*)(a.ws + a.lay.rho);
    const double px = (double)a.H * (double)a.W;
    for (long row = threadIdx.x; row < a.rows; row += NT) {
        double s[PART] = {0.0, 0.0, 0.0, 0.0};
        for (int g = 0; g < groups; ++g)
            for (int k = 0; k < PART; ++k) s[k] += part[(row * groups + g) * PART + k];
        sums[2 * row] = s[0] / px; sums[2 * row + 1] = s[1] / px;
        rho[2 * row] = sqrt(s[0] / s[1]); rho[2 * row + 1] = sqrt(s[2] / s[3]);
    }
    __syncthreads();
    double total = 0.0;
    for (int c = 0; c < C; ++c) {
        double aw = 0.0, a1 = 0.0;
        for (long f = threadIdx.x; f < frames; f += NT) { aw += rho[2 * (f * C + c)]; a1 += rho[2 * (f * C + c) + 1]; }
        const double tw = fa.a[c] * (block_reduce<RED_SUM, NT / 64>(aw, red) / (double)frames), t1 = fa.a[c] * (block_reduce<RED_SUM, NT / 64>(a1, red) / (double)frames);
        if (threadIdx.x == 0) { terms[c] = (float)tw; terms[C + c] = (float)t1; }
        total += tw;
    }
    if (threadIdx.x == 0) loss[0] = (float)total;
}

// backward: workgroup = (row, group of back_per lines y) of the saved half-spectrum Z = fft_y(conj(w E)): the Hermitian line in LDS, one
// transform along x, dpred = coef * Re(.), coef = g a_c / frames / sqrt(S_e S_y) / (H W) in fp64, every element rounded once; S_e = 0 writes zeros
__global__ void __launch_bounds__(NT) slp_bwd_kernel(const cplx* __restrict__ spec, const float* __restrict__ gout, const double* __restrict__ sums, long rows,
                                                    int C, int H, int W, int per, int groups, Plan pw, SlpFields fa, float* __restrict__ dpred) {
    __shared__ FftLds L;
    const int Wh = W / 2 + 1, ls = W | 1;
    const int g = blockIdx.x % groups;
    const long r = blockIdx.x / groups;
    const int y0 = g * per, n = min(per, H - y0);
    for (int i = threadIdx.x; i < W; i += NT) L.tw[i] = twiddle<cplx>(i, W);
    const double se = sums[2 * r], sy = sums[2 * r + 1];
    const double coef = se != 0.0 ? (double)gout[0] * fa.a[r % C] / (double)(rows / C) / sqrt(se * sy) / ((double)H * (double)W) : 0.0;
    const cplx* src = spec + (r * H + y0) * Wh;
    for (int i = threadIdx.x; i < n * W; i += NT) {
        const int l = i / W, kx = i - l * W;
        cplx v;
        if (kx < Wh) v = src[l * Wh + kx];
        else { v = src[l * Wh + W - kx]; v.y = -v.y; }
        L.a[l * ls + kx] = v;
    }
    __syncthreads();
    const cplx* out = fft_lines(L.a, L.b, L.tw, pw, n, ls);
    float* d = dpred + (r * H + y0) * W;
    for (int i = threadIdx.x; i < n * W; i += NT) {
        const int l = i / W, x = i - l * W;
        d[i] = se != 0.0 ? (float)(coef * (double)out[l * ls + x].x) : 0.f;
    }
}

bool slp_sizes_ok(int64_t frames, int C, int H, int W) {
    return frames > 0 && frames <= (int64_t)1 << 20 && C > 0 && C <= SLP_MAX_C && H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE;
}
// the checks bf_slp_fwd and bf_slp_bwd share; NULL = accepted
const char* slp_refusal(int64_t frames, int C, int H, int W, const double* field_weights) {
    if (!slp_sizes_ok(frames, C, H, W)) return "B*T must be 1 .. 2^20, C 1 .. 16, H and W 1 .. 1024";
    for (int c = 0; field_weights && c < C; ++c)
        if (!(field_weights[c] >= 0.0 && field_weights[c] < INFINITY)) return "field weights must be finite and >= 0";
    return nullptr;
}
SlpFields slp_fields(const double* field_weights, int C) {
    SlpFields fa;
    for (int c = 0; c < SLP_MAX_C; ++c) fa.a[c] = c < C ? (field_weights ? field_weights[c] : 1.0) : 0.0;
    return fa;
}
}  // namespace

extern "C" int64_t bf_slp_ws_bytes(int64_t frames, int C, int H, int W) {
    if (!slp_sizes_ok(frames, C, H, W)) return -1;
    return SlpLayout(frames * C, H, W).total;
}

extern "C" int bf_slp_fwd(const float* pred, const float* y, int64_t frames, int C, int H, int W, const double* shell_weights,
                          const double* shell_weights_host, int K, const double* field_weights, float* loss, float* terms, double* sums, void* spec,
                          void* ws, int64_t ws_bytes, bf_stream_t stream) {
    BF_REQUIRE(pred && y && shell_weights && shell_weights_host && loss && terms && sums && spec && ws, "bf_slp_fwd: null pointer");
    const char* why = slp_refusal(frames, C, H, W, field_weights);
    if (why) return bf_fail_msg((std::string("bf_slp_fwd: ") + why).c_str(), __FILE__, __LINE__);
    BF_REQUIRE(K == shell_count(H, W), "bf_slp_fwd: K is not the shell count of (H, W)");
    for (int c = 0; c < C; ++c) {
        bool live = false;
        for (int q = 0; q < K; ++q) {
            const double w = shell_weights_host[(long)c * K + q];
            BF_REQUIRE(w >= 0.0 && w < INFINITY, "bf_slp_fwd: shell weights must be finite and >= 0");
            live |= w > 0.0;
        }
        BF_REQUIRE(live, "bf_slp_fwd: a field's shell weights are all zero");
    }
    BF_REQUIRE((((uintptr_t)pred | (uintptr_t)y | (uintptr_t)loss | (uintptr_t)terms) & 3) == 0 &&
               (((uintptr_t)shell_weights | (uintptr_t)sums | (uintptr_t)spec) & 7) == 0 && ((uintptr_t)ws & 15) == 0, "bf_slp_fwd: misaligned pointer");
    SlpArgs a{};
    a.pred = pred; a.y = y; a.rows = frames * C; a.C = C; a.H = H; a.W = W; a.K = K;
    a.lay = SlpLayout(a.rows, H, W);
    BF_REQUIRE(ws_bytes >= a.lay.total, "bf_slp_fwd: workspace smaller than bf_slp_ws_bytes");
    BF_REQUIRE(a.rows * std::max(a.lay.rgroups, a.lay.cgroups) < ((int64_t)1 << 31), "bf_slp_fwd: too many frames");
    a.pw = make_plan(W); a.ph = make_plan(H); a.ws = (char*)ws; a.wtab = shell_weights; a.spec = (cplx*)spec;
    hipStream_t st = (hipStream_t)stream;
    const long ntab = (long)W + H + (long)H * a.lay.Wh;
    hipLaunchKernelGGL(slp_tables_kernel, dim3((unsigned)((ntab + NT - 1) / NT)), dim3(NT), 0, st, (cplx*)(a.ws + a.lay.tw_w), (cplx*)(a.ws + a.lay.tw_h),
                       (short*)(a.ws + a.lay.shell), H, W);
    BF_CHECK_LAUNCH();
    hipLaunchKernelGGL(slp_rows_kernel, dim3((unsigned)(a.rows * a.lay.rgroups)), dim3(NT), 0, st, a);
    BF_CHECK_LAUNCH();
    const SlpColsArgs ca{(const cplx*)(a.ws + a.lay.tw_h), (const short*)(a.ws + a.lay.shell), shell_weights, a.spec, (cplx*)(a.ws + a.lay.spec_y),
                         (double*)(a.ws + a.lay.part), C, H, W, K, a.lay.cols_per, a.lay.cgroups, a.ph};
    hipLaunchKernelGGL(slp_cols_kernel, dim3((unsigned)(a.rows * a.lay.cgroups)), dim3(NT), 0, st, ca);
    BF_CHECK_LAUNCH();
    hipLaunchKernelGGL(slp_finish_kernel, dim3(1), dim3(NT), 0, st, a, slp_fields(field_weights, C), sums, loss, terms);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_slp_bwd(const void* spec, const float* g, const double* sums, int64_t frames, int C, int H, int W, const double* field_weights,
                          float* dpred, bf_stream_t stream) {
    BF_REQUIRE(spec && g && sums && dpred, "bf_slp_bwd: null pointer");
    const char* why = slp_refusal(frames, C, H, W, field_weights);
    if (why) return bf_fail_msg((std::string("bf_slp_bwd: ") + why).c_str(), __FILE__, __LINE__);
    BF_REQUIRE((((uintptr_t)g | (uintptr_t)dpred) & 3) == 0 && (((uintptr_t)sums | (uintptr_t)spec) & 7) == 0, "bf_slp_bwd: misaligned pointer");
    const int64_t rows = frames * C;
    const char *s0 = (const char*)spec, *s1 = s0 + rows * H * (W / 2 + 1) * 8, *d0 = (const char*)dpred, *d1 = d0 + rows * H * W * 4;
    BF_REQUIRE(d1 <= s0 || s1 <= d0, "bf_slp_bwd: the gradient cannot alias the saved spectrum");
    const SlpLayout lay(rows, H, W);
    BF_REQUIRE(rows * lay.bgroups < ((int64_t)1 << 31), "bf_slp_bwd: too many frames");
    hipLaunchKernelGGL(slp_bwd_kernel, dim3((unsigned)(rows * lay.bgroups)), dim3(NT), 0, (hipStream_t)stream, (const cplx*)spec, g, sums, (long)rows, C, H, W,
                       lay.back_per, lay.bgroups, make_plan(W), slp_fields(field_weights, C), dpred);
    BF_CHECK_LAUNCH();
    return 0;
}
