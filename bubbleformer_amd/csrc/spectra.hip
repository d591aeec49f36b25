// Where a prediction is wrong, and at which scales: per (frame, field) the pointwise error rows (RMSE, maximum error, RMSE over the outer ring
// and over the cells at the liquid-vapour interface of the SIMULATED frame) and the shell power spectra of the error, of the prediction and of
// the target, with the band-limited RMSE of the error.  The reference has no program for this; DESIGN.md section 18 has the definitions.
// Everything is fp64 arithmetic on fp32 inputs, rounded once at the store; every sum is a fixed-order sum of fixed-order partials (no float
// atomics), so two calls give the same bits and a frame has the same bits alone and in a batch.
//
// Launches of one call, all on the caller's stream, all through the caller's workspace:
//   twiddles   exp(-2 pi i j / N) for N = W and N = H, fp64, by sincospi (built on the device in every call: no host table, nothing kept);
//   mask       (interface rows only) one byte per cell of every signed-distance frame: the (2r+1)^2 window holds vapour AND liquid;
//   pointwise  grid (chunks of a frame) x frames: one pass over prediction and target, {sum e^2, ring sum, interface sum, max, NaN, cells};
//   rows       L rows of one real field (e = p - y, p or y: never two fields in one transform) -> Hermitian half-spectrum [y][kx <= W/2];
//   columns    L columns kx of that half-spectrum -> the full transform in LDS -> |X|^2 per shell, per column in a set order;
//   finish     one workgroup per frame adds chunks and column groups in order, divides, takes roots and bands, rounds.
// The transform and a mode's shell are fft_lines.h's (the spectral criterion's too): a Stockham autosort in LDS over the mixed-radix
// factorisation of the side, here in complex fp64 on dense lines (line stride = side); the shell is decided in int64.
#include "clip_store.h"
#include "fft_lines.h"
#include <algorithm>

namespace {
constexpr int NT = 256;
constexpr int MAX_SIDE = 1024;
constexpr int LINE_ELEMS = 1024;                   // complex fp64 per ping-pong buffer: 2 x 16 KiB, plus 16 KiB of twiddles
constexpr int MAX_LINES = 8;
constexpr int PW_PIX = 4096, PW_MAX_CHUNKS = 64;   // pixels per pointwise workgroup until PW_MAX_CHUNKS share a frame
constexpr int PW_VALS = 6;                         // {sum e^2, ring sum e^2, interface sum e^2, max |e|, NaN seen, interface cells}

typedef double2 cplx;
static_assert(NT == FFT_NT, "the transform's stage loops stride by the workgroup size");
int lines_for(int n) { return std::max(1, std::min(MAX_LINES, LINE_ELEMS / n)); }
int pw_chunks(int H, int W) { return (int)std::max<long>(1, std::min<long>(PW_MAX_CHUNKS, ((long)H * W + PW_PIX - 1) / PW_PIX)); }

struct WsLayout {                                  // byte offsets into the workspace, each 16-byte aligned
    long tw_w, tw_h, mask, pw, inter, shells, total;
    int Wh, groups, K, chunks;
    WsLayout() = default;
    WsLayout(long F, int H, int W) {
        Wh = W / 2 + 1; groups = (Wh + lines_for(H) - 1) / lines_for(H); K = shell_count(H, W); chunks = pw_chunks(H, W);
        auto up = [](long b) { return (b + 15) / 16 * 16; };
        tw_w = 0; tw_h = tw_w + 16L * W; mask = tw_h + 16L * H;
        pw = mask + up(F * H * W);
        inter = pw + up(F * chunks * PW_VALS * 8);
        shells = inter + F * 3 * H * Wh * 16;
        total = shells + up(F * 3 * groups * K * 8);
    }
};

// ---------------------------------------------------------------------------- the frames of a call
// bf_field_errors: frame f of pred / target / sdf.  bf_rollout_errors: f = (b * T + t) * C + c of this step's prediction, the target read where
// it lies in the store with the gather's own map and normalisation (so it has the bits bf_clip_gather returns), the signed distance raw.
struct ErrArgs {
    int rollout; RolloutStep v; int sdf_c;         // the rollout view, or:
    const float* pred; const float* tgt; const float* sdf;
    long F; int H, W, radius, lo, hi, nfld, fld[3];        // fld: which of {0: e, 1: p, 2: y} are transformed, in slot order
    int rows_h, rows_w;                            // lines per workgroup of the row and of the column pass
    Plan pw, ph;
    char* ws; WsLayout lay;
    float* rmse; float* max_error; float* boundary_rmse; float* interface_rmse; int* interface_cells;
    float* bands; float* spec[3];
};
struct FrameView {                                 // value (y, x) of a frame on the model's grid
    const float* p; int ld, Hs, Ws; float sy, sx, d, q; bool ident, norm;
    __device__ __forceinline__ float at(int y, int x) const {
        const float v = p[(long)nearest_src(y, sy, Hs, ident) * ld + nearest_src(x, sx, Ws, ident)];
        return norm ? clip_norm(v, d, q) : v;
    }
};
// false: a rollout step outside [0, steps), where nothing is written
__device__ __forceinline__ bool live(const ErrArgs& a, int& s) { s = a.rollout ? a.v.current() : 0; return s >= 0; }
__device__ __forceinline__ FrameView pred_view(const ErrArgs& a, long f) {
    return FrameView{a.rollout ? a.v.pred + f * a.H * (long)a.W : a.pred + f * a.H * (long)a.W, a.W, a.H, a.W, 1.f, 1.f, 0.f, 1.f, true, false};
}
__device__ __forceinline__ FrameView target_view(const ErrArgs& a, long f, int s) {
    if (!a.rollout) return FrameView{a.tgt + f * a.H * (long)a.W, a.W, a.H, a.W, 1.f, 1.f, 0.f, 1.f, true, false};
    const RolloutStep& v = a.v;
    const int c = (int)(f % v.C), t = (int)((f / v.C) % v.T), b = (int)(f / ((long)v.C * v.T));
    return FrameView{v.stored(c, v.frame(s, b, t)), v.W, v.H, v.W, v.sy(), v.sx(), v.diff[c], v.dv[c], v.ident(), true};
}
__device__ __forceinline__ FrameView sdf_view(const ErrArgs& a, long m, int s) {       // m: the frame (direct) or b * T + t (rollout)
    if (!a.rollout) return FrameView{a.sdf + m * a.H * (long)a.W, a.W, a.H, a.W, 1.f, 1.f, 0.f, 1.f, true, false};
    const RolloutStep& v = a.v;
    return FrameView{v.stored(a.sdf_c, v.frame(s, (int)(m / v.T), (int)(m % v.T))), v.W, v.H, v.W, v.sy(), v.sx(), 0.f, 1.f, v.ident(), false};
}
__device__ __forceinline__ long mask_frame(const ErrArgs& a, long f) { return a.rollout ? f / a.v.C : f; }
__device__ __forceinline__ long out_row(const ErrArgs& a, long f, int s) {
    if (!a.rollout) return f;
    const RolloutStep& v = a.v;
    const int c = (int)(f % v.C), t = (int)((f / v.C) % v.T), b = (int)(f / ((long)v.C * v.T));
    return v.row(s, b, t) * v.C + c;
}

// ---------------------------------------------------------------------------- twiddles, mask, pointwise rows
__global__ void __launch_bounds__(NT) twiddle_kernel(cplx* tw_w, int W, cplx* tw_h, int H) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= W + H) return;
    const int n = i < W ? W : H, j = i < W ? i : i - W;
    (i < W ? tw_w : tw_h)[j] = twiddle<cplx>(j, n);
}

__global__ void __launch_bounds__(NT) interface_mask_kernel(ErrArgs a, long mframes) {
    int s;
    if (!live(a, s)) return;
    const long px = (long)a.H * a.W, i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= mframes * px) return;
    const long m = i / px;
    const int y = (int)((i - m * px) / a.W), x = (int)((i - m * px) % a.W), r = a.radius;
    const FrameView phi = sdf_view(a, m, s);
    bool vap = false, liq = false;
    for (int yy = max(y - r, 0); yy <= min(y + r, a.H - 1) && !(vap && liq); ++yy)
        for (int xx = max(x - r, 0); xx <= min(x + r, a.W - 1); ++xx) {
            const bool v = phi.at(yy, xx) > 0.f;                           // false for NaN and for an exact zero: the census's convention
            vap |= v; liq |= !v;
        }
    ((unsigned char*)(a.ws + a.lay.mask))[i] = vap && liq;
}

__global__ void __launch_bounds__(NT) pointwise_kernel(ErrArgs a) {
    __shared__ double red[NT / 64][PW_VALS];      // several values at once in this kernel's own order, which its restatement's bits pin: not bf_common.h's block_reduce
    int s;
    if (!live(a, s)) return;
    const int chunks = a.lay.chunks, H = a.H, W = a.W;
    const long f = blockIdx.x / chunks, px = (long)H * W;
    const int chunk = blockIdx.x % chunks;
    const long per = (px + chunks - 1) / chunks, lo = chunk * per, hi = min(px, lo + per);
    const FrameView P = pred_view(a, f), Y = target_view(a, f, s);
    const bool want_mask = a.interface_rmse || a.interface_cells;
    const unsigned char* mask = (const unsigned char*)(a.ws + a.lay.mask) + mask_frame(a, f) * px;
    double se = 0.0, sr = 0.0, si = 0.0, mx = 0.0, bad = 0.0, cells = 0.0;
    for (long i = lo + threadIdx.x; i < hi; i += NT) {
        const int y = (int)(i / W), x = (int)(i - (long)y * W);
        const double e = (double)P.at(y, x) - (double)Y.at(y, x), e2 = e * e;
        se += e2;
        if (y == 0 || y == H - 1 || x == 0 || x == W - 1) sr += e2;
        if (want_mask && mask[i]) { si += e2; cells += 1.0; }
        if (e != e) bad = 1.0; else mx = fmax(mx, fabs(e));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        se += __shfl_xor(se, o, 64); sr += __shfl_xor(sr, o, 64); si += __shfl_xor(si, o, 64); cells += __shfl_xor(cells, o, 64);
        mx = fmax(mx, __shfl_xor(mx, o, 64)); bad = fmax(bad, __shfl_xor(bad, o, 64));
    }
    if ((threadIdx.x & 63) == 0) { double* r = red[threadIdx.x >> 6]; r[0] = se; r[1] = sr; r[2] = si; r[3] = mx; r[4] = bad; r[5] = cells; }
    __syncthreads();
    if (threadIdx.x < PW_VALS) {
        const int k = threadIdx.x;
        double acc = red[0][k];
        for (int w = 1; w < NT / 64; ++w) acc = (k == 3 || k == 4) ? fmax(acc, red[w][k]) : acc + red[w][k];
        ((double*)(a.ws + a.lay.pw))[((long)f * chunks + chunk) * PW_VALS + k] = acc;
    }
}

// ---------------------------------------------------------------------------- the transform (fft_lines.h), dense lines
struct FftLds { cplx tw[MAX_SIDE]; cplx a[LINE_ELEMS]; cplx b[LINE_ELEMS]; };

// rows: workgroup = (frame, field slot, group of rows_w rows).  inter [frame][slot][y][kx] complex fp64, kx in [0, W/2]
__global__ void __launch_bounds__(NT) spectra_rows_kernel(ErrArgs a) {
    __shared__ FftLds L;
    int s;
    if (!live(a, s)) return;
    const int H = a.H, W = a.W, Wh = a.lay.Wh, per = a.rows_w, groups = (H + per - 1) / per;
    const int g = blockIdx.x % groups, slot = (int)((blockIdx.x / groups) % a.nfld), fld = a.fld[slot];
    const long f = blockIdx.x / ((long)groups * a.nfld);
    const int y0 = g * per, lines = min(per, H - y0);
    const cplx* tw = (const cplx*)(a.ws + a.lay.tw_w);
    for (int i = threadIdx.x; i < W; i += NT) L.tw[i] = tw[i];
    const FrameView P = pred_view(a, f), Y = target_view(a, f, s);
    for (int i = threadIdx.x; i < lines * W; i += NT) {
        const int l = i / W, x = i - l * W;
        const double p = fld != 2 ? (double)P.at(y0 + l, x) : 0.0, y = fld != 1 ? (double)Y.at(y0 + l, x) : 0.0;
        L.a[i] = make_double2(fld == 0 ? p - y : fld == 1 ? p : y, 0.0);
    }
    __syncthreads();
    const cplx* out = fft_lines(L.a, L.b, L.tw, a.pw, lines);
    cplx* inter = (cplx*)(a.ws + a.lay.inter) + ((f * 3 + slot) * H + y0) * Wh;
    for (int i = threadIdx.x; i < lines * Wh; i += NT) {
        const int l = i / Wh, kx = i - l * Wh;
        inter[(long)l * Wh + kx] = out[l * W + kx];
    }
}

// columns: workgroup = (frame, field slot, group of rows_h columns kx).  For a column the shell does not fall as |fy| grows, so the modes of
// shell q are one run of |fy|: thread q finds the run in the column's shell table and adds it, +fy before -fy, column after column.
__global__ void __launch_bounds__(NT) spectra_cols_kernel(ErrArgs a) {
    __shared__ FftLds L;
    __shared__ short shell[LINE_ELEMS / 2 + MAX_LINES];
    int s;
    if (!live(a, s)) return;
    const int H = a.H, W = a.W, Wh = a.lay.Wh, per = a.rows_h, groups = a.lay.groups, K = a.lay.K;
    const int g = blockIdx.x % groups, slot = (int)((blockIdx.x / groups) % a.nfld);
    const long f = blockIdx.x / ((long)groups * a.nfld);
    const int kx0 = g * per, lines = min(per, Wh - kx0), Hh = H / 2 + 1;
    const cplx* tw = (const cplx*)(a.ws + a.lay.tw_h);
    for (int i = threadIdx.x; i < H; i += NT) L.tw[i] = tw[i];
    const cplx* inter = (const cplx*)(a.ws + a.lay.inter) + (f * 3 + slot) * H * Wh + kx0;
    for (int i = threadIdx.x; i < lines * H; i += NT) {
        const int y = i / lines, l = i - y * lines;
        L.a[l * H + y] = inter[(long)y * Wh + l];
    }
    for (int i = threadIdx.x; i < lines * Hh; i += NT) {
        const int l = i / Hh, fy = i - l * Hh;
        shell[i] = (short)shell_of(fy, kx0 + l, H, W);
    }
    __syncthreads();
    const cplx* X = fft_lines(L.a, L.b, L.tw, a.ph, lines);
    double* part = (double*)(a.ws + a.lay.shells) + ((f * 3 + slot) * groups + g) * K;
    for (int q = threadIdx.x; q < K; q += NT) {
        double acc = 0.0;
        for (int l = 0; l < lines; ++l) {
            const short* sh = shell + l * Hh;
            int lo = 0, hi = Hh;                                           // first fy with shell >= q
            while (lo < hi) { const int m = (lo + hi) >> 1; if (sh[m] < q) lo = m + 1; else hi = m; }
            const cplx* col = X + l * H;
            const int kx = kx0 + l;
            double sum = 0.0;
            for (int fy = lo; fy < Hh && sh[fy] == q; ++fy) {
                const cplx u = col[fy];
                sum += u.x * u.x + u.y * u.y;
                if (fy > 0 && 2 * fy != H) { const cplx w = col[H - fy]; sum += w.x * w.x + w.y * w.y; }
            }
            acc += (kx == 0 || 2 * kx == W) ? sum : 2.0 * sum;              // the mirrored half of the plane: (-fy, -fx) is in the same shell
        }
        part[q] = acc;
    }
}

// one workgroup per frame: chunks and column groups in order, quotients, roots and bands in fp64, one rounding
__global__ void __launch_bounds__(NT) errors_finish_kernel(ErrArgs a) {
    __shared__ double pe[MAX_SIDE];
    int s;
    if (!live(a, s)) return;
    const long f = blockIdx.x, row = out_row(a, f, s);
    const int H = a.H, W = a.W, K = a.lay.K, groups = a.lay.groups;
    if (threadIdx.x == 0) {
        const double* part = (const double*)(a.ws + a.lay.pw) + f * a.lay.chunks * PW_VALS;
        double se = 0.0, sr = 0.0, si = 0.0, mx = 0.0, bad = 0.0, cells = 0.0;
        for (int c = 0; c < a.lay.chunks; ++c) {
            const double* p = part + c * PW_VALS;
            se += p[0]; sr += p[1]; si += p[2]; mx = fmax(mx, p[3]); bad = fmax(bad, p[4]); cells += p[5];
        }
        const double px = (double)H * (double)W, ring = px - (double)max(H - 2, 0) * (double)max(W - 2, 0);
        if (a.rmse) a.rmse[row] = (float)sqrt(se / px);
        if (a.max_error) a.max_error[row] = bad > 0.0 ? __builtin_nanf("") : (float)mx;
        if (a.boundary_rmse) a.boundary_rmse[row] = (float)sqrt(sr / ring);
        if (a.interface_rmse) a.interface_rmse[row] = cells > 0.0 ? (float)sqrt(si / cells) : __builtin_nanf("");
        if (a.interface_cells) a.interface_cells[row] = (int)cells;
    }
    const double norm = (double)H * (double)W * (double)H * (double)W;
    for (int slot = 0; slot < a.nfld; ++slot) {
        const int fld = a.fld[slot];
        const double* part = (const double*)(a.ws + a.lay.shells) + (f * 3 + slot) * groups * K;
        for (int q = threadIdx.x; q < K; q += NT) {
            double acc = 0.0;
            for (int g = 0; g < groups; ++g) acc += part[(long)g * K + q];
            acc /= norm;
            if (fld == 0) pe[q] = acc;
            if (a.spec[fld]) a.spec[fld][row * K + q] = (float)acc;
        }
    }
    __syncthreads();
    if (a.bands && a.nfld > 0 && a.fld[0] == 0 && threadIdx.x < 3) {
        const int lo = min(a.lo, K), hi = min(a.hi, K);
        const int q0 = threadIdx.x == 0 ? 0 : threadIdx.x == 1 ? lo : hi, q1 = threadIdx.x == 0 ? lo : threadIdx.x == 1 ? hi : K;
        double acc = 0.0;
        for (int q = q0; q < q1; ++q) acc += pe[q];
        a.bands[row * 3 + threadIdx.x] = (float)sqrt(acc);
    }
}

void set_rows(ErrArgs& a, const bf_error_rows& r) {                         // the nine optional outputs under the kernels' names
    a.rmse = r.rmse; a.max_error = r.max_error; a.boundary_rmse = r.boundary_rmse; a.interface_rmse = r.interface_rmse; a.interface_cells = r.interface_cells;
    a.bands = r.spectral_error; a.spec[0] = r.spectrum_error; a.spec[1] = r.spectrum_pred; a.spec[2] = r.spectrum_target;
}

int launch_errors(ErrArgs& a, long F, long mframes, bool have_sdf, int want_spectra, void* ws, int64_t ws_bytes, hipStream_t st) {
    const int H = a.H, W = a.W;
    BF_REQUIRE(H <= MAX_SIDE && W <= MAX_SIDE, "field errors: a side may be at most 1024");
    BF_REQUIRE(a.radius >= 1 && a.lo >= 0 && a.lo <= a.hi, "field errors: interface_radius >= 1 and bands 0 <= lo <= hi");
    BF_REQUIRE(have_sdf || (!a.interface_rmse && !a.interface_cells), "field errors: the interface rows need the signed-distance field");
    BF_REQUIRE(ws && (uintptr_t)ws % 16 == 0, "field errors: the workspace must be 16-byte aligned");
    a.lay = WsLayout(F, H, W);
    BF_REQUIRE(ws_bytes >= a.lay.total, "field errors: workspace smaller than bf_field_errors_ws_bytes");
    BF_REQUIRE(F * 3 * std::max((H + lines_for(W) - 1) / lines_for(W), a.lay.groups) <= 0x7fffffffL && F * a.lay.chunks <= 0x7fffffffL &&
               (mframes * H * W + NT - 1) / NT <= 0x7fffffffL, "field errors: too many frames for one call");
    a.F = F; a.ws = (char*)ws; a.rows_w = lines_for(W); a.rows_h = lines_for(H); a.pw = make_plan(W); a.ph = make_plan(H);
    a.nfld = 0;
    if (want_spectra) {
        if (a.spec[0] || a.bands) a.fld[a.nfld++] = 0;
        if (a.spec[1]) a.fld[a.nfld++] = 1;
        if (a.spec[2]) a.fld[a.nfld++] = 2;
    } else {
        a.bands = nullptr; a.spec[0] = a.spec[1] = a.spec[2] = nullptr;
    }
    if (a.interface_rmse || a.interface_cells) {
        hipLaunchKernelGGL(interface_mask_kernel, dim3((unsigned)((mframes * H * W + NT - 1) / NT)), dim3(NT), 0, st, a, mframes);
        BF_CHECK_LAUNCH();
    }
    if (a.rmse || a.max_error || a.boundary_rmse || a.interface_rmse || a.interface_cells) {
        hipLaunchKernelGGL(pointwise_kernel, dim3((unsigned)(F * a.lay.chunks)), dim3(NT), 0, st, a);
        BF_CHECK_LAUNCH();
    }
    if (a.nfld > 0) {
        hipLaunchKernelGGL(twiddle_kernel, dim3((unsigned)((W + H + NT - 1) / NT)), dim3(NT), 0, st, (cplx*)(a.ws + a.lay.tw_w), W,
                           (cplx*)(a.ws + a.lay.tw_h), H);
        BF_CHECK_LAUNCH();
        hipLaunchKernelGGL(spectra_rows_kernel, dim3((unsigned)(F * a.nfld * ((H + a.rows_w - 1) / a.rows_w))), dim3(NT), 0, st, a);
        BF_CHECK_LAUNCH();
        hipLaunchKernelGGL(spectra_cols_kernel, dim3((unsigned)(F * a.nfld * a.lay.groups)), dim3(NT), 0, st, a);
        BF_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(errors_finish_kernel, dim3((unsigned)F), dim3(NT), 0, st, a);
    BF_CHECK_LAUNCH();
    return 0;
}
}  // namespace

extern "C" int64_t bf_field_errors_ws_bytes(int64_t frames, int H, int W) {
    if (frames <= 0 || H <= 0 || W <= 0 || H > MAX_SIDE || W > MAX_SIDE || frames > (1L << 40) / ((int64_t)H * W)) return 0;
    return WsLayout(frames, H, W).total;
}

extern "C" int bf_field_errors(const float* pred, const float* target, const float* sdf, int64_t frames, int H, int W, int interface_radius, int lo,
                               int hi, int want_spectra, const bf_error_rows* rows, void* ws, int64_t ws_bytes, bf_stream_t stream) {
    BF_REQUIRE(pred && target && rows, "bf_field_errors: null pointer");
    BF_REQUIRE(frames > 0 && H > 0 && W > 0 && bf_field_errors_ws_bytes(frames, H, W) > 0, "bf_field_errors: bad sizes");
    ErrArgs a{};
    a.rollout = 0; a.pred = pred; a.tgt = target; a.sdf = sdf; a.H = H; a.W = W; a.radius = interface_radius; a.lo = lo; a.hi = hi;
    set_rows(a, *rows);
    return launch_errors(a, frames, frames, sdf != nullptr, want_spectra, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int bf_rollout_errors(const bf_rollout_step* s, int sdf_channel, int interface_radius, int lo, int hi, int want_spectra,
                                 const bf_error_rows* rows, void* ws, int64_t ws_bytes, bf_stream_t stream) {
    ErrArgs a{};
    if (const int rc = rollout_step_view(a.v, s, rows != nullptr, s && bf_field_errors_ws_bytes((int64_t)s->B * s->T * s->C, s->Ho, s->Wo) > 0,
                                         "bf_rollout_errors: null pointer", "bf_rollout_errors: bad sizes"))
        return rc;
    const RolloutStep& v = a.v;
    BF_REQUIRE(sdf_channel >= -1 && sdf_channel < v.C, "bf_rollout_errors: the signed-distance channel is -1 (none) or an output channel");
    a.rollout = 1; a.sdf_c = sdf_channel; a.H = v.Ho; a.W = v.Wo; a.radius = interface_radius; a.lo = lo; a.hi = hi;
    set_rows(a, *rows);
    return launch_errors(a, (long)v.B * v.T * v.C, (long)v.B * v.T, sdf_channel >= 0, want_spectra, ws, ws_bytes, (hipStream_t)stream);
}
