// The reference's utils/losses.py as stand-alone kernels: the relative Lp norm per row of LpLoss (utils/losses.py:67-94) forward and
// backward, the adjoint of the Eikonal residual (utils/losses.py:5-15; its value is bf_eikonal_sum in physics.hip), and the interface-weighted
// criterion (no reference program; its own comment further down).
//
// Lp rows.  pred, y are [rows][n] fp32.  Forward: S_e = sum |pred - y|^p and S_y = sum |y|^p per row in fp64, ratio = (S_e / S_y)^(1/p)
// rounded once.  Backward: dpred = coef * sign(e) |e|^(p-1) with coef = g / (S_e^((p-1)/p) * S_y^(1/p)) in fp64.  Two regimes:
//   * long rows (n > LP_SHORT_MAX): a row is cut into `chunks` spans of whole 16-byte groups, one workgroup each; the fp64 partials of the
//     spans go to the workspace and one thread per row adds them in span order (no atomics: the same bits on every call);
//   * short rows: a row is taken by 8, 16, 32 or 64 lanes of one wave, reduced by a shuffle butterfly.
// A span is read as: the <= 3 floats in front of the first 16-byte boundary of the prediction row, 16-byte loads, the <= 3 floats behind the
// last whole group.  The 16-byte form needs pred, y (and dpred) to sit at the same offset from a 16-byte boundary; where they do not the
// same loop reads four scalars instead.
// p = 1 and p = 2 take no transcendental per element and integer p <= LP_INT_MAX multiplies, all in fp64 (the difference of two fp32 numbers
// is exact there); every other p takes powf on the fp32 difference (about 2 ulp per element; VALU-bound, accepted for the generic case).
#include "bf_common.h"
#include <algorithm>
#include <string>

namespace {
constexpr int NT = 256;
constexpr long LP_SHORT_MAX = 2048;       // rows up to this length are taken by part of a wave
constexpr long LP_SPAN_MIN = 8192;        // a long row is not cut into spans shorter than this
constexpr int LP_TARGET_WGS = 2048;       // 256 CUs x 8 workgroups of 256 threads
constexpr int LP_INT_MAX = 16;
enum { LP_P1 = 0, LP_P2 = 1, LP_PINT = 2, LP_PGEN = 3 };

struct LpPow {
    int ip;        // integer p (LP_PINT)
    float pf;      // p, p - 1 (LP_PGEN)
    float pm1f;
};

__device__ __forceinline__ double ipow_d(double a, int k) {      // a^k, k >= 0, by multiplication in a fixed order
    double r = 1.0;
    for (int i = 0; i < k; ++i) r *= a;
    return r;
}
// |v|^p of one element (forward)
template <int MODE> __device__ __forceinline__ double lp_term(float v, const LpPow& pw) {
    if constexpr (MODE == LP_P1) return fabs((double)v);
    else if constexpr (MODE == LP_P2) return (double)v * (double)v;
    else if constexpr (MODE == LP_PINT) return ipow_d(fabs((double)v), pw.ip);
    else return (double)powf(fabsf(v), pw.pf);
}
template <int MODE> __device__ __forceinline__ double lp_err_term(float a, float b, const LpPow& pw) {
    if constexpr (MODE == LP_PGEN) return (double)powf(fabsf(a - b), pw.pf);
    else {
        const double e = (double)a - (double)b;
        if constexpr (MODE == LP_P1) return fabs(e);
        else if constexpr (MODE == LP_P2) return e * e;
        else return ipow_d(fabs(e), pw.ip);
    }
}
// coef * sign(e) |e|^(p-1) of one element (backward), rounded once
template <int MODE> __device__ __forceinline__ float lp_grad_term(float a, float b, double coef, const LpPow& pw) {
    if constexpr (MODE == LP_PGEN) {
        const float e = a - b;
        const double m = e == 0.f ? 0.0 : (double)powf(fabsf(e), pw.pm1f);
        return (float)(coef * copysign(m, (double)e));
    } else {
        const double e = (double)a - (double)b;
        if constexpr (MODE == LP_P1) return (float)(e > 0.0 ? coef : e < 0.0 ? -coef : 0.0 * coef);
        else if constexpr (MODE == LP_P2) return (float)(coef * e);
        else return (float)(coef * copysign(ipow_d(fabs(e), pw.ip - 1), e));
    }
}

// floats in front of the first 16-byte boundary at or after p, at most n
__device__ __forceinline__ long lp_head(const float* p, long n) { return min(n, (long)(((16 - ((uintptr_t)p & 15)) & 15) >> 2)); }

// Sums of one span [lo, hi) of the body of a row (body = the row without its head; lo is a multiple of 4) over `width` lanes, this lane = `lane`.
template <int MODE> __device__ __forceinline__ void lp_span_sums(const float* __restrict__ pb, const float* __restrict__ yb, long lo, long hi, int lane,
                                                                 int width, bool vec, const LpPow& pw, double& se, double& sy) {
    long i = lo + 4L * lane;
    if (vec) {
        for (; i + 3 < hi; i += 4L * width) {
            const float4 a = *reinterpret_cast<const float4*>(pb + i), b = *reinterpret_cast<const float4*>(yb + i);
            se += lp_err_term<MODE>(a.x, b.x, pw); sy += lp_term<MODE>(b.x, pw);
            se += lp_err_term<MODE>(a.y, b.y, pw); sy += lp_term<MODE>(b.y, pw);
            se += lp_err_term<MODE>(a.z, b.z, pw); sy += lp_term<MODE>(b.z, pw);
            se += lp_err_term<MODE>(a.w, b.w, pw); sy += lp_term<MODE>(b.w, pw);
        }
    } else {
        for (; i + 3 < hi; i += 4L * width)
            for (int j = 0; j < 4; ++j) { se += lp_err_term<MODE>(pb[i + j], yb[i + j], pw); sy += lp_term<MODE>(yb[i + j], pw); }
    }
    for (long j = i; j < hi && j < i + 4; ++j) { se += lp_err_term<MODE>(pb[j], yb[j], pw); sy += lp_term<MODE>(yb[j], pw); }      // the span's ragged end (one lane)
}
template <int MODE> __device__ __forceinline__ void lp_span_grad(const float* __restrict__ pb, const float* __restrict__ yb, float* __restrict__ db, long lo,
                                                                 long hi, int lane, int width, bool vec, double coef, const LpPow& pw) {
    long i = lo + 4L * lane;
    if (vec) {
        for (; i + 3 < hi; i += 4L * width) {
            const float4 a = *reinterpret_cast<const float4*>(pb + i), b = *reinterpret_cast<const float4*>(yb + i);
            float4 o;
            o.x = lp_grad_term<MODE>(a.x, b.x, coef, pw); o.y = lp_grad_term<MODE>(a.y, b.y, coef, pw);
            o.z = lp_grad_term<MODE>(a.z, b.z, coef, pw); o.w = lp_grad_term<MODE>(a.w, b.w, coef, pw);
            *reinterpret_cast<float4*>(db + i) = o;
        }
    } else {
        for (; i + 3 < hi; i += 4L * width)
            for (int j = 0; j < 4; ++j) db[i + j] = lp_grad_term<MODE>(pb[i + j], yb[i + j], coef, pw);
    }
    for (long j = i; j < hi && j < i + 4; ++j) db[j] = lp_grad_term<MODE>(pb[j], yb[j], coef, pw);
}

// the root and the row coefficient are specialised with the element code: p = 1 and p = 2 carry no pow(), whose registers would otherwise
// cost the streaming kernels a quarter of their waves
template <int MODE> __device__ __forceinline__ double lp_root(double q, double p) {
    if constexpr (MODE == LP_P1) return q;
    else if constexpr (MODE == LP_P2) return sqrt(q);
    else return pow(q, 1.0 / p);
}
// g / (S_e^((p-1)/p) * S_y^(1/p)); a row without error gets 0 (torch's norm backward: the subgradient 0 at e = 0)
template <int MODE> __device__ __forceinline__ double lp_coef(double g, double se, double sy, double p) {
    if (se == 0.0) return 0.0;
    if constexpr (MODE == LP_P1) return g / sy;
    else if constexpr (MODE == LP_P2) return g / sqrt(se * sy);
    else return g / (pow(se, (p - 1.0) / p) * pow(sy, 1.0 / p));
}
__device__ __forceinline__ long lp_span_len(long n, int chunks) { return ((n + chunks - 1) / chunks + 3) & ~3L; }

// ---- long rows: workgroup (row, span).  Span 0 also takes the row's head.
template <int MODE>
__global__ void __launch_bounds__(NT) lp_long_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ y, long n, int chunks, LpPow pw,
                                                        double* __restrict__ part) {
    __shared__ double red[NT / 64][2];      // several values at once in this kernel's own order, which its restatement's bits pin: not bf_common.h's block_reduce
    const long row = blockIdx.x / chunks;
    const int c = (int)(blockIdx.x % chunks);
    const float* p = pred + row * n;
    const float* q = y + row * n;
    const bool vec = (((uintptr_t)p ^ (uintptr_t)q) & 15) == 0;
    const long h = lp_head(p, n), body = n - h, per = lp_span_len(body, chunks);
    const long lo = min(body, c * per), hi = min(body, lo + per);
    double se = 0.0, sy = 0.0;
    if (c == 0 && (long)threadIdx.x < h) { se += lp_err_term<MODE>(p[threadIdx.x], q[threadIdx.x], pw); sy += lp_term<MODE>(q[threadIdx.x], pw); }
    lp_span_sums<MODE>(p + h, q + h, lo, hi, threadIdx.x, NT, vec, pw, se, sy);
    se = wave_sum(se); sy = wave_sum(sy);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = se; red[threadIdx.x >> 6][1] = sy; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int w = 0; w < NT / 64; ++w) { a += red[w][0]; b += red[w][1]; }
        part[2L * blockIdx.x] = a; part[2L * blockIdx.x + 1] = b;
    }
}
template <int MODE>
__global__ void __launch_bounds__(64) lp_finish_kernel(const double* __restrict__ part, long rows, int chunks, double p, float* __restrict__ ratio,
                                                      double* __restrict__ sums) {
    const long row = (long)blockIdx.x * 64 + threadIdx.x;
    if (row >= rows) return;
    double a = 0.0, b = 0.0;
    for (int c = 0; c < chunks; ++c) { a += part[2 * (row * chunks + c)]; b += part[2 * (row * chunks + c) + 1]; }
    sums[2 * row] = a; sums[2 * row + 1] = b;
    ratio[row] = (float)lp_root<MODE>(a / b, p);
}
template <int MODE>
__global__ void __launch_bounds__(NT, 8) lp_long_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ y, const float* __restrict__ g,
                                                        const double* __restrict__ sums, long n, int chunks, double p, LpPow pw, float* __restrict__ dpred) {
    const long row = blockIdx.x / chunks;
    const int c = (int)(blockIdx.x % chunks);
    const float* a = pred + row * n;
    const float* b = y + row * n;
    float* d = dpred + row * n;
    const bool vec = ((((uintptr_t)a ^ (uintptr_t)b) | ((uintptr_t)a ^ (uintptr_t)d)) & 15) == 0;
    const long h = lp_head(a, n), body = n - h, per = lp_span_len(body, chunks);
    const long lo = min(body, c * per), hi = min(body, lo + per);
    const double coef = lp_coef<MODE>((double)g[row], sums[2 * row], sums[2 * row + 1], p);      // wave-uniform: every lane computes the same bits
    if (c == 0 && (long)threadIdx.x < h) d[threadIdx.x] = lp_grad_term<MODE>(a[threadIdx.x], b[threadIdx.x], coef, pw);
    lp_span_grad<MODE>(a + h, b + h, d + h, lo, hi, threadIdx.x, NT, vec, coef, pw);
}

// ---- short rows: `width` (8 .. 64, a power of two) lanes per row, 256 / width rows per workgroup
template <int MODE>
__global__ void __launch_bounds__(NT) lp_short_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ y, long rows, long n, int width, double p,
                                                         LpPow pw, float* __restrict__ ratio, double* __restrict__ sums) {
    const int lane = threadIdx.x & (width - 1);
    const long row = ((long)blockIdx.x * NT + threadIdx.x) / width;
    double se = 0.0, sy = 0.0;
    if (row < rows) {                                 // no early return: the shuffles below need every lane of the wave
        const float* a = pred + row * n;
        const float* b = y + row * n;
        const bool vec = (((uintptr_t)a ^ (uintptr_t)b) & 15) == 0;
        const long h = lp_head(a, n);
        if (lane < h) { se += lp_err_term<MODE>(a[lane], b[lane], pw); sy += lp_term<MODE>(b[lane], pw); }
        lp_span_sums<MODE>(a + h, b + h, 0, n - h, lane, width, vec, pw, se, sy);
    }
    for (int o = width >> 1; o > 0; o >>= 1) { se += __shfl_xor(se, o, 64); sy += __shfl_xor(sy, o, 64); }
    if (row < rows && lane == 0) {
        sums[2 * row] = se; sums[2 * row + 1] = sy;
        ratio[row] = (float)lp_root<MODE>(se / sy, p);
    }
}
template <int MODE>
__global__ void __launch_bounds__(NT) lp_short_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ y, const float* __restrict__ g,
                                                         const double* __restrict__ sums, long rows, long n, int width, double p, LpPow pw,
                                                         float* __restrict__ dpred) {
    const int lane = threadIdx.x & (width - 1);
    const long row = ((long)blockIdx.x * NT + threadIdx.x) / width;
    double coef = 0.0;
    if (row < rows && lane == 0) coef = lp_coef<MODE>((double)g[row], sums[2 * row], sums[2 * row + 1], p);      // one lane per row pays for the roots
    coef = __shfl(coef, (threadIdx.x & 63) & ~(width - 1), 64);
    if (row >= rows) return;
    const float* a = pred + row * n;
    const float* b = y + row * n;
    float* d = dpred + row * n;
    const bool vec = ((((uintptr_t)a ^ (uintptr_t)b) | ((uintptr_t)a ^ (uintptr_t)d)) & 15) == 0;
    const long h = lp_head(a, n);
    if (lane < h) d[lane] = lp_grad_term<MODE>(a[lane], b[lane], coef, pw);
    lp_span_grad<MODE>(a + h, b + h, d + h, 0, n - h, lane, width, vec, coef, pw);
}

int lp_mode(double p, LpPow* pw) {
    pw->ip = 0; pw->pf = (float)p; pw->pm1f = (float)(p - 1.0);
    if (p == 1.0) return LP_P1;
    if (p == 2.0) return LP_P2;
    if (p == floor(p) && p <= (double)LP_INT_MAX) { pw->ip = (int)p; return LP_PINT; }
    return LP_PGEN;
}
// spans per long row: enough workgroups to fill the chip, none shorter than LP_SPAN_MIN
int lp_chunks(int64_t rows, int64_t n) {
    if (n <= LP_SHORT_MAX) return 0;
    const int64_t want = (LP_TARGET_WGS + rows - 1) / rows, most = n / LP_SPAN_MIN;
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min(want, most), 1024));
}
int lp_width(int64_t n) {      // about four 16-byte groups per lane
    int w = 8;
    while (w < 64 && (int64_t)w * 16 < n) w *= 2;
    return w;
}
bool lp_sizes_ok(int64_t rows, int64_t n) {
    return rows > 0 && n > 0 && rows <= (int64_t)1 << 40 && n <= (int64_t)1 << 40 && rows * n <= (int64_t)1 << 40;
}

// d/dphi of g * mean((|grad phi| - 1)^2), torch.gradient(spacing = dx, edge_order = 1) along H and W, in gather form: the cell (y, x) sums the
// contributions of the cells whose stencil reads it (itself at a border, its <= 4 neighbours), so nothing is accumulated across workgroups.
// With q_y(c) = w(c) * g_y(c), q_x(c) = w(c) * g_x(c), w = 2 g (m - 1) / (N m), m = |grad phi|(c), w = 0 where m = 0 (autograd gives 0 * inf there):
//   dphi[y][x] = sum_j k_y(j, y) q_y(j, x) + sum_i k_x(i, x) q_x(y, i), k = the stencil weight of phi[y] in g_y(j).  All in fp64, rounded once.
struct EikCell { double qy, qx; };
// torch.gradient(spacing = 1 / inv_dx, edge_order = 1) of the frame f at (y, x): {d/dy, d/dx}
__device__ __forceinline__ EikCell eik_grad(const float* __restrict__ f, int y, int x, int H, int W, double inv_dx) {
    const float* p = f + (long)y * W + x;
    double gy, gx;
    if (H == 1) gy = 0.0;
    else if (y == 0) gy = ((double)p[W] - (double)p[0]) * inv_dx;
    else if (y == H - 1) gy = ((double)p[0] - (double)p[-W]) * inv_dx;
    else gy = ((double)p[W] - (double)p[-W]) * (0.5 * inv_dx);
    if (W == 1) gx = 0.0;
    else if (x == 0) gx = ((double)p[1] - (double)p[0]) * inv_dx;
    else if (x == W - 1) gx = ((double)p[0] - (double)p[-1]) * inv_dx;
    else gx = ((double)p[1] - (double)p[-1]) * (0.5 * inv_dx);
    return {gy, gx};
}
__device__ __forceinline__ EikCell eik_cell(const float* __restrict__ f, int y, int x, int H, int W, double inv_dx, double scale) {
    const EikCell d = eik_grad(f, y, x, H, W, inv_dx);
    const double gy = d.qy, gx = d.qx;
    const double s = gy * gy + gx * gx;
    const double w = s > 0.0 ? scale * (1.0 - rsqrt(s)) : 0.0;
    return {w * gy, w * gx};
}
// weight of phi[i] in the derivative at cell j of an axis of n >= 2 points, times dx
__device__ __forceinline__ double eik_weight(int j, int i, int n) {
    if (j == 0) return i == 0 ? -1.0 : i == 1 ? 1.0 : 0.0;
    if (j == n - 1) return i == n - 1 ? 1.0 : i == n - 2 ? -1.0 : 0.0;
    return i == j + 1 ? 0.5 : i == j - 1 ? -0.5 : 0.0;
}
// One workgroup per EIK_TH x EIK_TW tile of one frame: q_y, q_x of the tile and a one-cell rim go to LDS once (1.16 roots per cell instead of 5), then
// every cell of the tile gathers from LDS.  The tile at (y0, x0) of the frame f: its adjoint is stored to the frame d, or added to it (ADD).
// The one text of eikonal_loss's backward and of the interface criterion's penalty: the same stencil, the same order of terms.
constexpr int EIK_TH = 16, EIK_TW = 64;
template <bool ADD>
__device__ __forceinline__ void eik_bwd_tile(const float* __restrict__ f, float* __restrict__ d, int H, int W, int y0, int x0, double inv_dx, double scale) {
    __shared__ double qy[EIK_TH + 2][EIK_TW + 2], qx[EIK_TH + 2][EIK_TW + 2];
    for (int i = threadIdx.x; i < (EIK_TH + 2) * (EIK_TW + 2); i += NT) {
        const int ly = i / (EIK_TW + 2), lx = i % (EIK_TW + 2), y = y0 - 1 + ly, x = x0 - 1 + lx;
        EikCell c = {0.0, 0.0};
        if (y >= 0 && y < H && x >= 0 && x < W) c = eik_cell(f, y, x, H, W, inv_dx, scale);
        qy[ly][lx] = c.qy; qx[ly][lx] = c.qx;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < EIK_TH * EIK_TW; i += NT) {
        const int ly = i / EIK_TW, lx = i % EIK_TW, y = y0 + ly, x = x0 + lx;
        if (y >= H || x >= W) continue;
        double acc = 0.0;
        if (H > 1) {
            for (int j = max(y - 1, 0); j <= min(y + 1, H - 1); ++j) {
                const double k = eik_weight(j, y, H);
                if (k != 0.0) acc += k * qy[j - y0 + 1][lx + 1];
            }
        }
        if (W > 1) {
            for (int j = max(x - 1, 0); j <= min(x + 1, W - 1); ++j) {
                const double k = eik_weight(j, x, W);
                if (k != 0.0) acc += k * qx[ly + 1][j - x0 + 1];
            }
        }
        float* o = d + (long)y * W + x;
        if constexpr (ADD) *o += (float)(acc * inv_dx);
        else *o = (float)(acc * inv_dx);
    }
}
__global__ void __launch_bounds__(NT) eikonal_bwd_kernel(const float* __restrict__ phi, long frames, int H, int W, int tiles_y, int tiles_x, double inv_dx,
                                                        const float* __restrict__ g, float* __restrict__ dphi) {
    const long tile = blockIdx.x;
    const int x0 = (int)(tile % tiles_x) * EIK_TW, y0 = (int)((tile / tiles_x) % tiles_y) * EIK_TH;
    const long frame = tile / ((long)tiles_x * tiles_y);
    const double scale = 2.0 * (double)g[0] / (double)(frames * H * W);
    eik_bwd_tile<false>(phi + frame * ((long)H * W), dphi + frame * ((long)H * W), H, W, y0, x0, inv_dx, scale);
}

// ---- The interface-weighted criterion.  pred, y are [frames][C][hw] fp32 (frames = B * T, hw = H * W), s the channel of the signed distance:
//   w[f][i]  = 1 + gain * max(0, 1 - |y[f][s][i] * div + diff| / band)      fp64, from the target alone, shared by the C fields of a frame
//   S_e[f][c] = sum_i w (pred - y)^2,  S_y[f][c] = sum_i w y^2,  rho = sqrt(S_e / S_y),  term[c] = a_c * mean_f rho[f][c]
//   eik = lambda * mean_{f,i} (|grad (pred[f][s] * div + diff)| - 1)^2,  loss = sum_c term[c] + eik.
// A group of `width` lanes owns one span of pixels of one frame across all C channels, so a pixel's weight is formed once: 256 lanes (one
// workgroup) and `chunks` spans per frame where hw > LP_SHORT_MAX, 8 .. 64 lanes of a wave and one span otherwise.  The fp64 partials go to the
// workspace and one workgroup adds them in span order, forms the ratios and their means over the frames in a fixed order (no atomics).  The
// 16-byte form needs hw to be a multiple of 4 (every channel of a frame then sits at the frame's offset from a 16-byte boundary) and pred, y
// (and dpred) at one offset; anything else reads scalars.  CT >= C is the compile-time count of per-channel accumulators.
// The affine map of the penalty never materialises: grad(pred * div + diff) = div * grad(pred), so the stencil runs on the stored channel at
// the spacing dx / div, and the chain factor div of the backward is the same factor again.
constexpr int WLP_MAX_C = 16;
constexpr int WLP_EIK_MAX_WGS = 2048;
struct WlpHat { double diff, div, inv_band, gain; };
struct WlpFields { double a[WLP_MAX_C]; };

__device__ __forceinline__ double wlp_weight(float ys, const WlpHat& hat) {
    return 1.0 + hat.gain * fmax(0.0, 1.0 - fabs((double)ys * hat.div + hat.diff) * hat.inv_band);
}
template <int CT> __device__ __forceinline__ void wlp_px_sums(const float* __restrict__ pf, const float* __restrict__ yf, long hw, int C, int s, long i,
                                                              const WlpHat& hat, double (&se)[CT], double (&sy)[CT]) {
    const double w = wlp_weight(yf[s * hw + i], hat);
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        if (c < C) {
            const double b = (double)yf[c * hw + i], e = (double)pf[c * hw + i] - b;
            se[c] += w * (e * e); sy[c] += w * (b * b);
        }
    }
}
template <int CT> __device__ __forceinline__ void wlp_px_grad(const float* __restrict__ pf, const float* __restrict__ yf, float* __restrict__ df, long hw, int C,
                                                              int s, long i, const WlpHat& hat, const double (&coef)[CT]) {
    const double w = wlp_weight(yf[s * hw + i], hat);
#pragma unroll
    for (int c = 0; c < CT; ++c)
        if (c < C) df[c * hw + i] = (float)(coef[c] * (w * ((double)pf[c * hw + i] - (double)yf[c * hw + i])));
}
// One span [lo, hi) of a frame's pixels behind its head (pf, yf, df point at the first pixel behind the head of channel 0; lo a multiple of 4).
template <int CT> __device__ __forceinline__ void wlp_span_sums(const float* __restrict__ pf, const float* __restrict__ yf, long hw, int C, int s, long lo, long hi,
                                                                int lane, int width, bool vec, const WlpHat& hat, double (&se)[CT], double (&sy)[CT]) {
    long i = lo + 4L * lane;
    if (vec) {
        for (; i + 3 < hi; i += 4L * width) {
            const float4 t = *reinterpret_cast<const float4*>(yf + s * hw + i);
            const double w0 = wlp_weight(t.x, hat), w1 = wlp_weight(t.y, hat), w2 = wlp_weight(t.z, hat), w3 = wlp_weight(t.w, hat);
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                if (c < C) {
                    const float4 a = *reinterpret_cast<const float4*>(pf + c * hw + i), b = *reinterpret_cast<const float4*>(yf + c * hw + i);
                    const double e0 = (double)a.x - (double)b.x, e1 = (double)a.y - (double)b.y, e2 = (double)a.z - (double)b.z, e3 = (double)a.w - (double)b.w;
                    se[c] += w0 * (e0 * e0); sy[c] += w0 * ((double)b.x * (double)b.x);
                    se[c] += w1 * (e1 * e1); sy[c] += w1 * ((double)b.y * (double)b.y);
                    se[c] += w2 * (e2 * e2); sy[c] += w2 * ((double)b.z * (double)b.z);
                    se[c] += w3 * (e3 * e3); sy[c] += w3 * ((double)b.w * (double)b.w);
                }
            }
        }
    } else {
        for (; i + 3 < hi; i += 4L * width)
            for (int j = 0; j < 4; ++j) wlp_px_sums<CT>(pf, yf, hw, C, s, i + j, hat, se, sy);
    }
    for (long j = i; j < hi && j < i + 4; ++j) wlp_px_sums<CT>(pf, yf, hw, C, s, j, hat, se, sy);      // the span's ragged end (one lane)
}
template <int CT> __device__ __forceinline__ void wlp_span_grad(const float* __restrict__ pf, const float* __restrict__ yf, float* __restrict__ df, long hw, int C,
                                                                int s, long lo, long hi, int lane, int width, bool vec, const WlpHat& hat,
                                                                const double (&coef)[CT]) {
    long i = lo + 4L * lane;
    if (vec) {
        for (; i + 3 < hi; i += 4L * width) {
            const float4 t = *reinterpret_cast<const float4*>(yf + s * hw + i);
            const double w0 = wlp_weight(t.x, hat), w1 = wlp_weight(t.y, hat), w2 = wlp_weight(t.z, hat), w3 = wlp_weight(t.w, hat);
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                if (c < C) {
                    const float4 a = *reinterpret_cast<const float4*>(pf + c * hw + i), b = *reinterpret_cast<const float4*>(yf + c * hw + i);
                    float4 o;
                    o.x = (float)(coef[c] * (w0 * ((double)a.x - (double)b.x))); o.y = (float)(coef[c] * (w1 * ((double)a.y - (double)b.y)));
                    o.z = (float)(coef[c] * (w2 * ((double)a.z - (double)b.z))); o.w = (float)(coef[c] * (w3 * ((double)a.w - (double)b.w)));
                    *reinterpret_cast<float4*>(df + c * hw + i) = o;
                }
            }
        }
    } else {
        for (; i + 3 < hi; i += 4L * width)
            for (int j = 0; j < 4; ++j) wlp_px_grad<CT>(pf, yf, df, hw, C, s, i + j, hat, coef);
    }
    for (long j = i; j < hi && j < i + 4; ++j) wlp_px_grad<CT>(pf, yf, df, hw, C, s, j, hat, coef);
}
// the frame, span and lane of this thread; false for the threads behind the last group
struct WlpGroup { long frame; int span, lane; bool live; };
__device__ __forceinline__ WlpGroup wlp_group(long frames, int chunks, int width) {
    const long grp = ((long)blockIdx.x * NT + threadIdx.x) / width;
    return {grp / chunks, (int)(grp % chunks), (int)(threadIdx.x & (width - 1)), grp < frames * chunks};
}
// part[((frame * C + c) * chunks + span) * 2] = {S_e, S_y} of the span
template <int CT>
__global__ void __launch_bounds__(NT) wlp_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ y, long frames, long hw, int C, int s, int chunks,
                                                    int width, WlpHat hat, double* __restrict__ part) {
    __shared__ double red[NT / 64][2 * CT];      // several values at once in this kernel's own order, which its restatement's bits pin: not bf_common.h's block_reduce
    const WlpGroup g = wlp_group(frames, chunks, width);
    double se[CT], sy[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) se[c] = sy[c] = 0.0;
    if (g.live) {                                     // no early return: the shuffles below need every lane of the wave
        const float* pf = pred + g.frame * C * hw;
        const float* yf = y + g.frame * C * hw;
        const bool vec = (hw & 3) == 0 && (((uintptr_t)pf ^ (uintptr_t)yf) & 15) == 0;
        const long h = vec ? lp_head(pf, hw) : 0, body = hw - h, per = lp_span_len(body, chunks);
        const long lo = min(body, g.span * per), hi = min(body, lo + per);
        if (g.span == 0 && g.lane < h) wlp_px_sums<CT>(pf, yf, hw, C, s, g.lane, hat, se, sy);
        wlp_span_sums<CT>(pf + h, yf + h, hw, C, s, lo, hi, g.lane, width, vec, hat, se, sy);
    }
    const int within = width < 64 ? width : 64;
#pragma unroll
    for (int c = 0; c < CT; ++c)
        for (int o = within >> 1; o > 0; o >>= 1) { se[c] += __shfl_xor(se[c], o, 64); sy[c] += __shfl_xor(sy[c], o, 64); }
    if (width == NT) {                                // one group per workgroup: the waves in order
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int c = 0; c < CT; ++c) { red[threadIdx.x >> 6][2 * c] = se[c]; red[threadIdx.x >> 6][2 * c + 1] = sy[c]; }
        }
        __syncthreads();
        if (threadIdx.x < 2 * C) {
            double a = 0.0;
            for (int w = 0; w < NT / 64; ++w) a += red[w][threadIdx.x];
            part[((g.frame * C + (threadIdx.x >> 1)) * chunks + g.span) * 2 + (threadIdx.x & 1)] = a;
        }
    } else if (g.live && g.lane == 0) {
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (c < C) { part[((g.frame * C + c) * chunks + g.span) * 2] = se[c]; part[((g.frame * C + c) * chunks + g.span) * 2 + 1] = sy[c]; }
    }
}
// Sum of (|grad phi_p| - 1)^2 over the cells this workgroup strides over, phi_p = the channel at `off` of every frame (frames fstride apart) at the
// spacing 1 / inv_dx (= dx / div); part[blockIdx.x] = the workgroup's sum.
__global__ void __launch_bounds__(NT) wlp_eik_fwd_kernel(const float* __restrict__ pred, long frames, long fstride, long off, int H, int W, double inv_dx,
                                                        double* __restrict__ part) {
    __shared__ double red[NT / 64];
    const long hw = (long)H * W, total = frames * hw;
    double acc = 0.0;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const long frame = i / hw;
        const int r = (int)(i - frame * hw);
        const EikCell d = eik_grad(pred + frame * fstride + off, r / W, r % W, H, W, inv_dx);
        const double m = sqrt(d.qy * d.qy + d.qx * d.qx) - 1.0;
        acc += m * m;
    }
    acc = block_reduce<RED_SUM, NT / 64>(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}
// One workgroup: sums[row] = the spans of row (frame, c) in span order; rho = sqrt(S_e / S_y); terms[1 + c] = a_c * mean over the frames of rho, added in a
// fixed order; terms[0] = eik_scale * (the penalty's partials in order); loss = their sum.  All fp64, each output rounded once.
__global__ void __launch_bounds__(NT) wlp_finish_kernel(const double* __restrict__ part, long frames, int C, int chunks, WlpFields fa,
                                                       const double* __restrict__ eik_part, int eik_n, double eik_scale, double* __restrict__ sums,
                                                       double* __restrict__ rho, float* __restrict__ loss, float* __restrict__ terms) {
    __shared__ double red[NT / 64];
    for (long row = threadIdx.x; row < frames * C; row += NT) {
        double a = 0.0, b = 0.0;
        for (int k = 0; k < chunks; ++k) { a += part[2 * (row * chunks + k)]; b += part[2 * (row * chunks + k) + 1]; }
        sums[2 * row] = a; sums[2 * row + 1] = b;
        rho[row] = sqrt(a / b);
    }
    __syncthreads();
    double total = 0.0;
    for (int c = 0; c < C; ++c) {
        double acc = 0.0;
        for (long f = threadIdx.x; f < frames; f += NT) acc += rho[f * C + c];
        const double term = fa.a[c] * (block_reduce<RED_SUM, NT / 64>(acc, red) / (double)frames);
        if (threadIdx.x == 0) terms[1 + c] = (float)term;
        total += term;
    }
    double acc = 0.0;
    for (int i = threadIdx.x; i < eik_n; i += NT) acc += eik_part[i];
    const double eik = eik_n > 0 ? eik_scale * block_reduce<RED_SUM, NT / 64>(acc, red) : 0.0;
    if (threadIdx.x == 0) { terms[0] = (float)eik; loss[0] = (float)(total + eik); }
}
// dpred = g * a_c / frames * w * (pred - y) / sqrt(S_e S_y): the row coefficient in fp64, every element rounded once; a row with S_e = 0 gets zeros
template <int CT>
__global__ void __launch_bounds__(NT) wlp_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ y, const float* __restrict__ gout,
                                                    const double* __restrict__ sums, long frames, long hw, int C, int s, int chunks, int width, WlpHat hat,
                                                    WlpFields fa, float* __restrict__ dpred) {
    const WlpGroup g = wlp_group(frames, chunks, width);
    if (!g.live) return;
    const float* pf = pred + g.frame * C * hw;
    const float* yf = y + g.frame * C * hw;
    float* df = dpred + g.frame * C * hw;
    const bool vec = (hw & 3) == 0 && ((((uintptr_t)pf ^ (uintptr_t)yf) | ((uintptr_t)pf ^ (uintptr_t)df)) & 15) == 0;
    const long h = vec ? lp_head(pf, hw) : 0, body = hw - h, per = lp_span_len(body, chunks);
    const long lo = min(body, g.span * per), hi = min(body, lo + per);
    const double gs = (double)gout[0] / (double)frames;
    double coef[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        coef[c] = 0.0;
        if (c < C) {
            const double a = sums[2 * (g.frame * C + c)], b = sums[2 * (g.frame * C + c) + 1];
            if (a != 0.0) coef[c] = gs * fa.a[c] / sqrt(a * b);
        }
    }
    if (g.span == 0 && g.lane < h) wlp_px_grad<CT>(pf, yf, df, hw, C, s, g.lane, hat, coef);
    wlp_span_grad<CT>(pf + h, yf + h, df + h, hw, C, s, lo, hi, g.lane, width, vec, hat, coef);
}
// eik_bwd_tile on a channel that lies inside pred: frames fstride apart, the channel at `off`, spacing 1 / inv_dx (= dx / div); the adjoint is ADDED to
// dpred's channel (the data term's launch has written it).  scale = 2 g lambda / (frames H W) is formed from g[0] here.
__global__ void __launch_bounds__(NT) wlp_eik_bwd_kernel(const float* __restrict__ pred, long frames, long fstride, long off, int H, int W, int tiles_y, int tiles_x,
                                                        double inv_dx, double lambda, const float* __restrict__ g, float* __restrict__ dpred) {
    const long tile = blockIdx.x;
    const int x0 = (int)(tile % tiles_x) * EIK_TW, y0 = (int)((tile / tiles_x) % tiles_y) * EIK_TH;
    const long frame = tile / ((long)tiles_x * tiles_y);
    const double scale = 2.0 * (double)g[0] * lambda / (double)(frames * H * W);
    eik_bwd_tile<true>(pred + frame * fstride + off, dpred + frame * fstride + off, H, W, y0, x0, inv_dx, scale);
}

// spans per frame: enough workgroups to fill the chip, every lane of a span with whole 16-byte groups
int wlp_chunks(int64_t frames, int C, int64_t hw) {
    if (hw <= LP_SHORT_MAX) return 1;
    const int64_t want = (LP_TARGET_WGS + frames - 1) / frames, most = hw * C / LP_SPAN_MIN;
    const int64_t c0 = std::max<int64_t>(1, std::min<int64_t>(std::min(want, most), 1024));
    const int64_t per = ((hw + c0 - 1) / c0 + 4 * NT - 1) / (4 * NT) * (4 * NT);
    return (int)((hw + per - 1) / per);
}
int wlp_width(int64_t hw) { return hw <= LP_SHORT_MAX ? lp_width(hw) : NT; }
int wlp_eik_wgs(int64_t frames, int64_t hw) { return (int)std::min<int64_t>((frames * hw + NT - 1) / NT, WLP_EIK_MAX_WGS); }
bool wlp_sizes_ok(int64_t frames, int C, int H, int W) {
    return frames > 0 && frames <= (int64_t)1 << 20 && C > 0 && C <= WLP_MAX_C && H > 0 && W > 0 && H <= 1 << 15 && W <= 1 << 15 &&
           frames * C * H * W <= (int64_t)1 << 40;
}
struct WlpPlan { int chunks, width; int64_t grid, rho, eik; };      // the span partials lie at 0, then the ratios, then the penalty's partials (doubles)
WlpPlan wlp_plan(int64_t frames, int C, int H, int W) {
    const int64_t hw = (int64_t)H * W;
    WlpPlan p;
    p.chunks = wlp_chunks(frames, C, hw); p.width = wlp_width(hw);
    p.grid = (frames * p.chunks * p.width + NT - 1) / NT;
    p.rho = 2 * frames * C * p.chunks; p.eik = p.rho + frames * C;
    return p;
}
// the checks bf_wlp_fwd and bf_wlp_bwd share; NULL = accepted
const char* wlp_refusal(int64_t frames, int C, int H, int W, int s, double diff_s, double div_s, double band, double gain, const double* field_weights,
                        double eikonal, double dx) {
    if (!wlp_sizes_ok(frames, C, H, W)) return "B*T must be 1 .. 2^20, C 1 .. 16, H and W 1 .. 32768";
    if (s < 0 || s >= C) return "the signed-distance channel must lie in [0, C)";
    if (!(gain >= 0.0 && gain < INFINITY)) return "gain must be finite and >= 0";
    if (gain > 0.0 && !(band > 0.0 && band < INFINITY)) return "band must be positive and finite where gain > 0";
    if (!(div_s != 0.0 && fabs(div_s) < INFINITY && fabs(diff_s) < INFINITY)) return "div must be finite and not 0, diff finite";
    for (int c = 0; field_weights && c < C; ++c)
        if (!(field_weights[c] >= 0.0 && field_weights[c] < INFINITY)) return "field weights must be finite and >= 0";
    if (!(eikonal >= 0.0 && eikonal < INFINITY)) return "the eikonal coefficient must be finite and >= 0";
    if (eikonal > 0.0 && !(dx > 0.0 && dx < INFINITY)) return "dx must be positive and finite where the eikonal coefficient > 0";
    return nullptr;
}
WlpHat wlp_hat(double diff_s, double div_s, double band, double gain) { return {diff_s, div_s, gain > 0.0 ? 1.0 / band : 0.0, gain}; }
WlpFields wlp_fields(const double* field_weights, int C) {
    WlpFields fa;
    for (int c = 0; c < WLP_MAX_C; ++c) fa.a[c] = c < C ? (field_weights ? field_weights[c] : 1.0) : 0.0;
    return fa;
}
}  // namespace

extern "C" int64_t bf_lp_rows_ws_doubles(int64_t rows, int64_t n) {
    if (!lp_sizes_ok(rows, n)) return -1;
    return 2 * rows * lp_chunks(rows, n);
}

#define LP_DISPATCH(mode, CALL)                                  \
    switch (mode) {                                              \
        case LP_P1: { constexpr int M = LP_P1; CALL; } break;     \
        case LP_P2: { constexpr int M = LP_P2; CALL; } break;     \
        case LP_PINT: { constexpr int M = LP_PINT; CALL; } break; \
        default: { constexpr int M = LP_PGEN; CALL; } break;      \
    }

extern "C" int bf_lp_rows_fwd(const float* pred, const float* y, int64_t rows, int64_t n, double p, float* ratio, double* sums, double* ws,
                              int64_t ws_doubles, bf_stream_t stream) {
    BF_REQUIRE(pred && y && ratio && sums && lp_sizes_ok(rows, n), "bf_lp_rows_fwd: bad arguments");
    BF_REQUIRE(p >= 1.0 && p < INFINITY, "bf_lp_rows_fwd: p must be finite and >= 1");
    BF_REQUIRE((((uintptr_t)pred | (uintptr_t)y | (uintptr_t)ratio) & 3) == 0 && ((uintptr_t)sums & 7) == 0, "bf_lp_rows_fwd: misaligned pointer");
    LpPow pw;
    const int mode = lp_mode(p, &pw), chunks = lp_chunks(rows, n);
    hipStream_t st = (hipStream_t)stream;
    if (chunks > 0) {
        BF_REQUIRE(ws && ((uintptr_t)ws & 7) == 0 && ws_doubles >= 2 * rows * chunks, "bf_lp_rows_fwd: workspace smaller than bf_lp_rows_ws_doubles");
        BF_REQUIRE(rows * chunks < ((int64_t)1 << 31), "bf_lp_rows_fwd: too many rows");
        LP_DISPATCH(mode, hipLaunchKernelGGL(lp_long_fwd_kernel<M>, dim3((unsigned)(rows * chunks)), dim3(NT), 0, st, pred, y, (long)n, chunks, pw, ws));
        BF_CHECK_LAUNCH();
        LP_DISPATCH(mode, hipLaunchKernelGGL(lp_finish_kernel<M>, dim3((unsigned)bf_cdiv(rows, 64)), dim3(64), 0, st, (const double*)ws, (long)rows, chunks, p, ratio, sums));
    } else {
        const int width = lp_width(n);
        const int64_t grid = (rows * width + NT - 1) / NT;
        BF_REQUIRE(grid < ((int64_t)1 << 31), "bf_lp_rows_fwd: too many rows");
        LP_DISPATCH(mode, hipLaunchKernelGGL(lp_short_fwd_kernel<M>, dim3((unsigned)grid), dim3(NT), 0, st, pred, y, (long)rows, (long)n, width, p, pw, ratio, sums));
    }
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_lp_rows_bwd(const float* pred, const float* y, const float* g, const double* sums, int64_t rows, int64_t n, double p, float* dpred,
                              bf_stream_t stream) {
    BF_REQUIRE(pred && y && g && sums && dpred && lp_sizes_ok(rows, n), "bf_lp_rows_bwd: bad arguments");
    BF_REQUIRE(p >= 1.0 && p < INFINITY, "bf_lp_rows_bwd: p must be finite and >= 1");
    BF_REQUIRE((((uintptr_t)pred | (uintptr_t)y | (uintptr_t)g | (uintptr_t)dpred) & 3) == 0 && ((uintptr_t)sums & 7) == 0, "bf_lp_rows_bwd: misaligned pointer");
    BF_REQUIRE(dpred != pred && dpred != y, "bf_lp_rows_bwd: the gradient cannot alias an input");
    LpPow pw;
    const int mode = lp_mode(p, &pw), chunks = lp_chunks(rows, n);
    hipStream_t st = (hipStream_t)stream;
    if (chunks > 0) {
        BF_REQUIRE(rows * chunks < ((int64_t)1 << 31), "bf_lp_rows_bwd: too many rows");
        LP_DISPATCH(mode, hipLaunchKernelGGL(lp_long_bwd_kernel<M>, dim3((unsigned)(rows * chunks)), dim3(NT), 0, st, pred, y, g, sums, (long)n, chunks, p, pw, dpred));
    } else {
        const int width = lp_width(n);
        const int64_t grid = (rows * width + NT - 1) / NT;
        BF_REQUIRE(grid < ((int64_t)1 << 31), "bf_lp_rows_bwd: too many rows");
        LP_DISPATCH(mode, hipLaunchKernelGGL(lp_short_bwd_kernel<M>, dim3((unsigned)grid), dim3(NT), 0, st, pred, y, g, sums, (long)rows, (long)n, width, p, pw, dpred));
    }
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_eikonal_bwd(const float* phi, int64_t frames, int H, int W, float dx, const float* g, float* dphi, bf_stream_t stream) {
    BF_REQUIRE(phi && g && dphi && frames > 0 && H > 0 && W > 0 && dx > 0.f && phi != dphi, "bf_eikonal_bwd: bad arguments");
    BF_REQUIRE(frames <= ((int64_t)1 << 40) / ((int64_t)H * W), "bf_eikonal_bwd: too many cells");
    const int tiles_y = bf_cdiv(H, EIK_TH), tiles_x = bf_cdiv(W, EIK_TW);
    const int64_t tiles = frames * tiles_y * tiles_x;
    BF_REQUIRE(tiles < ((int64_t)1 << 31), "bf_eikonal_bwd: too many tiles");
    hipLaunchKernelGGL(eikonal_bwd_kernel, dim3((unsigned)tiles), dim3(NT), 0, (hipStream_t)stream, phi, (long)frames, H, W, tiles_y, tiles_x,
                       1.0 / (double)dx, g, dphi);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t bf_wlp_ws_doubles(int64_t frames, int C, int H, int W) {
    if (!wlp_sizes_ok(frames, C, H, W)) return -1;
    return wlp_plan(frames, C, H, W).eik + WLP_EIK_MAX_WGS;
}

#define WLP_DISPATCH(C, CALL)                                   \
    if ((C) <= 1) { constexpr int CT = 1; CALL; }               \
    else if ((C) <= 2) { constexpr int CT = 2; CALL; }          \
    else if ((C) <= 4) { constexpr int CT = 4; CALL; }          \
    else if ((C) <= 8) { constexpr int CT = 8; CALL; }          \
    else { constexpr int CT = WLP_MAX_C; CALL; }

extern "C" int bf_wlp_fwd(const float* pred, const float* y, int64_t frames, int C, int H, int W, int s, double diff_s, double div_s, double band, double gain,
                          const double* field_weights, double eikonal, double dx, float* loss, float* terms, double* sums, double* ws, int64_t ws_doubles,
                          bf_stream_t stream) {
    BF_REQUIRE(pred && y && loss && terms && sums && ws, "bf_wlp_fwd: null pointer");
    const char* why = wlp_refusal(frames, C, H, W, s, diff_s, div_s, band, gain, field_weights, eikonal, dx);
    if (why) return bf_fail_msg((std::string("bf_wlp_fwd: ") + why).c_str(), __FILE__, __LINE__);
    BF_REQUIRE((((uintptr_t)pred | (uintptr_t)y | (uintptr_t)loss | (uintptr_t)terms) & 3) == 0 && (((uintptr_t)sums | (uintptr_t)ws) & 7) == 0,
               "bf_wlp_fwd: misaligned pointer");
    const WlpPlan p = wlp_plan(frames, C, H, W);
    BF_REQUIRE(ws_doubles >= p.eik + WLP_EIK_MAX_WGS, "bf_wlp_fwd: workspace smaller than bf_wlp_ws_doubles");
    BF_REQUIRE(p.grid < ((int64_t)1 << 31), "bf_wlp_fwd: too many frames");
    const long hw = (long)H * W;
    const WlpHat hat = wlp_hat(diff_s, div_s, band, gain);
    const int eik_n = eikonal > 0.0 ? wlp_eik_wgs(frames, hw) : 0;
    hipStream_t st = (hipStream_t)stream;
    WLP_DISPATCH(C, hipLaunchKernelGGL(wlp_fwd_kernel<CT>, dim3((unsigned)p.grid), dim3(NT), 0, st, pred, y, (long)frames, hw, C, s, p.chunks, p.width, hat,
                                       ws));
    BF_CHECK_LAUNCH();
    if (eik_n > 0) {
        hipLaunchKernelGGL(wlp_eik_fwd_kernel, dim3((unsigned)eik_n), dim3(NT), 0, st, pred, (long)frames, (long)C * hw, (long)s * hw, H, W, div_s / dx, ws + p.eik);
        BF_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(wlp_finish_kernel, dim3(1), dim3(NT), 0, st, (const double*)ws, (long)frames, C, p.chunks, wlp_fields(field_weights, C),
                       (const double*)(ws + p.eik), eik_n, eikonal / ((double)frames * (double)hw), sums, ws + p.rho, loss, terms);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_wlp_bwd(const float* pred, const float* y, const float* g, const double* sums, int64_t frames, int C, int H, int W, int s, double diff_s,
                          double div_s, double band, double gain, const double* field_weights, double eikonal, double dx, float* dpred, bf_stream_t stream) {
    BF_REQUIRE(pred && y && g && sums && dpred, "bf_wlp_bwd: null pointer");
    const char* why = wlp_refusal(frames, C, H, W, s, diff_s, div_s, band, gain, field_weights, eikonal, dx);
    if (why) return bf_fail_msg((std::string("bf_wlp_bwd: ") + why).c_str(), __FILE__, __LINE__);
    BF_REQUIRE((((uintptr_t)pred | (uintptr_t)y | (uintptr_t)g | (uintptr_t)dpred) & 3) == 0 && ((uintptr_t)sums & 7) == 0, "bf_wlp_bwd: misaligned pointer");
    const long hw = (long)H * W;
    const uintptr_t bytes = (uintptr_t)frames * C * hw * 4, d = (uintptr_t)dpred;
    BF_REQUIRE((d + bytes <= (uintptr_t)pred || (uintptr_t)pred + bytes <= d) && (d + bytes <= (uintptr_t)y || (uintptr_t)y + bytes <= d),
               "bf_wlp_bwd: the gradient cannot alias an input");
    const WlpPlan p = wlp_plan(frames, C, H, W);
    BF_REQUIRE(p.grid < ((int64_t)1 << 31), "bf_wlp_bwd: too many frames");
    const WlpHat hat = wlp_hat(diff_s, div_s, band, gain);
    hipStream_t st = (hipStream_t)stream;
    WLP_DISPATCH(C, hipLaunchKernelGGL(wlp_bwd_kernel<CT>, dim3((unsigned)p.grid), dim3(NT), 0, st, pred, y, g, sums, (long)frames, hw, C, s, p.chunks, p.width, hat,
                                       wlp_fields(field_weights, C), dpred));
    BF_CHECK_LAUNCH();
    if (eikonal > 0.0) {
        const int tiles_y = bf_cdiv(H, EIK_TH), tiles_x = bf_cdiv(W, EIK_TW);
        const int64_t tiles = frames * tiles_y * tiles_x;
        BF_REQUIRE(tiles < ((int64_t)1 << 31), "bf_wlp_bwd: too many tiles");
        hipLaunchKernelGGL(wlp_eik_bwd_kernel, dim3((unsigned)tiles), dim3(NT), 0, st, pred, (long)frames, (long)C * hw, (long)s * hw, H, W, tiles_y, tiles_x,
                           div_s / dx, eikonal, g, dpred);
        BF_CHECK_LAUNCH();
    }
    return 0;
}
