// Physics metrics of a clip, and the comparison of two flux series:
//   eikonal (sum of squares) / eikonal_l1 (the notebook's per-frame score) of a signed-distance field, heatflux_rows of a clip's heater rows.
//   Their per-pixel and per-row expressions are clip_store.h's, shared with the per-step rollout kernels (rollout.hip);
//   kde_kl: what examples/data_visualization.ipynb (cell 4) makes of two flux series: a Gaussian KDE of each, KL(sim || model) by Simpson's rule.
//
// KDE / KL, everything in fp64, three launches per call, no atomics (two calls give the same bits), O(n + m + points) memory:
//   kde_stats_kernel  grid (2 sets, R rows): count is n; mean, then centred squares (np.cov(ddof=1)), min and max, each reduced in a fixed order;
//   kde_partial_kernel grid (grid-point tiles of 256, slabs of both sets, R): a workgroup stages its slab of samples in LDS KDE_CHUNK at a time
//                     (every lane reads the same address: a broadcast) and each thread adds exp(-((x_i - s_j) / h)^2 / 2) over the slab into
//                     two accumulators (even / odd sample), leaving one fp64 partial per (slab, grid point) in the workspace.  The number of
//                     slabs depends on n alone (at most KDE_MAX_SLABS), so a row has the same bits alone and in a batch;
//   kde_finish_kernel grid (R): adds the slabs in slab order, divides by n h sqrt(2 pi), forms f = p log(p / q) (q == 0 -> eps; f = 0 where
//                     p == 0, the limit -- numpy has NaN there) and applies scipy.integrate.simpson's rule for a uniform grid.
#include "clip_store.h"
#include <algorithm>
#include <math.h>

namespace {
constexpr int NT = 256;
constexpr int KDE_CHUNK = 1024;        // samples in LDS at a time: 8 KiB
constexpr int KDE_SLAB_MIN = 256;      // a set is not cut into slabs shorter than this
constexpr int KDE_MAX_SLABS = 64;      // bounds the workspace at 2 * 64 * points doubles per row, whatever n
constexpr int KDE_STATS = 4;           // {mean, unbiased variance, min, max} per (row, set)

int grid_for(long total) { return (int)std::max<long>(1, std::min<long>((total + NT - 1) / NT, 256L * 16)); }

// ---------------------------------------------------------------------------- physics metrics of a clip
// Eikonal residual of a signed-distance field (utils/losses.py:5-15): torch.gradient(edge_order=1, spacing=dx) along H and W
// (central differences inside, one-sided at the borders), out += sum over pixels of (|grad phi| - 1)^2   (caller divides by the count)
__global__ void __launch_bounds__(NT) eikonal_kernel(const float* __restrict__ phi, long frames, int H, int W, float inv_dx, double* __restrict__ out) {
    __shared__ double red[NT / 64];
    const long total = frames * H * W;
    double acc = 0.0;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int x = (int)(i % W), y = (int)((i / W) % H);
        const float* p = phi + i;
        float gy, gx;
        if (H == 1) gy = 0.f;
        else if (y == 0) gy = (p[W] - p[0]) * inv_dx;
        else if (y == H - 1) gy = (p[0] - p[-W]) * inv_dx;
        else gy = (p[W] - p[-W]) * (0.5f * inv_dx);
        if (W == 1) gx = 0.f;
        else if (x == 0) gx = (p[1] - p[0]) * inv_dx;
        else if (x == W - 1) gx = (p[0] - p[-1]) * inv_dx;
        else gx = (p[1] - p[-1]) * (0.5f * inv_dx);
        const float r = sqrtf(gy * gy + gx * gx) - 1.f;
        acc += (double)(r * r);
    }
    const double t = block_reduce<RED_SUM, NT / 64>(acc, red);
    if (threadIdx.x == 0) atomicAdd(out, t);
}
// The rollout notebook's Eikonal score (scripts/inference_autoregressive.ipynb, `get_eikonal_loss`): per frame, the mean of
// | |grad phi| - 1 | with central differences at spacing dx in the interior and the border taking its neighbour's gradient
// (replicate padding).  One workgroup per frame.
__global__ void __launch_bounds__(NT) eikonal_l1_kernel(const float* __restrict__ phi, int H, int W, float inv_2dx, float* __restrict__ out) {
    __shared__ double red[NT / 64];
    const float* f = phi + (long)blockIdx.x * H * W;
    double acc = 0.0;
    for (int i = threadIdx.x; i < H * W; i += NT)
        acc += (double)eikonal_l1_px([&](int yy, int xx) { return f[yy * W + xx]; }, i % W, i / W, H, W, inv_2dx);
    const double t = block_reduce<RED_SUM, NT / 64>(acc, red);
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(t / ((double)H * W));
}
// Heater heat flux per frame (utils/heatflux.py:17-38): heater_row_flux of the bottom row y = 0, coef = 0.054 / (dx * lc).  A wave per frame.
__global__ void __launch_bounds__(64) heatflux_kernel(const float* __restrict__ dfun, const float* __restrict__ temp, long frame_stride, int W,
                                                     float x_min, float dx, float heater_temp, float coef, float* __restrict__ flux) {
    const float* d = dfun + (long)blockIdx.x * frame_stride;
    const float* t = temp + (long)blockIdx.x * frame_stride;
    const float f = heater_row_flux([&](int x) { return d[x]; }, [&](int x) { return t[x]; }, W, x_min, dx, heater_temp, coef);
    if (threadIdx.x == 0) flux[blockIdx.x] = f;
}

// ---------------------------------------------------------------------------- Gaussian KDE and KL(p || q)
__global__ void __launch_bounds__(NT) kde_stats_kernel(const double* __restrict__ p, const double* __restrict__ q, long n, long m, double* __restrict__ stats) {
    __shared__ double red[NT / 64];
    const int set = blockIdx.x, r = blockIdx.y;
    const long len = set ? m : n;
    const double* v = (set ? q : p) + (long)r * len;
    double sum = 0.0, lo = INFINITY, hi = -INFINITY;
    for (long j = threadIdx.x; j < len; j += NT) { const double x = v[j]; sum += x; lo = fmin(lo, x); hi = fmax(hi, x); }
    const double mean = block_reduce<RED_SUM, NT / 64>(sum, red) / (double)len;
    lo = block_reduce<RED_MIN, NT / 64>(lo, red);
    hi = block_reduce<RED_MAX, NT / 64>(hi, red);
    double sq = 0.0;
    for (long j = threadIdx.x; j < len; j += NT) { const double e = v[j] - mean; sq += e * e; }
    const double var = block_reduce<RED_SUM, NT / 64>(sq, red) / (double)(len - 1);
    if (threadIdx.x == 0) {
        double* st = stats + ((long)r * 2 + set) * KDE_STATS;
        st[0] = mean; st[1] = var; st[2] = lo; st[3] = hi;
    }
}

static int kde_slabs(long n) { return (int)std::max<long>(1, std::min<long>(KDE_MAX_SLABS, (n + KDE_SLAB_MIN - 1) / KDE_SLAB_MIN)); }

// grid point i of np.linspace(lo, hi, points): i * step + lo (a product, then a sum: two roundings, not one fused), the last one hi itself
__device__ __forceinline__ double kde_grid_x(int i, int points, double lo, double hi, double step) {
#pragma clang fp contract(off)
    const double prod = (double)i * step;
    return i == points - 1 ? hi : prod + lo;
}

__global__ void __launch_bounds__(NT) kde_partial_kernel(const double* __restrict__ p, const double* __restrict__ q, long n, long m, int points, int slabs_p,
                                                        int slabs_q, double scott_p, double scott_q, const double* __restrict__ stats,
                                                        double* __restrict__ part) {
    __shared__ double sm[KDE_CHUNK];
    const int r = blockIdx.z, slab = blockIdx.y, set = slab >= slabs_p;
    const int k = set ? slab - slabs_p : slab, nslab = set ? slabs_q : slabs_p;
    const long len = set ? m : n;
    const double* v = (set ? q : p) + (long)r * len;
    const double* st = stats + (long)r * 2 * KDE_STATS;
    const double lo = fmin(st[2], st[KDE_STATS + 2]), hi = fmax(st[3], st[KDE_STATS + 3]), step = (hi - lo) / (double)(points - 1);
    const double inv_h = 1.0 / ((set ? scott_q : scott_p) * sqrt(st[set * KDE_STATS + 1]));
    const long per = (len + nslab - 1) / nslab, j0 = (long)k * per, j1 = min(len, j0 + per);
    const int i = blockIdx.x * NT + threadIdx.x;
    const double x = kde_grid_x(min(i, points - 1), points, lo, hi, step);
    double a0 = 0.0, a1 = 0.0;
    for (long c0 = j0; c0 < j1; c0 += KDE_CHUNK) {
        const int cn = (int)min((long)KDE_CHUNK, j1 - c0);
        __syncthreads();
        for (int j = threadIdx.x; j < cn; j += NT) sm[j] = v[c0 + j];
        __syncthreads();
        int j = 0;
        for (; j + 1 < cn; j += 2) {
            const double d0 = (x - sm[j]) * inv_h, d1 = (x - sm[j + 1]) * inv_h;
            a0 += exp(-0.5 * (d0 * d0));
            a1 += exp(-0.5 * (d1 * d1));
        }
        if (j < cn) { const double d0 = (x - sm[j]) * inv_h; a0 += exp(-0.5 * (d0 * d0)); }
    }
    if (i < points) part[((long)r * (slabs_p + slabs_q) + slab) * points + i] = a0 + a1;
}

__global__ void __launch_bounds__(NT) kde_finish_kernel(long n, long m, int points, int slabs_p, int slabs_q, double scott_p, double scott_q, double eps,
                                                       const double* __restrict__ stats, const double* __restrict__ part, double* __restrict__ kl,
                                                       double* __restrict__ xs, double* __restrict__ pdf_p, double* __restrict__ pdf_q) {
    __shared__ double red[NT / 64];
    const int r = blockIdx.x;
    const double* st = stats + (long)r * 2 * KDE_STATS;
    const double var_p = st[1], var_q = st[KDE_STATS + 1];
    const bool ok = var_p > 0.0 && var_q > 0.0;                             // a constant set has no bandwidth (scipy raises): NaN
    const double lo = fmin(st[2], st[KDE_STATS + 2]), hi = fmax(st[3], st[KDE_STATS + 3]), step = (hi - lo) / (double)(points - 1);
    const double norm_p = (double)n * (scott_p * sqrt(var_p)) * sqrt(2.0 * M_PI), norm_q = (double)m * (scott_q * sqrt(var_q)) * sqrt(2.0 * M_PI);
    const double* pp = part + (long)r * (slabs_p + slabs_q) * points;
    const double* pq = pp + (long)slabs_p * points;
    const int simpson_n = (points & 1) ? points : points - 1;               // even point count: Simpson on the first points - 1, then the last interval
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < points; i += NT) {
        double sp = 0.0, sq = 0.0;
        for (int k = 0; k < slabs_p; ++k) sp += pp[(long)k * points + i];
        for (int k = 0; k < slabs_q; ++k) sq += pq[(long)k * points + i];
        const double dp = ok ? sp / norm_p : NAN, dq = ok ? sq / norm_q : NAN;
        if (xs) xs[(long)r * points + i] = kde_grid_x(i, points, lo, hi, step);
        if (pdf_p) pdf_p[(long)r * points + i] = dp;
        if (pdf_q) pdf_q[(long)r * points + i] = dq;
        const double f = dp == 0.0 ? 0.0 : dp * log(dp / (dq == 0.0 ? eps : dq));
        if (i < simpson_n) s1 += ((i == 0 || i == simpson_n - 1) ? 1.0 : (i & 1) ? 4.0 : 2.0) * f;
        if (simpson_n != points && i >= points - 3) s2 += (i == points - 1 ? 5.0 : i == points - 2 ? 8.0 : -1.0) * f;
    }
    s1 = block_reduce<RED_SUM, NT / 64>(s1, red);
    s2 = block_reduce<RED_SUM, NT / 64>(s2, red);
    if (threadIdx.x == 0) kl[r] = step * (s1 / 3.0) + step * (s2 / 12.0);
}
}  // namespace

extern "C" int bf_eikonal_sum(const float* phi, int64_t frames, int H, int W, float dx, double* out, bf_stream_t stream) {
    BF_REQUIRE(phi && out && frames > 0 && H > 0 && W > 0 && dx > 0.f, "bf_eikonal_sum: bad arguments");
    hipLaunchKernelGGL(eikonal_kernel, dim3(grid_for(frames * H * W)), dim3(NT), 0, (hipStream_t)stream, phi, (long)frames, H, W, 1.f / dx, out);
    BF_CHECK_LAUNCH();
    return 0;
}
extern "C" int bf_eikonal_l1_frames(const float* phi, int64_t frames, int H, int W, float dx, float* out, bf_stream_t stream) {
    BF_REQUIRE(phi && out && frames > 0 && H >= 3 && W >= 3 && dx > 0.f, "bf_eikonal_l1_frames: bad arguments (central differences need >= 3 points per axis)");
    hipLaunchKernelGGL(eikonal_l1_kernel, dim3((unsigned)frames), dim3(NT), 0, (hipStream_t)stream, phi, H, W, 0.5f / dx, out);
    BF_CHECK_LAUNCH();
    return 0;
}
extern "C" int bf_heatflux_rows(const float* dfun, const float* temp, int64_t frames, int64_t frame_stride, int W, float x_min, float dx,
                                float heater_temp, float lc, float* flux, bf_stream_t stream) {
    BF_REQUIRE(dfun && temp && flux && frames > 0 && W > 0 && dx > 0.f && lc > 0.f, "bf_heatflux_rows: bad arguments");
    hipLaunchKernelGGL(heatflux_kernel, dim3((unsigned)frames), dim3(64), 0, (hipStream_t)stream, dfun, temp, (long)frame_stride, W, x_min, dx,
                       heater_temp, 0.054f / (dx * lc), flux);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t bf_kde_kl_ws_doubles(int R, int64_t n, int64_t m, int points) {
    if (R <= 0 || n < 2 || m < 2 || points < 3) return 0;
    return (int64_t)R * (2 * KDE_STATS + (int64_t)(kde_slabs(n) + kde_slabs(m)) * points);
}

extern "C" int bf_kde_kl(const double* p, const double* q, int R, int64_t n, int64_t m, int points, double eps, double* kl, double* x, double* pdf_p,
                         double* pdf_q, double* ws, int64_t ws_doubles, bf_stream_t stream) {
    BF_REQUIRE(p && q && kl && ws, "bf_kde_kl: null pointer");
    BF_REQUIRE(R > 0 && R <= 65535 && n >= 2 && m >= 2 && points >= 3, "bf_kde_kl: needs 1 <= R <= 65535 rows, n >= 2, m >= 2 samples and points >= 3");
    BF_REQUIRE(ws_doubles >= bf_kde_kl_ws_doubles(R, n, m, points), "bf_kde_kl: workspace smaller than bf_kde_kl_ws_doubles");
    BF_REQUIRE(((uintptr_t)p % 8 == 0) && ((uintptr_t)q % 8 == 0) && ((uintptr_t)ws % 8 == 0), "bf_kde_kl: buffers must be 8-byte aligned");
    const int sp = kde_slabs(n), sq = kde_slabs(m);
    const double scott_p = pow((double)n, -0.2), scott_q = pow((double)m, -0.2);      // scipy's default factor for one dimension: n^(-1 / (d + 4))
    double* stats = ws;
    double* part = ws + (long)R * 2 * KDE_STATS;
    hipLaunchKernelGGL(kde_stats_kernel, dim3(2, (unsigned)R), dim3(NT), 0, (hipStream_t)stream, p, q, (long)n, (long)m, stats);
    BF_CHECK_LAUNCH();
    hipLaunchKernelGGL(kde_partial_kernel, dim3((unsigned)bf_cdiv(points, NT), (unsigned)(sp + sq), (unsigned)R), dim3(NT), 0, (hipStream_t)stream, p, q,
                       (long)n, (long)m, points, sp, sq, scott_p, scott_q, (const double*)stats, part);
    BF_CHECK_LAUNCH();
    hipLaunchKernelGGL(kde_finish_kernel, dim3((unsigned)R), dim3(NT), 0, (hipStream_t)stream, (long)n, (long)m, points, sp, sq, scott_p, scott_q, eps,
                       (const double*)stats, (const double*)part, kl, x, pdf_p, pdf_q);
    BF_CHECK_LAUNCH();
    return 0;
}
