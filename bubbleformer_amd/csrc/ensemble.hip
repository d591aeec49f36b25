// Ensemble statistics across the M members of a forecast, per frame: RMSE of the ensemble mean, spread, CRPS and the rank histogram of the truth
// (the reference has no program for it).  One body serves bf_ensemble_scores (members and truth as tensors) and
// bf_rollout_ensemble (one rollout step: the members are row blocks of the prediction, the truth is read where it lies in the store, through
// clip_store.h's RolloutStep as bf_rollout_score reads it).
// Pass 1: grid (rows, frames); a workgroup sweeps a contiguous share of one frame in 4-pixel groups of a row, holds the M values of its 4 pixels in
// registers (16-byte loads of every member and of the truth; a scalar path where alignment or a ragged last group forbid them) and leaves
// {sum (mean - y)^2, sum_p sum_m (x_m - mean)^2, sum_p sum_m |x_m - y|, sum_p sum_{m<n} |x_m - x_n|} in fp64 and its rank counts in int32.  Pass 2: one workgroup per frame
// adds the partials in row order and rounds once.  No float atomics (the counts go through integer LDS atomics, which are exact): two calls give the
// same bits, and a frame has the same bits in either entry point.
#include "clip_store.h"
#include <algorithm>

namespace {
constexpr int NT = 256;
constexpr int ENS_QUADS = 1024, ENS_MAX_ROWS = 64;    // 4-pixel groups per workgroup (4 per thread) until ENS_MAX_ROWS workgroups share a frame
constexpr int ENS_MAX_MEMBERS = 32;
int ens_rows(int H, int W) { return (int)std::max<long>(1, std::min<long>(ENS_MAX_ROWS, ((long)H * ((W + 3) / 4) + ENS_QUADS - 1) / ENS_QUADS)); }

struct EnsArgs {
    RolloutStep v; int rollout;                       // rollout: x = v.pred, the truth = the stored frames of step *v.step; else x / y below
    const float* x; long member_stride; const float* y;
    int M, H, W, f0, rows, fair;                      // H x W = the grid the members live on; f0 = the first frame of this launch
    int vec_x, vec_y, vec_mean;                       // 16-byte accesses allowed (alignment and W % 4 == 0, decided on the host)
    double* part; int* hist_part;                     // [frames][rows][4], [frames][rows][M + 1]
    float *mean_rmse, *spread, *crps, *mean; int* rank_hist;
    int frames, T, C;                                 // rollout: frame fc = (b * T + t) * C + c of the Bt = v.B / M trajectories
};

__device__ __forceinline__ float pick(const float4& q, int j) { return j == 0 ? q.x : j == 1 ? q.y : j == 2 ? q.z : q.w; }

// the report row of frame f: f itself, or (b, s * T + t, c) of (Bt, steps * T, C)
__device__ __forceinline__ long ens_out_row(const EnsArgs& a, int s, int f) {
    if (!a.rollout) return f;
    const int c = f % a.C, t = (f / a.C) % a.T, b = f / (a.C * a.T);
    return a.v.row(s, b, t) * a.C + c;
}

// MC = the member count rounded up to 4, 8, 16 or 32: the register arrays' extent.  Up to 8 members the four pixels of a group are unrolled; above,
// one pixel at a time is picked out of the loaded 16-byte groups, so that the pair loop's code (MC^2 / 2 differences) exists once, not four times.
template <int MC>
__global__ void __launch_bounds__(NT) ensemble_kernel(EnsArgs a) {
    constexpr int UJ = MC <= 8 ? 4 : 1;
    __shared__ double red[NT / 64][4];      // several values at once in this kernel's own order, which its restatement's bits pin: not bf_common.h's block_reduce
    __shared__ int hist[ENS_MAX_MEMBERS + 1];
    const RolloutStep& v = a.v;
    int s = 0;
    if (a.rollout) { s = v.current(); if (s < 0) return; }                 // a step behind the last row: nothing is written
    const int M = a.M, H = a.H, W = a.W, f = a.f0 + blockIdx.y;
    const long px = (long)H * W;
    const int wq = (W + 3) / 4, quads = H * wq, per = (quads + a.rows - 1) / a.rows;
    const int lo = blockIdx.x * per, hi = min(quads, lo + per);
    const float* xf = a.x + f * px;                                        // member 0 of this frame; member m lies m * member_stride behind
    const float* tf;
    float d = 0.f, q = 1.f, sy = 1.f, sx = 1.f;
    bool ident = true;
    int SH = H, SW = W;                                                    // the grid the truth lies on
    if (a.rollout) {
        const int c = f % a.C, t = (f / a.C) % a.T, b = f / (a.C * a.T);
        tf = v.stored(c, v.frame(s, b, t));                                // first[b]: rows b and m * Bt + b start at the same frame
        d = v.diff[c]; q = v.dv[c]; sy = v.sy(); sx = v.sx(); ident = v.ident(); SH = v.H; SW = v.W;
    } else
        tf = a.y + f * px;
    float* mf = a.mean ? a.mean + ens_out_row(a, s, f) * px : nullptr;
    const bool want_hist = a.rank_hist != nullptr;
    for (int i = threadIdx.x; i <= M; i += NT) hist[i] = 0;
    __syncthreads();
    double se = 0.0, sv = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = lo + threadIdx.x; i < hi; i += NT) {
        const int xq = i % wq, yo = i / wq, nv = min(4, W - 4 * xq);
        const long o = (long)yo * W + 4 * xq;
        float4 xv[MC], yv = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int m = 0; m < MC; ++m) {
            xv[m] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m < M) {
                const float* p = xf + m * a.member_stride + o;
                if (a.vec_x) xv[m] = *reinterpret_cast<const float4*>(p);
                else { xv[m].x = p[0]; if (nv > 1) xv[m].y = p[1]; if (nv > 2) xv[m].z = p[2]; if (nv > 3) xv[m].w = p[3]; }
            }
        }
        if (a.rollout) {
            const float* row = tf + (long)nearest_src(yo, sy, SH, ident) * SW;
            if (a.vec_y) {
                const float4 r = *reinterpret_cast<const float4*>(row + 4 * xq);
                yv = make_float4(clip_norm(r.x, d, q), clip_norm(r.y, d, q), clip_norm(r.z, d, q), clip_norm(r.w, d, q));
            } else {
                yv.x = clip_norm(row[nearest_src(4 * xq, sx, SW, ident)], d, q);
                if (nv > 1) yv.y = clip_norm(row[nearest_src(4 * xq + 1, sx, SW, ident)], d, q);
                if (nv > 2) yv.z = clip_norm(row[nearest_src(4 * xq + 2, sx, SW, ident)], d, q);
                if (nv > 3) yv.w = clip_norm(row[nearest_src(4 * xq + 3, sx, SW, ident)], d, q);
            }
        } else if (a.vec_y)
            yv = *reinterpret_cast<const float4*>(tf + o);
        else { yv.x = tf[o]; if (nv > 1) yv.y = tf[o + 1]; if (nv > 2) yv.z = tf[o + 2]; if (nv > 3) yv.w = tf[o + 3]; }
        float mv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll UJ
        for (int j = 0; j < 4; ++j) {
            if (j >= nv) break;
            double xd[MC];
#pragma unroll
            for (int m = 0; m < MC; ++m) xd[m] = (double)pick(xv[m], j);
            const double y = (double)pick(yv, j);
            double sum = 0.0, a1 = 0.0, a2 = 0.0;
            int below = 0;
#pragma unroll
            for (int m = 0; m < MC; ++m)
                if (m < M) {                                               // uniform: one scalar branch per member, none per pair
                    sum += xd[m]; a1 += fabs(xd[m] - y); below += xd[m] < y ? 1 : 0;
#pragma unroll
                    for (int n = 0; n < m; ++n) a2 += fabs(xd[m] - xd[n]);
                }
            const double mean = sum / (double)M;
            double ss = 0.0;
#pragma unroll
            for (int m = 0; m < MC; ++m)
                if (m < M) { const double c = xd[m] - mean; ss += c * c; }       // the second pass over the values in registers: centred squares
            const double e = mean - y;
            se += e * e; sv += ss; s1 += a1; s2 += a2;
            if (want_hist) atomicAdd(&hist[below], 1);
            const float mr = (float)mean;
            if (j == 0) mv[0] = mr; else if (j == 1) mv[1] = mr; else if (j == 2) mv[2] = mr; else mv[3] = mr;
        }
        if (mf) {
            if (a.vec_mean) *reinterpret_cast<float4*>(mf + o) = make_float4(mv[0], mv[1], mv[2], mv[3]);
            else { mf[o] = mv[0]; if (nv > 1) mf[o + 1] = mv[1]; if (nv > 2) mf[o + 2] = mv[2]; if (nv > 3) mf[o + 3] = mv[3]; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { se += __shfl_xor(se, o, 64); sv += __shfl_xor(sv, o, 64); s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
    if ((threadIdx.x & 63) == 0) { double* r = red[threadIdx.x >> 6]; r[0] = se; r[1] = sv; r[2] = s1; r[3] = s2; }
    __syncthreads();                                                       // also: every count of this workgroup is in hist
    const long slot = (long)f * a.rows + blockIdx.x;
    if (threadIdx.x < 4) {
        double sum = 0.0;
        for (int w = 0; w < NT / 64; ++w) sum += red[w][threadIdx.x];
        a.part[slot * 4 + threadIdx.x] = sum;
    }
    if (want_hist)
        for (int i = threadIdx.x; i <= M; i += NT) a.hist_part[slot * (M + 1) + i] = hist[i];
}

// part [frames][rows][4], hist_part [frames][rows][M + 1] -> the rows of frame blockIdx.x, the partials added in row order
__global__ void __launch_bounds__(64) ensemble_finish_kernel(EnsArgs a) {
    int s = 0;
    if (a.rollout) { s = a.v.current(); if (s < 0) return; }
    const int f = blockIdx.x, M = a.M;
    const long out = ens_out_row(a, s, f);
    if (threadIdx.x == 0) {
        double se = 0.0, sv = 0.0, s1 = 0.0, s2 = 0.0;
        for (int r = 0; r < a.rows; ++r) { const double* p = a.part + ((long)f * a.rows + r) * 4; se += p[0]; sv += p[1]; s1 += p[2]; s2 += p[3]; }
        const double n = (double)a.H * (double)a.W, m = (double)M;
        const double w = a.fair ? 1.0 / (2.0 * m * (m - 1.0)) : 1.0 / (2.0 * m * m);      // on the full double sum = 2 * s2
        a.mean_rmse[out] = (float)sqrt(se / n);
        a.spread[out] = (float)sqrt(sv / (m - 1.0) / n);                      // sv = the centred squares: the unbiased variance's divisor here
        a.crps[out] = (float)((s1 / m - w * (2.0 * s2)) / n);
    }
    if (a.rank_hist)
        for (int i = threadIdx.x; i <= M; i += 64) {
            int cnt = 0;
            for (int r = 0; r < a.rows; ++r) cnt += a.hist_part[((long)f * a.rows + r) * (M + 1) + i];
            a.rank_hist[out * (M + 1) + i] = cnt;
        }
}

long ens_ws_bytes(long frames, int M, int rows) { return (frames * rows * (4 * 8 + (M + 1) * 4L) + 15) / 16 * 16; }

bool ens_sizes_ok(long frames, int M, int H, int W) {
    return frames > 0 && frames <= 0x7fffffffL && M >= 2 && M <= ENS_MAX_MEMBERS && H > 0 && W > 0 && (long)H * W <= (1L << 30) &&
           frames <= (1L << 40) / ((long)H * W);
}

int launch_ensemble(EnsArgs& a, const bf_ensemble_rows& rows, void* ws, hipStream_t st) {
    a.rows = ens_rows(a.H, a.W);
    a.part = (double*)ws;
    a.hist_part = (int*)((char*)ws + (long)a.frames * a.rows * 4 * 8);
    a.mean_rmse = rows.mean_rmse; a.spread = rows.spread; a.crps = rows.crps; a.rank_hist = rows.rank_hist; a.mean = rows.mean;
    a.vec_mean = a.mean && (a.W & 3) == 0 && (uintptr_t)a.mean % 16 == 0;
    for (int f0 = 0; f0 < a.frames; f0 += 65535) {                         // the grid's y extent
        a.f0 = f0;
        const dim3 grid((unsigned)a.rows, (unsigned)std::min(65535, a.frames - f0));
        if (a.M <= 4) hipLaunchKernelGGL(ensemble_kernel<4>, grid, dim3(NT), 0, st, a);
        else if (a.M <= 8) hipLaunchKernelGGL(ensemble_kernel<8>, grid, dim3(NT), 0, st, a);
        else if (a.M <= 16) hipLaunchKernelGGL(ensemble_kernel<16>, grid, dim3(NT), 0, st, a);
        else hipLaunchKernelGGL(ensemble_kernel<32>, grid, dim3(NT), 0, st, a);
        BF_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ensemble_finish_kernel, dim3((unsigned)a.frames), dim3(64), 0, st, a);
    BF_CHECK_LAUNCH();
    return 0;
}
}  // namespace

extern "C" int64_t bf_ensemble_scores_ws_bytes(int frames, int members, int H, int W) {
    if (!ens_sizes_ok(frames, members, H, W)) return 0;
    return ens_ws_bytes(frames, members, ens_rows(H, W));
}

extern "C" int bf_ensemble_scores(const float* members_ptr, int64_t member_stride, const float* target, int frames, int members, int H, int W, int fair,
                                  const bf_ensemble_rows* rows, void* ws, int64_t ws_bytes, bf_stream_t stream) {
    BF_REQUIRE(rows && rows->mean_rmse && rows->spread && rows->crps && members_ptr && target && ws, "bf_ensemble_scores: null pointer");
    BF_REQUIRE(ens_sizes_ok(frames, members, H, W) && member_stride >= (int64_t)frames * H * W,
               "bf_ensemble_scores: bad sizes (2 to 32 members, at least one frame of at least one pixel, member_stride >= frames * H * W)");
    BF_REQUIRE((uintptr_t)ws % 8 == 0 && ws_bytes >= bf_ensemble_scores_ws_bytes(frames, members, H, W),
               "bf_ensemble_scores: the workspace must be 8-byte aligned and hold bf_ensemble_scores_ws_bytes");
    EnsArgs a{};
    a.rollout = 0; a.x = members_ptr; a.member_stride = (long)member_stride; a.y = target; a.M = members; a.H = H; a.W = W; a.fair = fair != 0;
    a.frames = frames; a.T = 1; a.C = 1;
    a.vec_x = (W & 3) == 0 && (member_stride & 3) == 0 && (uintptr_t)members_ptr % 16 == 0;
    a.vec_y = (W & 3) == 0 && (uintptr_t)target % 16 == 0;
    return launch_ensemble(a, *rows, ws, (hipStream_t)stream);
}

extern "C" int bf_rollout_ensemble(const bf_rollout_step* s, int members, int fair, const bf_ensemble_rows* rows, void* ws, int64_t ws_bytes,
                                   bf_stream_t stream) {
    EnsArgs a{};
    if (const int rc = rollout_step_view(a.v, s, rows && rows->mean_rmse && rows->spread && rows->crps && ws,
                                         s && members >= 2 && members <= ENS_MAX_MEMBERS && s->B % members == 0 &&
                                             ens_sizes_ok((int64_t)(s->B / members) * s->T * s->C, members, s->Ho, s->Wo),
                                         "bf_rollout_ensemble: null pointer",
                                         "bf_rollout_ensemble: bad sizes (2 to 32 members, and the record's B a multiple of them)"))
        return rc;
    const RolloutStep& v = a.v;
    const int Bt = v.B / members;
    a.frames = Bt * v.T * v.C;
    BF_REQUIRE((uintptr_t)ws % 8 == 0 && ws_bytes >= bf_ensemble_scores_ws_bytes(a.frames, members, v.Ho, v.Wo),
               "bf_rollout_ensemble: the workspace must be 8-byte aligned and hold bf_ensemble_scores_ws_bytes(B / members * T * C, members, Ho, Wo)");
    a.rollout = 1; a.x = v.pred; a.member_stride = (long)a.frames * v.Ho * v.Wo; a.y = nullptr; a.M = members; a.H = v.Ho; a.W = v.Wo; a.fair = fair != 0;
    a.T = v.T; a.C = v.C;
    a.vec_x = (v.Wo & 3) == 0 && (uintptr_t)v.pred % 16 == 0;
    a.vec_y = v.Ho == v.H && v.Wo == v.W && (v.W & 3) == 0 && (uintptr_t)v.src % 16 == 0 && (v.field_stride & 3) == 0;
    return launch_ensemble(a, *rows, ws, (hipStream_t)stream);
}
