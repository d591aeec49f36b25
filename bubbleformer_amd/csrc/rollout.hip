// The per-step calls of a batched rollout, prediction against store-resident targets: rollout_score (advances the step counter) and
// rollout_heatflux (only reads it); the third, bf_rollout_bubbles, is in bubbles.hip beside the census it runs.  All three see the step
// through clip_store.h's RolloutStep: the same step number, the same frames.
#include "clip_store.h"
#include <algorithm>

namespace {
constexpr int NT = 256;

// ---------------------------------------------------------------------------- rollout scoring (one call per autoregressive step)
// Everything scripts/inference.py:230-266 and the rollout notebook report about one predicted clip, from ONE pass over the prediction:
// per (trajectory, frame, field) the relative L2 error against the simulation (utils/plot_utils.py:30-33), their mean (the LpLoss the script
// prints), the notebook's Eikonal score of the predicted and of the simulated signed-distance field, plus the two copies the loop needs (the
// next step's input and the archive row).  The target is never materialised: it is read where it lies in the store, through the gather's own
// index map and normalisation (nearest_src / clip_norm), so it has the bits bf_clip_gather returns.  The step number is read from DEVICE
// memory and incremented by the last launch, so a captured graph replays without new arguments.
// Pass 1: grid (rows, B*T*C); a workgroup sweeps a contiguous share of one (b, t, c) frame in 4-pixel groups of a row and leaves
// {sum (pred - y)^2, sum y^2, Eikonal sum of the prediction, of the target} in fp64.  Pass 2: one workgroup adds the rows of every frame in
// row order (no atomics: two runs give the same bits), takes quotient, root and means in fp64 and rounds once at the store.
struct ScoreArgs { RolloutStep v; int sdf; float inv_2dx; float* next_in; float* archive; double* part; int rows; };
constexpr int RS_QUADS = 1024, RS_MAX_ROWS = 64;      // 4-pixel groups per workgroup (4 per thread) until RS_MAX_ROWS workgroups share a frame
int score_rows(int Ho, int Wo) { return (int)std::max<long>(1, std::min<long>(RS_MAX_ROWS, ((long)Ho * ((Wo + 3) / 4) + RS_QUADS - 1) / RS_QUADS)); }

__global__ void __launch_bounds__(NT) rollout_score_kernel(ScoreArgs a) {
    __shared__ double red[NT / 64][4];      // several values at once in this kernel's own order, which its restatement's bits pin: not bf_common.h's block_reduce
    const RolloutStep& v = a.v;
    const int s = v.current();
    if (s < 0) return;                                                     // a step behind the last row: nothing is written (pass 2 leaves the counter alone)
    const int fc = blockIdx.y, H = v.H, W = v.W, Ho = v.Ho, Wo = v.Wo;     // fc = (b * T + t) * C + c
    const int c = fc % v.C, t = (fc / v.C) % v.T, b = fc / (v.C * v.T);
    const int wq = (Wo + 3) / 4, quads = Ho * wq, per = (quads + a.rows - 1) / a.rows;
    const int lo = blockIdx.x * per, hi = min(quads, lo + per);
    const float sy = v.sy(), sx = v.sx();
    const bool ident = v.ident();
    const float* tf = v.stored(c, v.frame(s, b, t));
    const long px = (long)Ho * Wo;
    const float* pf = v.predicted(fc / v.C, c);
    float* nf = a.next_in ? a.next_in + fc * px : nullptr;
    float* af = a.archive ? a.archive + (v.row(s, b, t) * v.C + c) * px : nullptr;
    const float d = v.diff[c], q = v.dv[c], inv_2dx = a.inv_2dx;
    const bool eik = c == a.sdf, vec_p = (Wo & 3) == 0, vec_t = ident && (W & 3) == 0;
    auto phi_at = [&](int yy, int xx) { return __fadd_rn(__fmul_rn(pf[yy * Wo + xx], q), d); };      // physical units, unfused: torch's pred * div + diff
    auto tgt_at = [&](int yy, int xx) { return tf[(long)nearest_src(yy, sy, H, ident) * W + nearest_src(xx, sx, W, ident)]; };
    double n2 = 0.0, y2 = 0.0, ep = 0.0, et = 0.0;
    for (int i = lo + threadIdx.x; i < hi; i += NT) {
        const int xq = i % wq, yo = i / wq, nv = min(4, Wo - 4 * xq);
        const float* row = tf + (long)nearest_src(yo, sy, H, ident) * W;
        const long o = (long)yo * Wo + 4 * xq;
        float p[4] = {0.f, 0.f, 0.f, 0.f}, y[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec_p) { const float4 v4 = *reinterpret_cast<const float4*>(pf + o); p[0] = v4.x; p[1] = v4.y; p[2] = v4.z; p[3] = v4.w; }
        else for (int j = 0; j < nv; ++j) p[j] = pf[o + j];
        if (vec_t) {
            const float4 v4 = *reinterpret_cast<const float4*>(row + 4 * xq);
            y[0] = clip_norm(v4.x, d, q); y[1] = clip_norm(v4.y, d, q); y[2] = clip_norm(v4.z, d, q); y[3] = clip_norm(v4.w, d, q);
        } else
            for (int j = 0; j < nv; ++j) y[j] = clip_norm(row[nearest_src(4 * xq + j, sx, W, ident)], d, q);
        for (int j = 0; j < nv; ++j) { const double yy = (double)y[j], e = (double)p[j] - yy; n2 += e * e; y2 += yy * yy; }
        if (eik)
            for (int j = 0; j < nv; ++j) {
                ep += (double)eikonal_l1_px(phi_at, 4 * xq + j, yo, Ho, Wo, inv_2dx);
                et += (double)eikonal_l1_px(tgt_at, 4 * xq + j, yo, Ho, Wo, inv_2dx);
            }
        if (vec_p) {
            const float4 v4 = make_float4(p[0], p[1], p[2], p[3]);
            if (nf) *reinterpret_cast<float4*>(nf + o) = v4;
            if (af) *reinterpret_cast<float4*>(af + o) = v4;
        } else
            for (int j = 0; j < nv; ++j) { if (nf) nf[o + j] = p[j]; if (af) af[o + j] = p[j]; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { n2 += __shfl_xor(n2, o, 64); y2 += __shfl_xor(y2, o, 64); ep += __shfl_xor(ep, o, 64); et += __shfl_xor(et, o, 64); }
    if ((threadIdx.x & 63) == 0) { double* r = red[threadIdx.x >> 6]; r[0] = n2; r[1] = y2; r[2] = ep; r[3] = et; }
    __syncthreads();
    if (threadIdx.x < 4) {
        double sum = 0.0;
        for (int w = 0; w < NT / 64; ++w) sum += red[w][threadIdx.x];
        a.part[((long)fc * a.rows + blockIdx.x) * 4 + threadIdx.x] = sum;
    }
}
// part [B*T*C][rows][4] -> rel_l2 [B][steps*T][C], criterion [B][steps], eik_pred / eik_tgt [B][steps*T] at the rows of step *step; then ++*step.
// ratio [B*T*C]: the fp64 quotients of this step, kept for the mean (LpLoss reduce_dims=[0, 1], reductions=["mean", "mean"]: over T, then over C)
__global__ void __launch_bounds__(NT) rollout_score_finish_kernel(const double* __restrict__ part, double* ratio, int* step, float* __restrict__ rel_l2,
                                                                 float* __restrict__ criterion, float* __restrict__ eik_pred, float* __restrict__ eik_tgt,
                                                                 int B, int T, int C, int steps, int rows, int sdf, double px) {
    const int s = *step;
    if (s < 0 || s >= steps) return;
    for (int fc = threadIdx.x; fc < B * T * C; fc += NT) {
        const int c = fc % C, t = (fc / C) % T, b = fc / (C * T);
        double n2 = 0.0, y2 = 0.0, ep = 0.0, et = 0.0;
        for (int r = 0; r < rows; ++r) { const double* q = part + ((long)fc * rows + r) * 4; n2 += q[0]; y2 += q[1]; ep += q[2]; et += q[3]; }
        const double rr = sqrt(n2 / y2);                                   // a target frame of zeros: inf or NaN, as torch.norm(a) / torch.norm(b) gives
        const long fr = ((long)b * steps + s) * T + t;
        ratio[fc] = rr;
        rel_l2[fr * C + c] = (float)rr;
        if (c == sdf) { eik_pred[fr] = (float)(ep / px); eik_tgt[fr] = (float)(et / px); }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += NT) {
        double m = 0.0;
        for (int c = 0; c < C; ++c) {
            double mc = 0.0;
            for (int t = 0; t < T; ++t) mc += ratio[((long)b * T + t) * C + c];
            m += mc / (double)T;
        }
        criterion[(long)b * steps + s] = (float)(m / (double)C);
    }
    __syncthreads();                                                       // every thread has read *step
    if (threadIdx.x == 0) *step = s + 1;
}


// ---------------------------------------------------------------------------- heat flux of a rollout step
// The reference's heat-flux evaluation inside a rollout (utils/heatflux.py per step of scripts/inference.py:239-252): heater_row_flux on row 0
// of the two fields of ONE rollout step, once on the prediction (de-normalised: fp32 multiply, then add, unfused) and once on the stored
// simulation frame (through nearest_src, the gather's own map).  A wave per (trajectory, frame, side).
struct HeatfluxArgs { RolloutStep v; int dfun_c, temp_c; const float* heater_temp; float x_min, dx, coef; float* flux_pred; float* flux_tgt; };

__global__ void __launch_bounds__(64) rollout_heatflux_kernel(HeatfluxArgs a) {
    const RolloutStep& v = a.v;
    const int s = v.current();
    if (s < 0) return;                                                     // behind the last row: nothing is written
    const int bt = blockIdx.x, t = bt % v.T, b = bt / v.T;
    const bool sim = blockIdx.y == 1;
    const float ht = a.heater_temp[b];
    float flux;
    if (sim) {
        const float sx = v.sx();
        const bool ident = v.ident();
        const long frame = v.frame(s, b, t), off = (long)nearest_src(0, v.sy(), v.H, ident) * v.W;
        const float* d = v.stored(a.dfun_c, frame) + off;
        const float* tp = v.stored(a.temp_c, frame) + off;
        flux = heater_row_flux([&](int x) { return d[nearest_src(x, sx, v.W, ident)]; }, [&](int x) { return tp[nearest_src(x, sx, v.W, ident)]; },
                               v.Wo, a.x_min, a.dx, ht, a.coef);
    } else {
        const float* d = v.predicted(bt, a.dfun_c);                        // row 0 of the frame: the heater row ([:, 0, :])
        const float* tp = v.predicted(bt, a.temp_c);
        const float dq = v.dv[a.dfun_c], dd = v.diff[a.dfun_c], tq = v.dv[a.temp_c], td = v.diff[a.temp_c];
        flux = heater_row_flux([&](int x) { return denormalise(d[x], dq, dd); }, [&](int x) { return denormalise(tp[x], tq, td); },
                               v.Wo, a.x_min, a.dx, ht, a.coef);
    }
    if (threadIdx.x == 0) (sim ? a.flux_tgt : a.flux_pred)[v.row(s, b, t)] = flux;
}
}  // namespace

extern "C" int64_t bf_rollout_score_ws_doubles(int B, int T, int C, int Ho, int Wo) {
    if (B <= 0 || T <= 0 || C <= 0 || Ho <= 0 || Wo <= 0) return 0;
    return (int64_t)B * T * C * (score_rows(Ho, Wo) * 4 + 1);
}
extern "C" int bf_rollout_score(const bf_rollout_step* s, int sdf_channel, float dx, float* rel_l2, float* criterion, float* eik_pred, float* eik_tgt,
                                float* next_in, float* archive, double* ws, int64_t ws_doubles, bf_stream_t stream) {
    ScoreArgs a;
    if (const int rc = rollout_step_view(a.v, s, rel_l2 && criterion && ws, s && (int64_t)s->B * s->T * s->C <= 65535, "bf_rollout_score: null pointer",
                                         "bf_rollout_score: bad sizes"))
        return rc;
    const int B = a.v.B, T = a.v.T, C = a.v.C, Ho = a.v.Ho, Wo = a.v.Wo;
    BF_REQUIRE(sdf_channel >= -1 && sdf_channel < C, "bf_rollout_score: the signed-distance channel is -1 (none) or an output channel");
    BF_REQUIRE(sdf_channel < 0 || (eik_pred && eik_tgt && Ho >= 3 && Wo >= 3 && dx > 0.f),
               "bf_rollout_score: the Eikonal rows need their outputs, dx > 0 and >= 3 points per axis (central differences)");
    BF_REQUIRE(a.v.pred != next_in && a.v.pred != archive, "bf_rollout_score: the copies cannot alias the prediction");
    BF_REQUIRE(((uintptr_t)a.v.pred % 16 == 0) && ((uintptr_t)a.v.src % 16 == 0) && ((uintptr_t)next_in % 16 == 0) && ((uintptr_t)archive % 16 == 0) &&
               ((uintptr_t)ws % 8 == 0), "bf_rollout_score: prediction, frames and copies must be 16-byte aligned");
    BF_REQUIRE(ws_doubles >= bf_rollout_score_ws_doubles(B, T, C, Ho, Wo), "bf_rollout_score: workspace smaller than bf_rollout_score_ws_doubles");
    const int rows = score_rows(Ho, Wo);
    double* ratio = ws + (long)B * T * C * rows * 4;
    a.sdf = sdf_channel; a.inv_2dx = sdf_channel >= 0 ? 0.5f / dx : 0.f; a.next_in = next_in; a.archive = archive; a.part = ws; a.rows = rows;
    hipLaunchKernelGGL(rollout_score_kernel, dim3((unsigned)rows, (unsigned)(B * T * C)), dim3(NT), 0, (hipStream_t)stream, a);
    BF_CHECK_LAUNCH();
    hipLaunchKernelGGL(rollout_score_finish_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, (const double*)ws, ratio, (int*)s->step, rel_l2, criterion,
                       eik_pred, eik_tgt, B, T, C, a.v.steps, rows, sdf_channel, (double)Ho * (double)Wo);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_rollout_heatflux(const bf_rollout_step* s, int dfun_channel, int temp_channel, const float* heater_temp, float x_min, float dx, float lc,
                                   float conductivity, float* flux_pred, float* flux_tgt, bf_stream_t stream) {
    HeatfluxArgs a;
    if (const int rc = rollout_step_view(a.v, s, heater_temp && flux_pred && flux_tgt, s && (int64_t)s->B * s->T <= 0x7fffffff,
                                         "bf_rollout_heatflux: null pointer", "bf_rollout_heatflux: bad sizes"))
        return rc;
    const int C = a.v.C;
    BF_REQUIRE(dfun_channel >= 0 && dfun_channel < C && temp_channel >= 0 && temp_channel < C,
               "bf_rollout_heatflux: the signed-distance and the temperature channel must be output channels");
    BF_REQUIRE(dx > 0.f && lc > 0.f, "bf_rollout_heatflux: dx and lc must be positive");
    a.dfun_c = dfun_channel; a.temp_c = temp_channel; a.heater_temp = heater_temp; a.x_min = x_min; a.dx = dx; a.coef = conductivity / (dx * lc);
    a.flux_pred = flux_pred; a.flux_tgt = flux_tgt;
    hipLaunchKernelGGL(rollout_heatflux_kernel, dim3((unsigned)(a.v.B * a.v.T), 2), dim3(64), 0, (hipStream_t)stream, a);
    BF_CHECK_LAUNCH();
    return 0;
}
