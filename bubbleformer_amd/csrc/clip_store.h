// Device-side facts about the device clip store ([fields][total_frames][H][W] fp32 trajectories resident in HBM) that more than one
// translation unit relies on, one definition each: the gather's index map and normalisation (clip_store.hip, and every rollout kernel that
// builds its target on the fly, so that it has the bits a gathered clip has), the physical-units view of a prediction, the per-pixel and
// per-row expressions of the physics metrics (physics.hip on a clip, rollout.hip on a rollout step), and the view of "this step's
// prediction and its target frames in the store" that the three per-step rollout calls (rollout.hip, bubbles.hip) share.
#pragma once
#include "bf_common.h"

// Source index of F.interpolate(mode="nearest"): floor(dst * float(in / out)) clamped to in - 1 (identity at full resolution)
__device__ __forceinline__ int nearest_src(int dst, float scale, int n, bool ident) { return ident ? dst : min((int)floorf((float)dst * scale), n - 1); }

// (stored value - diff) / div: a clip as the dataset normalises it
__device__ __forceinline__ float clip_norm(float v, float d, float q) { return (v - d) / q; }

// pred * div + diff as torch forms it: an fp32 product, rounded, then an fp32 sum (contraction off: never one fused operation).  The physical
// field the rollout's heat-flux rows and bubble census see
__device__ __forceinline__ float denormalise(float v, float q, float d) {
#pragma clang fp contract(off)
    const float prod = v * q;
    return prod + d;
}

// What the batch gathers pass their kernels by value, for the fp32 store (clip_store.hip) and the 16-bit one (clip_store_q16.hip): one clip
// segment of a sample -- its channels' field ids and constants, its output, its frame count and first frame behind the sample's first --
// and the seeded mirror / window draw
struct ClipSeg { const int* field; const float* diff; const float* dv; float* out; int T, C, t0; };
struct ClipAugment { const int* odd_a; const int* odd_b; uint32_t k0, k1, draw; unsigned long long thr; int Hc, Wc, random_y, eval_view; };

// | |grad phi| - 1 | at pixel (x, y) of an H x W frame read through at(row, column): central differences, replicate-padded borders
template <class At>
__device__ __forceinline__ float eikonal_l1_px(At at, int x, int y, int H, int W, float inv_2dx) {
    const int xi = min(max(x, 1), W - 2), yi = min(max(y, 1), H - 2);
    const float gx = (at(y, xi + 1) - at(y, xi - 1)) * inv_2dx;
    const float gy = (at(yi + 1, x) - at(yi - 1, x)) * inv_2dx;
    return fabsf(sqrtf(gx * gx + gy * gy) - 1.f);
}

// Heater heat flux of FC-72 pool boiling from one heater row (utils/heatflux.py:17-38): W columns spanning x in [x_min, x_min + W*dx),
// mean_x( [ |x| <= 5 and dfun < 0 ] * (heater_temp - temp) ) * coef.  ONE WAVE calls this; dfun_at / temp_at give the value at column x.
// 64 lanes stride over the row, cell centres and the sum in fp64, one rounding.  Every lane returns the flux.
template <class DfunAt, class TempAt>
__device__ __forceinline__ float heater_row_flux(DfunAt dfun_at, TempAt temp_at, int W, float x_min, float dx, float heater_temp, float coef) {
    double acc = 0.0;
    for (int x = threadIdx.x; x < W; x += 64) {
        const double xc = (double)x_min + ((double)x + 0.5) * (double)dx;
        if (xc >= -5.0 && xc <= 5.0 && dfun_at(x) < 0.f) acc += (double)(heater_temp - temp_at(x));
    }
    return (float)(wave_sum(acc) / (double)W * (double)coef);
}

// ---------------------------------------------------------------------------- one step of a batched rollout
// The prediction (B, T, C, Ho, Wo) of rollout step s and its targets, the stored frames first[b] + (s + 1) * T + t, which are never
// materialised: every per-step kernel reads them where they lie, through these accessors, so all three report on the same frame.  s is read
// from DEVICE memory (a captured graph replays without new arguments).
struct RolloutStep {
    const float* pred; const float* src; long field_stride, total_frames; int nfields;
    const long* first; const int* step; const int* field; const float* diff; const float* dv;
    int B, T, C, H, W, Ho, Wo, steps;
    // the step this launch serves; -1 behind the last row, where a kernel writes nothing
    __device__ __forceinline__ int current() const { const int s = *step; return s < 0 || s >= steps ? -1 : s; }
    // the stored frame (b, t) is scored against, and that frame of output channel c: a start or a field id outside the store reads a valid one
    __device__ __forceinline__ long frame(int s, int b, int t) const { return min(max(first[b] + (long)(s + 1) * T + t, 0L), total_frames - 1); }
    __device__ __forceinline__ const float* stored(int c, long fr) const { return src + (long)min(max(field[c], 0), nfields - 1) * field_stride + fr * H * (long)W; }
    // channel c of prediction frame bt = b * T + t; the row of (b, t) in a (B, steps * T, ...) report
    __device__ __forceinline__ const float* predicted(long bt, int c) const { return pred + (bt * C + c) * ((long)Ho * Wo); }
    __device__ __forceinline__ long row(int s, int b, int t) const { return ((long)b * steps + s) * T + t; }
    // the downsampling map of the store onto the prediction's grid, for nearest_src
    __device__ __forceinline__ float sy() const { return (float)H / (float)Ho; }
    __device__ __forceinline__ float sx() const { return (float)W / (float)Wo; }
    __device__ __forceinline__ bool ident() const { return Ho == H && Wo == W; }
};

// The device view of an entry point's bf_rollout_step, after the null and size checks every per-step call makes; own_ptrs / own_sizes are the entry
// point's additions to them (a null record fails the first, so own_sizes may be `s && ...`)
inline int rollout_step_view(RolloutStep& v, const bf_rollout_step* s, bool own_ptrs, bool own_sizes, const char* null_msg, const char* size_msg) {
    BF_REQUIRE(s && s->pred && s->frames && s->first && s->step && s->field && s->diff && s->div && own_ptrs, null_msg);
    BF_REQUIRE(s->B > 0 && s->T > 0 && s->C > 0 && s->H > 0 && s->W > 0 && s->Ho > 0 && s->Wo > 0 && s->Ho <= s->H && s->Wo <= s->W && s->steps > 0 &&
               s->nfields > 0 && s->total_frames > 0 && s->field_stride >= s->total_frames * s->H * s->W && own_sizes, size_msg);
    v = RolloutStep{s->pred, s->frames, (long)s->field_stride, (long)s->total_frames, s->nfields, (const long*)s->first, s->step, s->field, s->diff, s->div,
                    s->B, s->T, s->C, s->H, s->W, s->Ho, s->Wo, s->steps};
    return 0;
}
