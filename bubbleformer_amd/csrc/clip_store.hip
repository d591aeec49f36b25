// The device clip store, trajectories resident in HBM as [fields][total_frames][H][W] fp32: the clip gather of a batch and the dataset's
// field statistics.  The index map and the normalisation are clip_store.h's: the rollout kernels build their targets through the same two.
#include "clip_store.h"
#include "philox.h"
#include <algorithm>

namespace {
constexpr int NT = 256;
int grid_for(long total) { return (int)std::max<long>(1, std::min<long>((total + NT - 1) / NT, 256L * 16)); }
// output pixels 4 xq .. 4 xq + 3 of a row: dst[j] = clip_norm(row[xs(4 xq + j)]), one 16-byte load and store at full resolution
__device__ __forceinline__ void gather_quad(const float* row, float* dst, int xq, float d, float q, float sx, int W, int Wo, bool ident) {
    if (ident && (W & 3) == 0) {
        const float4 v = *reinterpret_cast<const float4*>(row + 4 * xq);
        *reinterpret_cast<float4*>(dst) = make_float4(clip_norm(v.x, d, q), clip_norm(v.y, d, q), clip_norm(v.z, d, q), clip_norm(v.w, d, q));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xo = 4 * xq + j;
            if (xo < Wo) dst[j] = clip_norm(row[nearest_src(xo, sx, W, ident)], d, q);
        }
    }
}
}  // namespace

// ---------------------------------------------------------------------------- clip gather (device-resident trajectories -> batch)
// out[b][t][c][yo][xo] = (src[field[c]][first[b] + t0 + t][ys(yo)][xs(xo)] - diff[c]) / div[c]
// ys / xs: identity, or torch's F.interpolate(mode="nearest") source index floor(dst * float(in / out)) clamped to in - 1
// (bubbleformer/data/dataset.py:138-148).  One thread per 4 output pixels of a row; reads of a full-resolution row are 16-byte.
__global__ void __launch_bounds__(NT) clip_gather_kernel(const float* __restrict__ src, long field_stride, const int* __restrict__ field,
                                                        const long* __restrict__ first, int t0, const float* __restrict__ diff,
                                                        const float* __restrict__ dv, float* __restrict__ out, int B, int T, int C, int H, int W,
                                                        int Ho, int Wo) {
    const int wq = (Wo + 3) / 4;
    const long total = (long)B * T * C * Ho * wq;
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    const bool ident = Ho == H && Wo == W;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int xq = (int)(i % wq);
        long r = i / wq;
        const int yo = (int)(r % Ho); r /= Ho;
        const int c = (int)(r % C); r /= C;
        const int t = (int)(r % T);
        const int b = (int)(r / T);
        const int ys = nearest_src(yo, sy, H, ident);
        const float* row = src + (long)field[c] * field_stride + ((first[b] + t0 + t) * H + ys) * (long)W;
        float* dst = out + ((((long)b * T + t) * C + c) * Ho + yo) * (long)Wo + 4 * xq;
        const float d = diff[c], q = dv[c];
        gather_quad(row, dst, xq, d, q, sx, W, Wo, ident);
    }
}

extern "C" int bf_clip_gather(const float* src, int64_t field_stride, const int32_t* field, const int64_t* first, int t0,
                              const float* diff, const float* div, float* out, int B, int T, int C, int H, int W, int Ho, int Wo,
                              bf_stream_t stream) {
    BF_REQUIRE(src && field && first && diff && div && out, "bf_clip_gather: null pointer");
    BF_REQUIRE(B > 0 && T > 0 && C > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && Ho <= H && Wo <= W && t0 >= 0, "bf_clip_gather: bad sizes");
    BF_REQUIRE(((uintptr_t)src % 16 == 0) && ((uintptr_t)out % 16 == 0), "bf_clip_gather: buffers must be 16-byte aligned");
    const long total = (long)B * T * C * Ho * ((Wo + 3) / 4);
    hipLaunchKernelGGL(clip_gather_kernel, dim3(grid_for(total)), dim3(NT), 0, (hipStream_t)stream, src, (long)field_stride, (const int*)field,
                       (const long*)first, t0, diff, div, out, B, T, C, H, W, Ho, Wo);
    BF_CHECK_LAUNCH();
    return 0;
}

// A training batch in ONE launch: the input clips (frames first .. first + Tin - 1), the target clips (the Tout frames behind them) and the
// per-sample fluid-parameter rows, all indexed by SAMPLE number on the device (first_tab / file_tab: absolute first frame and file of every
// sample of the dataset) -- what took two launches and three index kernels of the host framework (first_tab[idx], file_tab[idx], fluid[...]).
__global__ void __launch_bounds__(NT) clip_gather_batch_kernel(const float* __restrict__ src, long field_stride, const long* __restrict__ idx, long nsamples,
                                                              const long* __restrict__ first_tab, ClipSeg a, ClipSeg b,
                                                              const float* __restrict__ fluid_tab, const long* __restrict__ file_tab, int P,
                                                              float* __restrict__ fluid_out, int B, int H, int W, int Ho, int Wo) {
    const int wq = (Wo + 3) / 4;
    const long per_a = (long)a.T * a.C * Ho * wq, per_b = (long)b.T * b.C * Ho * wq, per = per_a + per_b;
    const long total = (long)B * per;
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    const bool ident = Ho == H && Wo == W;
    if (fluid_out && blockIdx.x == 0)
        for (int i = threadIdx.x; i < B * P; i += NT) fluid_out[i] = fluid_tab[file_tab[min(max(idx[i / P], 0L), nsamples - 1)] * P + i % P];
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int bb = (int)(i / per);
        long r = i - (long)bb * per;
        const bool second = r >= per_a;
        if (second) r -= per_a;
        const ClipSeg& sg = second ? b : a;
        const int xq = (int)(r % wq); r /= wq;
        const int yo = (int)(r % Ho); r /= Ho;
        const int c = (int)(r % sg.C);
        const int t = (int)(r / sg.C);
        const int ys = nearest_src(yo, sy, H, ident);
        const long smp = min(max(idx[bb], 0L), nsamples - 1);      // an index out of range reads a valid sample, never past a table
        const float* row = src + (long)sg.field[c] * field_stride + ((first_tab[smp] + sg.t0 + t) * H + ys) * (long)W;
        float* dst = sg.out + ((((long)bb * sg.T + t) * sg.C + c) * Ho + yo) * (long)Wo + 4 * xq;
        const float d = sg.diff[c], q = sg.dv[c];
        gather_quad(row, dst, xq, d, q, sx, W, Wo, ident);
    }
}
// Its sibling for a training step unrolled through its own predictions: segment b holds `unroll` consecutive target clips of Tc = b.T / unroll
// frames each, written as (unroll, B, Tc, C, Ho, Wo) so that every clip is contiguous (one per pass).  The same index map and normalisation;
// a frame index is held below `nframes`, so that a device-side sample number whose later clips lie behind its file (the host path refuses
// those) reads the frames that follow on the store's frame axis -- the next file's -- and the store's last frame where the store ends,
// never past it.  A kernel of its own: sharing one body through a template made the compiler
// address the single-clip kernel's two segments differently (18 more instructions), and that one runs in every training step.
__global__ void __launch_bounds__(NT) clip_gather_unroll_kernel(const float* __restrict__ src, long field_stride, const long* __restrict__ idx, long nsamples,
                                                               const long* __restrict__ first_tab, ClipSeg a, ClipSeg b,
                                                               const float* __restrict__ fluid_tab, const long* __restrict__ file_tab, int P,
                                                               float* __restrict__ fluid_out, int B, int H, int W, int Ho, int Wo, int unroll, long nframes) {
    const int wq = (Wo + 3) / 4;
    const long per_a = (long)a.T * a.C * Ho * wq, per_b = (long)b.T * b.C * Ho * wq, per = per_a + per_b;
    const long total = (long)B * per;
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    const bool ident = Ho == H && Wo == W;
    const int Tc = b.T / unroll;
    if (fluid_out && blockIdx.x == 0)
        for (int i = threadIdx.x; i < B * P; i += NT) fluid_out[i] = fluid_tab[file_tab[min(max(idx[i / P], 0L), nsamples - 1)] * P + i % P];
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int bb = (int)(i / per);
        long r = i - (long)bb * per;
        const bool second = r >= per_a;
        if (second) r -= per_a;
        const ClipSeg& sg = second ? b : a;
        const int xq = (int)(r % wq); r /= wq;
        const int yo = (int)(r % Ho); r /= Ho;
        const int c = (int)(r % sg.C);
        const int t = (int)(r / sg.C);
        const int ys = nearest_src(yo, sy, H, ident);
        const long smp = min(max(idx[bb], 0L), nsamples - 1);
        const long frame = min(first_tab[smp] + sg.t0 + t, nframes - 1);
        const int j = second ? t / Tc : 0;
        const long orow = second ? ((long)j * B + bb) * Tc + (t - j * Tc) : (long)bb * sg.T + t;      // (unroll, B, Tc, ..) row (j, b, t'), or (B, T, ..) row (b, t)
        const float* row = src + (long)sg.field[c] * field_stride + (frame * H + ys) * (long)W;
        float* dst = sg.out + ((orow * sg.C + c) * Ho + yo) * (long)Wo + 4 * xq;
        const float d = sg.diff[c], q = sg.dv[c];
        gather_quad(row, dst, xq, d, q, sx, W, Wo, ident);
    }
}
// The unroll kernel's batch with a seeded mirror in x and a seeded Hc x Wc window per SAMPLE (unroll >= 1, the unroll
// kernel's output layout and frame clamp).  Everything is defined on the output grid, after the nearest-neighbour map:
//   out[c][t][y][x] = clip_norm(s_c * raw(c, t, y0 + y, xs), diff_c, div_c),  xs = x0 + x, or x0 + Wc - 1 - x when the sample is mirrored
//   s_c = -1 iff the sample is mirrored and odd[c] != 0 (a field that changes sign under x -> -x, velx): the sign goes on the STORED value
// One Philox4x32-10 block per sample (philox.h), key = the seed, counter {0xFFFFFFFF, low 32 bits of the clamped idx[b], draw, 0} -- word 0 of
// bf_clip_noise's counter is a group number < 2^29, so under one seed the two never share a block:
//   mirrored iff w0 < thr (thr = round(flip_p 2^32), 0 .. 2^32);  x0 = (w1 (Wo - Wc + 1)) >> 32;  y0 = (w2 (Ho - Hc + 1)) >> 32 or 0 (crop_y)
// eval_view: no block is drawn -- never mirrored, x0 = (Wo - Wc) / 2, y0 = 0.  The input clip, every target clip and all their frames share
// the sample's decision; the fluid row is the plain one.
// Samples lie on the grid's y axis: the block is computed ONCE per thread and sample, in front of that sample's pixel loop (it depends on
// nothing a lane owns, so the compiler may hold it in scalar registers), never per pixel, and no second launch or buffer is involved.
// A thread serves 4 output pixels of a row.  16-byte loads and stores when the map is the identity and W, Wc and x0 are multiples of 4
// (a mirrored quad is then one aligned quad read back to front); scalar loads otherwise (an odd origin, a ragged window, a downsampled
// store), still with one 16-byte store per quad when Wc is a multiple of 4.  A kernel of its own, as clip_gather_unroll_kernel is and for its reason.
__global__ void __launch_bounds__(NT) clip_gather_augment_kernel(const float* __restrict__ src, long field_stride, const long* __restrict__ idx, long nsamples,
                                                                const long* __restrict__ first_tab, ClipSeg a, ClipSeg b,
                                                                const float* __restrict__ fluid_tab, const long* __restrict__ file_tab, int P,
                                                                float* __restrict__ fluid_out, int B, int H, int W, int Ho, int Wo, int unroll, long nframes,
                                                                ClipAugment g) {
    const int Hc = g.Hc, Wc = g.Wc;
    const int wq = (Wc + 3) / 4;
    const long per_a = (long)a.T * a.C * Hc * wq, per_b = (long)b.T * b.C * Hc * wq, per = per_a + per_b;
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    const bool ident = Ho == H && Wo == W;
    const int Tc = b.T / unroll;
    if (fluid_out && blockIdx.x == 0 && blockIdx.y == 0)
        for (int i = threadIdx.x; i < B * P; i += NT) fluid_out[i] = fluid_tab[file_tab[min(max(idx[i / P], 0L), nsamples - 1)] * P + i % P];
    for (int bb = blockIdx.y; bb < B; bb += gridDim.y) {
        const long smp = min(max(idx[bb], 0L), nsamples - 1);
        bool flip = false;
        int x0 = (Wo - Wc) / 2, y0 = 0;
        if (!g.eval_view) {
            const Quad q = philox4x32_10(0xFFFFFFFFu, (uint32_t)(unsigned long)smp, g.draw, 0u, g.k0, g.k1);
            flip = (unsigned long long)q.w[0] < g.thr;
            x0 = (int)(((unsigned long long)q.w[1] * (unsigned long long)(Wo - Wc + 1)) >> 32);
            y0 = g.random_y ? (int)(((unsigned long long)q.w[2] * (unsigned long long)(Ho - Hc + 1)) >> 32) : 0;
        }
        const long first = first_tab[smp];
        const bool vec = ident && ((W | Wc | x0) & 3) == 0;
        for (long r0 = (long)blockIdx.x * NT + threadIdx.x; r0 < per; r0 += (long)gridDim.x * NT) {
            long r = r0;
            const bool second = r >= per_a;
            if (second) r -= per_a;
            const ClipSeg& sg = second ? b : a;
            const int xq = (int)(r % wq); r /= wq;
            const int y = (int)(r % Hc); r /= Hc;
            const int c = (int)(r % sg.C);
            const int t = (int)(r / sg.C);
            const int ys = nearest_src(y0 + y, sy, H, ident);
            const long frame = min(first + sg.t0 + t, nframes - 1);
            const int j = second ? t / Tc : 0;
            const long orow = second ? ((long)j * B + bb) * Tc + (t - j * Tc) : (long)bb * sg.T + t;      // as the unroll kernel lays its rows out
            const float* row = src + (long)sg.field[c] * field_stride + (frame * H + ys) * (long)W;
            float* dst = sg.out + ((orow * sg.C + c) * Hc + y) * (long)Wc + 4 * xq;
            const float d = sg.diff[c], q = sg.dv[c];
            const bool neg = flip && (second ? g.odd_b : g.odd_a)[c] != 0;
            if (vec) {                                                  // 4 xq + 3 < Wc: the window is whole quads
                const float4 v = *reinterpret_cast<const float4*>(row + (flip ? x0 + Wc - 4 - 4 * xq : x0 + 4 * xq));
                const float e0 = flip ? v.w : v.x, e1 = flip ? v.z : v.y, e2 = flip ? v.y : v.z, e3 = flip ? v.x : v.w;
                *reinterpret_cast<float4*>(dst) = make_float4(clip_norm(neg ? -e0 : e0, d, q), clip_norm(neg ? -e1 : e1, d, q),
                                                              clip_norm(neg ? -e2 : e2, d, q), clip_norm(neg ? -e3 : e3, d, q));
            } else if ((Wc & 3) == 0) {                                 // whole quads at an origin or through a map that is not aligned: scalar loads, one 16-byte store
                float o[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int x = 4 * xq + k;
                    const float v = row[nearest_src(flip ? x0 + Wc - 1 - x : x0 + x, sx, W, ident)];
                    o[k] = clip_norm(neg ? -v : v, d, q);
                }
                *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int x = 4 * xq + k;
                    if (x < Wc) {
                        const float v = row[nearest_src(flip ? x0 + Wc - 1 - x : x0 + x, sx, W, ident)];
                        dst[k] = clip_norm(neg ? -v : v, d, q);
                    }
                }
            }
        }
    }
}
extern "C" int bf_clip_gather_batch(const float* src, int64_t field_stride, const int64_t* idx, int64_t nsamples, const int64_t* first_tab, const int32_t* in_field,
                                    const float* in_diff, const float* in_div, int Cin, int Tin, float* in_out, const int32_t* out_field,
                                    const float* out_diff, const float* out_div, int Cout, int Tout, float* out_out, const float* fluid_tab,
                                    const int64_t* file_tab, int P, float* fluid_out, int B, int H, int W, int Ho, int Wo, bf_stream_t stream) {
    BF_REQUIRE(src && idx && first_tab && in_field && in_diff && in_div && in_out && out_field && out_diff && out_div && out_out,
               "bf_clip_gather_batch: null pointer");
    BF_REQUIRE(nsamples > 0 && B > 0 && Tin > 0 && Tout > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && Ho <= H && Wo <= W, "bf_clip_gather_batch: bad sizes");
    BF_REQUIRE(!fluid_out || (fluid_tab && file_tab && P > 0), "bf_clip_gather_batch: the fluid rows need their table, the file table and P > 0");
    BF_REQUIRE(((uintptr_t)src % 16 == 0) && ((uintptr_t)in_out % 16 == 0) && ((uintptr_t)out_out % 16 == 0), "bf_clip_gather_batch: buffers must be 16-byte aligned");
    const ClipSeg a{(const int*)in_field, in_diff, in_div, in_out, Tin, Cin, 0}, b{(const int*)out_field, out_diff, out_div, out_out, Tout, Cout, Tin};
    const long total = (long)B * ((long)Tin * Cin + (long)Tout * Cout) * Ho * ((Wo + 3) / 4);
    hipLaunchKernelGGL(clip_gather_batch_kernel, dim3(grid_for(total)), dim3(NT), 0, (hipStream_t)stream, src, (long)field_stride, (const long*)idx, (long)nsamples,
                       (const long*)first_tab, a, b, fluid_tab, (const long*)file_tab, P, fluid_out, B, H, W, Ho, Wo);
    BF_CHECK_LAUNCH();
    return 0;
}

// ... and with `unroll` target clips behind the input clip, out_out (unroll, B, Tout, Cout, Ho, Wo): clip j = frames first + Tin + j * Tout ..
extern "C" int bf_clip_gather_unroll(const float* src, int64_t field_stride, int64_t nframes, const int64_t* idx, int64_t nsamples, const int64_t* first_tab,
                                     const int32_t* in_field, const float* in_diff, const float* in_div, int Cin, int Tin, float* in_out,
                                     const int32_t* out_field, const float* out_diff, const float* out_div, int Cout, int Tout, int unroll, float* out_out,
                                     const float* fluid_tab, const int64_t* file_tab, int P, float* fluid_out, int B, int H, int W, int Ho, int Wo,
                                     bf_stream_t stream) {
    BF_REQUIRE(src && idx && first_tab && in_field && in_diff && in_div && in_out && out_field && out_diff && out_div && out_out,
               "bf_clip_gather_unroll: null pointer");
    BF_REQUIRE(nsamples > 0 && B > 0 && Tin > 0 && Tout > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && Ho <= H && Wo <= W, "bf_clip_gather_unroll: bad sizes");
    BF_REQUIRE(unroll >= 1 && unroll <= 1024 && nframes > 0 && field_stride >= nframes * (int64_t)H * W, "bf_clip_gather_unroll: bad unroll count or frame count");
    BF_REQUIRE(!fluid_out || (fluid_tab && file_tab && P > 0), "bf_clip_gather_unroll: the fluid rows need their table, the file table and P > 0");
    BF_REQUIRE(((uintptr_t)src % 16 == 0) && ((uintptr_t)in_out % 16 == 0) && ((uintptr_t)out_out % 16 == 0), "bf_clip_gather_unroll: buffers must be 16-byte aligned");
    const ClipSeg a{(const int*)in_field, in_diff, in_div, in_out, Tin, Cin, 0}, b{(const int*)out_field, out_diff, out_div, out_out, unroll * Tout, Cout, Tin};
    const long total = (long)B * ((long)Tin * Cin + (long)unroll * Tout * Cout) * Ho * ((Wo + 3) / 4);
    hipLaunchKernelGGL(clip_gather_unroll_kernel, dim3(grid_for(total)), dim3(NT), 0, (hipStream_t)stream, src, (long)field_stride, (const long*)idx, (long)nsamples,
                       (const long*)first_tab, a, b, fluid_tab, (const long*)file_tab, P, fluid_out, B, H, W, Ho, Wo, unroll, (long)nframes);
    BF_CHECK_LAUNCH();
    return 0;
}

// ... and with the seeded mirror and window of clip_gather_augment_kernel: bf_clip_gather_unroll's job as a record, and the draw as another
extern "C" int bf_clip_gather_augment(const bf_clip_gather_job* j, const bf_clip_augment* g, bf_stream_t stream) {
    BF_REQUIRE(j && g && j->src && j->idx && j->first_tab && j->in_field && j->in_diff && j->in_div && j->in_out && j->out_field && j->out_diff && j->out_div &&
               j->out_out && g->in_odd && g->out_odd, "bf_clip_gather_augment: null pointer");
    BF_REQUIRE(j->nsamples > 0 && j->B > 0 && j->Tin > 0 && j->Tout > 0 && j->Cin > 0 && j->Cout > 0 && j->H > 0 && j->W > 0 && j->Ho > 0 && j->Wo > 0 &&
               j->Ho <= j->H && j->Wo <= j->W, "bf_clip_gather_augment: bad sizes");
    BF_REQUIRE(j->unroll >= 1 && j->unroll <= 1024 && j->nframes > 0 && j->field_stride >= j->nframes * (int64_t)j->H * j->W,
               "bf_clip_gather_augment: bad unroll count or frame count");
    BF_REQUIRE(!j->fluid_out || (j->fluid_tab && j->file_tab && j->P > 0), "bf_clip_gather_augment: the fluid rows need their table, the file table and P > 0");
    BF_REQUIRE(((uintptr_t)j->src % 16 == 0) && ((uintptr_t)j->in_out % 16 == 0) && ((uintptr_t)j->out_out % 16 == 0),
               "bf_clip_gather_augment: buffers must be 16-byte aligned");
    BF_REQUIRE(g->Hc >= 1 && g->Hc <= j->Ho && g->Wc >= 1 && g->Wc <= j->Wo, "bf_clip_gather_augment: the window must be 1 .. Ho by 1 .. Wo");
    BF_REQUIRE(g->flip_thr >= 0 && g->flip_thr <= (1LL << 32) && (g->crop_y == 0 || g->crop_y == 1) && (g->eval_view == 0 || g->eval_view == 1),
               "bf_clip_gather_augment: bad flip threshold, crop_y or eval_view");
    const ClipSeg a{(const int*)j->in_field, j->in_diff, j->in_div, j->in_out, j->Tin, j->Cin, 0};
    const ClipSeg b{(const int*)j->out_field, j->out_diff, j->out_div, j->out_out, j->unroll * j->Tout, j->Cout, j->Tin};
    const ClipAugment aug{(const int*)g->in_odd, (const int*)g->out_odd, (uint32_t)(uint64_t)g->seed, (uint32_t)((uint64_t)g->seed >> 32), (uint32_t)g->draw,
                          (unsigned long long)g->flip_thr, g->Hc, g->Wc, g->crop_y, g->eval_view};
    const long per = ((long)j->Tin * j->Cin + (long)j->unroll * j->Tout * j->Cout) * g->Hc * ((g->Wc + 3) / 4);
    const int gy = std::min(j->B, 65535);
    const int gx = (int)std::max<long>(1, std::min<long>((per + NT - 1) / NT, std::max(1, 256 * 16 / gy)));
    hipLaunchKernelGGL(clip_gather_augment_kernel, dim3(gx, gy), dim3(NT), 0, (hipStream_t)stream, j->src, (long)j->field_stride, (const long*)j->idx,
                       (long)j->nsamples, (const long*)j->first_tab, a, b, j->fluid_tab, (const long*)j->file_tab, j->P, j->fluid_out, j->B, j->H, j->W, j->Ho,
                       j->Wo, j->unroll, (long)j->nframes, aug);
    BF_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------- field statistics of device-resident trajectories
// The normalisation constants of the dataset (bubbleformer/data/dataset.py:74-117: mean / std / min / max of every full field of every file,
// which the reference reads through h5py and reduces on the host) from the trajectories ALREADY resident in HBM: one launch over all
// (field, file) segments.  Pass 1: every workgroup sweeps a contiguous share of one segment (16-byte loads) and leaves {sum, sum of squares,
// min, max} in fp64; pass 2: one wave per segment adds the workgroup rows in row order (bit-reproducible; no atomics).
constexpr int FS_ROWS = 64;      // workgroups per segment
__global__ void __launch_bounds__(NT) field_stats_kernel(const float* __restrict__ src, const long* __restrict__ seg_begin, const long* __restrict__ seg_len,
                                                        double* __restrict__ part) {
    __shared__ double red[NT / 64][4];      // several values at once in this kernel's own order, which its restatement's bits pin: not bf_common.h's block_reduce
    const int seg = blockIdx.y;
    const float* p = src + seg_begin[seg];
    const long n = seg_len[seg];
    const long per = ((n + FS_ROWS - 1) / FS_ROWS + 3) & ~3L;                      // a multiple of 4 floats: whole 16-byte groups when the segment is aligned
    const long lo = (long)blockIdx.x * per, hi = min(n, lo + per);
    double s1 = 0.0, s2 = 0.0, mn = 1.0 / 0.0, mx = -1.0 / 0.0;
    auto take = [&](float v) { const double d = (double)v; s1 += d; s2 += d * d; mn = fmin(mn, d); mx = fmax(mx, d); };
    const bool vec = (((uintptr_t)p) & 15) == 0;
    long i = lo + 4L * threadIdx.x;
    if (vec)
        for (; i + 3 < hi; i += 4L * NT) { const float4 v = *reinterpret_cast<const float4*>(p + i); take(v.x); take(v.y); take(v.z); take(v.w); }
    else
        for (; i + 3 < hi; i += 4L * NT) { take(p[i]); take(p[i + 1]); take(p[i + 2]); take(p[i + 3]); }
    for (long j = i; j < hi && j < i + 4; ++j) take(p[j]);                            // the share's ragged end (at most one thread has one)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); mn = fmin(mn, __shfl_xor(mn, o, 64)); mx = fmax(mx, __shfl_xor(mx, o, 64)); }
    if ((threadIdx.x & 63) == 0) { double* r = red[threadIdx.x >> 6]; r[0] = s1; r[1] = s2; r[2] = mn; r[3] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0, c = 1.0 / 0.0, e = -1.0 / 0.0;
        for (int w = 0; w < NT / 64; ++w) { a += red[w][0]; b += red[w][1]; c = fmin(c, red[w][2]); e = fmax(e, red[w][3]); }
        double* o = part + ((long)seg * FS_ROWS + blockIdx.x) * 4;
        o[0] = a; o[1] = b; o[2] = c; o[3] = e;
    }
}
__global__ void __launch_bounds__(64) field_stats_finish_kernel(const double* __restrict__ part, double* __restrict__ out) {
    const int seg = blockIdx.x;
    if (threadIdx.x != 0) return;
    double a = 0.0, b = 0.0, c = 1.0 / 0.0, e = -1.0 / 0.0;
    for (int r = 0; r < FS_ROWS; ++r) { const double* q = part + ((long)seg * FS_ROWS + r) * 4; a += q[0]; b += q[1]; c = fmin(c, q[2]); e = fmax(e, q[3]); }
    out[seg * 4] = a; out[seg * 4 + 1] = b; out[seg * 4 + 2] = c; out[seg * 4 + 3] = e;
}
extern "C" int64_t bf_field_stats_ws_doubles(int nseg) { return nseg > 0 ? (int64_t)nseg * FS_ROWS * 4 : 0; }
extern "C" int bf_field_stats(const float* src, const int64_t* seg_begin, const int64_t* seg_len, int nseg, double* out, double* ws, bf_stream_t stream) {
    BF_REQUIRE(src && seg_begin && seg_len && out && ws && nseg > 0 && nseg <= 65535, "bf_field_stats: bad arguments");
    hipLaunchKernelGGL(field_stats_kernel, dim3(FS_ROWS, (unsigned)nseg), dim3(NT), 0, (hipStream_t)stream, src, (const long*)seg_begin, (const long*)seg_len, ws);
    BF_CHECK_LAUNCH();
    hipLaunchKernelGGL(field_stats_finish_kernel, dim3((unsigned)nseg), dim3(64), 0, (hipStream_t)stream, (const double*)ws, out);
    BF_CHECK_LAUNCH();
    return 0;
}
