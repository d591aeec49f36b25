// The device clip store, trajectories resident in HBM as [fields][total_frames][H][W] fp32: the clip gather of a batch and the dataset's
// field statistics.  The index map and the normalisation are clip_store.h's: the rollout kernels build their targets through the same two.
#include "clip_store.h"
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
struct ClipSeg { const int* field; const float* diff; const float* dv; float* out; int T, C, t0; };
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

// ---------------------------------------------------------------------------- field statistics of device-resident trajectories
// The normalisation constants of the dataset (bubbleformer/data/dataset.py:74-117: mean / std / min / max of every full field of every file,
// which the reference reads through h5py and reduces on the host) from the trajectories ALREADY resident in HBM: one launch over all
// (field, file) segments.  Pass 1: every workgroup sweeps a contiguous share of one segment (16-byte loads) and leaves {sum, sum of squares,
// min, max} in fp64; pass 2: one wave per segment adds the workgroup rows in row order (bit-reproducible; no atomics).
constexpr int FS_ROWS = 64;      // workgroups per segment
__global__ void __launch_bounds__(NT) field_stats_kernel(const float* __restrict__ src, const long* __restrict__ seg_begin, const long* __restrict__ seg_len,
                                                        double* __restrict__ part) {
    __shared__ double red[NT / 64][4];
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
