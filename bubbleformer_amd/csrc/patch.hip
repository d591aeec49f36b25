// Layout movers at the two ends of the model, FiLM, the relative-L2 loss and weight preparation.
//   im2col_nchw / col2im_nchw : (B*T, C, H, W) fp32 clip  <->  2x2 patch rows [P][Kp] (k = (c, ky, kx))
//   pm2nchw (+ loss partials)  : last debed GEMM output [P][Np] fp32 (n = (co, ky, kx)) -> (B*T, Co, H, W) fp32
//   nchw2pm (+ loss backward)  : d(pred) -> patch-major rows for the debed backward GEMMs
//   wprep / wgrad_unprep       : fp32 state_dict weights -> GEMM operand layout/dtype and back (gradients)
//   film_net fwd/bwd           : LayerNorm(P) + Linear(P, 2E) on B rows
// All are bandwidth-bound; each thread moves 8..16 contiguous bytes where the layout allows.
#include "bf_common.h"
#include "param_reduce.h"
#include <algorithm>

namespace {
constexpr int NT = 256;

// ---------------------------------------------------------------------------- im2col (stage 0 of HMLPEmbed)
// x: [F][C][H][W] fp32.  rows p = (f, y, x) over the (H/2, W/2) grid; row = Kp elements, k = c*4 + ky*2 + kx, zero padded.
template <typename T>
__global__ void __launch_bounds__(NT) im2col_kernel(const float* __restrict__ x, T* __restrict__ out, int C, int H, int W,
                                                   int Kp, long P) {
    const int W2 = W / 2, H2 = H / 2;
    const long total = P * C;   // one thread per (pixel, channel): reads 2 x float2, writes 4 elements
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int xo = (int)(i % W2);
        long t = i / W2;
        const int c = (int)(t % C);        // channel inner to x so that a wave reads contiguous image rows
        t /= C;
        const int yo = (int)(t % H2);
        const long f = t / H2;
        const float* src = x + ((f * C + c) * H + 2 * yo) * (long)W + 2 * xo;
        const float2 r0 = *reinterpret_cast<const float2*>(src);
        const float2 r1 = *reinterpret_cast<const float2*>(src + W);
        const long p = (f * H2 + yo) * W2 + xo;
        T* dst = out + p * Kp + c * 4;
        dst[0] = from_f<T>(r0.x); dst[1] = from_f<T>(r0.y); dst[2] = from_f<T>(r1.x); dst[3] = from_f<T>(r1.y);
    }
}
template <typename T>
__global__ void __launch_bounds__(NT) zero_pad_cols_kernel(T* __restrict__ out, int K, int Kp, long P) {
    const int padw = Kp - K;
    const long total = P * padw;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT)
        out[(i / padw) * Kp + K + (i % padw)] = from_f<T>(0.f);
}
// dx[f][c][2y+ky][2x+kx] = g[p][c*4 + ky*2 + kx]
template <typename T>
__global__ void __launch_bounds__(NT) col2im_kernel(const T* __restrict__ g, float* __restrict__ dx, int C, int H, int W, int Kp, long P) {
    const int W2 = W / 2, H2 = H / 2;
    const long total = P * C;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int xo = (int)(i % W2);
        long t = i / W2;
        const int c = (int)(t % C);
        t /= C;
        const int yo = (int)(t % H2);
        const long f = t / H2;
        const long p = (f * H2 + yo) * W2 + xo;
        const T* src = g + p * Kp + c * 4;
        float* dst = dx + ((f * C + c) * H + 2 * yo) * (long)W + 2 * xo;
        *reinterpret_cast<float2*>(dst) = make_float2(to_f(src[0]), to_f(src[1]));
        *reinterpret_cast<float2*>(dst + W) = make_float2(to_f(src[2]), to_f(src[3]));
    }
}

// ---------------------------------------------------------------------------- loss partial sums, order-independent
// The relative-L2 sums of a (frame, channel) come from dozens of workgroups.  Added as floats they depend on arrival order, and that
// last-bit noise reaches coef = 1 / (F sqrt(num) sqrt(den)), i.e. EVERY element of the loss gradient: in bf16 mode a few rounding flips
// there cascade through the K = 384 contractions of the backward until ~12 % of a gradient tensor's elements differ by an ulp between
// two runs on identical inputs (1.3 % in d(clip); measured).  So the partial sums are added as INTEGERS (exact, associative): a sum is
// LOSS_LIMBS 64-bit limbs holding base-2^48 digits of the value in units of 2^-112; a partial (an fp32 number: 24 significant bits) is cut
// into its digits exactly and each non-zero digit is one 64-bit integer atomic.  Covers every partial in [2^-112, 2^127) -- the whole
// useful fp32 range: un-normalised fields (norm="none" is the dataset default, bubbleformer/data/dataset.py:25) sum to 1e15 and beyond, a
// nearly converged numerator to 1e-12 and below; the reference's float sums (utils/losses.py:79-89) reach both, and a single 2^-32 limb
// (rounds 1-3) returned NaN above 2.7e8 and flushed below 2.3e-10.  lossbuf is [frames][Co][2][LOSS_LIMBS] int64, zeroed by the caller.
// A non-finite, negative or >= 2^127 partial poisons the sum (finalize returns NaN, as the float sum would give inf / NaN).
constexpr int LOSS_LIMBS = BF_LOSS_LIMBS;
constexpr long long LOSS_POISON = 1LL << 62;
__device__ __forceinline__ void loss_accum(float* lossbuf, long slot, float v) {
    unsigned long long* limb = reinterpret_cast<unsigned long long*>(lossbuf) + slot * LOSS_LIMBS;
    if (!(v >= 0.f) || !(v < 1.7014118346046923e38f)) { atomicAdd(limb + LOSS_LIMBS - 1, (unsigned long long)LOSS_POISON); return; }      // NaN, negative, >= 2^127
    double x = (double)v;                                  // exact; every step below is exact too (x has 24 significant bits)
#pragma unroll
    for (int k = LOSS_LIMBS - 1; k >= 1; --k) {
        const double unit = __builtin_ldexp(1.0, 48 * k - 112);
        const long long dgt = __double2ll_rd(x / unit);    // < 2^48
        if (dgt != 0) { atomicAdd(limb + k, (unsigned long long)dgt); x -= (double)dgt * unit; }
    }
    const long long d0 = __double2ll_rn(x * __builtin_ldexp(1.0, 112));      // what is left below 2^-64 (rounded to the 2^-112 grid)
    if (d0 != 0) atomicAdd(limb, (unsigned long long)d0);
}
__device__ __forceinline__ float loss_read(const float* lossbuf, long slot) {
    const long long* limb = reinterpret_cast<const long long*>(lossbuf) + slot * LOSS_LIMBS;
    if (limb[LOSS_LIMBS - 1] >= LOSS_POISON / 2 || limb[LOSS_LIMBS - 1] < 0) return __builtin_nanf("");
    double t = 0.0;
#pragma unroll
    for (int k = LOSS_LIMBS - 1; k >= 0; --k) t += (double)limb[k] * __builtin_ldexp(1.0, 48 * k - 112);      // same integers in -> same bits out
    return (float)t;
}

// ---------------------------------------------------------------------------- pm2nchw + loss partials
// pm: [P][Np] fp32, n = co*4 + ky*2 + kx; pred: [F][Co][H][W]; grid (blocks over h*w pixels, F)
// lossbuf[f][co][0] += sum (pred - y)^2, [1] += sum y^2   (integer limbs, see loss_accum)
__global__ void __launch_bounds__(NT) pm2nchw_kernel(const float* __restrict__ pm, float* __restrict__ pred, const float* __restrict__ y,
                                                    float* __restrict__ lossbuf, int Co, int h, int w, int Np) {
    __shared__ float red[NT / 64][2];
    const int f = blockIdx.y;
    const int H = 2 * h, W = 2 * w;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int co = 0; co < Co; ++co) {
        float num = 0.f, den = 0.f;
        for (int px = blockIdx.x * NT + threadIdx.x; px < h * w; px += gridDim.x * NT) {
            const int xo = px % w, yo = px / w;
            const float4 v = *reinterpret_cast<const float4*>(pm + ((long)f * h * w + px) * Np + co * 4);
            const long o = (((long)f * Co + co) * H + 2 * yo) * W + 2 * xo;
            *reinterpret_cast<float2*>(pred + o) = make_float2(v.x, v.y);
            *reinterpret_cast<float2*>(pred + o + W) = make_float2(v.z, v.w);
            if (y) {
                const float2 y0 = *reinterpret_cast<const float2*>(y + o);
                const float2 y1 = *reinterpret_cast<const float2*>(y + o + W);
                num += (v.x - y0.x) * (v.x - y0.x) + (v.y - y0.y) * (v.y - y0.y) + (v.z - y1.x) * (v.z - y1.x) + (v.w - y1.y) * (v.w - y1.y);
                den += y0.x * y0.x + y0.y * y0.y + y1.x * y1.x + y1.y * y1.y;
            }
        }
        if (y) {
            num = wave_sum(num); den = wave_sum(den);
            __syncthreads();
            if (lane == 0) { red[wave][0] = num; red[wave][1] = den; }
            __syncthreads();
            if (threadIdx.x == 0) {
                float a = 0.f, b = 0.f;
                for (int i = 0; i < NT / 64; ++i) { a += red[i][0]; b += red[i][1]; }
                loss_accum(lossbuf, ((long)f * Co + co) * 2, a);
                loss_accum(lossbuf, ((long)f * Co + co) * 2 + 1, b);
            }
        }
    }
}
// ---------------------------------------------------------------------------- last HMLPDebed stage in one pass (bf16)
// pred[f][co][2y+ky][2x+kx] = sum_ci gelu(act[p][ci] * sc[f][ci] + sh[f][ci]) * wc[ci][co*4 + ky*2 + kx]   (layers/patching.py:92-104:
// the last ConvTranspose2d(k=2, s=2) after InstanceNorm + GELU), plus the relative-L2 partial sums of pm2nchw_kernel.
// K = Ci <= 128 and N = 16: a 128-wide GEMM tile is 7/8 padding and each workgroup's life is a cold prologue and an epilogue; here a wave
// streams 16-row groups straight into MFMA operand registers (rows = 16 consecutive pixels of one image row), the normalisation and
// GELU are applied there, the 16 x 16 result is already (co, ky, kx) x pixel, and it leaves as float2 rows of the NCHW prediction --
// no patch-major fp32 intermediate and no second pass.  The MFMA sequence over k is the GEMM path's (32 at a time, ascending).
constexpr int DL_GPW = 16;      // 16-row groups per wave (contiguous: one frame, so the loss partials stay in registers)
template <int KS>
__global__ void __launch_bounds__(NT) debed_last_kernel(const bf16* __restrict__ act, const float* __restrict__ sc, const float* __restrict__ sh,
                                                       const bf16* __restrict__ wc, float* __restrict__ pred, const float* __restrict__ y,
                                                       float* __restrict__ lossbuf, int Co, int h, int w) {
    constexpr int Ci = 32 * KS;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int f = blockIdx.y;
    const int GF = h * w / 16;                                      // groups per frame
    const int g0 = (blockIdx.x * (NT / 64) + wave) * DL_GPW;
    if (g0 >= GF) return;
    const int g1 = min(g0 + DL_GPW, GF);
    const int H = 2 * h, W = 2 * w;
    // weights as the first MFMA operand: lane holds wc[k = 32 s + 8 lg + j][n = li]
    bf16x8 wf[KS];
    float a_sc[KS][8], a_sh[KS][8];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 32 * s + 8 * lg + j;
            wf[s][j] = wc[k * 16 + li];
            a_sc[s][j] = sc[(long)f * Ci + k];
            a_sh[s][j] = sh[(long)f * Ci + k];
        }
    }
    const bf16* rows = act + ((long)f * h * w + li) * Ci + 8 * lg;
    bf16x8 cur[KS], nxt[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) cur[s] = *reinterpret_cast<const bf16x8*>(rows + (long)g0 * 16 * Ci + 32 * s);
    float num = 0.f, den = 0.f;
    const bool live = lg < Co;
    for (int g = g0; g < g1; ++g) {
        if (g + 1 < g1) {
#pragma unroll
            for (int s = 0; s < KS; ++s) nxt[s] = *reinterpret_cast<const bf16x8*>(rows + (long)(g + 1) * 16 * Ci + 32 * s);
        }
        const int px = g * 16 + li, yo = px / w, xo = px - yo * w;
        const long o = (((long)f * Co + lg) * H + 2 * yo) * W + 2 * xo;
        float2 y0 = make_float2(0.f, 0.f), y1 = y0;
        if (y && live) { y0 = *reinterpret_cast<const float2*>(y + o); y1 = *reinterpret_cast<const float2*>(y + o + W); }
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            bf16x8 a;
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = (bf16)gelu_fast((float)cur[s][j] * a_sc[s][j] + a_sh[s][j]);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s], a, acc, 0, 0, 0);      // acc[j] = out[n = 4 lg + j][pixel li]
        }
        if (live) {
            *reinterpret_cast<float2*>(pred + o) = make_float2(acc[0], acc[1]);
            *reinterpret_cast<float2*>(pred + o + W) = make_float2(acc[2], acc[3]);
            if (y) {
                num += (acc[0] - y0.x) * (acc[0] - y0.x) + (acc[1] - y0.y) * (acc[1] - y0.y) + (acc[2] - y1.x) * (acc[2] - y1.x) + (acc[3] - y1.y) * (acc[3] - y1.y);
                den += y0.x * y0.x + y0.y * y0.y + y1.x * y1.x + y1.y * y1.y;
            }
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) cur[s] = nxt[s];
    }
    if (y) {        // the 16 lanes of a k-group share (f, co): one pair of atomics per wave and output channel
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) { num += __shfl_xor(num, m, 64); den += __shfl_xor(den, m, 64); }
        if (li == 0 && live) {
            loss_accum(lossbuf, ((long)f * Co + lg) * 2, num);
            loss_accum(lossbuf, ((long)f * Co + lg) * 2 + 1, den);
        }
    }
}
// The same stage backwards: dpm[p][co*4 + ky*2 + kx] = d pred[f][co][2y+ky][2x+kx] (given, or coef[f][co] * gscale * (pred - y) of the fused
// loss), written for the weight-gradient GEMM, and dact[p][ci] = sum_n dpm[p][n] * wc[ci][n] in the same pass (K = 16: one
// v_mfma_f32_16x16x16_bf16 per 16 input channels).  The weight rows are dealt to the MFMA tiles so that a lane ends up with runs of 8
// consecutive input channels of its pixel and the four lanes of a pixel with 32 (tile pair q, lane group lg  <->  ci = 32 q + 8 lg + ..):
// each store instruction writes 64 contiguous bytes of 16 rows, a wave 16 complete rows (BF_DL_PERM=0: 4T consecutive channels per
// lane, 16-byte pieces 8T bytes apart -- 0.13 % slower end to end).  Replaces bf_nchw2pm + a 128-wide GEMM tile with K = 16.
// BOTH: the third source mode, an explicit gradient AND the fused loss (a training step unrolled through its own predictions):
// d pred = dpred + coef[f][co] * gscale * (pred - y), formed in the same registers.  A template parameter, not a run-time branch: only
// its instantiations carry the third pair of float2 in the prefetch registers (about 10 VGPRs: one or two waves per SIMD fewer at T = 2, 4, 8), and this kernel
// is also bf_embed_first's, in the timed step.
__device__ __forceinline__ float loss_plus_given(float cf, float p, float t, float d) { return fmaf(cf, p - t, d); }      // the one expression all three entry points share (bit-identical dpm)
template <int T, bool BOTH>
__global__ void __launch_bounds__(NT) debed_last_bwd_kernel(const float* __restrict__ dpred, const float* __restrict__ pred, const float* __restrict__ y,
                                                           const float* __restrict__ coef, const float* __restrict__ gscale,
                                                           const bf16* __restrict__ wc, bf16* __restrict__ dpm, bf16* __restrict__ dact,
                                                           int Co, int h, int w, float* __restrict__ part, int perm) {
    constexpr int Ci = 16 * T;
    typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4v;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int f = blockIdx.y;
    const int GF = h * w / 16;
    const int g0 = (blockIdx.x * (NT / 64) + wave) * DL_GPW;
    if (g0 >= GF) return;
    const int g1 = min(g0 + DL_GPW, GF);
    const int H = 2 * h, W = 2 * w;
    const bool live = lg < Co;
    s16x4 wf[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        // lane (pixel li, group lg) ends up with output channel chan(k) in o[k], k = 4 t + j:
        //   perm 0: chan = 4T lg + k            (4T consecutive channels per lane: a store instruction writes 16-byte pieces 8T bytes apart)
        //   perm 1: chan = 32 (k / 8) + 8 lg + k % 8   (store instruction q writes the 64 contiguous bytes [64 q, 64 q + 64) of each row)
        const int ci = perm ? 32 * (t >> 1) + 8 * (li >> 2) + 4 * (t & 1) + (li & 3) : 4 * T * (li >> 2) + 4 * t + (li & 3);
        wf[t] = *reinterpret_cast<const s16x4*>(wc + ci * 16 + 4 * lg);
    }
    constexpr int NR = BOTH ? 6 : 4;
    const float cf = ((BOTH || !dpred) && live) ? coef[(long)f * Co + lg] * (gscale ? gscale[0] : 1.f) : 0.f;
    auto fetch = [&](int g, float2 (&r)[NR]) {
        const int px = g * 16 + li, yo = px / w, xo = px - yo * w;
        const long o = (((long)f * Co + lg) * H + 2 * yo) * W + 2 * xo;
        if constexpr (BOTH) {
            if (!live) { r[0] = r[1] = r[2] = r[3] = r[4] = r[5] = make_float2(0.f, 0.f); return; }
            r[0] = *reinterpret_cast<const float2*>(pred + o); r[1] = *reinterpret_cast<const float2*>(pred + o + W);
            r[2] = *reinterpret_cast<const float2*>(y + o); r[3] = *reinterpret_cast<const float2*>(y + o + W);
            r[4] = *reinterpret_cast<const float2*>(dpred + o); r[5] = *reinterpret_cast<const float2*>(dpred + o + W);
            return;
        }
        if (!live) { r[0] = r[1] = r[2] = r[3] = make_float2(0.f, 0.f); return; }
        if (dpred) { r[0] = *reinterpret_cast<const float2*>(dpred + o); r[1] = *reinterpret_cast<const float2*>(dpred + o + W); r[2] = r[3] = make_float2(0.f, 0.f); }
        else {
            r[0] = *reinterpret_cast<const float2*>(pred + o); r[1] = *reinterpret_cast<const float2*>(pred + o + W);
            r[2] = *reinterpret_cast<const float2*>(y + o); r[3] = *reinterpret_cast<const float2*>(y + o + W);
        }
    };
    float2 cur[NR], nxt[NR];
    fetch(g0, cur);
    float s1[4 * T], s2[4 * T];       // optional InstanceNorm statistics of the rows written (this wave's 16 DL_GPW rows = one slice)
#pragma unroll
    for (int k = 0; k < 4 * T; ++k) s1[k] = s2[k] = 0.f;
    for (int g = g0; g < g1; ++g) {
        if (g + 1 < g1) fetch(g + 1, nxt);
        float v[4];
        if constexpr (BOTH) {
            v[0] = loss_plus_given(cf, cur[0].x, cur[2].x, cur[NR - 2].x); v[1] = loss_plus_given(cf, cur[0].y, cur[2].y, cur[NR - 2].y);
            v[2] = loss_plus_given(cf, cur[1].x, cur[3].x, cur[NR - 1].x); v[3] = loss_plus_given(cf, cur[1].y, cur[3].y, cur[NR - 1].y);
        } else if (dpred) { v[0] = cur[0].x; v[1] = cur[0].y; v[2] = cur[1].x; v[3] = cur[1].y; }
        else { v[0] = cf * (cur[0].x - cur[2].x); v[1] = cf * (cur[0].y - cur[2].y); v[2] = cf * (cur[1].x - cur[3].x); v[3] = cf * (cur[1].y - cur[3].y); }
        const bf16x4v b = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
        const long p = (long)f * h * w + g * 16 + li;
        *reinterpret_cast<bf16x4v*>(dpm + p * 16 + 4 * lg) = b;
        const s16x4 bs = __builtin_bit_cast(s16x4, b);
        bf16 o[4 * T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(wf[t], bs, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[4 * t + j] = (bf16)acc[j];
        }
        if (part) {
#pragma unroll
            for (int k = 0; k < 4 * T; ++k) { const float v2 = (float)o[k]; s1[k] += v2; s2[k] += v2 * v2; }      // of the values as stored
        }
        if (dact) {                                     // (bf_embed_first without a map: only the patch rows and the statistics leave)
            bf16* dst = dact + p * Ci + (perm ? 8 * lg : 4 * T * lg);
            const int qs = perm ? 32 : 8;
#pragma unroll
            for (int q = 0; q < 4 * T / 8; ++q) {
                bf16x8 o8;
#pragma unroll
                for (int j = 0; j < 8; ++j) o8[j] = o[8 * q + j];
                *reinterpret_cast<bf16x8*>(dst + qs * q) = o8;
            }
        }
#pragma unroll
        for (int q = 0; q < NR; ++q) cur[q] = nxt[q];
    }
    if (part) {      // {slice mean, centred second moment} in in_stats_slice_kernel's layout: in_stats_merge_kernel finishes the frame
        const float n = (float)((g1 - g0) * 16);
        const int nsl = (GF + DL_GPW - 1) / DL_GPW, sl = g0 / DL_GPW;
        float2* o2 = reinterpret_cast<float2*>(part) + ((long)f * nsl + sl) * Ci;
#pragma unroll
        for (int k = 0; k < 4 * T; ++k) {
            const int chan = perm ? 32 * (k >> 3) + 8 * lg + (k & 7) : 4 * T * lg + k;
            float a = s1[k], b = s2[k];
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) { a += __shfl_xor(a, m, 64); b += __shfl_xor(b, m, 64); }
            const float mu = a / n;
            if (li == 0) o2[chan] = make_float2(mu, fmaxf(b - a * mu, 0.f));
        }
    }
}
// The last debed stage backwards TOGETHER with the InstanceNorm + GELU in front of it (layers/patching.py:92-104 under autograd).  The
// gradient of the 96-channel map at full patch-grid resolution (226 MB at the bench shape) has rank 16 -- dact = dpm @ wc^T -- so neither
// pass stores it: PASS 1 forms dpm (written: the weight gradient wants it), multiplies dact by gelu'(z) in registers and leaves the
// InstanceNorm backward's two sums per 256-row slice; PASS 2 rebuilds dact from the 16-wide rows and writes
// dx = rstd w (dd - s1/S - xh s2/S) directly.  Against debed_last_bwd_kernel + the two-phase sliced InstanceNorm backward: one write
// (226 MB) and two reads (452 MB) of the gradient map less.  Lane = (pixel li, channel runs 32 q + 8 lg .. +7): 16-byte loads of the
// activation map, 16-byte stores of dx.
struct DlInb {
    const bf16* ymap;                   // raw output of the stage in front [P][Ci]
    const float *mean, *rstd, *w, *b;   // its InstanceNorm: [frames][Ci], [Ci]
    const float* tot;                   // PASS 2: {s1, s2} per (frame, channel)
    float inv_s;                        // 1 / rows per frame
};
template <int T, int PASS, bool BOTH = false>      // BOTH (PASS 1 only): dpred and the fused loss together, as in debed_last_bwd_kernel
__global__ void __launch_bounds__(NT) debed_last_inbwd_kernel(const float* __restrict__ dpred, const float* __restrict__ pred, const float* __restrict__ y,
                                                             const float* __restrict__ coef, const float* __restrict__ gscale,
                                                             const bf16* __restrict__ wc, bf16* __restrict__ dpm, bf16* __restrict__ dx,
                                                             int Co, int h, int w, float* __restrict__ part, DlInb nb) {
    constexpr int Ci = 16 * T;
    typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4v;
    __shared__ float4 k1[Ci], k2[Ci];       // {sc, sh, rstd, -mean rstd} and {rstd w, s1 / S, s2 / S, -}
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int f = blockIdx.y;
    for (int c = threadIdx.x; c < Ci; c += NT) {
        const long o = (long)f * Ci + c;
        const float r = nb.rstd[o], m = nb.mean[o], a = r * nb.w[c];
        k1[c] = make_float4(a, fmaf(-m, a, nb.b[c]), r, -m * r);
        if (PASS == 2) k2[c] = make_float4(a, nb.tot[2 * o] * nb.inv_s, nb.tot[2 * o + 1] * nb.inv_s, 0.f);
    }
    __syncthreads();
    const int GF = h * w / 16;
    const int g0 = (blockIdx.x * (NT / 64) + wave) * DL_GPW;
    if (g0 >= GF) return;
    const int g1 = min(g0 + DL_GPW, GF);
    const int H = 2 * h, W = 2 * w;
    const bool live = lg < Co;
    s16x4 wf[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int ci = 32 * (t >> 1) + 8 * (li >> 2) + 4 * (t & 1) + (li & 3);      // lane (pixel li, group lg) gets channel 32 (k / 8) + 8 lg + k % 8 in slot k = 4 t + j
        wf[t] = *reinterpret_cast<const s16x4*>(wc + ci * 16 + 4 * lg);
    }
    static_assert(!BOTH || PASS == 1, "the second pass reads the stored rows: it has no source mode");
    constexpr int NR = BOTH ? 6 : 4;
    const float cf = (PASS == 1 && (BOTH || !dpred) && live) ? coef[(long)f * Co + lg] * (gscale ? gscale[0] : 1.f) : 0.f;
    struct Row { float2 r[NR]; bf16x8 yv[T / 2]; bf16x4v d; };
    auto fetch = [&](int g, Row& o) __attribute__((always_inline)) {
        const long p = (long)f * h * w + g * 16 + li;
#pragma unroll
        for (int q = 0; q < T / 2; ++q) o.yv[q] = *reinterpret_cast<const bf16x8*>(nb.ymap + p * Ci + 8 * lg + 32 * q);
        if (PASS == 2) { o.d = *reinterpret_cast<const bf16x4v*>(dpm + p * 16 + 4 * lg); return; }
        const int px = g * 16 + li, yo = px / w, xo = px - yo * w;
        const long oo = (((long)f * Co + lg) * H + 2 * yo) * W + 2 * xo;
        if constexpr (BOTH) {
            if (!live) { o.r[0] = o.r[1] = o.r[2] = o.r[3] = o.r[NR - 2] = o.r[NR - 1] = make_float2(0.f, 0.f); return; }
            o.r[0] = *reinterpret_cast<const float2*>(pred + oo); o.r[1] = *reinterpret_cast<const float2*>(pred + oo + W);
            o.r[2] = *reinterpret_cast<const float2*>(y + oo); o.r[3] = *reinterpret_cast<const float2*>(y + oo + W);
            o.r[NR - 2] = *reinterpret_cast<const float2*>(dpred + oo); o.r[NR - 1] = *reinterpret_cast<const float2*>(dpred + oo + W);
            return;
        }
        if (!live) { o.r[0] = o.r[1] = o.r[2] = o.r[3] = make_float2(0.f, 0.f); return; }
        if (dpred) { o.r[0] = *reinterpret_cast<const float2*>(dpred + oo); o.r[1] = *reinterpret_cast<const float2*>(dpred + oo + W); o.r[2] = o.r[3] = make_float2(0.f, 0.f); }
        else {
            o.r[0] = *reinterpret_cast<const float2*>(pred + oo); o.r[1] = *reinterpret_cast<const float2*>(pred + oo + W);
            o.r[2] = *reinterpret_cast<const float2*>(y + oo); o.r[3] = *reinterpret_cast<const float2*>(y + oo + W);
        }
    };
    Row cur, nxt, nx2;                  // two 16-pixel groups ahead: a wave has few registers left for anything but bytes in flight
    fetch(g0, cur);
    if (g0 + 1 < g1) fetch(g0 + 1, nxt);
    float s1[PASS == 1 ? 4 * T : 1], s2[PASS == 1 ? 4 * T : 1];
    if (PASS == 1) {
#pragma unroll
        for (int k = 0; k < 4 * T; ++k) s1[k] = s2[k] = 0.f;
    }
    for (int g = g0; g < g1; ++g) {
        if (g + 2 < g1) fetch(g + 2, nx2);
        const long p = (long)f * h * w + g * 16 + li;
        bf16x4v b;
        if (PASS == 1) {
            float v[4];
            if constexpr (BOTH) {
                v[0] = loss_plus_given(cf, cur.r[0].x, cur.r[2].x, cur.r[NR - 2].x); v[1] = loss_plus_given(cf, cur.r[0].y, cur.r[2].y, cur.r[NR - 2].y);
                v[2] = loss_plus_given(cf, cur.r[1].x, cur.r[3].x, cur.r[NR - 1].x); v[3] = loss_plus_given(cf, cur.r[1].y, cur.r[3].y, cur.r[NR - 1].y);
            } else if (dpred) { v[0] = cur.r[0].x; v[1] = cur.r[0].y; v[2] = cur.r[1].x; v[3] = cur.r[1].y; }
            else { v[0] = cf * (cur.r[0].x - cur.r[2].x); v[1] = cf * (cur.r[0].y - cur.r[2].y); v[2] = cf * (cur.r[1].x - cur.r[3].x); v[3] = cf * (cur.r[1].y - cur.r[3].y); }
            b = bf16x4v{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
            *reinterpret_cast<bf16x4v*>(dpm + p * 16 + 4 * lg) = b;
        } else b = cur.d;
        const s16x4 bs = __builtin_bit_cast(s16x4, b);
        bf16x8 o8[T / 2];
        // the per-channel constants are loop invariant: left alone the compiler keeps all 4 * 4T (+ 3 * 4T) of them in registers, which
        // halves the waves a SIMD can hold; an offset it cannot see through makes them 16-byte LDS reads per group instead
        int kofs = 8 * lg;
        asm volatile("" : "+v"(kofs));
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(wf[t], bs, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = 4 * t + j;
                const float4 c1 = k1[32 * (k >> 3) + kofs + (k & 7)];
                const float yv = (float)cur.yv[k >> 3][k & 7];
                const float dd = acc[j] * dgelu_fast(fmaf(yv, c1.x, c1.y)), xh = fmaf(yv, c1.z, c1.w);
                if (PASS == 1) { s1[k] += dd; s2[k] = fmaf(dd, xh, s2[k]); }
                else {
                    const float4 c2 = k2[32 * (k >> 3) + kofs + (k & 7)];
                    o8[k >> 3][k & 7] = (bf16)(c2.x * (dd - c2.y - xh * c2.z));
                }
            }
        }
        if (PASS == 2) {
#pragma unroll
            for (int q = 0; q < T / 2; ++q) *reinterpret_cast<bf16x8*>(dx + p * Ci + 8 * lg + 32 * q) = o8[q];
        }
        cur = nxt;
        nxt = nx2;
    }
    if (PASS == 1) {      // {sum dd, sum dd xh} of this wave's slice: part[(f * nsl + sl) * Ci + c]
        const int nsl = (GF + DL_GPW - 1) / DL_GPW, sl = g0 / DL_GPW;
        float2* o2 = reinterpret_cast<float2*>(part) + ((long)f * nsl + sl) * Ci;
#pragma unroll
        for (int k = 0; k < 4 * T; ++k) {
            float a = s1[k], b2 = s2[k];
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) { a += __shfl_xor(a, m, 64); b2 += __shfl_xor(b2, m, 64); }
            if (li == 0) o2[32 * (k >> 3) + 8 * lg + (k & 7)] = make_float2(a, b2);
        }
    }
}
// tot[f][c] = sum over slices, in slice order.  grid (ceil(C / 64), frames), 256 threads = 64 channels x 4 slice lanes
__global__ void __launch_bounds__(NT) dl_slice_sum_kernel(const float* __restrict__ part, int C, int nsl, float* __restrict__ tot) {
    __shared__ float red[2][4][64];
    const int l = threadIdx.x & 63, q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = blockIdx.x * 64 + l, f = blockIdx.y;
    const bool cv = c < C;
    const float2* pp = reinterpret_cast<const float2*>(part) + (long)f * nsl * C + (cv ? c : 0);
    float a = 0.f, b = 0.f;
    if (cv)
        for (int sl = q; sl < nsl; sl += 4) { const float2 v = pp[(long)sl * C]; a += v.x; b += v.y; }
    red[0][q][l] = a; red[1][q][l] = b;
    __syncthreads();
    if (q != 0 || !cv) return;
    reinterpret_cast<float2*>(tot)[(long)f * C + c] = make_float2((red[0][0][l] + red[0][1][l]) + (red[0][2][l] + red[0][3][l]),
                                                                 (red[1][0][l] + red[1][1][l]) + (red[1][2][l] + red[1][3][l]));
}
__global__ void __launch_bounds__(64 * BF_RED_FL) dl_param_reduce_kernel(InReduceJob j) {
    __shared__ float red[5][BF_RED_FL][64];
    in_reduce_block(j, blockIdx.x, blockIdx.y, red);
}
// loss = sum_c mean_f sqrt(num/den);  coef[f][c] = 1 / (F * sqrt(num) * sqrt(den))   (single block)
__global__ void lploss_finalize_kernel(const float* __restrict__ lossbuf, int F, int Co, float* __restrict__ loss, float* __restrict__ coef) {
    __shared__ float red[NT];
    float acc = 0.f;
    for (int i = threadIdx.x; i < F * Co; i += NT) {
        const float num = loss_read(lossbuf, 2 * i), den = loss_read(lossbuf, 2 * i + 1);
        acc += sqrtf(num) / sqrtf(den);
        if (coef) coef[i] = 1.0f / ((float)F * sqrtf(num) * sqrtf(den));
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) { if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    if (threadIdx.x == 0) loss[0] = red[0] / (float)F;
}
// dpm[p][n] = dpred[f][co][2y+ky][2x+kx]   with dpred either given, or coef[f][co] * gscale * (pred - y), or (BOTH) the sum of the two
template <typename T, bool BOTH>
__global__ void __launch_bounds__(NT) nchw2pm_kernel(const float* __restrict__ dpred, const float* __restrict__ pred, const float* __restrict__ y,
                                                    const float* __restrict__ coef, const float* __restrict__ gscale, T* __restrict__ dpm,
                                                    int Co, int h, int w, int Np, long P) {
    const int H = 2 * h, W = 2 * w;
    const int nq = Np / 4;   // groups of 4 columns (one co each; groups >= Co are zero padding)
    const long total = P * nq;
    const float gs = gscale ? gscale[0] : 1.f;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int co = (int)(i % nq);
        const long p = i / nq;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
        if (co < Co) {
            const int xo = (int)(p % w);
            const long t = p / w;
            const int yo = (int)(t % h);
            const long f = t / h;
            const long o = ((f * Co + co) * H + 2 * yo) * (long)W + 2 * xo;
            if constexpr (BOTH) {
                const float cf = coef[f * Co + co] * gs;
                const float2 a = *reinterpret_cast<const float2*>(pred + o), b = *reinterpret_cast<const float2*>(pred + o + W);
                const float2 c = *reinterpret_cast<const float2*>(y + o), d = *reinterpret_cast<const float2*>(y + o + W);
                const float2 e = *reinterpret_cast<const float2*>(dpred + o), g = *reinterpret_cast<const float2*>(dpred + o + W);
                v0 = loss_plus_given(cf, a.x, c.x, e.x); v1 = loss_plus_given(cf, a.y, c.y, e.y);
                v2 = loss_plus_given(cf, b.x, d.x, g.x); v3 = loss_plus_given(cf, b.y, d.y, g.y);
            } else if (dpred) {
                const float2 a = *reinterpret_cast<const float2*>(dpred + o), b = *reinterpret_cast<const float2*>(dpred + o + W);
                v0 = a.x; v1 = a.y; v2 = b.x; v3 = b.y;
            } else {
                const float cf = coef[f * Co + co] * gs;
                const float2 a = *reinterpret_cast<const float2*>(pred + o), b = *reinterpret_cast<const float2*>(pred + o + W);
                const float2 c = *reinterpret_cast<const float2*>(y + o), d = *reinterpret_cast<const float2*>(y + o + W);
                v0 = cf * (a.x - c.x); v1 = cf * (a.y - c.y); v2 = cf * (b.x - d.x); v3 = cf * (b.y - d.y);
            }
        }
        T* dst = dpm + p * Np + co * 4;
        dst[0] = from_f<T>(v0); dst[1] = from_f<T>(v1); dst[2] = from_f<T>(v2); dst[3] = from_f<T>(v3);
    }
}

// ---------------------------------------------------------------------------- weight preparation
// modes: 0 cast/pad rows: [R][K] -> [R][Kp]
//        1 conv k2s2  [Co][Ci][2][2] -> [Co][(ky,kx,ci)]
//        2 convT k2s2 [Ci][Co][2][2] -> [(ky,kx,co)][Ci]
template <typename T>
__global__ void __launch_bounds__(NT) wprep_kernel(const float* __restrict__ src, T* __restrict__ dst, int mode, int R, int K, int Kp) {
    const long total = (long)R * Kp;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int r = (int)(i / Kp), k = (int)(i % Kp);
        float v = 0.f;
        if (mode == 0) { if (k < K) v = src[(long)r * K + k]; }
        else if (mode == 1) {          // R = Co, K = Kp = 4*Ci ; k = (ky*2+kx)*Ci + ci
            const int Ci = K / 4, q = k / Ci, ci = k % Ci;
            v = src[((long)r * Ci + ci) * 4 + q];
        } else {                       // mode 2: R = 4*Co rows r = q*Co + co ; K = Ci
            const int Co = R / 4, q = r / Co, co = r % Co;
            v = src[((long)k * Co + co) * 4 + q];
        }
        dst[i] = from_f<T>(v);
    }
}
// all stages of an embed / debed call in ONE launch (blockIdx.y = stage)
struct WprepJobs { const float* src[BF_MAX_STAGES]; void* dst[BF_MAX_STAGES]; int mode[BF_MAX_STAGES], R[BF_MAX_STAGES], K[BF_MAX_STAGES], Kp[BF_MAX_STAGES]; };
template <typename T>
__global__ void __launch_bounds__(NT) wprep_multi_kernel(WprepJobs j) {
    const int s = blockIdx.y;
    const float* __restrict__ src = j.src[s];
    T* __restrict__ dst = reinterpret_cast<T*>(j.dst[s]);
    const int mode = j.mode[s], R = j.R[s], K = j.K[s], Kp = j.Kp[s];
    const long total = (long)R * Kp;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int r = (int)(i / Kp), k = (int)(i % Kp);
        float v = 0.f;
        if (mode == 0) { if (k < K) v = src[(long)r * K + k]; }
        else if (mode == 1) { const int Ci = K / 4, q = k / Ci, ci = k % Ci; v = src[((long)r * Ci + ci) * 4 + q]; }
        else { const int Co = R / 4, q = r / Co, co = r % Co; v = src[((long)k * Co + co) * 4 + q]; }
        dst[i] = from_f<T>(v);
    }
}
// gradient of the prepared operand (fp32, prepared layout) accumulated into the state_dict layout
__global__ void __launch_bounds__(NT) wgrad_unprep_kernel(const float* __restrict__ gsrc, float* __restrict__ gdst, int mode, int R, int K, int Kp,
                                                         int transposed) {
    const long total = (long)R * K;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int r = (int)(i / K), k = (int)(i % K);
        // transposed: gsrc is [Kp_rows = k][R] (the GEMM produced the transpose)
        const float v = transposed ? gsrc[(long)k * R + r] : gsrc[(long)r * Kp + k];
        long o;
        if (mode == 0) o = (long)r * K + k;
        else if (mode == 1) { const int Ci = K / 4, q = k / Ci, ci = k % Ci; o = ((long)r * Ci + ci) * 4 + q; }
        else { const int Co = R / 4, q = r / Co, co = r % Co; o = ((long)k * Co + co) * 4 + q; }
        gdst[o] += v;
    }
}

// ---------------------------------------------------------------------------- FiLM net (B rows; one block)
// gb[b][0:E] = gamma, gb[b][E:2E] = beta ;  c = LN(cond) ; gb = c @ W^T + bias
__global__ void film_net_fwd_kernel(const float* __restrict__ cond, const float* __restrict__ lnw, const float* __restrict__ lnb,
                                    const float* __restrict__ W, const float* __restrict__ bias, float* __restrict__ gb,
                                    float* __restrict__ chat, float* __restrict__ crstd, int B, int P, int E2) {
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        float mu = 0.f;
        for (int i = 0; i < P; ++i) mu += cond[b * P + i];
        mu /= (float)P;
        float var = 0.f;
        for (int i = 0; i < P; ++i) { const float t = cond[b * P + i] - mu; var += t * t; }
        const float r = rsqrtf(var / (float)P + BF_IN_EPS);
        if (threadIdx.x == 0) crstd[b] = r;
        for (int i = threadIdx.x; i < P; i += blockDim.x) chat[b * P + i] = (cond[b * P + i] - mu) * r;
        for (int o = threadIdx.x; o < E2; o += blockDim.x) {
            float acc = bias[o];
            for (int i = 0; i < P; ++i) acc += ((cond[b * P + i] - mu) * r * lnw[i] + lnb[i]) * W[(long)o * P + i];
            gb[(long)(o / (E2 / 2)) * B * (E2 / 2) + (long)b * (E2 / 2) + (o % (E2 / 2))] = acc;   // [2][B][E]
        }
    }
}
// dgb: [B][2E] (dgamma | dbeta).  dW[o][i] += sum_b dgb[b][o] c[b][i]; dbias[o] += sum_b dgb;
// dc[b][i] = sum_o dgb[b][o] W[o][i]; dlnw[i] += sum_b dc*chat; dlnb[i] += sum_b dc   (d cond is not needed)
__global__ void film_net_bwd_kernel(const float* __restrict__ dgb_, const float* __restrict__ chat, const float* __restrict__ lnw,
                                    const float* __restrict__ lnb, const float* __restrict__ W, float* __restrict__ dW,
                                    float* __restrict__ dbias, float* __restrict__ dlnw, float* __restrict__ dlnb, int B, int P, int E2) {
    const int E = E2 / 2;
    // fp64 accumulation: the LayerNorm(P) gradients are sums of 2E signed terms that largely cancel, and the kernel is tiny
    const int nmain = ((E2 + 63) / 64);
    if ((int)blockIdx.x >= nmain) {
        // P more workgroups (64 threads), one per LayerNorm input i: dlnw[i] / dlnb[i], each a sum over ALL outputs o and samples b -- lane l
        // takes o = l, l + 64, ... in order and the 64 partial sums meet in a fixed butterfly: one writer per value, no float atomics (they
        // used to arrive from every wave in arrival order: the two gradients differed from run to run)
        {
            const int i = (int)blockIdx.x - nmain;
            double sw = 0.0, sbias = 0.0;
            for (int o = threadIdx.x; o < E2; o += 64) {
                const double w = W[(long)o * P + i];
                for (int b = 0; b < B; ++b) {
                    const double dg = (double)dgb_[(long)(o / E) * B * E + (long)b * E + (o % E)];
                    sw += dg * w * chat[b * P + i];
                    sbias += dg * w;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { sw += __shfl_xor(sw, off, 64); sbias += __shfl_xor(sbias, off, 64); }
            if (threadIdx.x == 0) { dlnw[i] += (float)sw; dlnb[i] += (float)sbias; }
        }
        return;
    }
    // one thread per output row o of the Linear: dW[o][:] and dbias[o]
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= E2) return;
    double sb = 0.0;
    for (int b = 0; b < B; ++b) sb += (double)dgb_[(long)(o / E) * B * E + (long)b * E + (o % E)];
    dbias[o] += (float)sb;
    for (int i = 0; i < P; ++i) {
        double acc = 0.0;
        for (int b = 0; b < B; ++b)
            acc += (double)dgb_[(long)(o / E) * B * E + (long)b * E + (o % E)] * ((double)chat[b * P + i] * lnw[i] + lnb[i]);
        dW[(long)o * P + i] += (float)acc;
    }
}

int grid_for(long total) { return (int)std::max<long>(1, std::min<long>((total + NT - 1) / NT, 256L * 16)); }
}  // namespace

extern "C" int bf_im2col_nchw(int dtype, const float* x, void* out, int frames, int C, int H, int W, int Kp, bf_stream_t stream) {
    BF_REQUIRE(x && out && frames > 0 && C > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && Kp >= 4 * C, "bf_im2col_nchw: bad arguments");
    const long P = (long)frames * (H / 2) * (W / 2);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == BF_DTYPE_BF16) {
        hipLaunchKernelGGL(im2col_kernel<bf16>, dim3(grid_for(P * C)), dim3(NT), 0, st, x, (bf16*)out, C, H, W, Kp, P);
        if (Kp > 4 * C) hipLaunchKernelGGL(zero_pad_cols_kernel<bf16>, dim3(grid_for(P * (Kp - 4 * C))), dim3(NT), 0, st, (bf16*)out, 4 * C, Kp, P);
    } else {
        hipLaunchKernelGGL(im2col_kernel<float>, dim3(grid_for(P * C)), dim3(NT), 0, st, x, (float*)out, C, H, W, Kp, P);
        if (Kp > 4 * C) hipLaunchKernelGGL(zero_pad_cols_kernel<float>, dim3(grid_for(P * (Kp - 4 * C))), dim3(NT), 0, st, (float*)out, 4 * C, Kp, P);
    }
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_col2im_nchw(int dtype, const void* g, float* dx, int frames, int C, int H, int W, int Kp, bf_stream_t stream) {
    BF_REQUIRE(g && dx && frames > 0 && C > 0 && H % 2 == 0 && W % 2 == 0 && Kp >= 4 * C, "bf_col2im_nchw: bad arguments");
    const long P = (long)frames * (H / 2) * (W / 2);
    if (dtype == BF_DTYPE_BF16) hipLaunchKernelGGL(col2im_kernel<bf16>, dim3(grid_for(P * C)), dim3(NT), 0, (hipStream_t)stream, (const bf16*)g, dx, C, H, W, Kp, P);
    else hipLaunchKernelGGL(col2im_kernel<float>, dim3(grid_for(P * C)), dim3(NT), 0, (hipStream_t)stream, (const float*)g, dx, C, H, W, Kp, P);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_pm2nchw(const float* pm, float* pred, const float* y, float* lossbuf, int frames, int Co, int h, int w, int Np,
                          bf_stream_t stream) {
    BF_REQUIRE(pm && pred && frames > 0 && Co > 0 && h > 0 && w > 0 && Np >= 4 * Co && Np % 4 == 0, "bf_pm2nchw: bad arguments");
    BF_REQUIRE(!y || lossbuf, "bf_pm2nchw: loss buffer missing");
    dim3 grid(std::max(1, std::min(bf_cdiv((long)h * w, NT), 64)), frames);
    hipLaunchKernelGGL(pm2nchw_kernel, grid, dim3(NT), 0, (hipStream_t)stream, pm, pred, y, lossbuf, Co, h, w, Np);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_debed_last(int dtype, const void* act, const float* sc, const float* sh, const void* wc, float* pred, const float* y,
                             float* lossbuf, int frames, int Ci, int Co, int h, int w, int Np, bf_stream_t stream) {
    BF_REQUIRE(act && sc && sh && wc && pred && frames > 0 && Ci > 0 && Co > 0 && h > 0 && w > 0, "bf_debed_last: bad arguments");
    BF_REQUIRE(!y || lossbuf, "bf_debed_last: loss buffer missing");
    // shapes the streaming kernel does not take (the caller falls back to GEMM + bf_pm2nchw): not an error
    if (dtype != BF_DTYPE_BF16 || Np != 16 || Co > 4 || Ci % 32 != 0 || Ci > 128 || w % 16 != 0) return 1;
    static const bool off = bf_knob("BF_DEBED_LAST", 1) == 0;
    if (off) return 1;
    const int GF = h * w / 16;
    dim3 grid(bf_cdiv(GF, (NT / 64) * DL_GPW), frames);
    hipStream_t st = (hipStream_t)stream;
    const double P = (double)frames * h * w;
    BfProfScope prof(st, "debed_last", 2.0 * P * Ci * 16, P * (2.0 * Ci + 16.0 * Co * (y ? 2 : 1)));
#define DL(KS) hipLaunchKernelGGL(debed_last_kernel<KS>, grid, dim3(NT), 0, st, (const bf16*)act, sc, sh, (const bf16*)wc, pred, y, lossbuf, Co, h, w)
    switch (Ci / 32) { case 1: DL(1); break; case 2: DL(2); break; case 3: DL(3); break; default: DL(4); break; }
#undef DL
    BF_CHECK_LAUNCH();
    return 0;
}

// the source mode of the last debed stage's backward: dpred alone, (pred, y, coef) alone, or -- all of them given -- their sum
static inline bool dl_both(const float* dpred, const float* pred, const float* y) { return dpred && pred && y; }
static int debed_last_bwd_launch(int dtype, const float* dpred, const float* pred, const float* y, const float* coef, const float* gscale,
                                 const void* wc, void* dpm, void* dact, int frames, int Ci, int Co, int h, int w, int Np, float* part,
                                 bf_stream_t stream) {
    BF_REQUIRE(wc && dpm && (dact || part) && (dpred || (pred && y && coef)) && frames > 0 && Ci > 0 && Co > 0 && h > 0 && w > 0, "bf_debed_last_bwd: bad arguments");
    const bool both = dl_both(dpred, pred, y);
    BF_REQUIRE(!both || coef, "bf_debed_last_bwd: dpred beside (pred, y) adds the fused loss term and needs coef");
    if (dtype != BF_DTYPE_BF16 || Np != 16 || Co > 4 || Ci % 32 != 0 || Ci > 128 || w % 16 != 0) return 1;      // caller keeps bf_nchw2pm + GEMM
    static const bool off = bf_knob("BF_DEBED_LAST_BWD", 1) == 0;
    if (off) return 1;
    const int GF = h * w / 16;
    dim3 grid(bf_cdiv(GF, (NT / 64) * DL_GPW), frames);
    hipStream_t st = (hipStream_t)stream;
    static const int perm = bf_knob("BF_DL_PERM", 1);
    const double P = (double)frames * h * w;
    BfProfScope prof(st, both ? "patch16<both>" : "patch16", 2.0 * P * Ci * 16, P * (2.0 * Ci + 32.0 + 16.0 * Co * (both ? 3 : dpred ? 1 : 2)));
#define DLB(T, B) hipLaunchKernelGGL((debed_last_bwd_kernel<T, B>), grid, dim3(NT), 0, st, dpred, pred, y, coef, gscale, (const bf16*)wc, (bf16*)dpm, (bf16*)dact, Co, h, w, part, perm)
    if (both) switch (Ci / 32) { case 1: DLB(2, true); break; case 2: DLB(4, true); break; case 3: DLB(6, true); break; default: DLB(8, true); break; }
    else switch (Ci / 32) { case 1: DLB(2, false); break; case 2: DLB(4, false); break; case 3: DLB(6, false); break; default: DLB(8, false); break; }
#undef DLB
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_debed_last_bwd(int dtype, const float* dpred, const float* pred, const float* y, const float* coef, const float* gscale,
                                 const void* wc, void* dpm, void* dact, int frames, int Ci, int Co, int h, int w, int Np, bf_stream_t stream) {
    return debed_last_bwd_launch(dtype, dpred, pred, y, coef, gscale, wc, dpm, dact, frames, Ci, Co, h, w, Np, nullptr, stream);
}

// ... with the InstanceNorm + GELU in front of the stage folded in (debed_last_inbwd_kernel): dpm as above, dx [P][Ci] = the gradient of the
// RAW map ymap in front of that InstanceNorm, d_in_w / d_in_b accumulated.  ws: bf_in_ws_floats(dtype, frames, h*w, Ci) floats.
// Returns 1 (nothing launched) for the shapes bf_debed_last_bwd declines, Ci % 32, or a workspace that does not hold 256-row slices.
extern "C" int bf_debed_last_bwd_norm(int dtype, const float* dpred, const float* pred, const float* y, const float* coef, const float* gscale,
                                      const void* wc, void* dpm, const void* ymap, const float* mean, const float* rstd, const float* in_w,
                                      const float* in_b, void* dx, float* d_in_w, float* d_in_b, int frames, int Ci, int Co, int h, int w, int Np,
                                      float* ws, int64_t ws_floats, bf_stream_t stream) {
    if (dtype != BF_DTYPE_BF16 || Np != 16 || Co > 4 || Ci % 32 != 0 || Ci > 128 || w % 16 != 0)
        return bf_decline("bf_debed_last_bwd_norm covers bf16, Np = 16, Co <= 4, Ci a multiple of 32 up to 128, w a multiple of 16");
    static const bool off = bf_knob("BF_DEBED_LAST_NORM", 1) == 0;
    if (off) return bf_decline("bf_debed_last_bwd_norm: switched off (BF_DEBED_LAST_NORM=0)");
    BF_REQUIRE(wc && dpm && ymap && mean && rstd && in_w && in_b && dx && ws && (dpred || (pred && y && coef)) && frames > 0 && Co > 0 && h > 0 && w > 0,
               "bf_debed_last_bwd_norm: bad arguments");
    const bool both = dl_both(dpred, pred, y);
    BF_REQUIRE(!both || coef, "bf_debed_last_bwd_norm: dpred beside (pred, y) adds the fused loss term and needs coef");
    const int GF = h * w / 16, nsl = bf_cdiv(GF, DL_GPW);
    if (ws_floats < (int64_t)2 * frames * Ci * (1 + nsl))
        return bf_decline("bf_debed_last_bwd_norm: workspace smaller than 2 * frames * Ci * (1 + slices) floats (bf_in_ws_floats)");
    float* tot = ws;
    float* part = ws + (size_t)2 * frames * Ci;
    dim3 grid(bf_cdiv(GF, (NT / 64) * DL_GPW), frames);
    hipStream_t st = (hipStream_t)stream;
    const double P = (double)frames * h * w;
    const DlInb nb1{(const bf16*)ymap, mean, rstd, in_w, in_b, nullptr, 0.f};
    const DlInb nb2{(const bf16*)ymap, mean, rstd, in_w, in_b, tot, 1.0f / (float)(h * w)};
    {
        BfProfScope prof(st, both ? "debed_last_bwd<stats,both>" : "debed_last_bwd<stats>", 2.0 * P * Ci * 16, P * (2.0 * Ci + 32.0 + 16.0 * Co * (both ? 3 : dpred ? 1 : 2)));
#define DLN(T, B) hipLaunchKernelGGL((debed_last_inbwd_kernel<T, 1, B>), grid, dim3(NT), 0, st, dpred, pred, y, coef, gscale, (const bf16*)wc, (bf16*)dpm, (bf16*)dx, Co, h, w, part, nb1)
        if (both) switch (Ci / 32) { case 1: DLN(2, true); break; case 2: DLN(4, true); break; case 3: DLN(6, true); break; default: DLN(8, true); break; }
        else switch (Ci / 32) { case 1: DLN(2, false); break; case 2: DLN(4, false); break; case 3: DLN(6, false); break; default: DLN(8, false); break; }
#undef DLN
        BF_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(dl_slice_sum_kernel, dim3(bf_cdiv(Ci, 64), frames), dim3(NT), 0, st, (const float*)part, Ci, nsl, tot);
    BF_CHECK_LAUNCH();
    {
        BfProfScope prof(st, "debed_last_bwd<apply>", 2.0 * P * Ci * 16, P * (4.0 * Ci + 32.0));
#define DLN(T) hipLaunchKernelGGL((debed_last_inbwd_kernel<T, 2>), grid, dim3(NT), 0, st, nullptr, nullptr, nullptr, nullptr, nullptr, (const bf16*)wc, (bf16*)dpm, (bf16*)dx, Co, h, w, nullptr, nb2)
        switch (Ci / 32) { case 1: DLN(2); break; case 2: DLN(4); break; case 3: DLN(6); break; default: DLN(8); break; }
#undef DLN
        BF_CHECK_LAUNCH();
    }
    if (d_in_w || d_in_b) {
        const InReduceJob j{tot, frames, Ci, in_w, in_b, nullptr, 1, d_in_w, d_in_b, nullptr, nullptr, nullptr, nullptr};
        hipLaunchKernelGGL(dl_param_reduce_kernel, dim3(bf_cdiv(Ci, 64), bf_cdiv(frames, j.rdiv())), dim3(64 * BF_RED_FL), 0, st, j);
        BF_CHECK_LAUNCH();
    }
    return 0;
}

// The first HMLPEmbed stage is the same contraction (layers/patching.py:30-48, Conv2d(k=2, s=2, bias=False) on the NCHW clip): rows of 2x2
// patches of x (k = c*4 + ky*2 + kx) times conv weight [C0][16]; `patches` is kept for the weight-gradient GEMM.
// `stat_part` (optional): per 256-row slice {mean, centred second moment} of y0 as stored, [frames][ceil(h2*w2/256)][C0][2] floats -- the
// partials bf_in_stats_merge_slices turns into the stage's InstanceNorm statistics, so that y0 is not read again for them.
extern "C" int bf_embed_first(int dtype, const float* x, const void* wc, void* patches, void* y0, int frames, int C0, int cin, int h2, int w2,
                              int Kp, float* stat_part, bf_stream_t stream) {
    BF_REQUIRE(x && wc && patches && (y0 || stat_part), "bf_embed_first: null pointer");      // y0 may be null when its statistics are all that is wanted of it
    static const bool off = bf_knob("BF_EMBED_FIRST", 1) == 0;
    if (off) return 1;
    return debed_last_bwd_launch(dtype, x, nullptr, nullptr, nullptr, nullptr, wc, patches, y0, frames, C0, cin, h2, w2, Kp, stat_part, stream);
}

extern "C" int bf_lploss_finalize(const float* lossbuf, int frames, int Co, float* loss, float* coef, bf_stream_t stream) {
    BF_REQUIRE(lossbuf && loss && frames > 0 && Co > 0, "bf_lploss_finalize: bad arguments");
    hipLaunchKernelGGL(lploss_finalize_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, lossbuf, frames, Co, loss, coef);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_nchw2pm(int dtype, const float* dpred, const float* pred, const float* y, const float* coef, const float* gscale,
                          void* dpm, int frames, int Co, int h, int w, int Np, bf_stream_t stream) {
    BF_REQUIRE(dpm && (dpred || (pred && y && coef)) && Np >= 4 * Co && Np % 4 == 0, "bf_nchw2pm: bad arguments");
    const bool both = dl_both(dpred, pred, y);
    BF_REQUIRE(!both || coef, "bf_nchw2pm: dpred beside (pred, y) adds the fused loss term and needs coef");
    const long P = (long)frames * h * w;
#define N2P(T, B) hipLaunchKernelGGL((nchw2pm_kernel<T, B>), dim3(grid_for(P * (Np / 4))), dim3(NT), 0, (hipStream_t)stream, dpred, pred, y, coef, gscale, (T*)dpm, Co, h, w, Np, P)
    if (dtype == BF_DTYPE_BF16) { if (both) N2P(bf16, true); else N2P(bf16, false); }
    else { if (both) N2P(float, true); else N2P(float, false); }
#undef N2P
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_wprep(int dtype, int mode, const float* src, void* dst, int R, int K, int Kp, bf_stream_t stream) {
    BF_REQUIRE(src && dst && R > 0 && K > 0 && Kp >= K && mode >= 0 && mode <= 2, "bf_wprep: bad arguments");
    BF_REQUIRE(mode == 0 || Kp == K, "bf_wprep: padding only with mode 0");
    if (dtype == BF_DTYPE_BF16) hipLaunchKernelGGL(wprep_kernel<bf16>, dim3(grid_for((long)R * Kp)), dim3(NT), 0, (hipStream_t)stream, src, (bf16*)dst, mode, R, K, Kp);
    else hipLaunchKernelGGL(wprep_kernel<float>, dim3(grid_for((long)R * Kp)), dim3(NT), 0, (hipStream_t)stream, src, (float*)dst, mode, R, K, Kp);
    BF_CHECK_LAUNCH();
    return 0;
}

// bf_wprep for n <= BF_MAX_STAGES weights at once (same modes and argument meaning per entry)
int bf_wprep_multi(int dtype, int n, const int* mode, const float* const* src, void* const* dst, const int* R, const int* K, const int* Kp, hipStream_t st) {
    BF_REQUIRE(n >= 1 && n <= BF_MAX_STAGES && mode && src && dst && R && K && Kp, "bf_wprep_multi: bad arguments");
    WprepJobs j;
    long most = 0;
    for (int i = 0; i < n; ++i) {
        BF_REQUIRE(src[i] && dst[i] && R[i] > 0 && K[i] > 0 && Kp[i] >= K[i] && mode[i] >= 0 && mode[i] <= 2 && (mode[i] == 0 || Kp[i] == K[i]), "bf_wprep_multi: bad entry");
        j.src[i] = src[i]; j.dst[i] = dst[i]; j.mode[i] = mode[i]; j.R[i] = R[i]; j.K[i] = K[i]; j.Kp[i] = Kp[i];
        most = std::max(most, (long)R[i] * Kp[i]);
    }
    const dim3 grid(std::min<long>(bf_cdiv(most, NT), 256), n);
    if (dtype == BF_DTYPE_BF16) hipLaunchKernelGGL(wprep_multi_kernel<bf16>, grid, dim3(NT), 0, st, j);
    else hipLaunchKernelGGL(wprep_multi_kernel<float>, grid, dim3(NT), 0, st, j);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_wgrad_unprep(int mode, const float* gsrc, float* gdst, int R, int K, int Kp, int transposed, bf_stream_t stream) {
    BF_REQUIRE(gsrc && gdst && R > 0 && K > 0 && Kp >= K && mode >= 0 && mode <= 2, "bf_wgrad_unprep: bad arguments");
    hipLaunchKernelGGL(wgrad_unprep_kernel, dim3(grid_for((long)R * K)), dim3(NT), 0, (hipStream_t)stream, gsrc, gdst, mode, R, K, Kp, transposed);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_film_net_fwd(const float* cond, const float* lnw, const float* lnb, const float* W, const float* bias, float* gb,
                               float* chat, float* crstd, int B, int P, int E2, bf_stream_t stream) {
    BF_REQUIRE(cond && lnw && lnb && W && bias && gb && chat && crstd && B > 0 && P > 0 && E2 > 0, "bf_film_net_fwd: bad arguments");
    hipLaunchKernelGGL(film_net_fwd_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, cond, lnw, lnb, W, bias, gb, chat, crstd, B, P, E2);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_film_net_bwd(const float* dgb, const float* chat, const float* lnw, const float* lnb, const float* W, float* dW,
                               float* dbias, float* dlnw, float* dlnb, int B, int P, int E2, bf_stream_t stream) {
    BF_REQUIRE(dgb && chat && lnw && lnb && W && dW && dbias && dlnw && dlnb, "bf_film_net_bwd: bad arguments");
    hipLaunchKernelGGL(film_net_bwd_kernel, dim3(bf_cdiv(E2, 64) + P), dim3(64), 0, (hipStream_t)stream, dgb, chat, lnw, lnb, W, dW, dbias, dlnw, dlnb, B, P, E2);
    BF_CHECK_LAUNCH();
    return 0;
}
