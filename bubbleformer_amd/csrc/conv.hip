// Convolutions, GroupNorm and the relative-L2 loss of the ModernUnet baseline (bubbleformer/models/unets.py,
// bubbleformer/layers/conv_layers.py).
//
// Activations are channels-last ([frame][y][x][C]); the first and last layers of the network may also read / write the
// reference's (B, T*C, H, W) fp32 tensors in place (bf_conv_src.nchw).  Every convolution is one implicit GEMM:
//   rows    m = output pixel (frame, oy, ox)
//   columns n = output channel
//   k         = (tap, input channel); the operand row is gathered while it is staged to LDS (never materialised), from up to
//               two channel-concatenated sources, with the optional GroupNorm affine + GELU prologue applied to in-bounds taps
//               only (padding taps are exact zeros: the reference pads the already-activated tensor).
// Two gather modes share one kernel:
//   forward    iy = oy*s - p + ky                          (Conv2d 1x1 / 3x3 s1 / 3x3 s2)
//   transposed iy = (oy + p - ky) / s, exact division only (ConvTranspose2d k4 s2 p1 = Upsample; data gradient of every conv).
//              Output pixels are split into s*s parity phases (grid z); in a phase only the taps ky = (py+p)%s + s*j can hit,
//              so a k4 s2 phase is a 2x2-tap GEMM, a k3 s2 phase a 1- or 2-tap one, and s = 1 is the flipped-kernel conv.
// The weight operand is the caller's [kh*kw][Csrc][N] matrix (weights re-laid out once per call, in the compute dtype).
// Weight gradients are a second GEMM, dW[r][(tap, c)] = sum_m R[m][r] * gather(S)[m][(tap, c)], reduced over pixels in
// slabs whose fp32 images are summed in a fixed order: no float atomics, bit-reproducible.
// MFMA: bf16 v_mfma_f32_16x16x32_bf16, fp32 v_mfma_f32_16x16x4f32 (exact fp32), issued "swapped" so that a lane holds
// 4 consecutive output columns of one row (the convention of gemm.hip).
#include "bf_common.h"

namespace {

constexpr int CBM = 64, CBN = 64, CBK = 32, CNT = 256;
constexpr int LDK = CBK + 8;     // LDS row pitch (elements): 16-byte aligned rows, k-groups spread over banks

struct Src {
    const void* p;
    int C, nchw, f32;
};

__host__ __device__ inline Src mk(const bf_conv_src* s) {
    Src r{nullptr, 0, 0, 0};
    if (s && s->p) { r.p = s->p; r.C = s->C; r.nchw = s->nchw; r.f32 = s->f32; }
    return r;
}

template <typename T>
__device__ __forceinline__ int64_t src_off(const Src& s, int f, int y, int x, int c, int H, int W) {
    return s.nchw ? (((int64_t)f * s.C + c) * H + y) * W + x : (((int64_t)f * H + y) * W + x) * s.C + c;
}
template <typename T>
__device__ __forceinline__ float src_ld(const Src& s, int f, int y, int x, int c, int H, int W) {
    const int64_t o = src_off<T>(s, f, y, x, c, H, W);
    return s.f32 ? reinterpret_cast<const float*>(s.p)[o] : (float)reinterpret_cast<const T*>(s.p)[o];
}
template <typename T>
__device__ __forceinline__ void src_st(const Src& s, int f, int y, int x, int c, int H, int W, float v) {
    const int64_t o = src_off<T>(s, f, y, x, c, H, W);
    if (s.f32) reinterpret_cast<float*>(const_cast<void*>(s.p))[o] = v;
    else reinterpret_cast<T*>(const_cast<void*>(s.p))[o] = (T)v;
}

struct Gather {
    Src s0, s1;
    int C0, Cin;               // Cin = C0 + s1.C
    int pro;                   // BF_CONV_PRO_*
    const float* sc;           // [F][Cin]
    const float* sh;
    int F, Hi, Wi, Ho, Wo, kh, kw, stride, pad;
};

// value of operand row (f, oy, ox), k = (tap, c); tap counted over the taps of the current phase (transposed mode)
template <typename T, bool TR>
__device__ __forceinline__ float gather(const Gather& g, int f, int oy, int ox, int tap, int c, int ry, int rx, int ntx) {
    int iy, ix;
    if constexpr (TR) {
        const int jy = tap / ntx, jx = tap - jy * ntx;
        const int ky = ry + g.stride * jy, kx = rx + g.stride * jx;
        const int ny = oy + g.pad - ky, nx = ox + g.pad - kx;        // divisible by stride by construction of the phase
        if (ny < 0 || nx < 0) return 0.f;
        iy = ny / g.stride; ix = nx / g.stride;
    } else {
        const int ky = tap / g.kw, kx = tap - ky * g.kw;
        iy = oy * g.stride - g.pad + ky; ix = ox * g.stride - g.pad + kx;
        if (iy < 0 || ix < 0) return 0.f;
    }
    if (iy >= g.Hi || ix >= g.Wi) return 0.f;
    float v = c < g.C0 ? src_ld<T>(g.s0, f, iy, ix, c, g.Hi, g.Wi) : src_ld<T>(g.s1, f, iy, ix, c - g.C0, g.Hi, g.Wi);
    if (g.pro == BF_CONV_PRO_AFFINE_GELU) v = gelu_erff(fmaf(v, g.sc[(int64_t)f * g.Cin + c], g.sh[(int64_t)f * g.Cin + c]));
    else if (g.pro == BF_CONV_PRO_GELU) v = gelu_erff(v);
    return v;
}

template <typename T> struct MT { typedef bf16 type; };
template <> struct MT<float> { typedef float type; };

// one 64x32 K-slab of MFMAs on the LDS tiles A[m][k], B[n][k]; 4 waves in 2x2, 32x32 per wave
template <typename T>
__device__ __forceinline__ void mma_tile(const typename MT<T>::type* As, const typename MT<T>::type* Bs, f32x4 (&acc)[2][2], int wm, int wn,
                                         int lane) {
    const int i = lane & 15, g = lane >> 4;
    if constexpr (sizeof(T) == 2) {
        bf16x8 fa[2], fb[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            fa[t] = *reinterpret_cast<const bf16x8*>(As + (wm * 32 + t * 16 + i) * LDK + 8 * g);
            fb[t] = *reinterpret_cast<const bf16x8*>(Bs + (wn * 32 + t * 16 + i) * LDK + 8 * g);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[b], fa[a], acc[a][b], 0, 0, 0);
    } else {
#pragma unroll
        for (int kk = 0; kk < CBK; kk += 4) {
            float fa[2], fb[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                fa[t] = As[(wm * 32 + t * 16 + i) * LDK + kk + g];
                fb[t] = Bs[(wn * 32 + t * 16 + i) * LDK + kk + g];
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fb[b], fa[a], acc[a][b], 0, 0, 0);
        }
    }
}

struct Epi {
    const float* bias;   // [N] or null
    Src resid;           // output geometry, N channels, or p = null
    Src out;             // output geometry, N channels
};

// forward / transposed implicit-GEMM convolution.  grid: (ceil(N/64), ceil(Mphase/64), phases)
template <typename T, bool TR>
__global__ void __launch_bounds__(CNT) conv_gemm_kernel(Gather g, const T* __restrict__ w, int N, Epi e) {
    typedef typename MT<T>::type E;
    __shared__ __attribute__((aligned(16))) E As[CBM * LDK];
    __shared__ __attribute__((aligned(16))) E Bs[CBN * LDK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    // phase geometry
    int py = 0, px = 0, ry = 0, rx = 0, nty = g.kh, ntx = g.kw, Hq = g.Ho, Wq = g.Wo, step = 1;
    if constexpr (TR) {
        step = g.stride;
        py = blockIdx.z / g.stride; px = blockIdx.z % g.stride;
        ry = (py + g.pad) % g.stride; rx = (px + g.pad) % g.stride;
        nty = (g.kh - ry + g.stride - 1) / g.stride; ntx = (g.kw - rx + g.stride - 1) / g.stride;
        Hq = (g.Ho - py + g.stride - 1) / g.stride; Wq = (g.Wo - px + g.stride - 1) / g.stride;
    }
    const int64_t Mq = (int64_t)g.F * Hq * Wq;
    const int K = nty * ntx * g.Cin;
    const int64_t m0 = (int64_t)blockIdx.y * CBM;
    const int n0 = blockIdx.x * CBN;
    if (m0 >= Mq) return;
    // the 8 rows / columns this thread stages: A element (row tid/4 + 0, k 8*(tid%4) .. +7) ... one row, 8 consecutive k
    const int ar = tid >> 2, ak = (tid & 3) * 8;
    const int64_t am = m0 + ar;
    int af = 0, aoy = 0, aox = 0;
    const bool arow = am < Mq;
    if (arow) {
        af = (int)(am / ((int64_t)Hq * Wq));
        const int rem = (int)(am - (int64_t)af * Hq * Wq);
        aoy = (rem / Wq) * step + py; aox = (rem % Wq) * step + px;
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += CBK) {
        // A: gathered activation rows
        {
            int kidx = k0 + ak;
            int tap = kidx / g.Cin, c = kidx - tap * g.Cin;
            E v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float x = 0.f;
                if (arow && kidx + j < K) x = gather<T, TR>(g, af, aoy, aox, tap, c, ry, rx, ntx);
                v[j] = (E)x;
                if (++c == g.Cin) { c = 0; ++tap; }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) As[ar * LDK + ak + j] = v[j];
        }
        // B: weight rows W[(full tap)][c][n]; thread -> column n0 + tid % 64, k rows (tid / 64) + 4*i
        {
            const int bn = tid & 63, bk = tid >> 6;
            const int n = n0 + bn;
#pragma unroll
            for (int i = 0; i < CBK / 4; ++i) {
                const int kk = bk + 4 * i, kidx = k0 + kk;
                float x = 0.f;
                if (n < N && kidx < K) {
                    const int tap = kidx / g.Cin, c = kidx - tap * g.Cin;
                    int ft = tap;
                    if constexpr (TR) {
                        const int jy = tap / ntx, jx = tap - jy * ntx;
                        ft = (ry + g.stride * jy) * g.kw + rx + g.stride * jx;
                    }
                    x = (float)w[((int64_t)ft * g.Cin + c) * N + n];
                }
                Bs[bn * LDK + kk] = (E)x;
            }
        }
        __syncthreads();
        mma_tile<T>(As, Bs, acc, wm, wn, lane);
        __syncthreads();
    }
    // epilogue: lane row (lane & 15), columns 4*(lane >> 4) + r
    const int li = lane & 15, lg = lane >> 4;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int64_t m = m0 + wm * 32 + a * 16 + li;
        if (m >= Mq) continue;
        const int f = (int)(m / ((int64_t)Hq * Wq));
        const int rem = (int)(m - (int64_t)f * Hq * Wq);
        const int oy = (rem / Wq) * step + py, ox = (rem % Wq) * step + px;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + wn * 32 + b * 16 + 4 * lg + r;
                if (n >= N) continue;
                float v = acc[a][b][r];
                if (e.bias) v += e.bias[n];
                if (e.resid.p) v += src_ld<T>(e.resid, f, oy, ox, n, g.Ho, g.Wo);
                src_st<T>(e.out, f, oy, ox, n, g.Ho, g.Wo, v);
            }
    }
}

// weight gradient slab: ws[z][r][kidx] = sum_{m in slab z} R[m][r] * gather(S)[m][kidx]   (forward-mode gather)
// grid: (ceil(K/64), ceil(R/64), slabs)
template <typename T>
__global__ void __launch_bounds__(CNT) conv_wgrad_kernel(Gather g, Src rs, int R, int64_t chunk, float* __restrict__ ws) {
    typedef typename MT<T>::type E;
    __shared__ __attribute__((aligned(16))) E As[CBM * LDK];     // [r][m]
    __shared__ __attribute__((aligned(16))) E Bs[CBN * LDK];     // [kidx][m]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int K = g.kh * g.kw * g.Cin;
    const int64_t M = (int64_t)g.F * g.Ho * g.Wo;
    const int r0 = blockIdx.y * CBM, n0 = blockIdx.x * CBN;
    const int64_t mb = (int64_t)blockIdx.z * chunk, me = min(M, mb + chunk);
    const int HW = g.Ho * g.Wo;
    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    // thread -> column (tid & 63) of the tile, pixels (tid >> 6) + 4*i
    const int col = tid & 63, pr = tid >> 6;
    const int rr = r0 + col, kidx = n0 + col;
    int tap = 0, c = 0;
    if (kidx < K) { tap = kidx / g.Cin; c = kidx - tap * g.Cin; }
    for (int64_t k0 = mb; k0 < me; k0 += CBK) {
#pragma unroll
        for (int i = 0; i < CBK / 4; ++i) {
            const int kk = pr + 4 * i;
            const int64_t m = k0 + kk;
            float a = 0.f, b = 0.f;
            if (m < me) {
                const int f = (int)(m / HW), rem = (int)(m - (int64_t)f * HW), oy = rem / g.Wo, ox = rem - oy * g.Wo;
                if (rr < R) a = src_ld<T>(rs, f, oy, ox, rr, g.Ho, g.Wo);
                if (kidx < K) b = gather<T, false>(g, f, oy, ox, tap, c, 0, 0, 0);
            }
            As[col * LDK + kk] = (E)a;
            Bs[col * LDK + kk] = (E)b;
        }
        __syncthreads();
        mma_tile<T>(As, Bs, acc, wm, wn, lane);
        __syncthreads();
    }
    const int li = lane & 15, lg = lane >> 4;
    float* out = ws + (int64_t)blockIdx.z * R * K;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int r = r0 + wm * 32 + a * 16 + li;
        if (r >= R) continue;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = n0 + wn * 32 + b * 16 + 4 * lg + q;
                if (n < K) out[(int64_t)r * K + n] = acc[a][b][q];
            }
    }
}

// out[i] (+)= sum_z ws[z][i], z ascending
__global__ void slab_sum_kernel(const float* __restrict__ ws, int slabs, int64_t n, float* __restrict__ out, int accumulate) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int z = 0; z < slabs; ++z) s += ws[(int64_t)z * n + i];
    out[i] = accumulate ? out[i] + s : s;
}

// per-channel pixel sums over a slab of pixels: ws[z][c] (bias gradients).  grid (ceil(C/64), slabs), 256 threads = 64 ch x 4 rows
template <typename T>
__global__ void __launch_bounds__(256) colsum_kernel(Src s, int F, int H, int W, int64_t chunk, float* __restrict__ ws) {
    __shared__ float red[4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    const int64_t M = (int64_t)F * H * W, mb = (int64_t)blockIdx.y * chunk, me = min(M, mb + chunk);
    float acc = 0.f;
    if (c < s.C)
        for (int64_t m = mb + rl; m < me; m += 4) {
            const int f = (int)(m / (H * W)), rem = (int)(m - (int64_t)f * H * W);
            acc += src_ld<T>(s, f, rem / W, rem % W, c, H, W);
        }
    red[rl][cl] = acc;
    __syncthreads();
    if (rl == 0 && c < s.C) ws[(int64_t)blockIdx.y * s.C + c] = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
}

// ---------------------------------------------------------------------------------------------------- GroupNorm
// statistics partials: grid (F*G, slices); double sums of x and x^2 over the slice's (pixel, channel) pairs of the group
template <typename T>
__global__ void __launch_bounds__(256) gn_stats_kernel(Src s0, Src s1, int C0, int Cin, int G, int HW, int W, int slices, double* __restrict__ ws) {
    __shared__ double r1[256], r2[256];
    const int fg = blockIdx.x, f = fg / G, gi = fg % G, cg = Cin / G;
    const int64_t n = (int64_t)HW * cg, per = (n + slices - 1) / slices;
    const int64_t b = (int64_t)blockIdx.y * per, e = min(n, b + per);
    double a1 = 0.0, a2 = 0.0;
    for (int64_t i = b + threadIdx.x; i < e; i += 256) {
        const int pix = (int)(i / cg), c = gi * cg + (int)(i % cg);
        const int y = pix / W, x = pix - y * W;
        const float v = c < C0 ? src_ld<T>(s0, f, y, x, c, HW / W, W) : src_ld<T>(s1, f, y, x, c - C0, HW / W, W);
        a1 += v; a2 += (double)v * v;
    }
    r1[threadIdx.x] = a1; r2[threadIdx.x] = a2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { r1[threadIdx.x] += r1[threadIdx.x + o]; r2[threadIdx.x] += r2[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { ws[((int64_t)fg * slices + blockIdx.y) * 2] = r1[0]; ws[((int64_t)fg * slices + blockIdx.y) * 2 + 1] = r2[0]; }
}

// one thread per (frame, channel): mean / rstd of its group (slices summed in order) -> sc = gamma*rstd, sh = beta - mean*sc
__global__ void gn_finalize_kernel(const double* __restrict__ ws, int F, int Cin, int G, int HW, int slices, float eps, const float* gamma,
                                   const float* beta, float* mean, float* rstd, float* sc, float* sh) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F * Cin) return;
    const int f = i / Cin, c = i % Cin, cg = Cin / G, gi = c / cg;
    double s1 = 0.0, s2 = 0.0;
    for (int z = 0; z < slices; ++z) {
        s1 += ws[(((int64_t)f * G + gi) * slices + z) * 2];
        s2 += ws[(((int64_t)f * G + gi) * slices + z) * 2 + 1];
    }
    const double n = (double)HW * cg, mu = s1 / n;
    const double var = fmax(s2 / n - mu * mu, 0.0);
    const float m = (float)mu, r = (float)(1.0 / sqrt(var + (double)eps));
    const float a = gamma[c] * r;
    sc[i] = a;
    sh[i] = beta[c] - m * a;
    if (c % cg == 0) { mean[f * G + gi] = m; rstd[f * G + gi] = r; }
}

// backward partials per (frame, channel, slice): sum g and sum g*xhat, g = dA * gelu'(x*sc + sh).  grid (F, ceil(Cin/64), slices)
template <typename T>
__global__ void __launch_bounds__(256) gn_bwd_partial_kernel(const float* __restrict__ dA, Src s0, Src s1, int C0, int Cin, int G, int HW, int W,
                                                             const float* mean, const float* rstd, const float* sc, const float* sh, int slices,
                                                             double* __restrict__ ws) {
    __shared__ double r1[4][64], r2[4][64];
    const int f = blockIdx.x, cl = threadIdx.x & 63, rl = threadIdx.x >> 6, c = blockIdx.y * 64 + cl;
    const int per = (HW + slices - 1) / slices, b = blockIdx.z * per, e = min(HW, b + per);
    double a1 = 0.0, a2 = 0.0;
    if (c < Cin) {
        const int gi = c / (Cin / G);
        const float mu = mean ? mean[f * G + gi] : 0.f, r = rstd ? rstd[f * G + gi] : 1.f;
        const float a = sc ? sc[f * Cin + c] : 1.f, s = sc ? sh[f * Cin + c] : 0.f;
        for (int pix = b + rl; pix < e; pix += 4) {
            const int y = pix / W, x = pix - y * W;
            const float v = c < C0 ? src_ld<T>(s0, f, y, x, c, HW / W, W) : src_ld<T>(s1, f, y, x, c - C0, HW / W, W);
            const float gv = dA[((int64_t)f * HW + pix) * Cin + c] * dgelu_erff(fmaf(v, a, s));
            a1 += gv; a2 += (double)gv * ((v - mu) * r);
        }
    }
    r1[rl][cl] = a1; r2[rl][cl] = a2;
    __syncthreads();
    if (rl == 0 && c < Cin) {
        const int64_t o = (((int64_t)blockIdx.z * gridDim.x + f) * Cin + c) * 2;
        ws[o] = ((r1[0][cl] + r1[1][cl]) + r1[2][cl]) + r1[3][cl];
        ws[o + 1] = ((r2[0][cl] + r2[1][cl]) + r2[2][cl]) + r2[3][cl];
    }
}

// one thread per channel: dgamma / dbeta (frames and slices in order) and the per-(frame, channel) totals
__global__ void gn_bwd_param_kernel(double* __restrict__ ws, int F, int Cin, int slices, float* dgamma, float* dbeta, int accumulate, double* tot) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= Cin) return;
    double g1 = 0.0, g2 = 0.0;
    for (int f = 0; f < F; ++f) {
        double a1 = 0.0, a2 = 0.0;
        for (int z = 0; z < slices; ++z) {
            a1 += ws[(((int64_t)z * F + f) * Cin + c) * 2];
            a2 += ws[(((int64_t)z * F + f) * Cin + c) * 2 + 1];
        }
        tot[((int64_t)f * Cin + c) * 2] = a1; tot[((int64_t)f * Cin + c) * 2 + 1] = a2;
        g1 += a1; g2 += a2;
    }
    if (dgamma) {
        dbeta[c] = accumulate ? dbeta[c] + (float)g1 : (float)g1;
        dgamma[c] = accumulate ? dgamma[c] + (float)g2 : (float)g2;
    }
}

// one thread per (frame, group): the two group means of gamma*g and gamma*g*xhat -> coef[f][g] = {A, B}
__global__ void gn_bwd_group_kernel(const double* __restrict__ tot, int F, int Cin, int G, int HW, const float* gamma, float* coef) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F * G) return;
    const int f = i / G, gi = i % G, cg = Cin / G;
    double a = 0.0, b = 0.0;
    for (int c = gi * cg; c < (gi + 1) * cg; ++c) {
        a += (double)gamma[c] * tot[((int64_t)f * Cin + c) * 2];
        b += (double)gamma[c] * tot[((int64_t)f * Cin + c) * 2 + 1];
    }
    const double n = (double)HW * cg;
    coef[2 * i] = (float)(a / n);
    coef[2 * i + 1] = (float)(b / n);
}

// dx = rstd * (gamma*g - A - xhat*B) (+ add); without a norm dx = g (+ add).  Split into the two concatenated sources.
template <typename T>
__global__ void gn_bwd_apply_kernel(const float* __restrict__ dA, Src s0, Src s1, int C0, int Cin, int G, int HW, int W, const float* gamma,
                                    const float* mean, const float* rstd, const float* sc, const float* sh, const float* coef, Src add,
                                    Src d0, Src d1, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % Cin);
    const int64_t mp = i / Cin;
    const int f = (int)(mp / HW), pix = (int)(mp - (int64_t)f * HW), y = pix / W, x = pix - y * W, H = HW / W;
    const float v = c < C0 ? src_ld<T>(s0, f, y, x, c, H, W) : src_ld<T>(s1, f, y, x, c - C0, H, W);
    float gv;
    if (gamma) {
        const int gi = c / (Cin / G);
        const float g = dA[i] * dgelu_erff(fmaf(v, sc[f * Cin + c], sh[f * Cin + c]));
        const float r = rstd[f * G + gi], xh = (v - mean[f * G + gi]) * r;
        gv = r * (gamma[c] * g - coef[2 * (f * G + gi)] - xh * coef[2 * (f * G + gi) + 1]);
    } else {
        gv = dA[i] * dgelu_erff(v);
    }
    if (add.p) gv += src_ld<T>(add, f, y, x, c, H, W);
    if (c < C0) src_st<T>(d0, f, y, x, c, H, W, gv);
    else src_st<T>(d1, f, y, x, c - C0, H, W, gv);
}

// ---------------------------------------------------------------------------------------------------- relative-L2 loss
// per (b, t, c) plane: sum (p - y)^2 and sum y^2 in double, fixed tree.  grid = planes
__global__ void __launch_bounds__(256) lp_plane_kernel(const float* __restrict__ p, const float* __restrict__ y, int64_t HW, double* ws) {
    __shared__ double r1[256], r2[256];
    const float* pp = p + (int64_t)blockIdx.x * HW;
    const float* yy = y + (int64_t)blockIdx.x * HW;
    double a1 = 0.0, a2 = 0.0;
    for (int64_t i = threadIdx.x; i < HW; i += 256) {
        const double d = (double)pp[i] - (double)yy[i];
        a1 += d * d; a2 += (double)yy[i] * yy[i];
    }
    r1[threadIdx.x] = a1; r2[threadIdx.x] = a2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { r1[threadIdx.x] += r1[threadIdx.x + o]; r2[threadIdx.x] += r2[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { ws[2 * blockIdx.x] = r1[0]; ws[2 * blockIdx.x + 1] = r2[0]; }
}

// LpLoss(d=2, p=2, reduce_dims=[0,1,2], reductions=[mean, mean, sum]): sum over planes of ||p-y|| / ||y||, / (B*T); coef = dloss/d(p-y) factor
__global__ void lp_final_kernel(const double* ws, int planes, int BT, float* loss, float* coef) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < planes; ++i) {
        const double dn = sqrt(ws[2 * i]), yn = sqrt(ws[2 * i + 1]);
        s += dn / yn;
        coef[i] = (float)(1.0 / ((double)BT * dn * yn));
    }
    *loss = (float)(s / BT);
}

__global__ void lp_grad_kernel(const float* __restrict__ p, const float* __restrict__ y, const float* coef, const float* dloss, int64_t HW,
                               int64_t n, float* __restrict__ dp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    dp[i] = dloss[0] * coef[i / HW] * (p[i] - y[i]);
}

Gather mk_gather(const bf_conv_geo* g, const bf_conv_src* s0, const bf_conv_src* s1, int pro, const float* sc, const float* sh) {
    Gather r;
    r.s0 = mk(s0); r.s1 = mk(s1);
    r.C0 = r.s0.C; r.Cin = r.s0.C + r.s1.C;
    r.pro = pro; r.sc = sc; r.sh = sh;
    r.F = g->F; r.Hi = g->Hi; r.Wi = g->Wi; r.Ho = g->Ho; r.Wo = g->Wo; r.kh = g->kh; r.kw = g->kw; r.stride = g->stride; r.pad = g->pad;
    return r;
}

int check_geo(const bf_conv_geo* g) {
    if (!g || g->F <= 0 || g->Hi <= 0 || g->Wi <= 0 || g->Ho <= 0 || g->Wo <= 0 || g->kh <= 0 || g->kw <= 0 || g->stride <= 0 || g->pad < 0)
        return bf_fail_msg("bf_conv: bad geometry", __FILE__, __LINE__);
    return 0;
}

int wgrad_slabs(int R, int K, int64_t M) {
    const int64_t tiles = (int64_t)((R + CBM - 1) / CBM) * ((K + CBN - 1) / CBN);
    int64_t s = (512 + tiles - 1) / tiles;                       // about two workgroups per CU in all
    s = std::min<int64_t>(s, (M + 8 * CBK - 1) / (8 * CBK));      // at least 8 K-steps per slab
    s = std::min<int64_t>(s, 64);
    while (s > 1 && s * R * (int64_t)K > (int64_t)64 << 20) --s;  // workspace bound: 256 MB
    return (int)std::max<int64_t>(s, 1);
}

constexpr int COLSUM_SLABS = 64;
constexpr int GN_SLICES = 32;

}  // namespace

extern "C" int bf_conv_fwd(int dtype, const bf_conv_geo* geo, const bf_conv_src* s0, const bf_conv_src* s1, int pro, const float* sc,
                           const float* sh, const void* w, int N, const float* bias, const bf_conv_src* resid, const bf_conv_src* out,
                           int transposed, bf_stream_t stream) {
    if (int rc = check_geo(geo)) return rc;
    BF_REQUIRE(s0 && s0->p && out && out->p && w && N > 0, "bf_conv_fwd: null operand");
    BF_REQUIRE(dtype == BF_DTYPE_F32 || dtype == BF_DTYPE_BF16, "bf_conv_fwd: dtype");
    BF_REQUIRE(pro != BF_CONV_PRO_AFFINE_GELU || (sc && sh), "bf_conv_fwd: prologue needs sc / sh");
    BF_REQUIRE(!transposed || pro == BF_CONV_PRO_NONE, "bf_conv_fwd: the transposed gather has no prologue");
    Gather g = mk_gather(geo, s0, s1, pro, sc, sh);
    Epi e{bias, mk(resid), mk(out)};
    e.out.C = N;
    if (e.resid.p) e.resid.C = N;
    hipStream_t st = (hipStream_t)stream;
    const int ph = transposed ? geo->stride * geo->stride : 1;
    const int64_t Mq = transposed ? (int64_t)geo->F * ((geo->Ho + geo->stride - 1) / geo->stride) * ((geo->Wo + geo->stride - 1) / geo->stride)
                                  : (int64_t)geo->F * geo->Ho * geo->Wo;
    BF_REQUIRE((Mq + CBM - 1) / CBM < 65536 * 32768LL, "bf_conv_fwd: too many rows");
    dim3 grid((N + CBN - 1) / CBN, (unsigned)((Mq + CBM - 1) / CBM), ph);
    BfProfScope prof(st, transposed ? "conv_t" : "conv_fwd",
                     2.0 * geo->F * geo->Ho * geo->Wo * (double)N * g.Cin * geo->kh * geo->kw / (transposed ? geo->stride * geo->stride : 1), 0.0);
    if (dtype == BF_DTYPE_BF16) {
        if (transposed) hipLaunchKernelGGL((conv_gemm_kernel<bf16, true>), grid, dim3(CNT), 0, st, g, (const bf16*)w, N, e);
        else hipLaunchKernelGGL((conv_gemm_kernel<bf16, false>), grid, dim3(CNT), 0, st, g, (const bf16*)w, N, e);
    } else {
        if (transposed) hipLaunchKernelGGL((conv_gemm_kernel<float, true>), grid, dim3(CNT), 0, st, g, (const float*)w, N, e);
        else hipLaunchKernelGGL((conv_gemm_kernel<float, false>), grid, dim3(CNT), 0, st, g, (const float*)w, N, e);
    }
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t bf_conv_wgrad_ws_floats(int R, int K, int64_t M) {
    if (R <= 0 || K <= 0 || M <= 0) return -1;
    const int s = wgrad_slabs(R, K, M);
    return (int64_t)s * R * K + (int64_t)COLSUM_SLABS * std::max(R, K);
}

extern "C" int bf_conv_wgrad(int dtype, const bf_conv_geo* geo, const bf_conv_src* rows, const bf_conv_src* s0, const bf_conv_src* s1, int pro,
                             const float* sc, const float* sh, float* dw, int accumulate, float* ws, int64_t ws_floats, bf_stream_t stream) {
    if (int rc = check_geo(geo)) return rc;
    BF_REQUIRE(rows && rows->p && s0 && s0->p && dw && ws, "bf_conv_wgrad: null operand");
    BF_REQUIRE(dtype == BF_DTYPE_F32 || dtype == BF_DTYPE_BF16, "bf_conv_wgrad: dtype");
    BF_REQUIRE(pro != BF_CONV_PRO_AFFINE_GELU || (sc && sh), "bf_conv_wgrad: prologue needs sc / sh");
    Gather g = mk_gather(geo, s0, s1, pro, sc, sh);
    Src rs = mk(rows);
    const int R = rs.C, K = geo->kh * geo->kw * g.Cin;
    const int64_t M = (int64_t)geo->F * geo->Ho * geo->Wo;
    BF_REQUIRE(ws_floats >= bf_conv_wgrad_ws_floats(R, K, M), "bf_conv_wgrad: workspace too small");
    const int slabs = wgrad_slabs(R, K, M);
    const int64_t chunk = ((M + slabs - 1) / slabs + CBK - 1) / CBK * CBK;
    const int used = (int)((M + chunk - 1) / chunk);
    hipStream_t st = (hipStream_t)stream;
    BfProfScope prof(st, "conv_wgrad", 2.0 * M * (double)R * K, 0.0);
    dim3 grid((K + CBN - 1) / CBN, (R + CBM - 1) / CBM, used);
    if (dtype == BF_DTYPE_BF16) hipLaunchKernelGGL((conv_wgrad_kernel<bf16>), grid, dim3(CNT), 0, st, g, rs, R, chunk, ws);
    else hipLaunchKernelGGL((conv_wgrad_kernel<float>), grid, dim3(CNT), 0, st, g, rs, R, chunk, ws);
    BF_CHECK_LAUNCH();
    const int64_t n = (int64_t)R * K;
    hipLaunchKernelGGL(slab_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ws, used, n, dw, accumulate);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_conv_colsum(int dtype, const bf_conv_src* src, int F, int H, int W, float* out, int accumulate, float* ws, int64_t ws_floats,
                              bf_stream_t stream) {
    BF_REQUIRE(src && src->p && out && ws && F > 0 && H > 0 && W > 0 && src->C > 0, "bf_conv_colsum: bad arguments");
    BF_REQUIRE(ws_floats >= (int64_t)COLSUM_SLABS * src->C, "bf_conv_colsum: workspace too small");
    Src s = mk(src);
    const int64_t M = (int64_t)F * H * W, chunk = (M + COLSUM_SLABS - 1) / COLSUM_SLABS;
    const int used = (int)((M + chunk - 1) / chunk);
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((s.C + 63) / 64, used);
    if (dtype == BF_DTYPE_BF16) hipLaunchKernelGGL((colsum_kernel<bf16>), grid, dim3(256), 0, st, s, F, H, W, chunk, ws);
    else hipLaunchKernelGGL((colsum_kernel<float>), grid, dim3(256), 0, st, s, F, H, W, chunk, ws);
    BF_CHECK_LAUNCH();
    hipLaunchKernelGGL(slab_sum_kernel, dim3((s.C + 255) / 256), dim3(256), 0, st, ws, used, (int64_t)s.C, out, accumulate);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t bf_gn_ws_floats(int F, int C, int G) {
    if (F <= 0 || C <= 0 || G <= 0) return -1;
    // doubles: stats partials F*G*SL*2, backward partials SL*F*C*2 + totals F*C*2; floats: coef F*G*2
    const int64_t dbl = std::max<int64_t>((int64_t)F * G * GN_SLICES * 2, (int64_t)GN_SLICES * F * C * 2 + (int64_t)F * C * 2);
    return 2 * dbl + (int64_t)F * G * 2;
}

extern "C" int bf_gn_fwd(int dtype, const bf_conv_src* s0, const bf_conv_src* s1, int F, int H, int W, int G, const float* gamma, const float* beta,
                         float eps, float* mean, float* rstd, float* sc, float* sh, float* ws, bf_stream_t stream) {
    Src a = mk(s0), b = mk(s1);
    const int C = a.C + b.C;
    BF_REQUIRE(a.p && F > 0 && H > 0 && W > 0 && G > 0 && C % G == 0 && gamma && beta && mean && rstd && sc && sh && ws, "bf_gn_fwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    double* d = reinterpret_cast<double*>(ws);
    if (dtype == BF_DTYPE_BF16)
        hipLaunchKernelGGL((gn_stats_kernel<bf16>), dim3(F * G, GN_SLICES), dim3(256), 0, st, a, b, a.C, C, G, H * W, W, GN_SLICES, d);
    else hipLaunchKernelGGL((gn_stats_kernel<float>), dim3(F * G, GN_SLICES), dim3(256), 0, st, a, b, a.C, C, G, H * W, W, GN_SLICES, d);
    BF_CHECK_LAUNCH();
    hipLaunchKernelGGL(gn_finalize_kernel, dim3((F * C + 255) / 256), dim3(256), 0, st, d, F, C, G, H * W, GN_SLICES, eps, gamma, beta, mean, rstd,
                       sc, sh);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_gn_bwd(int dtype, const float* dA, const bf_conv_src* s0, const bf_conv_src* s1, int F, int H, int W, int G, const float* gamma,
                         const float* mean, const float* rstd, const float* sc, const float* sh, const bf_conv_src* add, const bf_conv_src* dx0,
                         const bf_conv_src* dx1, float* dgamma, float* dbeta, int accumulate, float* ws, bf_stream_t stream) {
    Src a = mk(s0), b = mk(s1), ad = mk(add), d0 = mk(dx0), d1 = mk(dx1);
    const int C = a.C + b.C;
    BF_REQUIRE(dA && a.p && d0.p && (b.C == 0 || d1.p) && F > 0 && H > 0 && W > 0 && G > 0 && C % G == 0, "bf_gn_bwd: bad arguments");
    BF_REQUIRE(!gamma || (mean && rstd && sc && sh && dgamma && dbeta && ws), "bf_gn_bwd: a norm needs its statistics and gradients");
    d0.C = a.C; d1.C = b.C;
    if (ad.p) ad.C = C;
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W;
    float* coef = nullptr;
    if (gamma) {
        double* part = reinterpret_cast<double*>(ws);
        double* tot = part + (int64_t)GN_SLICES * F * C * 2;
        coef = reinterpret_cast<float*>(tot + (int64_t)F * C * 2);
        const int sl = std::min(GN_SLICES, HW);
        dim3 grid(F, (C + 63) / 64, sl);
        if (dtype == BF_DTYPE_BF16)
            hipLaunchKernelGGL((gn_bwd_partial_kernel<bf16>), grid, dim3(256), 0, st, dA, a, b, a.C, C, G, HW, W, mean, rstd, sc, sh, sl, part);
        else hipLaunchKernelGGL((gn_bwd_partial_kernel<float>), grid, dim3(256), 0, st, dA, a, b, a.C, C, G, HW, W, mean, rstd, sc, sh, sl, part);
        BF_CHECK_LAUNCH();
        hipLaunchKernelGGL(gn_bwd_param_kernel, dim3((C + 255) / 256), dim3(256), 0, st, part, F, C, sl, dgamma, dbeta, accumulate, tot);
        BF_CHECK_LAUNCH();
        hipLaunchKernelGGL(gn_bwd_group_kernel, dim3((F * G + 255) / 256), dim3(256), 0, st, tot, F, C, G, HW, gamma, coef);
        BF_CHECK_LAUNCH();
    }
    const int64_t total = (int64_t)F * HW * C;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (dtype == BF_DTYPE_BF16)
        hipLaunchKernelGGL((gn_bwd_apply_kernel<bf16>), dim3(blocks), dim3(256), 0, st, dA, a, b, a.C, C, G, HW, W, gamma, mean, rstd, sc, sh, coef,
                           ad, d0, d1, total);
    else hipLaunchKernelGGL((gn_bwd_apply_kernel<float>), dim3(blocks), dim3(256), 0, st, dA, a, b, a.C, C, G, HW, W, gamma, mean, rstd, sc, sh,
                            coef, ad, d0, d1, total);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_unet_lploss_fwd(const float* pred, const float* target, int B, int T, int C, int64_t HW, float* loss, float* coef, float* ws,
                                  bf_stream_t stream) {
    BF_REQUIRE(pred && target && loss && coef && ws && B > 0 && T > 0 && C > 0 && HW > 0, "bf_unet_lploss_fwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int planes = B * T * C;
    hipLaunchKernelGGL(lp_plane_kernel, dim3(planes), dim3(256), 0, st, pred, target, HW, reinterpret_cast<double*>(ws));
    BF_CHECK_LAUNCH();
    hipLaunchKernelGGL(lp_final_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<const double*>(ws), planes, B * T, loss, coef);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_unet_lploss_bwd(const float* pred, const float* target, const float* coef, const float* dloss, int planes, int64_t HW,
                                  float* dpred, bf_stream_t stream) {
    BF_REQUIRE(pred && target && coef && dloss && dpred && planes > 0 && HW > 0, "bf_unet_lploss_bwd: bad arguments");
    const int64_t n = (int64_t)planes * HW;
    hipLaunchKernelGGL(lp_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pred, target, coef, dloss, HW, n, dpred);
    BF_CHECK_LAUNCH();
    return 0;
}
