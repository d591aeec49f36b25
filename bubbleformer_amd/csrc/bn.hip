// BatchNorm2d, GELU and MaxPool2d(2, 2) of the ClassicUnet baseline (bubbleformer/models/unets.py:186-320,
// bubbleformer/layers/conv_layers.py:96-141).  The convolutions themselves are conv.hip's.
//
// Activations are channels-last [M = B*H*W][C] in the compute dtype (fp32 or bf16); statistics are fp32, their sums fp64.
// Every streaming kernel maps a workgroup's 256 threads to CW consecutive channels x 256/CW pixel rows (CW the power of two covering
// min(C, 64)), so a wave's loads are consecutive addresses for any C, and every reduction runs in a fixed order: per-slab partial
// sums in fp64 reduced by an LDS tree over the rows, then one workgroup per channel sums the slabs (strided per thread, then an LDS
// tree).  The slab count depends on M and C only (about 2048 workgroups, enough waves in flight to stream HBM).  No float atomics:
// a training pass is bit-reproducible.  Statistics are per channel, so the kernels read sc / sh of frame 0 (the [B][C] broadcast is the
// conv prologue's layout).
//   bf_bn_fwd   batch statistics -> mean / rstd [C], the conv prologue's sc / sh [B][C], running statistics and num_batches_tracked
//   bf_bn_eval  sc / sh from the running statistics
//   bf_bn_act   a = gelu(c*sc + sh) and optionally p = maxpool2x2(a) with the window index of the maximum (2 bits, one byte)
//   bf_bn_bwd   dc from dA (+ the pooled gradient routed to the stored index), GELU' folded in; dgamma / dbeta
#include "bf_common.h"

namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_TARGET_WGS = 2048;

template <typename T>
__device__ __forceinline__ float ld(const T* p, int64_t i) { return (float)p[i]; }

int chan_width(int C) {
    int w = 1;
    while (w < C && w < 64) w <<= 1;
    return w;
}

// pixel slabs: a function of M and C only, so the reduction order (and every bit of the result) does not depend on the device; at least
// four pixels per row thread
int bn_slabs(int64_t M, int C) {
    const int CW = chan_width(C), gx = (C + CW - 1) / CW, rows = BN_THREADS / CW;
    const int64_t want = (BN_TARGET_WGS + gx - 1) / gx, most = M / (4 * rows);
    return (int)std::max<int64_t>(1, std::min(want, most));
}

// sum over slabs z of ws[z][c][0..1], in a fixed order, by the 256 threads of one workgroup per channel; the result is in r1[0], r2[0]
__device__ __forceinline__ void slab_sums(const double* __restrict__ ws, int slabs, int C, int c, double* r1, double* r2) {
    double s1 = 0.0, s2 = 0.0;
    for (int z = threadIdx.x; z < slabs; z += BN_THREADS) { s1 += ws[((int64_t)z * C + c) * 2]; s2 += ws[((int64_t)z * C + c) * 2 + 1]; }
    r1[threadIdx.x] = s1; r2[threadIdx.x] = s2;
    __syncthreads();
    for (int o = BN_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { r1[threadIdx.x] += r1[threadIdx.x + o]; r2[threadIdx.x] += r2[threadIdx.x + o]; }
        __syncthreads();
    }
}

// fixed LDS tree over the rows of a (CW x rows) block; leaves the column sums in r[0 .. CW)
__device__ __forceinline__ void tree_rows(double* r1, double* r2, int CW) {
    for (int o = BN_THREADS / 2; o >= CW; o >>= 1) {
        if ((int)threadIdx.x < o) { r1[threadIdx.x] += r1[threadIdx.x + o]; r2[threadIdx.x] += r2[threadIdx.x + o]; }
        __syncthreads();
    }
}

// ws[z][c] = {sum x, sum x^2} over the pixels of slab z.  grid (ceil(C/CW), slabs)
template <typename T>
__global__ void __launch_bounds__(BN_THREADS) bn_stats_kernel(const T* __restrict__ x, int64_t M, int C, int CW, int64_t chunk,
                                                              double* __restrict__ ws) {
    __shared__ double r1[BN_THREADS], r2[BN_THREADS];
    const int cl = threadIdx.x & (CW - 1), rl = threadIdx.x / CW, rows = BN_THREADS / CW, c = blockIdx.x * CW + cl;
    const int64_t mb = (int64_t)blockIdx.y * chunk, me = min(M, mb + chunk);
    double a1 = 0.0, a2 = 0.0;
    if (c < C)
        for (int64_t m = mb + rl; m < me; m += rows) {
            const float v = ld(x, m * C + c);
            a1 += v; a2 += (double)v * v;
        }
    r1[threadIdx.x] = a1; r2[threadIdx.x] = a2;
    __syncthreads();
    tree_rows(r1, r2, CW);
    if (rl == 0 && c < C) { ws[((int64_t)blockIdx.y * C + c) * 2] = r1[cl]; ws[((int64_t)blockIdx.y * C + c) * 2 + 1] = r2[cl]; }
}

// one workgroup per channel: slab sums -> mean, rstd, sc / sh for every frame, running statistics (PyTorch's update, unbiased
// variance), num_batches_tracked + 1
__global__ void __launch_bounds__(BN_THREADS) bn_finalize_kernel(const double* __restrict__ ws, int slabs, int64_t M, int B, int C, float eps,
                                                                 float momentum, const float* gamma, const float* beta, float* mean, float* rstd,
                                                                 float* sc, float* sh, float* rmean, float* rvar, int64_t* nbt) {
    __shared__ double r1[BN_THREADS], r2[BN_THREADS];
    const int c = blockIdx.x;
    slab_sums(ws, slabs, C, c, r1, r2);
    if (threadIdx.x != 0) return;
    const double s1 = r1[0], s2 = r2[0];
    const double n = (double)M, mu = s1 / n, var = fmax(s2 / n - mu * mu, 0.0);
    const float m = (float)mu, r = (float)(1.0 / sqrt(var + (double)eps));
    const float a = gamma[c] * r, b = beta[c] - m * a;
    mean[c] = m; rstd[c] = r;
    for (int f = 0; f < B; ++f) { sc[(int64_t)f * C + c] = a; sh[(int64_t)f * C + c] = b; }
    if (rmean) {
        rmean[c] = momentum * m + (1.0f - momentum) * rmean[c];
        rvar[c] = momentum * (float)(var * n / (n - 1.0)) + (1.0f - momentum) * rvar[c];
    }
    if (c == 0 && nbt) nbt[0] += 1;
}

// eval: sc = gamma / sqrt(running_var + eps), sh = beta - running_mean * sc, for every frame.  One thread per (frame, channel)
__global__ void bn_eval_kernel(int B, int C, float eps, const float* gamma, const float* beta, const float* rmean, const float* rvar,
                               float* sc, float* sh) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * C) return;
    const int c = i % C;
    const float r = (float)(1.0 / sqrt((double)rvar[c] + (double)eps));
    const float a = gamma[c] * r;
    sc[i] = a;
    sh[i] = beta[c] - rmean[c] * a;
}

// a = gelu(x*sc + sh), one thread per element
template <typename T>
__global__ void bn_act_kernel(const T* __restrict__ x, int C, int64_t total, const float* sc, const float* sh, T* __restrict__ a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    a[i] = (T)gelu_erff(fmaf(ld(x, i), sc[c], sh[c]));
}

// one thread per (2x2 window, channel), windows covering the frame (the last row / column of an odd frame forms partial windows that
// are activated but not pooled, as MaxPool2d(2, 2) floors).  The max is taken over the STORED activations; a later element replaces the
// running maximum only if it is strictly greater or NaN (PyTorch's rule: ties go to the first in row-major window order).
template <typename T>
__global__ void bn_act_pool_kernel(const T* __restrict__ x, int H, int W, int C, int64_t total, const float* sc, const float* sh,
                                   T* __restrict__ a, T* __restrict__ p, uint8_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int Hw = (H + 1) / 2, Ww = (W + 1) / 2, Hp = H / 2, Wp = W / 2;
    const int c = (int)(i % C);
    const int64_t q = i / C;
    const int wx = (int)(q % Ww), wy = (int)((q / Ww) % Hw), f = (int)(q / ((int64_t)Ww * Hw));
    const float s = sc[c], h = sh[c];
    float best = 0.f;
    int bi = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = 2 * wy + (j >> 1), xx = 2 * wx + (j & 1);
        if (y >= H || xx >= W) continue;
        const int64_t o = (((int64_t)f * H + y) * W + xx) * C + c;
        const T v = (T)gelu_erff(fmaf(ld(x, o), s, h));
        a[o] = v;
        const float vf = (float)v;
        if (j == 0 || vf > best || isnan(vf)) { best = vf; bi = j; }
    }
    if (wy < Hp && wx < Wp) {
        const int64_t o = (((int64_t)f * Hp + wy) * Wp + wx) * C + c;
        p[o] = (T)best;
        idx[o] = (uint8_t)bi;
    }
}

// gradient w.r.t. gelu's input at element (pixel m, channel c): (dA + the pooled gradient if this pixel is its window's argmax) * gelu'
template <typename T>
__device__ __forceinline__ float bn_grad_in(const float* dA, int64_t ldA, const T* dP, const uint8_t* idx, int m, int c, int C, int H, int W,
                                            float u) {
    float g = dA ? dA[(int64_t)m * ldA + c] : 0.f;
    if (dP) {
        const int HW = H * W, f = m / HW, r = m - f * HW, y = r / W, x = r - y * W, Hp = H / 2, Wp = W / 2;
        if ((y >> 1) < Hp && (x >> 1) < Wp) {
            const int64_t o = (((int64_t)f * Hp + (y >> 1)) * Wp + (x >> 1)) * C + c;
            if (idx[o] == ((y & 1) << 1 | (x & 1))) g += ld(dP, o);
        }
    }
    return g * dgelu_erff(u);
}

// ws[z][c] = {sum g, sum g*xhat} over slab z.  grid (ceil(C/CW), slabs)
template <typename T>
__global__ void __launch_bounds__(BN_THREADS) bn_bwd_partial_kernel(const float* __restrict__ dA, int64_t ldA, const T* __restrict__ dP,
                                                                    const uint8_t* __restrict__ idx, const T* __restrict__ x, int H, int W, int C,
                                                                    int CW, int64_t M, int64_t chunk, const float* mean, const float* rstd,
                                                                    const float* sc, const float* sh, double* __restrict__ ws) {
    __shared__ double r1[BN_THREADS], r2[BN_THREADS];
    const int cl = threadIdx.x & (CW - 1), rl = threadIdx.x / CW, rows = BN_THREADS / CW, c = blockIdx.x * CW + cl;
    const int mb = (int)(blockIdx.y * chunk), me = (int)min(M, mb + chunk);
    double a1 = 0.0, a2 = 0.0;
    if (c < C) {
        const float mu = mean[c], r = rstd[c], s = sc[c], h = sh[c];
        for (int m = mb + rl; m < me; m += rows) {
            const float v = ld(x, (int64_t)m * C + c);
            const float g = bn_grad_in(dA, ldA, dP, idx, m, c, C, H, W, fmaf(v, s, h));
            a1 += g; a2 += (double)g * ((v - mu) * r);
        }
    }
    r1[threadIdx.x] = a1; r2[threadIdx.x] = a2;
    __syncthreads();
    tree_rows(r1, r2, CW);
    if (rl == 0 && c < C) { ws[((int64_t)blockIdx.y * C + c) * 2] = r1[cl]; ws[((int64_t)blockIdx.y * C + c) * 2 + 1] = r2[cl]; }
}

// one workgroup per channel: dbeta = sum g, dgamma = sum g*xhat (slab sums); coef[c] = {sum g / M, sum g*xhat / M}
__global__ void __launch_bounds__(BN_THREADS) bn_bwd_param_kernel(const double* __restrict__ ws, int slabs, int64_t M, int C, float* dgamma,
                                                                  float* dbeta, int accumulate, float* coef) {
    __shared__ double r1[BN_THREADS], r2[BN_THREADS];
    const int c = blockIdx.x;
    slab_sums(ws, slabs, C, c, r1, r2);
    if (threadIdx.x != 0) return;
    const double s1 = r1[0], s2 = r2[0];
    dbeta[c] = accumulate ? dbeta[c] + (float)s1 : (float)s1;
    dgamma[c] = accumulate ? dgamma[c] + (float)s2 : (float)s2;
    coef[2 * c] = (float)(s1 / (double)M);
    coef[2 * c + 1] = (float)(s2 / (double)M);
}

// dx = gamma*rstd * (g - mean(g) - xhat*mean(g*xhat)) in the dtype, one thread per element
template <typename T>
__global__ void bn_bwd_apply_kernel(const float* __restrict__ dA, int64_t ldA, const T* __restrict__ dP, const uint8_t* __restrict__ idx,
                                    const T* __restrict__ x, int H, int W, int C, int64_t total, const float* gamma, const float* mean,
                                    const float* rstd, const float* sc, const float* sh, const float* coef, T* __restrict__ dx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C), m = (int)(i / C);
    const float v = ld(x, i);
    const float g = bn_grad_in(dA, ldA, dP, idx, m, c, C, H, W, fmaf(v, sc[c], sh[c]));
    const float r = rstd[c], xh = (v - mean[c]) * r;
    dx[i] = (T)(gamma[c] * r * (g - coef[2 * c] - xh * coef[2 * c + 1]));
}

}  // namespace

extern "C" int64_t bf_bn_ws_floats(int64_t M, int C) {
    if (M <= 0 || C <= 0) return -1;
    // doubles: slab partials slabs*C*2; floats: coef C*2
    return 2 * (int64_t)bn_slabs(M, C) * C * 2 + 2 * (int64_t)C;
}

extern "C" int bf_bn_fwd(int dtype, const void* x, int B, int64_t HW, int C, const float* gamma, const float* beta, float eps, float momentum,
                         float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean, float* rstd, float* sc, float* sh,
                         float* ws, bf_stream_t stream) {
    BF_REQUIRE(x && B > 0 && HW > 0 && C > 0 && gamma && beta && mean && rstd && sc && sh && ws, "bf_bn_fwd: bad arguments");
    BF_REQUIRE(dtype == BF_DTYPE_F32 || dtype == BF_DTYPE_BF16, "bf_bn_fwd: dtype");
    BF_REQUIRE(!running_mean == !running_var, "bf_bn_fwd: running_mean and running_var go together");
    const int64_t M = (int64_t)B * HW;
    BF_REQUIRE(M > 1, "bf_bn_fwd: more than one value per channel is needed in training");
    const int slabs = bn_slabs(M, C), CW = chan_width(C);
    const int64_t chunk = (M + slabs - 1) / slabs;
    const int used = (int)((M + chunk - 1) / chunk);
    hipStream_t st = (hipStream_t)stream;
    double* d = reinterpret_cast<double*>(ws);
    BfProfScope prof(st, "bn_stats", 0.0, (double)M * C * (dtype == BF_DTYPE_BF16 ? 2 : 4));
    dim3 grid((C + CW - 1) / CW, used);
    if (dtype == BF_DTYPE_BF16) hipLaunchKernelGGL((bn_stats_kernel<bf16>), grid, dim3(BN_THREADS), 0, st, (const bf16*)x, M, C, CW, chunk, d);
    else hipLaunchKernelGGL((bn_stats_kernel<float>), grid, dim3(BN_THREADS), 0, st, (const float*)x, M, C, CW, chunk, d);
    BF_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(C), dim3(BN_THREADS), 0, st, d, used, M, B, C, eps, momentum, gamma, beta, mean, rstd, sc, sh,
                       running_mean, running_var, num_batches_tracked);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_bn_eval(int B, int C, const float* gamma, const float* beta, float eps, const float* running_mean, const float* running_var,
                          float* sc, float* sh, bf_stream_t stream) {
    BF_REQUIRE(B > 0 && C > 0 && gamma && beta && running_mean && running_var && sc && sh, "bf_bn_eval: bad arguments");
    hipLaunchKernelGGL(bn_eval_kernel, dim3((B * C + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, C, eps, gamma, beta, running_mean,
                       running_var, sc, sh);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_bn_act(int dtype, const void* x, int B, int H, int W, int C, const float* sc, const float* sh, void* a, void* p, uint8_t* idx,
                         bf_stream_t stream) {
    BF_REQUIRE(x && a && sc && sh && B > 0 && H > 0 && W > 0 && C > 0, "bf_bn_act: bad arguments");
    BF_REQUIRE(dtype == BF_DTYPE_F32 || dtype == BF_DTYPE_BF16, "bf_bn_act: dtype");
    BF_REQUIRE(!p == !idx, "bf_bn_act: the pooled output needs its index buffer");
    BF_REQUIRE(!p || (H >= 2 && W >= 2), "bf_bn_act: a 2x2 pool needs H, W >= 2");
    hipStream_t st = (hipStream_t)stream;
    const int es = dtype == BF_DTYPE_BF16 ? 2 : 4;
    const int64_t n = (int64_t)B * H * W * C;
    BfProfScope prof(st, p ? "bn_act_pool" : "bn_act", 0.0, (double)n * es * 2 + (p ? (double)(n / 4) * (es + 1) : 0.0));
    if (p) {
        const int64_t total = (int64_t)B * ((H + 1) / 2) * ((W + 1) / 2) * C;
        const unsigned blocks = (unsigned)((total + 255) / 256);
        if (dtype == BF_DTYPE_BF16)
            hipLaunchKernelGGL((bn_act_pool_kernel<bf16>), dim3(blocks), dim3(256), 0, st, (const bf16*)x, H, W, C, total, sc, sh, (bf16*)a, (bf16*)p, idx);
        else hipLaunchKernelGGL((bn_act_pool_kernel<float>), dim3(blocks), dim3(256), 0, st, (const float*)x, H, W, C, total, sc, sh, (float*)a, (float*)p,
                                idx);
    } else {
        const unsigned blocks = (unsigned)((n + 255) / 256);
        if (dtype == BF_DTYPE_BF16) hipLaunchKernelGGL((bn_act_kernel<bf16>), dim3(blocks), dim3(256), 0, st, (const bf16*)x, C, n, sc, sh, (bf16*)a);
        else hipLaunchKernelGGL((bn_act_kernel<float>), dim3(blocks), dim3(256), 0, st, (const float*)x, C, n, sc, sh, (float*)a);
    }
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_bn_bwd(int dtype, const float* dA, int64_t ldA, int offA, const void* dP, const uint8_t* idx, const void* x, int B, int H, int W,
                         int C, const float* gamma, const float* mean, const float* rstd, const float* sc, const float* sh, void* dx, float* dgamma,
                         float* dbeta, int accumulate, float* ws, bf_stream_t stream) {
    BF_REQUIRE(x && dx && B > 0 && H > 0 && W > 0 && C > 0 && gamma && mean && rstd && sc && sh && dgamma && dbeta && ws, "bf_bn_bwd: bad arguments");
    BF_REQUIRE(dtype == BF_DTYPE_F32 || dtype == BF_DTYPE_BF16, "bf_bn_bwd: dtype");
    BF_REQUIRE(dA || dP, "bf_bn_bwd: no incoming gradient");
    BF_REQUIRE(!dA || (offA >= 0 && ldA >= (int64_t)offA + C), "bf_bn_bwd: dA row stride / channel offset");
    BF_REQUIRE(!dP || idx, "bf_bn_bwd: the pooled gradient needs the pool index");
    const int64_t M = (int64_t)B * H * W, total = M * C;
    BF_REQUIRE(M < (1LL << 31), "bf_bn_bwd: more than 2^31 pixels");
    const int slabs = bn_slabs(M, C), CW = chan_width(C);
    const int64_t chunk = (M + slabs - 1) / slabs;
    const int used = (int)((M + chunk - 1) / chunk);
    hipStream_t st = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(ws);
    float* coef = reinterpret_cast<float*>(part + (int64_t)used * C * 2);
    const float* dAo = dA ? dA + offA : nullptr;
    const int es = dtype == BF_DTYPE_BF16 ? 2 : 4;
    BfProfScope prof(st, "bn_bwd", 0.0, (double)total * (2.0 * es + (dA ? 8.0 : 0.0) + es) + (dP ? (double)(total / 4) * 2 * (es + 1) : 0.0));
    dim3 grid((C + CW - 1) / CW, used);
    if (dtype == BF_DTYPE_BF16)
        hipLaunchKernelGGL((bn_bwd_partial_kernel<bf16>), grid, dim3(BN_THREADS), 0, st, dAo, ldA, (const bf16*)dP, idx, (const bf16*)x, H, W, C, CW, M,
                           chunk, mean, rstd, sc, sh, part);
    else hipLaunchKernelGGL((bn_bwd_partial_kernel<float>), grid, dim3(BN_THREADS), 0, st, dAo, ldA, (const float*)dP, idx, (const float*)x, H, W, C, CW,
                            M, chunk, mean, rstd, sc, sh, part);
    BF_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_bwd_param_kernel, dim3(C), dim3(BN_THREADS), 0, st, part, used, M, C, dgamma, dbeta, accumulate, coef);
    BF_CHECK_LAUNCH();
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (dtype == BF_DTYPE_BF16)
        hipLaunchKernelGGL((bn_bwd_apply_kernel<bf16>), dim3(blocks), dim3(256), 0, st, dAo, ldA, (const bf16*)dP, idx, (const bf16*)x, H, W, C, total,
                           gamma, mean, rstd, sc, sh, coef, (bf16*)dx);
    else hipLaunchKernelGGL((bn_bwd_apply_kernel<float>), dim3(blocks), dim3(256), 0, st, dAo, ldA, (const float*)dP, idx, (const float*)x, H, W, C,
                            total, gamma, mean, rstd, sc, sh, coef, (float*)dx);
    BF_CHECK_LAUNCH();
    return 0;
}
