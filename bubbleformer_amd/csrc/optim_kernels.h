// The fused flat-buffer optimizers (AdamW, Adam, Lion) as kernel templates, shared by their two families of entry points,
// both in gradclip.hip:
//   bf_adamw / bf_adam / bf_lion              gradient scale = a host float                       (BF_OPT_HOST)
//   bf_adamw_dev / bf_adam_dev / bf_lion_dev  gradient scale = gscale * coef_dev[0] (device)      (BF_OPT_DEV)
//                                             ... and the scaled gradient clamped to +-clip       (BF_OPT_DEV_CLAMP)
// One body per optimizer: the variants differ in where the scale comes from (read once per thread, before the loop) and in one clamp on
// the scaled gradient.  BF_OPT_HOST compiles to the kernel the host-scale entry points always launched; BF_OPT_DEV runs the same loop
// body on gscale * coef_dev[0], which is gscale exactly when the coefficient is 1.0f.
#pragma once
#include <algorithm>

#include "bf_common.h"

namespace {
constexpr int BF_OPT_NT = 256;
enum { BF_OPT_HOST = 0, BF_OPT_DEV = 1, BF_OPT_DEV_CLAMP = 2 };

inline int opt_grid_for(long n) { return (int)std::max<long>(1, std::min<long>((n / 4 + 1 + BF_OPT_NT - 1) / BF_OPT_NT, 256L * 16)); }

template <int MODE>
__device__ __forceinline__ float opt_scale(float gscale, const float* __restrict__ coef) {
    if constexpr (MODE == BF_OPT_HOST) return gscale;
    else return coef ? gscale * coef[0] : gscale;
}
// the scaled gradient; the clamp keeps a NaN (both comparisons are false), as torch.clamp does
template <int MODE>
__device__ __forceinline__ float opt_grad(float g, float gs, float clip) {
    float gr = g * gs;
    if constexpr (MODE == BF_OPT_DEV_CLAMP) gr = gr > clip ? clip : (gr < -clip ? -clip : gr);
    return gr;
}

// ---------------------------------------------------------------------------- AdamW (torch.optim.AdamW semantics)
template <int MODE>
__global__ void __launch_bounds__(BF_OPT_NT) adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, long n, float lr, float b1, float b2, float eps, float wd,
                                                         float bc1, float sqrt_bc2, float gscale, const float* __restrict__ coef, float clip) {
    constexpr int NT = BF_OPT_NT;
    const float gs = opt_scale<MODE>(gscale, coef);
    const long n4 = n / 4;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long)gridDim.x * NT) {
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
#define BF_ADAM1(X)                                                        \
        { const float gr = opt_grad<MODE>(gg.X, gs, clip);                  \
          pp.X *= (1.f - lr * wd);                                          \
          mm.X = b1 * mm.X + (1.f - b1) * gr;                               \
          vv.X = b2 * vv.X + (1.f - b2) * gr * gr;                          \
          pp.X -= (lr / bc1) * mm.X / (sqrtf(vv.X) / sqrt_bc2 + eps); }
        BF_ADAM1(x) BF_ADAM1(y) BF_ADAM1(z) BF_ADAM1(w)
#undef BF_ADAM1
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
    }
    if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) {
        const long i = n4 * 4 + threadIdx.x;
        const float gr = opt_grad<MODE>(g[i], gs, clip);
        float pp = p[i] * (1.f - lr * wd);
        const float mm = b1 * m[i] + (1.f - b1) * gr;
        const float vv = b2 * v[i] + (1.f - b2) * gr * gr;
        pp -= (lr / bc1) * mm / (sqrtf(vv) / sqrt_bc2 + eps);
        p[i] = pp; m[i] = mm; v[i] = vv;
    }
}

// ---------------------------------------------------------------------------- Adam (torch.optim.Adam semantics, single-tensor path)
// Weight decay is an L2 term on the gradient (g += wd*p), so it passes through both moments; AdamW above decays the parameter instead.
// Zero padding stays zero: p = g = m = v = 0 gives m / (sqrt(v) / sqrt_bc2 + eps) = 0.
template <int MODE>
__global__ void __launch_bounds__(BF_OPT_NT) adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, long n, float lr, float b1, float b2, float eps, float wd,
                                                        float bc1, float sqrt_bc2, float gscale, const float* __restrict__ coef, float clip) {
    constexpr int NT = BF_OPT_NT;
    const float gs = opt_scale<MODE>(gscale, coef);
    const long n4 = n / 4;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long)gridDim.x * NT) {
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
#define BF_ADAML2(X)                                                       \
        { float gr = opt_grad<MODE>(gg.X, gs, clip);                        \
          if (wd != 0.f) gr += wd * pp.X;                                   \
          mm.X = b1 * mm.X + (1.f - b1) * gr;                               \
          vv.X = b2 * vv.X + (1.f - b2) * gr * gr;                          \
          pp.X -= (lr / bc1) * mm.X / (sqrtf(vv.X) / sqrt_bc2 + eps); }
        BF_ADAML2(x) BF_ADAML2(y) BF_ADAML2(z) BF_ADAML2(w)
#undef BF_ADAML2
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
    }
    if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) {
        const long i = n4 * 4 + threadIdx.x;
        float pp = p[i];
        float gr = opt_grad<MODE>(g[i], gs, clip);
        if (wd != 0.f) gr += wd * pp;
        const float mm = b1 * m[i] + (1.f - b1) * gr;
        const float vv = b2 * v[i] + (1.f - b2) * gr * gr;
        pp -= (lr / bc1) * mm / (sqrtf(vv) / sqrt_bc2 + eps);
        p[i] = pp; m[i] = mm; v[i] = vv;
    }
}

// ---------------------------------------------------------------------------- Lion (Chen et al. 2023, "Symbolic Discovery of Optimization
// Algorithms"; the update lion_pytorch.Lion applies at bubbleformer/modules.py:139-140):
//   p *= 1 - lr*wd;  p -= lr * sign(b1*m + (1-b1)*g);  m = b2*m + (1-b2)*g
template <int MODE>
__global__ void __launch_bounds__(BF_OPT_NT) lion_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, long n, float lr,
                                                        float b1, float b2, float wd, float gscale, const float* __restrict__ coef, float clip) {
    constexpr int NT = BF_OPT_NT;
    const float gs = opt_scale<MODE>(gscale, coef);
    const long n4 = n / 4;
    auto sgn = [](float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); };
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long)gridDim.x * NT) {
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i];
#define BF_LION1(X)                                                        \
        { const float gr = opt_grad<MODE>(gg.X, gs, clip);                  \
          pp.X = pp.X * (1.f - lr * wd) - lr * sgn(b1 * mm.X + (1.f - b1) * gr); \
          mm.X = b2 * mm.X + (1.f - b2) * gr; }
        BF_LION1(x) BF_LION1(y) BF_LION1(z) BF_LION1(w)
#undef BF_LION1
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
    }
    if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) {
        const long i = n4 * 4 + threadIdx.x;
        const float gr = opt_grad<MODE>(g[i], gs, clip);
        p[i] = p[i] * (1.f - lr * wd) - lr * sgn(b1 * m[i] + (1.f - b1) * gr);
        m[i] = b2 * m[i] + (1.f - b2) * gr;
    }
}

// launches, shared by both families of entry points (which check their own arguments)
#define BF_OPT_ALIGNED(x) ((uintptr_t)(x) % 16 == 0)
template <int MODE>
int opt_launch_adam(bool decoupled, float* p, const float* g, float* m, float* v, int64_t n, int step, float lr, float beta1, float beta2,
                    float eps, float wd, float gscale, const float* coef, float clip, hipStream_t st) {
    const float bc1 = 1.f - powf(beta1, (float)step);
    const float sbc2 = sqrtf(1.f - powf(beta2, (float)step));
    if (decoupled)
        hipLaunchKernelGGL(adamw_kernel<MODE>, dim3(opt_grid_for(n)), dim3(BF_OPT_NT), 0, st, p, g, m, v, (long)n, lr, beta1, beta2, eps, wd, bc1, sbc2,
                           gscale, coef, clip);
    else
        hipLaunchKernelGGL(adam_kernel<MODE>, dim3(opt_grid_for(n)), dim3(BF_OPT_NT), 0, st, p, g, m, v, (long)n, lr, beta1, beta2, eps, wd, bc1, sbc2,
                           gscale, coef, clip);
    BF_CHECK_LAUNCH();
    return 0;
}
template <int MODE>
int opt_launch_lion(float* p, const float* g, float* m, int64_t n, float lr, float beta1, float beta2, float wd, float gscale, const float* coef,
                    float clip, hipStream_t st) {
    hipLaunchKernelGGL(lion_kernel<MODE>, dim3(opt_grid_for(n)), dim3(BF_OPT_NT), 0, st, p, g, m, (long)n, lr, beta1, beta2, wd, gscale, coef, clip);
    BF_CHECK_LAUNCH();
    return 0;
}
}  // namespace
