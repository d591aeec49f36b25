// The fused flat-buffer optimizers (AdamW, Adam, Lion) as kernel templates <MODE, AVG, GRP, GUARD>, behind one entry point each in gradclip.hip
// (bf_adamw / bf_adam / bf_lion, which take a bf_opt_step record and choose the instantiation by one rule: opt_step there).
//   MODE  where the gradient scale comes from (read once per thread, before the loop), and one clamp on the scaled gradient:
//           BF_OPT_HOST       a host float, gscale
//           BF_OPT_DEV        gscale * coef_dev[0] (device), which is gscale exactly when the coefficient is 1.0f: the same loop body
//           BF_OPT_DEV_CLAMP  ... and the scaled gradient clamped to +-clip
//   AVG   the step also moves an averaged copy `a` of the parameters towards the value it has just formed, a <- a + w * (p - a) (avg_lerp; an
//         EMA or a running mean, by the caller's w), for one more read and one more write of one buffer and no launch.  AVG = false has no
//         trace of it.  bf_weight_average is the lerp alone and bf_swap_buffers exchanges two flat buffers; same grid rule, 16-byte body,
//         scalar tail.
//   GRP   every chunk of BF_OPT_CHUNK elements carries a group id (one byte per chunk), and the group's learning-rate scale, weight decay and
//         frozen flag replace the launch's lr and wd for that chunk (opt_group_table / opt_group_of).  A 16-byte access never straddles a
//         chunk, the 16 lanes that share a chunk share the lookup, and a frozen chunk is skipped by those 16 lanes together: the live chunks
//         keep their 256-byte runs.  GRP = false has no trace of it either.
//   GUARD the launch first reads one int32 in device memory (bf_step_guard's `live`) and, where that is 0, returns before it reads or writes
//         anything else: the step is skipped on the device, with no host round trip.  The flag is uniform, so every workgroup leaves
//         together, ahead of the group table's barrier.  GUARD = false: an empty record, nothing is passed or read.
// One body per optimizer; all 3 x 3 x 2 x 2 x 2 instantiations exist (opt_launch_table).
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

// the averaged copy's update, two roundings (the difference, then one fma); w == 1 copies p bit for bit.  Written once: the fused
// bodies, their tails and avg_kernel give the same bits.  Zero padding stays zero, and a NaN in p reaches a.
__device__ __forceinline__ float avg_lerp(float a, float p, float w) { return w == 1.f ? p : __fmaf_rn(w, p - a, a); }
__device__ __forceinline__ float4 avg_lerp4(float4 a, const float4 p, float w) {
    a.x = avg_lerp(a.x, p.x, w); a.y = avg_lerp(a.y, p.y, w); a.z = avg_lerp(a.z, p.z, w); a.w = avg_lerp(a.w, p.w, w);
    return a;
}

// ---------------------------------------------------------------------------- parameter groups
// BF_OPT_CHUNK consecutive elements are one chunk (trainer.FlatParams starts every parameter on such a boundary, so a chunk belongs to
// one parameter); chunk[] names each chunk's group.  GRP = false: an empty record, nothing is passed or read.
static_assert(BF_OPT_CHUNK % 4 == 0 && BF_OPT_MAX_GROUPS <= 256, "a 16-byte access stays inside one chunk; a group id is one byte");
constexpr int BF_OPT_CHUNK4 = BF_OPT_CHUNK / 4;      // 16-byte accesses per chunk
constexpr int BF_OPT_IDS = 256;                       // every value a map byte can take has a table row: an id past n_groups is frozen
template <bool GRP> struct opt_groups {};
template <> struct opt_groups<true> {
    const uint8_t* chunk;
    const float *lr_scale, *wd;
    const uint8_t* frozen;
    int n;
};
// the workgroup's copy of the group tables in LDS, one row per possible id: {lr * lr_scale[k], weight_decay[k]}, x < 0 = frozen (a
// scale is >= 0).  Built once per workgroup, so the loop's dependent lookup is one byte from the map and one LDS read.
__device__ __forceinline__ void opt_group_table(float2* tab, const opt_groups<true>& G, float lr) {
    static_assert(BF_OPT_NT == BF_OPT_IDS, "one table row per thread");
    const int k = threadIdx.x;
    const bool live = k < G.n && !G.frozen[k];
    tab[k] = live ? make_float2(lr * G.lr_scale[k], G.wd[k]) : make_float2(-1.f, 0.f);
    __syncthreads();
}
#define BF_OPT_GROUP_TABLE()                                   \
    float2* tab = nullptr;                                     \
    if constexpr (GRP) {                                       \
        __shared__ float2 tab_lds[BF_OPT_IDS];                 \
        tab = tab_lds;                                         \
        opt_group_table(tab, G, lr);                           \
    }
// lr_k and wd_k of 16-byte access I (for element e pass e / 4); a frozen chunk takes SKIP and touches nothing
#define BF_OPT_GROUP_OF(ID, SKIP)                              \
    float lr_k = lr, wd_k = wd;                                \
    if constexpr (GRP) {                                       \
        const float2 t = tab[ID];                              \
        if (t.x < 0.f) SKIP;                                   \
        lr_k = t.x; wd_k = t.y;                                \
    }
// the grid-stride loop's id, read one trip ahead: the map byte of the next access is in flight while this one's buffers are
#define BF_OPT_GROUP_FIRST()                                   \
    int id = 0, id_next = 0;                                   \
    if constexpr (GRP) {                                       \
        const long i0 = (long)blockIdx.x * NT + threadIdx.x;   \
        if (i0 < n4) id_next = G.chunk[i0 / BF_OPT_CHUNK4];    \
    }
#define BF_OPT_GROUP_NEXT(I)                                   \
    if constexpr (GRP) {                                       \
        id = id_next;                                          \
        const long i1 = (I) + (long)gridDim.x * NT;            \
        if (i1 < n4) id_next = G.chunk[i1 / BF_OPT_CHUNK4];    \
    }

// ---------------------------------------------------------------------------- the step guard
template <bool GUARD> struct opt_guard {};
template <> struct opt_guard<true> { const int32_t* live; };
#define BF_OPT_GUARD()                                         \
    if constexpr (GUARD) {                                     \
        if (L.live[0] == 0) return;                            \
    }

// ---------------------------------------------------------------------------- AdamW (torch.optim.AdamW semantics)
template <int MODE, bool AVG, bool GRP, bool GUARD>
__global__ void __launch_bounds__(BF_OPT_NT) adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, long n, float lr, float b1, float b2, float eps, float wd,
                                                         float bc1, float sqrt_bc2, float gscale, const float* __restrict__ coef, float clip, float* __restrict__ a, float w, const opt_groups<GRP> G,
                                                         const opt_guard<GUARD> L) {
    constexpr int NT = BF_OPT_NT;
    BF_OPT_GUARD()
    BF_OPT_GROUP_TABLE()
    const float gs = opt_scale<MODE>(gscale, coef);
    const long n4 = n / 4;
    BF_OPT_GROUP_FIRST()
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long)gridDim.x * NT) {
        BF_OPT_GROUP_NEXT(i)
        BF_OPT_GROUP_OF(id, continue)
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
        float4 aa;
        if constexpr (AVG) aa = reinterpret_cast<float4*>(a)[i];
#define BF_ADAM1(X)                                                        \
        { const float gr = opt_grad<MODE>(gg.X, gs, clip);                  \
          pp.X *= (1.f - lr_k * wd_k);                                       \
          mm.X = b1 * mm.X + (1.f - b1) * gr;                               \
          vv.X = b2 * vv.X + (1.f - b2) * gr * gr;                          \
          pp.X -= (lr_k / bc1) * mm.X / (sqrtf(vv.X) / sqrt_bc2 + eps); }
        BF_ADAM1(x) BF_ADAM1(y) BF_ADAM1(z) BF_ADAM1(w)
#undef BF_ADAM1
        reinterpret_cast<float4*>(p)[i] = pp;
        if constexpr (AVG) reinterpret_cast<float4*>(a)[i] = avg_lerp4(aa, pp, w);
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
    }
    if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) {
        const long i = n4 * 4 + threadIdx.x;
        if constexpr (GRP) id = G.chunk[i / BF_OPT_CHUNK];
        BF_OPT_GROUP_OF(id, return)
        const float gr = opt_grad<MODE>(g[i], gs, clip);
        float pp = p[i] * (1.f - lr_k * wd_k);
        const float mm = b1 * m[i] + (1.f - b1) * gr;
        const float vv = b2 * v[i] + (1.f - b2) * gr * gr;
        pp -= (lr_k / bc1) * mm / (sqrtf(vv) / sqrt_bc2 + eps);
        p[i] = pp; m[i] = mm; v[i] = vv;
        if constexpr (AVG) a[i] = avg_lerp(a[i], pp, w);
    }
}

// ---------------------------------------------------------------------------- Adam (torch.optim.Adam semantics, single-tensor path)
// Weight decay is an L2 term on the gradient (g += wd*p), so it passes through both moments; AdamW above decays the parameter instead.
// Zero padding stays zero: p = g = m = v = 0 gives m / (sqrt(v) / sqrt_bc2 + eps) = 0.
template <int MODE, bool AVG, bool GRP, bool GUARD>
__global__ void __launch_bounds__(BF_OPT_NT) adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, long n, float lr, float b1, float b2, float eps, float wd,
                                                        float bc1, float sqrt_bc2, float gscale, const float* __restrict__ coef, float clip, float* __restrict__ a, float w, const opt_groups<GRP> G,
                                                         const opt_guard<GUARD> L) {
    constexpr int NT = BF_OPT_NT;
    BF_OPT_GUARD()
    BF_OPT_GROUP_TABLE()
    const float gs = opt_scale<MODE>(gscale, coef);
    const long n4 = n / 4;
    BF_OPT_GROUP_FIRST()
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long)gridDim.x * NT) {
        BF_OPT_GROUP_NEXT(i)
        BF_OPT_GROUP_OF(id, continue)
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
        float4 aa;
        if constexpr (AVG) aa = reinterpret_cast<float4*>(a)[i];
#define BF_ADAML2(X)                                                       \
        { float gr = opt_grad<MODE>(gg.X, gs, clip);                        \
          if (wd_k != 0.f) gr += wd_k * pp.X;                                \
          mm.X = b1 * mm.X + (1.f - b1) * gr;                               \
          vv.X = b2 * vv.X + (1.f - b2) * gr * gr;                          \
          pp.X -= (lr_k / bc1) * mm.X / (sqrtf(vv.X) / sqrt_bc2 + eps); }
        BF_ADAML2(x) BF_ADAML2(y) BF_ADAML2(z) BF_ADAML2(w)
#undef BF_ADAML2
        reinterpret_cast<float4*>(p)[i] = pp;
        if constexpr (AVG) reinterpret_cast<float4*>(a)[i] = avg_lerp4(aa, pp, w);
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
    }
    if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) {
        const long i = n4 * 4 + threadIdx.x;
        if constexpr (GRP) id = G.chunk[i / BF_OPT_CHUNK];
        BF_OPT_GROUP_OF(id, return)
        float pp = p[i];
        float gr = opt_grad<MODE>(g[i], gs, clip);
        if (wd_k != 0.f) gr += wd_k * pp;
        const float mm = b1 * m[i] + (1.f - b1) * gr;
        const float vv = b2 * v[i] + (1.f - b2) * gr * gr;
        pp -= (lr_k / bc1) * mm / (sqrtf(vv) / sqrt_bc2 + eps);
        p[i] = pp; m[i] = mm; v[i] = vv;
        if constexpr (AVG) a[i] = avg_lerp(a[i], pp, w);
    }
}

// ---------------------------------------------------------------------------- Lion (Chen et al. 2023, "Symbolic Discovery of Optimization
// Algorithms"; the update lion_pytorch.Lion applies at bubbleformer/modules.py:139-140):
//   p *= 1 - lr*wd;  p -= lr * sign(b1*m + (1-b1)*g);  m = b2*m + (1-b2)*g
template <int MODE, bool AVG, bool GRP, bool GUARD>
__global__ void __launch_bounds__(BF_OPT_NT) lion_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, long n, float lr,
                                                        float b1, float b2, float wd, float gscale, const float* __restrict__ coef, float clip, float* __restrict__ a, float w, const opt_groups<GRP> G,
                                                         const opt_guard<GUARD> L) {
    constexpr int NT = BF_OPT_NT;
    BF_OPT_GUARD()
    BF_OPT_GROUP_TABLE()
    const float gs = opt_scale<MODE>(gscale, coef);
    const long n4 = n / 4;
    auto sgn = [](float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); };
    BF_OPT_GROUP_FIRST()
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long)gridDim.x * NT) {
        BF_OPT_GROUP_NEXT(i)
        BF_OPT_GROUP_OF(id, continue)
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i];
        float4 aa;
        if constexpr (AVG) aa = reinterpret_cast<float4*>(a)[i];
#define BF_LION1(X)                                                        \
        { const float gr = opt_grad<MODE>(gg.X, gs, clip);                  \
          pp.X = pp.X * (1.f - lr_k * wd_k) - lr_k * sgn(b1 * mm.X + (1.f - b1) * gr); \
          mm.X = b2 * mm.X + (1.f - b2) * gr; }
        BF_LION1(x) BF_LION1(y) BF_LION1(z) BF_LION1(w)
#undef BF_LION1
        reinterpret_cast<float4*>(p)[i] = pp;
        if constexpr (AVG) reinterpret_cast<float4*>(a)[i] = avg_lerp4(aa, pp, w);
        reinterpret_cast<float4*>(m)[i] = mm;
    }
    if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) {
        const long i = n4 * 4 + threadIdx.x;
        if constexpr (GRP) id = G.chunk[i / BF_OPT_CHUNK];
        BF_OPT_GROUP_OF(id, return)
        const float gr = opt_grad<MODE>(g[i], gs, clip);
        const float pp = p[i] * (1.f - lr_k * wd_k) - lr_k * sgn(b1 * m[i] + (1.f - b1) * gr);
        p[i] = pp;
        m[i] = b2 * m[i] + (1.f - b2) * gr;
        if constexpr (AVG) a[i] = avg_lerp(a[i], pp, w);
    }
}

// ---------------------------------------------------------------------------- the averaged copy on its own, and the exchange
// a <- avg_lerp(a, p, w): what the AVG bodies do after their step, for an average taken outside the optimizer
__global__ void __launch_bounds__(BF_OPT_NT) avg_kernel(float* __restrict__ a, const float* __restrict__ p, long n, float w) {
    constexpr int NT = BF_OPT_NT;
    const long n4 = n / 4;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long)gridDim.x * NT)
        reinterpret_cast<float4*>(a)[i] = avg_lerp4(reinterpret_cast<float4*>(a)[i], reinterpret_cast<const float4*>(p)[i], w);
    if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) {
        const long i = n4 * 4 + threadIdx.x;
        a[i] = avg_lerp(a[i], p[i], w);
    }
}
// a <-> b exactly: every element is read and written by one thread (the entry point refuses overlapping buffers)
__global__ void __launch_bounds__(BF_OPT_NT) swap_kernel(float* __restrict__ a, float* __restrict__ b, long n) {
    constexpr int NT = BF_OPT_NT;
    const long n4 = n / 4;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long)gridDim.x * NT) {
        const float4 x = reinterpret_cast<float4*>(a)[i], y = reinterpret_cast<float4*>(b)[i];
        reinterpret_cast<float4*>(a)[i] = y;
        reinterpret_cast<float4*>(b)[i] = x;
    }
    if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) {
        const long i = n4 * 4 + threadIdx.x;
        const float x = a[i], y = b[i];
        a[i] = y;
        b[i] = x;
    }
}

#define BF_OPT_ALIGNED(x) ((uintptr_t)(x) % 16 == 0)
enum { BF_OPT_ADAMW = 0, BF_OPT_ADAM = 1, BF_OPT_LION = 2 };      // the update rule of a launch

// the launch of one checked step (gradclip.hip: opt_step).  Without groups the kernel gets the record's wd, with them 0 (every group brings
// its own); without an average it gets a = nullptr, w = 0.
template <int MODE, bool AVG, bool GRP, bool GUARD>
int opt_launch(int rule, const bf_opt_step& s, hipStream_t st) {
    opt_groups<GRP> G;
    if constexpr (GRP) G = {s.chunk_group, s.group_lr_scale, s.group_weight_decay, s.group_frozen, s.n_groups};
    opt_guard<GUARD> L;
    if constexpr (GUARD) L = {s.live_dev};
    const float wd = GRP ? 0.f : s.wd, w = AVG ? s.avg_weight : 0.f;
    float* a = AVG ? s.avg : nullptr;
    const dim3 grid(opt_grid_for(s.n)), block(BF_OPT_NT);
    if (rule == BF_OPT_LION) {
        hipLaunchKernelGGL((lion_kernel<MODE, AVG, GRP, GUARD>), grid, block, 0, st, s.p, s.g, s.m, (long)s.n, s.lr, s.beta1, s.beta2, wd, s.gscale, s.coef_dev,
                           s.clip_value, a, w, G, L);
    } else {
        const float bc1 = 1.f - powf(s.beta1, (float)s.step);
        const float sbc2 = sqrtf(1.f - powf(s.beta2, (float)s.step));
        if (rule == BF_OPT_ADAMW)
            hipLaunchKernelGGL((adamw_kernel<MODE, AVG, GRP, GUARD>), grid, block, 0, st, s.p, s.g, s.m, s.v, (long)s.n, s.lr, s.beta1, s.beta2, s.eps, wd, bc1,
                               sbc2, s.gscale, s.coef_dev, s.clip_value, a, w, G, L);
        else
            hipLaunchKernelGGL((adam_kernel<MODE, AVG, GRP, GUARD>), grid, block, 0, st, s.p, s.g, s.m, s.v, (long)s.n, s.lr, s.beta1, s.beta2, s.eps, wd, bc1,
                               sbc2, s.gscale, s.coef_dev, s.clip_value, a, w, G, L);
    }
    BF_CHECK_LAUNCH();
    return 0;
}
// [MODE][AVG][GRP][GUARD]: every instantiation, named once
#define BF_OPT_PAIR(MODE, AVG, GRP) {opt_launch<MODE, AVG, GRP, false>, opt_launch<MODE, AVG, GRP, true>}
#define BF_OPT_ROW(MODE) {{BF_OPT_PAIR(MODE, false, false), BF_OPT_PAIR(MODE, false, true)}, {BF_OPT_PAIR(MODE, true, false), BF_OPT_PAIR(MODE, true, true)}}
constexpr int (*opt_launch_table[3][2][2][2])(int, const bf_opt_step&, hipStream_t) = {BF_OPT_ROW(BF_OPT_HOST), BF_OPT_ROW(BF_OPT_DEV),
                                                                                       BF_OPT_ROW(BF_OPT_DEV_CLAMP)};
#undef BF_OPT_ROW
#undef BF_OPT_PAIR
}  // namespace
