// Gradient clipping for the training step, without a host round trip:
//   bf_grad_norm                             -> {norm, coef} of the flat gradient buffer in device memory (torch.nn.utils.clip_grad_norm_,
//                                               norm_type 2: what Lightning's Trainer(gradient_clip_val=...) calls)
//   bf_adamw / bf_adam / bf_lion             -> the fused optimizers of optim_kernels.h, one entry each: a bf_opt_step record says whether the
//                                               gradient scale is a host float or completed by that coefficient in device memory, whether the
//                                               scaled gradient is clamped (gradient_clip_algorithm="value"), whether an averaged copy of the
//                                               weights is kept in the same launch (EMA / SWA) and whether a group id per 64-element chunk
//                                               selects the learning-rate scale, the weight decay and a frozen flag (parameter groups)
//   bf_weight_average / bf_swap_buffers      -> the average's update alone; two flat buffers exchanged
//   bf_group_sumsq / bf_group_clip_coef      -> the norm above per group, and over the groups that are not frozen
//   bf_step_guard                            -> whether that norm is finite, as a flag in device memory the optimizers' live_dev reads (a step on
//                                               a non-finite gradient is skipped on the device), with the skip counters beside it
//   bf_nonfinite_scan                        -> where a buffer's first inf / NaN is and how many it holds (the diagnostic, outside the step)
//
// The norm is a fixed-order reduction: no float atomics, and nothing in its order depends on the device.
//   pass 1  the buffer's G = n / 4 16-byte groups are cut into slabs of gn_slab_groups(G) groups -- a function of n alone.  Workgroup s
//           sweeps slab s: thread t takes groups t, t + 256, ... of the slab with one 16-byte load each, squares in fp64 into four
//           accumulators (one per component), adds them as (x + y) + (z + w); the 64 lanes of a wave meet in an xor butterfly (1, 2, .. 32),
//           the 4 waves are added in wave order.  One fp64 partial per slab; the n % 4 trailing elements join the last slab's partial.
//   pass 2  one workgroup: thread t adds partials 4t .. 4t + 3 in order, then the same butterfly and wave order.
//           norm = fp32(gscale * sqrt(sum)) (one rounding), coef = min(max_norm / (norm + 1e-6f), 1) in fp32 with an IEEE divide.
// At most GN_MAX_SLABS partials, so pass 2 is one load per thread.
#include "optim_kernels.h"

namespace {
constexpr int GN_NT = 256;
constexpr int GN_MAX_SLABS = 1024;
constexpr long GN_MIN_SLAB_GROUPS = 1024;      // 16 KB: below this a slab is not worth a workgroup

// groups per slab: at least GN_MIN_SLAB_GROUPS, at most GN_MAX_SLABS slabs, a whole number of sweeps of the workgroup
inline long gn_slab_groups(long G) {
    const long per = std::max<long>(GN_MIN_SLAB_GROUPS, (G + GN_MAX_SLABS - 1) / GN_MAX_SLABS);
    return (per + GN_NT - 1) / GN_NT * GN_NT;
}
inline int gn_slabs(long G) { return (int)std::max<long>(1, (G + gn_slab_groups(G) - 1) / gn_slab_groups(G)); }

// not bf_common.h's wave_sum: that butterfly runs o = 32..1, this one 1..32 -- in fp64 another association, other bits
__device__ __forceinline__ double gn_wave_sum(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);      // every lane ends with the same tree over the 64 values
    return v;
}
// sum over the workgroup in a fixed order; the result is valid in thread 0.  Not bf_common.h's block_reduce: gn_wave_sum's order gives other bits
__device__ __forceinline__ double gn_block_sum(double v, double* red) {
    v = gn_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < GN_NT / 64; ++w) s += red[w];
    return s;
}

__global__ void __launch_bounds__(GN_NT) grad_sumsq_kernel(const float* __restrict__ g, long n, long slab_groups, double* __restrict__ part) {
    __shared__ double red[GN_NT / 64];
    const long G = n / 4;
    const long g0 = (long)blockIdx.x * slab_groups, g1 = min(G, g0 + slab_groups);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    double ax = 0.0, ay = 0.0, az = 0.0, aw = 0.0;
    long i = g0 + threadIdx.x;
    for (; i + 3 * GN_NT < g1; i += 4 * GN_NT) {          // four loads in flight per thread; the adds stay in group order
        float4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = g4[i + u * GN_NT];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            ax += (double)q[u].x * (double)q[u].x; ay += (double)q[u].y * (double)q[u].y;
            az += (double)q[u].z * (double)q[u].z; aw += (double)q[u].w * (double)q[u].w;
        }
    }
    for (; i < g1; i += GN_NT) {
        const float4 q = g4[i];
        ax += (double)q.x * (double)q.x; ay += (double)q.y * (double)q.y;
        az += (double)q.z * (double)q.z; aw += (double)q.w * (double)q.w;
    }
    double s = gn_block_sum((ax + ay) + (az + aw), red);
    if (threadIdx.x == 0) {
        if (blockIdx.x == gridDim.x - 1)
            for (long k = G * 4; k < n; ++k) s += (double)g[k] * (double)g[k];
        part[blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(GN_NT) grad_norm_finish_kernel(const double* __restrict__ part, int nslabs, float gscale, float max_norm,
                                                                float* __restrict__ out) {
    __shared__ double red[GN_NT / 64];
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < GN_MAX_SLABS / GN_NT; ++k) {
        const int s = threadIdx.x * (GN_MAX_SLABS / GN_NT) + k;
        if (s < nslabs) a += part[s];
    }
    const double sum = gn_block_sum(a, red);
    if (threadIdx.x == 0) {
        const float norm = (float)((double)gscale * sqrt(sum));
        const float c = __fdiv_rn(max_norm, norm + 1e-6f);
        out[0] = norm;
        out[1] = c > 1.f ? 1.f : c;                      // a NaN norm stays a NaN coefficient (torch.clamp)
    }
}

// ---------------------------------------------------------------------------- sums of squares per parameter group
// bf_group_sumsq keeps bf_grad_norm's slabs (gn_slab_groups: a function of n alone, a whole number of chunks) and its fp64 squares, but a
// slab yields one partial per group.  A wave sweeps 64 consecutive 16-byte groups = 4 chunks per load; the 16 lanes of a chunk share its
// group id.  A lane adds its squares into `a` while its chunk's group stays the same (parameters are long runs of chunks); when a run of
// lanes meets another group, the wave reduces `a` over each 16-lane run (xor 1, 2, 4, 8) and the runs that changed add theirs to the wave's
// own LDS row, run 0 first: every order here is fixed by the chunk map alone.  The 4 wave rows are added in wave order, the slab partials
// by group_sumsq_finish_kernel in a fixed order.  A map byte can take 256 values, so the LDS rows have 256 columns: an id the caller did
// not mean writes inside the row and is never read back.
constexpr int GS_IDS = 256;
constexpr int GS_RUN = BF_OPT_CHUNK / 4;      // 16 lanes share a chunk
static_assert(GN_NT % GS_RUN == 0 && 64 % GS_RUN == 0, "a slab starts on a chunk boundary and a chunk does not straddle two waves");

__device__ __forceinline__ void gs_flush(double (*acc)[GS_IDS], int wave, int lane, double a, int cur, bool flush) {
    double r = a;
#pragma unroll
    for (int o = 1; o < GS_RUN; o <<= 1) r += __shfl_xor(r, o, 64);
#pragma unroll
    for (int q = 0; q < 64 / GS_RUN; ++q)          // one run at a time: two runs of the wave may hold the same group
        if (lane == q * GS_RUN && flush && cur >= 0) acc[wave][cur] += r;
}

__global__ void __launch_bounds__(GN_NT) group_sumsq_kernel(const float* __restrict__ x, long n, long slab_groups, const uint8_t* __restrict__ chunk,
                                                           double* __restrict__ part) {
    __shared__ double acc[GN_NT / 64][GS_IDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = lane; k < GS_IDS; k += 64) acc[wave][k] = 0.0;      // a wave clears, fills and flushes its own row: no barrier before the end
    const long G = n / 4;
    const long g0 = (long)blockIdx.x * slab_groups, g1 = min(G, g0 + slab_groups);
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
    double a = 0.0;
    int cur = -1;
    for (long base = g0 + wave * 64; base < g1; base += GN_NT) {     // wave-uniform trip count: shuffles and votes see all 64 lanes
        const long i = base + lane;
        const bool run_in = (i & ~(long)(GS_RUN - 1)) < g1;           // the lane's chunk has elements below g1 (whole runs, so uniform per run)
        const int k = run_in ? (int)chunk[i / GS_RUN] : cur;
        double s = 0.0;
        if (i < g1) {
            const float4 q = x4[i];
            s = ((double)q.x * (double)q.x + (double)q.y * (double)q.y) + ((double)q.z * (double)q.z + (double)q.w * (double)q.w);
        }
        const bool changed = k != cur;
        if (__any(changed)) {
            gs_flush(acc, wave, lane, a, cur, changed);
            if (changed) { a = 0.0; cur = k; }
        }
        a += s;
    }
    gs_flush(acc, wave, lane, a, cur, true);
    __syncthreads();
    if (threadIdx.x < BF_OPT_MAX_GROUPS) {
        const int k = threadIdx.x;
        double s = acc[0][k];
#pragma unroll
        for (int w = 1; w < GN_NT / 64; ++w) s += acc[w][k];
        if (blockIdx.x == gridDim.x - 1)
            for (long e = G * 4; e < n; ++e)
                if (chunk[e / BF_OPT_CHUNK] == k) s += (double)x[e] * (double)x[e];
        part[(long)blockIdx.x * BF_OPT_MAX_GROUPS + k] = s;
    }
}

// sums[k] = the slab partials of group k: thread t adds slabs t / 64, t / 64 + 4, ... of group t % 64 in order, the four quarters in order
__global__ void __launch_bounds__(GN_NT) group_sumsq_finish_kernel(const double* __restrict__ part, int nslabs, int n_groups, double* __restrict__ sums) {
    static_assert(BF_OPT_MAX_GROUPS == 64 && GN_NT == 256, "four threads per group");
    __shared__ double red[GN_NT / BF_OPT_MAX_GROUPS][BF_OPT_MAX_GROUPS];
    const int k = threadIdx.x % BF_OPT_MAX_GROUPS, q = threadIdx.x / BF_OPT_MAX_GROUPS;
    double a = 0.0;
    for (int s = q; s < nslabs; s += GN_NT / BF_OPT_MAX_GROUPS) a += part[(long)s * BF_OPT_MAX_GROUPS + k];
    red[q][k] = a;
    __syncthreads();
    if (threadIdx.x < n_groups) sums[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}

// {norm, coef} over the groups that are not frozen, as grad_norm_finish_kernel forms them; one workgroup of BF_OPT_MAX_GROUPS threads
__global__ void __launch_bounds__(BF_OPT_MAX_GROUPS) group_clip_coef_kernel(const double* __restrict__ sums, const uint8_t* __restrict__ frozen, int n_groups,
                                                                           float gscale, float max_norm, float* __restrict__ out,
                                                                           float* __restrict__ group_norm) {
    const int t = threadIdx.x;
    if (group_norm && t < n_groups) group_norm[t] = (float)((double)gscale * sqrt(sums[t]));
    if (t == 0) {
        double sum = 0.0;
        for (int k = 0; k < n_groups; ++k)
            if (!frozen[k]) sum += sums[k];
        const float norm = (float)((double)gscale * sqrt(sum));
        const float c = __fdiv_rn(max_norm, norm + 1e-6f);
        out[0] = norm;
        out[1] = c > 1.f ? 1.f : c;                      // a NaN norm stays a NaN coefficient (torch.clamp)
    }
}

// ---------------------------------------------------------------------------- the step guard and the non-finite scan
// guard = {live, consecutive, skipped, last_skipped_step}; one lane, plain stores
__global__ void step_guard_kernel(const float* __restrict__ norm, int step, int32_t* __restrict__ guard) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool live = (__float_as_uint(norm[0]) & 0x7f800000u) != 0x7f800000u;      // isfinite, whatever the floating-point flags of the build
    guard[0] = live ? 1 : 0;
    if (live) {
        guard[1] = 0;
    } else {
        guard[1] = guard[1] + 1;
        guard[2] = guard[2] + 1;
        guard[3] = step;
    }
}

constexpr long long NF_NONE = 0x7fffffffffffffffLL;      // no non-finite element seen
// {minimum, sum} over the workgroup, valid in thread 0; integers, so any order gives the same result.  Two values at once: not bf_common.h's block_reduce
__device__ __forceinline__ void nf_block_reduce(long long& first, long long& count, long long (*red)[2]) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long f = __shfl_xor(first, o, 64), c = __shfl_xor(count, o, 64);
        first = f < first ? f : first;
        count += c;
    }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = first; red[threadIdx.x >> 6][1] = count; }
    __syncthreads();
    first = red[0][0]; count = red[0][1];
#pragma unroll
    for (int w = 1; w < GN_NT / 64; ++w) {
        first = red[w][0] < first ? red[w][0] : first;
        count += red[w][1];
    }
}
__device__ __forceinline__ void nf_take(float x, long e, long long& first, long long& count) {
    if ((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u) {
        first = e < first ? e : first;
        ++count;
    }
}

// slab s of grad_sumsq_kernel's cut: part[2 s] = the slab's smallest non-finite index (NF_NONE: none), part[2 s + 1] = how many it holds
__global__ void __launch_bounds__(GN_NT) nonfinite_slab_kernel(const float* __restrict__ x, long n, long slab_groups, long long* __restrict__ part) {
    __shared__ long long red[GN_NT / 64][2];
    const long G = n / 4;
    const long g0 = (long)blockIdx.x * slab_groups, g1 = min(G, g0 + slab_groups);
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
    long long first = NF_NONE, count = 0;
    for (long i = g0 + threadIdx.x; i < g1; i += GN_NT) {
        const float4 q = x4[i];
        nf_take(q.x, 4 * i, first, count); nf_take(q.y, 4 * i + 1, first, count);
        nf_take(q.z, 4 * i + 2, first, count); nf_take(q.w, 4 * i + 3, first, count);
    }
    nf_block_reduce(first, count, red);
    if (threadIdx.x == 0) {
        if (blockIdx.x == gridDim.x - 1)
            for (long k = G * 4; k < n; ++k) nf_take(x[k], k, first, count);
        part[2 * blockIdx.x] = first;
        part[2 * blockIdx.x + 1] = count;
    }
}

__global__ void __launch_bounds__(GN_NT) nonfinite_finish_kernel(const long long* __restrict__ part, int nslabs, long long* __restrict__ out) {
    __shared__ long long red[GN_NT / 64][2];
    long long first = NF_NONE, count = 0;
#pragma unroll
    for (int k = 0; k < GN_MAX_SLABS / GN_NT; ++k) {
        const int s = threadIdx.x * (GN_MAX_SLABS / GN_NT) + k;
        if (s < nslabs) {
            first = part[2 * s] < first ? part[2 * s] : first;
            count += part[2 * s + 1];
        }
    }
    nf_block_reduce(first, count, red);
    if (threadIdx.x == 0) {
        out[0] = first == NF_NONE ? -1 : first;
        out[1] = count;
    }
}
}  // namespace

extern "C" int64_t bf_grad_norm_ws_doubles(int64_t n) { return n > 0 ? gn_slabs((long)(n / 4)) : 0; }

extern "C" int bf_grad_norm(const float* g, int64_t n, float gscale, float max_norm, float* out, double* ws, int64_t ws_doubles,
                            bf_stream_t stream) {
    BF_REQUIRE(g && n > 0, "bf_grad_norm: bad arguments");
    BF_REQUIRE(out, "bf_grad_norm: the output {norm, coef} is null");
    BF_REQUIRE(max_norm > 0.f, "bf_grad_norm: max_norm must be positive");
    BF_REQUIRE(BF_OPT_ALIGNED(g), "bf_grad_norm: the gradient buffer must be 16-byte aligned");
    const long G = (long)(n / 4);
    const int nslabs = gn_slabs(G);
    BF_REQUIRE(ws && ws_doubles >= nslabs && (uintptr_t)ws % 8 == 0, "bf_grad_norm: the workspace is smaller than bf_grad_norm_ws_doubles(n)");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(nslabs), dim3(GN_NT), 0, st, g, (long)n, gn_slab_groups(G), ws);
    BF_CHECK_LAUNCH();
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(GN_NT), 0, st, (const double*)ws, nslabs, gscale, max_norm, out);
    BF_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------- the optimizers
// The one checked path of bf_adamw / bf_adam / bf_lion: every check of the record, each under the calling entry's name and before any HIP
// call, then the instantiation by one rule -- GRP when there is a chunk map, AVG when there is an average, GUARD when there is a guard flag, and MODE = the clamp when
// clip_value is finite (+inf = no clamp: the other two have no clamp code at all), else the device coefficient when there is one, else the
// host scale (whose bits a coefficient of 1 would give).
#define BF_OPT_REQUIRE(who, cond, what)                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            char msg[128];                                           \
            snprintf(msg, sizeof(msg), "%s: %s", who, what);         \
            return bf_fail_msg(msg, __FILE__, __LINE__);             \
        }                                                            \
    } while (0)

static int opt_step(int rule, const char* who, const bf_opt_step* s, bf_stream_t stream) {
    const bool adam = rule != BF_OPT_LION;
    BF_OPT_REQUIRE(who, s && s->p && s->g && s->m && (s->v || !adam), "null pointer");
    BF_OPT_REQUIRE(who, s->n > 0, "n must be positive");
    BF_OPT_REQUIRE(who, !adam || s->step >= 1, "step must be >= 1");
    BF_OPT_REQUIRE(who, BF_OPT_ALIGNED(s->p) && BF_OPT_ALIGNED(s->g) && BF_OPT_ALIGNED(s->m) && (!adam || BF_OPT_ALIGNED(s->v)),
                   "buffers must be 16-byte aligned");
    BF_OPT_REQUIRE(who, s->clip_value > 0.f, "clip_value must be positive (+inf: no clamp)");      // refuses a NaN too
    if (s->avg) {
        BF_OPT_REQUIRE(who, BF_OPT_ALIGNED(s->avg), "the average buffer must be 16-byte aligned");
        BF_OPT_REQUIRE(who, s->avg_weight > 0.f && s->avg_weight <= 1.f, "avg_weight must be in (0, 1]");
    }
    if (s->chunk_group) {
        BF_OPT_REQUIRE(who, s->group_lr_scale && s->group_weight_decay && s->group_frozen, "a chunk map needs the three group tables");
        BF_OPT_REQUIRE(who, s->n_groups >= 1 && s->n_groups <= BF_OPT_MAX_GROUPS, "n_groups must be 1 .. 64");
        BF_OPT_REQUIRE(who, (uintptr_t)s->group_lr_scale % 4 == 0 && (uintptr_t)s->group_weight_decay % 4 == 0, "the group tables must be 4-byte aligned");
    }
    BF_OPT_REQUIRE(who, (uintptr_t)s->live_dev % 4 == 0, "the guard flag must be 4-byte aligned");
    const int mode = !isinf(s->clip_value) ? BF_OPT_DEV_CLAMP : (s->coef_dev ? BF_OPT_DEV : BF_OPT_HOST);
    return opt_launch_table[mode][s->avg != nullptr][s->chunk_group != nullptr][s->live_dev != nullptr](rule, *s, (hipStream_t)stream);
}
#undef BF_OPT_REQUIRE

extern "C" int bf_adamw(const bf_opt_step* s, bf_stream_t stream) { return opt_step(BF_OPT_ADAMW, "bf_adamw", s, stream); }
extern "C" int bf_adam(const bf_opt_step* s, bf_stream_t stream) { return opt_step(BF_OPT_ADAM, "bf_adam", s, stream); }
extern "C" int bf_lion(const bf_opt_step* s, bf_stream_t stream) { return opt_step(BF_OPT_LION, "bf_lion", s, stream); }

extern "C" int bf_weight_average(float* avg, const float* p, int64_t n, float w, bf_stream_t stream) {
    BF_REQUIRE(avg && p && n > 0, "bf_weight_average: bad arguments");
    BF_REQUIRE(BF_OPT_ALIGNED(avg) && BF_OPT_ALIGNED(p), "bf_weight_average: buffers must be 16-byte aligned");
    BF_REQUIRE(w > 0.f && w <= 1.f, "bf_weight_average: w must be in (0, 1]");
    hipLaunchKernelGGL(avg_kernel, dim3(opt_grid_for(n)), dim3(BF_OPT_NT), 0, (hipStream_t)stream, avg, p, (long)n, w);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_swap_buffers(float* a, float* b, int64_t n, bf_stream_t stream) {
    BF_REQUIRE(a && b && n > 0, "bf_swap_buffers: bad arguments");
    BF_REQUIRE(BF_OPT_ALIGNED(a) && BF_OPT_ALIGNED(b), "bf_swap_buffers: buffers must be 16-byte aligned");
    BF_REQUIRE(a + n <= b || b + n <= a, "bf_swap_buffers: the buffers overlap");
    hipLaunchKernelGGL(swap_kernel, dim3(opt_grid_for(n)), dim3(BF_OPT_NT), 0, (hipStream_t)stream, a, b, (long)n);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t bf_group_sumsq_ws_doubles(int64_t n) { return n > 0 ? (int64_t)gn_slabs((long)(n / 4)) * BF_OPT_MAX_GROUPS : 0; }

extern "C" int bf_group_sumsq(const float* x, int64_t n, const uint8_t* chunk_group, int n_groups, double* sums, double* ws, int64_t ws_doubles,
                              bf_stream_t stream) {
    BF_REQUIRE(x && n > 0, "bf_group_sumsq: bad arguments");
    BF_REQUIRE(chunk_group && sums && (uintptr_t)sums % 8 == 0, "bf_group_sumsq: the chunk map and the output sums are required");
    BF_REQUIRE(n_groups >= 1 && n_groups <= BF_OPT_MAX_GROUPS, "bf_group_sumsq: n_groups must be 1 .. 64");
    BF_REQUIRE(BF_OPT_ALIGNED(x), "bf_group_sumsq: the buffer must be 16-byte aligned");
    const long G = (long)(n / 4);
    const int nslabs = gn_slabs(G);
    BF_REQUIRE(ws && ws_doubles >= (int64_t)nslabs * BF_OPT_MAX_GROUPS && (uintptr_t)ws % 8 == 0,
               "bf_group_sumsq: the workspace is smaller than bf_group_sumsq_ws_doubles(n)");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(group_sumsq_kernel, dim3(nslabs), dim3(GN_NT), 0, st, x, (long)n, gn_slab_groups(G), chunk_group, ws);
    BF_CHECK_LAUNCH();
    hipLaunchKernelGGL(group_sumsq_finish_kernel, dim3(1), dim3(GN_NT), 0, st, (const double*)ws, nslabs, n_groups, sums);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_group_clip_coef(const double* sums, const uint8_t* frozen, int n_groups, float gscale, float max_norm, float* out,
                                  float* group_norm, bf_stream_t stream) {
    BF_REQUIRE(sums && frozen && (uintptr_t)sums % 8 == 0, "bf_group_clip_coef: the sums and the frozen table are required");
    BF_REQUIRE(out, "bf_group_clip_coef: the output {norm, coef} is null");
    BF_REQUIRE(n_groups >= 1 && n_groups <= BF_OPT_MAX_GROUPS, "bf_group_clip_coef: n_groups must be 1 .. 64");
    BF_REQUIRE(max_norm > 0.f, "bf_group_clip_coef: max_norm must be positive");
    hipLaunchKernelGGL(group_clip_coef_kernel, dim3(1), dim3(BF_OPT_MAX_GROUPS), 0, (hipStream_t)stream, sums, frozen, n_groups, gscale, max_norm, out,
                       group_norm);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_step_guard(const float* norm, int32_t step, int32_t* guard, bf_stream_t stream) {
    BF_REQUIRE(norm && guard, "bf_step_guard: null pointer");
    BF_REQUIRE((uintptr_t)norm % 4 == 0 && (uintptr_t)guard % 4 == 0, "bf_step_guard: the norm and the guard record must be 4-byte aligned");
    hipLaunchKernelGGL(step_guard_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, norm, (int)step, guard);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t bf_nonfinite_scan_ws_len(int64_t n) { return n > 0 ? 2 * (int64_t)gn_slabs((long)(n / 4)) : 0; }

extern "C" int bf_nonfinite_scan(const float* x, int64_t n, int64_t* out, int64_t* ws, int64_t ws_len, bf_stream_t stream) {
    BF_REQUIRE(x && out, "bf_nonfinite_scan: null pointer");
    BF_REQUIRE(n > 0, "bf_nonfinite_scan: n must be positive");
    BF_REQUIRE(BF_OPT_ALIGNED(x) && (uintptr_t)out % 8 == 0, "bf_nonfinite_scan: the buffer must be 16-byte aligned and the output 8-byte aligned");
    const long G = (long)(n / 4);
    const int nslabs = gn_slabs(G);
    BF_REQUIRE(ws && ws_len >= 2 * (int64_t)nslabs && (uintptr_t)ws % 8 == 0, "bf_nonfinite_scan: the workspace is smaller than bf_nonfinite_scan_ws_len(n)");
    static_assert(sizeof(long long) == sizeof(int64_t), "the kernels' long long is the ABI's int64_t");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nonfinite_slab_kernel, dim3(nslabs), dim3(GN_NT), 0, st, x, (long)n, gn_slab_groups(G), reinterpret_cast<long long*>(ws));
    BF_CHECK_LAUNCH();
    hipLaunchKernelGGL(nonfinite_finish_kernel, dim3(1), dim3(GN_NT), 0, st, reinterpret_cast<const long long*>(ws), nslabs, reinterpret_cast<long long*>(out));
    BF_CHECK_LAUNCH();
    return 0;
}
