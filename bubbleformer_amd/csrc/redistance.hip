// Redistancing (reinitialisation) of a signed-distance field: phi is replaced by the signed distance to phi's own zero level set, first order.
// The reference has no program for this; DESIGN.md section 25 has the definition.  Per frame phi [H][W] fp32 in physical units, spacing h:
//   sign      vapour (+) iff phi > 0, an exact zero is liquid (-): the census' convention;
//   interface a cell with a 4-neighbour of the other sign is frozen at d = the distance to the linearly interpolated crossings:
//             t = h |phi_c| / (|phi_c| + |phi_n|) per such neighbour, tx / ty the smaller per axis, d = t with one axis, 1 / sqrt(1/tx^2 + 1/ty^2) with both;
//   the rest  start at +inf and take the fixed point of the Godunov upwind update of |grad d| = 1 (a = min(left, right), b = min(up, down),
//             u = lo + h when hi is absent or hi - lo >= h, else (lo + hi + sqrt(2 h^2 - (hi - lo)^2)) / 2, capped at `band`), replaced only by a
//             strictly smaller u, passes until one changes nothing;
//   output    +d on vapour, -d on liquid cells.
//
// One workgroup of 1024 threads owns a frame from start to end, so no two workgroups ever exchange data.  The distances (one fp32 per cell,
// the sign bit set on a frozen cell: a distance is never negative) live in dynamic LDS when the frame has at most REDIST_LDS_CELLS cells, in a
// slice of the caller's workspace otherwise; there every access is an agent-scope atomic (served by the L2, never by this CU's L1) and every
// barrier first waits for the wave's own stores.  A pass is two checkerboard half-passes in place: a cell of colour (x + y) & 1 reads only
// cells of the other colour, so a half-pass has no race and the result is the same bits on every call, alone or in a batch.  The two colours
// are two compact planes (cell i = y W + x lies at [colour][i >> 1]): the lanes of a wave then read and write consecutive dwords, where a
// stride-2 walk over one row-major plane would put two lanes of every 32-lane group on each of ds_read_b32's 32 banks.  Every loop is bounded
// by max_rounds or a cell count; convergence is one workgroup-wide vote per pass.  No float atomics; fp32 distances without contraction (the
// Makefile compiles this file with -ffp-contract=off), fp64 for change_rms in a fixed order.
#include "clip_store.h"
#include "lane_ops.h"

namespace {
constexpr int NT = 1024;
constexpr int NW = NT / 64;
constexpr int REDIST_LDS_CELLS = 40704;            // 159 KiB of distances; the last KiB of the CU's 160 is for the vote's and the sum's statics
constexpr long REDIST_MAX_CELLS = 1L << 24;        // cell indices are exact in fp32 (the row / column split below) and int32 with room to spare

typedef __attribute__((address_space(1))) unsigned guint;
#define BF_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct LdsDist {
    unsigned* L;
    __device__ __forceinline__ unsigned ld(int i) const { return L[i]; }
    __device__ __forceinline__ void st(int i, unsigned v) const { L[i] = v; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};
struct GlobalDist {
    guint* L;
    __device__ __forceinline__ unsigned ld(int i) const { return __hip_atomic_load(L + i, BF_RLX_AGENT); }
    __device__ __forceinline__ void st(int i, unsigned v) const { __hip_atomic_store(L + i, v, BF_RLX_AGENT); }
    __device__ __forceinline__ void sync() const { drain_vm(); __syncthreads(); }      // the wave's stores have reached the L2 before anybody goes on
};

constexpr unsigned FROZEN = 0x80000000u;
constexpr unsigned INF_BITS = 0x7f800000u;

// m = y * w + x with 0 <= x < w, for m < 2^24: the fp32 quotient is off by at most one
__device__ __forceinline__ void split(int m, int w, float inv_w, int& y, int& x) {
    y = (int)((float)m * inv_w);
    x = m - y * w;
    if (x < 0) { --y; x += w; }
    else if (x >= w) { ++y; x -= w; }
}

// the physical field of a frame, plain or the de-normalised channel of a prediction
struct PhiSrc {
    const float* p; bool denorm; float q, d;
    __device__ __forceinline__ float at(int i) const { const float v = p[i]; return denorm ? denormalise(v, q, d) : v; }
};

__device__ __forceinline__ float crossing(float h, float ac, float an) { return h * ac / (ac + an); }

// one frame, start to end; rounds_out / change_out as include/bubbleformer_hip.h documents them.  write(i, v) stores cell i of the result
template <class D, class Write>
__device__ void redistance_frame(const D dist, const PhiSrc src, Write write, bool copy_unchanged, int H, int W, float h, float band, int max_rounds,
                                 int* rounds_out, float* change_out) {
    __shared__ int s_flag[2];
    __shared__ int s_count[2];
    __shared__ double s_sum[NW];      // added from 0.0 by one thread in this kernel's own order, which its restatement's bits pin: not bf_common.h's block_reduce
    const int n = H * W, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int plane1 = (n + 1) >> 1;                                        // where the cells of colour 1 begin
    const float inv_W = 1.f / (float)W, inf = __uint_as_float(INF_BITS);
    if (tid == 0) { s_flag[0] = 0; s_flag[1] = 0; s_count[0] = 0; s_count[1] = 0; }
    __syncthreads();
    // 1: the frozen interface cells, +inf elsewhere; non-finite values and interface cells are counted
    int bad = 0, iface = 0;
    for (int i = tid; i < n; i += NT) {
        int y, x;
        split(i, W, inv_W, y, x);
        const float c = src.at(i);
        const bool pos = c > 0.f;
        const float ac = fabsf(c);
        bad += !(ac < inf);                                                 // NaN or inf
        float tx = inf, ty = inf;
        if (x > 0) { const float v = src.at(i - 1); if ((v > 0.f) != pos) tx = fminf(tx, crossing(h, ac, fabsf(v))); }
        if (x < W - 1) { const float v = src.at(i + 1); if ((v > 0.f) != pos) tx = fminf(tx, crossing(h, ac, fabsf(v))); }
        if (y > 0) { const float v = src.at(i - W); if ((v > 0.f) != pos) ty = fminf(ty, crossing(h, ac, fabsf(v))); }
        if (y < H - 1) { const float v = src.at(i + W); if ((v > 0.f) != pos) ty = fminf(ty, crossing(h, ac, fabsf(v))); }
        unsigned bits = INF_BITS;
        if (tx < inf || ty < inf) {
            float d;
            if (!(ty < inf)) d = tx;
            else if (!(tx < inf)) d = ty;
            else if (tx == 0.f || ty == 0.f) d = 0.f;
            else d = 1.f / sqrtf(1.f / (tx * tx) + 1.f / (ty * ty));
            bits = __float_as_uint(d) | FROZEN;
            ++iface;
        }
        dist.st(((x + y) & 1) * plane1 + (i >> 1), bits);
    }
    if (__any(bad) && lane == 0) s_count[0] = 1;
    if (__any(iface) && lane == 0) s_count[1] = 1;
    dist.sync();
    int status;
    if (s_count[0]) status = -1;
    else if (!s_count[1]) status = 0;
    else {
        // 2: checkerboard passes until a quiet one.  Colour c's cells are plane indices k < (n + 1 - c) / 2; with an even W cell k of a plane is
        // (y, 2 (k mod W/2) + ((y + c) & 1)), with an odd W it is cell i = 2 k + c of the frame
        const bool even = (W & 1) == 0;
        const int wd = even ? W >> 1 : W;
        const float inv_wd = 1.f / (float)wd;
        const float two_h2 = 2.f * h * h;
        status = -2;
        for (int r = 1; r <= max_rounds; ++r) {
            int changed = 0;
            for (int c = 0; c < 2; ++c) {
                const int mine = c * plane1, other = plane1 - mine, cells = (n + 1 - c) >> 1;
                for (int k = tid; k < cells; k += NT) {
                    // the five loads are issued together, whatever the cell: a neighbour outside the frame reads the cell itself and counts as
                    // +inf, a frozen cell computes and stores nothing (one LDS round trip per cell, not one per neighbour)
                    int y, x;
                    split(even ? k : 2 * k + c, wd, inv_wd, y, x);
                    if (even) x = 2 * x + ((y + c) & 1);
                    const int i = y * W + x, self = mine + k;
                    const bool has_l = x > 0, has_r = x < W - 1, has_u = y > 0, has_d = y < H - 1;
                    const unsigned own = dist.ld(self);
                    const unsigned vl = dist.ld(has_l ? other + ((i - 1) >> 1) : self), vr = dist.ld(has_r ? other + ((i + 1) >> 1) : self);
                    const unsigned vu = dist.ld(has_u ? other + ((i - W) >> 1) : self), vd = dist.ld(has_d ? other + ((i + W) >> 1) : self);
                    const float a = fminf(has_l ? __uint_as_float(vl & ~FROZEN) : inf, has_r ? __uint_as_float(vr & ~FROZEN) : inf);
                    const float b = fminf(has_u ? __uint_as_float(vu & ~FROZEN) : inf, has_d ? __uint_as_float(vd & ~FROZEN) : inf);
                    const float lo = fminf(a, b), hi = fmaxf(a, b);
                    float u;
                    if (!(hi < inf) || hi - lo >= h) u = lo + h;
                    else { const float df = hi - lo; u = (lo + hi + sqrtf(two_h2 - df * df)) * 0.5f; }
                    if (band > 0.f) u = fminf(u, band);
                    if (!(own & FROZEN) && u < __uint_as_float(own)) { dist.st(self, __float_as_uint(u)); changed = 1; }
                }
                if (c == 0) dist.sync();
            }
            if (__any(changed) && lane == 0) s_flag[r & 1] = 1;
            dist.sync();
            const int any = s_flag[r & 1];
            if (tid == 0) s_flag[(r + 1) & 1] = 0;                           // nobody sets it before the next pass's first barrier
            if (!any) { status = r; break; }
        }
    }
    // 3: the signed result and the root mean square change, fp64 per thread in cell order, then over the lanes and the waves in a fixed order
    double acc = 0.0;
    if (status > 0 || status == -2) {
        const float unreached = band > 0.f ? band : (float)(H + W) * h;
        for (int i = tid; i < n; i += NT) {
            int y, x;
            split(i, W, inv_W, y, x);
            float d = __uint_as_float(dist.ld(((x + y) & 1) * plane1 + (i >> 1)) & ~FROZEN);
            if (!(d < inf)) d = unreached;
            const float old = src.at(i);
            const float v = old > 0.f ? d : -d;
            write(i, v);
            const double e = (double)v - (double)old;
            acc += e * e;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) s_sum[wave] = acc;
        __syncthreads();
        acc = 0.0;
        for (int w = 0; w < NW; ++w) acc += s_sum[w];
    } else if (copy_unchanged) {
        for (int i = tid; i < n; i += NT) write(i, src.at(i));
    }
    if (tid == 0) {
        if (rounds_out) *rounds_out = status;
        if (change_out) *change_out = (float)sqrt(acc / (double)n);
    }
}

template <class D> __device__ __forceinline__ D dist_at(char* ws_slot);
template <> __device__ __forceinline__ LdsDist dist_at<LdsDist>(char*) {
    extern __shared__ unsigned redistance_cells[];
    return LdsDist{redistance_cells};
}
template <> __device__ __forceinline__ GlobalDist dist_at<GlobalDist>(char* ws_slot) { return GlobalDist{(guint*)ws_slot}; }

struct RedistanceArgs {
    const float* phi; float* out; int H, W; float h, band; int max_rounds;
    int* rounds; float* change; char* ws; long slot;
};

template <class D> __global__ void __launch_bounds__(NT) redistance_kernel(RedistanceArgs a) {
    const long f = blockIdx.x, n = (long)a.H * a.W;
    float* const out = a.out + f * n;
    const PhiSrc src{a.phi + f * n, false, 1.f, 0.f};
    redistance_frame(dist_at<D>(a.ws + f * a.slot), src, [out](int i, float v) { out[i] = v; }, a.out != a.phi, a.H, a.W, a.h, a.band, a.max_rounds,
                     a.rounds ? a.rounds + f : nullptr, a.change ? a.change + f : nullptr);
}

struct RolloutRedistanceArgs {
    RolloutStep v; float* pred;
    int sdf_c, every; float h, band; int max_rounds;
    int* rounds; float* change; char* ws; long slot;
};

template <class D> __global__ void __launch_bounds__(NT) rollout_redistance_kernel(RolloutRedistanceArgs a) {
    const RolloutStep& v = a.v;
    const int s = v.current();
    if (s < 0) return;                                                     // behind the last row: nothing is written
    const int bt = blockIdx.x, t = bt % v.T, b = bt / v.T;
    const long row = v.row(s, b, t);
    if ((s + 1) % a.every != 0) {                                          // a step the correction skips: the prediction stays as the model left it
        if (threadIdx.x == 0) {
            if (a.rounds) a.rounds[row] = 0;
            if (a.change) a.change[row] = 0.f;
        }
        return;
    }
    const long off = ((long)bt * v.C + a.sdf_c) * ((long)v.Ho * v.Wo);
    const float q = v.dv[a.sdf_c], d = v.diff[a.sdf_c];
    float* const out = a.pred + off;
    const PhiSrc src{a.pred + off, true, q, d};
    redistance_frame(dist_at<D>(a.ws + (long)bt * a.slot), src, [out, q, d](int i, float val) { out[i] = clip_norm(val, d, q); }, false, v.Ho, v.Wo, a.h,
                     a.band, a.max_rounds, a.rounds ? a.rounds + row : nullptr, a.change ? a.change + row : nullptr);
}

long ws_slot(long n) { return n > REDIST_LDS_CELLS ? (4 * n + 15) / 16 * 16 : 0; }

// the LDS kernels ask for more dynamic LDS than the default limit: raised once per device and kernel
template <class K> int allow_lds(K kernel, BfPerDeviceOnce& once) {
    if (bool& done = once.flag(); !done) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, REDIST_LDS_CELLS * 4);
        if (e != hipSuccess) return bf_fail(e, __FILE__, __LINE__);
        done = true;
    }
    return 0;
}
}  // namespace

extern "C" int64_t bf_redistance_lds_cells(void) { return REDIST_LDS_CELLS; }

extern "C" int64_t bf_redistance_ws_bytes(int64_t frames, int H, int W) {
    if (frames <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > REDIST_MAX_CELLS) return 0;
    return std::max<int64_t>(16, frames * ws_slot((long)H * W));
}

extern "C" int bf_redistance(const float* phi, int64_t frames, int H, int W, float dx, float band, int max_rounds, float* out, int32_t* rounds,
                             float* change_rms, void* ws, int64_t ws_bytes, bf_stream_t stream) {
    BF_REQUIRE(phi && out && ws, "bf_redistance: null pointer");
    BF_REQUIRE(frames > 0 && frames <= 0x7fffffff && H > 0 && W > 0 && dx > 0.f, "bf_redistance: bad sizes");
    BF_REQUIRE((int64_t)H * W <= REDIST_MAX_CELLS, "bf_redistance: a frame may have at most 2^24 cells");
    BF_REQUIRE(ws_bytes >= bf_redistance_ws_bytes(frames, H, W), "bf_redistance: workspace smaller than bf_redistance_ws_bytes");
    BF_REQUIRE((uintptr_t)ws % 16 == 0, "bf_redistance: the workspace must be 16-byte aligned");
    const long n = (long)H * W;
    const RedistanceArgs a{phi, out, H, W, dx, band > 0.f ? band : 0.f, max_rounds > 0 ? max_rounds : H + W, rounds, change_rms, (char*)ws, ws_slot(n)};
    if (n <= REDIST_LDS_CELLS) {
        static BfPerDeviceOnce once;
        if (const int rc = allow_lds(redistance_kernel<LdsDist>, once)) return rc;
        hipLaunchKernelGGL(redistance_kernel<LdsDist>, dim3((unsigned)frames), dim3(NT), (size_t)n * 4, (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL(redistance_kernel<GlobalDist>, dim3((unsigned)frames), dim3(NT), 0, (hipStream_t)stream, a);
    }
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_rollout_redistance(const bf_rollout_step* s, int sdf_channel, float dx, float band, int max_rounds, int every, float* pred,
                                     int32_t* rounds, float* change_rms, void* ws, int64_t ws_bytes, bf_stream_t stream) {
    RolloutStep v;
    if (const int rc = rollout_step_view(v, s, pred && ws, s && (int64_t)s->B * s->T <= 0x3fffffff && dx > 0.f && every >= 1,
                                         "bf_rollout_redistance: null pointer", "bf_rollout_redistance: bad sizes"))
        return rc;
    BF_REQUIRE(pred == v.pred, "bf_rollout_redistance: pred must be the tensor the step record names");
    BF_REQUIRE(sdf_channel >= 0 && sdf_channel < v.C, "bf_rollout_redistance: the signed-distance channel must be an output channel");
    BF_REQUIRE((int64_t)v.Ho * v.Wo <= REDIST_MAX_CELLS, "bf_rollout_redistance: a frame may have at most 2^24 cells");
    BF_REQUIRE(ws_bytes >= bf_redistance_ws_bytes((int64_t)v.B * v.T, v.Ho, v.Wo), "bf_rollout_redistance: workspace smaller than bf_redistance_ws_bytes(B T, Ho, Wo)");
    BF_REQUIRE((uintptr_t)ws % 16 == 0, "bf_rollout_redistance: the workspace must be 16-byte aligned");
    const long n = (long)v.Ho * v.Wo;
    const RolloutRedistanceArgs a{v, pred, sdf_channel, every, dx, band > 0.f ? band : 0.f, max_rounds > 0 ? max_rounds : v.Ho + v.Wo, rounds, change_rms,
                                  (char*)ws, ws_slot(n)};
    const dim3 grid((unsigned)(v.B * v.T));
    if (n <= REDIST_LDS_CELLS) {
        static BfPerDeviceOnce once;
        if (const int rc = allow_lds(rollout_redistance_kernel<LdsDist>, once)) return rc;
        hipLaunchKernelGGL(rollout_redistance_kernel<LdsDist>, grid, dim3(NT), (size_t)n * 4, (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL(rollout_redistance_kernel<GlobalDist>, grid, dim3(NT), 0, (hipStream_t)stream, a);
    }
    BF_CHECK_LAUNCH();
    return 0;
}
