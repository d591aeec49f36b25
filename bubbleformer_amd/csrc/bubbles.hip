// The bubble census of a frame: connected components of the vapour mask (phi > 0 in physical units; exact zeros and NaN are liquid) under
// 4- or 8-connectivity, numbered 1, 2, ... in raster order of their first cell (scipy.ndimage.label's numbering), with the per-frame counts
// and per-bubble records of include/bubbleformer_hip.h.  The reference has no program for this; DESIGN.md section 16 has the definitions.
//
// One workgroup of 1024 threads owns a frame from the mask to the records, so no two workgroups ever exchange data.  The parent array of the
// union-find (one int32 per cell, parent <= self, liquid = -1) lives in dynamic LDS when the frame has at most BUBBLE_LDS_CELLS cells, in
// a slice of the caller's workspace otherwise; there every access to it is an agent-scope atomic (served by the L2, never by this CU's L1).
// Phases, each closed by a workgroup barrier:
//   1 mask: parent = the left neighbour inside a row run, self at a run start;
//   2 ceil(log2 W) rounds of parent = parent[parent]: every cell then points at the start of its run (a fixed number of rounds);
//   3 vertical (and for 8-connectivity diagonal) links: the roots of the two cells are united by atomicMin of the larger root's parent, the
//     loop of Komura's label-equivalence scheme: when the atomicMin finds somebody else's smaller link it goes on with that one.  Only links
//     that the row runs and the links of the cell to the left do not already imply are made;
//   4 every run start is pointed at its root, 5 every other cell copies its run start's: the root of a component is its smallest index;
//   6 roots are counted per contiguous chunk of cells (one chunk per thread) and a block-wide exclusive scan numbers them in raster order;
//     roots in row 0 come first, so `attached` is their number and bubble k is on the heater exactly when k <= attached;
//   7 label image, and area / sum y / sum x of the first max_bubbles components by integer atomics (one per run of equal labels inside a chunk);
//   8 centroids: exact int64 sums, one fp64 division, one rounding.
// Every loop is bounded by construction: a root chase must strictly descend (it raises the error flag and stops otherwise), and a union
// continues only with a strictly smaller pair.  The error flag turns the frame's count into -1.  Integer atomics only: the same bits on every
// call, and a frame has the same bits alone and in a batch.
#include "clip_store.h"
#include "lane_ops.h"
#include <algorithm>

namespace {
constexpr int NT = 1024;
constexpr int NW = NT / 64;
constexpr int BUBBLE_LDS_CELLS = 40704;            // 159 KiB of parents; the last KiB of the CU's 160 is for the scan's statics
constexpr long BUBBLE_MAX_CELLS = 1L << 24;        // int32 indices and chunk arithmetic with room to spare (4096 x 4096)

typedef __attribute__((address_space(1))) int gint;
typedef __attribute__((address_space(1))) long long glong;
#define BF_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define BF_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP


struct LdsParents {
    int* L;
    __device__ __forceinline__ int ld(int i) const { return __hip_atomic_load(L + i, BF_RLX_WG); }
    __device__ __forceinline__ void st(int i, int v) const { __hip_atomic_store(L + i, v, BF_RLX_WG); }
    __device__ __forceinline__ int amin(int i, int v) const { return __hip_atomic_fetch_min(L + i, v, BF_RLX_WG); }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};
struct GlobalParents {
    gint* L;
    __device__ __forceinline__ int ld(int i) const { return __hip_atomic_load(L + i, BF_RLX_AGENT); }
    __device__ __forceinline__ void st(int i, int v) const { __hip_atomic_store(L + i, v, BF_RLX_AGENT); }
    __device__ __forceinline__ int amin(int i, int v) const { return __hip_atomic_fetch_min(L + i, v, BF_RLX_AGENT); }
    __device__ __forceinline__ void sync() const { drain_and_sync(); }
};

struct FrameSrc {                                  // the field of one frame: p[nearest_src(y) * ld + nearest_src(x)], de-normalised or not
    const float* p; int ld, Hs, Ws; float sy, sx; bool ident, denorm; float q, d;
};
struct FrameOut {                                  // this frame's slots; centroid, on_heater and labels may be null
    int* count; int* cells; int* attached; int* area; float* centroid; unsigned char* on_heater; int* labels; long long* sums;
};

__device__ __forceinline__ bool is_vapour(const FrameSrc& s, int y, int x) {
    float v = s.p[(long)nearest_src(y, s.sy, s.Hs, s.ident) * s.ld + nearest_src(x, s.sx, s.Ws, s.ident)];
    if (s.denorm) v = denormalise(v, s.q, s.d);
    return v > 0.f;                                // false for NaN and for an exact zero
}

// the root of x: parents strictly descend, so at most x steps; anything else is a corrupted array and ends the chase
template <class P> __device__ __forceinline__ int find_root(const P& lab, int x, int* err) {
    const int cap = x;
    for (int it = 0; it <= cap; ++it) {
        const int p = lab.ld(x);
        if (p == x) return x;
        if (p < 0 || p > x) break;
        x = p;
    }
    *err = 1;
    return x;
}

// one tree for a and b.  Every round ends the loop or replaces the larger root by a strictly smaller index: at most a + b rounds
template <class P> __device__ __forceinline__ void unite(const P& lab, int a, int b, int* err) {
    const int cap = a + b + 2;
    for (int it = 0; it < cap; ++it) {
        a = find_root(lab, a, err);
        b = find_root(lab, b, err);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = lab.amin(a, b);            // a was a root when it was found: link it below b
        if (old == a) return;
        if (old > a || old < 0) break;
        a = old;                                   // somebody linked a first: their target and b must meet too
    }
    *err = 1;
}

template <class P> __device__ void census_frame(const P lab, const FrameSrc src, const FrameOut o, int H, int W, bool conn8, int mb) {
    __shared__ int s_part[3][NW];
    __shared__ int s_err;
    const int n = H * W, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    gint* const area = (gint*)o.area;
    glong* const sums = (glong*)o.sums;
    if (tid == 0) s_err = 0;
    for (int k = tid; k < mb; k += NT) {
        __hip_atomic_store(area + k, 0, BF_RLX_AGENT);
        __hip_atomic_store(sums + 2 * k, 0LL, BF_RLX_AGENT);
        __hip_atomic_store(sums + 2 * k + 1, 0LL, BF_RLX_AGENT);
    }
    // 1: the mask, and the link to the left neighbour of the same row
    for (int i = tid; i < n; i += NT) {
        const int y = i / W, x = i - y * W;
        const bool v = is_vapour(src, y, x);
        lab.st(i, !v ? -1 : (x > 0 && is_vapour(src, y, x - 1)) ? i - 1 : i);
    }
    drain_and_sync();
    // 2: pointer jumping inside the row runs (a run is shorter than W + 1: ceil(log2 W) rounds reach its start)
    for (int span = 1; span < W; span <<= 1) {
        for (int i = tid; i < n; i += NT) {
            const int p = lab.ld(i);
            if (p >= 0 && p != i) {
                const int g = lab.ld(p);
                if (g >= 0 && g < p) lab.st(i, g);
            }
        }
        lab.sync();
    }
    // 3: the links to the row above that the runs and the left neighbour's links do not imply
    int err = 0;
    for (int i = tid + W; i < n; i += NT) {
        if (lab.ld(i) < 0) continue;
        const int y = i / W, x = i - y * W;
        const bool up = lab.ld(i - W) >= 0, left = x > 0 && lab.ld(i - 1) >= 0, upleft = x > 0 && lab.ld(i - W - 1) >= 0;
        if (!conn8) {
            if (up && !(left && upleft)) unite(lab, i, i - W, &err);
        } else if (up) {
            if (!left) unite(lab, i, i - W, &err);                         // left is joined to up by its own diagonal
        } else {
            if (upleft && !left) unite(lab, i, i - W - 1, &err);           // left is right below upleft
            if (x < W - 1 && lab.ld(i - W + 1) >= 0) unite(lab, i, i - W + 1, &err);
        }
    }
    lab.sync();
    // 4: run starts take their root (only run starts were ever linked, so the others still name their run start)
    for (int i = tid; i < n; i += NT) {
        const int p = lab.ld(i);
        if (p < 0) continue;
        const int y = i / W, x = i - y * W;
        if (x > 0 && lab.ld(i - 1) >= 0) continue;
        const int r = find_root(lab, i, &err);
        if (r != p) lab.st(i, r);
    }
    lab.sync();
    // 5: every other cell copies the root of its run start
    for (int i = tid; i < n; i += NT) {
        const int p = lab.ld(i);
        if (p < 0 || p == i) continue;
        const int y = i / W, x = i - y * W;
        if (x > 0 && lab.ld(i - 1) >= 0) lab.st(i, lab.ld(p));
    }
    if (err) s_err = 1;
    lab.sync();
    // 6: roots, vapour cells and roots of row 0 per chunk (an odd chunk length keeps the lanes on different LDS banks)
    const int chunk = ((n + NT - 1) / NT) | 1;
    const int i0 = min(tid * chunk, n), i1 = min(i0 + chunk, n);
    int roots = 0, cells = 0, heater = 0;
    for (int i = i0; i < i1; ++i) {
        const int p = lab.ld(i);
        cells += p >= 0;
        roots += p == i;
        heater += p == i && i < W;
    }
    int incl = roots;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { cells += __shfl_xor(cells, d, 64); heater += __shfl_xor(heater, d, 64); }
    if (lane == 63) s_part[0][wave] = incl;
    if (lane == 0) { s_part[1][wave] = cells; s_part[2][wave] = heater; }
    __syncthreads();
    int base = incl - roots, count = 0, vapour = 0, attached = 0;
    for (int w = 0; w < NW; ++w) {
        if (w < wave) base += s_part[0][w];
        count += s_part[0][w]; vapour += s_part[1][w]; attached += s_part[2][w];
    }
    // number the roots of this chunk: parent = -(number + 1), so -1 stays liquid
    for (int i = i0; i < i1; ++i)
        if (lab.ld(i) == i) lab.st(i, -(++base) - 1);
    lab.sync();
    // 7: the label image, lanes on neighbouring cells; then the records: a run of equal labels inside a chunk costs one set of atomics
    if (o.labels)
        for (int i = tid; i < n; i += NT) {
            const int v = lab.ld(i);
            o.labels[i] = v >= 0 ? -lab.ld(v) - 1 : -v - 1;                   // liquid (-1) gives 0
        }
    {
        int y = i0 / max(W, 1), x = i0 - y * W, cur = 0, a = 0;
        long long sy = 0, sx = 0;
        auto flush = [&]() {
            if (cur > 0 && cur <= mb) {
                __hip_atomic_fetch_add(area + (cur - 1), a, BF_RLX_AGENT);
                __hip_atomic_fetch_add(sums + 2 * (cur - 1), sy, BF_RLX_AGENT);
                __hip_atomic_fetch_add(sums + 2 * (cur - 1) + 1, sx, BF_RLX_AGENT);
            }
        };
        for (int i = i0; i < i1; ++i) {
            const int v = lab.ld(i);
            const int id = v >= 0 ? -lab.ld(v) - 1 : -v - 1;
            if (id != cur) { flush(); cur = id; a = 0; sy = 0; sx = 0; }
            a += 1; sy += y; sx += x;
            if (++x == W) { x = 0; ++y; }
        }
        flush();
    }
    drain_and_sync();
    // 8: the records of the first max_bubbles components; the slots behind them stay 0
    const int kept = min(count, mb);
    for (int k = tid; k < mb; k += NT) {
        float cy = 0.f, cx = 0.f;
        if (k < kept) {
            const double a = (double)__hip_atomic_load(area + k, BF_RLX_AGENT);
            cy = (float)((double)__hip_atomic_load(sums + 2 * k, BF_RLX_AGENT) / a);
            cx = (float)((double)__hip_atomic_load(sums + 2 * k + 1, BF_RLX_AGENT) / a);
        }
        if (o.centroid) { o.centroid[2 * k] = cy; o.centroid[2 * k + 1] = cx; }
        if (o.on_heater) o.on_heater[k] = k < min(attached, kept);
    }
    if (tid == 0) { *o.count = s_err ? -1 : count; *o.cells = vapour; *o.attached = attached; }
}

struct WsLayout {                                  // per frame: int64 {sum y, sum x} per record, then the parents when they do not fit the LDS
    long slot; long parents_off;
    WsLayout(int H, int W, int mb) : parents_off(16L * mb) {
        const long n = (long)H * W;
        slot = parents_off + (n > BUBBLE_LDS_CELLS ? (4 * n + 15) / 16 * 16 : 0);
    }
};

struct CensusArgs {
    const float* phi; int H, W, conn8, mb;
    int* count; int* cells; int* attached; int* area; float* centroid; unsigned char* on_heater; int* labels;
    char* ws; long slot, parents_off;
};

template <class P> __device__ __forceinline__ P parents_at(char* ws_slot, long parents_off);
template <> __device__ __forceinline__ LdsParents parents_at<LdsParents>(char*, long) {
    extern __shared__ int bubble_parents[];
    return LdsParents{bubble_parents};
}
template <> __device__ __forceinline__ GlobalParents parents_at<GlobalParents>(char* ws_slot, long parents_off) {
    return GlobalParents{(gint*)(ws_slot + parents_off)};
}

template <class P> __global__ void __launch_bounds__(NT) bubble_census_kernel(CensusArgs a) {
    const long f = blockIdx.x, n = (long)a.H * a.W;
    char* slot = a.ws + f * a.slot;
    const FrameSrc src{a.phi + f * n, a.W, a.H, a.W, 1.f, 1.f, true, false, 1.f, 0.f};
    const FrameOut out{a.count + f, a.cells + f, a.attached + f, a.area + f * a.mb, a.centroid ? a.centroid + 2 * f * a.mb : nullptr,
                       a.on_heater ? a.on_heater + f * a.mb : nullptr, a.labels ? a.labels + f * n : nullptr, (long long*)slot};
    census_frame(parents_at<P>(slot, a.parents_off), src, out, a.H, a.W, a.conn8 != 0, a.mb);
}

struct RolloutBubbleArgs {
    RolloutStep v;                                                         // clip_store.h: this step's prediction and its stored target frames
    int sdf_c, conn8, mb;
    int* count[2]; int* cells[2]; int* attached[2]; int* area[2];          // [0] the prediction, [1] the simulation
    char* ws; long slot, parents_off;
    int* ring;                                                             // null, or the label images [2 sides][2 halves][B][T][Ho][Wo]: half s & 1
};

template <class P> __global__ void __launch_bounds__(NT) rollout_bubbles_kernel(RolloutBubbleArgs a) {
    const RolloutStep& v = a.v;
    const int s = v.current();
    if (s < 0) return;                                                     // behind the last row: nothing is written
    const int bt = blockIdx.x, t = bt % v.T, b = bt / v.T, side = blockIdx.y;
    FrameSrc src;
    if (side == 1) src = FrameSrc{v.stored(a.sdf_c, v.frame(s, b, t)), v.W, v.H, v.W, v.sy(), v.sx(), v.ident(), false, 1.f, 0.f};
    else src = FrameSrc{v.predicted(bt, a.sdf_c), v.Wo, v.Ho, v.Wo, 1.f, 1.f, true, true, v.dv[a.sdf_c], v.diff[a.sdf_c]};
    const long row = v.row(s, b, t);
    char* slot = a.ws + ((long)bt * 2 + side) * a.slot;
    int* const labels = a.ring ? a.ring + ((((long)side * 2 + (s & 1)) * v.B + b) * v.T + t) * ((long)v.Ho * v.Wo) : nullptr;
    const FrameOut out{a.count[side] + row, a.cells[side] + row, a.attached[side] + row, a.area[side] + row * a.mb, nullptr, nullptr, labels,
                       (long long*)slot};
    census_frame(parents_at<P>(slot, a.parents_off), src, out, v.Ho, v.Wo, a.conn8 != 0, a.mb);
}

// the LDS kernels ask for more dynamic LDS than the default limit: raised once per device and kernel
template <class K> int allow_lds(K kernel, BfPerDeviceOnce& once) {
    if (bool& done = once.flag(); !done) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, BUBBLE_LDS_CELLS * 4);
        if (e != hipSuccess) return bf_fail(e, __FILE__, __LINE__);
        done = true;
    }
    return 0;
}
}  // namespace

extern "C" int64_t bf_bubble_census_lds_cells(void) { return BUBBLE_LDS_CELLS; }

extern "C" int64_t bf_bubble_census_ws_bytes(int64_t frames, int H, int W, int max_bubbles) {
    if (frames <= 0 || H <= 0 || W <= 0 || max_bubbles <= 0 || (int64_t)H * W > BUBBLE_MAX_CELLS) return 0;
    return frames * WsLayout(H, W, max_bubbles).slot;
}

extern "C" int bf_bubble_census(const float* phi, int64_t frames, int H, int W, int connectivity, int max_bubbles, int32_t* count,
                                int32_t* vapour_cells, int32_t* attached, int32_t* area, float* centroid, unsigned char* on_heater, int32_t* labels,
                                void* ws, int64_t ws_bytes, bf_stream_t stream) {
    BF_REQUIRE(phi && count && vapour_cells && attached && area && ws, "bf_bubble_census: null pointer");
    BF_REQUIRE(frames > 0 && frames <= 0x7fffffff && H > 0 && W > 0 && max_bubbles > 0, "bf_bubble_census: bad sizes");
    BF_REQUIRE(connectivity == 4 || connectivity == 8, "bf_bubble_census: connectivity must be 4 or 8");
    BF_REQUIRE((int64_t)H * W <= BUBBLE_MAX_CELLS, "bf_bubble_census: a frame may have at most 2^24 cells");
    BF_REQUIRE(ws_bytes >= bf_bubble_census_ws_bytes(frames, H, W, max_bubbles), "bf_bubble_census: workspace smaller than bf_bubble_census_ws_bytes");
    BF_REQUIRE((uintptr_t)ws % 16 == 0, "bf_bubble_census: the workspace must be 16-byte aligned");
    const WsLayout lay(H, W, max_bubbles);
    const CensusArgs a{phi, H, W, connectivity == 8, max_bubbles, count, vapour_cells, attached, area, centroid, on_heater, labels, (char*)ws, lay.slot,
                       lay.parents_off};
    const long n = (long)H * W;
    if (n <= BUBBLE_LDS_CELLS) {
        static BfPerDeviceOnce once;
        if (const int rc = allow_lds(bubble_census_kernel<LdsParents>, once)) return rc;
        hipLaunchKernelGGL(bubble_census_kernel<LdsParents>, dim3((unsigned)frames), dim3(NT), (size_t)n * 4, (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL(bubble_census_kernel<GlobalParents>, dim3((unsigned)frames), dim3(NT), 0, (hipStream_t)stream, a);
    }
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_rollout_bubbles(const bf_rollout_step* s, int sdf_channel, int connectivity, int max_bubbles, const bf_census_rows* pred,
                                  const bf_census_rows* tgt, int32_t* labels, void* ws, int64_t ws_bytes, bf_stream_t stream) {
    RolloutStep v;
    if (const int rc = rollout_step_view(v, s, pred && tgt && pred->count && tgt->count && pred->cells && tgt->cells && pred->attached && tgt->attached &&
                                         pred->area && tgt->area && ws, s && (int64_t)s->B * s->T <= 0x3fffffff && max_bubbles > 0,
                                         "bf_rollout_bubbles: null pointer", "bf_rollout_bubbles: bad sizes"))
        return rc;
    const int B = v.B, T = v.T, Ho = v.Ho, Wo = v.Wo;
    BF_REQUIRE(sdf_channel >= 0 && sdf_channel < v.C, "bf_rollout_bubbles: the signed-distance channel must be an output channel");
    BF_REQUIRE(connectivity == 4 || connectivity == 8, "bf_rollout_bubbles: connectivity must be 4 or 8");
    BF_REQUIRE((int64_t)Ho * Wo <= BUBBLE_MAX_CELLS, "bf_rollout_bubbles: a frame may have at most 2^24 cells");
    BF_REQUIRE(ws_bytes >= bf_bubble_census_ws_bytes(2 * (int64_t)B * T, Ho, Wo, max_bubbles), "bf_rollout_bubbles: workspace smaller than bf_bubble_census_ws_bytes(2 B T, Ho, Wo, max_bubbles)");
    BF_REQUIRE((uintptr_t)ws % 16 == 0, "bf_rollout_bubbles: the workspace must be 16-byte aligned");
    const WsLayout lay(Ho, Wo, max_bubbles);
    const RolloutBubbleArgs a{v, sdf_channel, connectivity == 8, max_bubbles, {pred->count, tgt->count}, {pred->cells, tgt->cells}, {pred->attached, tgt->attached},
                              {pred->area, tgt->area}, (char*)ws, lay.slot, lay.parents_off, labels};
    const long n = (long)Ho * Wo;
    const dim3 grid((unsigned)(B * T), 2);
    if (n <= BUBBLE_LDS_CELLS) {
        static BfPerDeviceOnce once;
        if (const int rc = allow_lds(rollout_bubbles_kernel<LdsParents>, once)) return rc;
        hipLaunchKernelGGL(rollout_bubbles_kernel<LdsParents>, grid, dim3(NT), (size_t)n * 4, (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL(rollout_bubbles_kernel<GlobalParents>, grid, dim3(NT), 0, (hipStream_t)stream, a);
    }
    BF_CHECK_LAUNCH();
    return 0;
}
