// Bubbles followed from one frame to the next: the links between the census label images (csrc/bubbles.hip) of two consecutive frames, the
// events they imply, and the track ids of a sequence; and predicted bubbles matched to simulated ones, frame by frame.  The reference has no program for this; DESIGN.md section 17 has the definitions and
// include/bubbleformer_hip.h the contract.
//
// bf_bubble_links: one workgroup of 1024 threads owns a pair (frame a at t, frame b at t + 1) from the two label images to its records, so no
// two workgroups ever exchange data.  With ka / kb = min(count, max_bubbles) of the two frames, the ka x kb overlap table (int32 cells with
// La == i and Lb == j) lives in dynamic LDS when ka * kb <= LINKS_LDS_ENTRIES, in this workgroup's slice of the caller's workspace otherwise;
// ka * kb is known on the device only, so the choice is a workgroup-uniform branch inside the one kernel.  A workspace table is zeroed by the
// workgroup itself and touched only with agent-scope relaxed integer atomics (served by the L2, never by this CU's L1), and each of its barriers
// waits for vmcnt(0) first.  Phases, each closed by a barrier:
//   1 the table is zeroed;
//   2 cell pass: every thread walks a contiguous chunk of cells; a run of equal (La, Lb) inside the chunk costs one atomic add of its length;
//   3 row pass, a wave per bubble of a (lanes stride over the row, a butterfly keeps the largest overlap and among equals the smallest j):
//     successor and n_successors; column pass, a thread per bubble of b (neighbouring lanes read neighbouring entries): predecessor, n_predecessors;
//   4 a thread per record: departures (which need predecessor[successor[i]]), the zeros behind ka / kb, and the five event counts by a block reduction.
// Every loop runs over a range fixed before it starts.  Integer adds only: the same bits on every call, and for a pair alone or in a batch.
//
// bf_bubble_track_ids: one workgroup per sequence walks its frames in order; per frame a thread per chunk of records decides continue (mutual
// predecessor / successor) or new, a block-wide exclusive scan numbers the new tracks in bubble order, and one drained barrier closes the frame
// (the next frame reads this frame's ids back through the L2).
//
// bf_bubble_match: the same table over another pair of images -- the prediction frame and the simulation frame of one time --
// with a new record phase behind it.  One workgroup owns a pair; phases 1 to 3 are link_tables unchanged, its four result rows kept in the pair's
// workspace slice; a second cell pass takes the exact y / x sums per label (a run of one label inside a chunk costs two 64-bit agent-scope atomic
// adds into the slice) and the two mask counts; phase 4, a thread per record, decides the matches (mutual best overlap, IoU bound in fp64), writes
// the three rows and the centroid displacement (fp64, unfused, one rounding) and reduces the six counts.
#include "clip_store.h"
#include "lane_ops.h"
#include <algorithm>

namespace {
constexpr int NT = 1024;
constexpr int NW = NT / 64;
constexpr int LINKS_LDS_ENTRIES = 16384;           // 64 KiB of overlaps (a 128 x 128 table): two pairs share a CU's 160 KiB
constexpr int LINKS_MAX_BUBBLES = 1 << 15;         // ka * kb <= 2^30: int32 table indices
constexpr long LINKS_MAX_CELLS = 1L << 24;         // as the census: int32 chunk arithmetic with room to spare

typedef __attribute__((address_space(1))) int gint;
#define BF_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define BF_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

// a value another thread of this workgroup left in global memory before the last drained barrier, and such a value's store: both through the L2
__device__ __forceinline__ int ld_l2(const int* p) { return __hip_atomic_load((gint*)p, BF_RLX_AGENT); }
__device__ __forceinline__ void st_l2(int* p, int v) { __hip_atomic_store((gint*)p, v, BF_RLX_AGENT); }

struct LdsTable {
    int* L;
    __device__ __forceinline__ int ld(int i) const { return L[i]; }
    __device__ __forceinline__ void zero(int i) const { L[i] = 0; }
    __device__ __forceinline__ void add(int i, int v) const { __hip_atomic_fetch_add(L + i, v, BF_RLX_WG); }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};
struct GlobalTable {
    gint* L;
    __device__ __forceinline__ int ld(int i) const { return __hip_atomic_load(L + i, BF_RLX_AGENT); }
    __device__ __forceinline__ void zero(int i) const { __hip_atomic_store(L + i, 0, BF_RLX_AGENT); }
    __device__ __forceinline__ void add(int i, int v) const { __hip_atomic_fetch_add(L + i, v, BF_RLX_AGENT); }
    __device__ __forceinline__ void sync() const { drain_and_sync(); }
};

struct PairIn {                                    // the two frames of a pair: label images and census rows
    const int* la; const int* lb; const int* count_a; const int* count_b; const int* attached_a; const int* attached_b; const int* area_a;
};
struct PairOut {                                   // this pair's slots: five rows of max_bubbles and the five event counts
    int* successor; int* n_successors; int* predecessor; int* n_predecessors; int* departure_area; int* events;
};

template <class Tab> __device__ void link_tables(const Tab tab, const PairIn in, const PairOut o, int n, int ka, int kb) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int entries = ka * kb;
    // 1: an empty table
    for (int e = tid; e < entries; e += NT) tab.zero(e);
    tab.sync();
    // 2: the cell pass (labels above ka / kb are liquid here: their bubbles have no record)
    {
        const int chunk = ((n + NT - 1) / NT) | 1;
        const int i0 = min(tid * chunk, n), i1 = min(i0 + chunk, n);
        int cur = -1, len = 0;
        for (int i = i0; i < i1; ++i) {
            const int a = in.la[i], b = in.lb[i];
            const int e = (a >= 1 && a <= ka && b >= 1 && b <= kb) ? (a - 1) * kb + (b - 1) : -1;
            if (e != cur) {
                if (cur >= 0) tab.add(cur, len);
                cur = e; len = 0;
            }
            ++len;
        }
        if (cur >= 0) tab.add(cur, len);
    }
    tab.sync();
    // 3: rows, a wave each
    for (int i = wave; i < ka; i += NW) {
        int best = 0, arg = 0, cnt = 0;
        for (int j = lane; j < kb; j += 64) {
            const int v = tab.ld(i * kb + j);
            cnt += v > 0;
            if (v > best) { best = v; arg = j + 1; }                           // j ascends: the first of equals stays
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const int ob = __shfl_xor(best, d, 64), oa = __shfl_xor(arg, d, 64);
            cnt += __shfl_xor(cnt, d, 64);
            if (ob > best || (ob == best && ob > 0 && oa < arg)) { best = ob; arg = oa; }
        }
        if (lane == 0) { st_l2(o.successor + i, arg); st_l2(o.n_successors + i, cnt); }
    }
    // columns, a thread each
    for (int j = tid; j < kb; j += NT) {
        int best = 0, arg = 0, cnt = 0;
        for (int i = 0; i < ka; ++i) {
            const int v = tab.ld(i * kb + j);
            cnt += v > 0;
            if (v > best) { best = v; arg = i + 1; }
        }
        st_l2(o.predecessor + j, arg);
        st_l2(o.n_predecessors + j, cnt);
    }
    drain_and_sync();
}

// the records of a pair whose tables are done: departures, zeros behind ka / kb, events
__device__ void link_records(const PairIn in, const PairOut o, int mb, int ka, int kb) {
    __shared__ int s_ev[5][NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int att_a = *in.attached_a, att_b = *in.attached_b;
    int ev[5] = {0, 0, 0, 0, 0};                                               // births, deaths, merges, splits, departures
    for (int k = tid; k < mb; k += NT) {
        int dep_area = 0;
        if (k < ka) {
            const int s = ld_l2(o.successor + k);
            ev[1] += s == 0;
            ev[3] += ld_l2(o.n_successors + k) >= 2;
            if (k + 1 <= att_a && s > 0 && s > att_b && ld_l2(o.predecessor + (s - 1)) == k + 1) { dep_area = in.area_a[k]; ev[4] += 1; }
        } else {
            o.successor[k] = 0; o.n_successors[k] = 0;
        }
        o.departure_area[k] = dep_area;
        if (k < kb) {
            ev[0] += ld_l2(o.predecessor + k) == 0;
            ev[2] += ld_l2(o.n_predecessors + k) >= 2;
        } else {
            o.predecessor[k] = 0; o.n_predecessors[k] = 0;
        }
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) ev[q] += __shfl_xor(ev[q], d, 64);
        if (lane == 0) s_ev[q][wave] = ev[q];
    }
    __syncthreads();
    if (tid < 5) {
        int total = 0;
        for (int w = 0; w < NW; ++w) total += s_ev[tid][w];
        o.events[tid] = total;
    }
}

__device__ void link_pair(const PairIn in, const PairOut o, int n, int mb, gint* ws_table) {
    extern __shared__ int link_overlaps[];
    const int ca = *in.count_a, cb = *in.count_b;                              // workgroup-uniform, as every branch on them below
    if (ca < 0 || cb < 0) {                                                    // a census that gave up: the pair says so everywhere
        for (int k = threadIdx.x; k < mb; k += NT) {
            o.successor[k] = -1; o.n_successors[k] = -1; o.predecessor[k] = -1; o.n_predecessors[k] = -1; o.departure_area[k] = -1;
        }
        if (threadIdx.x < 5) o.events[threadIdx.x] = -1;
        return;
    }
    const int ka = min(ca, mb), kb = min(cb, mb);
    if (ka * kb <= LINKS_LDS_ENTRIES) link_tables(LdsTable{link_overlaps}, in, o, n, ka, kb);
    else link_tables(GlobalTable{ws_table}, in, o, n, ka, kb);
    link_records(in, o, mb, ka, kb);
}

__device__ __forceinline__ PairOut pair_out(const PairOut base, long row, int mb) {
    return PairOut{base.successor + row * mb, base.n_successors + row * mb, base.predecessor + row * mb, base.n_predecessors + row * mb,
                   base.departure_area + row * mb, base.events + row * 5};
}

struct LinksArgs {
    const int* labels; const int* count; const int* attached; const int* area;     // [N][T]..., as bf_bubble_census left them
    int T, n, mb;
    PairOut out;                                                                   // [N][T - 1]...
    char* ws; long slot;
};

__global__ void __launch_bounds__(NT) bubble_links_kernel(LinksArgs a) {
    const long p = blockIdx.x, seq = p / (a.T - 1), fa = seq * a.T + p % (a.T - 1), fb = fa + 1;
    const PairIn in{a.labels + fa * a.n, a.labels + fb * a.n, a.count + fa, a.count + fb, a.attached + fa, a.attached + fb, a.area + fa * a.mb};
    link_pair(in, pair_out(a.out, p, a.mb), a.n, a.mb, (gint*)(a.ws + p * a.slot));
}

struct RolloutLinksArgs {
    RolloutStep v;                                                                 // clip_store.h: the step counter and the report's rows
    const int* ring;                                                               // [2 sides][2 halves][B][T][Ho][Wo] label images
    const int* count[2]; const int* attached[2]; const int* area[2];              // [B][steps*T]...: [0] the prediction, [1] the simulation
    int mb;
    PairOut out[2];                                                                // [B][steps*T - 1]...
    char* ws; long slot;
};

__global__ void __launch_bounds__(NT) rollout_links_kernel(RolloutLinksArgs a) {
    const RolloutStep& v = a.v;
    const int s = v.current();
    if (s < 0) return;                                                             // behind the last row: nothing is written
    const int bt = blockIdx.x, t = bt % v.T, b = bt / v.T, side = blockIdx.y;
    if (s == 0 && t == 0) return;                                                  // the first frame of a rollout has no earlier one
    const int n = v.Ho * v.Wo;
    const int sa = t > 0 ? s : s - 1, ta = t > 0 ? t - 1 : v.T - 1;                // the earlier frame: of this step, or the last of the one before
    auto image = [&](int step, int frame) { return a.ring + ((((long)side * 2 + (step & 1)) * v.B + b) * v.T + frame) * n; };
    const long ra = v.row(sa, b, ta), rb = v.row(s, b, t);
    const PairIn in{image(sa, ta), image(s, t), a.count[side] + ra, a.count[side] + rb, a.attached[side] + ra, a.attached[side] + rb,
                    a.area[side] + ra * a.mb};
    const long pair = (long)b * (v.steps * v.T - 1) + (s * v.T + t - 1);
    link_pair(in, pair_out(a.out[side], pair, a.mb), n, a.mb, (gint*)(a.ws + ((long)bt * 2 + side) * a.slot));
}

struct TrackArgs {
    const int* count; const int* successor; const int* predecessor;               // [N][T], [N][T - 1][mb] twice
    int* track_id; int* n_tracks;                                                  // [N][T][mb], [N]
    int T, mb;
};

__global__ void __launch_bounds__(NT) bubble_track_ids_kernel(TrackArgs a) {
    __shared__ int s_part[NW];                                                     // read before the barrier that closes a frame, written after it
    const long seq = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, mb = a.mb;
    const int per = (mb + NT - 1) / NT, k0 = min(tid * per, mb), k1 = min(k0 + per, mb);
    int next = 0;                                                                  // tracks so far: the same number in every thread
    for (int t = 0; t < a.T; ++t) {
        const int c = a.count[seq * a.T + t], kept = max(0, min(c, mb));
        const long pair = seq * (a.T - 1) + max(t - 1, 0);                         // the pair that ends in this frame (read for t > 0 only)
        const int* succ = a.successor + pair * mb;
        const int* pred = a.predecessor + pair * mb;
        int* ids = a.track_id + (seq * a.T + t) * mb;
        const int* before = a.track_id + (seq * a.T + max(t - 1, 0)) * mb;
        // bubble k continues the track of bubble p of the frame before when each is the other's largest overlap; -1 (an invalid pair) starts a track
        auto continues = [&](int k) { const int p = t > 0 ? pred[k] : 0; return (p > 0 && p <= mb && succ[p - 1] == k + 1) ? p : 0; };
        int fresh = 0;
        for (int k = k0; k < k1; ++k) {
            if (k < kept) fresh += continues(k) == 0;
        }
        int incl = fresh;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int u = __shfl_up(incl, d, 64); if (lane >= d) incl += u; }
        if (lane == 63) s_part[wave] = incl;
        __syncthreads();
        int base = next + incl - fresh;
        for (int w = 0; w < NW; ++w) {
            if (w < wave) base += s_part[w];
            next += s_part[w];
        }
        for (int k = k0; k < k1; ++k) {
            int id = 0;
            if (k < kept) {
                const int p = continues(k);
                id = p > 0 ? ld_l2(before + (p - 1)) : ++base;
            }
            st_l2(ids + k, id);
        }
        drain_and_sync();                                                          // closes the frame: its ids are in the L2 for the next one
    }
    if (tid == 0) a.n_tracks[seq] = next;
}

// ---- prediction against simulation: the same table over (prediction frame, simulation frame), and the match records behind it ----
typedef __attribute__((address_space(1))) unsigned long long gu64;

struct MatchSide { const int* area_s; };          // what PairIn does not carry: the simulation's areas (PairIn::area_a is the prediction's)
struct MatchOut {                                  // this pair's slots: three rows of max_bubbles, the displacements, six counts, two mask counts
    int* match_pred; int* match_target; int* overlap; float* displacement; int* counts; int* mask;
};
// a pair's workspace slice: 4 x mb y / x sums (64-bit), the four best-partner rows link_tables leaves, then the table that does not fit LDS
struct MatchScratch {
    gu64* sums; int* rows; gint* table;
    __device__ __forceinline__ gu64* sum(int q, int mb) const { return sums + (long)q * mb; }      // q: 0 y of P, 1 x of P, 2 y of S, 3 x of S
};

// mutual best overlap above the IoU bound: the one decision both the prediction's and the simulation's slot take
__device__ __forceinline__ bool iou_passes(int o, int area_p, int area_s, float min_iou) {
    return (double)o >= (double)min_iou * (double)(area_p + area_s - o);       // the union is below 2^24: the product is exact
}

// 4 of the match: a thread per record decides it and writes the rows; a block reduction writes the counts
template <class Tab> __device__ void match_records(const Tab tab, const PairIn in, const MatchSide sd, const MatchOut o, const MatchScratch sc, int mb,
                                                   int kp, int ks, float min_iou) {
    __shared__ int s_hit[2][NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int att_p = *in.attached_a, att_s = *in.attached_b;
    const int* best_s = sc.rows;                                               // link_tables' successor row: per predicted bubble
    const int* best_p = sc.rows + 2 * (long)mb;                                // its predecessor row: per simulated bubble
    int hits = 0, heater_hits = 0;
    for (int k = tid; k < mb; k += NT) {
        int mp = 0, ov = 0, mt = 0;
        float disp = 0.f;
        if (k < kp) {
            const int j = ld_l2(best_s + k);
            if (j > 0 && ld_l2(best_p + (j - 1)) == k + 1) {
                const int v = tab.ld(k * ks + (j - 1)), ap = in.area_a[k], as = sd.area_s[j - 1];
                if (iou_passes(v, ap, as, min_iou)) {
#pragma clang fp contract(off)
                    mp = j; ov = v;
                    const double yp = (double)__hip_atomic_load(sc.sum(0, mb) + k, BF_RLX_AGENT) / (double)ap;
                    const double xp = (double)__hip_atomic_load(sc.sum(1, mb) + k, BF_RLX_AGENT) / (double)ap;
                    const double ys = (double)__hip_atomic_load(sc.sum(2, mb) + (j - 1), BF_RLX_AGENT) / (double)as;
                    const double xs = (double)__hip_atomic_load(sc.sum(3, mb) + (j - 1), BF_RLX_AGENT) / (double)as;
                    const double dy = yp - ys, dx = xp - xs;
                    disp = (float)sqrt(dy * dy + dx * dx);
                    hits += 1;
                    heater_hits += k + 1 <= att_p && j <= att_s;
                }
            }
        }
        if (k < ks) {
            const int i = ld_l2(best_p + k);
            if (i > 0 && ld_l2(best_s + (i - 1)) == k + 1 && iou_passes(tab.ld((i - 1) * ks + k), in.area_a[i - 1], sd.area_s[k], min_iou)) mt = i;
        }
        o.match_pred[k] = mp; o.overlap[k] = ov; o.displacement[k] = disp; o.match_target[k] = mt;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { hits += __shfl_xor(hits, d, 64); heater_hits += __shfl_xor(heater_hits, d, 64); }
    if (lane == 0) { s_hit[0][wave] = hits; s_hit[1][wave] = heater_hits; }
    __syncthreads();
    if (tid == 0) {
        int h = 0, hh = 0;
        for (int w = 0; w < NW; ++w) { h += s_hit[0][w]; hh += s_hit[1][w]; }
        o.counts[0] = h; o.counts[1] = ks - h; o.counts[2] = kp - h;
        o.counts[3] = hh; o.counts[4] = min(att_s, ks) - hh; o.counts[5] = min(att_p, kp) - hh;
    }
}

// 1 to 3 are link_tables; then the centroid pass (a run of one label inside a thread's chunk costs two 64-bit atomic adds of its y and x sums)
// and the mask counts, closed by a drained barrier; then the records
template <class Tab> __device__ void match_tables(const Tab tab, const PairIn in, const MatchSide sd, const MatchOut o, const MatchScratch sc, int n, int W,
                                                  int mb, int kp, int ks, float min_iou) {
    __shared__ int s_mask[2][NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < mb; k += NT) {                                       // empty sums; link_tables' closing barrier drains these stores
        if (k < kp) { __hip_atomic_store(sc.sum(0, mb) + k, 0ull, BF_RLX_AGENT); __hip_atomic_store(sc.sum(1, mb) + k, 0ull, BF_RLX_AGENT); }
        if (k < ks) { __hip_atomic_store(sc.sum(2, mb) + k, 0ull, BF_RLX_AGENT); __hip_atomic_store(sc.sum(3, mb) + k, 0ull, BF_RLX_AGENT); }
    }
    link_tables(tab, in, PairOut{sc.rows, sc.rows + mb, sc.rows + 2 * (long)mb, sc.rows + 3 * (long)mb, nullptr, nullptr}, n, kp, ks);
    int both = 0, either = 0;
    {
        const int chunk = ((n + NT - 1) / NT) | 1;
        const int i0 = min(tid * chunk, n), i1 = min(i0 + chunk, n);
        int y = i0 / W, x = i0 - y * W;
        int cur_p = 0, cur_s = 0;                                              // the label of the open run of each side, 0: none
        unsigned long long yp = 0, xp = 0, ys = 0, xs = 0;
        for (int i = i0; i < i1; ++i) {
            const int a = in.la[i], b = in.lb[i];
            both += a > 0 && b > 0;
            either += a > 0 || b > 0;
            const int p = a <= kp ? a : 0, s = b <= ks ? b : 0;                // labels above kp / ks have no record
            if (p != cur_p) {
                if (cur_p > 0) { __hip_atomic_fetch_add(sc.sum(0, mb) + (cur_p - 1), yp, BF_RLX_AGENT); __hip_atomic_fetch_add(sc.sum(1, mb) + (cur_p - 1), xp, BF_RLX_AGENT); }
                cur_p = p; yp = 0; xp = 0;
            }
            if (s != cur_s) {
                if (cur_s > 0) { __hip_atomic_fetch_add(sc.sum(2, mb) + (cur_s - 1), ys, BF_RLX_AGENT); __hip_atomic_fetch_add(sc.sum(3, mb) + (cur_s - 1), xs, BF_RLX_AGENT); }
                cur_s = s; ys = 0; xs = 0;
            }
            yp += y; xp += x; ys += y; xs += x;
            if (++x == W) { x = 0; ++y; }
        }
        if (cur_p > 0) { __hip_atomic_fetch_add(sc.sum(0, mb) + (cur_p - 1), yp, BF_RLX_AGENT); __hip_atomic_fetch_add(sc.sum(1, mb) + (cur_p - 1), xp, BF_RLX_AGENT); }
        if (cur_s > 0) { __hip_atomic_fetch_add(sc.sum(2, mb) + (cur_s - 1), ys, BF_RLX_AGENT); __hip_atomic_fetch_add(sc.sum(3, mb) + (cur_s - 1), xs, BF_RLX_AGENT); }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { both += __shfl_xor(both, d, 64); either += __shfl_xor(either, d, 64); }
    if (lane == 0) { s_mask[0][wave] = both; s_mask[1][wave] = either; }
    drain_and_sync();
    if (tid < 2) {
        int total = 0;
        for (int w = 0; w < NW; ++w) total += s_mask[tid][w];
        o.mask[tid] = total;
    }
    match_records(tab, in, sd, o, sc, mb, kp, ks, min_iou);
}

__device__ void match_pair(const PairIn in, const MatchSide sd, const MatchOut o, int n, int W, int mb, float min_iou, char* slice) {
    extern __shared__ int link_overlaps[];
    const int cp = *in.count_a, cs = *in.count_b;                              // workgroup-uniform, as every branch on them below
    if (cp < 0 || cs < 0) {                                                    // a census that gave up: the pair says so everywhere
        for (int k = threadIdx.x; k < mb; k += NT) { o.match_pred[k] = -1; o.match_target[k] = -1; o.overlap[k] = -1; o.displacement[k] = __builtin_nanf(""); }
        if (threadIdx.x < 6) o.counts[threadIdx.x] = -1;
        if (threadIdx.x < 2) o.mask[threadIdx.x] = -1;
        return;
    }
    const int kp = min(cp, mb), ks = min(cs, mb);
    const MatchScratch sc{(gu64*)slice, (int*)(slice + 32L * mb), (gint*)(slice + 48L * mb)};
    if (kp * ks <= LINKS_LDS_ENTRIES) match_tables(LdsTable{link_overlaps}, in, sd, o, sc, n, W, mb, kp, ks, min_iou);
    else match_tables(GlobalTable{sc.table}, in, sd, o, sc, n, W, mb, kp, ks, min_iou);
}

__device__ __forceinline__ MatchOut match_out(const MatchOut base, long row, int mb) {
    return MatchOut{base.match_pred + row * mb, base.match_target + row * mb, base.overlap + row * mb, base.displacement + row * mb, base.counts + row * 6,
                    base.mask + row * 2};
}

struct MatchCensus { const int* count[2]; const int* attached[2]; const int* area[2]; };      // [0] the prediction, [1] the simulation

struct MatchArgs {
    const int* labels[2]; MatchCensus c;                                           // [frames][H][W]; [frames], [frames][mb]
    int n, W, mb; float min_iou;
    MatchOut out;                                                                  // [frames]...
    char* ws; long slot;
};

__global__ void __launch_bounds__(NT) bubble_match_kernel(MatchArgs a) {
    const long f = blockIdx.x;
    const PairIn in{a.labels[0] + f * a.n, a.labels[1] + f * a.n, a.c.count[0] + f, a.c.count[1] + f, a.c.attached[0] + f, a.c.attached[1] + f,
                    a.c.area[0] + f * a.mb};
    match_pair(in, MatchSide{a.c.area[1] + f * a.mb}, match_out(a.out, f, a.mb), a.n, a.W, a.mb, a.min_iou, a.ws + f * a.slot);
}

struct RolloutMatchArgs {
    RolloutStep v;
    const int* ring;                                                               // [2 sides][2 halves][B][T][Ho][Wo] label images
    MatchCensus c;                                                                 // [B][steps*T]...
    int mb; float min_iou;
    MatchOut out;                                                                  // [B][steps*T]...
    char* ws; long slot;
};

__global__ void __launch_bounds__(NT) rollout_match_kernel(RolloutMatchArgs a) {
    const RolloutStep& v = a.v;
    const int s = v.current();
    if (s < 0) return;                                                             // behind the last row: nothing is written
    const int bt = blockIdx.x, t = bt % v.T, b = bt / v.T;
    const int n = v.Ho * v.Wo;
    auto image = [&](int side) { return a.ring + ((((long)side * 2 + (s & 1)) * v.B + b) * v.T + t) * n; };
    const long r = v.row(s, b, t);
    const PairIn in{image(0), image(1), a.c.count[0] + r, a.c.count[1] + r, a.c.attached[0] + r, a.c.attached[1] + r, a.c.area[0] + r * a.mb};
    match_pair(in, MatchSide{a.c.area[1] + r * a.mb}, match_out(a.out, r, a.mb), n, v.Wo, a.mb, a.min_iou, a.ws + (long)bt * a.slot);
}

// a side's link rows: all six present; as the kernels' PairOut
bool all_rows(const bf_link_rows* r) { return r && r->successor && r->n_successors && r->predecessor && r->n_predecessors && r->departure_area && r->events; }
PairOut pair_out(const bf_link_rows* r) { return PairOut{r->successor, r->n_successors, r->predecessor, r->n_predecessors, r->departure_area, r->events}; }

long links_slot(int mb) { return (long)mb * mb > LINKS_LDS_ENTRIES ? 4L * mb * mb : 0; }
size_t links_lds_bytes(int mb) { return (size_t)std::min((long)mb * mb, (long)LINKS_LDS_ENTRIES) * 4; }

// 64 KiB of dynamic LDS beside the statics is more than the default limit: raised once per device and kernel
template <class K> int allow_lds(K kernel, BfPerDeviceOnce& once) {
    if (bool& done = once.flag(); !done) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LINKS_LDS_ENTRIES * 4);
        if (e != hipSuccess) return bf_fail(e, __FILE__, __LINE__);
        done = true;
    }
    return 0;
}
}  // namespace

extern "C" int64_t bf_bubble_links_lds_entries(void) { return LINKS_LDS_ENTRIES; }

extern "C" int64_t bf_bubble_links_ws_bytes(int64_t pairs, int max_bubbles) {
    if (pairs <= 0 || max_bubbles <= 0 || max_bubbles > LINKS_MAX_BUBBLES) return 0;
    return 16 + pairs * links_slot(max_bubbles);
}

extern "C" int bf_bubble_links(const int32_t* labels, const bf_census_rows* census, int64_t sequences, int T, int H, int W, int max_bubbles,
                               const bf_link_rows* links, void* ws, int64_t ws_bytes, bf_stream_t stream) {
    BF_REQUIRE(sequences > 0 && T > 0 && H > 0 && W > 0 && max_bubbles > 0, "bf_bubble_links: bad sizes");
    BF_REQUIRE(max_bubbles <= LINKS_MAX_BUBBLES, "bf_bubble_links: at most 2^15 records per frame");
    BF_REQUIRE((int64_t)H * W <= LINKS_MAX_CELLS, "bf_bubble_links: a frame may have at most 2^24 cells");
    if (T == 1) return 0;                                                          // no pair: nothing to launch
    const int64_t pairs = sequences * (T - 1);
    BF_REQUIRE(pairs <= 0x7fffffff, "bf_bubble_links: bad sizes");
    BF_REQUIRE(labels && census && census->count && census->attached && census->area && all_rows(links) && ws, "bf_bubble_links: null pointer");
    BF_REQUIRE(ws_bytes >= bf_bubble_links_ws_bytes(pairs, max_bubbles), "bf_bubble_links: workspace smaller than bf_bubble_links_ws_bytes");
    BF_REQUIRE((uintptr_t)ws % 16 == 0, "bf_bubble_links: the workspace must be 16-byte aligned");
    const LinksArgs a{labels, census->count, census->attached, census->area, T, H * W, max_bubbles, pair_out(links), (char*)ws, links_slot(max_bubbles)};
    static BfPerDeviceOnce once;
    if (const int rc = allow_lds(bubble_links_kernel, once)) return rc;
    hipLaunchKernelGGL(bubble_links_kernel, dim3((unsigned)pairs), dim3(NT), links_lds_bytes(max_bubbles), (hipStream_t)stream, a);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_bubble_track_ids(const int32_t* count, const int32_t* successor, const int32_t* predecessor, int64_t sequences, int T, int max_bubbles,
                                   int32_t* track_id, int32_t* n_tracks, bf_stream_t stream) {
    BF_REQUIRE(sequences > 0 && sequences <= 0x7fffffff && T > 0 && max_bubbles > 0, "bf_bubble_track_ids: bad sizes");
    BF_REQUIRE(max_bubbles <= LINKS_MAX_BUBBLES, "bf_bubble_track_ids: at most 2^15 records per frame");
    BF_REQUIRE(count && track_id && n_tracks && (T == 1 || (successor && predecessor)), "bf_bubble_track_ids: null pointer");
    const TrackArgs a{count, successor, predecessor, track_id, n_tracks, T, max_bubbles};
    hipLaunchKernelGGL(bubble_track_ids_kernel, dim3((unsigned)sequences), dim3(NT), 0, (hipStream_t)stream, a);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_rollout_bubble_links(const bf_rollout_step* s, int max_bubbles, const int32_t* labels, const bf_census_rows* census_pred,
                                       const bf_census_rows* census_tgt, const bf_link_rows* links_pred, const bf_link_rows* links_tgt, void* ws,
                                       int64_t ws_bytes, bf_stream_t stream) {
    RolloutStep v;
    const bf_census_rows *cp = census_pred, *ct = census_tgt;
    const bool ptrs = labels && cp && ct && cp->count && ct->count && cp->attached && ct->attached && cp->area && ct->area && all_rows(links_pred) &&
                      all_rows(links_tgt) && ws;
    if (const int rc = rollout_step_view(v, s, ptrs, s && (int64_t)s->B * s->T <= 0x3fffffff && max_bubbles > 0 && (int64_t)s->steps * s->T >= 2,
                                         "bf_rollout_bubble_links: null pointer", "bf_rollout_bubble_links: bad sizes"))
        return rc;
    BF_REQUIRE(max_bubbles <= LINKS_MAX_BUBBLES, "bf_rollout_bubble_links: at most 2^15 records per frame");
    BF_REQUIRE((int64_t)v.Ho * v.Wo <= LINKS_MAX_CELLS, "bf_rollout_bubble_links: a frame may have at most 2^24 cells");
    BF_REQUIRE(ws_bytes >= bf_bubble_links_ws_bytes(2 * (int64_t)v.B * v.T, max_bubbles),
               "bf_rollout_bubble_links: workspace smaller than bf_bubble_links_ws_bytes(2 B T, max_bubbles)");
    BF_REQUIRE((uintptr_t)ws % 16 == 0, "bf_rollout_bubble_links: the workspace must be 16-byte aligned");
    const RolloutLinksArgs a{v, labels, {cp->count, ct->count}, {cp->attached, ct->attached}, {cp->area, ct->area}, max_bubbles,
                             {pair_out(links_pred), pair_out(links_tgt)}, (char*)ws, links_slot(max_bubbles)};
    static BfPerDeviceOnce once;
    if (const int rc = allow_lds(rollout_links_kernel, once)) return rc;
    hipLaunchKernelGGL(rollout_links_kernel, dim3((unsigned)(v.B * v.T), 2), dim3(NT), links_lds_bytes(max_bubbles), (hipStream_t)stream, a);
    BF_CHECK_LAUNCH();
    return 0;
}

namespace {
bool all_rows(const bf_match_rows* r) { return r && r->match_pred && r->match_target && r->overlap && r->displacement && r->counts && r->mask; }
MatchOut match_out(const bf_match_rows* r) { return MatchOut{r->match_pred, r->match_target, r->overlap, r->displacement, r->counts, r->mask}; }
bool census_read(const bf_census_rows* c) { return c && c->count && c->attached && c->area; }
// per pair: 32 mb bytes of sums, 16 mb of best-partner rows, the table that does not fit LDS; a multiple of 16 (the next slice's sums are 64-bit)
long match_slot(int mb) { return (48L * mb + links_slot(mb) + 15) / 16 * 16; }
}  // namespace

extern "C" int64_t bf_bubble_match_ws_bytes(int64_t pairs, int max_bubbles) {
    if (pairs <= 0 || max_bubbles <= 0 || max_bubbles > LINKS_MAX_BUBBLES) return 0;
    return 16 + pairs * match_slot(max_bubbles);
}

extern "C" int bf_bubble_match(const int32_t* labels_pred, const int32_t* labels_tgt, const bf_census_rows* census_pred, const bf_census_rows* census_tgt,
                               int64_t frames, int H, int W, int max_bubbles, float min_iou, const bf_match_rows* rows, void* ws, int64_t ws_bytes,
                               bf_stream_t stream) {
    BF_REQUIRE(frames > 0 && frames <= 0x7fffffff && H > 0 && W > 0 && max_bubbles > 0, "bf_bubble_match: bad sizes");
    BF_REQUIRE(max_bubbles <= LINKS_MAX_BUBBLES, "bf_bubble_match: at most 2^15 records per frame");
    BF_REQUIRE((int64_t)H * W <= LINKS_MAX_CELLS, "bf_bubble_match: a frame may have at most 2^24 cells");
    BF_REQUIRE(min_iou >= 0.f && min_iou <= 1.f, "bf_bubble_match: min_iou must be in [0, 1]");
    BF_REQUIRE(labels_pred && labels_tgt && census_read(census_pred) && census_read(census_tgt) && all_rows(rows) && ws, "bf_bubble_match: null pointer");
    BF_REQUIRE(ws_bytes >= bf_bubble_match_ws_bytes(frames, max_bubbles), "bf_bubble_match: workspace smaller than bf_bubble_match_ws_bytes");
    BF_REQUIRE((uintptr_t)ws % 16 == 0, "bf_bubble_match: the workspace must be 16-byte aligned");
    const MatchArgs a{{labels_pred, labels_tgt},
                      {{census_pred->count, census_tgt->count}, {census_pred->attached, census_tgt->attached}, {census_pred->area, census_tgt->area}},
                      H * W, W, max_bubbles, min_iou, match_out(rows), (char*)ws, match_slot(max_bubbles)};
    static BfPerDeviceOnce once;
    if (const int rc = allow_lds(bubble_match_kernel, once)) return rc;
    hipLaunchKernelGGL(bubble_match_kernel, dim3((unsigned)frames), dim3(NT), links_lds_bytes(max_bubbles), (hipStream_t)stream, a);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_rollout_bubble_match(const bf_rollout_step* s, int max_bubbles, float min_iou, const int32_t* labels, const bf_census_rows* census_pred,
                                       const bf_census_rows* census_tgt, const bf_match_rows* rows, void* ws, int64_t ws_bytes, bf_stream_t stream) {
    RolloutStep v;
    const bool ptrs = labels && census_read(census_pred) && census_read(census_tgt) && all_rows(rows) && ws;
    if (const int rc = rollout_step_view(v, s, ptrs, s && (int64_t)s->B * s->T <= 0x3fffffff && max_bubbles > 0, "bf_rollout_bubble_match: null pointer",
                                         "bf_rollout_bubble_match: bad sizes"))
        return rc;
    BF_REQUIRE(max_bubbles <= LINKS_MAX_BUBBLES, "bf_rollout_bubble_match: at most 2^15 records per frame");
    BF_REQUIRE((int64_t)v.Ho * v.Wo <= LINKS_MAX_CELLS, "bf_rollout_bubble_match: a frame may have at most 2^24 cells");
    BF_REQUIRE(min_iou >= 0.f && min_iou <= 1.f, "bf_rollout_bubble_match: min_iou must be in [0, 1]");
    BF_REQUIRE(ws_bytes >= bf_bubble_match_ws_bytes((int64_t)v.B * v.T, max_bubbles),
               "bf_rollout_bubble_match: workspace smaller than bf_bubble_match_ws_bytes(B T, max_bubbles)");
    BF_REQUIRE((uintptr_t)ws % 16 == 0, "bf_rollout_bubble_match: the workspace must be 16-byte aligned");
    const RolloutMatchArgs a{v, labels,
                             {{census_pred->count, census_tgt->count}, {census_pred->attached, census_tgt->attached}, {census_pred->area, census_tgt->area}},
                             max_bubbles, min_iou, match_out(rows), (char*)ws, match_slot(max_bubbles)};
    static BfPerDeviceOnce once;
    if (const int rc = allow_lds(rollout_match_kernel, once)) return rc;
    hipLaunchKernelGGL(rollout_match_kernel, dim3((unsigned)(v.B * v.T)), dim3(NT), links_lds_bytes(max_bubbles), (hipStream_t)stream, a);
    BF_CHECK_LAUNCH();
    return 0;
}
