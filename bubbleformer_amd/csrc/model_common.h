// What the stage-level orchestration files (model.hip: the training trunk and the call-to-call record; trunk_eval.hip: the inference
// trunk; embed_debed.hip: patch embed / debed) share, each item once: dims, the arena, GEMM operand / epilogue shorthands, the side
// stream and the per-device record that links one library call to the next, the transient scratch layout and a stage's weight preparation.
// Everything here lives in ONE named namespace with inline members, so every file sees the same types and a function-local static (a
// knob read once) exists once per program.  The record's state has a single definition, in model.hip: see links() / side_defer() below.
#pragma once
#include <algorithm>
#include <functional>
#include <vector>
#include "bf_common.h"
#include "param_reduce.h"
#include <stdlib.h>
#include <string.h>

int bf_gemm_tokred_flush(hipStream_t st);
bool bf_gemm_tokred_pending();

namespace bfm __attribute__((visibility("hidden"))) {      // library-internal: nothing here joins the exported symbol list

struct D {
    int dtype, B, T, h, w, E, heads, attn_scale, feat_scale, patch, cin, cout, nfluid;
    long N, F, S;
    int d, nst;
    size_t es;
};
inline int get_dims(const bf_dims* s, D* o) {
    if (!s) return bf_fail_msg("dims: null", __FILE__, __LINE__);
    o->dtype = s->dtype; o->B = s->B; o->T = s->T; o->h = s->h; o->w = s->w; o->E = s->E; o->heads = s->heads;
    o->attn_scale = s->attn_scale; o->feat_scale = s->feat_scale; o->patch = s->patch; o->cin = s->cin; o->cout = s->cout;
    o->nfluid = s->nfluid;
    if (o->B < 1 || o->T < 1 || o->h < 1 || o->w < 1 || o->E < 8 || o->E > 1024 || o->heads < 1 || o->E % o->heads)
        return bf_fail_msg("dims: bad sizes", __FILE__, __LINE__);
    if (o->dtype != BF_DTYPE_F32 && o->dtype != BF_DTYPE_BF16) return bf_fail_msg("dims: bad dtype", __FILE__, __LINE__);
    o->F = (long)o->B * o->T; o->S = (long)o->h * o->w; o->N = o->F * o->S; o->d = o->E / o->heads;
    o->es = bf_esize(o->dtype);
    const int ch = o->dtype == BF_DTYPE_BF16 ? 8 : 4;
    if (o->E % ch || o->d % ch) return bf_fail_msg("dims: E and head dim must be multiples of the 16-byte chunk", __FILE__, __LINE__);
    if (o->T > 128 || o->h > 128 || o->w > 128) return bf_fail_msg("dims: attention axes are limited to 128 tokens", __FILE__, __LINE__);
    o->nst = 0;
    if (o->patch > 0) {
        int p = o->patch;
        while (p > 1) { if (p & 1) return bf_fail_msg("dims: patch must be a power of two", __FILE__, __LINE__); p >>= 1; o->nst++; }
        if (o->nst < 1 || o->nst > BF_MAX_STAGES) return bf_fail_msg("dims: patch size out of range", __FILE__, __LINE__);
        if (o->nst > 1 && (o->E / 4) % ch) return bf_fail_msg("dims: E/4 must be a multiple of the 16-byte chunk", __FILE__, __LINE__);
    }
    return 0;
}

// bump allocator over a caller-owned buffer, 256-byte aligned pieces
struct Arena {
    char* base; size_t off;
    explicit Arena(void* p) : base((char*)p), off(0) {}
    void* take(size_t bytes) { void* r = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return r; }
    float* f32(size_t n) { return (float*)take(n * 4); }
};

inline bf_operand op_plain(const void* p, long ld, int layout) {
    bf_operand o; memset(&o, 0, sizeof(o)); o.p = p; o.ld = ld; o.layout = layout; return o;
}
inline void op_affine(bf_operand& o, int pro, const float* sc, const float* sh, long rpf, int nch) {
    o.pro = pro; o.sc = sc; o.sh = sh; o.rows_per_frame = (int)rpf; o.nch = nch;
}
// rows are output-resolution pixels (gw x gh grid per frame) of a k2s2 patch over a [.., 2gh, 2gw, C] image
inline void op_gather(bf_operand& o, int gw, int gh, int C) { o.gw = gw; o.gh = gh; o.gc = C; o.seglen = 2 * C; o.segstride = 2L * gw * C; }
inline bf_epilogue epi_store(void* c, long ldc) { bf_epilogue e; memset(&e, 0, sizeof(e)); e.c = c; e.ldc = ldc; e.out_mode = BF_OUT_STORE; return e; }
inline bf_epilogue epi_atomic(float* c, long ldc) { bf_epilogue e = epi_store(c, ldc); e.out_mode = BF_OUT_ATOMIC_F32; return e; }
inline void epi_scatter(bf_epilogue& e, int gw, int gh, int C) { e.gw = gw; e.gh = gh; e.gc = C; e.seglen = 2 * C; e.segstride = 2L * gw * C; }

inline int splitk_for(int M, int N, long K) {
    // the split-K partials are added with fp32 atomics, so splits cost write traffic in proportion to the output size.  An isolated
    // sweep prefers ~64/sqrt(tiles) slices, but inside the full step that loses 5% (A/B on the bench: 351 vs
    // 369 samples/s) to the rule below.
    const long tiles = (long)bf_cdiv(M, 128) * bf_cdiv(N, 128);
    static const long target = bf_knob("BF_SPLITK_TARGET", 256);
    long s = (target + tiles / 2) / tiles;   // ~one wave of tiles over 256 CUs; more slices lose to atomic traffic in the full step
    const long kt = (K + 63) / 64;
    if (s > kt / 4) s = kt / 4;                         // at least 4 K-steps per slice
    if (s < 1) s = 1;
    return (int)s;
}

#define TRY(x) do { int rc__ = (x); if (rc__) return rc__; } while (0)
#define ZERO(ptr, bytes) do { hipError_t e__ = hipMemsetAsync((ptr), 0, (bytes), st); if (e__ != hipSuccess) return bf_fail(e__, __FILE__, __LINE__); } while (0)
#define ZERO_ON(stream, ptr, bytes) do { hipError_t e__ = hipMemsetAsync((ptr), 0, (bytes), (stream)); if (e__ != hipSuccess) return bf_fail(e__, __FILE__, __LINE__); } while (0)
#define HIP_TRY(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) return bf_fail(e__, __FILE__, __LINE__); } while (0)

// ------------------------------------------------------------------------------------------------ side stream
// The backward of every linear layer has two independent GEMMs over the same dy: the data gradient (on the critical path)
// and the weight gradient (needed only by the optimizer).  Alone, each runs ~one wave of tiles with its load / MFMA / epilogue
// phases in lock step across the chip; issued on two HIP streams they interleave and fill each other's bubbles.  The library
// owns one extra stream per device; a stage forks work onto it with an event and joins it before it returns, so the caller
// still sees plain stream-ordered semantics on ITS stream (and the fork/join pattern is hipGraph-capturable).
// BF_SIDE_STREAM=0 runs everything on the caller's stream.  The launch profiler times each kernel with events on the stream it was
// launched on, so its per-kernel durations are the contended ones of the real schedule (they agree with a rocprofv3 trace).
struct SideStream { hipStream_t st = nullptr; hipEvent_t fork = nullptr, join = nullptr, tail[2] = {nullptr, nullptr}; bool failed = false; bool pending[2] = {false, false}; };
// bf_side_defer's process-wide mode (defined in model.hip, with what it means)
bool side_defer();

// ------------------------------------------------------------------------------------------------ what links one call to the next
// Hints for the call made next.  A setter (bf_stage_prepared, bf_stage_chain_next / _head, bf_stage_chain_tail, bf_stage_next_scale) arms
// them; the next trunk stage entry point takes ALL of them out of the record at its top, whatever it then does with them (a call that
// fails early leaves nothing armed for an unrelated later one).  The native trunk driver builds them locally instead: it knows the sequence.
//  * prepared: the stage forward finds its weights prepared in `saved` (bf_prep_stages) and skips its own launch
//  * head: a stage that ends in `out = resid + InstanceNorm(z)` (the spatial stage's MLP branch) or in the out-projection (temporal) leaves the
//    next stage's opening InstanceNorm(out) behind in the same launch (norm.hip InChain, bf_gemm_fwd_frames): that stage's parameters and record
//  * tail: the mirror image in the backward.  The temporal stage's last kernel (QKV data gradient + norm1 backward) produces the output
//    gradient of the spatial stage in front of it, whose backward opens with its MLP-branch InstanceNorm: that stage's parameters, saved
//    record and whether its MLP branch carried stochastic depth
//  * scale: a temporal stage multiplies its incoming gradient by its per-sample stochastic-depth factors before anything else reads it.  That
//    gradient is produced by the last kernel of the spatial stage in front of it: told the factors, the kernel writes the scaled copy as well
//    (one elementwise launch and one read of the gradient less per block)
struct NextHead { bool armed = false; const float *w = nullptr, *b = nullptr; float *mean = nullptr, *rstd = nullptr, *sc = nullptr, *sh = nullptr; void* xn = nullptr; const void* saved = nullptr; };
struct NextTail { bool armed = false; const bf_spatial_params* p = nullptr; const void* saved = nullptr; bool drop = false; };
struct NextScale { const float* f = nullptr; int fdiv = 1; };
struct StageHints { bool prepared = false; NextHead head; NextTail tail; NextScale scale; };

// All InstanceNorm / attention parameter-gradient reductions of one stage backward go out in ONE launch (stage_param_reduce_kernel).  Room for
// a spatial (3 + 2) and a temporal (2 + 1) stage: see TrunkLinks::reduce
struct ReduceJobs {
    static constexpr int IN_CAP = 6, ATTN_CAP = 4;
    int n_in = 0, n_attn = 0; InReduceJob in[IN_CAP]; AttnReduceJob at[ATTN_CAP];
    bool at_follows[ATTN_CAP] = {};      // set at launch: job i adds into job i - 1's slots and runs behind it in the SAME workgroups (see launch_reduce_jobs)
    bool fits(const ReduceJobs& o) const { return n_in + o.n_in <= IN_CAP && n_attn + o.n_attn <= ATTN_CAP; }
    int push(const InReduceJob& j) { BF_REQUIRE(n_in < IN_CAP, "ReduceJobs: more InstanceNorm reductions than one launch holds"); in[n_in++] = j; return 0; }
    int push(const AttnReduceJob& j) { BF_REQUIRE(n_attn < ATTN_CAP, "ReduceJobs: more attention reductions than one launch holds"); at[n_attn++] = j; return 0; }
};

// Host-side state that links one library call to the next: ONE record per device, looked up once by each exported entry point and handed
// down by reference.  The record is per device, not per stream: every item remembers the stream it was made on.  A carry-over item found
// by a call on another stream counts as absent (the consumer recomputes: the unchained path is always right); an obligation is launched
// on the stream that produced its partial sums and the new stream waits for it (`handoff`).  Two trunk passes running CONCURRENTLY on two
// streams of one device remain unsupported: they would interleave their hints and alternation bits.
struct TrunkLinks {
    // ---- 1. hints (see StageHints)
    StageHints hints;
    StageHints take_hints() { const StageHints h = hints; hints = StageHints{}; return h; }
    // ---- 2. carry-over: what one stage call leaves for a later one
    struct HeadDone { const void* saved = nullptr; hipStream_t st = nullptr; } head_done;      // the stage whose norm1 statistics and xn the stage in front left behind (hints.head)
    // the spatial stage whose MLP-branch norm backward the temporal stage behind it applied (hints.tail): dz and the partial sums `ws` are in
    // place -- usable only if that stage's dout IS `dx`, the gradient tensor the chained tail was computed from
    struct TailDone { const void* saved = nullptr; const void* dx = nullptr; float* ws = nullptr; hipStream_t st = nullptr; } tail_done;
    struct DbrReady { const void* dx = nullptr; const float* f = nullptr; void* buf = nullptr; hipStream_t st = nullptr; } dbr_ready;      // the pre-scaled copy `buf` of gradient `dx` (hints.scale)
    // alternation bits.  scratch_parity: the scratch set of a trunk backward stage (deferred mode alternates, so that the side stream may still
    // read the previous stage's set).  tail_ws_flip: where the chained tail leaves the norm's partial sums -- the spatial stage's reduction of
    // them waits for the temporal stage behind it (reduce), whose own chained tail, for the NEXT spatial stage and the same scratch set, must
    // not overwrite them.  dbr_flip: the two pre-scaled gradient buffers -- the temporal stage's side-stream work may still read its copy
    // while the next spatial stage writes the next one
    int scratch_parity = 0; bool tail_ws_flip = false, dbr_flip = false;
    bool take_head_done(const void* saved, hipStream_t st) { const bool hit = head_done.saved == saved && head_done.st == st; head_done = HeadDone{}; return hit; }
    // ---- 3. obligations: GPU work not yet launched that somebody must launch (the deferred slab sum is gemm_tokred.hip's own)
    // Deferred mode (bf_side_defer): the spatial stage's reductions wait for the temporal stage's backward that follows it and ride in ITS launch
    // (one launch per block pair instead of two: 12 launches less on the caller's queue per step).  The two stages use different scratch sets, so
    // the spatial stage's partial sums are intact until the next spatial stage, which flushes a leftover first -- as does every full join.
    struct { ReduceJobs jobs; bool on = false; hipStream_t st = nullptr; } reduce;
    hipEvent_t handoff = nullptr;       // orders an obligation launched on its producing stream before a caller on another one
    // ---- the library's own stream of this device, and saved records whose stage-0 embed map was NOT stored by the forward (host-side memory of
    // a per-call decision; the record itself is device memory)
    SideStream side;
    std::vector<const void*> embed_lean;

    SideStream* side_stream() {
        static const bool enabled = bf_knob("BF_SIDE_STREAM", 1) != 0;
        if (!enabled) return nullptr;
        SideStream& s = side;
        if (!s.st && !s.failed) {
            // lowest priority: the caller's stream is the one a consumer waits on (round 2: +0.3-0.5 % against normal priority; round 3: no
            // difference between lowest, normal and highest)
            int lo = 0, hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&lo, &hi);      // lo = least urgent (numerically greatest)
            // the two streams are on one device: the events need no system-scope fence (an L2 write-back + invalidate at every fork / join)
            const unsigned ef = hipEventDisableTiming | hipEventDisableSystemFence;
            if (hipStreamCreateWithPriority(&s.st, hipStreamNonBlocking, lo) != hipSuccess || hipEventCreateWithFlags(&s.fork, ef) != hipSuccess ||
                hipEventCreateWithFlags(&s.join, ef) != hipSuccess || hipEventCreateWithFlags(&s.tail[0], ef) != hipSuccess ||
                hipEventCreateWithFlags(&s.tail[1], ef) != hipSuccess) { s.failed = true; s.st = nullptr; }
        }
        return s.st ? &s : nullptr;
    }
    // `to` waits for what has been enqueued on `from` so far
    int hand_over(hipStream_t from, hipStream_t to) {
        if (from == to) return 0;
        if (!handoff) HIP_TRY(hipEventCreateWithFlags(&handoff, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(handoff, from));
        HIP_TRY(hipStreamWaitEvent(to, handoff, 0));
        return 0;
    }
    // A forward pass starts at the embed and a backward pass at the debed: what an aborted pass left armed (a hint whose consumer never ran, a
    // "done for" record whose address a later allocation may reuse) must not survive into the next one.
    void clear(bool forward_side) {
        if (forward_side) { hints.prepared = false; hints.head = NextHead{}; head_done = HeadDone{}; }
        hints.tail = NextTail{}; hints.scale = NextScale{}; tail_done = TailDone{}; dbr_ready = DbrReady{};
    }
    bool embed_lean_get(const void* saved) const { return std::find(embed_lean.begin(), embed_lean.end(), saved) != embed_lean.end(); }
    void embed_lean_set(const void* saved, bool lean) {
        const auto it = std::find(embed_lean.begin(), embed_lean.end(), saved);
        if (it == embed_lean.end()) { if (lean) embed_lean.push_back(saved); }
        else if (!lean) { *it = embed_lean.back(); embed_lean.pop_back(); }
    }
};
// the calling thread's current device's record (the table itself is model.hip's)
TrunkLinks& links();
// a spatial stage's parameter reductions waiting for the temporal stage behind it: launched on the stream that made their partial sums
int flush_pending_reduce(TrunkLinks& L, hipStream_t st);
// the previous stage's deferred tail (if any) is ordered before what `main` is given next
int side_join_pending(TrunkLinks& L, hipStream_t main, int set = -1);      // set: 0 / 1 = the work that reads that scratch set, -1 = everything

struct Fork {
    hipStream_t main; SideStream* s; bool used = false; bool deferred; int set;
    std::vector<std::function<int(hipStream_t)>> jobs;          // deferred mode: the stage's side work, launched by flush()
    std::vector<std::function<int(hipStream_t)>> late;          // ... and what must follow the stage's LAST weight-gradient launch (see run_late)
    hipStream_t last_side = nullptr;
    explicit Fork(TrunkLinks& L, hipStream_t m, bool may_defer = false, int scratch_set = 0) : main(m), s(L.side_stream()), set(scratch_set) {
        deferred = may_defer && side_defer() && s != nullptr;
    }
    // stream for work that depends only on what has been issued on `main` so far
    int begin(hipStream_t* out) {
        *out = main;
        if (!s) return 0;
        HIP_TRY(hipEventRecord(s->fork, main));
        HIP_TRY(hipStreamWaitEvent(s->st, s->fork, 0));
        used = true;
        *out = s->st;
        return 0;
    }
    // side work: job(stream) enqueues it.  Eager mode forks here; deferred mode keeps it for flush().
    template <class F> int run(F&& job) {
        hipStream_t ss;
        const int rc = begin(&ss);
        last_side = ss;
        return rc ? rc : job(ss);
    }
    // work that reads the result of a token-reduction GEMM whose slab sum rides in the NEXT such launch (bf_gemm_tokred_deferred): queued here,
    // it runs on the side stream after the stage's remaining weight-gradient launches (join() / flush())
    template <class F> void run_late(F&& job) { late.push_back(job); }
    int drain_late() {
        if (late.empty()) return 0;
        hipStream_t ss = last_side ? last_side : main;
        for (auto& j : late) TRY(j(ss));
        late.clear();
        return 0;
    }
    // deferred mode: one fork for everything collected so far
    int flush() {
        if (!deferred || jobs.empty()) return 0;
        hipStream_t ss;
        TRY(begin(&ss));
        for (auto& j : jobs) TRY(j(ss));
        jobs.clear();
        return 0;
    }
    // everything forked so far is ordered before what `main` is given next (deferred mode: before the next stage's fork point)
    int join() {
        if (deferred) {
            TRY(flush());
            TRY(drain_late());
            if (used) { HIP_TRY(hipEventRecord(s->tail[set], s->st)); s->pending[set] = true; used = false; }
            return 0;
        }
        TRY(drain_late());      // plain stream-ordered semantics: nothing of the stage may stay pending
        if (bf_gemm_tokred_pending()) TRY(bf_gemm_tokred_flush(last_side ? last_side : main));
        if (!s || !used) return 0;
        HIP_TRY(hipEventRecord(s->join, s->st));
        HIP_TRY(hipStreamWaitEvent(main, s->join, 0));
        used = false;
        return 0;
    }
};

// transient scratch (backward is the larger user)
struct Scratch {
    float *G, *csum, *zeros, *ones, *wg, *attn_ws, *attn_ws2, *in_ws, *in_ws2, *in_ws3, *in_ws4, *in_ws5;   // wg: prepared-layout weight gradient scratch; in_ws4 / 5: the chained tails' partials (bf_stage_chain_tail), alternating
    float* tokred_ws; int64_t tokred_floats;      // slabs of the token-reduction (weight-gradient) GEMM
    static constexpr long ATTN_WS_FLOATS = 1024L * (4 * 128 + 32 * 16 + 16);
    void *t1, *t3, *t4, *t1b; int64_t t1b_floats;
    void *s1, *e5, *e6, *e7;     // [N][E] each: s1 feeds side-stream GEMMs only; e5..e7 keep side-stream inputs from being recycled within a stage
    size_t bytes;
    Scratch(const D& d, void* base) {
        Arena a(base);
        const int cm = d.nst > 1 ? d.E / 4 : d.E;
        size_t wgn = (size_t)d.E * d.E;
        wgn = std::max(wgn, (size_t)4 * cm * d.E);             // conv / convT prepared weights
        wgn = std::max(wgn, (size_t)d.E * 64);
        G = a.f32((size_t)d.E * d.E);
        csum = a.f32((size_t)4 * d.E);
        zeros = a.f32((size_t)4 * d.E);
        ones = a.f32((size_t)4 * d.E);
        wg = a.f32(wgn);
        tokred_floats = bf_gemm_tokred_ws_floats(4 * d.E, d.E, d.N);
        tokred_ws = a.f32((size_t)tokred_floats);
        attn_ws = a.f32(ATTN_WS_FLOATS);
        attn_ws2 = a.f32(ATTN_WS_FLOATS);       // second axial pass: both passes' rows are reduced together at the end of the stage
        {   // InstanceNorm workspace: the trunk (S tokens x E) and every embed / debed resolution (S * 4^i tokens x E/4)
            int64_t n = bf_in_ws_floats(d.dtype, (int)d.F, (int)d.S, d.E);
            long Si = d.S;
            for (int i = 1; i < d.nst; ++i) { Si *= 4; n = std::max(n, bf_in_ws_floats(d.dtype, (int)d.F, (int)Si, cm)); }
            in_ws = a.f32((size_t)n);
            // one partials region per InstanceNorm of a block: their reductions run together at the end of the stage
            const size_t nt = (size_t)bf_in_ws_floats(d.dtype, (int)d.F, (int)d.S, d.E);
            in_ws2 = a.f32(nt); in_ws3 = a.f32(nt); in_ws4 = a.f32(nt); in_ws5 = a.f32(nt);
        }
        // activation-sized transients; embed/debed stages work at up to (patch/2)^2 * N pixels of E/4 (or cin/cout) channels
        size_t tok = (size_t)d.N * d.E;
        size_t big = tok * 4;
        if (d.patch > 1) {
            const size_t P0 = (size_t)d.N * (d.patch / 2) * (d.patch / 2);
            const int kp = ((4 * std::max(d.cin, d.cout) + 7) / 8) * 8;
            big = std::max(big, P0 * (size_t)std::max(cm, kp) * 2);   // *2: fp32 patch-major prediction
        }
        t4 = a.take(big * d.es);
        t3 = a.take(std::max(tok * 3, big / 2) * d.es);
        t1 = a.take(std::max(tok, big / 2) * d.es);
        t1b = a.take(std::max(tok, big / 2) * d.es);
        t1b_floats = (int64_t)(std::max(tok, big / 2) * d.es / 4);
        s1 = a.take(tok * d.es); e5 = a.take(tok * d.es); e6 = a.take(tok * d.es); e7 = a.take(tok * d.es);
        bytes = a.off;
    }
};

// ------------------------------------------------------------------------------------------------ a trunk stage's weight preparation
// out-projection fold.  mc[n] = <W[n,:], nb> + bias[n]; alpha = gamma*(1+hi); beta = gamma*(bias*(1+hi) + mc*(lo-hi))
struct PrepArgs { const float *W, *bias, *nb, *gamma, *lo, *hi; float *alpha, *beta, *mc; int E;
                  void* wscaled; int dtype;                                  // wscaled[n][k] = alpha[n] * W[n][k] (compute dtype): the data-gradient GEMM's weight
                  const float *tab_m, *tab_v; float* tab_out; int tab_F;     // optional stochastic-depth table tab_out[f][c] = tab_m[f] * tab_v[c] (E columns)
                  const float* tr_src; void* tr_dst; int tr_R, tr_C; };      // optional transposed bf16 copy tr_dst[c][r] = tr_src[r][c] (the K-contiguous operand of a data gradient / the frame-pair forward)
// up to four plain fp32 -> bf16 weight casts in ONE launch (a stage's projection weights)
struct Cast4 { const float* src[4]; bf16* dst[4]; long n[4]; };
// one stage's preparation: the casts, how many of them (the planes behind them: fold, table, transposed copy) and the fold
struct StagePrep { Cast4 j; int cnt; PrepArgs a; };
// ... and of up to PREP_BATCH stages in one launch (launch_stage_prep)
constexpr int PREP_BATCH = 12;
struct PrepBatch { StagePrep s[PREP_BATCH]; };
// where a stage's prepared operands go; what a caller does not keep is null (the eval arena: no wout_s, no transposed copy, no table)
struct PrepDst { void *win_c, *wout_c, *w1_c, *w2_c; float *alpha, *beta, *mc; void *wout_s, *wt; float* gtab; };

// THE statement of which fp32 parameters of a trunk stage are cast or folded and where the results go: every preparation site (the stage
// forwards, prep_stages, bf_trunk_eval_prepare) asks here.  kind 0: params = bf_temporal_params*, 1: bf_spatial_params*; drop_mlp: the
// spatial stage's MLP-branch stochastic-depth factors or null.
inline StagePrep stage_prep(const D& d, int kind, const void* params, const PrepDst& o, const float* drop_mlp) {
    const long EE = (long)d.E * d.E;
    StagePrep r;
    memset(&r, 0, sizeof(r));
    auto cast = [&r](const float* src, void* dst, long n) { r.j.src[r.cnt] = src; r.j.dst[r.cnt] = (bf16*)dst; r.j.n[r.cnt] = n; ++r.cnt; };
    const float *W, *bias, *nb, *gamma, *lo = nullptr, *hi = nullptr, *tab_v = nullptr, *tr_src;
    int tr_C;
    if (kind == 0) {
        const bf_temporal_params* p = (const bf_temporal_params*)params;
        cast(p->input_head_w, o.win_c, 3 * EE); cast(p->output_head_w, o.wout_c, EE);
        for (int q = 2; q < 4; ++q) { r.j.src[q] = r.j.src[0]; r.j.dst[q] = r.j.dst[0]; }      // unused slots: slot 0 with a count of 0
        W = p->output_head_w; bias = p->output_head_b; nb = p->norm2_b; gamma = p->gamma;
        tr_src = p->output_head_w; tr_C = d.E;                  // W_out^T [E][E]: the frame-pair forward kernel's operand
    } else {
        const bf_spatial_params* p = (const bf_spatial_params*)params;
        cast(p->input_head_w, o.win_c, 3 * EE); cast(p->output_head_w, o.wout_c, EE); cast(p->fc1_w, o.w1_c, 4 * EE); cast(p->fc2_w, o.w2_c, 4 * EE);
        W = p->output_head_w; bias = p->output_head_b; nb = p->norm2_b; gamma = p->gamma_att;
        if (d.feat_scale) { lo = p->low_freq_scalar; hi = p->high_freq_scalar; }
        tab_v = p->gamma_mlp;
        tr_src = p->fc2_w; tr_C = 4 * d.E;                      // fc2.weight^T [4E][E]: K-contiguous operand of the fc2 data gradient
    }
    // gtab[f][c] = drop_mlp[f] * gamma_mlp[c] rides in the same launch only outside fp32 (there spatial_fwd launches frame_table_kernel)
    const bool tab = drop_mlp && tab_v && o.gtab && d.dtype != BF_DTYPE_F32;
    const bool tr = o.wt && d.dtype == BF_DTYPE_BF16;           // the transposed copy is bf16 only
    r.a = PrepArgs{W, bias, nb, gamma, lo, hi, o.alpha, o.beta, o.mc, d.E, o.wout_s, d.dtype,
                   tab ? drop_mlp : nullptr, tab ? tab_v : nullptr, tab ? o.gtab : nullptr, tab ? (int)d.F : 0,
                   tr ? tr_src : nullptr, tr ? o.wt : nullptr, tr ? d.E : 0, tr ? tr_C : 0};
    return r;
}
// stages [0, m) of `b` in one launch (model.hip: stage_prep_multi_kernel); planes = the most casts of a stage + the planes behind them
// that any stage of the batch has (7 with a training record's table and transposed copy, 5 for the eval arena's casts + fold)
int launch_stage_prep(const D& d, const PrepBatch& b, int m, int planes, hipStream_t st);

}  // namespace bfm
