// The training trunk: each FiLMAViT trunk stage (temporal block, axial block) as one stream-ordered chain of the kernels in
// gemm/norm/attn.hip, forward and backward, per stage (bf_temporal_* / bf_spatial_*) and for all stages in one call per direction
// (bf_trunk_train_*) -- plus the state of the per-device record that links one library call to the next (model_common.h: TrunkLinks) and
// the parameter-only kernels of a stage (weight preparation, the fold's parameter gradients, the stage-end reductions).  The inference
// trunk is trunk_eval.hip, patch embed / debed are embed_debed.hip.
// No allocation, no synchronisation: activations that the backward needs live in a caller-owned
// "saved" record per stage, transients in a caller-owned scratch arena.
//
// Algebra used to avoid extra passes (all exact in real arithmetic):
//  * InstanceNorm is applied in the consumer GEMM's operand prologue as a per-(frame, channel) affine;
//    only its statistics are a separate (two-pass, fp32) kernel.
//  * layer scale / residual / feature scaling are folded into the out-projection epilogue
//       out = x + alpha[n] * (on @ W^T)[m, n] + beta[n].
//    The spatial mean over (h, w) that feature scaling needs is data independent: InstanceNorm output has
//    per-channel mean exactly norm2.bias, so mean_hw(y)[n] = W[n, :] . norm2.bias + bias[n]  =: mc[n].
//  * parameter gradients of those folds come from G = dout^T @ on (one split-K GEMM) instead of a saved y:
//       dW = alpha * G (+ dmc x norm2.bias), dalpha[n] = <W[n, :], G[n, :]>, dbeta = colsum(dout).
#include "model_common.h"

bool bf_attn_raw_modes(int dtype, int d);
int bf_gemm_tokred_deferred(int dtype, int Nout, int Kin, int64_t M, const void* dy, int64_t ldy, const void* x, int64_t ldx, float* out,
                            int accumulate, float* colsum, float* ws, int64_t ws_floats, hipStream_t stream);
const float* bf_gemm_tokred_pending_out();
int bf_gemm_inbwd_frames_scaled(int dtype, int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb, const void* x,
                                const void* add, void* out, int S, const float* mean, const float* rstd, const float* w, float* ws,
                                const float* fscale, int fdiv, void* out_s, const float* f_s, int fdiv_s, hipStream_t stream);

using namespace bfm;

namespace {

// bf_side_defer(1): a trunk stage's backward does not join its weight-gradient work before it returns (every fork / join is a
// barrier packet that costs the caller's stream ~6 us, and the wait itself idles it when the side stream is behind).  Consecutive
// stages alternate between two scratch sets and a stage first waits for the side work of the stage before the previous one (the
// last user of its set), so nothing the side stream still reads is overwritten and the side stream may lag by a whole stage.
// Every other stage entry point joins everything at its start, as does bf_side_join().  Off by default: plain stream-ordered
// semantics (every stage joins before it returns).
// A process-wide MODE, not per-device state: bf_side_defer is documented as one and the Python binding's set_side_defer relies on it.
bool g_side_defer = false;

BfPerDevice<TrunkLinks> g_links;

int launch_reduce_jobs(ReduceJobs& J, hipStream_t st);
__global__ void __launch_bounds__(256) stage_prep_multi_kernel(PrepBatch b);

}  // namespace

// what model_common.h declares of the record (qualified definitions: they keep the namespace's hidden visibility)
bool bfm::side_defer() { return g_side_defer; }
TrunkLinks& bfm::links() { return g_links.get(); }
int bfm::flush_pending_reduce(TrunkLinks& L, hipStream_t st) {
    if (!L.reduce.on) return 0;
    L.reduce.on = false;
    TRY(launch_reduce_jobs(L.reduce.jobs, L.reduce.st));
    return L.hand_over(L.reduce.st, st);
}
int bfm::side_join_pending(TrunkLinks& L, hipStream_t main, int set) {
    if (set < 0) TRY(flush_pending_reduce(L, main));
    SideStream* s = L.side_stream();
    if (set < 0 && bf_gemm_tokred_pending()) {               // the last weight-gradient GEMM's slab sum is still pending (bf_gemm_tokred_deferred): run it now
        hipStream_t ws_st = s ? s->st : main;
        TRY(bf_gemm_tokred_flush(ws_st));
        if (s) { HIP_TRY(hipEventRecord(s->join, s->st)); HIP_TRY(hipStreamWaitEvent(main, s->join, 0)); }
    }
    if (!s) return 0;
    for (int i = 0; i < 2; ++i)
        if ((set < 0 || set == i) && s->pending[i]) {
            HIP_TRY(hipStreamWaitEvent(main, s->tail[i], 0));
            s->pending[i] = false;
        }
    return 0;
}
int bfm::launch_stage_prep(const D& d, const PrepBatch& b, int m, int planes, hipStream_t st) {
    hipLaunchKernelGGL(stage_prep_multi_kernel, dim3(std::max(64, d.E), planes, m), dim3(256), 0, st, b);
    BF_CHECK_LAUNCH();
    return 0;
}

namespace {

// J's launch carries the pending jobs where they were made on the same stream and fit; otherwise they go out first, as a launch of their own
int launch_with_pending(TrunkLinks& L, ReduceJobs& J, hipStream_t st) {
    if (L.reduce.on && L.reduce.st == st && J.fits(L.reduce.jobs)) {
        L.reduce.on = false;
        const ReduceJobs& P = L.reduce.jobs;
        for (int i = 0; i < P.n_in; ++i) TRY(J.push(P.in[i]));
        for (int i = 0; i < P.n_attn; ++i) TRY(J.push(P.at[i]));
    }
    TRY(flush_pending_reduce(L, st));
    return launch_reduce_jobs(J, st);
}

// ------------------------------------------------------------------------------------------------ small param kernels
// out-projection fold (model_common.h: PrepArgs)
__device__ __forceinline__ void outproj_prep_row(const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ nb,
                                                 const float* __restrict__ gamma, const float* __restrict__ lo, const float* __restrict__ hi,
                                                 float* __restrict__ alpha, float* __restrict__ beta, float* __restrict__ mc, int E, int n,
                                                 void* __restrict__ wscaled, int dtype) {
    __shared__ float red[4];
    __shared__ float s_alpha;
    float acc = 0.f;
    if (lo) for (int k = threadIdx.x; k < E; k += blockDim.x) acc += W[(long)n * E + k] * nb[k];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float m = bias[n];
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) m += red[i];
        const float l = lo ? lo[n] : 0.f, h = hi ? hi[n] : 0.f, g = gamma[n];
        alpha[n] = g * (1.f + h);
        beta[n] = g * (bias[n] * (1.f + h) + (lo ? m * (l - h) : 0.f));
        mc[n] = m;
        s_alpha = g * (1.f + h);
    }
    if (wscaled) {
        __syncthreads();
        const float al = s_alpha;
        for (int k = threadIdx.x; k < E; k += blockDim.x) {
            const float v = al * W[(long)n * E + k];
            if (dtype == BF_DTYPE_BF16) reinterpret_cast<bf16*>(wscaled)[(long)n * E + k] = (bf16)v;
            else reinterpret_cast<float*>(wscaled)[(long)n * E + k] = v;
        }
    }
}
__global__ void __launch_bounds__(256) outproj_prep_kernel(PrepArgs a) {
    outproj_prep_row(a.W, a.bias, a.nb, a.gamma, a.lo, a.hi, a.alpha, a.beta, a.mc, a.E, blockIdx.x, a.wscaled, a.dtype);
}
// parameter gradients of the fold (see header comment).  grid = E rows.
__global__ void outproj_finalize_kernel(const float* __restrict__ G, const float* __restrict__ csum, const float* __restrict__ W,
                                        const float* __restrict__ bias, const float* __restrict__ nb, const float* __restrict__ gamma,
                                        const float* __restrict__ lo, const float* __restrict__ hi, const float* __restrict__ mc,
                                        float* __restrict__ dW, float* __restrict__ dbias, float* __restrict__ dnb, float* __restrict__ dgamma,
                                        float* __restrict__ dlo, float* __restrict__ dhi, int E) {
    __shared__ float red[4];
    __shared__ float s_dmc, s_alpha;
    if ((int)blockIdx.x >= E) {      // extra workgroups (feature scaling only): dnb[k] += sum_n dmc[n] * W[n][k], 16 columns each -- dmc[n] =
        // csum[n] * gamma[n] * (lo[n] - hi[n]) needs nothing the row workgroups compute, and one writer per column replaces E x E float
        // atomics on E addresses (the launch took 14 us with them)
        // 16 columns x 16 row groups per workgroup (row group q: rows q, q + 16, ...): with 64 columns x 4 row groups a thread walked 96 rows in
        // twelve dependent batches of eight loads, ~24 us on six workgroups while the rest of the launch took 5 -- the whole launch waited
        // for them (26 us, 24 times a step on the side queue).  Now three batches.
        __shared__ float part[16][16];
        __shared__ float coef[1024];           // dmc[n] (E <= 1024: host-checked)
        for (int n = threadIdx.x; n < E; n += blockDim.x) coef[n] = csum[n] * gamma[n] * (lo[n] - hi[n]);
        __syncthreads();
        const int c = threadIdx.x & 15, k = ((int)blockIdx.x - E) * 16 + c, q = threadIdx.x >> 4;
        float a = 0.f;
        if (k < E) {
            int n = q;
            for (; n + 112 < E; n += 128) {      // eight rows of W in flight per thread (a load-then-add loop pays a round trip per row)
                float wv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) wv[u] = W[(long)(n + 16 * u) * E + k];
#pragma unroll
                for (int u = 0; u < 8; ++u) a = fmaf(coef[n + 16 * u], wv[u], a);
            }
            for (; n < E; n += 16) a = fmaf(coef[n], W[(long)n * E + k], a);
        }
        part[q][c] = a;
        __syncthreads();
        // one atomic per column: the caller's stream adds norm2's own bias gradient to the same addresses at the same time (the stage's
        // InReduceJob) -- two addends on a zeroed slot give the same bits in either order, a plain += could lose one of them
        if (q == 0 && k < E) {
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) t += part[i][c];      // fixed order
            atomicAdd(dnb + k, t);
        }
        return;
    }
    const int n = blockIdx.x;
    float acc = 0.f;
    for (int k = threadIdx.x; k < E; k += blockDim.x) acc += W[(long)n * E + k] * G[(long)n * E + k];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float dalpha = 0.f;
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) dalpha += red[i];
        const float dbeta = csum[n];
        const float l = lo ? lo[n] : 0.f, h = hi ? hi[n] : 0.f, g = gamma[n], b = bias[n], m = mc[n];
        const float mterm = lo ? m * (l - h) : 0.f;
        dgamma[n] += dalpha * (1.f + h) + dbeta * (b * (1.f + h) + mterm);
        float dmc = 0.f;
        if (lo) {
            dhi[n] += dalpha * g + dbeta * g * (b - m);
            dlo[n] += dbeta * g * m;
            dmc = dbeta * g * (l - h);
        }
        dbias[n] += dbeta * g * (1.f + h) + dmc;
        s_dmc = dmc;
        s_alpha = g * (1.f + h);
    }
    __syncthreads();
    const float dmc = s_dmc, alpha = s_alpha;
    for (int k = threadIdx.x; k < E; k += blockDim.x) {
        float v = alpha * G[(long)n * E + k];
        if (lo) v += dmc * nb[k];
        dW[(long)n * E + k] += v;
    }
}
// stochastic-depth helper: out[f][c] = m[f / fdiv] * (v ? v[c] : 1)
__global__ void frame_table_kernel(const float* __restrict__ m, int fdiv, const float* __restrict__ v, float* __restrict__ out, int F, int C) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)F * C) return;
    const int f = (int)(i / C), c = (int)(i % C);
    out[i] = m[f / fdiv] * (v ? v[c] : 1.f);
}

// dst[c][r] = (bf16) src[r][c] (R x C fp32 -> C x R bf16) in 64 x 64 tiles through LDS: coalesced 16-byte reads along c, 16-byte stores along r
// (the first form read 8 rows per thread with a stride of C floats: every 4-byte read its own cache line -- 16x the bytes of the weight).
// `tile0`, `tstride`: the calling workgroup's first tile and the tile stride (256 threads; R, C multiples of 64).
__device__ __forceinline__ void transpose_cast(const float* __restrict__ src, bf16* __restrict__ dst, int R, int C, int tile0, int tstride) {
    __shared__ float tl[64][65];
    const int tr_ = (R + 63) / 64, tc_ = (C + 63) / 64;      // (R, C are multiples of 8: whole float4 reads, whole 8-row stores; edge tiles are partial)
    const int tid = threadIdx.x;
    for (int t = tile0; t < tr_ * tc_; t += tstride) {
        const int r0 = (t / tc_) * 64, c0 = (t % tc_) * 64;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {                  // 64 rows x 16 float4
            const int i = tid + 256 * k, r = i >> 4, c4 = (i & 15) * 4;
            if (r0 + r < R && c0 + c4 < C) {
                const float4 v = *reinterpret_cast<const float4*>(src + (long)(r0 + r) * C + c0 + c4);
                tl[r][c4] = v.x; tl[r][c4 + 1] = v.y; tl[r][c4 + 2] = v.z; tl[r][c4 + 3] = v.w;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; ++k) {                  // 64 columns x 8 groups of 8 rows
            const int i = tid + 256 * k, c = i >> 3, r8 = (i & 7) * 8;
            if (c0 + c < C && r0 + r8 < R) {
                bf16x8 o;
#pragma unroll
                for (int q = 0; q < 8; ++q) o[q] = (bf16)tl[r8 + q][c];
                *reinterpret_cast<bf16x8*>(dst + (long)(c0 + c) * R + r0 + r8) = o;
            }
        }
    }
}
// The planes of a stage's preparation, each written once (256 threads; cast4_kernel, stage_prep_kernel and stage_prep_multi_kernel call them).
// cast: one of up to four plain fp32 -> bf16 weight casts (a stage's projection weights), grid-stride over 16-byte groups
__device__ __forceinline__ void prep_cast(const Cast4& j, int w) {
    const long n4 = j.n[w] / 4;
    const float4* s4 = reinterpret_cast<const float4*>(j.src[w]);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 v = s4[i];
        const bf16x4 o = {(bf16)v.x, (bf16)v.y, (bf16)v.z, (bf16)v.w};
        *reinterpret_cast<bf16x4*>(j.dst[w] + 4 * i) = o;
    }
}
// table: the stage's stochastic-depth table (frame_table_kernel's work, no launch of its own)
__device__ __forceinline__ void prep_table(const PrepArgs& a) {
    if (!a.tab_out) return;
    const long n = (long)a.tab_F * a.E;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) a.tab_out[i] = a.tab_m[i / a.E] * a.tab_v[i % a.E];
}
__device__ __forceinline__ void prep_transposed(const PrepArgs& a) {
    if (a.tr_dst) transpose_cast(a.tr_src, (bf16*)a.tr_dst, a.tr_R, a.tr_C, (int)blockIdx.x, (int)gridDim.x);
}
// grid rows [0, cnt): the casts; cnt: the fold; cnt + 1: the table; cnt + 2: the transposed copy -- a stage's parameter-only work in ONE launch
__device__ __forceinline__ void prep_plane(const Cast4& j, int cnt, const PrepArgs& a) {
    const int y = blockIdx.y;
    if (y == cnt + 2) prep_transposed(a);
    else if (y == cnt + 1) prep_table(a);
    else if (y == cnt) {       // the fold: one workgroup per output channel
        if ((int)blockIdx.x < a.E) outproj_prep_row(a.W, a.bias, a.nb, a.gamma, a.lo, a.hi, a.alpha, a.beta, a.mc, a.E, blockIdx.x, a.wscaled, a.dtype);
    }
    else prep_cast(j, y);
}
__global__ void __launch_bounds__(256) cast4_kernel(Cast4 j) { prep_cast(j, blockIdx.y); }
__global__ void __launch_bounds__(256) stage_prep_kernel(Cast4 j, int cnt, PrepArgs a) { prep_plane(j, cnt, a); }
// ... and the same for up to PREP_BATCH stages in one launch (blockIdx.z = stage): bf_prep_stages, bf_trunk_eval_prepare
__global__ void __launch_bounds__(256) stage_prep_multi_kernel(PrepBatch b) {
    const StagePrep& s = b.s[blockIdx.z];
    if ((int)blockIdx.y > s.cnt + 2) return;      // the grid has the planes of the batch's largest stage
    prep_plane(s.j, s.cnt, s.a);
}
// a stage's weights as compute-dtype operands, out[i] for i < cnt: aliases of the fp32 parameters in f32 mode (one launch for the fold),
// the bf16 copies in bf16 mode -- made here in one launch with the fold (`fold`), or by a cast-only launch, or already in place (`ready`:
// bf_prep_stages made them)
int wviews(const D& d, const StagePrep& sp, bool ready, const void** out, hipStream_t st, bool fold = true) {
    const bool f32 = d.dtype == BF_DTYPE_F32;
    for (int i = 0; i < sp.cnt; ++i) out[i] = f32 ? (const void*)sp.j.src[i] : (const void*)sp.j.dst[i];
    if (f32) {
        if (fold) { hipLaunchKernelGGL(outproj_prep_kernel, dim3(sp.a.E), dim3(256), 0, st, sp.a); BF_CHECK_LAUNCH(); }
        return 0;
    }
    if (ready) return 0;
    if (fold) hipLaunchKernelGGL(stage_prep_kernel, dim3(std::max(64, sp.a.E), sp.cnt + (sp.a.tr_dst ? 3 : sp.a.tab_out ? 2 : 1)), dim3(256), 0, st, sp.j, sp.cnt, sp.a);
    else hipLaunchKernelGGL(cast4_kernel, dim3(64, sp.cnt), dim3(256), 0, st, sp.j);
    BF_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------ saved-record layouts
struct TemporalSaved {
    float *mean1, *rstd1, *sc1, *sh1, *mean2, *rstd2, *sc2, *sh2, *alpha, *beta, *mc;
    void *qkv, *o, *xn, *on, *win_c, *wout_c, *wout_s;      // wout_s = diag(alpha) W_out (data-gradient operand); xn / on: InstanceNorm'd block input / attention output (GEMM operands, fwd and dW)
    void* wout_t;                                           // W_out^T [in][out]: the frame-pair forward kernel's operand (bf_gemm_fwd_frames)
    size_t bytes;
    TemporalSaved(const D& d, void* base) {
        Arena a(base);
        const size_t fe = (size_t)d.F * d.E;
        mean1 = a.f32(fe); rstd1 = a.f32(fe); sc1 = a.f32(fe); sh1 = a.f32(fe);
        mean2 = a.f32(fe); rstd2 = a.f32(fe); sc2 = a.f32(fe); sh2 = a.f32(fe);
        alpha = a.f32(d.E); beta = a.f32(d.E); mc = a.f32(d.E);
        qkv = a.take((size_t)d.N * 3 * d.E * d.es);
        o = a.take((size_t)d.N * d.E * d.es);
        xn = a.take((size_t)d.N * d.E * d.es);
        on = a.take((size_t)d.N * d.E * d.es);
        win_c = a.take((size_t)3 * d.E * d.E * d.es);
        wout_c = a.take((size_t)d.E * d.E * d.es);
        wout_s = a.take((size_t)d.E * d.E * d.es);
        wout_t = a.take((size_t)d.E * d.E * d.es);
        bytes = a.off;
    }
    PrepDst prep_dst() const { return PrepDst{win_c, wout_c, nullptr, nullptr, alpha, beta, mc, wout_s, wout_t, nullptr}; }
};
struct SpatialSaved {
    float *mean1, *rstd1, *sc1, *sh1, *mean2, *rstd2, *sc2, *sh2, *mean3, *rstd3, *sc3, *sh3, *alpha, *beta, *mc, *gtab;
    void *qkv, *o, *xn, *on, *x1, *pre, *hid, *z, *win_c, *wout_c, *wout_s, *w1_c, *w2_c, *w2t_c;      // w2t_c = fc2.weight^T [4E][E]: K-contiguous operand of the fc2 data gradient
    size_t bytes;
    SpatialSaved(const D& d, void* base) {
        Arena a(base);
        const size_t fe = (size_t)d.F * d.E;
        mean1 = a.f32(fe); rstd1 = a.f32(fe); sc1 = a.f32(fe); sh1 = a.f32(fe);
        mean2 = a.f32(fe); rstd2 = a.f32(fe); sc2 = a.f32(fe); sh2 = a.f32(fe);
        mean3 = a.f32(fe); rstd3 = a.f32(fe); sc3 = a.f32(fe); sh3 = a.f32(fe);
        alpha = a.f32(d.E); beta = a.f32(d.E); mc = a.f32(d.E); gtab = a.f32(fe);
        qkv = a.take((size_t)d.N * 3 * d.E * d.es);
        o = a.take((size_t)d.N * d.E * d.es);
        xn = a.take((size_t)d.N * d.E * d.es);
        on = a.take((size_t)d.N * d.E * d.es);
        x1 = a.take((size_t)d.N * d.E * d.es);
        pre = a.take((size_t)d.N * 4 * d.E * d.es);
        hid = a.take((size_t)d.N * 4 * d.E * d.es);
        z = a.take((size_t)d.N * d.E * d.es);
        win_c = a.take((size_t)3 * d.E * d.E * d.es);
        wout_c = a.take((size_t)d.E * d.E * d.es);
        wout_s = a.take((size_t)d.E * d.E * d.es);
        w1_c = a.take((size_t)4 * d.E * d.E * d.es);
        w2_c = a.take((size_t)4 * d.E * d.E * d.es);
        w2t_c = a.take((size_t)4 * d.E * d.E * d.es);
        bytes = a.off;
    }
    PrepDst prep_dst() const { return PrepDst{win_c, wout_c, w1_c, w2_c, alpha, beta, mc, wout_s, w2t_c, gtab}; }
};


// ------------------------------------------------------------------------------------------------ stage-end parameter reductions
// All InstanceNorm / attention parameter-gradient reductions of one stage backward in ONE launch (grid z = job): nothing on the
// critical path reads them, and eight dependent ~5 us launches per block are worth ~3 % of the step.
__global__ void __launch_bounds__(64 * BF_RED_FL) stage_param_reduce_kernel(ReduceJobs J) {
    __shared__ float red[5][BF_RED_FL][64];
    const int z = blockIdx.z;
    if (z < J.n_in) {
        const InReduceJob& j = J.in[z];
        if ((int)blockIdx.x < (j.C + 63) / 64 && (int)blockIdx.y < (j.frames + j.rdiv() - 1) / j.rdiv()) in_reduce_block(j, blockIdx.x, blockIdx.y, red);
    } else {
        int a = z - J.n_in;
        if (J.at_follows[a]) return;             // done by the workgroups of the job it follows
        for (;; ++a) {
            const AttnReduceJob& j = J.at[a];
            const int nvals = 4 * j.D + 32 * j.heads + j.heads;
            if ((int)blockIdx.x < (nvals + 63) / 64 && blockIdx.y == 0) attn_reduce_block(j, blockIdx.x, 0, 1, red);
            if (a + 1 >= J.n_attn || !J.at_follows[a + 1]) break;
            __syncthreads();                     // `red` is reused
        }
    }
}
int launch_reduce_jobs(ReduceJobs& J, hipStream_t st) {
    int k = 0;                                   // drop attention jobs without rows (no workspace: the kernel accumulated directly)
    for (int i = 0; i < J.n_attn; ++i) if (J.at[i].rows > 0) J.at[k++] = J.at[i];
    J.n_attn = k;
    // two jobs on the same slots (the W and the H pass of a spatial stage share their LayerNorms and bias table): each value's thread adds
    // the first job's sum, then the second's -- slot + a + b in that order.  As two concurrent workgroups they were order free only on a
    // zeroed slot (0 + a + b); under gradient accumulation the slot holds the earlier micro-batches' sum.
    for (int i = 0; i < J.n_attn; ++i)
        J.at_follows[i] = i > 0 && J.at[i].D == J.at[i - 1].D && J.at[i].heads == J.at[i - 1].heads &&
                          ((J.at[i].dqw && J.at[i].dqw == J.at[i - 1].dqw) || (J.at[i].demb && J.at[i].demb == J.at[i - 1].demb));
    if (J.n_in + J.n_attn == 0) return 0;
    int gx = 1, gy = 1;
    for (int i = 0; i < J.n_in; ++i) { gx = std::max(gx, bf_cdiv(J.in[i].C, 64)); gy = std::max(gy, bf_cdiv(J.in[i].frames, J.in[i].rdiv())); }
    for (int i = 0; i < J.n_attn; ++i) { gx = std::max(gx, bf_cdiv(4 * J.at[i].D + 33 * J.at[i].heads, 64)); }
    hipLaunchKernelGGL(stage_param_reduce_kernel, dim3(gx, gy, J.n_in + J.n_attn), dim3(64 * BF_RED_FL), 0, st, J);
    BF_CHECK_LAUNCH();
    return 0;
}

// QKV projection + attention shared pieces -------------------------------------------------------
// The InstanceNorm'd operand is materialised by the statistics kernel itself (bf_in_stats_apply: the frame is in registers there),
// so the projection GEMMs run the prologue-free, double-buffered-LDS kernel and the weight-gradient GEMMs reuse the same tensor.
int qkv_gemm(const D& d, const void* xn, const void* w_c, const float* bias, void* qkv, hipStream_t st) {
    bf_operand A = op_plain(xn, d.E, BF_LAY_KC);
    bf_operand Bo = op_plain(w_c, d.E, BF_LAY_KC);
    bf_epilogue e = epi_store(qkv, 3L * d.E);
    e.bias = bias;
    return bf_gemm(d.dtype, (int)d.N, 3 * d.E, d.E, &A, &Bo, &e, 1, st);
}
// out = x + alpha * (affine(o) @ W^T) + beta
int outproj_gemm(const D& d, const void* on, const void* w_c, const float* alpha, const float* beta,
                 const void* resid, void* out, const float* drop, long rows_per_group, hipStream_t st) {
    bf_operand A = op_plain(on, d.E, BF_LAY_KC);
    bf_operand Bo = op_plain(w_c, d.E, BF_LAY_KC);
    bf_epilogue e = epi_store(out, d.E);
    e.colscale = alpha; e.colshift = beta; e.aux_mode = BF_AUX_ADD; e.aux = resid; e.ld_aux = d.E;
    e.rowscale = drop; e.rows_per_group = (int)rows_per_group;
    return bf_gemm(d.dtype, (int)d.N, d.E, d.E, &A, &Bo, &e, 1, st);
}
// scratch set of a trunk backward stage (TrunkLinks::scratch_parity)
void* bwd_scratch(TrunkLinks& L, const D& d, void* scratch) {
    if (!g_side_defer || !L.side_stream()) return scratch;
    L.scratch_parity ^= 1;
    return (char*)scratch + (size_t)L.scratch_parity * Scratch(d, nullptr).bytes;
}
// A data gradient dy @ W whose consumer is the backward of the InstanceNorm that fed the projection: when a frame is one
// 144-row GEMM tile the two run as ONE kernel (gemm_frame.hip); otherwise GEMM into `tmp`, then the InstanceNorm backward.
// the backward of the NEXT InstanceNorm in line, applied by the same launch where the frame-pair kernel covers it (bf_gemm_inbwd_frames_chain)
struct TailNorm { const void* z; void* dz; const float *mean, *rstd, *w, *g; int gdiv; float* ws; bool* done; };
struct InFuse { const void* x; const void* add; void* dx; const float* mean; const float* rstd; const float* w; const float* b; float* ws;
                const float* fscale = nullptr; int fdiv = 1;         // fscale: optional per-frame-group factor on dy (stochastic depth)
                const TailNorm* tail = nullptr;
                void* scaled_out = nullptr; const float* scaled_f = nullptr; int scaled_fdiv = 1; bool* scaled_done = nullptr; };      // optional second copy dx * scaled_f[frame / fdiv]
int dgrad_inbwd(const D& d, const void* dy, int Kdim, const void* w_xc, int Nout, void* tmp, const InFuse& f, hipStream_t st) {
    if (f.tail) {
        const TailNorm& t = *f.tail;
        const int crc = bf_gemm_inbwd_frames_chain(d.dtype, (int)d.N, Nout, Kdim, dy, Kdim, w_xc, Nout, f.x, f.add, f.dx, (int)d.S, f.mean, f.rstd, f.w, f.ws,
                                                   f.fscale, f.fdiv, t.z, t.dz, t.mean, t.rstd, t.w, t.g, t.gdiv, t.ws, st);
        if (crc < 0) return crc;
        if (crc == 0) { *t.done = true; return 0; }
    }
    if (f.scaled_out) {
        const int src = bf_gemm_inbwd_frames_scaled(d.dtype, (int)d.N, Nout, Kdim, dy, Kdim, w_xc, Nout, f.x, f.add, f.dx, (int)d.S, f.mean, f.rstd, f.w, f.ws,
                                                    f.fscale, f.fdiv, f.scaled_out, f.scaled_f, f.scaled_fdiv, st);
        if (src < 0) return src;
        if (src == 0) { *f.scaled_done = true; return 0; }
    }
    const int rc = bf_gemm_inbwd_frames(d.dtype, (int)d.N, Nout, Kdim, dy, Kdim, w_xc, Nout, f.x, f.add, f.dx, (int)d.S, f.mean, f.rstd, f.w, f.ws,
                                        f.fscale, f.fdiv, st);
    if (rc <= 0) return rc;
    bf_operand A = op_plain(dy, Kdim, BF_LAY_KC);
    bf_operand Bo = op_plain(w_xc, Nout, BF_LAY_XC);
    bf_epilogue e = epi_store(tmp, Nout);
    if (f.fscale) { e.rowscale = f.fscale; e.rows_per_group = (int)(d.S * f.fdiv); }
    TRY(bf_gemm(d.dtype, (int)d.N, Nout, Kdim, &A, &Bo, &e, 1, st));
    return bf_in_bwd_partials(d.dtype, tmp, f.x, f.add, f.dx, (int)d.F, (int)d.S, Nout, f.mean, f.rstd, f.w, f.b, nullptr, 1, 0, f.ws, st);
}
// backward of the folded out-projection: param grads + don = (dout * alpha) @ W
int outproj_bwd(const D& d, const Scratch& sc, const void* dout, const void* on, const void* w_s,
                const float* W, const float* bias, const float* nb, const float* gamma, const float* lo, const float* hi,
                const float* alpha, const float* mc, float* dW, float* dbias, float* dnb, float* dgamma, float* dlo, float* dhi,
                void* don, hipStream_t st, Fork& fk, const InFuse* fu = nullptr) {
    TRY(fk.run([=](hipStream_t ss) -> int {           // parameter-gradient side: G GEMM, finalize
        const void* dsrc = dout;
        // G[n][k] = sum_m dout[m][n] * on[m][k]; `on` is the normalised operand the forward saved; dbeta = colsum(dout) from the same pass
        const int trc = bf_gemm_tokred_deferred(d.dtype, d.E, d.E, d.N, dsrc, d.E, on, d.E, sc.G, 0, sc.csum, sc.tokred_ws, sc.tokred_floats, ss);
        if (trc < 0) return trc;
        if (trc == 1) {
            ZERO_ON(ss, sc.G, (size_t)((char*)sc.csum - (char*)sc.G) + (size_t)d.E * 4);     // G and csum are adjacent in the arena: one memset
            bf_operand A = op_plain(dsrc, d.E, BF_LAY_XC);
            bf_operand Bo = op_plain(on, d.E, BF_LAY_XC);
            bf_epilogue e = epi_atomic(sc.G, d.E);
            e.colsum = sc.csum;                  // dbeta = colsum(dout), fused into the same pass over dout
            TRY(bf_gemm(d.dtype, d.E, d.E, (int)d.N, &A, &Bo, &e, splitk_for(d.E, d.E, d.N), ss));
        }
        return 0;
    }));
    // G's slab sum rides in the stage's NEXT weight-gradient launch (bf_gemm_tokred_deferred): the fold's parameter gradients, which read G, follow
    // the stage's last such launch on the side stream (or flush the sum themselves when nothing followed)
    fk.run_late([=](hipStream_t ss) -> int {
        if (bf_gemm_tokred_pending_out() == sc.G) TRY(bf_gemm_tokred_flush(ss));
        hipLaunchKernelGGL(outproj_finalize_kernel, dim3(d.E + (lo ? bf_cdiv(d.E, 16) : 0)), dim3(256), 0, ss, sc.G, sc.csum, W, bias, nb, gamma, lo, hi, mc,
                           dW, dbias, dnb, dgamma, dlo, dhi, d.E);
        BF_CHECK_LAUNCH();
        return 0;
    });
    if (fu) return dgrad_inbwd(d, dout, d.E, w_s, d.E, don, *fu, st);      // ... followed by norm2's backward
    {   // don = (dout * alpha) @ W = dout @ (diag(alpha) W): the scaled weight was written by the forward's parameter prep
        bf_operand A = op_plain(dout, d.E, BF_LAY_KC);
        bf_operand Bo = op_plain(w_s, d.E, BF_LAY_XC);
        bf_epilogue e = epi_store(don, d.E);
        TRY(bf_gemm(d.dtype, (int)d.N, d.E, d.E, &A, &Bo, &e, 1, st));
    }
    return 0;
}
// backward of y = affine(x) @ W^T + b:  dW += dy^T affine(x), db += colsum(dy), dxn = dy @ W
int linear_bwd(const D& d, const Scratch& sc, const void* dy, int Nout, const void* x, int Kin, int xpro, const float* xsc, const float* xsh,
               const void* w_c, float* dW, float* db, void* dxn, const bf_epilogue* dx_epi, hipStream_t st, Fork& fk, const InFuse* fu = nullptr,
               bool last = false, const void* w_t = nullptr, void* scaled_out = nullptr, const float* rowfac = nullptr, int rpg = 1,
               bool* scaled_done = nullptr) {      // w_t: the weight transposed ([Kin][Nout], K-contiguous for the data gradient)
    TRY(fk.run([=](hipStream_t ss) -> int {      // weight gradient: side stream
        const void* xo = x;
        int pro = xpro;
        bf_operand A = op_plain(dy, Nout, BF_LAY_XC);
        if (pro == BF_PRO_AFFINE) {              // see outproj_bwd: materialise the normalised operand once
            TRY(bf_affine_apply(d.dtype, x, nullptr, xsc, xsh, sc.s1, d.N, (int)d.S, Kin, ss));
            xo = sc.s1;
            pro = BF_PRO_NONE;
        }
        bf_operand Bo = op_plain(xo, Kin, BF_LAY_XC);
        if (pro == BF_PRO_NONE) {
            const int trc = bf_gemm_tokred_deferred(d.dtype, Nout, Kin, d.N, dy, Nout, xo, Kin, dW, 1, db, sc.tokred_ws, sc.tokred_floats, ss);
            if (trc <= 0) return trc;
        }
        if (pro != BF_PRO_NONE) op_affine(Bo, pro, xsc, xsh, d.S, Kin);
        bf_epilogue e = epi_atomic(dW, Kin);
        e.colsum = db;                       // bias gradient = colsum(dy), fused into the same pass over dy
        return bf_gemm(d.dtype, Nout, Kin, (int)d.N, &A, &Bo, &e, splitk_for(Nout, Kin, d.N), ss);
    }));
    if (last) TRY(fk.flush());                   // deferred mode: the stage's one fork, ahead of its last kernel on the caller's stream
    if (fu) return dgrad_inbwd(d, dy, Nout, w_c, Kin, dxn, *fu, st);
    {
        bf_operand A = op_plain(dy, Nout, BF_LAY_KC);
        bf_operand Bo = w_t ? op_plain(w_t, Nout, BF_LAY_KC) : op_plain(w_c, Kin, BF_LAY_XC);      // K-contiguous: the streaming kernel's form
        bf_epilogue e = dx_epi ? *dx_epi : epi_store(dxn, Kin);
        e.c = dxn; e.ldc = Kin;
        if (scaled_out && rowfac && d.dtype == BF_DTYPE_BF16) {      // the row-scaled copy of dxn from the same kernel, where its shape is covered
            const int rc = bf_gemm_pair_scaled((int)d.N, Kin, Nout, &A, &Bo, &e, scaled_out, rowfac, rpg, st);
            if (rc < 0) return rc;
            if (rc == 0) { if (scaled_done) *scaled_done = true; return 0; }
        }
        TRY(bf_gemm(d.dtype, (int)d.N, Kin, Nout, &A, &Bo, &e, 1, st));
    }
    return 0;
}

}  // namespace

// ================================================================================================= sizes
extern "C" int64_t bf_temporal_saved_bytes(const bf_dims* s) { D d; if (get_dims(s, &d)) return -1; return (int64_t)TemporalSaved(d, nullptr).bytes; }
extern "C" int64_t bf_spatial_saved_bytes(const bf_dims* s) { D d; if (get_dims(s, &d)) return -1; return (int64_t)SpatialSaved(d, nullptr).bytes; }
// two scratch sets: consecutive trunk backward stages alternate between them in deferred mode (see SideStream)
// ... and, behind them, two [N][E] buffers for the pre-scaled gradient a spatial stage leaves for the temporal stage behind it (bf_stage_next_scale)
static size_t dbr_bytes(const D& d) { return (((size_t)d.N * d.E * d.es) + 255) & ~(size_t)255; }
extern "C" int64_t bf_scratch_bytes(const bf_dims* s) { D d; if (get_dims(s, &d)) return -1; return 2 * (int64_t)Scratch(d, nullptr).bytes + 2 * (int64_t)dbr_bytes(d); }

// Deferred weight-gradient tails (see SideStream): opt-in for callers that join explicitly before they consume parameter gradients
extern "C" void bf_side_defer(int on) { g_side_defer = on != 0; }
extern "C" int bf_side_join(bf_stream_t s) { return side_join_pending(g_links.get(), (hipStream_t)s); }

// ================================================================================================= hint setters (see StageHints)
// The per-stage callers arm a hint right before the stage call it is meant for; each setter only writes the record's slot.
extern "C" void bf_stage_prepared(int on) { g_links.get().hints.prepared = on != 0; }
extern "C" int bf_stage_chain_tail(const bf_spatial_params* prev_p, const void* prev_saved, int has_drop_mlp) {
    g_links.get().hints.tail = NextTail{prev_p && prev_saved, prev_p, prev_saved, has_drop_mlp != 0};
    return 0;
}
extern "C" int bf_stage_next_scale(const float* factors, int fdiv) { g_links.get().hints.scale = NextScale{factors, fdiv > 0 ? fdiv : 1}; return 0; }
static NextHead next_head(const D& d, int kind, const void* params, void* saved) {      // kind: 0 temporal, 1 spatial (both name norm1 and its saved outputs alike)
    auto of = [&](auto* np, const auto& sv) { return NextHead{true, np->norm1_w, np->norm1_b, sv.mean1, sv.rstd1, sv.sc1, sv.sh1, sv.xn, saved}; };
    return kind == 0 ? of((const bf_temporal_params*)params, TemporalSaved(d, saved)) : of((const bf_spatial_params*)params, SpatialSaved(d, saved));
}
extern "C" int bf_stage_chain_next(const bf_dims* dims, int next_kind, const void* next_params, void* next_saved) {
    NextHead& h = g_links.get().hints.head;
    h = NextHead{};
    if (!dims || !next_params || !next_saved) return 0;     // disarm
    BF_REQUIRE(next_kind == 0 || next_kind == 1, "bf_stage_chain_next: kind must be 0 (temporal) or 1 (spatial)");
    D d; TRY(get_dims(dims, &d));
    h = next_head(d, next_kind, next_params, next_saved);
    return 0;
}
extern "C" int bf_stage_chain_head(const bf_dims* dims, const bf_temporal_params* next_p, void* next_saved) {
    return bf_stage_chain_next(dims, 0, next_p, next_saved);
}

// ================================================================================================= temporal block
static int temporal_fwd(TrunkLinks& L, const StageHints& H, const bf_dims* dims, const bf_temporal_params* p, const void* x, void* out, void* saved,
                        void* scratch, const float* drop, bf_stream_t s) {
    D d; TRY(get_dims(dims, &d));
    BF_REQUIRE(p && x && out && saved && scratch, "bf_temporal_fwd: null pointer");
    hipStream_t st = (hipStream_t)s;
    const bool head_done = L.take_head_done(saved, st);      // the stage in front left norm1's statistics and xn behind (hints.head)
    TRY(side_join_pending(L, st));
    TemporalSaved sv(d, saved);
    Scratch sc(d, scratch);
    const void* wv[4];
    TRY(wviews(d, stage_prep(d, 0, p, sv.prep_dst(), nullptr), H.prepared, wv, st));
    const void *win_c = wv[0], *wout_c = wv[1];
    if (!head_done)
        TRY(bf_in_stats_apply(d.dtype, x, (int)d.F, (int)d.S, d.E, p->norm1_w, p->norm1_b, nullptr, 1, nullptr, sv.mean1, sv.rstd1, sv.sc1, sv.sh1, sc.in_ws,
                              nullptr, sv.xn, st));
    TRY(qkv_gemm(d, sv.xn, win_c, p->input_head_b, sv.qkv, st));
    // sequences along T for every (b, y, x): token = b*T*S + pos + t*S
    TRY(bf_attn_fwd(d.dtype, sv.qkv, sv.o, (long)d.B * d.S, d.T, d.S, (long)d.T * d.S, 1, d.S, d.heads, d.d, p->qnorm_w, p->qnorm_b,
                    p->knorm_w, p->knorm_b, p->rel_pos_emb, d.attn_scale ? p->attn_scale_factor : nullptr, 1.f, 0, st));
    TRY(bf_in_stats_apply(d.dtype, sv.o, (int)d.F, (int)d.S, d.E, p->norm2_w, p->norm2_b, nullptr, 1, nullptr, sv.mean2, sv.rstd2, sv.sc2, sv.sh2, sc.in_ws,
                          nullptr, sv.on, st));
    if (H.head.armed) {      // the stage behind opens with InstanceNorm(out): it rides in the out-projection's launch
        const NextHead& h = H.head;
        const bf_frame_norm n2{h.w, h.b, nullptr, 1, h.mean, h.rstd, h.sc, h.sh, nullptr, h.xn};
        const int rc = bf_gemm_fwd_frames(d.dtype, (int)d.N, d.E, d.E, sv.on, d.E, sv.wout_t, d.E, nullptr, sv.alpha, sv.beta, drop, d.T, x, out, (int)d.S,
                                          nullptr, &n2, s);
        if (rc < 0) return rc;
        if (rc == 0) { L.head_done = {h.saved, st}; return 0; }
    }
    TRY(outproj_gemm(d, sv.on, wout_c, sv.alpha, sv.beta, x, out, drop, (long)d.T * d.S, st));   // mask per batch element
    return 0;
}

static int temporal_bwd(TrunkLinks& L, const StageHints& H, const bf_dims* dims, const bf_temporal_params* p, const bf_temporal_params* g, const void* x,
                        const void* dout, void* dx, void* saved, void* scratch, const float* drop, bf_stream_t s) {
    D d; TRY(get_dims(dims, &d));
    BF_REQUIRE(p && g && x && dout && dx && saved && scratch, "bf_temporal_bwd: null pointer");
    hipStream_t st = (hipStream_t)s;
    TemporalSaved sv(d, saved);
    Scratch sc(d, bwd_scratch(L, d, scratch));
    const void* win_c = d.dtype == BF_DTYPE_F32 ? (const void*)p->input_head_w : sv.win_c;
    Fork fk(L, st, true, L.scratch_parity);      // weight-gradient GEMMs go to the side stream; nothing they read (dbr, t3, s1) is rewritten before the join
    if (fk.deferred) TRY(side_join_pending(L, st, fk.set));      // the stage before the previous one used this scratch set
    void* don = sc.t1;      // [N][E]
    void* dO = sc.t1b;      // [N][E]
    void* dqkv = sc.t3;     // [N][3E]
    // branch = drop[b] * (...): scale the incoming gradient once (2U pass), the rest is unchanged (making the scaled tensor on the side
    // stream instead was measured twice and lost: EXPERIMENTS.md)
    const void* dbr = dout;
    if (drop) {
        const TrunkLinks::DbrReady& r = L.dbr_ready;
        if (r.dx == dout && r.f == drop && r.buf && r.st == st) dbr = r.buf;      // the stage in front left the scaled copy behind
        else {
            TRY(bf_frame_scale(d.dtype, dout, drop, d.T, sc.t4, d.N, (int)d.S, d.E, st));
            dbr = sc.t4;
        }
    }
    L.dbr_ready = TrunkLinks::DbrReady{};
    const InFuse fu2{sv.o, nullptr, dO, sv.mean2, sv.rstd2, p->norm2_w, p->norm2_b, sc.in_ws2};      // don @ ... then norm2's backward -> dO
    TRY(outproj_bwd(d, sc, dbr, sv.on, sv.wout_s, p->output_head_w, p->output_head_b, p->norm2_b, p->gamma, nullptr, nullptr,
                    sv.alpha, sv.mc, g->output_head_w, g->output_head_b, nullptr, g->gamma, nullptr, nullptr, don, st, fk, &fu2));
    ReduceJobs jobs;        // parameter-gradient reductions, all launched together at the end
    TRY(jobs.push(InReduceJob{sc.in_ws2, (int)d.F, d.E, p->norm2_w, p->norm2_b, nullptr, 1, g->norm2_w, g->norm2_b, nullptr, nullptr, nullptr, nullptr}));
    {
        int rows = 0;
        TRY(bf_attn_bwd_partials(d.dtype, sv.qkv, dO, dqkv, (long)d.B * d.S, d.T, d.S, (long)d.T * d.S, 1, d.S, d.heads, d.d, p->qnorm_w, p->qnorm_b,
                                 p->knorm_w, p->knorm_b, p->rel_pos_emb, d.attn_scale ? p->attn_scale_factor : nullptr, g->qnorm_w, g->qnorm_b,
                                 g->knorm_w, g->knorm_b, g->rel_pos_emb, d.attn_scale ? g->attn_scale_factor : nullptr, 1.f, 0, sc.attn_ws,
                                 Scratch::ATTN_WS_FLOATS, &rows, st));
        TRY(jobs.push(AttnReduceJob{sc.attn_ws, rows, d.d, d.heads, g->qnorm_w, g->qnorm_b, g->knorm_w, g->knorm_b, g->rel_pos_emb,
                                    d.attn_scale ? g->attn_scale_factor : nullptr}));
    }
    void* dxn = sc.t1;      // don is dead
    InFuse fu1{x, dout, dx, sv.mean1, sv.rstd1, p->norm1_w, p->norm1_b, sc.in_ws};             // dqkv @ W_in, then norm1's backward + residual
    // Chained tail (hints.tail): dx is the output gradient of the spatial stage in front, whose backward opens with its MLP-branch
    // InstanceNorm -- applied here, into THAT stage's scratch set (the other one: its earlier user's side work is joined first, as the
    // spatial stage itself would at its start).
    TailNorm tn;
    bool tail_done = false;
    static const bool chain_on = bf_knob("BF_BWD_CHAIN", 1) != 0;
    if (H.tail.armed && chain_on && fk.deferred && d.dtype == BF_DTYPE_BF16 && d.S == 144 && d.F % 2 == 0) {
        const NextTail& h = H.tail;
        const int oset = L.scratch_parity ^ 1;
        TRY(side_join_pending(L, st, oset));
        Scratch so(d, (char*)scratch + (size_t)oset * Scratch(d, nullptr).bytes);
        SpatialSaved ps(d, const_cast<void*>(h.saved));
        tn = TailNorm{ps.z, so.t1, ps.mean3, ps.rstd3, h.p->mlp_norm_w, h.drop ? ps.gtab : h.p->gamma_mlp, h.drop ? 1 : (int)d.F, L.tail_ws_flip ? so.in_ws5 : so.in_ws4, &tail_done};
        L.tail_ws_flip = !L.tail_ws_flip;
        fu1.tail = &tn;
    }
    if (H.tail.armed) L.tail_done = TrunkLinks::TailDone{};
    TRY(linear_bwd(d, sc, dqkv, 3 * d.E, sv.xn, d.E, BF_PRO_NONE, nullptr, nullptr, win_c, g->input_head_w, g->input_head_b, dxn, nullptr, st, fk, &fu1, true));
    if (tail_done) L.tail_done = {H.tail.saved, dx, tn.ws, st};
    TRY(jobs.push(InReduceJob{sc.in_ws, (int)d.F, d.E, p->norm1_w, p->norm1_b, nullptr, 1, g->norm1_w, g->norm1_b, nullptr, nullptr, nullptr, nullptr}));
    TRY(launch_with_pending(L, jobs, st));      // ... with the reductions the spatial stage behind (in the forward) left pending
    return fk.join();
}
extern "C" int bf_temporal_fwd(const bf_dims* dims, const bf_temporal_params* p, const void* x, void* out, void* saved, void* scratch,
                               const float* drop, bf_stream_t s) {
    TrunkLinks& L = g_links.get();
    return temporal_fwd(L, L.take_hints(), dims, p, x, out, saved, scratch, drop, s);
}
extern "C" int bf_temporal_bwd(const bf_dims* dims, const bf_temporal_params* p, const bf_temporal_params* g, const void* x, const void* dout,
                               void* dx, void* saved, void* scratch, const float* drop, bf_stream_t s) {
    TrunkLinks& L = g_links.get();
    return temporal_bwd(L, L.take_hints(), dims, p, g, x, dout, dx, saved, scratch, drop, s);
}

// Parameter preparation of many trunk stages at once (what each stage forward otherwise launches for itself): bf16 weight copies, the
// out-projection fold and the MLP branch's stochastic-depth table, written into each stage's `saved` record.  kinds[i]: 0 temporal
// (params[i] = bf_temporal_params*), 1 spatial (bf_spatial_params*); drop_mlp[i]: the spatial stage's MLP-branch factors or NULL.
// A stage forward consumes it when bf_stage_prepared(1) was called just before.  bf16 only (returns 1 in fp32 mode: nothing to cast).
static int prep_stages(TrunkLinks& L, const bf_dims* dims, int n, const int32_t* kinds, const void* const* params, void* const* saved,
                       const float* const* drop_mlp, bf_stream_t s) {
    D d; TRY(get_dims(dims, &d));
    BF_REQUIRE(n >= 1 && kinds && params && saved, "bf_prep_stages: bad arguments");
    if (d.dtype != BF_DTYPE_BF16) return 1;
    hipStream_t st = (hipStream_t)s;
    TRY(side_join_pending(L, st));
    for (int i0 = 0; i0 < n; i0 += PREP_BATCH) {
        PrepBatch b;
        memset(&b, 0, sizeof(b));
        const int m = std::min(PREP_BATCH, n - i0);
        for (int i = 0; i < m; ++i) {
            const int k = i0 + i;
            BF_REQUIRE(params[k] && saved[k] && (kinds[k] == 0 || kinds[k] == 1), "bf_prep_stages: bad stage entry");
            b.s[i] = kinds[k] == 0 ? stage_prep(d, 0, params[k], TemporalSaved(d, saved[k]).prep_dst(), nullptr)
                                   : stage_prep(d, 1, params[k], SpatialSaved(d, saved[k]).prep_dst(), drop_mlp ? drop_mlp[k] : nullptr);
        }
        TRY(launch_stage_prep(d, b, m, 7, st));
    }
    return 0;
}
extern "C" int bf_prep_stages(const bf_dims* dims, int n, const int32_t* kinds, const void* const* params, void* const* saved,
                              const float* const* drop_mlp, bf_stream_t s) {
    return prep_stages(g_links.get(), dims, n, kinds, params, saved, drop_mlp, s);
}

// ================================================================================================= axial (spatial) block
static int spatial_fwd(TrunkLinks& L, const StageHints& H, const bf_dims* dims, const bf_spatial_params* p, const void* x, void* out, void* saved,
                       void* scratch, const float* drop_att, const float* drop_mlp, bf_stream_t s) {
    D d; TRY(get_dims(dims, &d));
    BF_REQUIRE(p && x && out && saved && scratch, "bf_spatial_fwd: null pointer");
    hipStream_t st = (hipStream_t)s;
    // the temporal stage in front left norm1's statistics and xn behind (a chained head is consumed by the stage called right after the stage that made it)
    const bool head_done = L.take_head_done(saved, st);
    TRY(side_join_pending(L, st));
    SpatialSaved sv(d, saved);
    Scratch sc(d, scratch);
    const void* wv[4];
    TRY(wviews(d, stage_prep(d, 1, p, sv.prep_dst(), drop_mlp), H.prepared, wv, st));      // (bf16: with gtab[f][c] = drop_mlp[f] * gamma_mlp[c])
    const void *win_c = wv[0], *wout_c = wv[1], *w1_c = wv[2], *w2_c = wv[3];
    if (!head_done)
        TRY(bf_in_stats_apply(d.dtype, x, (int)d.F, (int)d.S, d.E, p->norm1_w, p->norm1_b, nullptr, 1, nullptr, sv.mean1, sv.rstd1, sv.sc1, sv.sh1, sc.in_ws,
                              nullptr, sv.xn, st));
    TRY(qkv_gemm(d, sv.xn, win_c, p->input_head_b, sv.qkv, st));
    // along w (one sequence per (frame, row): contiguous tokens), then along h (per (frame, column): stride w), averaged
    {   // ... and norm2 in the same launch where the one-launch form applies
        const int rc = bf_attn_axial_norm_fwd(d.dtype, sv.qkv, sv.o, sv.on, d.F, (int)d.h, (int)d.w, d.heads, d.d, p->qnorm_w, p->qnorm_b, p->knorm_w,
                                              p->knorm_b, p->rel_pos_emb, d.attn_scale ? p->attn_scale_factor_x : nullptr,
                                              d.attn_scale ? p->attn_scale_factor_y : nullptr, p->norm2_w, p->norm2_b, sv.mean2, sv.rstd2, sv.sc2,
                                              sv.sh2, st);
        if (rc < 0) return rc;
        if (rc == 1) {
            TRY(bf_attn_axial_fwd(d.dtype, sv.qkv, sv.o, d.F, (int)d.h, (int)d.w, d.heads, d.d, p->qnorm_w, p->qnorm_b, p->knorm_w, p->knorm_b,
                                  p->rel_pos_emb, d.attn_scale ? p->attn_scale_factor_x : nullptr, d.attn_scale ? p->attn_scale_factor_y : nullptr, st));
            TRY(bf_in_stats_apply(d.dtype, sv.o, (int)d.F, (int)d.S, d.E, p->norm2_w, p->norm2_b, nullptr, 1, nullptr, sv.mean2, sv.rstd2, sv.sc2, sv.sh2,
                                  sc.in_ws, nullptr, sv.on, st));
        }
    }
    TRY(outproj_gemm(d, sv.on, wout_c, sv.alpha, sv.beta, x, sv.x1, drop_att, d.S, st));     // mask per frame
    {   // pre = x1 @ W1^T + b1 ; hid = gelu(pre) (both kept: pre for gelu', hid as the fc2 operand -- no erf in any prologue)
        bf_operand A = op_plain(sv.x1, d.E, BF_LAY_KC);
        bf_operand Bo = op_plain(w1_c, d.E, BF_LAY_KC);
        bf_epilogue e = epi_store(sv.pre, 4L * d.E);
        e.bias = p->fc1_b;
        e.gelu_out = sv.hid;
        TRY(bf_gemm(d.dtype, (int)d.N, 4 * d.E, d.E, &A, &Bo, &e, 1, st));
    }
    // out = x1 + drop_mlp[f] * gamma_mlp * InstanceNorm(z): the per-(frame, channel) factor rides in the InstanceNorm affine
    const float* g3 = p->gamma_mlp;
    int g3div = (int)d.F;
    if (drop_mlp) {
        if (d.dtype == BF_DTYPE_F32) {      // bf16: made by the stage's preparation launch above
            hipLaunchKernelGGL(frame_table_kernel, dim3(bf_cdiv(d.F * d.E, 256)), dim3(256), 0, st, drop_mlp, 1, (const float*)p->gamma_mlp, sv.gtab, (int)d.F, d.E);
            BF_CHECK_LAUNCH();
        }
        g3 = sv.gtab; g3div = 1;
    }
    if (d.dtype == BF_DTYPE_BF16) {      // z = hid @ W2^T + b2, the MLP-branch norm + residual and (armed) the next stage's opening norm in ONE launch
        const bf_frame_norm n1{p->mlp_norm_w, p->mlp_norm_b, g3, g3div, sv.mean3, sv.rstd3, sv.sc3, sv.sh3, sv.x1, out};
        const NextHead& h = H.head;
        const bf_frame_norm n2{h.w, h.b, nullptr, 1, h.mean, h.rstd, h.sc, h.sh, nullptr, h.xn};
        const int rc = bf_gemm_fwd_frames(d.dtype, (int)d.N, d.E, 4 * d.E, sv.hid, 4L * d.E, sv.w2t_c, d.E, p->fc2_b, nullptr, nullptr, nullptr, 1, nullptr, sv.z,
                                          (int)d.S, &n1, h.armed ? &n2 : nullptr, s);
        if (rc < 0) return rc;
        if (rc == 0) {
            if (h.armed) L.head_done = {h.saved, st};
            return 0;
        }
    }
    {   // z = hid @ W2^T + b2
        bf_operand A = op_plain(sv.hid, 4L * d.E, BF_LAY_KC);
        bf_operand Bo = op_plain(w2_c, 4L * d.E, BF_LAY_KC);
        bf_epilogue e = epi_store(sv.z, d.E);
        e.bias = p->fc2_b;
        TRY(bf_gemm(d.dtype, (int)d.N, d.E, 4 * d.E, &A, &Bo, &e, 1, st));
    }
    if (H.head.armed) {
        const NextHead& h = H.head;
        bool chained = false;
        TRY(bf_in_stats_apply_chain(d.dtype, sv.z, (int)d.F, (int)d.S, d.E, p->mlp_norm_w, p->mlp_norm_b, g3, g3div, nullptr, sv.mean3, sv.rstd3, sv.sc3, sv.sh3,
                                    sc.in_ws, sv.x1, out, h.w, h.b, h.mean, h.rstd, h.sc, h.sh, h.xn, &chained, st));
        if (chained) L.head_done = {h.saved, st};
        return 0;
    }
    TRY(bf_in_stats_apply(d.dtype, sv.z, (int)d.F, (int)d.S, d.E, p->mlp_norm_w, p->mlp_norm_b, g3, g3div, nullptr, sv.mean3, sv.rstd3,
                          sv.sc3, sv.sh3, sc.in_ws, sv.x1, out, st));
    return 0;
}

static int spatial_bwd(TrunkLinks& L, const StageHints& H, const bf_dims* dims, const bf_spatial_params* p, const bf_spatial_params* g, const void* x,
                       const void* dout, void* dx, void* saved, void* scratch, const float* drop_att, const float* drop_mlp, bf_stream_t s) {
    D d; TRY(get_dims(dims, &d));
    BF_REQUIRE(p && g && x && dout && dx && saved && scratch, "bf_spatial_bwd: null pointer");
    hipStream_t st = (hipStream_t)s;
    SpatialSaved sv(d, saved);
    Scratch sc(d, bwd_scratch(L, d, scratch));
    const bool f32 = d.dtype == BF_DTYPE_F32;
    const void* win_c = f32 ? (const void*)p->input_head_w : sv.win_c;
    const void* w1_c = f32 ? (const void*)p->fc1_w : sv.w1_c;
    const void* w2_c = f32 ? (const void*)p->fc2_w : sv.w2_c;
    // weight-gradient GEMMs go to the side stream and are joined at the end; every buffer they read (dz = t1, dpre = t4,
    // dx1 = t1b, dbr = e5, dqkv = t3, s1) is written once per call, so the critical path below never recycles one under them.
    TRY(flush_pending_reduce(L, st));      // (a spatial stage that no temporal stage followed: its partial sums live in the set this stage is about to use)
    Fork fk(L, st, true, L.scratch_parity);
    if (fk.deferred) TRY(side_join_pending(L, st, fk.set));      // the stage before the previous one used this scratch set
    // out = x1 + gamma_mlp * IN(z)
    void* dz = sc.t1;
    ReduceJobs jobs;        // parameter-gradient reductions, all launched together at the end
    // the temporal stage behind left dz and the partial sums in place (hints.tail) -- usable only if this call's dout IS the dx that stage
    // wrote (another consumer of the stage's output, or a gradient hook, makes autograd hand over a different, summed tensor: recompute then)
    const TrunkLinks::TailDone td = L.tail_done;
    L.tail_done = TrunkLinks::TailDone{};
    const bool tail_done = td.saved == saved && td.dx == dout && td.st == st;
    {   // with stochastic depth gtab[f][c] = drop_mlp[f] * gamma_mlp[c] was the scale: d gamma_mlp = sum_f drop_mlp[f] * (w s2 + b s1), folded in the reduction
        const float* gsc = drop_mlp ? sv.gtab : p->gamma_mlp;
        const int gdiv = drop_mlp ? 1 : (int)d.F;
        if (!tail_done)
            TRY(bf_in_bwd_partials(d.dtype, dout, sv.z, nullptr, dz, (int)d.F, (int)d.S, d.E, sv.mean3, sv.rstd3, p->mlp_norm_w, p->mlp_norm_b, gsc, gdiv, 0, sc.in_ws3, st));
        TRY(jobs.push(InReduceJob{tail_done ? td.ws : sc.in_ws3, (int)d.F, d.E, p->mlp_norm_w, p->mlp_norm_b, gsc, gdiv, g->mlp_norm_w, g->mlp_norm_b,
                                  drop_mlp ? nullptr : g->gamma_mlp, nullptr, drop_mlp, drop_mlp ? g->gamma_mlp : nullptr}));
    }
    // fc2: z = gelu(pre) @ W2^T + b2 ; dpre = (dz @ W2) * gelu'(pre)
    void* dpre = sc.t4;
    {
        bf_epilogue e; memset(&e, 0, sizeof(e));
        e.aux_mode = BF_AUX_DGELU; e.aux = sv.pre; e.ld_aux = 4L * d.E; e.out_mode = BF_OUT_STORE;
        static const bool use_t = bf_knob("BF_FC2_DGRAD_T", 1) != 0;      // K-contiguous transposed weight: the weight-stationary ring kernel's form
        TRY(linear_bwd(d, sc, dz, d.E, sv.hid, 4 * d.E, BF_PRO_NONE, nullptr, nullptr, w2_c, g->fc2_w, g->fc2_b, dpre, &e, st, fk, nullptr, false,
                       (!f32 && use_t) ? sv.w2t_c : nullptr));
    }
    // fc1: pre = x1 @ W1^T + b1 ; dx1 = dout + dpre @ W1
    void* dx1 = sc.t1b;
    bool dbr_done = false;
    {
        bf_epilogue e; memset(&e, 0, sizeof(e));
        e.aux_mode = BF_AUX_ADD; e.aux = dout; e.ld_aux = d.E; e.out_mode = BF_OUT_STORE;
        // ... and, under stochastic depth, the gradient entering the attention branch (drop_att[f] * dx1) as the kernel's second output
        TRY(linear_bwd(d, sc, dpre, 4 * d.E, sv.x1, d.E, BF_PRO_NONE, nullptr, nullptr, w1_c, g->fc1_w, g->fc1_b, dx1, &e, st, fk, nullptr, false, nullptr,
                       drop_att ? sc.e5 : nullptr, drop_att, (int)d.S, &dbr_done));
    }
    // folded out-projection
    void* don = sc.e6;
    const void* dbr = dx1;  // gradient entering the attention branch (dx1 itself continues down the residual)
    if (dbr_done) dbr = sc.e5;
    else if (drop_att) {
        TRY(bf_frame_scale(d.dtype, dx1, drop_att, 1, sc.e5, d.N, (int)d.S, d.E, st));
        dbr = sc.e5;
    }
    void* dO = sc.e7;       // [N][E]
    const InFuse fu2{sv.o, nullptr, dO, sv.mean2, sv.rstd2, p->norm2_w, p->norm2_b, sc.in_ws2};      // don @ ... then norm2's backward -> dO
    TRY(outproj_bwd(d, sc, dbr, sv.on, sv.wout_s, p->output_head_w, p->output_head_b, p->norm2_b, p->gamma_att,
                    d.feat_scale ? p->low_freq_scalar : nullptr, d.feat_scale ? p->high_freq_scalar : nullptr, sv.alpha, sv.mc,
                    g->output_head_w, g->output_head_b, g->norm2_b, g->gamma_att, d.feat_scale ? g->low_freq_scalar : nullptr,
                    d.feat_scale ? g->high_freq_scalar : nullptr, don, st, fk, &fu2));
    TRY(jobs.push(InReduceJob{sc.in_ws2, (int)d.F, d.E, p->norm2_w, p->norm2_b, nullptr, 1, g->norm2_w, g->norm2_b, nullptr, nullptr, nullptr, nullptr}));
    void* dqkv = sc.t3;
    {
        int rows = 0;
        // the two passes share their tokens' q / k LayerNorms, whose backward is linear in the incoming gradient: the W pass leaves its raw
        // gradients, the H pass adds its own and runs that backward (and the LayerNorm parameter sums) once (bf16 MFMA path)
        static const bool raw_on = bf_knob("BF_ATTN_RAW", 1) != 0;
        const bool rawm = raw_on && bf_attn_raw_modes(d.dtype, d.d);
        TRY(bf_attn_bwd_partials(d.dtype, sv.qkv, dO, dqkv, d.F * d.h, d.w, 1, d.w, 0, 1, d.heads, d.d, p->qnorm_w, p->qnorm_b, p->knorm_w, p->knorm_b,
                                 p->rel_pos_emb, d.attn_scale ? p->attn_scale_factor_x : nullptr, g->qnorm_w, g->qnorm_b, g->knorm_w, g->knorm_b,
                                 g->rel_pos_emb, d.attn_scale ? g->attn_scale_factor_x : nullptr, 0.5f, rawm ? 2 : 0, sc.attn_ws, Scratch::ATTN_WS_FLOATS, &rows, st));
        TRY(jobs.push(AttnReduceJob{sc.attn_ws, rows, d.d, d.heads, g->qnorm_w, g->qnorm_b, g->knorm_w, g->knorm_b, g->rel_pos_emb,
                                    d.attn_scale ? g->attn_scale_factor_x : nullptr}));
        TRY(bf_attn_bwd_partials(d.dtype, sv.qkv, dO, dqkv, d.F * d.w, d.h, d.w, d.S, 1, d.w, d.heads, d.d, p->qnorm_w, p->qnorm_b, p->knorm_w, p->knorm_b,
                                 p->rel_pos_emb, d.attn_scale ? p->attn_scale_factor_y : nullptr, g->qnorm_w, g->qnorm_b, g->knorm_w, g->knorm_b,
                                 g->rel_pos_emb, d.attn_scale ? g->attn_scale_factor_y : nullptr, 0.5f, rawm ? 5 : 1, sc.attn_ws2, Scratch::ATTN_WS_FLOATS, &rows, st));
        TRY(jobs.push(AttnReduceJob{sc.attn_ws2, rows, d.d, d.heads, g->qnorm_w, g->qnorm_b, g->knorm_w, g->knorm_b, g->rel_pos_emb,
                                    d.attn_scale ? g->attn_scale_factor_y : nullptr}));
    }
    void* dxn = sc.e6;      // don is dead (it was only read on this stream)
    InFuse fu1{x, dx1, dx, sv.mean1, sv.rstd1, p->norm1_w, p->norm1_b, sc.in_ws};              // dqkv @ W_in, then norm1's backward + residual
    bool scaled_done = false;
    const NextScale& ns = H.scale;
    L.dbr_ready = TrunkLinks::DbrReady{};
    static const bool scaled_on = bf_knob("BF_BWD_SCALED_COPY", 1) != 0;
    if (ns.f && scaled_on && fk.deferred && d.dtype == BF_DTYPE_BF16) {
        fu1.scaled_out = (char*)scratch + 2 * Scratch(d, nullptr).bytes + (L.dbr_flip ? dbr_bytes(d) : 0);
        fu1.scaled_f = ns.f; fu1.scaled_fdiv = ns.fdiv; fu1.scaled_done = &scaled_done;
    }
    TRY(linear_bwd(d, sc, dqkv, 3 * d.E, sv.xn, d.E, BF_PRO_NONE, nullptr, nullptr, win_c, g->input_head_w, g->input_head_b, dxn, nullptr, st, fk, &fu1, true));
    if (scaled_done) { L.dbr_ready = {dx, ns.f, fu1.scaled_out, st}; L.dbr_flip = !L.dbr_flip; }
    TRY(jobs.push(InReduceJob{sc.in_ws, (int)d.F, d.E, p->norm1_w, p->norm1_b, nullptr, 1, g->norm1_w, g->norm1_b, nullptr, nullptr, nullptr, nullptr}));
    static const bool merge_on = bf_knob("BF_REDUCE_MERGE", 1) != 0;
    if (fk.deferred && merge_on) { L.reduce.jobs = jobs; L.reduce.on = true; L.reduce.st = st; }      // rides in the next temporal stage's launch (or the next join)
    else TRY(launch_reduce_jobs(jobs, st));
    return fk.join();
}
extern "C" int bf_spatial_fwd(const bf_dims* dims, const bf_spatial_params* p, const void* x, void* out, void* saved, void* scratch,
                              const float* drop_att, const float* drop_mlp, bf_stream_t s) {
    TrunkLinks& L = g_links.get();
    return spatial_fwd(L, L.take_hints(), dims, p, x, out, saved, scratch, drop_att, drop_mlp, s);
}
extern "C" int bf_spatial_bwd(const bf_dims* dims, const bf_spatial_params* p, const bf_spatial_params* g, const void* x, const void* dout,
                              void* dx, void* saved, void* scratch, const float* drop_att, const float* drop_mlp, bf_stream_t s) {
    TrunkLinks& L = g_links.get();
    return spatial_bwd(L, L.take_hints(), dims, p, g, x, dout, dx, saved, scratch, drop_att, drop_mlp, s);
}

// ================================================================================================= the training trunk in one call per direction
// The n trunk stages of a training step (SpaceTimeBlock x 12: temporal, spatial, temporal, ...; models/axial_vit.py:58-63, 234-235) enqueued
// by ONE native call each way instead of one Python -> ctypes round trip per stage: the stage forwards / backwards above, called in a
// loop, each with the StageHints that this driver builds for it -- the whole sequence is known here, so nothing goes through the record's
// hint slots.  Everything is caller-owned: saved[i] = stage i's record (bf_temporal_saved_bytes / bf_spatial_saved_bytes), acts[i] = stage
// i's output [N][E] (the last one is the trunk's output), three [N][E] gradient buffers that rotate between consecutive backward stages
// (a stage's side-stream work may read its incoming gradient until the stage after the next one starts).
extern "C" int bf_trunk_train_fwd(const bf_dims* dims, int n, const int32_t* kinds, const void* const* params, void* const* saved,
                                  const float* const* drop_a, const float* const* drop_b, const void* x, void* const* acts, void* scratch,
                                  bf_stream_t s) {
    D d; TRY(get_dims(dims, &d));
    BF_REQUIRE(n >= 1 && kinds && params && saved && x && acts && scratch, "bf_trunk_train_fwd: bad arguments");
    for (int i = 0; i < n; ++i)
        BF_REQUIRE(params[i] && saved[i] && acts[i] && (kinds[i] == 0 || kinds[i] == 1), "bf_trunk_train_fwd: bad stage entry");
    TrunkLinks& L = g_links.get();
    (void)L.take_hints();      // (armed for a per-stage call that never came: not this pass's)
    const bool b16 = d.dtype == BF_DTYPE_BF16;
    if (b16) {
        const int rc = prep_stages(L, dims, n, kinds, params, saved, drop_b, s);
        if (rc < 0) return rc;
    }
    for (int i = 0; i < n; ++i) {
        const void* in = i ? acts[i - 1] : x;
        StageHints H;
        H.prepared = b16;
        // the next stage's opening InstanceNorm rides in this stage's last GEMM launch where the kinds alternate (bf16)
        if (b16 && i + 1 < n && kinds[i + 1] != kinds[i]) H.head = next_head(d, kinds[i + 1], params[i + 1], saved[i + 1]);
        TRY(kinds[i] == 0
            ? temporal_fwd(L, H, dims, (const bf_temporal_params*)params[i], in, acts[i], saved[i], scratch, drop_a ? drop_a[i] : nullptr, s)
            : spatial_fwd(L, H, dims, (const bf_spatial_params*)params[i], in, acts[i], saved[i], scratch, drop_a ? drop_a[i] : nullptr,
                          drop_b ? drop_b[i] : nullptr, s));
    }
    return 0;
}

// grads[i]: the gradient struct of stage i (same type as params[i]); gradients ACCUMULATE.  dout: gradient of acts[n - 1]; dx: gradient of x.
// stage_done (optional) is called on the host right after stage i's backward has been enqueued (its last weight-gradient GEMM possibly still
// deferred, see bf_side_defer): the data-parallel bucket reducer's hook.
extern "C" int bf_trunk_train_bwd(const bf_dims* dims, int n, const int32_t* kinds, const void* const* params, const void* const* grads,
                                  void* const* saved, const float* const* drop_a, const float* const* drop_b, const void* x, void* const* acts,
                                  const void* dout, void* const* gbuf3, void* dx, void* scratch, bf_stage_done_fn stage_done, void* user,
                                  bf_stream_t s) {
    D d; TRY(get_dims(dims, &d));
    BF_REQUIRE(n >= 1 && kinds && params && grads && saved && x && acts && dout && gbuf3 && dx && scratch, "bf_trunk_train_bwd: bad arguments");
    BF_REQUIRE(gbuf3[0] && gbuf3[1] && gbuf3[2], "bf_trunk_train_bwd: three gradient buffers are needed");
    TrunkLinks& L = g_links.get();
    (void)L.take_hints();      // (armed for a per-stage call that never came: not this pass's)
    const void* cur = dout;
    int rot = 0;
    for (int i = n - 1; i >= 0; --i) {
        BF_REQUIRE(params[i] && grads[i] && saved[i] && (kinds[i] == 0 || kinds[i] == 1), "bf_trunk_train_bwd: bad stage entry");
        const void* in = i ? acts[i - 1] : x;
        void* gout = i ? gbuf3[rot] : dx;
        rot = (rot + 1) % 3;
        StageHints H;
        if (kinds[i] == 0) {
            // the spatial stage in front (in the forward) opens its backward with its MLP-branch norm: applied by this stage's last kernel
            if (i > 0 && kinds[i - 1] == 1) H.tail = NextTail{true, (const bf_spatial_params*)params[i - 1], saved[i - 1], drop_b && drop_b[i - 1]};
            TRY(temporal_bwd(L, H, dims, (const bf_temporal_params*)params[i], (const bf_temporal_params*)grads[i], in, cur, gout, saved[i], scratch,
                             drop_a ? drop_a[i] : nullptr, s));
        } else {
            // the temporal stage in front scales this stage's input gradient by its stochastic-depth factors: written here as a second copy
            if (i > 0 && kinds[i - 1] == 0 && drop_a && drop_a[i - 1]) H.scale = NextScale{drop_a[i - 1], d.T};
            TRY(spatial_bwd(L, H, dims, (const bf_spatial_params*)params[i], (const bf_spatial_params*)grads[i], in, cur, gout, saved[i], scratch,
                            drop_a ? drop_a[i] : nullptr, drop_b ? drop_b[i] : nullptr, s));
        }
        if (stage_done) stage_done(i, user);
        cur = gout;
    }
    return 0;
}

