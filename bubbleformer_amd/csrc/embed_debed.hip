// Patch embed (+ FiLM) and debed (+ relative-L2 loss): each as one stream-ordered chain of the kernels in gemm/norm/patch/gather_gemm/
// embed_tail.hip, forward and backward.  They share the trunk's plumbing (model_common.h: dims, scratch, the side stream and the
// per-device record, whose state model.hip owns): a forward pass starts at the embed and a backward pass at the debed, which is where
// what an aborted pass left armed in the record is cleared.
#include "model_common.h"

using namespace bfm;

// ================================================================================================= patch embed (+ FiLM)
namespace {
inline int roundup(int v, int m) { return (v + m - 1) / m * m; }

struct EmbedSaved {
    float *gb, *dgb, *chat, *crstd;
    void* patches; int Kp;
    void* y[BF_MAX_STAGES]; void* wc[BF_MAX_STAGES];
    float *mean[BF_MAX_STAGES], *rstd[BF_MAX_STAGES], *sc[BF_MAX_STAGES], *sh[BF_MAX_STAGES];
    int C[BF_MAX_STAGES], gh[BF_MAX_STAGES], gw[BF_MAX_STAGES]; long P[BF_MAX_STAGES];
    size_t bytes;
    EmbedSaved(const D& d, void* base) {
        Arena a(base);
        const int np = d.nfluid > 0 ? d.nfluid : 1;
        gb = a.f32((size_t)2 * d.B * d.E); dgb = a.f32((size_t)2 * d.B * d.E); chat = a.f32((size_t)d.B * np); crstd = a.f32(d.B);
        Kp = roundup(4 * d.cin, 8);
        const int H = d.h * d.patch, W = d.w * d.patch;
        for (int i = 0; i < d.nst; ++i) {
            C[i] = (i == d.nst - 1) ? d.E : d.E / 4;
            gh[i] = H >> (i + 1); gw[i] = W >> (i + 1);
            P[i] = d.F * gh[i] * gw[i];
        }
        patches = a.take((size_t)P[0] * Kp * d.es);
        for (int i = 0; i < d.nst; ++i) {
            const int kin = i == 0 ? Kp : 4 * C[i - 1];
            y[i] = a.take((size_t)P[i] * C[i] * d.es);
            wc[i] = a.take((size_t)C[i] * kin * d.es);
            const size_t fc = (size_t)d.F * C[i];
            mean[i] = a.f32(fc); rstd[i] = a.f32(fc); sc[i] = a.f32(fc); sh[i] = a.f32(fc);
        }
        bytes = a.off;
    }
};
struct DebedSaved {
    float *lossbuf, *coef;
    void* y[BF_MAX_STAGES]; void* wc[BF_MAX_STAGES];
    float *mean[BF_MAX_STAGES], *rstd[BF_MAX_STAGES], *sc[BF_MAX_STAGES], *sh[BF_MAX_STAGES];
    int Cin[BF_MAX_STAGES], Co[BF_MAX_STAGES], gh[BF_MAX_STAGES], gw[BF_MAX_STAGES]; long Pin[BF_MAX_STAGES];
    int Np;
    size_t bytes;
    DebedSaved(const D& d, void* base) {
        Arena a(base);
        lossbuf = a.f32((size_t)d.F * d.cout * 2 * 2 * BF_LOSS_LIMBS); coef = a.f32((size_t)d.F * d.cout);      // [F][Co][2][limbs] int64
        Np = roundup(4 * d.cout, 8);
        for (int i = 0; i < d.nst; ++i) {
            Cin[i] = i == 0 ? d.E : d.E / 4;
            Co[i] = (i == d.nst - 1) ? d.cout : d.E / 4;
            gh[i] = d.h << i; gw[i] = d.w << i;
            Pin[i] = d.F * gh[i] * gw[i];
            const bool last = i == d.nst - 1;
            wc[i] = a.take((size_t)Cin[i] * (last ? Np : 4 * Co[i]) * d.es);
            if (!last) {
                y[i] = a.take((size_t)Pin[i] * 4 * Co[i] * d.es);
                const size_t fc = (size_t)d.F * Co[i];
                mean[i] = a.f32(fc); rstd[i] = a.f32(fc); sc[i] = a.f32(fc); sh[i] = a.f32(fc);
            } else { y[i] = nullptr; mean[i] = rstd[i] = sc[i] = sh[i] = nullptr; }
        }
        bytes = a.off;
    }
};
// A weight gradient sc.wg[M][N] = A^T B over K rows: split-K into per-slice images summed in order (no float atomics on shared addresses:
// the same bits every run); atomics only where the slab form does not apply (`slabs` false) or the workspace cannot hold the images
int wgrad_slabs_else_atomics(const D& d, const Scratch& sc, int M, int N, long K, const bf_operand& A, const bf_operand& Bo, long ld, hipStream_t ss,
                             bool slabs = true) {
    const int splitk = splitk_for(M, N, K);
    const int src = slabs ? bf_gemm_slabs(d.dtype, M, N, (int)K, &A, &Bo, sc.wg, ld, 0, splitk, (float*)sc.t1b, sc.t1b_floats, ss) : 1;
    if (src <= 0) return src;
    ZERO_ON(ss, sc.wg, (size_t)M * N * 4);
    bf_epilogue e = epi_atomic(sc.wg, ld);
    return bf_gemm(d.dtype, M, N, (int)K, &A, &Bo, &e, splitk, ss);
}
}  // namespace

extern "C" int64_t bf_embed_saved_bytes(const bf_dims* s) { D d; if (get_dims(s, &d) || d.nst < 1) return -1; return (int64_t)EmbedSaved(d, nullptr).bytes; }
extern "C" int64_t bf_debed_saved_bytes(const bf_dims* s) { D d; if (get_dims(s, &d) || d.nst < 1) return -1; return (int64_t)DebedSaved(d, nullptr).bytes; }

extern "C" int bf_embed_fwd(const bf_dims* dims, const bf_embed_params* p, const float* x, const float* fluid, void* out, void* saved,
                            void* scratch, bf_stream_t s) {
    D d; TRY(get_dims(dims, &d));
    BF_REQUIRE(p && x && out && saved && scratch && d.nst >= 1 && d.cin >= 1, "bf_embed_fwd: bad arguments");
    BF_REQUIRE((d.nfluid > 0) == (fluid != nullptr), "bf_embed_fwd: fluid parameters must be given exactly when nfluid > 0");
    hipStream_t st = (hipStream_t)s;
    TrunkLinks& L = links();
    L.clear(true);
    TRY(side_join_pending(L, st));
    EmbedSaved sv(d, saved);
    Scratch sc(d, scratch);
    const int n = d.nst, H = d.h * d.patch, W = d.w * d.patch;
    if (d.nfluid > 0)
        TRY(bf_film_net_fwd(fluid, p->film_ln_w, p->film_ln_b, p->film_w, p->film_b, sv.gb, sv.chat, sv.crstd, d.B, d.nfluid, 2 * d.E, st));
    bool stats_done = false;
    {   // every stage's convolution weight in GEMM layout / compute dtype: one launch
        int mode[BF_MAX_STAGES], R[BF_MAX_STAGES], K[BF_MAX_STAGES], Kp[BF_MAX_STAGES];
        const float* src[BF_MAX_STAGES]; void* dst[BF_MAX_STAGES];
        for (int i = 0; i < n; ++i) {
            src[i] = p->conv_w[i]; dst[i] = sv.wc[i]; mode[i] = i == 0 ? 0 : 1; R[i] = sv.C[i];
            K[i] = i == 0 ? 4 * d.cin : 4 * sv.C[i - 1]; Kp[i] = i == 0 ? sv.Kp : K[i];
        }
        TRY(bf_wprep_multi(d.dtype, n, mode, src, dst, R, K, Kp, st));
    }
    for (int i = 0; i < n; ++i) {
        const void* wc;
        if (i == 0) {
            wc = sv.wc[0];
            // patch rows and the K = 16 contraction in one streaming pass where it applies, else im2col + GEMM
            // ... which also leaves the InstanceNorm slice partials of its output (no second read of the 226 MB map for the statistics)
            const int S0 = sv.gh[0] * sv.gw[0];
            static const bool part_on = bf_knob("BF_EMBED_STATS", 1) != 0;
            const bool part_ok = part_on && n > 1 && bf_in_ws_floats(d.dtype, (int)d.F, S0, sv.C[0]) >= (int64_t)2 * d.F * sv.C[0] * (1 + (S0 + 255) / 256);      // the sliced workspace holds 256-row slices
            // lean: the stage-0 map is W0 . patch -- when every consumer of this call's saved record can rebuild its rows (the streaming
            // stage-1 kernels, the one-pass backward tail) it is not stored at all; the record's embed_lean list remembers the decision for the backward
            static const bool lean_on = bf_knob("BF_EMBED_LEAN", 1) != 0;
            // ... and only when the BACKWARD kernels that rebuild the rows will take this frame count with the workspaces this call's scratch holds
            // (the one-pass tail's partials live in the token-reduction workspace, the rebuilt-rows weight gradient's slabs in t1b: a batch of
            // 23+ clips of 16 frames at 192 x 192 exceeds the first): otherwise the map is stored and the generic chain runs, as before
            const int64_t tail_need = n > 1 ? bf_embed_tail_ws_floats((int)d.F, sv.gh[1], sv.gw[1], sv.C[0], sv.Kp) : 0;
            const bool bwd_fits = tail_need > 0 && tail_need + (int64_t)sv.C[0] * sv.Kp <= sc.tokred_floats && d.F <= 512 &&
                                  (int64_t)d.F * (4 * 96 * 96) <= sc.t1b_floats;
            const bool lean = lean_on && part_ok && bwd_fits && d.dtype == BF_DTYPE_BF16 && sv.Kp == 16 && d.cin <= 4 && sv.C[0] == 96 && sv.C[1] == 96 && (W / 2) % 16 == 0 &&
                              sv.gw[1] % 16 == 0 && ((long)sv.gh[1] * sv.gw[1]) % 128 == 0 && S0 >= 1024;
            const int rc = bf_embed_first(d.dtype, x, wc, sv.patches, lean ? nullptr : sv.y[0], (int)d.F, sv.C[0], d.cin, H / 2, W / 2, sv.Kp,
                                          part_ok ? sc.in_ws + (size_t)2 * d.F * sv.C[0] : nullptr, st);
            if (rc < 0) return rc;
            if (rc == 1 && lean) return bf_fail_msg("bf_embed_fwd: the first-stage kernel declined a shape the lean path was chosen for", __FILE__, __LINE__);
            L.embed_lean_set(saved, lean);
            stats_done = rc == 0 && part_ok;
            if (rc == 1) {
                TRY(bf_im2col_nchw(d.dtype, x, sv.patches, (int)d.F, d.cin, H, W, sv.Kp, st));
                bf_operand A = op_plain(sv.patches, sv.Kp, BF_LAY_KC);
                bf_operand Bo = op_plain(wc, sv.Kp, BF_LAY_KC);
                bf_epilogue e = epi_store(sv.y[0], sv.C[0]);
                TRY(bf_gemm(d.dtype, (int)sv.P[0], sv.C[0], sv.Kp, &A, &Bo, &e, 1, st));
            }
        } else {
            const int cp = sv.C[i - 1];
            // the 96 -> 96 channel stages stream their map once through a weight-stationary kernel (gather_gemm.hip)
            const bool reb = i == 1 && L.embed_lean_get(saved);
            const int grc = reb ? bf_gather_gemm_rebuilt(d.dtype, sv.patches, sv.wc[0], sv.wc[i], 0, sv.sc[0], sv.sh[0], sv.y[i], (int)d.F, sv.gh[i], sv.gw[i], cp, sv.C[i], st)
                                : bf_gather_gemm(d.dtype, sv.y[i - 1], sv.wc[i], 0, sv.sc[i - 1], sv.sh[i - 1], sv.y[i], (int)d.F, sv.gh[i], sv.gw[i], cp, sv.C[i], st);
            if (grc < 0) return grc;
            if (grc == 1 && reb) return bf_fail_msg("bf_embed_fwd: the rebuilt-rows stage kernel declined a shape the lean path was chosen for", __FILE__, __LINE__);
            if (grc == 1) {
                bf_operand A = op_plain(sv.y[i - 1], cp, BF_LAY_KC);
                op_gather(A, sv.gw[i], sv.gh[i], cp);
                op_affine(A, BF_PRO_AFFINE_GELU, sv.sc[i - 1], sv.sh[i - 1], (long)sv.gh[i] * sv.gw[i], cp);
                bf_operand Bo = op_plain(sv.wc[i], 4L * cp, BF_LAY_KC);
                bf_epilogue e = epi_store(sv.y[i], sv.C[i]);
                TRY(bf_gemm(d.dtype, (int)sv.P[i], sv.C[i], 4 * cp, &A, &Bo, &e, 1, st));
            }
        }
        const bool last = i == n - 1;
        const bool film = last && d.nfluid > 0;
        if (i == 0 && stats_done) {
            const int mrc = bf_in_stats_merge_slices(d.dtype, (int)d.F, sv.gh[0] * sv.gw[0], sv.C[0], 256, p->in_w[0], p->in_b[0], nullptr, 1, nullptr,
                                                     sv.mean[0], sv.rstd[0], sv.sc[0], sv.sh[0], sc.in_ws, st);
            if (mrc < 0) return mrc;
            if (mrc == 0) continue;
            if (L.embed_lean_get(saved)) return bf_fail_msg("bf_embed_fwd: slice statistics declined on the lean path", __FILE__, __LINE__);
        }
        if (last) {       // the tokens (InstanceNorm affine, FiLM folded in) leave the statistics kernel itself where a frame fits its registers
            TRY(bf_in_stats_apply(d.dtype, sv.y[i], (int)d.F, sv.gh[i] * sv.gw[i], sv.C[i], p->in_w[i], p->in_b[i], film ? sv.gb : nullptr, d.T,
                                  film ? sv.gb + (size_t)d.B * d.E : nullptr, sv.mean[i], sv.rstd[i], sv.sc[i], sv.sh[i], sc.in_ws, nullptr, out, st));
            break;
        }
        TRY(bf_in_stats(d.dtype, sv.y[i], (int)d.F, sv.gh[i] * sv.gw[i], sv.C[i], p->in_w[i], p->in_b[i], film ? sv.gb : nullptr, d.T,
                        film ? sv.gb + (size_t)d.B * d.E : nullptr, sv.mean[i], sv.rstd[i], sv.sc[i], sv.sh[i], sc.in_ws, st));
    }
    return 0;
}

extern "C" int bf_embed_bwd(const bf_dims* dims, const bf_embed_params* p, const bf_embed_params* g, const void* dout, float* dx_in,
                            void* saved, void* scratch, bf_stream_t s) {
    D d; TRY(get_dims(dims, &d));
    BF_REQUIRE(p && g && dout && saved && scratch && d.nst >= 1, "bf_embed_bwd: bad arguments");
    hipStream_t st = (hipStream_t)s;
    TrunkLinks& L = links();
    TRY(side_join_pending(L, st));
    EmbedSaved sv(d, saved);
    Scratch sc(d, scratch);
    const int n = d.nst, H = d.h * d.patch, W = d.w * d.patch;
    auto buf = [&](int stage) { return (stage & 1) ? sc.t3 : sc.t4; };
    const bool film = d.nfluid > 0;
    if (film) ZERO(sv.dgb, (size_t)2 * d.B * d.E * 4);
    // last stage: out = (xhat*w + b) * gamma_b + beta_b
    void* dy = buf(n - 1);
    TRY(bf_in_bwd(d.dtype, dout, sv.y[n - 1], nullptr, dy, (int)d.F, sv.gh[n - 1] * sv.gw[n - 1], sv.C[n - 1], sv.mean[n - 1], sv.rstd[n - 1],
                  p->in_w[n - 1], p->in_b[n - 1], film ? sv.gb : nullptr, d.T, 0, g->in_w[n - 1], g->in_b[n - 1], film ? sv.dgb : nullptr,
                  film ? sv.dgb + (size_t)d.B * d.E : nullptr, sc.in_ws, st));
    if (film)
        TRY(bf_film_net_bwd(sv.dgb, sv.chat, p->film_ln_w, p->film_ln_b, p->film_w, g->film_w, g->film_b, g->film_ln_w, g->film_ln_b, d.B,
                            d.nfluid, 2 * d.E, st));
    // Weight gradients (memset, split-K GEMM into the prepared-layout scratch, un-prepare into the gradient) run on the side
    // stream while this stream continues with the data gradient and the InstanceNorm backward of the same stage.  The side work
    // of stage i is joined before stage i-1 forks: the two ping-pong gradient buffers and sc.wg are then never recycled under it.
    Fork fk(L, st);
    hipStream_t ss;
    for (int i = n - 1; i >= 1; --i) {
        const int cp = sv.C[i - 1], K4 = 4 * cp;
        const long rpf = (long)sv.gh[i] * sv.gw[i];
        TRY(fk.join());
        TRY(fk.begin(&ss));
        // dWprep[co][k] = sum_p dy[p][co] * act(patch)[p][k]: the 96-channel stages as one stream over the map with slabs summed in a fixed
        // order (gather_gemm.hip; its slabs live in t1b, which nothing else of this call touches), else split-K with fp32 atomics
        const bool lean = L.embed_lean_get(saved);
        if (i == 1 && lean && dx_in) {      // the input wants a gradient after all: the generic chain below reads the map, so store it now (y0 = patches @ W0^T)
            bf_operand A0 = op_plain(sv.patches, sv.Kp, BF_LAY_KC);
            bf_operand B0 = op_plain(sv.wc[0], sv.Kp, BF_LAY_KC);
            bf_epilogue e0 = epi_store(sv.y[0], sv.C[0]);
            TRY(bf_gemm(d.dtype, (int)sv.P[0], sv.C[0], sv.Kp, &A0, &B0, &e0, 1, st));
            L.embed_lean_set(saved, false);
            TRY(fk.join());                 // the side stream forked before the map existed
            TRY(fk.begin(&ss));
        }
        const bool reb = i == 1 && L.embed_lean_get(saved);
        const int wrc = reb ? bf_gather_wgrad_rebuilt(d.dtype, sv.patches, sv.wc[0], dy, sv.sc[0], sv.sh[0], sc.wg, 1, (int)d.F, sv.gh[i], sv.gw[i], cp, sv.C[i],
                                                      (float*)sc.t1b, sc.t1b_floats, ss)
                            : bf_gather_wgrad(d.dtype, sv.y[i - 1], dy, sv.sc[i - 1], sv.sh[i - 1], nullptr, nullptr, sc.wg, 1, (int)d.F, sv.gh[i], sv.gw[i], cp,
                                              sv.C[i], (float*)sc.t1b, sc.t1b_floats, ss);
        if (wrc < 0) return wrc;
        if (wrc == 1 && reb) return bf_fail_msg("bf_embed_bwd: the rebuilt-rows weight gradient declined a shape the lean path was chosen for", __FILE__, __LINE__);
        if (wrc == 1) {
            bf_operand A = op_plain(dy, sv.C[i], BF_LAY_XC);
            bf_operand Bo = op_plain(sv.y[i - 1], cp, BF_LAY_XC);
            op_gather(Bo, sv.gw[i], sv.gh[i], cp);
            op_affine(Bo, BF_PRO_AFFINE_GELU, sv.sc[i - 1], sv.sh[i - 1], rpf, cp);
            TRY(wgrad_slabs_else_atomics(d, sc, sv.C[i], K4, sv.P[i], A, Bo, K4, ss));
        }
        TRY(bf_wgrad_unprep(1, sc.wg, g->conv_w[i], sv.C[i], K4, K4, 0, ss));
        if (i == 1 && !dx_in) {
            // Nothing but sums over pixels is wanted behind this stage's data gradient (GELU', the stage-0 InstanceNorm backward, the
            // stage-0 weight gradient): one pass that keeps the gradient map in registers (embed_tail.hip).  Its partials and the
            // prepared-layout gradient live in the token-reduction workspace, which no side-stream kernel of this call touches.
            static const bool tail_on = bf_knob("BF_EMBED_TAIL", 1) != 0;
            const int64_t need = bf_embed_tail_ws_floats((int)d.F, sv.gh[1], sv.gw[1], cp, sv.Kp);
            if (tail_on && need > 0 && need + (int64_t)cp * sv.Kp <= sc.tokred_floats) {
                float* dwprep = sc.tokred_ws + need;
                static const bool tail_map = bf_knob("BF_EMBED_TAIL_MAP", 0) != 0;      // 1: read the stored stage-0 map instead of rebuilding its rows
                const int trc = bf_embed_tail_bwd(d.dtype, dy, sv.wc[1], (tail_map && !L.embed_lean_get(saved)) ? sv.y[0] : nullptr, sv.patches, sv.wc[0], sv.sc[0], sv.sh[0], sv.mean[0], sv.rstd[0],
                                                  p->in_w[0], dwprep, g->in_w[0], g->in_b[0], (int)d.F, sv.gh[1], sv.gw[1], sv.C[1], cp, sv.Kp,
                                                  sc.tokred_ws, need, s);
                if (trc < 0) return trc;
                if (trc == 0) {
                    TRY(bf_wgrad_unprep(0, dwprep, g->conv_w[0], sv.C[0], 4 * d.cin, sv.Kp, 0, st));
                    return fk.join();
                }
            }
            if (L.embed_lean_get(saved)) return bf_fail_msg("bf_embed_bwd: the one-pass tail declined on the lean path (no stored stage-0 map)", __FILE__, __LINE__);
        }
        void* dact = buf(i - 1);
        {   // d(act patch)[p][k] = sum_co dy[p][co] * Wprep[co][k], scattered back to the input grid
            const int src = bf_scatter_gemm(d.dtype, dy, sv.wc[i], 1, nullptr, nullptr, dact, nullptr, (int)d.F, sv.gh[i], sv.gw[i], sv.C[i], cp, st);
            if (src < 0) return src;
            if (src == 1) {
                bf_operand A = op_plain(dy, sv.C[i], BF_LAY_KC);
                bf_operand Bo = op_plain(sv.wc[i], K4, BF_LAY_XC);
                bf_epilogue e = epi_store(dact, cp);
                epi_scatter(e, sv.gw[i], sv.gh[i], cp);
                TRY(bf_gemm(d.dtype, (int)sv.P[i], K4, sv.C[i], &A, &Bo, &e, 1, st));
            }
        }
        TRY(bf_in_bwd(d.dtype, dact, sv.y[i - 1], nullptr, dact, (int)d.F, sv.gh[i - 1] * sv.gw[i - 1], cp, sv.mean[i - 1], sv.rstd[i - 1],
                      p->in_w[i - 1], p->in_b[i - 1], nullptr, 1, 1, g->in_w[i - 1], g->in_b[i - 1], nullptr, nullptr, sc.in_ws, st));
        dy = dact;
    }
    {   // stage 0
        TRY(fk.join());
        if (dx_in) TRY(fk.begin(&ss)); else ss = st;      // nothing left to overlap with when the input needs no gradient
        // dWprep[co][k] = sum_p dy[p][co] * patch[p][k]: a 16-wide stream where it applies (the LAST kernel of the step: nothing to hide behind)
        const int nrc = sv.Kp == 16 ? bf_tokred_narrow(d.dtype, sv.C[0], sv.P[0], dy, sv.patches, sc.wg, sv.Kp, 0, 0, nullptr, nullptr, 0, sc.tokred_ws, sc.tokred_floats, ss) : 1;
        if (nrc < 0) return nrc;
        if (nrc == 1) {
            bf_operand A = op_plain(dy, sv.C[0], BF_LAY_XC);
            bf_operand Bo = op_plain(sv.patches, sv.Kp, BF_LAY_XC);
            TRY(wgrad_slabs_else_atomics(d, sc, sv.C[0], sv.Kp, sv.P[0], A, Bo, sv.Kp, ss));
        }
        TRY(bf_wgrad_unprep(0, sc.wg, g->conv_w[0], sv.C[0], 4 * d.cin, sv.Kp, 0, ss));
        if (dx_in) {
            void* dpatch = sc.t1;
            bf_operand A2 = op_plain(dy, sv.C[0], BF_LAY_KC);
            bf_operand B2 = op_plain(sv.wc[0], sv.Kp, BF_LAY_XC);
            bf_epilogue e2 = epi_store(dpatch, sv.Kp);
            TRY(bf_gemm(d.dtype, (int)sv.P[0], sv.Kp, sv.C[0], &A2, &B2, &e2, 1, st));
            TRY(bf_col2im_nchw(d.dtype, dpatch, dx_in, (int)d.F, d.cin, H, W, sv.Kp, st));
        }
    }
    return fk.join();
}

// ================================================================================================= debed (+ relative-L2 loss)
extern "C" int bf_debed_fwd(const bf_dims* dims, const bf_debed_params* p, const void* x, float* pred, const float* target, float* loss,
                            void* saved, void* scratch, bf_stream_t s) {
    D d; TRY(get_dims(dims, &d));
    BF_REQUIRE(p && x && pred && saved && scratch && d.nst >= 1 && d.cout >= 1, "bf_debed_fwd: bad arguments");
    BF_REQUIRE(!target || loss, "bf_debed_fwd: loss output missing");
    hipStream_t st = (hipStream_t)s;
    TrunkLinks& L = links();
    TRY(side_join_pending(L, st));
    DebedSaved sv(d, saved);
    Scratch sc(d, scratch);
    const int n = d.nst;
    {   // every stage's transposed-convolution weight in GEMM layout / compute dtype: one launch
        int mode[BF_MAX_STAGES], R[BF_MAX_STAGES], K[BF_MAX_STAGES], Kp[BF_MAX_STAGES];
        const float* src[BF_MAX_STAGES]; void* dst[BF_MAX_STAGES];
        for (int i = 0; i < n; ++i) {
            const bool last = i == n - 1;
            src[i] = p->conv_w[i]; dst[i] = sv.wc[i]; mode[i] = last ? 0 : 2;
            R[i] = last ? sv.Cin[i] : 4 * sv.Co[i]; K[i] = last ? 4 * sv.Co[i] : sv.Cin[i]; Kp[i] = last ? sv.Np : sv.Cin[i];
        }
        TRY(bf_wprep_multi(d.dtype, n, mode, src, dst, R, K, Kp, st));
    }
    for (int i = 0; i < n; ++i) {
        const bool last = i == n - 1;
        const int cin = sv.Cin[i], co = sv.Co[i];
        bf_operand A = op_plain(i == 0 ? x : sv.y[i - 1], cin, BF_LAY_KC);
        if (i > 0) op_affine(A, BF_PRO_AFFINE_GELU, sv.sc[i - 1], sv.sh[i - 1], (long)sv.gh[i] * sv.gw[i], cin);
        if (!last) {
            // the 96 -> 4 x 96 channel stages: one streaming kernel that also leaves the InstanceNorm slice partials of the map it writes
            // (gather_gemm.hip); the statistics then need no second pass over the map
            const int S4 = 4 * sv.gh[i] * sv.gw[i];
            const bool part_ok = i > 0 && S4 % 128 == 0 &&
                                 bf_in_ws_floats(d.dtype, (int)d.F, S4, co) >= (int64_t)2 * d.F * co * (1 + S4 / 128);
            const int src = i > 0 ? bf_scatter_gemm(d.dtype, sv.y[i - 1], sv.wc[i], 0, sv.sc[i - 1], sv.sh[i - 1], sv.y[i],
                                                    part_ok ? sc.in_ws + (size_t)2 * d.F * co : nullptr, (int)d.F, sv.gh[i], sv.gw[i], cin, co, st) : 1;
            if (src < 0) return src;
            if (src == 0 && part_ok) {
                const int mrc = bf_in_stats_merge_slices(d.dtype, (int)d.F, S4, co, 128, p->in_w[i], p->in_b[i], nullptr, 1, nullptr, sv.mean[i], sv.rstd[i],
                                                         sv.sc[i], sv.sh[i], sc.in_ws, st);
                if (mrc < 0) return mrc;
                if (mrc == 0) continue;
            }
            if (src == 1) {
                bf_operand Bo = op_plain(sv.wc[i], cin, BF_LAY_KC);
                bf_epilogue e = epi_store(sv.y[i], co);
                epi_scatter(e, sv.gw[i], sv.gh[i], co);
                TRY(bf_gemm(d.dtype, (int)sv.Pin[i], 4 * co, cin, &A, &Bo, &e, 1, st));
            }
            TRY(bf_in_stats(d.dtype, sv.y[i], (int)d.F, S4, co, p->in_w[i], p->in_b[i], nullptr, 1, nullptr, sv.mean[i],
                            sv.rstd[i], sv.sc[i], sv.sh[i], sc.in_ws, st));
        } else {
            if (target) ZERO(sv.lossbuf, (size_t)d.F * d.cout * 2 * BF_LOSS_LIMBS * 8);
            // InstanceNorm affine + GELU + the 2x2 transposed convolution + NCHW store + loss partials in one streaming pass where it applies
            const int rc = i > 0 ? bf_debed_last(d.dtype, sv.y[i - 1], sv.sc[i - 1], sv.sh[i - 1], sv.wc[i], pred, target, sv.lossbuf, (int)d.F, cin, co,
                                                 sv.gh[i], sv.gw[i], sv.Np, st) : 1;
            if (rc < 0) return rc;
            if (rc == 1) {
                bf_operand Bo = op_plain(sv.wc[i], sv.Np, BF_LAY_XC);
                float* pm = (float*)sc.t4;
                bf_epilogue e = epi_store(pm, sv.Np);
                e.out_mode = BF_OUT_STORE_F32;
                TRY(bf_gemm(d.dtype, (int)sv.Pin[i], sv.Np, cin, &A, &Bo, &e, 1, st));
                TRY(bf_pm2nchw(pm, pred, target, sv.lossbuf, (int)d.F, co, sv.gh[i], sv.gw[i], sv.Np, st));
            }
            if (target) TRY(bf_lploss_finalize(sv.lossbuf, (int)d.F, co, loss, sv.coef, st));
        }
    }
    return 0;
}

extern "C" int bf_debed_bwd(const bf_dims* dims, const bf_debed_params* p, const bf_debed_params* g, const void* x, const float* dpred,
                            const float* pred, const float* target, const float* loss_scale, void* dx, void* saved, void* scratch,
                            bf_stream_t s) {
    D d; TRY(get_dims(dims, &d));
    BF_REQUIRE(p && g && x && dx && saved && scratch && d.nst >= 1, "bf_debed_bwd: bad arguments");
    BF_REQUIRE(dpred || (pred && target), "bf_debed_bwd: need dpred or (pred, target) of the fused loss");
    BF_REQUIRE(!pred == !target, "bf_debed_bwd: pred and target of the fused loss come together");
    // dpred AND (pred, target): both go through to the last stage's kernels, which add the two in registers (an unrolled training step:
    // the gradient that came back through the fed-back prediction, plus this pass's own loss term)
    hipStream_t st = (hipStream_t)s;
    TrunkLinks& L = links();
    L.clear(false);
    TRY(side_join_pending(L, st));
    DebedSaved sv(d, saved);
    Scratch sc(d, scratch);
    const int n = d.nst;
    auto buf = [&](int stage) { return (stage & 1) ? sc.t3 : sc.t4; };   // gradient w.r.t. the INPUT of `stage`
    void* dy = nullptr;   // gradient w.r.t. the raw output of stage i-1 == (after IN/GELU backward) input of stage i
    Fork fk(L, st);          // weight gradients on the side stream, joined before the next stage forks (see bf_embed_bwd)
    hipStream_t ss;
    for (int i = n - 1; i >= 0; --i) {
        const bool last = i == n - 1;
        const int cin = sv.Cin[i], co = sv.Co[i];
        const long rpf = (long)sv.gh[i] * sv.gw[i];
        const void* ain = i == 0 ? x : sv.y[i - 1];
        void* dact = i == 0 ? dx : buf(i);
        bool normed = false;          // dact already holds the gradient of the raw map in front of stage i-1's InstanceNorm
        if (last) {
            void* dpm = sc.t1;
            // ... together with the InstanceNorm + GELU backward of the stage in front where that applies: the full-resolution gradient map
            // has rank 16 and is never stored (patch.hip, debed_last_inbwd_kernel)
            if (i > 0) {
                const int nrc = bf_debed_last_bwd_norm(d.dtype, dpred, pred, target, sv.coef, loss_scale, sv.wc[i], dpm, ain, sv.mean[i - 1], sv.rstd[i - 1],
                                                       p->in_w[i - 1], p->in_b[i - 1], dact, g->in_w[i - 1], g->in_b[i - 1], (int)d.F, cin, co, sv.gh[i],
                                                       sv.gw[i], sv.Np, sc.in_ws, bf_in_ws_floats(d.dtype, (int)d.F, (int)rpf, cin), st);
                if (nrc < 0) return nrc;
                normed = nrc == 0;
            }
            // the loss gradient in patch-major rows and the data gradient of the transposed convolution in one pass where it applies
            const int rc = normed ? 0 : bf_debed_last_bwd(d.dtype, dpred, pred, target, sv.coef, loss_scale, sv.wc[i], dpm, dact, (int)d.F, cin, co, sv.gh[i], sv.gw[i], sv.Np, st);
            if (rc < 0) return rc;
            if (rc == 1) TRY(bf_nchw2pm(d.dtype, dpred, pred, target, sv.coef, loss_scale, dpm, (int)d.F, co, sv.gh[i], sv.gw[i], sv.Np, st));
            TRY(fk.begin(&ss));
            // wg[n][ci] = sum_p dpm[p][n] * act[p][ci]: the 16-wide stream (transposed output, InstanceNorm + GELU applied to the map's
            // fragments in registers) where it applies
            const int nrc = (sv.Np == 16 && i > 0) ? bf_tokred_narrow(d.dtype, cin, sv.Pin[i], ain, dpm, sc.wg, cin, 0, 1, sv.sc[i - 1], sv.sh[i - 1], rpf,
                                                                      sc.tokred_ws, sc.tokred_floats, ss) : 1;
            if (nrc < 0) return nrc;
            if (nrc == 1) {
                bf_operand A = op_plain(dpm, sv.Np, BF_LAY_XC);
                bf_operand Bo = op_plain(ain, cin, BF_LAY_XC);
                if (i > 0) op_affine(Bo, BF_PRO_AFFINE_GELU, sv.sc[i - 1], sv.sh[i - 1], rpf, cin);
                TRY(wgrad_slabs_else_atomics(d, sc, sv.Np, cin, sv.Pin[i], A, Bo, cin, ss, cin % 4 == 0));      // (the slab form wants whole 16-byte rows)
            }
            TRY(bf_wgrad_unprep(0, sc.wg, g->conv_w[i], cin, 4 * co, sv.Np, 1, ss));
            if (rc == 1) {   // dact[p][ci] = sum_n dpm[p][n] * wt[ci][n]
                bf_operand A = op_plain(dpm, sv.Np, BF_LAY_KC);
                bf_operand Bo = op_plain(sv.wc[i], sv.Np, BF_LAY_KC);
                bf_epilogue e = epi_store(dact, cin);
                TRY(bf_gemm(d.dtype, (int)sv.Pin[i], cin, sv.Np, &A, &Bo, &e, 1, st));
            }
        } else {
            const int N4 = 4 * co;
            TRY(fk.join());
            TRY(fk.begin(&ss));
            // wg[(q,co)][ci] = sum_p dy_gathered[p][(q,co)] * act[p][ci]: as in bf_embed_bwd, the transformed side here being the coarse rows
            const int wrc = i > 0 ? bf_gather_wgrad(d.dtype, dy, ain, nullptr, nullptr, sv.sc[i - 1], sv.sh[i - 1], sc.wg, 0, (int)d.F, sv.gh[i], sv.gw[i], co,
                                                    cin, (float*)sc.t1b, sc.t1b_floats, ss) : 1;
            if (wrc < 0) return wrc;
            if (wrc == 1) {
                bf_operand A = op_plain(dy, co, BF_LAY_XC);
                op_gather(A, sv.gw[i], sv.gh[i], co);
                bf_operand Bo = op_plain(ain, cin, BF_LAY_XC);
                if (i > 0) op_affine(Bo, BF_PRO_AFFINE_GELU, sv.sc[i - 1], sv.sh[i - 1], rpf, cin);
                TRY(wgrad_slabs_else_atomics(d, sc, N4, cin, sv.Pin[i], A, Bo, cin, ss));
            }
            TRY(bf_wgrad_unprep(2, sc.wg, g->conv_w[i], N4, cin, cin, 0, ss));
            {
                const int grc = bf_gather_gemm(d.dtype, dy, sv.wc[i], 1, nullptr, nullptr, dact, (int)d.F, sv.gh[i], sv.gw[i], co, cin, st);
                if (grc < 0) return grc;
                if (grc == 1) {
                    bf_operand A = op_plain(dy, co, BF_LAY_KC);
                    op_gather(A, sv.gw[i], sv.gh[i], co);
                    bf_operand Bo = op_plain(sv.wc[i], cin, BF_LAY_XC);
                    bf_epilogue e = epi_store(dact, cin);
                    TRY(bf_gemm(d.dtype, (int)sv.Pin[i], cin, N4, &A, &Bo, &e, 1, st));
                }
            }
        }
        if (i > 0) {
            if (!normed)
                TRY(bf_in_bwd(d.dtype, dact, sv.y[i - 1], nullptr, dact, (int)d.F, (int)rpf, cin, sv.mean[i - 1], sv.rstd[i - 1], p->in_w[i - 1],
                              p->in_b[i - 1], nullptr, 1, 1, g->in_w[i - 1], g->in_b[i - 1], nullptr, nullptr, sc.in_ws, st));
            dy = dact;
        }
    }
    return fk.join();
}
