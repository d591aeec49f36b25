/*
 * bubbleformer_hip.h -- C ABI of libbubbleformer_hip.so (gfx950 / MI355X).
 *
 * The reference (HPCForge/Bubbleformer) has no FFI: its hot path is a Python
 * nn.Module tree that dispatches stock ATen ops.  This header is the boundary a
 * native replacement binds instead: plain device pointers, sizes and a HIP
 * stream -- no torch types.  Every entry point is stream-ordered, performs no
 * allocation and no device-wide synchronisation (hipGraph-capturable), and
 * returns 0 on success or a negative code (bf_last_error() gives the text).
 *
 * Tensors.  Activations are token-major / channels-last: [N, C] with
 * N = ((b*T + t)*h + y)*w + x.  `dtype` selects the activation storage type
 * (BF_DTYPE_F32 = exact-fp32 parity mode on f32 MFMA; BF_DTYPE_BF16 = bf16
 * storage + bf16 MFMA, fp32 accumulate and fp32 statistics).  Parameters and
 * parameter gradients are always fp32 in the reference's state_dict layout.
 *
 * Reference interface each group of entry points replaces (file:line relative to
 * the reference repository root):
 *   bf_gemm .................. nn.Conv2d 1x1 / nn.Linear / k2s2 (transposed) conv GEMMs:
 *                              layers/attention.py:78,121,210,299; linear_layers.py:25;
 *                              layers/patching.py:36-44,92-100 (stages with C >= 8)
 *   bf_in_stats / bf_in_bwd .. nn.InstanceNorm2d(affine): layers/attention.py:77,120,208,298,316
 *   bf_frame_linear / bf_trunk_eval_*  the same layers' forward in eval mode, whole-frame tiles (scripts/inference.py:239-252)
 *   bf_gemm_tokred ........... weight gradients of the same layers (autograd); bf_gemm_inbwd_frames: their data gradient + InstanceNorm backward
 *   bf_attn_fwd / bf_attn_bwd  AttentionBlock.forward attention core: layers/attention.py:80-119 (and each axial pass)
 *   bf_attn_axial_fwd / bf_attn_axial_norm_fwd  AxialAttentionBlock.forward attention core: layers/attention.py:212-297
 *   bf_embed_first_* ......... HMLPEmbed stage 0 (Conv2d k2s2 on NCHW input): layers/patching.py:36-44
 *   bf_debed_last_* .......... HMLPDebed last stage + LpLoss: layers/patching.py:92-100, utils/losses.py:67-94
 *   bf_film_* ................ FiLMMLP.forward: layers/linear_layers.py:63-77
 *   bf_adamw ................. torch.optim.AdamW as configured at bubbleformer/modules.py:135-136
 *   bf_adam .................. torch.optim.Adam as configured at bubbleformer/modules.py:137-138 (config/optim_cfg/adam.yaml)
 *   bf_clip_gather ........... BubbleForecast.__getitem__ + DataLoader collate for a batch of clips: bubbleformer/data/dataset.py:120-182
 *   bf_clip_gather_augment ... the unrolled batch gather with a seeded mirror in x and a seeded window per sample (no reference program)
 *   bf_clip_noise ............ seeded Gaussian input noise of a training step (no reference program; Philox4x32-10 + Box-Muller)
 *   bf_eikonal_sum / bf_heatflux_rows .. eikonal_loss utils/losses.py:5-15, heatflux utils/heatflux.py:3-38
 *   bf_lp_rows_* / bf_eikonal_bwd .. LpLoss.forward for any d / p (and its autograd) utils/losses.py:67-94; autograd of eikonal_loss utils/losses.py:5-15
 *   bf_wlp_* ................. the interface-weighted criterion: a hat weight around the target's zero level set, field weights, Eikonal penalty (no reference program)
 *   bf_slp_* ................. the shell-weighted spectral criterion: one weight per radial shell and field on |FFT|^2, field weights (no reference program)
 *   bf_rollout_score ......... the evaluation loop's scores of one step: scripts/inference.py:230-266, utils/plot_utils.py:30-33
 *   bf_rollout_heatflux ...... heatflux utils/heatflux.py:3-38 per step of that loop; bf_kde_kl: examples/data_visualization.ipynb cell 4
 *   bf_bubble_census ......... connected components of the vapour mask per frame (no reference program); bf_rollout_bubbles: per step of that loop
 *   bf_redistance ............ first-order redistancing of a signed-distance field (no reference program); bf_rollout_redistance: per step, in place
 *   bf_bubble_links .......... bubbles followed from frame to frame, bf_bubble_track_ids (no reference program); bf_rollout_bubble_links: per step
 *   bf_bubble_match .......... predicted bubbles matched to simulated ones (no reference program); bf_rollout_bubble_match: per step
 *   bf_field_errors .......... pointwise, interface and shell-spectrum error rows per frame (no reference program); bf_rollout_errors: per step
 *   bf_ensemble_scores ....... ensemble-mean RMSE, spread, CRPS and rank histogram across members (no reference program); bf_rollout_ensemble: per step
 *   bf_flow_consistency ...... divergence, kinetic energy, enstrophy and the level-set transport residual of (sdf, velocity) (no reference program); bf_rollout_flow: per step
 *   bf_render_ranges / bf_render_tiles .. plot_bubbleml and the wandb_*_plotter strips: utils/plot_utils.py:12-228 (no matplotlib, no cv2)
 *   bf_lion .................. lion_pytorch.Lion (the reference's default optimizer) at bubbleformer/modules.py:139-140
 *   bf_grad_norm, bf_opt_step's coef_dev / clip_value .. Trainer(gradient_clip_val, gradient_clip_algorithm): scripts/train.py:158-172 (torch.nn.utils.clip_grad_norm_ / clip_grad_value_)
 */
#ifndef BUBBLEFORMER_HIP_H
#define BUBBLEFORMER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* bf_stream_t; /* hipStream_t */

enum { BF_DTYPE_F32 = 0, BF_DTYPE_BF16 = 1 };

/* operand memory layouts for bf_gemm */
enum { BF_LAY_KC = 0, /* [outer][k]   : reduction index contiguous      */
       BF_LAY_XC = 1  /* [k][outer]   : outer index contiguous          */ };
/* prologues applied to an operand element while it is staged (fp32 math) */
enum { BF_PRO_NONE = 0, BF_PRO_AFFINE = 1, BF_PRO_AFFINE_GELU = 2, BF_PRO_GELU = 3 };
/* what the epilogue combines with the accumulator */
enum { BF_AUX_NONE = 0, BF_AUX_ADD = 1 /* += aux[m][n] */, BF_AUX_DGELU = 2 /* *= gelu'(aux[m][n]) */ };
enum { BF_OUT_STORE = 0 /* store activation dtype */, BF_OUT_ATOMIC_F32 = 2 /* atomicAdd into fp32 */,
       BF_OUT_STORE_F32 = 1 /* store fp32 */ };

/* One GEMM operand.  Memory "rows" are tokens (or weight rows); "columns" are
 * channels.  address(row, col) = rowbase(row) + (col / seglen) * segstride + col % seglen,
 * rowbase(row) = row * ld, or, when gw > 0, the top-left pixel of a 2x2 patch:
 * row = (f*gh + y)*gw + x  ->  ((f*2*gh + 2*y) * 2*gw + 2*x) * gc   (k2s2 patch gather / scatter). */
typedef struct bf_operand {
    const void* p;          /* activation dtype (weights: dtype of the GEMM) */
    int64_t ld;
    int32_t layout;         /* BF_LAY_* */
    int32_t seglen;         /* 0 = no segmentation */
    int64_t segstride;
    int32_t gw, gh, gc;     /* 0 = plain rows */
    int32_t pro;            /* BF_PRO_* */
    const float* sc;        /* [frames][nch] scale  (AFFINE*) */
    const float* sh;        /* [frames][nch] shift (NULL = 0) */
    int32_t rows_per_frame; /* frame = row / rows_per_frame   */
    int32_t nch;            /* channel = col % nch            */
} bf_operand;

typedef struct bf_epilogue {
    const float* bias;      /* [N] or NULL: v += bias[n]                    */
    const float* colscale;  /* [N] or NULL: v  = v * colscale[n] + colshift[n] */
    const float* colshift;  /* [N] or NULL                                   */
    int32_t aux_mode;       /* BF_AUX_* */
    const void* aux;        /* activation dtype, [M][ld_aux] */
    int64_t ld_aux;
    int32_t out_mode;       /* BF_OUT_* */
    void* c;                /* output */
    int64_t ldc;
    int32_t seglen;         /* output scatter (same addressing as bf_operand) */
    int64_t segstride;
    int32_t gw, gh, gc;
    void* gelu_out;         /* optional second output (activation dtype, same addressing as c): gelu(value stored to c) */
    float* colsum;          /* token-reduction form only (A outer-contiguous): colsum[m] += sum_k A[k][m] (bias gradient) */
    const float* rowscale;  /* optional per-row-group factor applied to the value before aux / store (stochastic depth) */
    int32_t rows_per_group; /* group = row / rows_per_group */
} bf_epilogue;

/* C[M,N] (+)= epi( sum_k pro(A)[m,k] * pro(B)[n,k] ).  splitk > 1 requires BF_OUT_ATOMIC_F32. */
int bf_gemm(int dtype, int M, int N, int K, const bf_operand* A, const bf_operand* B, const bf_epilogue* E,
            int splitk, bf_stream_t stream);

/* Data-gradient GEMM fused with the InstanceNorm backward that consumes it (whole-frame row tiles, gemm_frame.hip):
 *   dy = A[M][K] @ B[K][N] (both row-major), frames of S consecutive rows; per (frame, column):
 *   out = rstd*w*(dy - s1/S - xhat*s2/S) [+ add],  s1 = sum dy, s2 = sum dy*xhat, xhat = (x - mean)*rstd;  ws[(f*N+n)*2..] = {s1, s2}.
 * Replaces the conv1x1 backward + InstanceNorm2d backward pair of layers/attention.py:77-78,120-121,208-210,298-299 (autograd).
 * Returns 0 when done, 1 when the shape is not covered (bf16, S = 144, M % 144 = N % 128 = K % 64 = 0): the caller then runs
 * bf_gemm + bf_in_bwd; < 0 on error. */
int bf_gemm_inbwd_frames(int dtype, int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb, const void* x,
                         const void* add, void* out, int S, const float* mean, const float* rstd, const float* w, float* ws,
                         const float* fscale /* optional: dy of frame f is multiplied by fscale[f / fdiv] (stochastic depth) */, int fdiv,
                         bf_stream_t stream);
/* ... and the backward of a SECOND InstanceNorm applied to `out` in the same launch: the norm whose output gradient `out` is (in the model: the
 * MLP-branch norm of the spatial stage in front of a temporal stage, autograd of layers/attention.py:305-317 behind :77-78).  cz: that norm's
 * input rows, cmean / crstd its statistics [frames][N], cw its weight, cg an optional post scale [frames / cgdiv][N] (layer scale, or the
 * stochastic-depth table).  cdz = crstd cw cg (out - (s1 + xh s2) / S), xh = (cz - cmean) crstd; partials {s1, s2} to cws (ws layout; cws may
 * be null: the sums are then not kept).  cz / cdz are [M][N] with row stride N (the x / out stride).
 * Returns 1 (nothing launched) where the two-frames-per-tile kernel does not apply (S != 144, odd frame counts, fp32). */
int bf_gemm_inbwd_frames_chain(int dtype, int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb, const void* x,
                               const void* add, void* out, int S, const float* mean, const float* rstd, const float* w, float* ws,
                               const float* fscale, int fdiv, const void* cz, void* cdz, const float* cmean, const float* crstd,
                               const float* cw, const float* cg, int cgdiv, float* cws, bf_stream_t stream);

/* The forward twin: out[M][N] = lin(A[M][K] @ Bt[K][N]) [+ add], lin(v) = ((v + bias) * colscale + colshift) * fscale[frame / fdiv], frames of
 * S = 144 consecutive rows, followed IN THE SAME LAUNCH by up to two InstanceNorm2d over the frame (layers/attention.py:77,208 norm1;
 * 312-317 the MLP-branch norm + layer scale + residual): n1 (optional): y = resid + g * IN(out), written to n1->out; n2 (optional): the NEXT
 * stage's opening norm of the last tensor written, n2->out = IN(.) * w + b (no g, no resid).  Each leaves mean / rstd / sc / sh [frames][N]
 * as bf_in_stats does.  Bt is the weight TRANSPOSED ([in][out], N contiguous).  Replaces bf_gemm + bf_in_stats (+ bf_affine_apply) -- one
 * read of the activation and one launch per norm less -- with identical bits.  Returns 0 when done, 1 when the shape is not covered
 * (bf16, S = 144, M % 288 = N % 128 = K % 64 = 0, K >= 128, 16-byte aligned operands, fscale only together with colscale / colshift),
 * < 0 on error. */
typedef struct bf_frame_norm {
    const float *w, *b;             /* affine [N] */
    const float* g; int32_t gdiv;   /* optional post scale [frames / gdiv][N] */
    float *mean, *rstd, *sc, *sh;   /* [frames][N] */
    const void* resid;              /* optional [M][N] */
    void* out;                      /* [M][N] */
} bf_frame_norm;
int bf_gemm_fwd_frames(int dtype, int M, int N, int K, const void* A, int64_t lda, const void* Bt, int64_t ldb, const float* bias,
                       const float* colscale, const float* colshift, const float* fscale, int fdiv, const void* add, void* out, int S,
                       const bf_frame_norm* n1, const bf_frame_norm* n2, bf_stream_t stream);

/* Token-reduction GEMM (weight gradient of a 1x1 conv / Linear: autograd of layers/attention.py:78,121,210,299, linear_layers.py:18-25):
 *   out[Nout][Kin] = (accumulate ? out : 0) + sum_tok dy[tok][Nout] * x[tok][Kin],  colsum[Nout] likewise + sum_tok dy[tok][:]  (optional)
 * dy [M][ldy], x [M][ldx] token-major bf16.  Few long token slices, one 128 x 128 tile x slice per workgroup, partial tiles to fp32
 * slabs in `ws` (bf_gemm_tokred_ws_floats), summed in slice order by a second launch: bit-reproducible, no float atomics.
 * Returns 0 when done, 1 when the shape is not covered (bf16, Nout % 128 = Kin % 128 = M % 64 = 0): the caller then uses bf_gemm's
 * outer-contiguous form; < 0 on error. */
int bf_gemm_tokred(int dtype, int Nout, int Kin, int64_t M, const void* dy, int64_t ldy, const void* x, int64_t ldx, float* out,
                   int accumulate, float* colsum, float* ws, int64_t ws_floats, bf_stream_t stream);
int64_t bf_gemm_tokred_ws_floats(int Nout, int Kin, int64_t M);

/* Whole-frame forward projection for inference (frame_fwd.hip): out[f*S + s][:] = epi( IN(A)[f*S + s][:K] @ W[:N][:K]^T ), one workgroup
 * per (frame of S = 144 tokens, block of output columns).  Replaces, in ONE launch each, the pairs the reference runs as separate modules:
 *   norm_w/norm_b != NULL: nn.InstanceNorm2d(affine) in front of the 1x1 conv (layers/attention.py:77-78 / 208-210 norm1 + input_head,
 *     120-121 norm2 + output_head); K = 384 only (the frame's operand is LDS-resident);
 *   en_w/en_b/en_g != NULL: the InstanceNorm behind fc2 with layer scale and residual, out = resid + en_g * IN(A @ W^T + bias)
 *     (layers/attention.py:316-322);
 *   otherwise v = acc + bias; v = v * colscale + colshift (if given); v += resid (if given); v = gelu(v) (if gelu);
 *   out_n != NULL: a second output, the NEXT layer's InstanceNorm of `out` (its norm1: out_n = IN(out) * next_w + next_b, statistics
 *     over the stored bf16 values) -- the tile holds whole-frame columns of `out`, so the next projection needs no norm in front.
 * A [frames*S][lda], W [N][ldw] (K-contiguous), resid / out [frames*S][ld*], all bf16.  Statistics are summed in bf_in_stats' order and
 * the products in bf_gemm's: results equal the separate launches bit for bit.  Returns 0 when done, 1 when the shape is not covered
 * (bf16, S = 144, N % 32 = 0, K = 384 or (no norm in front) K % 64 = 0), < 0 on error. */
int bf_frame_linear(int dtype, int frames, int S, int K, int N, const void* A, int64_t lda, const void* W, int64_t ldw,
                    const float* norm_w, const float* norm_b, const float* bias, const float* colscale, const float* colshift,
                    const void* resid, int64_t ldr, int gelu, const float* en_w, const float* en_b, const float* en_g,
                    void* out, int64_t ldo,
                    const float* next_w, const float* next_b, void* out_n, int64_t ldn, /* optional second output, see above */
                    bf_stream_t stream);

/* ---------------------------------------------------------------- kernel-level entry points (unit-testable) */

/* InstanceNorm statistics over the S tokens of each frame, per channel (two-pass, fp32):
 * mean/rstd [frames][C]; sc = rstd*w (*g), sh = (b - mean*rstd*w) (*g + gb): the affine the consumer GEMM applies.
 * g/gb (optional): [frames/gdiv][C] post scale / shift (FiLM gamma/beta per batch element, or a layer scale). */
int bf_in_stats(int dtype, const void* x, int frames, int S, int C, const float* w, const float* b, const float* g, int gdiv,
                const float* gb, float* mean, float* rstd, float* sc, float* sh,
                float* ws /* optional, bf_in_ws_floats(): long frames are reduced in slices (frames x slices workgroups) */,
                bf_stream_t stream);
/* floats of workspace bf_in_stats / bf_in_bwd want for this problem (2*frames*C, plus slice partials for long frames) */
int64_t bf_in_ws_floats(int dtype, int frames, int S, int C);
/* out = [resid +] z * sc[f,c] + sh[f,c]   (sh may be NULL = 0) */
int bf_affine_apply(int dtype, const void* z, const void* resid, const float* sc, const float* sh, void* out, int64_t nrows,
                    int S, int C, bf_stream_t stream);
/* backward of y = act(xhat*w + b) [*g]; dx = ... [+ add]; dw/db/dg/dgb accumulate (fp32 atomics).  dg / dgb [ceil(frames/gdiv)][C] are the
 * gradients of the post scale / shift of an identity act (dg = w*s2 + b*s1, dgb = s1); with gelu they are refused (an error is returned). */
int bf_in_bwd(int dtype, const void* dy, const void* x, const void* add, void* dx, int frames, int S, int C, const float* mean,
              const float* rstd, const float* w, const float* b, const float* g, int gdiv, int gelu, float* dw, float* db,
              float* dg, float* dgb, float* ws /* optional, bf_in_ws_floats(): per-frame partials + reduce instead of atomics */,
              bf_stream_t stream);
/* out[c] += scale[c] * sum_rows x[row][c] */
int bf_colsum(int dtype, const void* x, int64_t nrows, int C, const float* scale, float* out, bf_stream_t stream);

/* Strided small-sequence attention on the head-interleaved QKV tensor [N][3E] (channel = head*3d + {q,k,v}*d + e):
 * token(l) of sequence s = (s / inner) * outer_stride + (s % inner) * inner_stride + l * tok_stride.
 * q/k LayerNorm(d) + q k^T d^-1/2 + T5 bias (emb [32][heads] or NULL) + softmax + high-frequency rescale
 * (hscale [heads] or NULL) + P V.  out [N][E] = (accumulate ? out : 0) + out_scale * result.  1 <= L <= 128: L <= 32 runs the one-wave
 * kernels, 33..128 the long-axis kernels (one workgroup per sequence and head, fp32 arithmetic in both dtypes); L > 128 returns an error. */
int bf_attn_fwd(int dtype, const void* qkv, void* out, int64_t nseq, int L, int64_t inner, int64_t outer_stride,
                int64_t inner_stride, int64_t tok_stride, int heads, int d, const float* qw, const float* qb, const float* kw,
                const float* kb, const float* emb, const float* hscale, float out_scale, int accumulate, bf_stream_t stream);
/* AxialAttentionBlock's attention core (layers/attention.py:212-297): attention along W with hscale_x, along H with hscale_y, both on
 * the shared q/k LayerNorm and T5 table, out = (xx + xy) / 2.  qkv [frames*h*w][3E] token-major, out [frames*h*w][E].  One launch
 * where h, w <= 16 (bf16), otherwise the two bf_attn_fwd passes; the results are bit-identical either way. */
int bf_attn_axial_fwd(int dtype, const void* qkv, void* out, int64_t frames, int h, int w, int heads, int d, const float* qw,
                      const float* qb, const float* kw, const float* kb, const float* emb, const float* hscale_x,
                      const float* hscale_y, bf_stream_t stream);
/* The same followed, in the same launch, by AxialAttentionBlock.norm2 (InstanceNorm2d over the frame, layers/attention.py:298): also
 * writes out_n = (out - mean) * rstd * norm_w + norm_b and mean / rstd / sc / sh [frames][E] exactly as bf_in_stats lays them out.
 * Returns 0 when done, 1 when the one-launch form does not cover the shape (h, w <= 16, bf16): the caller then runs bf_attn_axial_fwd
 * and bf_in_stats + bf_affine_apply. */
int bf_attn_axial_norm_fwd(int dtype, const void* qkv, void* out, void* out_n, int64_t frames, int h, int w, int heads, int d,
                           const float* qw, const float* qb, const float* kw, const float* kb, const float* emb, const float* hscale_x,
                           const float* hscale_y, const float* norm_w, const float* norm_b, float* mean, float* rstd, float* sc,
                           float* sh, bf_stream_t stream);
/* Backward of bf_attn_fwd.  accumulate: 0 = dqkv is written, 1 = added to.  Two passes over the SAME tokens (the axial block's W and H
 * attention, layers/attention.py:218-277, share one q / k LayerNorm) may run that LayerNorm's backward -- linear in its incoming gradient --
 * once: first pass accumulate = 2 (q / k columns of dqkv receive the raw gradient with respect to the LayerNorm outputs; no LayerNorm
 * parameter sums), second pass accumulate = 5 (adds the raw values in front of its LayerNorm backward, v as with 1).  bf16 MFMA path only. */
int bf_attn_bwd(int dtype, const void* qkv, const void* dout, void* dqkv, int64_t nseq, int L, int64_t inner,
                int64_t outer_stride, int64_t inner_stride, int64_t tok_stride, int heads, int d, const float* qw,
                const float* qb, const float* kw, const float* kb, const float* emb, const float* hscale, float* dqw,
                float* dqb, float* dkw, float* dkb, float* demb, float* dhscale, float out_scale, int accumulate,
                float* ws, int64_t ws_floats, /* optional workspace for the block-partial parameter gradients (NULL: atomics) */
                bf_stream_t stream);

/* test hook: route bf16 attention through the generic fp32-VALU kernel instead of the MFMA kernel (L <= 32; the long-axis kernels,
 * L > 32, compute in fp32 VALU already and are the only path there: the hook does not change them, but with it on the raw-gradient
 * modes are refused at every L, as bf_attn_raw_modes answers) */
/* Weight-gradient GEMMs run on a library-owned side stream that every stage joins before it returns.  bf_side_defer(1) lets a
 * temporal / spatial backward return with its LAST weight-gradient GEMM still in flight: the next stage call on the stream joins it
 * (before it reuses what that GEMM reads), as does bf_side_join().  A caller that opts in must call bf_side_join(stream) before it
 * reads parameter gradients outside the library (optimizer step, all-reduce of the stage's bucket).  Default: off. */
void bf_side_defer(int on);
int bf_side_join(bf_stream_t stream);
void bf_debug_force_generic_attn(int on);
/* test hook: 0 = every weight-gradient slab sum runs as a launch of its own right behind its GEMM; 1 (default) = inside the stage backwards it
 * rides in the NEXT token-reduction launch (extra workgroups) -- the results are bit-identical either way */
void bf_debug_tokred_fold(int on);

int bf_im2col_nchw(int dtype, const float* x, void* out, int frames, int C, int H, int W, int Kp, bf_stream_t stream);
int bf_col2im_nchw(int dtype, const void* g, float* dx, int frames, int C, int H, int W, int Kp, bf_stream_t stream);
/* lossbuf (here, in bf_debed_last and bf_lploss_finalize): [frames][Co][2][BF_LOSS_LIMBS] int64, zeroed by the caller: the sums of (pred - y)^2
 * and of y^2 as integers -- base-2^48 digits in units of 2^-112, one 64-bit integer atomic per non-zero digit of a partial.  Integer adds are
 * order independent, so the loss and its gradient are bit-reproducible run to run; the limbs cover partial sums in [2^-112, 2^127), i.e. the
 * range of the reference's float sums (utils/losses.py:79-89): un-normalised fields and nearly converged numerators included. */
#define BF_LOSS_LIMBS 5
int bf_pm2nchw(const float* pm, float* pred, const float* y, float* lossbuf, int frames, int Co, int h, int w, int Np,
               bf_stream_t stream);
/* Last HMLPDebed stage in one pass (layers/patching.py:92-104: InstanceNorm affine + GELU on the input rows, ConvTranspose2d(k=2,s=2)
 * to the NCHW prediction) with the relative-L2 partial sums of bf_pm2nchw; act [frames*h*w][Ci], sc/sh [frames][Ci], wc [Ci][Np] with
 * n = co*4 + ky*2 + kx.  Returns 1 (nothing launched) for shapes it does not take: fp32, Np != 16, Co > 4, Ci % 32, Ci > 128, w % 16. */
int bf_debed_last(int dtype, const void* act, const float* sc, const float* sh, const void* wc, float* pred, const float* y,
                  float* lossbuf, int frames, int Ci, int Co, int h, int w, int Np, bf_stream_t stream);
/* ... and its backward: dpm [frames*h*w][Np] (bf_nchw2pm's output, kept for the weight-gradient GEMM) and dact[p][ci] = sum_n dpm[p][n]*wc[ci][n]
 * in one pass.  Same declined shapes (returns 1).  Three source modes, here and in bf_debed_last_bwd_norm / bf_nchw2pm: dpred alone (pred = y =
 * NULL), the fused loss alone (dpred = NULL; pred, y, coef given): d pred = coef[f][co] * gscale[0] * (pred - y), or BOTH (dpred, pred, y and
 * coef all given): d pred = dpred + coef[f][co] * gscale[0] * (pred - y), formed in fp32 registers in the same pass -- the backward of one
 * pass of a training step unrolled through its own predictions.  gscale = NULL means 1. */
int bf_debed_last_bwd(int dtype, const float* dpred, const float* pred, const float* y, const float* coef, const float* gscale,
                      const void* wc, void* dpm, void* dact, int frames, int Ci, int Co, int h, int w, int Np, bf_stream_t stream);
/* ... and with the InstanceNorm + GELU in front of the stage folded in (layers/patching.py:92-104 under autograd): dpm as above, and
 * dx [frames*h*w][Ci] = the gradient of the RAW map ymap in front of that InstanceNorm (mean / rstd [frames][Ci], affine in_w / in_b) --
 * two passes over ymap around the frame-wide sums, the rank-16 gradient map itself is never stored.  d_in_w / d_in_b are accumulated
 * (optional).  ws: bf_in_ws_floats(dtype, frames, h*w, Ci) floats.  Same declined shapes (returns 1), also for a workspace too small. */
int bf_debed_last_bwd_norm(int dtype, const float* dpred, const float* pred, const float* y, const float* coef, const float* gscale,
                           const void* wc, void* dpm, const void* ymap, const float* mean, const float* rstd, const float* in_w,
                           const float* in_b, void* dx, float* d_in_w, float* d_in_b, int frames, int Ci, int Co, int h, int w, int Np,
                           float* ws, int64_t ws_floats, bf_stream_t stream);
/* First HMLPEmbed stage (layers/patching.py:30-48: Conv2d(k=2, s=2, bias=False) on the NCHW fp32 clip) in one pass: patches [P][Kp]
 * (k = c*4 + ky*2 + kx, what bf_im2col_nchw writes; kept for the weight gradient) and y0[p][co] = sum_k patches[p][k] * wc[co][k].
 * Same kernel and declined shapes as bf_debed_last_bwd (returns 1). */
int bf_embed_first(int dtype, const float* x, const void* wc, void* patches, void* y0, int frames, int C0, int cin, int h2, int w2,
                   int Kp, float* stat_part, bf_stream_t stream);
/* y0 may be NULL when stat_part is given: the map is then not stored at all -- its consumers rebuild its rows from `patches` and `wc`
 * (bf_gather_gemm_rebuilt, bf_gather_wgrad_rebuilt, bf_embed_tail_bwd with y0 = NULL), which is 226 MB less to write and three reads of it
 * less per training step at the bench shape. */
/* stat_part (optional): {mean, centred second moment} of y0 per 256-row slice, [frames][ceil(h2*w2/256)][C0][2]; finished by
 * bf_in_stats_merge_slices(..., rows = 256, ws) with ws + 2*frames*C0 == stat_part (the layout bf_in_stats uses for long frames). */
int bf_in_stats_merge_slices(int dtype, int frames, int S, int C, int rows, const float* w, const float* b, const float* g, int gdiv,
                             const float* gb, float* mean, float* rstd, float* sc, float* sh, float* ws, bf_stream_t stream);
/* The tail of the HMLPEmbed backward when the input needs no gradient (layers/patching.py:24-56 under autograd): the stage-1 data
 * gradient dy1 [frames*gh1*gw1][C1] times w1c [C1][4*C0] (the stage-1 weight, columns (2*ky + kx)*C0 + c), GELU', the stage-0 InstanceNorm
 * backward and the stage-0 weight gradient in one pass that never writes the [frames*4*gh1*gw1][C0] gradient map.  y0: raw stage-0
 * output, or NULL (its rows are then rebuilt from the patch rows: y0 = W0 . patch); patches [..][Kp] (bf_embed_first), w0c [C0][Kp], sc / sh / mean / rstd [frames][C0] of the stage-0 InstanceNorm, in_w its
 * weight.  dwprep [C0][Kp] is WRITTEN (bf_wgrad_unprep folds it into the gradient), d_in_w / d_in_b [C0] are accumulated (optional).
 * ws: bf_embed_tail_ws_floats floats.  Returns 1 (nothing launched) for shapes it does not take: fp32, C0 != 96, C1 not in {96, 192}, Kp != 16,
 * gw1 % 16, gh1*gw1 % 128, or a workspace that is too small. */
/* The 2x2 / stride-2 stages at 96 channels as one streaming GEMM: out[p][n] = sum_{q, c} f(map[pixel(p, q)][c]) * W[(q, c)][n], p over the
 * coarse grid [frames][gh][gw], pixel(p, q) = (2y + q/2, 2x + q%2) of the fine grid [frames][2gh][2gw][C0].  f = GELU(x * sc + sh)
 * (sc / sh [frames][C0]: the HMLPEmbed convolutions after the first, layers/patching.py:30-56) or the identity (sc = sh = NULL: the data
 * gradients of the HMLPDebed transposed convolutions).  w: [4*C0][N] (w_kn = 1) or [N][4*C0] (w_kn = 0).  Returns 1 (nothing launched)
 * for shapes it does not take: fp32, C0 != 96, N != 96, gh*gw % 32. */
int bf_gather_gemm(int dtype, const void* map, const void* w, int w_kn, const float* sc, const float* sh, void* out, int frames, int gh,
                   int gw, int C0, int N, bf_stream_t stream);
/* ... and the transposed direction (HMLPDebed's ConvTranspose2d(k=2, s=2) stages, layers/patching.py:80-104): map[pixel(p, q)][c] =
 * sum_k f(a[p][k]) * w[q*C0 + c][k] (w_kn = 0; or w [K][4*C0] with w_kn = 1), a [frames*gh*gw][K], map [frames][2gh][2gw][C0].  stat_part (optional): {mean, centred second moment} of the
 * map as stored per 128-pixel slice, [frames][gh*gw/32][C0][2]; finished by bf_in_stats_merge_slices(..., rows = 128, ws) with
 * ws + 2*frames*C0 == stat_part.  Returns 1 (nothing launched) for: fp32, K != 96, C0 != 96, gh*gw % 32. */
int bf_scatter_gemm(int dtype, const void* a, const void* w, int w_kn, const float* sc, const float* sh, void* map, float* stat_part, int frames,
                    int gh, int gw, int K, int C0, bf_stream_t stream);
/* ... and their weight gradients: dW[(q, c)][k] = sum_p ff(fine[pixel(p, q)][c]) * fc(coarse[p][k]), fine [frames][2gh][2gw][C0], coarse
 * [frames*gh*gw][Kc]; at most one side through GELU(x * sc + sh) ([frames][96] each; the embed stages transform the fine side, the debed
 * stages the coarse side).  out is WRITTEN: [4*C0][Kc] (transposed = 0) or [Kc][4*C0] (transposed = 1); per-workgroup slabs summed in a
 * fixed order (bit-reproducible).  ws: bf_gather_wgrad_ws_floats floats for the preferred launch (anything from frames * 36864 floats
 * up is accepted: fewer, longer runs).  Returns 1 (nothing launched) for: fp32, C0 != 96, Kc != 96,
 * gh*gw % 32, both sides transformed, a workspace too small. */
int64_t bf_gather_wgrad_ws_floats(int frames, int gh, int gw);
int bf_gather_wgrad(int dtype, const void* fine, const void* coarse, const float* fsc, const float* fsh, const float* csc, const float* csh,
                    float* out, int transposed, int frames, int gh, int gw, int C0, int Kc, float* ws, int64_t ws_floats, bf_stream_t stream);
/* bf_gather_gemm / bf_gather_wgrad with the fine map given as its factors, map[pixel][c] = sum_k patches[pixel][k] * w0c[c][k] (Kp = 16: the
 * output of bf_embed_first), rebuilt per tile and rounded to bf16 like a stored map; the fine side is transformed by GELU(x * sc + sh). */
int bf_gather_gemm_rebuilt(int dtype, const void* patches, const void* w0c, const void* w, int w_kn, const float* sc, const float* sh, void* out,
                           int frames, int gh, int gw, int C0, int N, bf_stream_t stream);
int bf_gather_wgrad_rebuilt(int dtype, const void* patches, const void* w0c, const void* coarse, const float* fsc, const float* fsh, float* out,
                            int transposed, int frames, int gh, int gw, int C0, int Kc, float* ws, int64_t ws_floats, bf_stream_t stream);
int64_t bf_embed_tail_ws_floats(int frames, int gh1, int gw1, int C0, int Kp);
int bf_embed_tail_bwd(int dtype, const void* dy1, const void* w1c, const void* y0, const void* patches, const void* w0c, const float* sc,
                      const float* sh, const float* mean, const float* rstd, const float* in_w, float* dwprep, float* d_in_w, float* d_in_b,
                      int frames, int gh1, int gw1, int C1, int C0, int Kp, float* ws, int64_t ws_floats, bf_stream_t stream);
int bf_lploss_finalize(const float* lossbuf, int frames, int Co, float* loss, float* coef, bf_stream_t stream);
int bf_nchw2pm(int dtype, const float* dpred, const float* pred, const float* y, const float* coef, const float* gscale,
               void* dpm, int frames, int Co, int h, int w, int Np, bf_stream_t stream);
int bf_wprep(int dtype, int mode, const float* src, void* dst, int R, int K, int Kp, bf_stream_t stream);
int bf_wgrad_unprep(int mode, const float* gsrc, float* gdst, int R, int K, int Kp, int transposed, bf_stream_t stream);
/* gb: [2][B][E] (gamma block, beta block) */
int bf_film_net_fwd(const float* cond, const float* lnw, const float* lnb, const float* W, const float* bias, float* gb,
                    float* chat, float* crstd, int B, int P, int E2, bf_stream_t stream);
int bf_film_net_bwd(const float* dgb, const float* chat, const float* lnw, const float* lnb, const float* W, float* dW,
                    float* dbias, float* dlnw, float* dlnb, int B, int P, int E2, bf_stream_t stream);
/* Batch of normalised clips from device-resident trajectories src [fields][frames][H][W] (fp32):
 * out[b][t][c][yo][xo] = (src[field[c]][first[b] + t0 + t][ys][xs] - diff[c]) / div[c], (ys, xs) = nearest-neighbour source pixel of
 * (yo, xo) when Ho x Wo < H x W (F.interpolate(mode="nearest") index rule), identity otherwise.  out is (B, T, C, Ho, Wo) fp32. */
int bf_clip_gather(const float* src, int64_t field_stride, const int32_t* field, const int64_t* first, int t0, const float* diff,
                   const float* div, float* out, int B, int T, int C, int H, int W, int Ho, int Wo, bf_stream_t stream);
/* The same for a whole training batch in one launch, indexed by SAMPLE number on the device: idx [B] (int64; clamped to 0 .. nsamples - 1 in the
 * kernel, so a bad index reads another sample, never past a table), first_tab / file_tab [nsamples] = absolute first input frame and file of every sample.  in_out (B, Tin, Cin, Ho, Wo) = frames
 * first .. first + Tin - 1 of the input fields, out_out (B, Tout, Cout, Ho, Wo) = the Tout frames behind them of the output fields (each with
 * its own field ids and constants), fluid_out (B, P) = fluid_tab[file_tab[idx[b]]] (optional: fluid_out may be null).
 * Replaces BubbleForecast.__getitem__ + the DataLoader's collate for a batch (bubbleformer/data/dataset.py:120-182). */
int bf_clip_gather_batch(const float* src, int64_t field_stride, const int64_t* idx, int64_t nsamples, const int64_t* first_tab, const int32_t* in_field,
                         const float* in_diff, const float* in_div, int Cin, int Tin, float* in_out, const int32_t* out_field,
                         const float* out_diff, const float* out_div, int Cout, int Tout, float* out_out, const float* fluid_tab,
                         const int64_t* file_tab, int P, float* fluid_out, int B, int H, int W, int Ho, int Wo, bf_stream_t stream);
/* ... with `unroll` >= 1 target clips behind the input clip, for a training step unrolled through its own predictions: out_out is
 * (unroll, B, Tout, Cout, Ho, Wo), clip j = frames first + Tin + j*Tout .. first + Tin + (j+1)*Tout - 1, each clip contiguous; one launch.
 * nframes = frames per field in src: idx is clamped as above, and a frame index is held below nframes, so a sample whose later clips lie
 * behind its own file (the caller's business: DeviceClipStore.gather refuses such host indices) reads the next file's frames (the store's last frame where the store ends), never
 * past it. */
int bf_clip_gather_unroll(const float* src, int64_t field_stride, int64_t nframes, const int64_t* idx, int64_t nsamples, const int64_t* first_tab,
                          const int32_t* in_field, const float* in_diff, const float* in_div, int Cin, int Tin, float* in_out,
                          const int32_t* out_field, const float* out_diff, const float* out_div, int Cout, int Tout, int unroll, float* out_out,
                          const float* fluid_tab, const int64_t* file_tab, int P, float* fluid_out, int B, int H, int W, int Ho, int Wo,
                          bf_stream_t stream);
/* bf_clip_gather_unroll with a seeded mirror in x and a seeded window per sample (csrc/clip_store.hip), one launch.
 * bf_clip_gather_job carries bf_clip_gather_unroll's arguments under their names there (unroll >= 1; reserved is unread); the outputs are
 * in_out (B, Tin, Cin, Hc, Wc), out_out (unroll, B, Tout, Cout, Hc, Wc) and the plain fluid_out (B, P).  With plain[c][t][y][x] the value
 * bf_clip_gather_unroll forms on its Ho x Wo grid BEFORE normalisation, sample b gets
 *   out[c][t][y][x] = (s_c * plain[c][t][y0 + y][xs] - diff[c]) / div[c],   xs = x0 + x, or x0 + Wc - 1 - x when the sample is mirrored
 *   (the window is chosen first, then mirrored), s_c = -1 iff the sample is mirrored and the segment's odd table holds a non-zero at c
 *   (in_odd [Cin], out_odd [Cout], int32 in DEVICE memory: 1 where the channel's field changes sign under x -> -x), else +1.
 * The decision is one Philox4x32-10 block per sample (Random123's constants, as bf_clip_noise): key = {low, high word of seed}, counter =
 *   {0xFFFFFFFF, low 32 bits of idx[b] clamped to 0 .. nsamples - 1, draw, 0} -> (w0, w1, w2, w3).  bf_clip_noise's counter word 0 is a group
 *   number < 2^29, so under one seed the two never share a block.
 *   mirrored iff w0 < flip_thr      (flip_thr = min(round(p * 2^32), 2^32) as a 64-bit value: 0 never mirrors, 2^32 always does)
 *   x0 = (w1 * (Wo - Wc + 1)) >> 32 in 64-bit arithmetic;  y0 = (w2 * (Ho - Hc + 1)) >> 32 when crop_y == 1, 0 when crop_y == 0 (the window
 *   keeps output row 0, the heater row);  w3 is unused.  seed and draw are read as unsigned bit patterns.
 *   eval_view == 1 draws nothing: never mirrored, x0 = (Wo - Wc) / 2, y0 = 0 (the deterministic view for validation).
 * The input clip, every target clip and all frames of a sample share its decision: a pure function of (seed, sample, draw), whatever B and
 * the sample's place in the batch.  Requires bf_clip_gather_unroll's conditions and 1 <= Hc <= Ho, 1 <= Wc <= Wo; a null record or a null
 * required member is refused as "bf_clip_gather_augment: null pointer", every check is made before any HIP call.  Loads and stores are 16
 * bytes wide when Ho x Wo = H x W and W, Wc and the sample's x0 are multiples of 4, scalar otherwise. */
typedef struct bf_clip_gather_job {
    const float* src; const int64_t *idx, *first_tab;
    const int32_t* in_field; const float *in_diff, *in_div; float* in_out;
    const int32_t* out_field; const float *out_diff, *out_div; float* out_out;
    const float* fluid_tab; const int64_t* file_tab; float* fluid_out;
    int64_t field_stride, nframes, nsamples;
    int32_t Cin, Tin, Cout, Tout, unroll, P, B, H, W, Ho, Wo, reserved;
} bf_clip_gather_job;
typedef struct bf_clip_augment {
    const int32_t *in_odd, *out_odd;
    int64_t seed, flip_thr;
    int32_t draw, Hc, Wc, crop_y, eval_view, reserved;
} bf_clip_augment;
int bf_clip_gather_augment(const bf_clip_gather_job* job, const bf_clip_augment* augment, bf_stream_t stream);
/* The 16-bit form of the store (csrc/clip_store_q16.hip states the format): codes [fields][frames][H][W] of 16 bits,
 * one affine scale per SEGMENT = all frames of one field of one file, tables indexed field * nfiles + file.  Per segment lo / hi = the exact
 * fp32 minimum / maximum, step = fp32(((double)hi - (double)lo) / 65535.0), inv = fp32(65535.0 / ((double)hi - (double)lo)), both 0 when
 * hi == lo.  code = clamp(rintf((x - lo) * inv), 0, 65535) and x^ = fp32(fp32((float)code * step) + lo), every operation rounded on its
 * own (no fma): np.float32 arithmetic gives the same bits.  |x^ - x| <= 0.53 step + 2^-24 max(|lo|, |hi|); a constant segment and lo decode
 * exactly; a value closer to zero than step / 2 may change sign.
 * bf_clip_encode_q16: dst[i] = code(src[i]) for the n values of one staged chunk of one segment (src 4-byte, dst 2-byte aligned; 16-byte
 *   loads and 8-byte stores when src is 16-byte and dst 8-byte aligned, scalar otherwise and for the last n % 4 values).
 * bf_clip_decode_q16: dst [nfields][nframes][H][W] fp32, contiguous, = the decoded store, one launch; frame_seg [nframes] int32 = the file
 *   of every frame of the store's frame axis (held into 0 .. nfiles - 1), seg_lo / seg_step [nfields * nfiles] fp32, all on the DEVICE.
 * bf_clip_gather_q16: ONE launch for what bf_clip_gather_batch, bf_clip_gather_unroll and bf_clip_gather_augment give on the decoded store,
 *   bit for bit: x^ takes the stored value's place in their expressions (the mirror's sign goes on x^, then (.. - diff) / div).  The job is
 *   bf_clip_gather_job's members (unroll >= 1) with `codes`, the three tables of bf_clip_decode_q16 and nfiles in front of them; augment may
 *   be NULL: the whole Ho x Wo grid, no mirror, in_out (B, Tin, Cin, Ho, Wo), out_out (unroll, B, Tout, Cout, Ho, Wo).  The scale of a value
 *   is that of the frame actually read (frame_seg of the clamped frame number), not of the sample's file.  Requires what
 *   bf_clip_gather_augment requires of its records (the codes in src's place: 2-byte aligned, and 8-byte aligned with field_stride a
 *   multiple of 4 when Ho x Wo = H x W and W and the window's width are multiples of 4: rows are then read four codes at a time wherever a
 *   sample's x0 is a multiple of 4, scalar otherwise); a null job or required member is refused as "bf_clip_gather_q16: null pointer", and
 *   every check is made before any HIP call.  No LDS, no atomics, no workspace; capturable; two calls give the same bits. */
typedef struct bf_clip_gather_q16_job {
    const uint16_t* codes; const int32_t* frame_seg; const float *seg_lo, *seg_step;
    const int64_t *idx, *first_tab;
    const int32_t* in_field; const float *in_diff, *in_div; float* in_out;
    const int32_t* out_field; const float *out_diff, *out_div; float* out_out;
    const float* fluid_tab; const int64_t* file_tab; float* fluid_out;
    int64_t field_stride, nframes, nsamples;
    int32_t nfiles, Cin, Tin, Cout, Tout, unroll, P, B, H, W, Ho, Wo;
} bf_clip_gather_q16_job;
int bf_clip_encode_q16(const float* src, uint16_t* dst, int64_t n, float lo, float inv, bf_stream_t stream);
int bf_clip_decode_q16(const uint16_t* codes, int64_t field_stride, const int32_t* frame_seg, const float* seg_lo, const float* seg_step, float* dst,
                       int64_t nframes, int nfields, int nfiles, int H, int W, bf_stream_t stream);
int bf_clip_gather_q16(const bf_clip_gather_q16_job* job, const bf_clip_augment* augment, bf_stream_t stream);
/* Seeded Gaussian noise on a batch of clips (csrc/noise.hip): dst[b][t][c][y][x] = fmaf(sigma[c], z, src[b][t][c][y][x]) on contiguous fp32
 * (B, T, C, H, W); an element of a channel with sigma[c] == 0 is handed back bit for bit.  dst == src (in place) or two buffers that do not
 * overlap.  z is a pure function of (seed, sample id, draw, pass, element index e inside the sample's flattened (T, C, H, W) clip):
 *   (w0, w1, w2, w3) = Philox4x32-10(counter = {e / 4, low 32 bits of sample_ids[b] (b itself when sample_ids is NULL), draw, pass},
 *                                    key = {low, high word of seed}), Random123's constants;
 *   Box-Muller per pair (a, b) = (w0, w1) for elements 4g, 4g + 1 and (w2, w3) for 4g + 2, 4g + 3: u1 = ((a >> 8) + 1) * 2^-24,
 *   u2 = (b >> 8) * 2^-24, r = sqrtf(-2 * logf(u1)), the pair r * cospif(2 * u2), r * sinpif(2 * u2); |z| <= 5.77.  A sample size that is no
 *   multiple of 4 uses the leading words of its last group.
 * sigma [C] fp32 and sample_ids [B] int64 are DEVICE tables.  One launch, no workspace, no LDS, no atomics, capturable; two calls give the same
 * bits, and a sample's row does not depend on B or on its position in the batch.  T * C * H * W < 2^31.  Loads and stores are 16 bytes wide when
 * that size is a multiple of 4 and both pointers are 16-byte aligned, scalar otherwise. */
int bf_clip_noise(const float* src, float* dst, const float* sigma, const int64_t* sample_ids, uint64_t seed, uint32_t draw, uint32_t pass,
                  int B, int T, int C, int H, int W, bf_stream_t stream);
/* Normalisation statistics of device-resident trajectories (BubbleForecast.normalize, bubbleformer/data/dataset.py:74-117: mean / std / min /
 * max of every full field of every file): segment i = seg_len[i] floats at src + seg_begin[i] (both arrays on the DEVICE);
 * out[i] = {sum, sum of squares, min, max} in fp64, summed in a fixed order (bit-reproducible).  ws: bf_field_stats_ws_doubles(nseg) doubles. */
int64_t bf_field_stats_ws_doubles(int nseg);
int bf_field_stats(const float* src, const int64_t* seg_begin, const int64_t* seg_len, int nseg, double* out, double* ws, bf_stream_t stream);
/* Rollout physics metrics (scripts/inference.py; utils/losses.py:5-15, utils/heatflux.py:17-38).
 * bf_eikonal_sum: *out (fp64, caller zeroes) += sum over frames x H x W of (|grad phi| - 1)^2, gradients as torch.gradient(spacing=dx).
 * bf_heatflux_rows: flux[t] = mean over the W bottom-row cells of [|x_c| <= 5 and dfun < 0] * (heater_temp - temp) * 0.054 / (dx * lc),
 * x_c = x_min + (i + 0.5) * dx; dfun / temp point at row 0 of frame 0, frames are frame_stride elements apart. */
int bf_eikonal_sum(const float* phi, int64_t frames, int H, int W, float dx, double* out, bf_stream_t stream);
/* out[frame] = mean over the frame of | |grad phi| - 1 |, central differences at spacing dx, borders replicate their neighbour's
 * gradient: `get_eikonal_loss` of scripts/inference_autoregressive.ipynb (the rollout notebook's per-time-step SDF score). */
int bf_eikonal_l1_frames(const float* phi, int64_t frames, int H, int W, float dx, float* out, bf_stream_t stream);
int bf_heatflux_rows(const float* dfun, const float* temp, int64_t frames, int64_t frame_stride, int W, float x_min, float dx,
                     float heater_temp, float lc, float* flux, bf_stream_t stream);
/* The records of the rollout-evaluation calls.  The library reads a record DURING the call only and keeps no pointer to it; what a kernel needs
 * of it is copied by value into the kernel's arguments, so the calls stay capturable and a record may live on the caller's stack.
 * bf_rollout_step (the calls' parameter `s`): ONE autoregressive rollout step, the prediction and where its targets lie.  pred (B, T, C, Ho, Wo)
 * fp32; frames [nfields][total_frames][H][W] fp32 with field_stride floats per field (DeviceClipStore.frames); first [B] int64 (device) = absolute
 * first INPUT frame of step 0 per trajectory; step = one int32 in DEVICE memory, the step NUMBER s = *step: READ by every call and written by
 * bf_rollout_score alone (its last launch increments it, hence not const), so a step's other calls are issued BEFORE its bf_rollout_score;
 * field / diff / div [C] = the store's output-field table.  Target of (b, t, c): y = (frames[field[c]][first[b] + (s + 1) * T + t][ys][xs] - diff[c]) /
 * div[c], the expression and nearest-neighbour map of bf_clip_gather (the same device functions), frame index clamped into the store.  steps = the
 * steps a report has rows for: with s outside [0, steps) a call writes nothing.  reserved is unread: it spells out the padding that ends the record. */
typedef struct bf_rollout_step {
    const float *pred, *frames;
    int64_t field_stride, total_frames;
    const int64_t* first; int32_t* step; const int32_t* field;
    const float *diff, *div;
    int32_t nfields, B, T, C, H, W, Ho, Wo, steps, reserved;
} bf_rollout_step;
/* One side's census rows: bf_bubble_census' count / vapour_cells / attached [rows] and area [rows][max_bubbles] */
typedef struct bf_census_rows { int32_t *count, *cells, *attached, *area; } bf_census_rows;
/* One side's link rows: bf_bubble_links' five [pairs][max_bubbles] outputs and events [pairs][5] */
typedef struct bf_link_rows { int32_t *successor, *n_successors, *predecessor, *n_predecessors, *departure_area, *events; } bf_link_rows;
/* bf_bubble_match's outputs, row = frame pair: three int32 rows and displacement [rows][max_bubbles], counts [rows][6], mask [rows][2]; all required */
typedef struct bf_match_rows { int32_t *match_pred, *match_target, *overlap; float* displacement; int32_t *counts, *mask; } bf_match_rows;
/* bf_field_errors' outputs; each may be NULL and is then not computed */
typedef struct bf_error_rows {
    float *rmse, *max_error, *boundary_rmse, *interface_rmse;
    int32_t* interface_cells;
    float *spectral_error, *spectrum_error, *spectrum_pred, *spectrum_target;
} bf_error_rows;
/* All scores of ONE autoregressive rollout step from one pass over the prediction (scripts/inference.py:230-266, utils/plot_utils.py:30-33, the
 * rollout notebook's get_eikonal_loss); allocation-free, capturable, no atomics (two calls on the same inputs give the same bits).
 * s: see bf_rollout_step.  Written at row s * T + t:
 *   rel_l2 [B][steps*T][C]  = sqrt(sum (pred - y)^2 / sum y^2) over (Ho, Wo): differences, squares, sums, quotient and root in fp64, rounded once
 *                             (a target frame of zeros gives inf or NaN, as the reference's quotient of norms does);
 *   criterion [B][steps]    = mean over t, then over c, of those fp64 quotients (LpLoss(d=2, p=2, reduce_dims=[0, 1], reductions=["mean", "mean"]));
 *   eik_pred, eik_tgt [B][steps*T] (sdf_channel >= 0 only; Ho, Wo >= 3) = bf_eikonal_l1_frames' score at spacing dx of the signed-distance field in
 *                             physical units: prediction pred * div + diff (fp32 multiply, then add, unfused), target the stored frame (downsampled);
 *   next_in (B, T, C, Ho, Wo), archive (B, steps*T, C, Ho, Wo) rows s*T .. s*T + T - 1 (each optional) = copies of pred.
 * The last launch sets *step = s + 1.  The host cannot see s: with s outside [0, steps) the call writes nothing and leaves *step as it is.
 * ws: bf_rollout_score_ws_doubles(B, T, C, Ho, Wo) doubles (fp64 partials per workgroup, added in a fixed order).  pred, frames and the copies
 * 16-byte aligned; B * T * C <= 65535. */
int64_t bf_rollout_score_ws_doubles(int B, int T, int C, int Ho, int Wo);
int bf_rollout_score(const bf_rollout_step* s, int sdf_channel, float dx, float* rel_l2, float* criterion, float* eik_pred, float* eik_tgt,
                     float* next_in, float* archive, double* ws, int64_t ws_doubles, bf_stream_t stream);
/* The heat-flux rows of ONE rollout step (utils/heatflux.py:3-38 per step of scripts/inference.py:239-252; csrc/rollout.hip), for the prediction
 * and for the simulation; allocation-free, capturable, no atomics (the same bits on every call), never makes the host wait.  s: see
 * bf_rollout_step.  With the step number s = *s->step, row s * T + t of trajectory b of flux_pred / flux_tgt [B][steps*T] is
 * bf_heatflux_rows' expression on row 0 (the heater row) of frame t:
 *   mean over ALL Wo cells of [-5 <= x_c <= 5 and dfun < 0] * (heater_temp[b] - temp) * conductivity / (dx * lc),  x_c = x_min + (i + 0.5) * dx in fp64,
 * the difference in fp32, the sum in fp64 in a fixed order, one rounding; heater_temp [B] fp32 on the DEVICE.
 *   flux_pred: dfun = pred * div + diff of channel dfun_channel, temp likewise of temp_channel (fp32 multiply, then add, unfused: the physical
 *              field bf_rollout_score's Eikonal rows see);
 *   flux_tgt:  the stored raw frame first[b] + (s + 1) * T + t (clamped into the store) of fields field[dfun_channel] / field[temp_channel],
 *              through bf_clip_gather's nearest-neighbour map when Ho x Wo < H x W.
 * With s outside [0, steps) nothing is written. */
int bf_rollout_heatflux(const bf_rollout_step* s, int dfun_channel, int temp_channel, const float* heater_temp, float x_min, float dx, float lc,
                        float conductivity, float* flux_pred, float* flux_tgt, bf_stream_t stream);
/* KL(p || q) of the Gaussian kernel density estimates of two sample sets, for R independent rows (examples/data_visualization.ipynb cell 4:
 * scipy.stats.gaussian_kde of each set, np.linspace grid, scipy.integrate.simpson; csrc/physics.hip).  Everything fp64 on the device, allocation-free,
 * capturable, no atomics (the same bits on every call, and a row has the same bits alone and in a batch).  p [R][n] (the simulation), q [R][m]
 * (the model), n, m >= 2, points >= 3, R <= 65535.  Per row: mean, then unbiased variance from centred squares, min and max of each set;
 * bandwidth h = n^(-1/5) * sqrt(var) (Scott's factor); grid x_i = lo + i * (hi - lo) / (points - 1), x_{points-1} = hi over the smaller minimum /
 * larger maximum; pdf(x_i) = sum_j exp(-((x_i - s_j) / h)^2 / 2) / (n * h * sqrt(2 pi)), partial sums per slab of samples added in slab order;
 * q_i == 0 becomes eps; f_i = p_i * log(p_i / q_i), and f_i = 0 where p_i == 0 (the limit; numpy has 0 * -inf = NaN there, so the notebook
 * returns NaN for far-apart sets -- the one deliberate deviation); kl[r] = Simpson's rule on the uniform grid as scipy 1.15 applies it: composite
 * Simpson for odd points, for even points composite Simpson over the first points - 1 nodes plus step * (5 f_{N-1} + 8 f_{N-2} - f_{N-3}) / 12.
 * A set of zero variance gives kl = NaN (and NaN densities).  x, pdf_p, pdf_q [R][points] are optional (null: not written).
 * ws: bf_kde_kl_ws_doubles(R, n, m, points) doubles = R * (8 + slabs * points) with at most 128 slabs: O(points) per row, no points x n matrix. */
int64_t bf_kde_kl_ws_doubles(int R, int64_t n, int64_t m, int points);
int bf_kde_kl(const double* p, const double* q, int R, int64_t n, int64_t m, int points, double eps, double* kl, double* x, double* pdf_p,
              double* pdf_q, double* ws, int64_t ws_doubles, bf_stream_t stream);
/* The bubble census of `frames` fields phi [frames][H][W] fp32 in physical units (csrc/bubbles.hip; the reference has no program for it).  Vapour is
 * phi > 0: an exact zero and a NaN are liquid.  A bubble is a connected component of vapour cells under connectivity 4 or 8; the bubbles of a frame
 * are numbered 1, 2, ... in raster order of their first cell (smallest y * W + x), which is scipy.ndimage.label's numbering.  Per frame:
 *   count [frames] int32         the number of components, also above max_bubbles; -1 if a bounded loop of the kernel ran out (a corrupted run);
 *   vapour_cells [frames] int32  the number of vapour cells;
 *   attached [frames] int32      the number of components with a cell in row 0 (the heater row); they are the first `attached` of the numbering;
 *   area [frames][max_bubbles] int32, centroid [frames][max_bubbles][2] fp32 (y, x), on_heater [frames][max_bubbles] bytes: the first max_bubbles
 *                                components in that order, unused slots 0; a centroid is the quotient of exact integer sums, one fp64 division
 *                                rounded once to fp32; centroid and on_heater are optional (null: not written);
 *   labels [frames][H][W] int32  optional: the label image, 0 = liquid.
 * One workgroup owns a frame; integer atomics only: the same bits on every call, and a frame has the same bits alone and in a batch.  Allocation-free,
 * capturable, never makes the host wait.  Any H, W >= 1 with H * W <= 2^24 (refused beyond, before any launch).  Frames of at most
 * bf_bubble_census_lds_cells() cells keep the union-find's parents in LDS, larger ones in the workspace.
 * ws: bf_bubble_census_ws_bytes(frames, H, W, max_bubbles) bytes, 16-byte aligned (0 from the query: sizes out of range). */
int64_t bf_bubble_census_lds_cells(void);
int64_t bf_bubble_census_ws_bytes(int64_t frames, int H, int W, int max_bubbles);
int bf_bubble_census(const float* phi, int64_t frames, int H, int W, int connectivity, int max_bubbles, int32_t* count, int32_t* vapour_cells,
                     int32_t* attached, int32_t* area, float* centroid, unsigned char* on_heater, int32_t* labels, void* ws, int64_t ws_bytes,
                     bf_stream_t stream);
/* The bubble census of ONE rollout step, of the prediction and of the simulation in one call.  s: see bf_rollout_step.  With the step number s = *s->step, row
 * s * T + t of trajectory b of a side's count / cells / attached [B][steps*T] and area [B][steps*T][max_bubbles] is bf_bubble_census' count /
 * vapour_cells / attached / area of
 *   pred: pred * div + diff of channel sdf_channel (fp32 multiply, then add, unfused), frame t of trajectory b;
 *   tgt:  the stored raw frame first[b] + (s + 1) * T + t (clamped into the store) of field field[sdf_channel] (clamped likewise), through
 *         bf_clip_gather's nearest-neighbour map when Ho x Wo < H x W: the grid the model sees.
 * labels may be NULL; otherwise the call also leaves its label images: labels [2 sides][2 halves][B][T][Ho][Wo] int32 is a ring of two steps, side 0
 * the prediction, side 1 the simulation; the call for step s writes bf_bubble_census' label image of frame (b, t) into half s & 1 and touches nothing
 * of the other half, which still holds step s - 1 for bf_rollout_bubble_links.
 * With s outside [0, steps) nothing is written.  ws: bf_bubble_census_ws_bytes(2 * B * T, Ho, Wo, max_bubbles) bytes, 16-byte aligned. */
int bf_rollout_bubbles(const bf_rollout_step* s, int sdf_channel, int connectivity, int max_bubbles, const bf_census_rows* pred,
                       const bf_census_rows* tgt, int32_t* labels, void* ws, int64_t ws_bytes, bf_stream_t stream);
/* Redistancing (reinitialisation) of `frames` signed-distance fields phi [frames][H][W] fp32 in physical units with square cells of size dx
 * (csrc/redistance.hip; the reference has no program for it): out = the signed distance to phi's own zero level set, first order.
 *   sign       a cell is vapour (+) iff phi > 0; an exact zero is liquid (-), bf_bubble_census' convention;
 *   interface  a cell with a 4-neighbour inside the frame of the other sign.  Per such neighbour n the crossing distance is t = dx |phi_c| / (|phi_c| + |phi_n|);
 *              tx = the smaller t over left / right, ty over up / down; d = t with one axis present, 1 / sqrt(1 / tx^2 + 1 / ty^2) with both, 0 if a present
 *              t is 0.  Interface cells are frozen;
 *   the rest   start at +inf and take the fixed point of the Godunov upwind update of |grad d| = 1: a = min(left, right), b = min(up, down) (neighbours
 *              outside the frame are absent), lo = min(a, b), hi = max(a, b); u = lo + dx if hi is absent, infinite or hi - lo >= dx, else
 *              (lo + hi + sqrt(2 dx^2 - (hi - lo)^2)) / 2; with band > 0, u = min(u, band); a value is replaced only by a strictly smaller u.  A pass is two
 *              checkerboard half-passes in place, cells with even x + y first; passes run until one changes no cell;
 *   out        +d on vapour, -d on liquid cells: the signs and the interface cells of phi exactly.  out may be phi.
 *   rounds [frames] int32 (may be NULL)      >= 1: passes executed, the quiet last one included; 0: the frame has one sign throughout and is returned unchanged;
 *              -1: the frame holds a NaN or an inf and is returned unchanged; -2: max_rounds passes ran without a quiet one: the frame holds the values
 *              reached, cells no pass reached hold sign * (band if given, else (H + W) dx).  max_rounds <= 0 means H + W;
 *   change_rms [frames] fp32 (may be NULL)   sqrt(mean (out - phi)^2): differences and the sum in fp64 in a fixed order, one rounding; 0 for an unchanged frame.
 * One workgroup owns a frame; fp32 distances without fused contraction, no float atomics, no race between the cells of a half-pass: the same bits on every
 * call, and a frame has the same bits alone and in a batch.  Allocation-free, capturable, never makes the host wait.  Any H, W >= 1 with H * W <= 2^24
 * (refused beyond, before any launch).  Frames of at most bf_redistance_lds_cells() cells keep the distances in LDS, larger ones in the workspace.
 * ws: bf_redistance_ws_bytes(frames, H, W) bytes (at least 16), 16-byte aligned (0 from the query: sizes out of range). */
int64_t bf_redistance_lds_cells(void);
int64_t bf_redistance_ws_bytes(int64_t frames, int H, int W);
int bf_redistance(const float* phi, int64_t frames, int H, int W, float dx, float band, int max_rounds, float* out, int32_t* rounds, float* change_rms,
                  void* ws, int64_t ws_bytes, bf_stream_t stream);
/* bf_redistance of the signed-distance channel of ONE rollout step's prediction, IN PLACE: issue it before every other call of the step, which then all see the
 * corrected prediction.  s: see bf_rollout_step; pred is the tensor s->pred names, here written.  With the step number s = *s->step in [0, steps) and
 * (s + 1) % every == 0, frame (b, t) of channel sdf_channel is read as pred * div + diff (fp32 multiply, then add, unfused: the physical field the other
 * rollout calls see), redistanced, and written back as (d - diff) / div (bf_clip_gather's expression); row s * T + t of trajectory b of rounds / change_rms
 * [B][steps*T] (each may be NULL) is bf_redistance's status and change of that frame (in physical units).  A frame with status 0 or -1 is not written.
 * One exception to "the signs of the input exactly": the write-back rounds, so a cell whose distance is 0 or within the rounding of diff comes back as a
 * physical value of 0 (liquid to every later call) or, rarely, of the other sign, whichever its sign was; bf_redistance itself has no such case.  On a
 * step in [0, steps) that `every` skips, the call writes rounds = 0 and change_rms = 0 in the step's rows and nothing else; with s outside [0, steps) nothing.
 * ws: bf_redistance_ws_bytes(B * T, Ho, Wo) bytes, 16-byte aligned. */
int bf_rollout_redistance(const bf_rollout_step* s, int sdf_channel, float dx, float band, int max_rounds, int every, float* pred, int32_t* rounds,
                          float* change_rms, void* ws, int64_t ws_bytes, bf_stream_t stream);
/* Bubbles followed from frame to frame (csrc/bubble_tracks.hip; the reference has no program for it).  labels [sequences][T][H][W] and census' count / attached
 * [sequences][T] and area [sequences][T][max_bubbles] (cells is unread and may be NULL) are what bf_bubble_census left for sequences * T frames; a pair is two consecutive frames a, b
 * of one sequence, pair row q = sequence * (T - 1) + t of the link rows for frames t, t + 1.  With ka = min(count_a, max_bubbles), kb likewise (labels above them count
 * as liquid) and overlap[i][j] = the number of cells with La == i and Lb == j, per pair:
 *   successor [pairs][max_bubbles] int32       slot i - 1: the j of the largest overlap[i][j] > 0, ties to the smallest j, 0 if none;
 *   n_successors                               the number of j with overlap[i][j] > 0;
 *   predecessor, n_predecessors                the same per bubble j of b over the bubbles i of a (ties to the smallest i);
 *   departure_area                             area_a[i] when bubble i departs, else 0: i <= attached_a, j = successor[i] > attached_b, predecessor[j] == i;
 *   events [pairs][5] int32                    births (j without predecessor), deaths (i without successor), merges (n_predecessors >= 2),
 *                                              splits (n_successors >= 2), departures.
 * Slots behind ka / kb hold 0.  A pair with a frame whose count is -1 holds -1 in every output.  T == 1 launches nothing.  One workgroup owns a pair;
 * its ka x kb table is in LDS when ka * kb <= bf_bubble_links_lds_entries(), in its slice of the workspace otherwise (a workgroup-uniform branch on the
 * device).  Integer adds only: the same bits on every call, and for a pair alone or in a batch.  Any H, W >= 1 with H * W <= 2^24, max_bubbles <= 2^15.
 * Allocation-free, capturable, never makes the host wait.  ws: bf_bubble_links_ws_bytes(pairs, max_bubbles) bytes, 16-byte aligned, contents
 * irrelevant before and after (0 from the query: sizes out of range). */
int64_t bf_bubble_links_lds_entries(void);
int64_t bf_bubble_links_ws_bytes(int64_t pairs, int max_bubbles);
int bf_bubble_links(const int32_t* labels, const bf_census_rows* census, int64_t sequences, int T, int H, int W, int max_bubbles,
                    const bf_link_rows* links, void* ws, int64_t ws_bytes, bf_stream_t stream);
/* Track ids from the links: bubble j of frame t + 1 continues bubble i of frame t iff predecessor[j] == i and successor[i] == j; every other bubble
 * (every bubble of frame 0, and of the later frame of a pair that holds -1) starts a new track.  Tracks are numbered 1, 2, ... per sequence in order of
 * (frame, bubble number) of their first member.  count [sequences][T]; successor, predecessor [sequences][T - 1][max_bubbles] (unread when T == 1);
 * track_id [sequences][T][max_bubbles] int32, 0 in unused slots; n_tracks [sequences] int32.  One workgroup per sequence walks the frames in order. */
int bf_bubble_track_ids(const int32_t* count, const int32_t* successor, const int32_t* predecessor, int64_t sequences, int T, int max_bubbles,
                        int32_t* track_id, int32_t* n_tracks, bf_stream_t stream);
/* bf_bubble_links for ONE rollout step, both sides in one call, on the ring `labels` the step's bf_rollout_bubbles filled and the census rows it
 * wrote: issue the call after it.  s: see bf_rollout_step (checked, the fields unread).  With the step number s = *s->step, per side and trajectory b the pairs that
 * end in a frame of step s: (t - 1, t) for t = 1 .. T - 1 from half s & 1, and for s > 0 the pair (frame T - 1 of half (s - 1) & 1, frame 0 of
 * half s & 1).  The pair that ends in frame t goes to row s * T + t - 1 of a side's link rows [B][steps*T - 1][max_bubbles] (events:
 * [B][steps*T - 1][5]); no other row is touched, and with s outside [0, steps) nothing is written.  census_*: count / attached [B][steps*T] and area
 * [B][steps*T][max_bubbles]; cells is unread and may be NULL.  steps * T >= 2.  ws: bf_bubble_links_ws_bytes(2 * B * T, max_bubbles) bytes,
 * 16-byte aligned. */
int bf_rollout_bubble_links(const bf_rollout_step* s, int max_bubbles, const int32_t* labels, const bf_census_rows* census_pred,
                            const bf_census_rows* census_tgt, const bf_link_rows* links_pred, const bf_link_rows* links_tgt, void* ws,
                            int64_t ws_bytes, bf_stream_t stream);
/* Predicted bubbles scored against simulated ones, object by object (csrc/bubble_tracks.hip; the reference has no program for it).
 * A pair is a prediction frame P and the simulation frame S of the same time: labels_pred, labels_tgt [frames][H][W] and each census' count / attached
 * [frames] and area [frames][max_bubbles] are what bf_bubble_census left for the two sides (cells is unread and may be NULL).  With kp = min(count_p,
 * max_bubbles), ks likewise (labels above them have no record and count as liquid for the table), overlap[i][j] = the number of cells with Lp == i and
 * Ls == j, best_s[i] = the j of the largest overlap[i][j] > 0 (ties to the smallest j, 0 if none) and best_p[j] the same per simulated bubble over
 * the predicted ones, predicted bubble i and simulated bubble j are MATCHED iff best_s[i] == j, best_p[j] == i and
 *   (double)overlap[i][j] >= (double)min_iou * (double)(area_p[i] + area_s[j] - overlap[i][j])
 * (the union is below 2^24, so the fp64 product is exact and the comparison has one answer everywhere; min_iou = 0 is mutual best overlap alone).
 * Per pair, row = pair:
 *   match_pred [rows][max_bubbles] int32     slot i - 1: the matched j, or 0;
 *   match_target [rows][max_bubbles] int32   slot j - 1: the matched i, or 0;
 *   overlap [rows][max_bubbles] int32        slot i - 1: overlap[i][match], or 0 (the pair's IoU is overlap / (area_p[i] + area_s[j] - overlap));
 *   displacement [rows][max_bubbles] fp32    slot i - 1: the Euclidean distance in cells between the centroids of a matched pair; a centroid is the
 *                                            quotient of exact integer sums of y and x per label (taken by this kernel) by the census area; quotients,
 *                                            differences, squares, their sum and the root in fp64 without fused contraction, one rounding to fp32;
 *                                            0 in unmatched and unused slots;
 *   counts [rows][6] int32                   hits (matched pairs), misses (ks - hits), false alarms (kp - hits); then the same three for bubbles on the
 *                                            heater: a heater hit is a matched pair with i <= attached_p and j <= attached_s, heater misses are
 *                                            min(attached_s, ks) - heater hits, heater false alarms min(attached_p, kp) - heater hits;
 *   mask [rows][2] int32                     the cells that are vapour on both sides, and on either side; any label > 0 counts, also above max_bubbles.
 * Slots behind kp / ks hold 0.  A pair with a frame whose count is -1 holds -1 in every integer output and NaN in displacement.  Every member of
 * rows is required.  One workgroup owns a pair; its kp x ks table is in LDS when kp * ks <= bf_bubble_links_lds_entries(), in its slice of the
 * workspace otherwise (bf_bubble_links' workgroup-uniform branch); the y / x sums are 64-bit integers in the slice.  Integer atomics only: the same bits
 * on every call, and for a pair alone or in a batch.  Any H, W >= 1 with H * W <= 2^24 and max_bubbles <= 2^15 (refused beyond, before any launch);
 * min_iou outside [0, 1] or NaN is refused.  Allocation-free, capturable, never makes the host wait.  ws: bf_bubble_match_ws_bytes(frames,
 * max_bubbles) bytes, 16-byte aligned, contents irrelevant before and after (0 from the query: sizes out of range). */
int64_t bf_bubble_match_ws_bytes(int64_t pairs, int max_bubbles);
int bf_bubble_match(const int32_t* labels_pred, const int32_t* labels_tgt, const bf_census_rows* census_pred, const bf_census_rows* census_tgt,
                    int64_t frames, int H, int W, int max_bubbles, float min_iou, const bf_match_rows* rows, void* ws, int64_t ws_bytes,
                    bf_stream_t stream);
/* bf_bubble_match for ONE rollout step, on the ring `labels` the step's bf_rollout_bubbles filled and the census rows it wrote: issue the call after
 * it.  s: see bf_rollout_step (checked, the fields unread).  With the step number s = *s->step, the pair (side 0, side 1) of frame (b, t) from half
 * s & 1 goes to row s * T + t of rows shaped [B][steps*T][...]; no other row is touched, and with s outside [0, steps) nothing is written.
 * census_*: count / attached [B][steps*T] and area [B][steps*T][max_bubbles]; cells is unread and may be NULL.
 * ws: bf_bubble_match_ws_bytes(B * T, max_bubbles) bytes, 16-byte aligned. */
int bf_rollout_bubble_match(const bf_rollout_step* s, int max_bubbles, float min_iou, const int32_t* labels, const bf_census_rows* census_pred,
                            const bf_census_rows* census_tgt, const bf_match_rows* rows, void* ws, int64_t ws_bytes, bf_stream_t stream);
/* Where a prediction is wrong and at which scales (csrc/spectra.hip; the reference has no program for it).  pred, target
 * [frames][H][W] fp32, e = pred - target in fp64; sdf (optional) [frames][H][W] fp32 in physical units.  Any member of rows may be NULL and is then not computed:
 *   rmse, max_error, boundary_rmse [frames] fp32   sqrt(mean e^2); max |e| (NaN if any e is NaN); the root mean square over the outer ring of cells;
 *   interface_rmse [frames] fp32, interface_cells [frames] int32   the same over the cells whose (2 r + 1)^2 window (r = interface_radius >= 1, clipped to
 *     the frame) holds both vapour (sdf > 0) and liquid (anything else: zero and NaN too), and their number; NaN where there is none.  Both need sdf;
 *   spectrum_error / spectrum_pred / spectrum_target [frames][K] fp32   shell power of e / pred / target: the sum of |X|^2 / (H W)^2 over the modes of
 *     shell q, X the unnormalised 2-D DFT, q the largest integer with q^2 H^2 W^2 <= S^2 (fy^2 W^2 + fx^2 H^2) for the signed frequencies fy, fx and
 *     S = min(H, W) (decided in int64), K = isqrt(S * S / 2) + 1 shells; the K values of a field add up to its mean square;
 *   spectral_error [frames][3] fp32   sqrt of spectrum_error summed over the shells [0, lo), [lo, hi), [hi, K) (lo, hi clipped to K; 0 <= lo <= hi).
 * want_spectra == 0 skips the transforms: the four spectral outputs are then left untouched.  fp64 arithmetic, fixed-order sums, one rounding: the same
 * bits on every call and for a frame alone or in a batch; e == 0 everywhere gives exact zeros.  H, W in [1, 1024].  Allocation-free, capturable, never
 * makes the host wait.  ws: bf_field_errors_ws_bytes(frames, H, W) bytes, 16-byte aligned (0 from the query: sizes out of range). */
int64_t bf_field_errors_ws_bytes(int64_t frames, int H, int W);
int bf_field_errors(const float* pred, const float* target, const float* sdf, int64_t frames, int H, int W, int interface_radius, int lo, int hi,
                    int want_spectra, const bf_error_rows* rows, void* ws, int64_t ws_bytes, bf_stream_t stream);
/* bf_field_errors of ONE rollout step: frame (b, t, c) of the prediction against the stored frame first[b] + (s + 1) * T + t of field[c], read where it
 * lies with the bits bf_clip_gather returns; the interface mask from the raw stored frame of channel sdf_channel (-1: none, the interface rows must be
 * NULL), one mask for all C channels of (b, t).  Rows (b, s * T + t, c) of [B][steps*T][C]([K] or [3]) are written and no other; with the step number s = *s->step outside
 * [0, steps) nothing is written.  s: see bf_rollout_step.  ws: bf_field_errors_ws_bytes(B * T * C, Ho, Wo) bytes, 16-byte aligned. */
int bf_rollout_errors(const bf_rollout_step* s, int sdf_channel, int interface_radius, int lo, int hi, int want_spectra, const bf_error_rows* rows,
                      void* ws, int64_t ws_bytes, bf_stream_t stream);
/* bf_ensemble_scores' outputs: mean_rmse, spread, crps [rows] are required together; rank_hist [rows][members + 1] and mean [rows][H][W] may be NULL
 * and are then not computed */
typedef struct bf_ensemble_rows { float *mean_rmse, *spread, *crps; int32_t* rank_hist; float* mean; } bf_ensemble_rows;
/* The statistics across the M = members members of an ensemble forecast, per frame (csrc/ensemble.hip; the reference has no program for it; DESIGN.md
 * section 23).  members_ptr[m * member_stride + f * H * W + p] fp32 is member m of frame f, target[f * H * W + p] fp32 the truth; 2 <= M <= 32,
 * n = H * W, member_stride >= frames * H * W.  Differences, squares, sums, quotients and roots in fp64 from the fp32 inputs, one rounding to fp32:
 *   mean_rmse [frames]           sqrt(1/n sum_p (xbar_p - y_p)^2), xbar_p the member mean;
 *   spread [frames]              sqrt(1/n sum_p s2_p), s2_p the unbiased member variance, from centred squares (a second pass over the values in registers);
 *   crps [frames]                1/n sum_p [ 1/M sum_m |x_m - y| - w sum_m sum_n |x_m - x_n| ], w = 1 / (2 M^2), or 1 / (2 M (M - 1)) with fair != 0: the
 *                                pairwise form, the two non-negative sums kept apart in fp64 until the last line (a shared offset of the members cancels
 *                                in every difference, not in the sum);
 *   rank_hist [frames][M + 1]    int32: the number of pixels whose truth has exactly r members STRICTLY below it (a member equal to the truth is not below);
 *   mean [frames][H][W]          fp32: xbar_p rounded once.
 * fp64 partials per workgroup added in a fixed order, the counts through integer atomics: the same bits on every call, and for a frame alone or in a
 * batch.  16-byte loads where W % 4 == 0, member_stride % 4 == 0 and the pointers are 16-byte aligned, 4-byte loads otherwise (any alignment of
 * fp32 data works).  Allocation-free, capturable, never makes the host wait.  ws: bf_ensemble_scores_ws_bytes(frames, members, H, W) bytes, 8-byte
 * aligned (0 from the query: sizes out of range). */
int64_t bf_ensemble_scores_ws_bytes(int frames, int members, int H, int W);
int bf_ensemble_scores(const float* members_ptr, int64_t member_stride, const float* target, int frames, int members, int H, int W, int fair,
                       const bf_ensemble_rows* rows, void* ws, int64_t ws_bytes, bf_stream_t stream);
/* bf_ensemble_scores of ONE rollout step.  s: see bf_rollout_step; its B = members * Bt rows are member-major: row m * Bt + b is member m of trajectory
 * b (B % members != 0 is a size error), and first[b] == first[m * Bt + b] (row b's is read).  Frame (b, t, c) is scored against the stored frame
 * first[b] + (s + 1) * T + t of field[c], read where it lies with the bits bf_clip_gather returns.  Rows (b, s * T + t, c) of [Bt][steps*T][C]([M + 1] or
 * [Ho][Wo]) are written and no other; with the step number s = *s->step outside [0, steps) nothing is written.  The counter is read, not advanced: issue the
 * call before the step's bf_rollout_score.  ws: bf_ensemble_scores_ws_bytes(Bt * T * C, members, Ho, Wo) bytes. */
int bf_rollout_ensemble(const bf_rollout_step* s, int members, int fair, const bf_ensemble_rows* rows, void* ws, int64_t ws_bytes, bf_stream_t stream);
/* bf_flow_consistency's outputs */
typedef struct bf_flow_rows {
    float *divergence_rms, *kinetic_energy, *enstrophy; int32_t* bulk_cells;              /* [rows]  per frame */
    float *transport_rms, *interface_speed_rms;         int32_t* transport_cells;         /* [pairs] per pair  */
} bf_flow_rows;   /* any member may be NULL and is then not computed */
/* Do a signed-distance field and a velocity field agree with each other (csrc/flow.hip; the reference has no program for it)?
 * sdf, velx, vely [sequences][T][H][W] fp32 in physical units; x runs along W and y along H, row 0 is the heater row, the spacing is dx on both axes.
 * Vapour is sdf > 0, anything else is liquid, an exact zero and a NaN too (bf_field_errors' convention).  Interior cells are 1 <= i <= H - 2,
 * 1 <= j <= W - 2.  Every input is widened to fp64 before any arithmetic.  Per frame, row = sequence * T + t:
 *   div(i, j) = ((u[i][j+1] - u[i][j-1]) + (v[i+1][j] - v[i-1][j])) / (2 dx),  w(i, j) = ((v[i][j+1] - v[i][j-1]) - (u[i+1][j] - u[i-1][j])) / (2 dx);
 *   bulk_cells [rows] int32      the interior cells whose (2 r + 1)^2 window (r = interface_radius >= 1, clipped to the frame) holds no vapour cell;
 *   divergence_rms [rows]        sqrt(sum over the bulk cells of div^2 / bulk_cells); NaN where there is none;
 *   kinetic_energy [rows]        sum over ALL cells of (u^2 + v^2) / 2, divided by H W;
 *   enstrophy [rows]             sum over the interior cells of w^2 / 2, divided by (H - 2) (W - 2).
 * Per pair of consecutive frames of one sequence (0 the earlier, 1 the later), row = sequence * (T - 1) + t - 1 for the pair that ends in frame t
 * (bf_bubble_links' convention), with pm = (phi0 + phi1) / 2, um = (u0 + u1) / 2, vm = (v0 + v1) / 2 and s = (phi1 - phi0) / dt:
 *   transport_cells [pairs] int32   n = the band cells: the interior cells with |pm| < band;
 *   transport_rms [pairs]           sqrt(sum over the band cells of (s + um dpm/dx + vm dpm/dy)^2 / n), central differences of pm at spacing dx;
 *   interface_speed_rms [pairs]     sqrt(sum over the band cells of s^2 / n); both NaN where n = 0.
 * T = 1 has no pairs and the three pair members are unread.  fp64 arithmetic, every sum in a fixed order (no float atomics), each value rounded once to
 * fp32: the same bits on every call, and for a sequence alone or in a batch; a NaN or an inf that enters a sum makes that row non-finite and no other.
 * One workgroup per frame does the frame's rows and the pair that ends in it.  H, W in [3, 1024], dx, dt, band > 0 (refused otherwise, before any
 * HIP call).  No workspace; allocation-free, capturable, never makes the host wait. */
int bf_flow_consistency(const float* sdf, const float* velx, const float* vely, int64_t sequences, int T, int H, int W, float dx, float dt,
                        float band, int interface_radius, const bf_flow_rows* rows, bf_stream_t stream);
/* bf_flow_consistency of ONE rollout step, of the prediction and of the simulation in one call.  s: see bf_rollout_step.  With the step number
 * s = *s->step (read on the device, never written):
 *   pred:   channels sdf_channel / velx_channel / vely_channel of s->pred as pred * div + diff (fp32 multiply, then add, unfused: the physical fields
 *           bf_rollout_score's Eikonal rows and bf_rollout_heatflux see);
 *   target: the stored raw frames first[b] + (s + 1) * T + t (clamped into the store) of field[channel], through bf_clip_gather's nearest-neighbour map
 *           when Ho x Wo < H x W.
 * The frame rows of (b, t) go to row s * T + t of a side's [B][steps*T], the pair that ends in frame t to row s * T + t - 1 of its [B][steps*T - 1];
 * no other row is touched.  The pair from the last INPUT frame to the first predicted frame is not scored (bf_rollout_bubble_links does the same).
 * The earlier frame of a pair across a step boundary is, for the target, the stored frame first[b] + (s + 1) * T - 1, and for the prediction the
 * carry: carry [2][B][3][Ho][Wo] fp32, which the caller allocates and nothing else reads or writes; half s & 1 receives the physical (phi, u, v) of the
 * step's last predicted frame, half (s - 1) & 1 is read at s >= 1 (two halves: reader and writer are different workgroups of one launch).  With s
 * outside [0, steps) nothing is written, the carry included.  Refused before any HIP call: a null record or carry, a channel outside [0, C), Ho or
 * Wo outside [3, 1024].  Issue the call before the step's bf_rollout_score, and after bf_rollout_redistance if that is used. */
int bf_rollout_flow(const bf_rollout_step* s, int sdf_channel, int velx_channel, int vely_channel, float dx, float dt, float band,
                    int interface_radius, float* carry, const bf_flow_rows* pred, const bf_flow_rows* target, bf_stream_t stream);
/* The stand-alone criterion (utils/losses.py:67-94 for any d and any finite p >= 1; csrc/losses.hip).  pred, y [rows][n] fp32 (rows = product of the
 * leading dims, n = product of the last d), 4-byte aligned; 16-byte loads where pred and y (and dpred) sit at the same offset from a 16-byte boundary.
 * bf_lp_rows_fwd: sums[r] = {S_e = sum |pred - y|^p, S_y = sum |y|^p} in fp64, added in a fixed order (no atomics: the same bits on every call),
 *   ratio[r] = (S_e / S_y)^(1/p), quotient and root in fp64, rounded once (S_y = 0 gives inf or NaN, as the reference's quotient of norms does).
 *   ws: bf_lp_rows_ws_doubles(rows, n) doubles (0 for short rows; may then be NULL).
 * bf_lp_rows_bwd: dpred[r][i] = g[r] * sign(e) |e|^(p-1) / (S_e^((p-1)/p) * S_y^(1/p)), e = pred - y, from the sums the forward left; g [rows] fp32 on
 *   the device.  The row coefficient is fp64 and every element is rounded once.  A row with S_e = 0 gets zeros (torch's norm backward).
 * p = 1, p = 2 and integer p <= 16 take no transcendental per element (fp64 products); any other p takes powf on the fp32 difference. */
int64_t bf_lp_rows_ws_doubles(int64_t rows, int64_t n);
int bf_lp_rows_fwd(const float* pred, const float* y, int64_t rows, int64_t n, double p, float* ratio, double* sums, double* ws, int64_t ws_doubles,
                   bf_stream_t stream);
int bf_lp_rows_bwd(const float* pred, const float* y, const float* g, const double* sums, int64_t rows, int64_t n, double p, float* dpred,
                   bf_stream_t stream);
/* dphi = d/dphi of g[0] * mean over frames x H x W of (|grad phi| - 1)^2 (the adjoint of bf_eikonal_sum's expression divided by the count); g = one fp32
 * in DEVICE memory.  Gather form (no atomics), fp64 arithmetic, one rounding.  A cell with |grad phi| = 0 contributes 0 (autograd of the reference's
 * expression gives 0 * inf = NaN there).  A 1-wide axis has a zero derivative. */
int bf_eikonal_bwd(const float* phi, int64_t frames, int H, int W, float dx, const float* g, float* dphi, bf_stream_t stream);
/* The interface-weighted criterion (no reference program; csrc/losses.hip).  pred, y [frames][C][H][W] fp32 in the dataset's normalised units
 * (frames = B * T in 1 .. 2^20, C in 1 .. 16, H and W in 1 .. 32768), 4-byte aligned; 16-byte loads where H * W is a multiple of 4 and pred, y
 * (and dpred) sit at the same offset from a 16-byte boundary, scalars otherwise.  s in [0, C) is the channel of the signed distance, stored as
 * (phi - diff_s) / div_s (div_s != 0).  With phi_t = y[f][s] * div_s + diff_s:
 *   w[f][i]   = 1 + gain * max(0, 1 - |phi_t[i]| / band)     fp64, from the target alone, one weight for the C fields of a pixel
 *               (gain >= 0 and finite; band > 0 in phi's units where gain > 0, not read where gain = 0)
 *   S_e[f][c] = sum_i w (pred - y)^2,  S_y[f][c] = sum_i w y^2     fp64, added in a fixed order (no atomics: the same bits on every call)
 *   terms[1 + c] = field_weights[c] * mean over f of sqrt(S_e / S_y)     quotient, root and mean in fp64, rounded once
 *   terms[0]  = eikonal * mean over f, i of (|grad (pred[f][s] * div_s + diff_s)| - 1)^2, gradients as torch.gradient(spacing=dx, edge_order=1) in
 *               fp64 on the channel where it lies inside pred (eikonal >= 0; 0 launches nothing for it and leaves terms[0] = 0; dx > 0 otherwise)
 *   loss[0]   = sum_c terms[1 + c] + terms[0], added in fp64, rounded once.
 * field_weights: C fp64 in HOST memory, finite and >= 0, read during the call; NULL = all 1.  loss (1 fp32), terms (1 + C fp32) and sums
 * (2 * frames * C fp64: {S_e, S_y} per row, what bf_wlp_bwd reads) are DEVICE memory, sums and ws 8-byte aligned; ws: bf_wlp_ws_doubles(frames, C, H, W)
 * doubles (-1: sizes out of range).  A row with S_y = 0 gives an inf or NaN ratio (and term, and loss), as the reference's quotient of norms
 * does; a row with S_e = 0 gives the ratio 0.
 * bf_wlp_bwd: dpred[f][c][i] = g[0] * field_weights[c] / frames * w * (pred - y) / sqrt(S_e S_y), the row coefficient in fp64 and every element rounded
 * once; a row with S_e = 0 gets zeros.  With eikonal > 0 a second launch adds g[0] * d terms[0] / d pred to channel s (bf_eikonal_bwd's gather
 * form with the chain factor div_s; a cell with |grad| = 0 contributes 0).  Every element of dpred is written, whatever the options; dpred may
 * not overlap pred or y.  g = one fp32 in DEVICE memory.  The other arguments are those of the forward call that left `sums`.
 * Every check runs before any HIP call. */
int64_t bf_wlp_ws_doubles(int64_t frames, int C, int H, int W);
int bf_wlp_fwd(const float* pred, const float* y, int64_t frames, int C, int H, int W, int s, double diff_s, double div_s, double band, double gain,
               const double* field_weights, double eikonal, double dx, float* loss, float* terms, double* sums, double* ws, int64_t ws_doubles,
               bf_stream_t stream);
int bf_wlp_bwd(const float* pred, const float* y, const float* g, const double* sums, int64_t frames, int C, int H, int W, int s, double diff_s,
               double div_s, double band, double gain, const double* field_weights, double eikonal, double dx, float* dpred, bf_stream_t stream);
/* The shell-weighted spectral criterion (no reference program; csrc/spectral_loss.hip).  pred, y [frames][C][H][W] fp32 in
 * normalised units (frames = B * T in 1 .. 2^20, C in 1 .. 16, H and W in 1 .. 1024), 4-byte aligned, read as scalars.  With X(ky, kx) the
 * unnormalised 2-D DFT, q(ky, kx) the shell of bf_field_errors (signed frequencies folded at H/2, W/2; S = min(H, W); the largest q with
 * q^2 H^2 W^2 <= S^2 (fy^2 W^2 + fx^2 H^2) in int64) and K = isqrt(S^2 / 2) + 1 shells:
 *   S_e[f][c] = sum_k w[c][q(k)] |E_k|^2 / (H W),  E = DFT(pred - y);  S_y the same sum over DFT(y)      fp32 transforms, fp64 sums in a fixed order
 *   terms[c]     = field_weights[c] * mean over f of sqrt(S_e / S_y)       quotient, root and mean in fp64, rounded once
 *   terms[C + c] = the same at w = 1 (the plain relative L2, for monitoring)
 *   loss[0]      = sum_c terms[c], added in fp64, rounded once.
 * shell_weights: the (C, K) table of doubles in DEVICE memory, 8-byte aligned, read by the kernels; shell_weights_host: the same table in HOST
 * memory, read during the call for the checks only (every weight finite and >= 0, no field's row all zero); K must be the shell count of (H, W).
 * Nothing in the library compares the two tables (that would take a copy from the device, and no HIP call precedes the checks): that they hold the
 * same values is the CALLER's duty.  utils.losses.SpectralLpLoss builds both from one host tensor, once per device, and never writes either again.
 * field_weights: C fp64 in HOST memory, finite and >= 0, read during the call; NULL = all 1.  loss (1 fp32), terms (2 C fp32), sums (2 * frames * C
 * fp64: {S_e, S_y} per row) and spec (frames * C * H * (W/2 + 1) * 8 bytes, 8-byte aligned: the filtered half-spectrum of the error, inverse-
 * transformed along y -- with sums, all bf_slp_bwd reads) are DEVICE memory; ws: bf_slp_ws_bytes(frames, C, H, W) bytes, 16-byte aligned
 * (-1: sizes out of range).  A row with S_y = 0 gives an inf or NaN ratio, as the quotient of norms does; a row with S_e = 0 gives the ratio 0.
 * bf_slp_bwd: dpred[f][c] = g[0] * field_weights[c] / frames * Re ifft2(w E) / sqrt(S_e S_y), the row coefficient in fp64, every element
 * written and rounded once; a row with S_e = 0 gets zeros.  g = one fp32 in DEVICE memory; dpred may not overlap spec.  The other arguments
 * are those of the forward call that left `sums` and `spec`.  Every check runs before any HIP call. */
int64_t bf_slp_ws_bytes(int64_t frames, int C, int H, int W);
int bf_slp_fwd(const float* pred, const float* y, int64_t frames, int C, int H, int W, const double* shell_weights, const double* shell_weights_host,
               int K, const double* field_weights, float* loss, float* terms, double* sums, void* spec, void* ws, int64_t ws_bytes, bf_stream_t stream);
int bf_slp_bwd(const void* spec, const float* g, const double* sums, int64_t frames, int C, int H, int W, const double* field_weights, float* dpred,
               bf_stream_t stream);
/* Gradient clipping without a host round trip (csrc/gradclip.hip).
 * bf_grad_norm: out = {norm, coef} (two fp32 in DEVICE memory) of the flat gradient buffer g[n] (fp32, 16-byte aligned, n > 0):
 *   norm = gscale * sqrt(sum g^2)   squares and sums in fp64, rounded once to fp32; gscale = the factor the optimizer applies to g
 *   coef = min(max_norm / (norm + 1e-6), 1)   in fp32, IEEE divide; a NaN norm gives a NaN coefficient
 * i.e. torch.nn.utils.clip_grad_norm_(norm_type=2, error_if_nonfinite=False).  A fixed-order two-pass reduction, no float atomics: the
 * buffer is cut into slabs by a rule that depends on n only, one fp64 partial per slab in ws (at least bf_grad_norm_ws_doubles(n)
 * doubles, 8-byte aligned, at most 1024), which one workgroup then adds in slab order.  Two calls on one buffer give the same bits on
 * any device.  max_norm <= 0 or a null out is an error. */
int64_t bf_grad_norm_ws_doubles(int64_t n);
int bf_grad_norm(const float* g, int64_t n, float gscale, float max_norm, float* out, double* ws, int64_t ws_doubles, bf_stream_t stream);
/* The fused flat-buffer optimizers (csrc/optim_kernels.h, csrc/gradclip.hip; DESIGN.md sections 22 and 24): ONE entry point per optimizer, which
 * takes one step as a record.  The library reads the record DURING the call only and keeps no pointer to it; what the kernel needs is copied by
 * value into its arguments, so the calls stay capturable and a record may live on the caller's stack.  One launch per call.
 * Buffers: p, g, m, v [n] fp32 in DEVICE memory, 16-byte aligned, n > 0; bf_lion has no second moment and ignores v, step and eps; step >= 1 for
 * the Adams (bc1 = 1 - beta1^step, bc2 = 1 - beta2^step).  With G[i] the effective gradient (below):
 *   bf_adamw (torch.optim.AdamW)  p *= 1 - lr*wd; m = beta1*m + (1-beta1)*G; v = beta2*v + (1-beta2)*G^2; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
 *   bf_adam  (torch.optim.Adam, amsgrad = maximize = False)  weight decay is an L2 term on the gradient: G += wd*p (wd != 0), then m, v and p as above
 *   bf_lion  (lion_pytorch.Lion)  p *= 1 - lr*wd; p -= lr*sign(beta1*m + (1-beta1)*G); m = beta2*m + (1-beta2)*G
 * Effective gradient: G[i] = (gscale * coef_dev[0]) * g[i], clamped to [-clip_value, clip_value] before any use (before Adam's L2 term too).
 *   coef_dev = one fp32 in DEVICE memory, e.g. bf_grad_norm's out + 1; NULL = 1.  clip_value > 0; +inf = no clamp; a NaN gradient stays a NaN.
 *   The kernel is chosen by one rule: the clamping body when clip_value is finite, else the body that reads coef_dev when it is not NULL, else the
 *   host-scale body (G = gscale * g[i]).  The three run the same loop: coef_dev[0] == 1.0f and clip_value = +inf give the host-scale body's bits,
 *   which is why coef_dev == NULL with clip_value = +inf launches that body and reads no coefficient.
 * Average (EMA / SWA; no reference program): avg = NULL keeps none and avg_weight is unread.  Otherwise avg [n] fp32, 16-byte aligned,
 *   0 < avg_weight <= 1, and the same launch moves it towards the p[i] it has just formed, whatever the scale mode and the groups:
 *     avg[i] = avg_weight == 1 ? p[i] : fma(avg_weight, p[i] - avg[i], avg[i])      two roundings
 *   so zero padding stays zero and a NaN in p reaches avg; p, m and v come out bit for bit as without it.
 * Parameter groups (freeze, per-group learning-rate scale and weight decay): chunk_group = NULL means none; n_groups and the three tables are then
 *   unread and wd is every element's weight decay.  Otherwise the flat buffer is cut into chunks of BF_OPT_CHUNK consecutive elements
 *   (trainer.FlatParams starts every parameter on a chunk boundary, so a chunk belongs to one parameter); chunk_group[ceil(n / BF_OPT_CHUNK)] (uint8,
 *   DEVICE memory) names each chunk's group, and three tables in DEVICE memory describe the n_groups groups (1 <= n_groups <= BF_OPT_MAX_GROUPS):
 *   group_lr_scale[k] (fp32, >= 0), group_weight_decay[k] (fp32, >= 0, absolute) and group_frozen[k] (uint8).  wd is then unread: every group
 *   brings its own.  An element of group k is stepped with lr * group_lr_scale[k] and group_weight_decay[k] by the same kernel body as without
 *   groups: one group of scale 1 gives those bits.  group_lr_scale[k] == 0 with group_frozen[k] == 0 is torch's lr = 0: the moments move, the
 *   parameter does not.  A chunk of a frozen group is neither read nor written: p, m, v and avg keep their bits and nothing in its gradient (a NaN
 *   included) reaches anything.  The entry points cannot check the map's ids without reading it; the kernels treat an id >= n_groups as frozen.
 * Step guard: live_dev = NULL means none, and the launch is the one made before the member existed.  Otherwise live_dev is
 *   one int32 in DEVICE memory, 4-byte aligned ("<entry>: the guard flag must be 4-byte aligned"), e.g. bf_step_guard's guard[0].  The launch reads
 *   it first.  live_dev[0] == 0: it reads nothing else and writes nothing -- p, m, v and avg keep their bits, in every scale mode, with and without
 *   the average and the groups, whatever g holds.  live_dev[0] != 0: the results are bit for bit those of the same record with live_dev = NULL.
 *   The record grew by this member without a new bf_abi_version: a caller zero-initialises the record and is compiled against this header.
 * A null record or a null required pointer is refused as "<entry>: null pointer", and every other check is made, before any HIP call. */
#define BF_OPT_CHUNK 64
#define BF_OPT_MAX_GROUPS 64
typedef struct bf_opt_step {
    float* p; const float* g; float *m, *v;
    const float* coef_dev; float* avg;
    const uint8_t* chunk_group; const float *group_lr_scale, *group_weight_decay; const uint8_t* group_frozen;
    const int32_t* live_dev;
    int64_t n;
    int32_t step, n_groups;
    float lr, beta1, beta2, eps, wd, gscale, clip_value, avg_weight;
} bf_opt_step;
int bf_adamw(const bf_opt_step* s, bf_stream_t stream);
int bf_adam(const bf_opt_step* s, bf_stream_t stream);
int bf_lion(const bf_opt_step* s, bf_stream_t stream);
/* bf_step_guard: the device decision whether an optimizer step is taken (one tiny launch, no host round trip).  norm = one fp32 in DEVICE memory,
 * out[0] of bf_grad_norm or bf_group_clip_coef; guard = four int32 in DEVICE memory, {live, consecutive, skipped, last_skipped_step}:
 *   live = isfinite(norm[0]);   not live: consecutive += 1, skipped += 1, last_skipped_step = step;   live: consecutive = 0
 * guard + 0 is what bf_opt_step's live_dev takes.  Why the norm is a sufficient witness: it is gscale * sqrt(sum g^2) with the squares and the
 * sum in fp64 over fp32 values.  A finite fp32 square is below 1.2e77, so the sum of n of them cannot overflow fp64 (1.8e308) for any n a
 * buffer can have, and an inf or a NaN element makes the sum inf or NaN, which nothing later removes: with a finite gscale the sum is non-finite
 * exactly when some element is.  The one extra case is the rounding to fp32: a finite gradient whose scaled 2-norm exceeds 3.4e38 has an inf
 * norm and is skipped too.  Elements of frozen groups are outside bf_group_clip_coef's norm and so outside the decision.
 * Both pointers must be 4-byte aligned and not NULL; refused before any HIP call. */
int bf_step_guard(const float* norm, int32_t step, int32_t* guard, bf_stream_t stream);
/* bf_nonfinite_scan: the diagnostic after a skipped step -- out = {index of the first element of x[n] (fp32, 16-byte aligned, n > 0) that is an inf
 * or a NaN, or -1; the number of such elements} (two int64 in DEVICE memory).  bf_grad_norm's slab rule: 16-byte loads, the n % 4 trailing
 * elements joined to the last slab, one {minimum index, count} per slab in ws (at least bf_nonfinite_scan_ws_len(n) int64, 8-byte aligned) and
 * one finishing workgroup; integers only, no atomics, so two calls agree. */
int64_t bf_nonfinite_scan_ws_len(int64_t n);
int bf_nonfinite_scan(const float* x, int64_t n, int64_t* out, int64_t* ws, int64_t ws_len, bf_stream_t stream);
/* bf_weight_average is the optimizers' avg update alone (same bits; w as avg_weight); bf_swap_buffers exchanges two non-overlapping 16-byte
 * aligned buffers exactly, in one launch. */
int bf_weight_average(float* avg, const float* p, int64_t n, float w, bf_stream_t stream);
int bf_swap_buffers(float* a, float* b, int64_t n, bf_stream_t stream);
/* The gradient norm per parameter group (chunk_group and group tables as in bf_opt_step).
 * bf_group_sumsq: sums[k] = sum of x[i]^2 over the elements whose chunk has group k (fp64, n_groups doubles in DEVICE memory), in a fixed
 *   order with no float atomics: the same bits on every call.  ws: at least bf_group_sumsq_ws_doubles(n) doubles, 8-byte aligned.
 * bf_group_clip_coef: from those sums, out = {norm, coef} (two fp32 in DEVICE memory) as bf_grad_norm writes them, with
 *   norm = gscale * sqrt(sum over the groups with frozen[k] == 0 of sums[k]), added in group order -- clip_grad_norm_ over the parameters a
 *   torch optimizer would hold -- and, when group_norm is not NULL, group_norm[k] = gscale * sqrt(sums[k]) for every group (fp32). */
int64_t bf_group_sumsq_ws_doubles(int64_t n);
int bf_group_sumsq(const float* x, int64_t n, const uint8_t* chunk_group, int n_groups, double* sums, double* ws, int64_t ws_doubles,
                   bf_stream_t stream);
int bf_group_clip_coef(const double* sums, const uint8_t* frozen, int n_groups, float gscale, float max_norm, float* out,
                       float* group_norm, bf_stream_t stream);

/* ---------------------------------------------------------------- stage-level entry points (what the nn.Modules call) */

typedef struct bf_dims {
    int32_t dtype;              /* BF_DTYPE_* */
    int32_t B, T, h, w;         /* batch, frames per clip, token grid */
    int32_t E, heads;           /* embed dim, attention heads (d = E / heads) */
    int32_t attn_scale, feat_scale;
    int32_t patch;              /* patch size (power of two) */
    int32_t cin, cout;          /* input / output fields */
    int32_t nfluid;             /* FiLM parameters, 0 = unconditioned AViT */
} bf_dims;

/* Parameters of one AttentionBlock (layers/attention.py:25-64) in state_dict order; the gradient struct mirrors it. */
typedef struct bf_temporal_params {
    float *gamma, *attn_scale_factor, *norm1_w, *norm1_b, *norm2_w, *norm2_b, *input_head_w, *input_head_b,
          *output_head_w, *output_head_b, *qnorm_w, *qnorm_b, *knorm_w, *knorm_b, *rel_pos_emb;
} bf_temporal_params;
/* Parameters of one AxialAttentionBlock (layers/attention.py:137-197) */
typedef struct bf_spatial_params {
    float *gamma_att, *gamma_mlp, *attn_scale_factor_x, *attn_scale_factor_y, *low_freq_scalar, *high_freq_scalar,
          *norm1_w, *norm1_b, *norm2_w, *norm2_b, *input_head_w, *input_head_b, *output_head_w, *output_head_b,
          *qnorm_w, *qnorm_b, *knorm_w, *knorm_b, *rel_pos_emb, *fc1_w, *fc1_b, *fc2_w, *fc2_b, *mlp_norm_w, *mlp_norm_b;
} bf_spatial_params;
/* HMLPEmbed (+ FiLMMLP): up to 5 stages (patch <= 32) */
#define BF_MAX_STAGES 5
typedef struct bf_embed_params {
    float* conv_w[BF_MAX_STAGES];
    float* in_w[BF_MAX_STAGES];
    float* in_b[BF_MAX_STAGES];
    float *film_ln_w, *film_ln_b, *film_w, *film_b;   /* NULL for AViT */
} bf_embed_params;
typedef struct bf_debed_params {
    float* conv_w[BF_MAX_STAGES];
    float* in_w[BF_MAX_STAGES];    /* last stage unused */
    float* in_b[BF_MAX_STAGES];
} bf_debed_params;

/* Bytes of the per-stage activation record the forward fills and the backward reads, and of the transient scratch
 * arena any stage call needs (forward or backward).  Both are plain device allocations owned by the caller. */
int64_t bf_temporal_saved_bytes(const bf_dims* d);
int64_t bf_spatial_saved_bytes(const bf_dims* d);
int64_t bf_embed_saved_bytes(const bf_dims* d);
int64_t bf_debed_saved_bytes(const bf_dims* d);
int64_t bf_scratch_bytes(const bf_dims* d);

/* Parameter preparation (bf16 weight copies, out-projection fold, MLP-branch stochastic-depth table) of n trunk stages in one launch per
 * 12 stages, written into each stage's `saved` record; kinds[i] 0 = temporal (params[i]: bf_temporal_params*), 1 = spatial
 * (bf_spatial_params*); drop_mlp[i]: that spatial stage's MLP-branch factors or NULL.  bf_stage_prepared(1) just before a stage forward
 * tells it to use them instead of launching its own preparation (the flag is consumed by that call).  Returns 1 in fp32 mode. */
int bf_prep_stages(const bf_dims* dims, int n, const int32_t* kinds, const void* const* params, void* const* saved,
                   const float* const* drop_mlp, bf_stream_t stream);
void bf_stage_prepared(int on);
/* Inference forward of n trunk stages in one call (scripts/inference.py:239-252 runs FiLMConditionedAViT.forward under no_grad, one clip
 * at a time; the stages are SpaceTimeBlock's temporal and axial blocks, models/axial_vit.py:18-60).  Nothing is saved for a backward, the
 * InstanceNorms run inside the whole-frame projection kernels (bf_frame_linear) and the bf16 weight copies / out-projection folds live in
 * a caller-owned arena (bf_trunk_eval_weights_bytes) that bf_trunk_eval_prepare fills once per set of weights: call it again after the
 * parameters change.  kinds / params as bf_prep_stages; x, out [N][E]; scratch: bf_scratch_bytes.  No stochastic depth (eval).
 * bf_trunk_eval_prepare / _fwd return 0 when done, 1 when the shape is not covered (bf16, 12 x 12-token frames, E = 384: the caller then
 * runs the stage forwards), < 0 on error. */
int64_t bf_trunk_eval_weights_bytes(const bf_dims* dims, int n, const int32_t* kinds);
int bf_trunk_eval_prepare(const bf_dims* dims, int n, const int32_t* kinds, const void* const* params, void* weights, bf_stream_t stream);
int bf_trunk_eval_fwd(const bf_dims* dims, int n, const int32_t* kinds, const void* const* params, const void* weights, const void* x,
                      void* out, void* scratch, bf_stream_t stream);
/* The n trunk stages of a TRAINING step in one native call per direction (the reference runs them as a Python loop over SpaceTimeBlock,
 * models/axial_vit.py:234-235 -> :58-63): kinds / params as bf_prep_stages; saved[i]: stage i's record (bf_temporal_saved_bytes /
 * bf_spatial_saved_bytes); acts[i]: stage i's output [N][E] (acts[n - 1] is the trunk's output; the backward reads acts[0 .. n - 2] as stage
 * inputs); drop_a[i] / drop_b[i]: the stage's stochastic-depth factors or NULL (the arrays themselves may be NULL).  The forward prepares
 * the weights (bf_prep_stages) and chains every stage's opening InstanceNorm into the launch in front of it.  Backward: grads[i] mirrors
 * params[i] (gradients accumulate); dout = d(acts[n - 1]), dx = d(x); gbuf3: three [N][E] buffers for the gradients between stages;
 * stage_done(i, user) (optional) is called on the host after stage i's backward has been enqueued. */
typedef void (*bf_stage_done_fn)(int stage, void* user);
int bf_trunk_train_fwd(const bf_dims* dims, int n, const int32_t* kinds, const void* const* params, void* const* saved,
                       const float* const* drop_a, const float* const* drop_b, const void* x, void* const* acts, void* scratch, bf_stream_t stream);
int bf_trunk_train_bwd(const bf_dims* dims, int n, const int32_t* kinds, const void* const* params, const void* const* grads, void* const* saved,
                       const float* const* drop_a, const float* const* drop_b, const void* x, void* const* acts, const void* dout,
                       void* const* gbuf3, void* dx, void* scratch, bf_stage_done_fn stage_done, void* user, bf_stream_t stream);
/* x, out, dout, dx: [N][E] activations.  Gradients ACCUMULATE into `g` (zero it first). */
/* Chained stage heads (optional, forward only): arm the NEXT temporal stage's opening InstanceNorm (norm1 of next_p, written into next_saved)
 * to be computed by the tail of the spatial stage called next, whose output it normalises -- one launch and one read of the activation
 * less per block pair; bf_temporal_fwd on next_saved then skips its own norm1.  Results are bit-identical to the unchained calls.
 * NULL arguments disarm.  A spatial stage that cannot chain (fp32 frames longer than the register cache, ...) leaves the norm to the
 * temporal stage as usual. */
int bf_stage_chain_head(const bf_dims* dims, const bf_temporal_params* next_p, void* next_saved);
/* ... in either direction: next_kind 0 = a temporal stage follows (next_params: bf_temporal_params*), 1 = a spatial stage follows
 * (bf_spatial_params*).  The stage forward called next folds that stage's opening InstanceNorm into its last GEMM's launch
 * (bf_gemm_fwd_frames: the temporal stage's out-projection, the spatial stage's fc2 + MLP-branch norm) where the frame-pair kernel covers
 * the shape, or into its last InstanceNorm launch; the stage on next_saved then skips its own norm1.  Bit-identical to the unchained calls. */
int bf_stage_chain_next(const bf_dims* dims, int next_kind, const void* next_params, void* next_saved);
/* The mirror image in the backward: the temporal stage's last kernel produces the output gradient of the spatial stage in front of it (prev_p,
 * prev_saved; has_drop_mlp: its MLP branch carried stochastic-depth factors), whose backward opens with its MLP-branch InstanceNorm -- armed
 * here, that norm's backward is applied by the temporal backward called next (bf_gemm_inbwd_frames_chain) and bf_spatial_bwd on prev_saved
 * skips it.  bf16, 144-token frames, an even number of frames; otherwise nothing changes.  NULL arguments disarm. */
int bf_stage_chain_tail(const bf_spatial_params* prev_p, const void* prev_saved, int has_drop_mlp);
/* Stochastic depth in the backward (optional, deferred-side-work mode): `factors` [frames / fdiv] are what the NEXT stage backward to be called
 * (a temporal stage) multiplies its incoming gradient by -- the gradient the spatial stage backward called next produces.  Armed, that stage's
 * last kernel also writes the scaled copy and the temporal backward, given the same dout and drop pointers, uses it instead of scaling in a
 * launch of its own.  The flag is consumed by the next bf_spatial_bwd; NULL disarms. */
int bf_stage_next_scale(const float* factors, int fdiv);
/* Stochastic depth (timm DropPath at layers/attention.py:123,309,317): `drop*` are the per-sample factors (0 or 1/keep) the
 * caller drew -- [B] for the temporal block (dim 0 = batch), [B*T] each for the two branches of the axial block -- or NULL. */
int bf_temporal_fwd(const bf_dims* d, const bf_temporal_params* p, const void* x, void* out, void* saved, void* scratch,
                    const float* drop, bf_stream_t s);
int bf_temporal_bwd(const bf_dims* d, const bf_temporal_params* p, const bf_temporal_params* g, const void* x, const void* dout,
                    void* dx, void* saved, void* scratch, const float* drop, bf_stream_t s);
int bf_spatial_fwd(const bf_dims* d, const bf_spatial_params* p, const void* x, void* out, void* saved, void* scratch,
                   const float* drop_att, const float* drop_mlp, bf_stream_t s);
int bf_spatial_bwd(const bf_dims* d, const bf_spatial_params* p, const bf_spatial_params* g, const void* x, const void* dout,
                   void* dx, void* saved, void* scratch, const float* drop_att, const float* drop_mlp, bf_stream_t s);
/* x: (B*T, cin, H, W) fp32 clip; fluid: [B][nfluid] fp32 or NULL; out: [N][E].  dx_in (optional): d(loss)/d(clip). */
int bf_embed_fwd(const bf_dims* d, const bf_embed_params* p, const float* x, const float* fluid, void* out, void* saved, void* scratch, bf_stream_t s);
int bf_embed_bwd(const bf_dims* d, const bf_embed_params* p, const bf_embed_params* g, const void* dout, float* dx_in, void* saved,
                 void* scratch, bf_stream_t s);
/* x: [N][E]; pred: (B*T, cout, H, W) fp32.  If target != NULL the relative-L2 loss (utils/losses.py:67-94 as
 * configured at modules.py:50) is fused: loss[0] and the per-(frame, channel) backward coefficients are produced. */
int bf_debed_fwd(const bf_dims* d, const bf_debed_params* p, const void* x, float* pred, const float* target, float* loss,
                 void* saved, void* scratch, bf_stream_t s);
/* dpred: explicit (B*T, cout, H, W) fp32 gradient, or NULL to use the fused loss backward (pred, target, loss_scale[0] or 1); dpred
 * together with (pred, target): the sum of the two, d pred = dpred + loss_scale[0] * d(loss)/d(pred) (see bf_debed_last_bwd). */
int bf_debed_bwd(const bf_dims* d, const bf_debed_params* p, const bf_debed_params* g, const void* x, const float* dpred,
                 const float* pred, const float* target, const float* loss_scale, void* dx, void* saved, void* scratch,
                 bf_stream_t s);

/* ---------------------------------------------------------------------------------------------------- ModernUnet (conv.hip)
 * Replaces, for models/unets.py:67-209 (ModernUnet) and layers/conv_layers.py:5-86 (ResidualBlock, MiddleBlock):
 *   bf_conv_fwd ......... nn.Conv2d 1x1 / 3x3 s1 / 3x3 s2 (unets.py:93,37-62; conv_layers.py:28-29,34) and nn.ConvTranspose2d k4 s2 p1
 *                         (unets.py:10-34, transposed = 1); with transposed = 1 also the data gradient of every conv
 *   bf_conv_wgrad ....... their weight gradients (autograd); bf_conv_colsum their bias gradients
 *   bf_gn_fwd / bf_gn_bwd nn.GroupNorm(8, C) + nn.GELU in front of every conv (conv_layers.py:38-39, unets.py:140,205)
 *   bf_unet_lploss_* .... LpLoss(d=2, p=2, reduce_dims=[0,1,2], reductions=[mean, mean, sum]) (modules.py:50, utils/losses.py:67-94)
 * A bf_conv_src is one activation tensor: element (frame, y, x, c) at ((frame*H + y)*W + x)*C + c (channels-last), or, with nchw = 1,
 * at ((frame*C + c)*H + y)*W + x (the reference's (B, T*C, H, W) clip / prediction).  f32 = 1: fp32 storage, else the call's dtype.
 * Two sources are concatenated along channels (torch.cat((x, s), 1)) without being materialised. */
enum { BF_CONV_PRO_NONE = 0, BF_CONV_PRO_AFFINE_GELU = 1 /* gelu(x*sc[f][c] + sh[f][c]) */, BF_CONV_PRO_GELU = 2 /* gelu(x) */ };
typedef struct bf_conv_src {
    const void* p;
    int32_t C, nchw, f32;
} bf_conv_src;
/* F frames; input Hi x Wi, output Ho x Wo; kernel kh x kw, stride, pad (the forward conv's, also when transposed) */
typedef struct bf_conv_geo {
    int32_t F, Hi, Wi, Ho, Wo, kh, kw, stride, pad;
} bf_conv_geo;
/* out[f][oy][ox][n] = bias[n] + resid + sum_(tap, c) w[tap][c][n] * pro(src(f, iy, ix, c)); w: [kh*kw][C0+C1][N] in the dtype.
 * transposed = 0: iy = oy*stride - pad + ky.  transposed = 1: iy = (oy + pad - ky) / stride where exact (no prologue).
 * The prologue is applied to in-bounds taps only; padding taps are zeros.  sc / sh: [F][C0+C1]. */
int bf_conv_fwd(int dtype, const bf_conv_geo* geo, const bf_conv_src* s0, const bf_conv_src* s1, int pro, const float* sc, const float* sh,
                const void* w, int N, const float* bias, const bf_conv_src* resid, const bf_conv_src* out, int transposed, bf_stream_t stream);
/* dw[r][(ky*kw + kx)*Cs + c] (+)= sum over output pixels m of rows(m, r) * pro(src(m, tap, c)) (forward-mode gather), in fixed-order slabs */
int64_t bf_conv_wgrad_ws_floats(int R, int K, int64_t M);
int bf_conv_wgrad(int dtype, const bf_conv_geo* geo, const bf_conv_src* rows, const bf_conv_src* s0, const bf_conv_src* s1, int pro,
                  const float* sc, const float* sh, float* dw, int accumulate, float* ws, int64_t ws_floats, bf_stream_t stream);
/* out[c] (+)= sum over pixels of src; ws: 64 * C floats */
int bf_conv_colsum(int dtype, const bf_conv_src* src, int F, int H, int W, float* out, int accumulate, float* ws, int64_t ws_floats,
                   bf_stream_t stream);
/* GroupNorm(G) statistics over the concatenation of s0 and s1 (fp64 partial sums, fixed order): mean / rstd [F][G], sc / sh [F][C] */
int64_t bf_gn_ws_floats(int F, int C, int G);
int bf_gn_fwd(int dtype, const bf_conv_src* s0, const bf_conv_src* s1, int F, int H, int W, int G, const float* gamma, const float* beta,
              float eps, float* mean, float* rstd, float* sc, float* sh, float* ws, bf_stream_t stream);
/* dA: [F*H*W][C] fp32 gradient w.r.t. gelu(gn(x)).  dx0 / dx1 (stored, the sources' layouts) = d/dx (+ add[F*H*W][C]); dgamma / dbeta
 * (+)= (accumulate).  gamma = NULL: no norm (the prologue was gelu(x)). */
int bf_gn_bwd(int dtype, const float* dA, const bf_conv_src* s0, const bf_conv_src* s1, int F, int H, int W, int G, const float* gamma,
              const float* mean, const float* rstd, const float* sc, const float* sh, const bf_conv_src* add, const bf_conv_src* dx0,
              const bf_conv_src* dx1, float* dgamma, float* dbeta, int accumulate, float* ws, bf_stream_t stream);
/* pred, target: (B, T, C, HW) fp32; loss[0]; coef: [B*T*C]; ws: 4 * B*T*C floats */
int bf_unet_lploss_fwd(const float* pred, const float* target, int B, int T, int C, int64_t HW, float* loss, float* coef, float* ws,
                       bf_stream_t stream);
/* dpred = dloss[0] * coef[plane] * (pred - target) */
int bf_unet_lploss_bwd(const float* pred, const float* target, const float* coef, const float* dloss, int planes, int64_t HW, float* dpred,
                       bf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------- ClassicUnet (bn.hip)
 * Replaces, for models/unets.py:186-320 (ClassicUnet) and layers/conv_layers.py:96-141 (ClassicUnetBlock), together with conv.hip's
 * bf_conv_fwd / bf_conv_wgrad / bf_conv_colsum (the bias-free 3x3 convs, ConvTranspose2d k2 s2 as the transposed gather, the final 1x1):
 *   bf_bn_fwd / bf_bn_eval nn.BatchNorm2d (conv_layers.py:116,125) in training / eval mode, as the next conv's prologue coefficients
 *   bf_bn_act ............. nn.BatchNorm2d + nn.GELU (conv_layers.py:117,126) materialised, optionally with nn.MaxPool2d(2, 2) (unets.py:209-236)
 *   bf_bn_bwd ............. their backward (autograd)
 * x is channels-last [B*H*W][C] in the dtype; statistics fp32, summed in fp64 in a fixed order (bit-reproducible). */
/* ws floats for bf_bn_fwd / bf_bn_bwd over M = B*H*W pixels */
int64_t bf_bn_ws_floats(int64_t M, int C);
/* batch statistics over all B*HW pixels: mean / rstd [C]; sc = gamma*rstd, sh = beta - mean*sc broadcast to [B][C] (the conv prologue's
 * layout); running_mean / running_var (may be NULL together) <- (1 - momentum)*r + momentum*stat, the variance unbiased by M/(M-1);
 * num_batches_tracked[0] += 1 (may be NULL).  M > 1. */
int bf_bn_fwd(int dtype, const void* x, int B, int64_t HW, int C, const float* gamma, const float* beta, float eps, float momentum,
              float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean, float* rstd, float* sc, float* sh, float* ws,
              bf_stream_t stream);
/* eval: sc = gamma / sqrt(running_var + eps), sh = beta - running_mean*sc, broadcast to [B][C] */
int bf_bn_eval(int B, int C, const float* gamma, const float* beta, float eps, const float* running_mean, const float* running_var, float* sc,
               float* sh, bf_stream_t stream);
/* a = gelu(x*sc[f][c] + sh[f][c]) in the dtype; p != NULL: also p [B][H/2][W/2][C] = 2x2 stride-2 max of the stored a, idx = its
 * row-major window position (0..3; ties to the first, NaN wins) */
int bf_bn_act(int dtype, const void* x, int B, int H, int W, int C, const float* sc, const float* sh, void* a, void* p, uint8_t* idx,
              bf_stream_t stream);
/* g = (dA[m*ldA + offA + c] + dP routed to idx) * gelu'(x*sc + sh), dA fp32 (NULL: none), dP [B][H/2][W/2][C] in the dtype (NULL: none);
 * dx = gamma*rstd*(g - sum(g)/M - xhat*sum(g*xhat)/M) in the dtype; dbeta = sum g, dgamma = sum g*xhat ((+)= with accumulate) */
int bf_bn_bwd(int dtype, const float* dA, int64_t ldA, int offA, const void* dP, const uint8_t* idx, const void* x, int B, int H, int W, int C,
              const float* gamma, const float* mean, const float* rstd, const float* sc, const float* sh, void* dx, float* dgamma, float* dbeta,
              int accumulate, float* ws, bf_stream_t stream);

/* Pictures of fields (plot_bubbleml and the wandb_*_plotter strips of bubbleformer/utils/plot_utils.py), fields in, uint8 RGB out.
 * bf_render_ranges: src (frames, C, H, W) fp32; out[q] = {n, sum, sum of squares, min, max} in fp64 for q = 0 the channel c_sdf, 1 the channel
 * c_temp, 2 the speed sqrt(velx^2 + vely^2) formed in fp64; a quantity with a channel of -1 is skipped (n = 0).  A NaN propagates into the sums,
 * min and max ignore it.  Summed in a fixed order (bit-reproducible, no atomics).  ws: bf_render_ranges_ws_doubles() doubles. */
enum { BF_RENDER_SDF = 0 /* Blues, interface outline */, BF_RENDER_TEMP = 1 /* turbo */, BF_RENDER_SPEED = 2 /* turbo of the speed, arrows */ };
#define BF_RENDER_MAX_TILES 6
typedef struct bf_render_tile {
    const float* a;                 /* the field; BF_RENDER_SPEED: the x velocity */
    const float* b;                 /* BF_RENDER_SPEED: the y velocity */
    const float* mask;              /* BF_RENDER_SPEED: a signed distance whose positive cells carry no arrow, or NULL */
    int64_t frame_stride;           /* floats from one image's field to the next image's (a and b) */
    int64_t slot_stride;            /* floats from one round of slots to the next (a and b) */
    int64_t mask_frame_stride, mask_slot_stride;
    const double* range;            /* {vmin, vmax} on the device */
    int32_t kind;                   /* BF_RENDER_* */
} bf_render_tile;
/* An image is rows x cols slots; slot (r, c) has its tile's top-left pixel at (oy + r * pitch_y, ox + c * pitch_x), the tile is H * scale x
 * W * scale pixels and its colour bar is bar_w pixels wide from bar_dx pixels right of the tile's left edge. */
typedef struct bf_render_geom {
    int32_t H, W, scale, rows, cols, ox, oy, pitch_x, pitch_y, bar_dx, bar_w, img_h, img_w, stride;
    double stroke;                  /* half-width of an arrow stroke in pixels */
} bf_render_geom;
int64_t bf_render_ranges_ws_doubles(void);
int bf_render_ranges(const float* src, int64_t frames, int C, int H, int W, int c_sdf, int c_temp, int c_velx, int c_vely, double* out, double* ws,
                     bf_stream_t stream);
/* out (images, img_h, img_w, 3) uint8, img_w a multiple of 4.  Slot k = r * cols + c of image f is drawn from description k % ntiles at
 * a + f * frame_stride + (k / ntiles) * slot_stride: a 2 x 3 panel has six descriptions, a strip one.  Tile pixel (py, px) shows field cell
 * (H - 1 - py / scale, px / scale).  Colour: idx = clamp(floor(256 (x - vmin) / (vmax - vmin)), 0, 255) in fp64 into the 256 x 3 table (NaN: white;
 * vmax == vmin: 0).  SDF tiles: black on the 3 x 3 dilation of the liquid cells (sdf < 0) that have an in-range 4-neighbour which is not liquid.
 * Speed tiles: white within `stroke` pixels of an arrow (shaft and two head strokes) anchored at the cells i % stride == j % stride == stride / 2.
 * The bar shows the table from vmin (bottom) to vmax (top); everything else is white. */
int bf_render_tiles(const bf_render_tile* tiles, int ntiles, const bf_render_geom* geom, int64_t images, const uint8_t* lut_blues,
                    const uint8_t* lut_turbo, uint8_t* out, bf_stream_t stream);

/* Optional per-launch HIP-event timing on the launch stream (bench.py's roofline leg); off by default. */
void bf_prof_enable(int on);
int bf_prof_report(char* buf, int n);   /* JSON {kernel: {calls, ms, flops, bytes}}; bytes written or -1 */

const char* bf_last_error(void);
/* 3.  The number changes when a declaration of this header changes or is removed (a caller built against the older header would pass garbage without
 * any error); a declaration that is only added leaves it as it is. */
int bf_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
