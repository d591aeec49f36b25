"""ctypes binding of libbubbleformer_hip.so (the C ABI declared in include/bubbleformer_hip.h).

There is NO fallback: if the library is missing, or a call fails, this raises.  PyTorch is used only for
device memory (caching allocator), streams and autograd plumbing; every pointer handed to the library is a
raw device address.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbubbleformer_hip.so")
CSRC = os.path.join(_HERE, "csrc")

BF_DTYPE_F32, BF_DTYPE_BF16 = 0, 1
BF_LAY_KC, BF_LAY_XC = 0, 1
BF_PRO_NONE, BF_PRO_AFFINE, BF_PRO_AFFINE_GELU, BF_PRO_GELU = 0, 1, 2, 3
BF_AUX_NONE, BF_AUX_ADD, BF_AUX_DGELU = 0, 1, 2
BF_OUT_STORE, BF_OUT_STORE_F32, BF_OUT_ATOMIC_F32 = 0, 1, 2
BF_MAX_STAGES = 5
BF_LOSS_LIMBS = 5          # int64 limbs per relative-L2 partial sum (include/bubbleformer_hip.h)
BF_OPT_CHUNK, BF_OPT_MAX_GROUPS = 64, 64      # elements per parameter-group chunk, groups per step (include/bubbleformer_hip.h)

vp, fp, i32, i64, f32 = C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_float


class Operand(C.Structure):
    _fields_ = [("p", vp), ("ld", i64), ("layout", i32), ("seglen", i32), ("segstride", i64), ("gw", i32), ("gh", i32),
                ("gc", i32), ("pro", i32), ("sc", fp), ("sh", fp), ("rows_per_frame", i32), ("nch", i32)]


class Epilogue(C.Structure):
    _fields_ = [("bias", fp), ("colscale", fp), ("colshift", fp), ("aux_mode", i32), ("aux", vp), ("ld_aux", i64),
                ("out_mode", i32), ("c", vp), ("ldc", i64), ("seglen", i32), ("segstride", i64), ("gw", i32), ("gh", i32),
                ("gc", i32), ("gelu_out", vp), ("colsum", fp), ("rowscale", fp), ("rows_per_group", i32)]


class Dims(C.Structure):
    _fields_ = [(n, i32) for n in ("dtype", "B", "T", "h", "w", "E", "heads", "attn_scale", "feat_scale", "patch", "cin",
                                   "cout", "nfluid")]


TEMPORAL_FIELDS = ("gamma", "attn_scale_factor", "norm1_w", "norm1_b", "norm2_w", "norm2_b", "input_head_w", "input_head_b",
                   "output_head_w", "output_head_b", "qnorm_w", "qnorm_b", "knorm_w", "knorm_b", "rel_pos_emb")
SPATIAL_FIELDS = ("gamma_att", "gamma_mlp", "attn_scale_factor_x", "attn_scale_factor_y", "low_freq_scalar",
                  "high_freq_scalar", "norm1_w", "norm1_b", "norm2_w", "norm2_b", "input_head_w", "input_head_b",
                  "output_head_w", "output_head_b", "qnorm_w", "qnorm_b", "knorm_w", "knorm_b", "rel_pos_emb", "fc1_w", "fc1_b",
                  "fc2_w", "fc2_b", "mlp_norm_w", "mlp_norm_b")


class TemporalParams(C.Structure):
    _fields_ = [(n, fp) for n in TEMPORAL_FIELDS]


class SpatialParams(C.Structure):
    _fields_ = [(n, fp) for n in SPATIAL_FIELDS]


class FrameNorm(C.Structure):
    """bf_frame_norm: an InstanceNorm folded into a frame-pair GEMM launch (bf_gemm_fwd_frames)."""
    _fields_ = [("w", fp), ("b", fp), ("g", fp), ("gdiv", i32), ("mean", fp), ("rstd", fp), ("sc", fp), ("sh", fp), ("resid", vp), ("out", vp)]


class EmbedParams(C.Structure):
    _fields_ = [("conv_w", fp * BF_MAX_STAGES), ("in_w", fp * BF_MAX_STAGES), ("in_b", fp * BF_MAX_STAGES), ("film_ln_w", fp),
                ("film_ln_b", fp), ("film_w", fp), ("film_b", fp)]


class DebedParams(C.Structure):
    _fields_ = [("conv_w", fp * BF_MAX_STAGES), ("in_w", fp * BF_MAX_STAGES), ("in_b", fp * BF_MAX_STAGES)]


class ConvSrc(C.Structure):
    """bf_conv_src: one activation tensor of a ModernUnet conv / GroupNorm call (channels-last, or NCHW with nchw = 1)."""
    _fields_ = [("p", vp), ("C", i32), ("nchw", i32), ("f32", i32)]


class ConvGeo(C.Structure):
    _fields_ = [(n, i32) for n in ("F", "Hi", "Wi", "Ho", "Wo", "kh", "kw", "stride", "pad")]


BF_CONV_PRO_NONE, BF_CONV_PRO_AFFINE_GELU, BF_CONV_PRO_GELU = 0, 1, 2


class RolloutStep(C.Structure):
    """bf_rollout_step: one rollout step's prediction, store, counters and field table (read during the call only)."""
    _fields_ = [("pred", fp), ("frames", fp), ("field_stride", i64), ("total_frames", i64), ("first", vp), ("step", vp), ("field", vp), ("diff", fp),
                ("div", fp)] + [(n, i32) for n in ("nfields", "B", "T", "C", "H", "W", "Ho", "Wo", "steps", "reserved")]


class CensusRows(C.Structure):
    _fields_ = [(n, vp) for n in ("count", "cells", "attached", "area")]


class LinkRows(C.Structure):
    _fields_ = [(n, vp) for n in ("successor", "n_successors", "predecessor", "n_predecessors", "departure_area", "events")]


class MatchRows(C.Structure):
    """bf_match_rows: bf_bubble_match's six outputs, all required."""
    _fields_ = [(n, vp) for n in ("match_pred", "match_target", "overlap", "displacement", "counts", "mask")]


class ErrorRows(C.Structure):
    _fields_ = [(n, vp) for n in ("rmse", "max_error", "boundary_rmse", "interface_rmse", "interface_cells", "spectral_error", "spectrum_error",
                                  "spectrum_pred", "spectrum_target")]


class EnsembleRows(C.Structure):
    """bf_ensemble_rows: mean_rmse, spread and crps are required together; rank_hist and mean may be NULL."""
    _fields_ = [(n, vp) for n in ("mean_rmse", "spread", "crps", "rank_hist", "mean")]


class FlowRows(C.Structure):
    """bf_flow_rows: four per-frame rows, then three per-pair rows; any may be NULL and is then not computed."""
    _fields_ = [(n, vp) for n in ("divergence_rms", "kinetic_energy", "enstrophy", "bulk_cells", "transport_rms", "interface_speed_rms",
                                  "transport_cells")]


class OptStep(C.Structure):
    """bf_opt_step: one fused optimizer step -- buffers, clip coefficient, average, parameter groups, guard flag, sizes, scalars (read during the call only)."""
    _fields_ = [("p", fp), ("g", fp), ("m", fp), ("v", fp), ("coef_dev", fp), ("avg", fp), ("chunk_group", vp), ("group_lr_scale", fp),
                ("group_weight_decay", fp), ("group_frozen", vp), ("live_dev", vp), ("n", i64), ("step", i32), ("n_groups", i32)] + [
        (n, f32) for n in ("lr", "beta1", "beta2", "eps", "wd", "gscale", "clip_value", "avg_weight")]


class ClipGatherJob(C.Structure):
    """bf_clip_gather_job: what bf_clip_gather_unroll takes, as a record (bf_clip_gather_augment; read during the call only)."""
    _fields_ = [("src", fp), ("idx", vp), ("first_tab", vp), ("in_field", vp), ("in_diff", fp), ("in_div", fp), ("in_out", fp), ("out_field", vp),
                ("out_diff", fp), ("out_div", fp), ("out_out", fp), ("fluid_tab", fp), ("file_tab", vp), ("fluid_out", fp), ("field_stride", i64),
                ("nframes", i64), ("nsamples", i64)] + [(n, i32) for n in ("Cin", "Tin", "Cout", "Tout", "unroll", "P", "B", "H", "W", "Ho", "Wo", "reserved")]


class ClipAugment(C.Structure):
    """bf_clip_augment: the seeded mirror / window draw of bf_clip_gather_augment (seed and draw as signed bit patterns)."""
    _fields_ = [("in_odd", vp), ("out_odd", vp), ("seed", i64), ("flip_thr", i64)] + [(n, i32) for n in ("draw", "Hc", "Wc", "crop_y", "eval_view", "reserved")]


class ClipGatherQ16Job(C.Structure):
    """bf_clip_gather_q16_job: the 16-bit store's codes and segment tables, then bf_clip_gather_job's members (read during the call only)."""
    _fields_ = [("codes", vp), ("frame_seg", vp), ("seg_lo", fp), ("seg_step", fp), ("idx", vp), ("first_tab", vp), ("in_field", vp), ("in_diff", fp),
                ("in_div", fp), ("in_out", fp), ("out_field", vp), ("out_diff", fp), ("out_div", fp), ("out_out", fp), ("fluid_tab", fp), ("file_tab", vp),
                ("fluid_out", fp), ("field_stride", i64), ("nframes", i64), ("nsamples", i64)] + [
        (n, i32) for n in ("nfiles", "Cin", "Tin", "Cout", "Tout", "unroll", "P", "B", "H", "W", "Ho", "Wo")]


class RenderTile(C.Structure):
    """bf_render_tile: what one slot of an image shows (bf_render_tiles)."""
    _fields_ = [("a", fp), ("b", fp), ("mask", fp), ("frame_stride", i64), ("slot_stride", i64), ("mask_frame_stride", i64), ("mask_slot_stride", i64),
                ("range", vp), ("kind", i32)]


class RenderGeom(C.Structure):
    _fields_ = [(n, i32) for n in ("H", "W", "scale", "rows", "cols", "ox", "oy", "pitch_x", "pitch_y", "bar_dx", "bar_w", "img_h", "img_w", "stride")] + [
        ("stroke", C.c_double)]


BF_RENDER_SDF, BF_RENDER_TEMP, BF_RENDER_SPEED = 0, 1, 2
BF_RENDER_MAX_TILES = 6

STAGE_DONE_FN = C.CFUNCTYPE(None, C.c_int, C.c_void_p)      # bf_stage_done_fn
P = C.POINTER
# name -> (restype, argtypes); mirrors include/bubbleformer_hip.h one to one
SIGNATURES = {
    "bf_last_error": (C.c_char_p, []),
    "bf_abi_version": (C.c_int, []),
    "bf_prof_enable": (None, [C.c_int]),
    "bf_debug_force_generic_attn": (None, [C.c_int]),
    "bf_debug_tokred_fold": (None, [C.c_int]),
    "bf_side_defer": (None, [C.c_int]),
    "bf_prep_stages": (C.c_int, [C.POINTER(Dims), C.c_int, C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp]),
    "bf_stage_prepared": (None, [C.c_int]),
    "bf_trunk_train_fwd": (C.c_int, [C.POINTER(Dims), C.c_int, C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp,
                                     C.POINTER(vp), vp, vp]),
    "bf_trunk_train_bwd": (C.c_int, [C.POINTER(Dims), C.c_int, C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                     C.POINTER(vp), vp, C.POINTER(vp), vp, C.POINTER(vp), vp, vp, vp, vp, vp]),
    "bf_field_stats_ws_doubles": (i64, [C.c_int]),
    "bf_field_stats": (C.c_int, [fp, vp, vp, C.c_int, vp, vp, vp]),
    "bf_stage_chain_next": (C.c_int, [C.POINTER(Dims), C.c_int, vp, vp]),
    "bf_stage_next_scale": (C.c_int, [fp, C.c_int]),
    "bf_gemm_fwd_frames": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, vp, i64, vp, i64, fp, fp, fp, fp, C.c_int, vp, vp, C.c_int,
                                     C.POINTER(FrameNorm), C.POINTER(FrameNorm), vp]),
    "bf_trunk_eval_weights_bytes": (i64, [C.POINTER(Dims), C.c_int, C.POINTER(C.c_int32)]),
    "bf_trunk_eval_prepare": (C.c_int, [C.POINTER(Dims), C.c_int, C.POINTER(C.c_int32), C.POINTER(vp), vp, vp]),
    "bf_trunk_eval_fwd": (C.c_int, [C.POINTER(Dims), C.c_int, C.POINTER(C.c_int32), C.POINTER(vp), vp, vp, vp, vp, vp]),
    "bf_frame_linear": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, i64, vp, i64, fp, fp, fp, fp, fp, vp, i64, C.c_int, fp, fp, fp,
                                  vp, i64, fp, fp, vp, i64, vp]),
    "bf_side_join": (C.c_int, [vp]),
    "bf_prof_report": (C.c_int, [C.c_char_p, C.c_int]),
    "bf_gemm": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, P(Operand), P(Operand), P(Epilogue), C.c_int, vp]),
    "bf_gemm_tokred": (C.c_int, [C.c_int, C.c_int, C.c_int, i64, vp, i64, vp, i64, fp, C.c_int, fp, fp, i64, vp]),
    "bf_gemm_tokred_ws_floats": (i64, [C.c_int, C.c_int, i64]),
    "bf_gemm_inbwd_frames": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, vp, i64, vp, i64, vp, vp, vp, C.c_int, fp, fp, fp, fp, fp, C.c_int, vp]),
    "bf_gemm_inbwd_frames_chain": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, vp, i64, vp, i64, vp, vp, vp, C.c_int, fp, fp, fp, fp, fp, C.c_int,
                                             vp, vp, fp, fp, fp, fp, C.c_int, fp, vp]),
    "bf_in_stats": (C.c_int, [C.c_int, vp, C.c_int, C.c_int, C.c_int, fp, fp, fp, C.c_int, fp, fp, fp, fp, fp, fp, vp]),
    "bf_in_ws_floats": (i64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "bf_affine_apply": (C.c_int, [C.c_int, vp, vp, fp, fp, vp, i64, C.c_int, C.c_int, vp]),
    "bf_in_bwd": (C.c_int, [C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, fp, fp, fp, fp, fp, C.c_int, C.c_int, fp, fp,
                            fp, fp, fp, vp]),
    "bf_colsum": (C.c_int, [C.c_int, vp, i64, C.c_int, fp, fp, vp]),
    "bf_attn_axial_fwd": (C.c_int, [C.c_int, vp, vp, i64, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, fp, fp, fp, fp, fp, vp]),
    "bf_attn_axial_norm_fwd": (C.c_int, [C.c_int, vp, vp, vp, i64, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp,
                                         fp, vp]),
    "bf_attn_fwd": (C.c_int, [C.c_int, vp, vp, i64, C.c_int, i64, i64, i64, i64, C.c_int, C.c_int, fp, fp, fp, fp, fp, fp, f32,
                              C.c_int, vp]),
    "bf_attn_bwd": (C.c_int, [C.c_int, vp, vp, vp, i64, C.c_int, i64, i64, i64, i64, C.c_int, C.c_int, fp, fp, fp, fp, fp, fp,
                              fp, fp, fp, fp, fp, fp, f32, C.c_int, fp, i64, vp]),
    "bf_im2col_nchw": (C.c_int, [C.c_int, fp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "bf_col2im_nchw": (C.c_int, [C.c_int, vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "bf_pm2nchw": (C.c_int, [fp, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "bf_debed_last_bwd": (C.c_int, [C.c_int, fp, fp, fp, fp, fp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "bf_debed_last_bwd_norm": (C.c_int, [C.c_int, fp, fp, fp, fp, fp, vp, vp, vp, fp, fp, fp, fp, vp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, fp, C.c_int64, vp]),
    "bf_gather_gemm": (C.c_int, [C.c_int, vp, vp, C.c_int, fp, fp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "bf_scatter_gemm": (C.c_int, [C.c_int, vp, vp, C.c_int, fp, fp, vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "bf_gather_wgrad_ws_floats": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "bf_gather_wgrad": (C.c_int, [C.c_int, vp, vp, fp, fp, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp, C.c_int64, vp]),
    "bf_gather_gemm_rebuilt": (C.c_int, [C.c_int, vp, vp, vp, C.c_int, fp, fp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "bf_gather_wgrad_rebuilt": (C.c_int, [C.c_int, vp, vp, vp, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp, C.c_int64, vp]),
    "bf_stage_chain_head": (C.c_int, [vp, vp, vp]),
    "bf_stage_chain_tail": (C.c_int, [vp, vp, C.c_int]),
    "bf_embed_tail_ws_floats": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bf_embed_tail_bwd": (C.c_int, [C.c_int, vp, vp, vp, vp, vp, fp, fp, fp, fp, fp, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    fp, C.c_int64, vp]),
    "bf_embed_first": (C.c_int, [C.c_int, fp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp, vp]),
    "bf_in_stats_merge_slices": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, fp, C.c_int, fp, fp, fp, fp, fp, fp, vp]),
    "bf_debed_last": (C.c_int, [C.c_int, vp, fp, fp, vp, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "bf_lploss_finalize": (C.c_int, [fp, C.c_int, C.c_int, fp, fp, vp]),
    "bf_nchw2pm": (C.c_int, [C.c_int, fp, fp, fp, fp, fp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "bf_wprep": (C.c_int, [C.c_int, C.c_int, fp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "bf_wgrad_unprep": (C.c_int, [C.c_int, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "bf_film_net_fwd": (C.c_int, [fp, fp, fp, fp, fp, fp, fp, fp, C.c_int, C.c_int, C.c_int, vp]),
    "bf_film_net_bwd": (C.c_int, [fp, fp, fp, fp, fp, fp, fp, fp, fp, C.c_int, C.c_int, C.c_int, vp]),
    "bf_adamw": (C.c_int, [P(OptStep), vp]),
    "bf_adam": (C.c_int, [P(OptStep), vp]),
    "bf_lion": (C.c_int, [P(OptStep), vp]),
    "bf_grad_norm_ws_doubles": (i64, [i64]),
    "bf_grad_norm": (C.c_int, [fp, i64, f32, f32, fp, vp, i64, vp]),
    "bf_weight_average": (C.c_int, [fp, fp, i64, f32, vp]),
    "bf_swap_buffers": (C.c_int, [fp, fp, i64, vp]),
    "bf_group_sumsq_ws_doubles": (i64, [i64]),
    "bf_group_sumsq": (C.c_int, [fp, i64, vp, C.c_int, vp, vp, i64, vp]),
    "bf_group_clip_coef": (C.c_int, [vp, vp, C.c_int, f32, f32, fp, fp, vp]),
    "bf_step_guard": (C.c_int, [fp, i32, vp, vp]),
    "bf_nonfinite_scan_ws_len": (i64, [i64]),
    "bf_nonfinite_scan": (C.c_int, [fp, i64, vp, vp, i64, vp]),
    "bf_eikonal_sum": (C.c_int, [fp, i64, C.c_int, C.c_int, f32, vp, vp]),
    "bf_eikonal_l1_frames": (C.c_int, [fp, i64, C.c_int, C.c_int, f32, fp, vp]),
    "bf_heatflux_rows": (C.c_int, [fp, fp, i64, i64, C.c_int, f32, f32, f32, f32, fp, vp]),
    "bf_clip_gather": (C.c_int, [fp, i64, vp, vp, C.c_int, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "bf_clip_gather_batch": (C.c_int, [fp, i64, vp, i64, vp, vp, fp, fp, C.c_int, C.c_int, fp, vp, fp, fp, C.c_int, C.c_int, fp, fp, vp, C.c_int, fp,
                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "bf_clip_gather_unroll": (C.c_int, [fp, i64, i64, vp, i64, vp, vp, fp, fp, C.c_int, C.c_int, fp, vp, fp, fp, C.c_int, C.c_int, C.c_int, fp, fp, vp, C.c_int,
                                        fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "bf_clip_gather_augment": (C.c_int, [P(ClipGatherJob), P(ClipAugment), vp]),
    "bf_clip_encode_q16": (C.c_int, [fp, vp, i64, f32, f32, vp]),
    "bf_clip_decode_q16": (C.c_int, [vp, i64, vp, fp, fp, fp, i64, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "bf_clip_gather_q16": (C.c_int, [P(ClipGatherQ16Job), P(ClipAugment), vp]),
    "bf_clip_noise": (C.c_int, [fp, fp, fp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "bf_rollout_score_ws_doubles": (i64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bf_rollout_score": (C.c_int, [P(RolloutStep), C.c_int, f32, fp, fp, fp, fp, fp, fp, vp, i64, vp]),
    "bf_rollout_heatflux": (C.c_int, [P(RolloutStep), C.c_int, C.c_int, fp, f32, f32, f32, f32, fp, fp, vp]),
    "bf_kde_kl_ws_doubles": (i64, [C.c_int, i64, i64, C.c_int]),
    "bf_kde_kl": (C.c_int, [vp, vp, C.c_int, i64, i64, C.c_int, C.c_double, vp, vp, vp, vp, vp, i64, vp]),
    "bf_bubble_census_lds_cells": (i64, []),
    "bf_bubble_census_ws_bytes": (i64, [i64, C.c_int, C.c_int, C.c_int]),
    "bf_bubble_census": (C.c_int, [fp, i64, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, fp, vp, vp, vp, i64, vp]),
    "bf_rollout_bubbles": (C.c_int, [P(RolloutStep), C.c_int, C.c_int, C.c_int, P(CensusRows), P(CensusRows), vp, vp, i64, vp]),
    "bf_redistance_lds_cells": (i64, []),
    "bf_redistance_ws_bytes": (i64, [i64, C.c_int, C.c_int]),
    "bf_redistance": (C.c_int, [fp, i64, C.c_int, C.c_int, f32, f32, C.c_int, fp, vp, fp, vp, i64, vp]),
    "bf_rollout_redistance": (C.c_int, [P(RolloutStep), C.c_int, f32, f32, C.c_int, C.c_int, fp, vp, fp, vp, i64, vp]),
    "bf_bubble_links_lds_entries": (i64, []),
    "bf_bubble_links_ws_bytes": (i64, [i64, C.c_int]),
    "bf_bubble_links": (C.c_int, [vp, P(CensusRows), i64, C.c_int, C.c_int, C.c_int, C.c_int, P(LinkRows), vp, i64, vp]),
    "bf_bubble_track_ids": (C.c_int, [vp, vp, vp, i64, C.c_int, C.c_int, vp, vp, vp]),
    "bf_rollout_bubble_links": (C.c_int, [P(RolloutStep), C.c_int, vp, P(CensusRows), P(CensusRows), P(LinkRows), P(LinkRows), vp, i64, vp]),
    "bf_bubble_match_ws_bytes": (i64, [i64, C.c_int]),
    "bf_bubble_match": (C.c_int, [vp, vp, P(CensusRows), P(CensusRows), i64, C.c_int, C.c_int, C.c_int, C.c_float, P(MatchRows), vp, i64, vp]),
    "bf_rollout_bubble_match": (C.c_int, [P(RolloutStep), C.c_int, C.c_float, vp, P(CensusRows), P(CensusRows), P(MatchRows), vp, i64, vp]),
    "bf_field_errors_ws_bytes": (i64, [i64, C.c_int, C.c_int]),
    "bf_field_errors": (C.c_int, [fp, fp, fp, i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P(ErrorRows), vp, i64, vp]),
    "bf_rollout_errors": (C.c_int, [P(RolloutStep), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P(ErrorRows), vp, i64, vp]),
    "bf_ensemble_scores_ws_bytes": (i64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "bf_ensemble_scores": (C.c_int, [fp, i64, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P(EnsembleRows), vp, i64, vp]),
    "bf_rollout_ensemble": (C.c_int, [P(RolloutStep), C.c_int, C.c_int, P(EnsembleRows), vp, i64, vp]),
    "bf_flow_consistency": (C.c_int, [fp, fp, fp, i64, C.c_int, C.c_int, C.c_int, f32, f32, f32, C.c_int, P(FlowRows), vp]),
    "bf_rollout_flow": (C.c_int, [P(RolloutStep), C.c_int, C.c_int, C.c_int, f32, f32, f32, C.c_int, fp, P(FlowRows), P(FlowRows), vp]),
    "bf_render_ranges_ws_doubles": (i64, []),
    "bf_render_ranges": (C.c_int, [fp, i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "bf_render_tiles": (C.c_int, [P(RenderTile), C.c_int, P(RenderGeom), i64, vp, vp, vp, vp]),
    "bf_lp_rows_ws_doubles": (i64, [i64, i64]),
    "bf_lp_rows_fwd": (C.c_int, [fp, fp, i64, i64, C.c_double, fp, vp, vp, i64, vp]),
    "bf_lp_rows_bwd": (C.c_int, [fp, fp, fp, vp, i64, i64, C.c_double, fp, vp]),
    "bf_eikonal_bwd": (C.c_int, [fp, i64, C.c_int, C.c_int, f32, fp, fp, vp]),
    "bf_wlp_ws_doubles": (i64, [i64, C.c_int, C.c_int, C.c_int]),
    "bf_wlp_fwd": (C.c_int, [fp, fp, i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, P(C.c_double), C.c_double,
                             C.c_double, fp, fp, vp, vp, i64, vp]),
    "bf_wlp_bwd": (C.c_int, [fp, fp, fp, vp, i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, P(C.c_double),
                             C.c_double, C.c_double, fp, vp]),
    "bf_slp_ws_bytes": (i64, [i64, C.c_int, C.c_int, C.c_int]),
    "bf_slp_fwd": (C.c_int, [fp, fp, i64, C.c_int, C.c_int, C.c_int, vp, P(C.c_double), C.c_int, P(C.c_double), fp, fp, vp, vp, vp, i64, vp]),
    "bf_slp_bwd": (C.c_int, [vp, fp, vp, i64, C.c_int, C.c_int, C.c_int, P(C.c_double), fp, vp]),
    "bf_temporal_saved_bytes": (i64, [P(Dims)]),
    "bf_spatial_saved_bytes": (i64, [P(Dims)]),
    "bf_embed_saved_bytes": (i64, [P(Dims)]),
    "bf_debed_saved_bytes": (i64, [P(Dims)]),
    "bf_scratch_bytes": (i64, [P(Dims)]),
    "bf_temporal_fwd": (C.c_int, [P(Dims), P(TemporalParams), vp, vp, vp, vp, fp, vp]),
    "bf_temporal_bwd": (C.c_int, [P(Dims), P(TemporalParams), P(TemporalParams), vp, vp, vp, vp, vp, fp, vp]),
    "bf_spatial_fwd": (C.c_int, [P(Dims), P(SpatialParams), vp, vp, vp, vp, fp, fp, vp]),
    "bf_spatial_bwd": (C.c_int, [P(Dims), P(SpatialParams), P(SpatialParams), vp, vp, vp, vp, vp, fp, fp, vp]),
    "bf_embed_fwd": (C.c_int, [P(Dims), P(EmbedParams), fp, fp, vp, vp, vp, vp]),
    "bf_embed_bwd": (C.c_int, [P(Dims), P(EmbedParams), P(EmbedParams), vp, fp, vp, vp, vp]),
    "bf_debed_fwd": (C.c_int, [P(Dims), P(DebedParams), vp, fp, fp, fp, vp, vp, vp]),
    "bf_debed_bwd": (C.c_int, [P(Dims), P(DebedParams), P(DebedParams), vp, fp, fp, fp, fp, vp, vp, vp, vp]),
    "bf_conv_fwd": (C.c_int, [C.c_int, P(ConvGeo), P(ConvSrc), P(ConvSrc), C.c_int, fp, fp, vp, C.c_int, fp, P(ConvSrc), P(ConvSrc),
                              C.c_int, vp]),
    "bf_conv_wgrad_ws_floats": (i64, [C.c_int, C.c_int, i64]),
    "bf_conv_wgrad": (C.c_int, [C.c_int, P(ConvGeo), P(ConvSrc), P(ConvSrc), P(ConvSrc), C.c_int, fp, fp, fp, C.c_int, fp, i64, vp]),
    "bf_conv_colsum": (C.c_int, [C.c_int, P(ConvSrc), C.c_int, C.c_int, C.c_int, fp, C.c_int, fp, i64, vp]),
    "bf_gn_ws_floats": (i64, [C.c_int, C.c_int, C.c_int]),
    "bf_gn_fwd": (C.c_int, [C.c_int, P(ConvSrc), P(ConvSrc), C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, f32, fp, fp, fp, fp, fp, vp]),
    "bf_gn_bwd": (C.c_int, [C.c_int, fp, P(ConvSrc), P(ConvSrc), C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, fp, fp, fp, P(ConvSrc), P(ConvSrc),
                            P(ConvSrc), fp, fp, C.c_int, fp, vp]),
    "bf_unet_lploss_fwd": (C.c_int, [fp, fp, C.c_int, C.c_int, C.c_int, i64, fp, fp, fp, vp]),
    "bf_unet_lploss_bwd": (C.c_int, [fp, fp, fp, fp, C.c_int, i64, fp, vp]),
    "bf_bn_ws_floats": (i64, [i64, C.c_int]),
    "bf_bn_fwd": (C.c_int, [C.c_int, vp, C.c_int, i64, C.c_int, fp, fp, f32, f32, fp, fp, vp, fp, fp, fp, fp, fp, vp]),
    "bf_bn_eval": (C.c_int, [C.c_int, C.c_int, fp, fp, f32, fp, fp, fp, fp, vp]),
    "bf_bn_act": (C.c_int, [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, vp, vp, vp, vp]),
    "bf_bn_bwd": (C.c_int, [C.c_int, fp, i64, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, fp, fp, fp, vp, fp, fp, C.c_int,
                            fp, vp]),
}

_lib = None


class BubbleformerHipError(RuntimeError):
    pass


def build(verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    res = subprocess.run(["make", "-j8", "-C", CSRC], capture_output=True, text=True)
    if verbose or res.returncode:
        print(res.stdout[-4000:])
        print(res.stderr[-4000:])
    if res.returncode:
        raise BubbleformerHipError("building libbubbleformer_hip.so failed")
    return LIB_PATH


def lib():
    """Load the native library (once).  Raises if it has not been built -- there is no CPU path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BubbleformerHipError(
                f"{LIB_PATH} is missing: build it with `make -C {CSRC}` (or __graft_entry__.build()). "
                "bubbleformer_amd has no CPU / eager fallback.")
        # PyTorch-ROCm ships its own libamdhip64; make sure THAT runtime instance is the one this library binds to
        # (two HIP runtimes in one process do not share devices, streams or allocations).
        import torch  # noqa: F401
        tl = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(tl):
            C.CDLL(tl, mode=C.RTLD_GLOBAL)
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)          # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = h
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().bf_last_error().decode(errors="replace")
        if rc == 1 and not msg.startswith("declined"):      # a refusal that left no text of its own (the last-error text may be stale)
            msg = "declined: the entry point does not cover this shape / dtype / workspace (nothing was launched)"
        raise BubbleformerHipError(f"{what} failed (code {rc}): {msg}")
