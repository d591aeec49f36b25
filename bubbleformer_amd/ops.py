"""autograd bindings of the stage-level HIP entry points.

Activations between stages are token-major tensors of shape (B, T, h, w, E) (contiguous) in the compute dtype
(torch.float32 = exact-fp32 parity mode, torch.bfloat16 = throughput mode).  The reference's logical layout
(B, T, E, h, w) is a zero-copy ``permute`` of that memory (see ``as_reference_layout`` / ``as_tokens``).

Parameters stay ordinary fp32 ``nn.Parameter``s owned by the modules; every Function returns one gradient per
parameter so autograd accumulation hooks (and therefore DDP bucket hooks) fire per stage during backward.
"""
import collections
import ctypes as C
import os
from typing import List, Optional, Sequence

import torch

from . import _lib as L

_SCRATCH = {}


def _require_gpu(t: torch.Tensor) -> None:
    if not t.is_cuda:
        raise L.BubbleformerHipError(
            "bubbleformer_amd runs only on a ROCm GPU (gfx950): got a tensor on %s; there is no CPU fallback" % t.device)


def _dt(t: torch.dtype) -> int:
    if t == torch.float32:
        return L.BF_DTYPE_F32
    if t == torch.bfloat16:
        return L.BF_DTYPE_BF16
    raise L.BubbleformerHipError(f"unsupported compute dtype {t}")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def make_dims(dtype, B, T, h, w, E, heads, attn_scale=True, feat_scale=True, patch=0, cin=0, cout=0, nfluid=0) -> L.Dims:
    return L.Dims(_dt(dtype), B, T, h, w, E, heads, int(bool(attn_scale)), int(bool(feat_scale)), patch, cin, cout, nfluid)


def _dims_key(d: L.Dims):
    return tuple(getattr(d, n) for n, _ in L.Dims._fields_)


_SCRATCH_BYTES = {}


_SCRATCH_PINNED: list = []      # arenas a HIP-graph capture has seen: a captured graph holds their raw addresses, so they are never freed


def scratch_for(d: L.Dims, device) -> torch.Tensor:
    """The transient arena of the current stream on `device`, grown to the largest problem seen on that stream (a ragged last batch or
    a validation batch do not pin further arenas): stage calls are stream-ordered and a stage never keeps scratch contents across
    calls, so every shape can share it.  One arena per (device, stream): two streams of one device never share scratch, whatever
    their host threads do (BF_SCRATCH_SHARED=1 opts into ONE arena per device for callers that order their streams themselves).
    An arena that was handed out while its stream was being captured into a HIP graph is pinned: the graph's kernels hold its raw
    address, so a later, larger problem gets a NEW arena and the captured one stays alive until clear_scratch()."""
    key = _dims_key(d)
    n = _SCRATCH_BYTES.get(key)
    if n is None:
        n = L.lib().bf_scratch_bytes(C.byref(d))
        if n < 0:
            L.check(-1, "bf_scratch_bytes")
        _SCRATCH_BYTES[key] = n
    slot = str(device) if os.environ.get("BF_SCRATCH_SHARED") == "1" else (str(device), _stream())
    capturing = torch.cuda.is_current_stream_capturing()
    buf = _SCRATCH.get(slot)
    if buf is None or buf.numel() < n:
        if buf is not None and not capturing:       # the library's side stream may still read the old arena: order it before the arena can be recycled
            L.check(L.lib().bf_side_join(_stream()), "bf_side_join")
        buf = torch.empty(n, dtype=torch.uint8, device=device)
        _SCRATCH[slot] = buf
    if capturing and not any(b is buf for b in _SCRATCH_PINNED):
        _SCRATCH_PINNED.append(buf)
    return buf


def clear_scratch() -> None:
    """Release the scratch arenas, the pinned ones included (after the work -- and every captured graph -- that used them is gone)."""
    if _SCRATCH:
        L.check(L.lib().bf_side_join(_stream()), "bf_side_join")
    _SCRATCH.clear()
    _SCRATCH_PINNED.clear()


def _saved(nbytes: int, device, what: str) -> torch.Tensor:
    if nbytes < 0:
        L.check(-1, what)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _f32c(p: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if p is None:
        return None
    _require_gpu(p)
    if p.dtype != torch.float32:
        raise L.BubbleformerHipError("parameters must be fp32 (master weights); got %s" % p.dtype)
    return p if p.is_contiguous() else p.contiguous()


def _grad_views(params: Sequence[Optional[torch.Tensor]]):
    """One zeroed flat fp32 buffer for a stage's parameter gradients, and per-parameter views into it."""
    total = sum(((p.numel() + 3) // 4) * 4 for p in params if p is not None)
    dev = next(p.device for p in params if p is not None)
    flat = torch.zeros(total, dtype=torch.float32, device=dev)
    views, off = [], 0
    for p in params:
        if p is None:
            views.append(None)
            continue
        views.append(flat[off:off + p.numel()].view(p.shape))
        off += ((p.numel() + 3) // 4) * 4
    return flat, views


# "direct gradient" mode (used by trainer.TrainStep): when every parameter of a stage has a registered fp32 gradient
# slot (a view into the flat gradient buffer), the kernels accumulate straight into it and autograd gets None -- no
# per-parameter temporaries, no 500 tiny accumulate kernels per step.  `on_ready` tells the bucket reducer that a
# stage's gradients are enqueued on the current stream.  Outside this mode gradients are returned to autograd as usual
# (so DDP / optimizer hooks of an unmodified training script still fire).
_DIRECT = {"slots": None, "on_ready": None, "on_join": None}


def set_direct_grad_slots(slots, on_ready=None, on_join=None) -> None:
    """slots: {param.data_ptr(): fp32 gradient view} or None to switch the mode off.  on_join(): called when everything the stages so
    far put on the library's side stream has been ordered on the current stream (see _joined)."""
    _DIRECT["slots"] = slots
    _DIRECT["on_ready"] = on_ready
    _DIRECT["on_join"] = on_join


# Deferred weight-gradient work (bf_side_defer): a trunk stage's side-stream GEMMs may still read its saved activations and its
# incoming gradient while the NEXT stage runs, so those tensors are kept alive for two more stage calls (the library orders the
# side work before the end of the next stage; the caching allocator knows nothing about the library's side stream).
_DEFER = {"on": False, "keep": collections.deque(maxlen=2)}


def set_side_defer(on: bool) -> None:
    """on: opt in (TrainStep does, around forward + backward).  off: join the side stream on the current stream and drop the kept tensors."""
    h = L.lib()
    h.bf_side_defer(1 if on else 0)
    _DEFER["on"] = bool(on)
    if not on:
        L.check(h.bf_side_join(_stream()), "bf_side_join")
        _DEFER["keep"].clear()


def release_deferred() -> None:
    """Deferred mode, between two backward passes inside one set_side_defer(True) window (a training step unrolled through several passes):
    order what the stages put on the side stream before the current stream's next work and drop the tensors kept alive for it, so that a
    finished pass's saved activations go back to the allocator before the next pass runs instead of at the end of the window."""
    if _DEFER["on"]:
        L.check(L.lib().bf_side_join(_stream()), "bf_side_join")
        _DEFER["keep"].clear()


def _joined() -> None:
    """Deferred mode, before the patch-embedding backward (the last, long stage of a backward pass): join the side stream here, on
    the Python side, so that the gradient buckets of the processor blocks can be handed to the all-reduce BEFORE that stage's kernels
    are enqueued and travel under them, instead of after."""
    if _DEFER["on"]:
        L.check(L.lib().bf_side_join(_stream()), "bf_side_join")
        if _DIRECT["on_join"] is not None:
            _DIRECT["on_join"]()


def _stage_grads(params: Sequence[Optional[torch.Tensor]]):
    """-> (gradient tensors the kernels accumulate into, what to hand back to autograd)"""
    slots = _DIRECT["slots"]
    if slots is not None:
        gs = [None if p is None else slots.get(p.data_ptr()) for p in params]
        if all((p is None) == (g is None) for p, g in zip(params, gs)):
            return gs, [None] * len(params), True
    _, views = _grad_views(params)
    return views, views, False


def _stage_done(params, direct: bool) -> None:
    if not direct:      # gradients go back through autograd on this stream: nothing of the stage may still be in flight on the side stream
        L.check(L.lib().bf_side_join(_stream()), "bf_side_join")
    if direct and _DIRECT["on_ready"] is not None:
        _DIRECT["on_ready"]([p.data_ptr() for p in params if p is not None])


def as_tokens(x: torch.Tensor) -> torch.Tensor:
    """(..., E, h, w) reference layout -> (..., h, w, E) token-major contiguous (zero-copy when x is already a
    permuted view of token-major memory)."""
    nd = x.dim()
    return x.permute(*range(nd - 3), nd - 2, nd - 1, nd - 3).contiguous()


def as_reference_layout(tok: torch.Tensor) -> torch.Tensor:
    """(..., h, w, E) token-major -> logical (..., E, h, w) view (no copy)."""
    nd = tok.dim()
    return tok.permute(*range(nd - 3), nd - 1, nd - 3, nd - 2)


# ------------------------------------------------------------------------------------------------ processor blocks
# What one per-stage forward call leaves for the next (the Python mirror of the library's per-device record).  Everything here holds tensors of
# the pass in flight, so clear() -- called when a forward ends, see discard_prepared -- drops all of it:
#   prepared        (kind, pointer of the stage's first parameter) -> (dims key, saved record with prepared weights, drop_mlp, params struct)
#   next            key of the stage announced by chain_next
#   last_spatial    (output pointer, (shape, dtype), params struct, saved, has drop_mlp, params) of the spatial stage just run
#   last_temporal   (output pointer, stochastic-depth factors, T) of the temporal stage just run: the spatial stage behind it remembers them
class _StageLinks:
    def __init__(self):
        self.clear()

    def clear(self) -> None:
        self.prepared = {}
        self.next = self.last_spatial = self.last_temporal = None


_LINKS = _StageLinks()


def chain_next(params, kind: str = "temporal") -> None:
    """Announce the stage (`kind`, its parameters in ``_lib.TEMPORAL_FIELDS`` / ``SPATIAL_FIELDS`` order) that will consume the output of the
    stage called next: when both were prepared by `prepare_stages` for the same shape, that stage's opening InstanceNorm is computed by the
    last launch of the stage in front of it (bf_stage_chain_next: the temporal stage's out-projection, the spatial stage's fc2 + MLP-branch
    norm; bit-identical results, one launch and one read of the activation less)."""
    on = _LINKS.prepared and os.environ.get("BF_STAGE_CHAIN", "1") != "0"
    _LINKS.next = _stage_key(kind, [_f32c(p) for p in params]) if on else None


def _stage_key(kind: str, params) -> tuple:
    return kind, next(p.data_ptr() for p in params if p is not None)


def prepare_stages(tok: torch.Tensor, heads: int, attn_scale: bool, feat_scale: bool, stages) -> None:
    """Parameter preparation of all trunk stages of one forward in one launch per 12 stages (bf_prep_stages) instead of one launch
    inside every stage.  stages: [(kind, params, drop_mlp or None)] in call order; each stage's `saved` record is allocated here and
    handed to the stage's forward, which must follow with the same tok shape / dtype.  bf16 on the GPU only; otherwise a no-op."""
    _LINKS.prepared = {}
    if not tok.is_cuda or tok.dtype != torch.bfloat16 or not stages or os.environ.get("BF_PREP_AHEAD", "1") == "0":
        return
    B, T, h, w, E = tok.shape
    d = make_dims(tok.dtype, B, T, h, w, E, heads, attn_scale, feat_scale)
    keys = {"temporal": _dims_key(make_dims(tok.dtype, B, T, h, w, E, heads, attn_scale, True)), "spatial": _dims_key(d)}
    lib = L.lib()
    n = len(stages)
    nb = {"temporal": lib.bf_temporal_saved_bytes(C.byref(d)), "spatial": lib.bf_spatial_saved_bytes(C.byref(d))}
    kinds = (C.c_int32 * n)()
    pp, sp, dp = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
    keep = []
    for i, (kind, params, drop_mlp) in enumerate(stages):
        params = [_f32c(p) for p in params]
        st = (L.TemporalParams if kind == "temporal" else L.SpatialParams)(*[_p(p) for p in params])
        saved = _saved(nb[kind], tok.device, f"bf_{kind}_saved_bytes")
        if drop_mlp is not None:
            drop_mlp = drop_mlp.contiguous().float()
        keep.append((st, params, drop_mlp))
        kinds[i] = 0 if kind == "temporal" else 1
        pp[i], sp[i], dp[i] = C.addressof(st), _p(saved), _p(drop_mlp)
        _LINKS.prepared[_stage_key(kind, params)] = (keys[kind], saved, drop_mlp, st)
    rc = lib.bf_prep_stages(C.byref(d), n, kinds, pp, sp, dp, _stream())
    if rc != 0:
        _LINKS.prepared = {}
        L.check(min(rc, 0), "bf_prep_stages")


def discard_prepared() -> None:
    """End of a forward: drop the prepared records no stage consumed and what the last per-stage calls remembered of each other."""
    _LINKS.clear()


# ------------------------------------------------------------------------------------------------ inference forward of the trunk
_EVAL_ARENAS: dict = {}     # (device, parameter pointers, dims) -> [weights stamp, arena]: bf16 weight copies + out-projection folds
_WEIGHTS_EPOCH = [0]        # bumped by this package's own in-place optimizer kernels (they write parameters behind torch's version counters)


def _weights_changed() -> None:
    _WEIGHTS_EPOCH[0] += 1


def _evict_eval_arenas(limit: int = 8) -> None:
    """Least recently used first; entries a captured graph reads are kept."""
    for k in list(_EVAL_ARENAS):
        if len(_EVAL_ARENAS) < limit:
            break
        if not _EVAL_ARENAS[k][2]:
            del _EVAL_ARENAS[k]


def refresh_eval_weights(owner: int) -> None:
    """Re-prepare, in place and on the current stream, the inference weights of every cache entry of `owner` whose parameters changed
    since they were prepared (torch version counters / this package's optimizer epoch).  utils.rollout.GraphedForward calls it before
    each replay: a captured graph contains only bf_trunk_eval_fwd reading the arena, so without it a graph kept across optimizer
    steps would replay with the weights of capture time."""
    for key, ent in _EVAL_ARENAS.items():
        if key[0] != int(owner) or ent[3] is None:
            continue
        d, n, kinds, pp, _structs, plist = ent[3]
        flat = [p for ps in plist for p in ps if p is not None]
        stamp = (_WEIGHTS_EPOCH[0], tuple(p._version for p in flat))
        if stamp != ent[0]:
            L.check(L.lib().bf_trunk_eval_prepare(C.byref(d), n, kinds, pp, _p(ent[1]), _stream()), "bf_trunk_eval_prepare")
            ent[0] = stamp


def clear_eval_weights() -> None:
    """Drop the prepared inference weights (they are re-made on the next eval forward).  Needed only after parameters were rewritten
    through raw pointers by code outside this package; torch in-place ops and ops.adamw_ / ops.adam_ / ops.lion_ are noticed by themselves."""
    _EVAL_ARENAS.clear()


def trunk_eval_applies(tok: torch.Tensor) -> bool:
    """Whether ops.trunk_eval is the path for this token tensor: bf16 on the GPU, 12 x 12-token frames, E = 384, not switched off, and at most
    BF_TRUNK_EVAL_MAX_FRAMES frames (default 96).  The whole-frame kernels are built for few frames: measured eval forward, 16x192x192 clips,
    batch 1 / 2 / 4 / 8 / 16: 2.23 / 1.83 / 2.76 / 4.67 / 8.97 ms against 3.20 / 2.37 / 3.02 / 4.09 / 7.71 ms for the stage forwards (eager) --
    from 128 frames on the streaming GEMMs of the training-shaped forward win (one workgroup per CU pays its prologue and epilogue serially)."""
    ok = (tok.is_cuda and tok.dtype == torch.bfloat16 and tok.dim() == 5 and tok.shape[2] * tok.shape[3] == 144 and tok.shape[4] == 384
          and tok.shape[2] <= 16 and tok.shape[3] <= 16 and tok.shape[1] <= 32 and os.environ.get("BF_TRUNK_EVAL", "1") != "0"
          and tok.shape[0] * tok.shape[1] <= int(os.environ.get("BF_TRUNK_EVAL_MAX_FRAMES", "96")))
    if (not ok and tok.is_cuda and tok.dtype == torch.bfloat16 and tok.dim() == 5 and tok.shape[0] * tok.shape[1] <= 96
            and os.environ.get("BF_TRUNK_EVAL", "1") != "0" and not _SLOW_EVAL_WARNED):
        # few frames but not the shape the whole-frame kernels are built for (144-token frames, E = 384): say so once instead of silently
        # running the training-shaped stage forwards (about 1.6x slower per rollout step at batch 1)
        _SLOW_EVAL_WARNED.append(True)
        import warnings
        warnings.warn("bubbleformer_amd: eval forward of a %s token tensor takes the stage-by-stage path; the whole-frame inference kernels "
                      "cover 144-token frames with embed_dim 384 only" % (tuple(tok.shape),), RuntimeWarning, stacklevel=3)
    return ok


_SLOW_EVAL_WARNED: list = []


def _stage_param_shapes(kind: str, E: int, heads: int) -> dict:
    """Element counts the native stage reads from each parameter (layers/attention.py:35-63, 149-197): a shorter tensor would be read
    out of bounds on the GPU."""
    d = E // heads
    base = {"gamma": E, "gamma_att": E, "gamma_mlp": E, "attn_scale_factor": heads, "attn_scale_factor_x": heads, "attn_scale_factor_y": heads,
            "low_freq_scalar": E, "high_freq_scalar": E, "norm1_w": E, "norm1_b": E, "norm2_w": E, "norm2_b": E, "mlp_norm_w": E, "mlp_norm_b": E,
            "input_head_w": 3 * E * E, "input_head_b": 3 * E, "output_head_w": E * E, "output_head_b": E, "qnorm_w": d, "qnorm_b": d,
            "knorm_w": d, "knorm_b": d, "rel_pos_emb": 32 * heads, "fc1_w": 4 * E * E, "fc1_b": 4 * E, "fc2_w": 4 * E * E, "fc2_b": E}
    return base


def _check_stage_params(kind: str, params, E: int, heads: int, device) -> None:
    fields = L.TEMPORAL_FIELDS if kind == "temporal" else L.SPATIAL_FIELDS
    if len(params) != len(fields):
        raise L.BubbleformerHipError(f"{kind} stage: expected {len(fields)} parameters, got {len(params)}")
    want = _stage_param_shapes(kind, E, heads)
    for name, p in zip(fields, params):
        if p is None:
            continue
        if p.device != device:
            raise L.BubbleformerHipError(f"{kind} stage: parameter {name} is on {p.device}, the tokens on {device}")
        if name in want and p.numel() != want[name]:
            raise L.BubbleformerHipError(f"{kind} stage: parameter {name} has {p.numel()} elements, the kernels read {want[name]}")


_EVAL_TOKENS = [0]


def new_eval_token() -> int:
    """A process-unique id for one owner of prepared inference weights (a model instance).  The prepared-weights cache is keyed by it:
    parameter ADDRESSES alone would let a new model that the allocator placed where a freed one lived, with equal version counters,
    find the old model's weights."""
    _EVAL_TOKENS[0] += 1
    return _EVAL_TOKENS[0]


def trunk_eval(tok: torch.Tensor, heads: int, attn_scale: bool, feat_scale: bool, stages, owner: int = 0) -> Optional[torch.Tensor]:
    """Eval forward of all trunk stages in ONE native call (bf_trunk_eval_fwd: whole-frame projection kernels with the InstanceNorms
    inside, nothing saved for a backward).  stages: [(kind, params)] in call order.  The bf16 weight copies and out-projection folds
    are prepared once per set of weights (torch version counters + this package's optimizer epoch) and kept per model.
    Returns None when the path does not apply (not bf16 on the GPU, shape not covered, BF_TRUNK_EVAL=0): the caller then runs the
    stage forwards.  Under HIP-graph capture the preparation must already have happened (utils/rollout.py warms up first).
    owner: ops.new_eval_token() of the caller that owns these parameters (models pass theirs); 0 = keyed by parameter addresses only."""
    if not tok.is_cuda or tok.dtype != torch.bfloat16 or not stages or os.environ.get("BF_TRUNK_EVAL", "1") == "0":
        return None
    tok = tok.contiguous()
    if tok.dim() != 5:
        raise L.BubbleformerHipError("trunk_eval: tokens must be (B, T, h, w, E)")
    B, T, h, w, E = tok.shape
    if heads < 1 or E % heads:
        raise L.BubbleformerHipError(f"trunk_eval: embed dim {E} is not a multiple of {heads} heads")
    d = make_dims(tok.dtype, B, T, h, w, E, heads, attn_scale, feat_scale)
    lib = L.lib()
    n = len(stages)
    kinds = (C.c_int32 * n)(*[0 if kind == "temporal" else 1 for kind, _ in stages])
    plist = [[_f32c(p) for p in params] for _, params in stages]
    for (kind, _), ps in zip(stages, plist):
        _check_stage_params(kind, ps, E, heads, tok.device)
    structs = [(L.TemporalParams if kind == "temporal" else L.SpatialParams)(*[_p(p) for p in ps]) for (kind, _), ps in zip(stages, plist)]
    pp = (C.c_void_p * n)(*[C.addressof(s) for s in structs])
    flat = [p for ps in plist for p in ps if p is not None]
    key = (int(owner), str(tok.device), tuple(p.data_ptr() for p in flat), h, w, E, heads, bool(attn_scale), bool(feat_scale))
    stamp = (_WEIGHTS_EPOCH[0], tuple(p._version for p in flat))
    ent = _EVAL_ARENAS.get(key)
    capturing = torch.cuda.is_current_stream_capturing()
    if ent is None or ent[0] != stamp:
        if capturing and ent is None:
            raise L.BubbleformerHipError("trunk_eval: run one eval forward before capturing it in a HIP graph (the weights are prepared on the first call)")
        nbytes = lib.bf_trunk_eval_weights_bytes(C.byref(d), n, kinds)
        arena = ent[1] if ent is not None else _saved(nbytes, tok.device, "bf_trunk_eval_weights_bytes")
        # re-preparing inside a capture puts the launch INTO the graph (same arena): every replay then re-reads the live parameters
        rc = lib.bf_trunk_eval_prepare(C.byref(d), n, kinds, pp, _p(arena), _stream())
        if rc == 1:
            return None
        L.check(rc, "bf_trunk_eval_prepare")
        if ent is None:
            _evict_eval_arenas()
            ent = _EVAL_ARENAS[key] = [stamp, arena, False, None]
        else:
            ent[0] = stamp
    if capturing:
        ent[2] = True         # a captured graph reads this arena by address: never evicted, refreshed in place (refresh_eval_weights)
    ent[3] = (d, n, kinds, pp, structs, plist)      # what a refresh needs (keeps the parameter tensors and ctypes records alive)
    _EVAL_ARENAS[key] = _EVAL_ARENAS.pop(key)       # most recently used last
    out = torch.empty_like(tok)
    rc = lib.bf_trunk_eval_fwd(C.byref(d), n, kinds, pp, _p(ent[1]), _p(tok), _p(out), _p(scratch_for(d, tok.device)), _stream())
    if rc == 1:
        return None
    L.check(rc, "bf_trunk_eval_fwd")
    return out


class _BlockFn(torch.autograd.Function):
    """Shared driver for the temporal and the axial block."""

    @staticmethod
    def forward(ctx, x, kind, heads, attn_scale, feat_scale, drop_a, drop_b, *params):
        # drop_a / drop_b: per-sample stochastic-depth factors (0 or 1/keep) or None
        _require_gpu(x)
        x = x.contiguous()
        B, T, h, w, E = x.shape
        d = make_dims(x.dtype, B, T, h, w, E, heads, attn_scale, feat_scale)
        lib = L.lib()
        params = [_f32c(p) for p in params]
        drop_a = None if drop_a is None else drop_a.contiguous().float()
        drop_b = None if drop_b is None else drop_b.contiguous().float()
        pre = _LINKS.prepared.pop(_stage_key(kind, params), None) if _LINKS.prepared else None
        if pre is not None and (pre[0] != _dims_key(d) or (pre[2] is None) != (drop_b is None) or
                                (drop_b is not None and pre[2].data_ptr() != drop_b.data_ptr())):
            pre = None                                  # prepared for another shape or another stochastic-depth table: prepare here
        nxt, _LINKS.next = _LINKS.next, None
        if nxt is not None and nxt[0] != kind:          # the next stage's opening InstanceNorm rides in this stage's last launch
            pn = _LINKS.prepared.get(nxt)
            if pn is not None and pn[0][:7] == _dims_key(d)[:7]:      # same dtype and token geometry (the stages' own switches may differ)
                dn = L.Dims(*pn[0])
                L.check(lib.bf_stage_chain_next(C.byref(dn), 0 if nxt[0] == "temporal" else 1, C.addressof(pn[3]), _p(pn[1])), "bf_stage_chain_next")
        if kind == "temporal":
            st = pre[3] if pre else L.TemporalParams(*[_p(p) for p in params])
            saved = pre[1] if pre else _saved(lib.bf_temporal_saved_bytes(C.byref(d)), x.device, "bf_temporal_saved_bytes")
            fwd = lib.bf_temporal_fwd
        else:
            st = pre[3] if pre else L.SpatialParams(*[_p(p) for p in params])
            saved = pre[1] if pre else _saved(lib.bf_spatial_saved_bytes(C.byref(d)), x.device, "bf_spatial_saved_bytes")
            fwd = lib.bf_spatial_fwd
        out = torch.empty_like(x)
        lib.bf_stage_prepared(1 if pre else 0)
        if kind == "temporal":
            rc = fwd(C.byref(d), C.byref(st), _p(x), _p(out), _p(saved), _p(scratch_for(d, x.device)), _p(drop_a), _stream())
        else:
            rc = fwd(C.byref(d), C.byref(st), _p(x), _p(out), _p(saved), _p(scratch_for(d, x.device)), _p(drop_a), _p(drop_b), _stream())
        L.check(rc, f"bf_{kind}_fwd")
        # Backward chain (bf_stage_chain_tail): a temporal stage fed by a spatial stage's output remembers that stage -- its backward's last
        # kernel produces that stage's output gradient and can open that stage's backward (the MLP-branch InstanceNorm) in the same launch
        last, _LINKS.last_spatial = _LINKS.last_spatial, None
        lastt, _LINKS.last_temporal = _LINKS.last_temporal, None
        ctx.prev_spatial = ctx.next_scale = None
        if kind == "temporal" and drop_a is not None and x.dtype == torch.bfloat16:
            _LINKS.last_temporal = (out.data_ptr(), drop_a, T)
        if kind == "spatial" and lastt is not None and lastt[0] == x.data_ptr():
            ctx.next_scale = (lastt[1], lastt[2])      # the backward of the temporal stage in front scales this stage's dx by these factors (bf_stage_next_scale)
        if kind == "spatial":
            if x.dtype == torch.bfloat16 and os.environ.get("BF_STAGE_CHAIN", "1") != "0":
                _LINKS.last_spatial = (out.data_ptr(), (tuple(x.shape), x.dtype), st, saved, drop_b is not None, params)
        elif last is not None and last[0] == x.data_ptr() and last[1] == (tuple(x.shape), x.dtype):
            ctx.prev_spatial = last[2:]
        ctx.drops = (drop_a, drop_b)
        ctx.kind, ctx.cfg = kind, (heads, attn_scale, feat_scale)
        ctx.save_for_backward(x, saved, *[p for p in params if p is not None])
        ctx.mask = [p is not None for p in params]
        return out

    @staticmethod
    def backward(ctx, dout):
        x, saved, *ps = ctx.saved_tensors
        it = iter(ps)
        params = [next(it) if m else None for m in ctx.mask]
        heads, attn_scale, feat_scale = ctx.cfg
        B, T, h, w, E = x.shape
        d = make_dims(x.dtype, B, T, h, w, E, heads, attn_scale, feat_scale)
        lib = L.lib()
        dout = dout.contiguous()
        gviews, ret, direct = _stage_grads(params)
        if ctx.kind == "temporal":
            st, gs, bwd = L.TemporalParams(*[_p(p) for p in params]), L.TemporalParams(*[_p(g) for g in gviews]), lib.bf_temporal_bwd
        else:
            st, gs, bwd = L.SpatialParams(*[_p(p) for p in params]), L.SpatialParams(*[_p(g) for g in gviews]), lib.bf_spatial_bwd
        dx = torch.empty_like(x)
        drop_a, drop_b = ctx.drops
        if ctx.kind == "temporal":
            ps = getattr(ctx, "prev_spatial", None)
            if ps is not None and direct:       # (the chained norm's partial sums are reduced by the spatial stage's own backward, which must follow)
                L.check(lib.bf_stage_chain_tail(C.byref(ps[0]), _p(ps[1]), 1 if ps[2] else 0), "bf_stage_chain_tail")
            rc = bwd(C.byref(d), C.byref(st), C.byref(gs), _p(x), _p(dout), _p(dx), _p(saved), _p(scratch_for(d, x.device)), _p(drop_a), _stream())
        else:
            ns = getattr(ctx, "next_scale", None)
            if ns is not None and direct:
                lib.bf_stage_next_scale(_p(ns[0]), ns[1])
            rc = bwd(C.byref(d), C.byref(st), C.byref(gs), _p(x), _p(dout), _p(dx), _p(saved), _p(scratch_for(d, x.device)), _p(drop_a),
                     _p(drop_b), _stream())      # (the stage call takes its hints out of the library's record at its top: nothing to disarm)
        L.check(rc, f"bf_{ctx.kind}_bwd")
        if _DEFER["on"]:
            _DEFER["keep"].append((saved, dout, x))
        _stage_done(params, direct)
        return (dx, None, None, None, None, None, None, *ret)


# ------------------------------------------------------------------------------------------------ the training trunk in one call per direction
class _TrunkFn(torch.autograd.Function):
    """All trunk stages of a training step through bf_trunk_train_fwd / bf_trunk_train_bwd: one native call per direction instead of one
    Python -> ctypes round trip (and one autograd node) per stage.  Same kernels, same chain hints, same saved records as the per-stage
    Functions; the per-stage gradient-ready notifications of the data-parallel reducer come through a host callback."""

    @staticmethod
    def forward(ctx, x, cfg, kinds, masks, drops, *flat):
        _require_gpu(x)
        heads, attn_scale, feat_scale = cfg
        x = x.contiguous()
        B, T, h, w, E = x.shape
        d = make_dims(x.dtype, B, T, h, w, E, heads, attn_scale, feat_scale)
        lib = L.lib()
        n = len(kinds)
        it = iter(flat)
        plist = [[_f32c(next(it)) if m else None for m in mask] for mask in masks]
        for kind, ps in zip(kinds, plist):
            _check_stage_params(kind, ps, E, heads, x.device)
        structs = [(L.TemporalParams if kind == "temporal" else L.SpatialParams)(*[_p(p) for p in ps]) for kind, ps in zip(kinds, plist)]
        kinds_c = (C.c_int32 * n)(*[0 if k == "temporal" else 1 for k in kinds])
        pp = (C.c_void_p * n)(*[C.addressof(s) for s in structs])
        nb = {"temporal": lib.bf_temporal_saved_bytes(C.byref(d)), "spatial": lib.bf_spatial_saved_bytes(C.byref(d))}
        if min(nb.values()) < 0:
            L.check(-1, "bf_*_saved_bytes")
        offs, total = [], 0
        for k in kinds:
            offs.append(total)
            total += (nb[k] + 255) // 256 * 256
        arena = torch.empty(total, dtype=torch.uint8, device=x.device)
        sp = (C.c_void_p * n)(*[arena.data_ptr() + o for o in offs])
        acts = torch.empty((max(n - 1, 1),) + tuple(x.shape), dtype=x.dtype, device=x.device)      # the outputs of stages 0 .. n - 2 (inputs of 1 .. n - 1)
        out = torch.empty_like(x)
        ap = (C.c_void_p * n)(*([acts[i].data_ptr() for i in range(n - 1)] + [out.data_ptr()]))
        da = [None if dr is None or dr[0] is None else dr[0].contiguous().float() for dr in drops]
        db = [None if dr is None or len(dr) < 2 or dr[1] is None else dr[1].contiguous().float() for dr in drops]
        dap = (C.c_void_p * n)(*[_p(t) for t in da])
        dbp = (C.c_void_p * n)(*[_p(t) for t in db])
        L.check(lib.bf_trunk_train_fwd(C.byref(d), n, kinds_c, pp, sp, dap, dbp, _p(x), ap, _p(scratch_for(d, x.device)), _stream()), "bf_trunk_train_fwd")
        ctx.cfg, ctx.kinds, ctx.masks, ctx.offs = cfg, kinds, masks, offs
        ctx.drops = (da, db)
        ctx.save_for_backward(x, arena, acts, *[p for ps in plist for p in ps if p is not None])      # what the native call was given (see _BlockFn)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, arena, acts, *flat = ctx.saved_tensors
        heads, attn_scale, feat_scale = ctx.cfg
        kinds, masks = ctx.kinds, ctx.masks
        B, T, h, w, E = x.shape
        d = make_dims(x.dtype, B, T, h, w, E, heads, attn_scale, feat_scale)
        lib = L.lib()
        n = len(kinds)
        it = iter(flat)
        plist = [[next(it) if m else None for m in mask] for mask in masks]
        pstructs, gstructs, rets, directs = [], [], [], []
        for kind, ps in zip(kinds, plist):
            gviews, ret, direct = _stage_grads(ps)
            cls = L.TemporalParams if kind == "temporal" else L.SpatialParams
            pstructs.append(cls(*[_p(p) for p in ps]))
            gstructs.append(cls(*[_p(g) for g in gviews]))
            rets.append(ret)
            directs.append(direct)
        kinds_c = (C.c_int32 * n)(*[0 if k == "temporal" else 1 for k in kinds])
        pp = (C.c_void_p * n)(*[C.addressof(s) for s in pstructs])
        gp = (C.c_void_p * n)(*[C.addressof(s) for s in gstructs])
        sp = (C.c_void_p * n)(*[arena.data_ptr() + o for o in ctx.offs])
        ap = (C.c_void_p * n)(*([acts[i].data_ptr() for i in range(n - 1)] + [None]))
        da, db = ctx.drops
        dap = (C.c_void_p * n)(*[_p(t) for t in da])
        dbp = (C.c_void_p * n)(*[_p(t) for t in db])
        dout = dout.contiguous()
        gbuf = torch.empty((3,) + tuple(x.shape), dtype=x.dtype, device=x.device)
        g3 = (C.c_void_p * 3)(*[gbuf[i].data_ptr() for i in range(3)])
        dx = torch.empty_like(x)
        on_ready = _DIRECT["on_ready"]
        errs = []

        def done(i, _user):          # host callback from inside the native call: stage i's backward is enqueued
            try:
                if directs[i] and on_ready is not None:
                    on_ready([p.data_ptr() for p in plist[i] if p is not None])
            except BaseException as e:      # an exception must not unwind through the C frames
                errs.append(e)

        cb = L.STAGE_DONE_FN(done)
        rc = lib.bf_trunk_train_bwd(C.byref(d), n, kinds_c, pp, gp, sp, dap, dbp, _p(x), ap, _p(dout), g3, _p(dx), _p(scratch_for(d, x.device)),
                                    C.cast(cb, C.c_void_p), None, _stream())
        L.check(rc, "bf_trunk_train_bwd")
        if errs:
            raise errs[0]
        if not all(directs):             # gradients go back through autograd on this stream: nothing may still be in flight on the side stream
            L.check(lib.bf_side_join(_stream()), "bf_side_join")
        if _DEFER["on"]:
            _DEFER["keep"].append((arena, acts, dout, x, gbuf))
        flat_ret = [g for ret, mask in zip(rets, masks) for g, m in zip(ret, mask) if m]
        return (dx, None, None, None, None, *flat_ret)


def trunk_train(tok: torch.Tensor, heads: int, attn_scale: bool, feat_scale: bool, stages) -> Optional[torch.Tensor]:
    """Training forward of all trunk stages in ONE native call (and their backward in one more).  stages: [(kind, params, drops)] in call
    order, drops = None, (drop,) for a temporal stage, (drop_att, drop_mlp) for a spatial one.  Returns None when the per-stage path is
    asked for (BF_TRUNK_NATIVE=0, or BF_STAGE_CHAIN=0: the native call always chains the stage heads) -- the caller then runs the stages."""
    if not tok.is_cuda or not stages or os.environ.get("BF_TRUNK_NATIVE", "1") == "0" or os.environ.get("BF_STAGE_CHAIN", "1") == "0":
        return None
    if tok.dim() != 5:
        raise L.BubbleformerHipError("trunk_train: tokens must be (B, T, h, w, E)")
    kinds = tuple(k for k, _, _ in stages)
    masks = tuple(tuple(p is not None for p in ps) for _, ps, _ in stages)
    flat = [p for _, ps, _ in stages for p in ps if p is not None]
    drops = [dr for _, _, dr in stages]
    return _TrunkFn.apply(tok, (heads, bool(attn_scale), bool(feat_scale)), kinds, masks, drops, *flat)


def temporal_block(x: torch.Tensor, heads: int, attn_scale: bool, params: List[Optional[torch.Tensor]], drop=None) -> torch.Tensor:
    """x: (B, T, h, w, E) tokens.  params in ``_lib.TEMPORAL_FIELDS`` order (None where the reference has no parameter).
    drop: optional [B] stochastic-depth factors (0 or 1/keep) for the attention branch."""
    return _BlockFn.apply(x, "temporal", heads, attn_scale, True, drop, None, *params)


def spatial_block(x: torch.Tensor, heads: int, attn_scale: bool, feat_scale: bool, params: List[Optional[torch.Tensor]], drop_att=None,
                  drop_mlp=None) -> torch.Tensor:
    """x: (B, T, h, w, E) tokens (frames = B*T).  params in ``_lib.SPATIAL_FIELDS`` order.
    drop_att / drop_mlp: optional [B*T] stochastic-depth factors for the attention and the MLP branch."""
    return _BlockFn.apply(x, "spatial", heads, attn_scale, feat_scale, drop_att, drop_mlp, *params)


def drop_path_factors(n: int, drop_prob: float, device) -> torch.Tensor:
    """timm.layers.DropPath semantics (scale_by_keep=True): one Bernoulli(keep) / keep factor per sample of dim 0."""
    keep = 1.0 - drop_prob
    return torch.empty(n, dtype=torch.float32, device=device).bernoulli_(keep).div_(keep)


# ------------------------------------------------------------------------------------------------ embed / debed
def _stage_arrays(conv, inw, inb):
    n = L.BF_MAX_STAGES
    arr = lambda xs: (L.fp * n)(*([_p(t) for t in xs] + [None] * (n - len(xs))))
    return arr(conv), arr(inw), arr(inb)


class _EmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fluid, compute_dtype, patch, embed_dim, nst, *params):
        # params: conv_w[nst], in_w[nst], in_b[nst], then (film_ln_w, film_ln_b, film_w, film_b) or nothing
        _require_gpu(x)
        x = x.contiguous().float()
        B, T, Cin, H, W = x.shape
        if H % patch or W % patch:
            raise L.BubbleformerHipError(f"input {H}x{W} is not a multiple of the patch size {patch}")
        h, w = H // patch, W // patch
        params = [_f32c(p) for p in params]
        conv, inw, inb, film = params[:nst], params[nst:2 * nst], params[2 * nst:3 * nst], params[3 * nst:]
        nfluid = 0
        if film:
            fluid = fluid.contiguous().float()
            nfluid = fluid.shape[1]
        d = make_dims(compute_dtype, B, T, h, w, embed_dim, 1, patch=patch, cin=Cin, cout=1, nfluid=nfluid)
        lib = L.lib()
        cw, iw, ib = _stage_arrays(conv, inw, inb)
        st = L.EmbedParams(cw, iw, ib, *([_p(t) for t in film] if film else [None] * 4))
        saved = _saved(lib.bf_embed_saved_bytes(C.byref(d)), x.device, "bf_embed_saved_bytes")
        out = torch.empty((B, T, h, w, embed_dim), dtype=compute_dtype, device=x.device)
        L.check(lib.bf_embed_fwd(C.byref(d), C.byref(st), _p(x), _p(fluid) if film else None, _p(out), _p(saved),
                                 _p(scratch_for(d, x.device)), _stream()), "bf_embed_fwd")
        ctx.cfg = (compute_dtype, patch, embed_dim, nst, nfluid, tuple(x.shape))
        ctx.save_for_backward(saved, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        saved, *params = ctx.saved_tensors
        compute_dtype, patch, E, nst, nfluid, xshape = ctx.cfg
        B, T, Cin, H, W = xshape
        h, w = H // patch, W // patch
        d = make_dims(compute_dtype, B, T, h, w, E, 1, patch=patch, cin=Cin, cout=1, nfluid=nfluid)
        lib = L.lib()
        conv, inw, inb, film = params[:nst], params[nst:2 * nst], params[2 * nst:3 * nst], params[3 * nst:]
        gv, ret, direct = _stage_grads(params)
        cw, iw, ib = _stage_arrays(conv, inw, inb)
        st = L.EmbedParams(cw, iw, ib, *([_p(t) for t in film] if film else [None] * 4))
        gcw, giw, gib = _stage_arrays(gv[:nst], gv[nst:2 * nst], gv[2 * nst:3 * nst])
        gs = L.EmbedParams(gcw, giw, gib, *([_p(t) for t in gv[3 * nst:]] if film else [None] * 4))
        dout = dout.contiguous()
        dx = torch.empty(xshape, dtype=torch.float32, device=dout.device) if ctx.needs_input_grad[0] else None
        _joined()
        L.check(lib.bf_embed_bwd(C.byref(d), C.byref(st), C.byref(gs), _p(dout), _p(dx), _p(saved), _p(scratch_for(d, dout.device)),
                                 _stream()), "bf_embed_bwd")
        _stage_done(params, direct)
        return (dx, None, None, None, None, None, *ret)


def embed(x, fluid, compute_dtype, patch, embed_dim, conv_w, in_w, in_b, film_params=()):
    """x: (B, T, C, H, W) fp32 clip -> (B, T, h, w, E) tokens.  film_params = (ln_w, ln_b, lin_w, lin_b) or ()."""
    nst = len(conv_w)
    return _EmbedFn.apply(x, fluid, compute_dtype, patch, embed_dim, nst, *conv_w, *in_w, *in_b, *film_params)


class _DebedFn(torch.autograd.Function):
    """tokens -> (B, T, Cout, H, W) fp32; with ``target`` also the fused relative-L2 loss.  ``pred_grad``: beside the fused loss the
    prediction stays differentiable (a training step unrolled through its own predictions feeds it back)."""

    @staticmethod
    def forward(ctx, x, target, patch, cout, nst, pred_grad, *params):
        _require_gpu(x)
        x = x.contiguous()
        B, T, h, w, E = x.shape
        params = [_f32c(p) for p in params]
        conv, inw, inb = params[:nst], params[nst:2 * nst - 1], params[2 * nst - 1:]
        d = make_dims(x.dtype, B, T, h, w, E, 1, patch=patch, cin=1, cout=cout)
        lib = L.lib()
        cw, iw, ib = _stage_arrays(conv, inw, inb)
        st = L.DebedParams(cw, iw, ib)
        saved = _saved(lib.bf_debed_saved_bytes(C.byref(d)), x.device, "bf_debed_saved_bytes")
        pred = torch.empty((B, T, cout, h * patch, w * patch), dtype=torch.float32, device=x.device)
        loss = torch.zeros((), dtype=torch.float32, device=x.device)
        if target is not None:
            target = target.contiguous().float()
            if target.shape != pred.shape:
                raise L.BubbleformerHipError(f"target shape {tuple(target.shape)} != prediction shape {tuple(pred.shape)}")
        L.check(lib.bf_debed_fwd(C.byref(d), C.byref(st), _p(x), _p(pred), _p(target), _p(loss) if target is not None else None,
                                 _p(saved), _p(scratch_for(d, x.device)), _stream()), "bf_debed_fwd")
        ctx.cfg = (patch, cout, nst, target is not None, bool(pred_grad))
        ctx.save_for_backward(x, saved, pred, target if target is not None else pred, *params)
        ctx.set_materialize_grads(False)      # an unused output must not cost a zero-filled gradient the size of the prediction
        return pred, loss

    @staticmethod
    def backward(ctx, dpred, dloss):
        x, saved, pred, target, *params = ctx.saved_tensors
        patch, cout, nst, fused, pred_grad = ctx.cfg
        if fused and dpred is not None and not pred_grad:
            raise L.BubbleformerHipError("debed_with_loss: a gradient w.r.t. the prediction is not supported beside the fused loss; "
                                         "use debed() and a separate loss for that")
        if dpred is None and (dloss is None or not fused):
            return (None,) * (6 + len(params))
        B, T, h, w, E = x.shape
        d = make_dims(x.dtype, B, T, h, w, E, 1, patch=patch, cin=1, cout=cout)
        lib = L.lib()
        conv, inw, inb = params[:nst], params[nst:2 * nst - 1], params[2 * nst - 1:]
        gv, ret, direct = _stage_grads(params)
        cw, iw, ib = _stage_arrays(conv, inw, inb)
        st = L.DebedParams(cw, iw, ib)
        gcw, giw, gib = _stage_arrays(gv[:nst], gv[nst:2 * nst - 1], gv[2 * nst - 1:])
        gs = L.DebedParams(gcw, giw, gib)
        dx = torch.empty_like(x)
        # the three source modes of bf_debed_bwd: the loss term dloss * coef[f, c] * (pred - target) alone, an explicit dpred alone, or
        # (pred_grad) both, added in the registers of the last stage's kernels
        with_loss = fused and dloss is not None
        scale = dloss.contiguous().float().reshape(1) if with_loss else None
        dpred = dpred.contiguous().float() if dpred is not None else None
        L.check(lib.bf_debed_bwd(C.byref(d), C.byref(st), C.byref(gs), _p(x), _p(dpred), _p(pred) if with_loss else None,
                                 _p(target) if with_loss else None, _p(scale), _p(dx), _p(saved), _p(scratch_for(d, x.device)), _stream()),
                "bf_debed_bwd")
        _stage_done(params, direct)
        return (dx, None, None, None, None, None, *ret)


def debed(x, patch, cout, conv_w, in_w, in_b):
    """x: (B, T, h, w, E) tokens -> (B, T, Cout, H, W) fp32 prediction."""
    pred, _ = _DebedFn.apply(x, None, patch, cout, len(conv_w), False, *conv_w, *in_w, *in_b)
    return pred


def debed_with_loss(x, target, patch, cout, conv_w, in_w, in_b, pred_grad=False):
    """Fused debed + relative-L2 loss (LpLoss d=2, p=2, mean B, mean T, sum C).  Returns (loss, pred).  By default only ``loss`` carries
    gradient (pred is produced for logging).  ``pred_grad=True`` keeps the prediction in the graph as well: the backward then takes a
    gradient w.r.t. the prediction and one w.r.t. the loss together (their sum is formed inside the last stage's backward kernels, no
    composed gradient in memory), either one alone, or neither."""
    pred, loss = _DebedFn.apply(x, target, patch, cout, len(conv_w), pred_grad, *conv_w, *in_w, *in_b)
    return loss, (pred if pred_grad else pred.detach())


# ------------------------------------------------------------------------------------------------ optimizer
class _GeluMlpFn(torch.autograd.Function):
    """fc2(gelu(fc1(x))) on the last dimension as four (forward: two) native GEMMs -- `GeluMLP.forward` used on its own
    (bubbleformer/layers/linear_layers.py:18-25); inside the axial block the same GEMMs run as part of bf_spatial_fwd / bwd."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        _require_gpu(x)
        from . import kernels as K
        dt = x.dtype if x.dtype in (torch.float32, torch.bfloat16) else torch.float32
        D, Hd = w1.shape[1], w1.shape[0]
        x2 = x.reshape(-1, D).to(dt).contiguous()
        M = x2.shape[0]
        w1c, w2c = w1.to(dt).contiguous(), w2.to(dt).contiguous()
        pre = torch.empty(M, Hd, dtype=dt, device=x.device)
        hid = torch.empty(M, Hd, dtype=dt, device=x.device)
        out = torch.empty(M, D, dtype=dt, device=x.device)
        K.gemm(dt, M, Hd, D, K.operand(x2, D), K.operand(w1c, D), K.epilogue(pre, Hd, bias=_f32c(b1), gelu_out=hid))
        K.gemm(dt, M, D, Hd, K.operand(hid, Hd), K.operand(w2c, Hd), K.epilogue(out, D, bias=_f32c(b2)))
        ctx.save_for_backward(x2, pre, hid, w1c, w2c)
        ctx.shape, ctx.in_dtype = x.shape, x.dtype
        return out.reshape(x.shape).to(x.dtype)

    @staticmethod
    def backward(ctx, dout):
        from . import kernels as K
        x2, pre, hid, w1c, w2c = ctx.saved_tensors
        dt = x2.dtype
        M, D = x2.shape
        Hd = pre.shape[1]
        dev = x2.device
        dy = dout.reshape(M, D).to(dt).contiguous()
        dw1 = torch.zeros(Hd, D, dtype=torch.float32, device=dev)
        db1 = torch.zeros(Hd, dtype=torch.float32, device=dev)
        dw2 = torch.zeros(D, Hd, dtype=torch.float32, device=dev)
        db2 = torch.zeros(D, dtype=torch.float32, device=dev)
        dpre = torch.empty(M, Hd, dtype=dt, device=dev)
        dx = torch.empty(M, D, dtype=dt, device=dev)
        sk = max(1, min(64, M // 512))
        XC, AT = L.BF_LAY_XC, L.BF_OUT_ATOMIC_F32
        K.gemm(dt, D, Hd, M, K.operand(dy, D, layout=XC), K.operand(hid, Hd, layout=XC), K.epilogue(dw2, Hd, out_mode=AT, colsum=db2), splitk=sk)
        K.gemm(dt, M, Hd, D, K.operand(dy, D), K.operand(w2c, Hd, layout=XC), K.epilogue(dpre, Hd, aux_mode=L.BF_AUX_DGELU, aux=pre, ld_aux=Hd))
        K.gemm(dt, Hd, D, M, K.operand(dpre, Hd, layout=XC), K.operand(x2, D, layout=XC), K.epilogue(dw1, D, out_mode=AT, colsum=db1), splitk=sk)
        K.gemm(dt, M, D, Hd, K.operand(dpre, Hd), K.operand(w1c, D, layout=XC), K.epilogue(dx, D))
        return dx.reshape(ctx.shape).to(ctx.in_dtype), dw1, db1, dw2, db2


def gelu_mlp(x: torch.Tensor, w1, b1, w2, b2) -> torch.Tensor:
    return _GeluMlpFn.apply(x, w1, b1, w2, b2)


class _FilmFn(torch.autograd.Function):
    """`FiLMMLP.forward` used on its own (bubbleformer/layers/linear_layers.py:63-77): gamma, beta = Linear(LayerNorm(cond)).chunk(2);
    out = gamma * x + beta over x (B, T, C, h, w).  Native pieces: bf_film_net_fwd / bwd for the conditioning network,
    bf_affine_apply for the modulation and its data gradient, and the InstanceNorm-backward reduction (mean 0, rstd 1: its
    per-frame partials are exactly sum(dout) and sum(dout * x)) for d gamma / d beta.  In the model FiLM rides inside bf_embed_fwd."""

    @staticmethod
    def forward(ctx, x, cond, lnw, lnb, W, bias):
        _require_gpu(x)
        lib = L.lib()
        B, T, Cc, h, w = x.shape
        dt = x.dtype if x.dtype in (torch.float32, torch.bfloat16) else torch.float32
        tok = as_tokens(x.to(dt))                                     # (B, T, h, w, C)
        cond = cond.contiguous().float()
        P = cond.shape[1]
        prm = [_f32c(t) for t in (lnw, lnb, W, bias)]
        gb = torch.empty(2, B, Cc, dtype=torch.float32, device=x.device)          # the kernel's layout: [gamma | beta][B][C]
        chat = torch.empty(B, P, dtype=torch.float32, device=x.device)
        crstd = torch.empty(B, dtype=torch.float32, device=x.device)
        L.check(lib.bf_film_net_fwd(_p(cond), *[_p(t) for t in prm], _p(gb), _p(chat), _p(crstd), B, P, 2 * Cc, _stream()), "bf_film_net_fwd")
        gamma, beta = gb[0], gb[1]
        out = torch.empty_like(tok)
        S = T * h * w
        L.check(lib.bf_affine_apply(_dt(dt), _p(tok), None, _p(gamma), _p(beta), _p(out), B * S, S, Cc, _stream()), "bf_affine_apply")
        ctx.save_for_backward(tok, gamma, chat, *prm)
        ctx.dims = (B, T, Cc, h, w, P, x.dtype)
        return as_reference_layout(out).to(x.dtype)

    @staticmethod
    def backward(ctx, dout):
        lib = L.lib()
        tok, gamma, chat, lnw, lnb, W, bias = ctx.saved_tensors
        B, T, Cc, h, w, P, in_dtype = ctx.dims
        dt, dev, S = tok.dtype, tok.device, T * h * w
        dtok = as_tokens(dout.to(dt))
        dx = torch.empty_like(tok)
        L.check(lib.bf_affine_apply(_dt(dt), _p(dtok), None, _p(gamma), None, _p(dx), B * S, S, Cc, _stream()), "bf_affine_apply")
        zero = torch.zeros(B, Cc, dtype=torch.float32, device=dev)
        one = torch.ones(B, Cc, dtype=torch.float32, device=dev)
        ws = torch.zeros(lib.bf_in_ws_floats(_dt(dt), B, S, Cc), dtype=torch.float32, device=dev)
        junk = torch.empty_like(tok)
        L.check(lib.bf_in_bwd(_dt(dt), _p(dtok), _p(tok), None, _p(junk), B, S, Cc, _p(zero), _p(one), _p(one[0].contiguous()), _p(zero[0].contiguous()),
                              None, 1, 0, None, None, None, None, _p(ws), _stream()), "bf_in_bwd")
        part = ws[:B * Cc * 2].view(B, Cc, 2)                         # {sum dout, sum dout * x} per (batch element, channel)
        dgb = torch.stack([part[..., 1], part[..., 0]]).contiguous()          # [d gamma | d beta][B][C]
        gr = [torch.zeros_like(t) for t in (W, bias, lnw, lnb)]
        L.check(lib.bf_film_net_bwd(_p(dgb), _p(chat), _p(lnw), _p(lnb), _p(W), *[_p(t) for t in gr], B, P, 2 * Cc, _stream()), "bf_film_net_bwd")
        dW, dbias, dlnw, dlnb = gr
        return as_reference_layout(dx).to(in_dtype), None, dlnw, dlnb, dW, dbias


def film(x: torch.Tensor, cond: torch.Tensor, lnw, lnb, W, bias) -> torch.Tensor:
    return _FilmFn.apply(x, cond, lnw, lnb, W, bias)


def clip_gather(frames: torch.Tensor, first: torch.Tensor, t0: int, T: int, table, Ho: int, Wo: int) -> torch.Tensor:
    """frames [fields][total_frames][H][W] fp32 (device), first [B] int64 absolute first input frame per sample, table =
    (field ids int32 [C], diff fp32 [C], div fp32 [C]) -> (B, T, C, Ho, Wo) fp32 normalised clips (data/dataset.py)."""
    _require_gpu(frames)
    ids, diff, div = table
    nf, total, H, W = frames.shape
    B, Cn = first.numel(), ids.numel()
    out = torch.empty((B, T, Cn, Ho, Wo), dtype=torch.float32, device=frames.device)
    L.check(L.lib().bf_clip_gather(_p(frames), total * H * W, _p(ids), _p(first), int(t0), _p(diff), _p(div), _p(out), B, T, Cn, H, W, Ho, Wo,
                                   _stream()), "bf_clip_gather")
    return out


def clip_gather_batch(frames: torch.Tensor, idx: torch.Tensor, first_tab: torch.Tensor, T: int, in_table, out_table, Ho: int, Wo: int,
                      fluid_tab: Optional[torch.Tensor] = None, file_tab: Optional[torch.Tensor] = None):
    """One launch for a batch: idx [B] int64 sample numbers (device), first_tab / file_tab per-sample tables (device) -> input clips
    (B, T, Cin, Ho, Wo), target clips (B, T, Cout, Ho, Wo) and, when fluid_tab is given, the (B, P) fluid-parameter rows."""
    _require_gpu(frames)
    (iid, idf, idv), (oid, odf, odv) = in_table, out_table
    nf, total, H, W = frames.shape
    B = idx.numel()
    inp = torch.empty((B, T, iid.numel(), Ho, Wo), dtype=torch.float32, device=frames.device)
    out = torch.empty((B, T, oid.numel(), Ho, Wo), dtype=torch.float32, device=frames.device)
    P = int(fluid_tab.shape[1]) if fluid_tab is not None else 0
    fl = torch.empty((B, P), dtype=torch.float32, device=frames.device) if fluid_tab is not None else None
    L.check(L.lib().bf_clip_gather_batch(_p(frames), total * H * W, _p(idx), first_tab.numel(), _p(first_tab), _p(iid), _p(idf), _p(idv), iid.numel(), T, _p(inp),
                                         _p(oid), _p(odf), _p(odv), oid.numel(), T, _p(out), _p(fluid_tab) if fl is not None else None,
                                         _p(file_tab) if fl is not None else None, P, _p(fl) if fl is not None else None, B, H, W, Ho, Wo,
                                         _stream()), "bf_clip_gather_batch")
    return inp, out, fl


def clip_gather_unroll(frames: torch.Tensor, idx: torch.Tensor, first_tab: torch.Tensor, T: int, unroll: int, in_table, out_table, Ho: int, Wo: int,
                       fluid_tab: Optional[torch.Tensor] = None, file_tab: Optional[torch.Tensor] = None):
    """clip_gather_batch with ``unroll`` target clips behind the input clip, still one launch: -> input clips (B, T, Cin, Ho, Wo), target
    clips (unroll, B, T, Cout, Ho, Wo) -- targets[j] contiguous, frames first + (j + 1) T .. first + (j + 2) T - 1 -- and the fluid rows.
    idx is clamped into the sample range and every frame number below the store's frame count on the device (a sample whose later clips
    lie behind its own file then reads the next file's frames, and the store's last frame where the store ends, never past it); the
    caller checks what it can on the host (DeviceClipStore.gather)."""
    _require_gpu(frames)
    (iid, idf, idv), (oid, odf, odv) = in_table, out_table
    nf, total, H, W = frames.shape
    B = idx.numel()
    if int(unroll) != unroll or unroll < 1:
        raise ValueError(f"clip_gather_unroll: unroll {unroll!r} must be an integer >= 1")
    inp = torch.empty((B, T, iid.numel(), Ho, Wo), dtype=torch.float32, device=frames.device)
    out = torch.empty((int(unroll), B, T, oid.numel(), Ho, Wo), dtype=torch.float32, device=frames.device)
    P = int(fluid_tab.shape[1]) if fluid_tab is not None else 0
    fl = torch.empty((B, P), dtype=torch.float32, device=frames.device) if fluid_tab is not None else None
    L.check(L.lib().bf_clip_gather_unroll(_p(frames), total * H * W, total, _p(idx), first_tab.numel(), _p(first_tab), _p(iid), _p(idf), _p(idv), iid.numel(), T,
                                          _p(inp), _p(oid), _p(odf), _p(odv), oid.numel(), T, int(unroll), _p(out), _p(fluid_tab) if fl is not None else None,
                                          _p(file_tab) if fl is not None else None, P, _p(fl) if fl is not None else None, B, H, W, Ho, Wo,
                                          _stream()), "bf_clip_gather_unroll")
    return inp, out, fl


def clip_gather_augment(frames: torch.Tensor, idx: torch.Tensor, first_tab: torch.Tensor, T: int, unroll: int, in_table, out_table, Ho: int, Wo: int,
                        in_odd: torch.Tensor, out_odd: torch.Tensor, seed: int, draw: int, flip_thr: int, Hc: int, Wc: int, random_y: bool = False,
                        eval_view: bool = False, fluid_tab: Optional[torch.Tensor] = None, file_tab: Optional[torch.Tensor] = None):
    """clip_gather_unroll with a seeded mirror in x and a seeded ``Hc x Wc`` window of the ``Ho x Wo`` output grid per sample, one launch
    (bf_clip_gather_augment; utils/augment.py states the draw): -> input clips (B, T, Cin, Hc, Wc), target clips (unroll, B, T, Cout, Hc, Wc)
    and the plain fluid rows.  in_odd [Cin] / out_odd [Cout]: int32 device tables, 1 where the channel's field changes sign when mirrored.
    ``seed`` counts modulo 2^64 and ``draw`` modulo 2^32; ``flip_thr`` = min(round(flip_p 2^32), 2^32); ``eval_view`` draws nothing (never
    mirrored, the window centred in x at y0 = 0)."""
    _require_gpu(frames)
    (iid, idf, idv), (oid, odf, odv) = in_table, out_table
    nf, total, H, W = frames.shape
    B = idx.numel()
    if int(unroll) != unroll or unroll < 1:
        raise ValueError(f"clip_gather_augment: unroll {unroll!r} must be an integer >= 1")
    if not (1 <= int(Hc) <= Ho and 1 <= int(Wc) <= Wo):
        raise ValueError(f"clip_gather_augment: the window {(Hc, Wc)} must lie inside the output grid {(Ho, Wo)}")
    _check_tensors("clip_gather_augment", frames.device, {"in_odd": (in_odd, (iid.numel(),), torch.int32), "out_odd": (out_odd, (oid.numel(),), torch.int32)})
    inp = torch.empty((B, T, iid.numel(), Hc, Wc), dtype=torch.float32, device=frames.device)
    out = torch.empty((int(unroll), B, T, oid.numel(), Hc, Wc), dtype=torch.float32, device=frames.device)
    P = int(fluid_tab.shape[1]) if fluid_tab is not None else 0
    fl = torch.empty((B, P), dtype=torch.float32, device=frames.device) if fluid_tab is not None else None
    signed = lambda v, bits: (v & (2 ** bits - 1)) - (2 ** bits if v & 2 ** (bits - 1) else 0)      # noqa: E731  (the record's signed bit patterns)
    job = L.ClipGatherJob(src=_p(frames), idx=_p(idx), first_tab=_p(first_tab), in_field=_p(iid), in_diff=_p(idf), in_div=_p(idv), in_out=_p(inp),
                          out_field=_p(oid), out_diff=_p(odf), out_div=_p(odv), out_out=_p(out), fluid_tab=_p(fluid_tab) if fl is not None else None,
                          file_tab=_p(file_tab) if fl is not None else None, fluid_out=_p(fl) if fl is not None else None, field_stride=total * H * W,
                          nframes=total, nsamples=first_tab.numel(), Cin=iid.numel(), Tin=T, Cout=oid.numel(), Tout=T, unroll=int(unroll), P=P, B=B, H=H, W=W,
                          Ho=Ho, Wo=Wo)
    aug = L.ClipAugment(in_odd=_p(in_odd), out_odd=_p(out_odd), seed=signed(int(seed), 64), flip_thr=int(flip_thr), draw=signed(int(draw), 32), Hc=int(Hc),
                        Wc=int(Wc), crop_y=int(bool(random_y)), eval_view=int(bool(eval_view)))
    L.check(L.lib().bf_clip_gather_augment(C.byref(job), C.byref(aug), _stream()), "bf_clip_gather_augment")
    return inp, out, fl


def clip_encode_q16(src: torch.Tensor, dst: torch.Tensor, lo: float, inv: float) -> torch.Tensor:
    """dst = the 16-bit codes of the contiguous fp32 ``src`` under one segment's (lo, inv) (bf_clip_encode_q16; csrc/clip_store_q16.hip
    states the format): ``dst`` is a contiguous int16 tensor of src's element count holding the codes' bit patterns, typically a slice
    of the store the chunk ``src`` belongs to.  One launch on the current stream."""
    _require_gpu(src)
    if src.dtype != torch.float32 or dst.dtype != torch.int16 or not src.is_contiguous() or not dst.is_contiguous() or src.numel() != dst.numel() or dst.device != src.device:
        raise L.BubbleformerHipError("clip_encode_q16: src must be contiguous fp32 and dst contiguous int16 of the same size on the same device")
    L.check(L.lib().bf_clip_encode_q16(_p(src), _p(dst), src.numel(), float(lo), float(inv), _stream()), "bf_clip_encode_q16")
    return dst


def _q16_tables(who: str, codes: torch.Tensor, frame_seg: torch.Tensor, seg_lo: torch.Tensor, seg_step: torch.Tensor) -> int:
    """The checks the two readers of a 16-bit store share: codes [fields][frames][H][W] int16, frame_seg [frames] int32, seg_lo / seg_step
    [fields][files] fp32 -> the file count."""
    _require_gpu(codes)
    if codes.dim() != 4 or codes.dtype != torch.int16 or not codes.is_contiguous():
        raise L.BubbleformerHipError(f"{who}: codes must be a contiguous int16 tensor [fields][frames][H][W]")
    nf, total = codes.shape[:2]
    if seg_lo.dim() != 2 or seg_lo.shape[0] != nf:
        raise L.BubbleformerHipError(f"{who}: seg_lo must be [fields][files]")
    shape = tuple(seg_lo.shape)
    _check_tensors(who, codes.device, {"frame_seg": (frame_seg, (total,), torch.int32), "seg_lo": (seg_lo, shape, torch.float32), "seg_step": (seg_step, shape, torch.float32)})
    return shape[1]


def clip_decode_q16(codes: torch.Tensor, frame_seg: torch.Tensor, seg_lo: torch.Tensor, seg_step: torch.Tensor) -> torch.Tensor:
    """The fp32 frames [fields][frames][H][W] a 16-bit store decodes to, one launch (bf_clip_decode_q16)."""
    nfiles = _q16_tables("clip_decode_q16", codes, frame_seg, seg_lo, seg_step)
    nf, total, H, W = codes.shape
    out = torch.empty((nf, total, H, W), dtype=torch.float32, device=codes.device)
    L.check(L.lib().bf_clip_decode_q16(_p(codes), total * H * W, _p(frame_seg), _p(seg_lo), _p(seg_step), _p(out), total, nf, nfiles, H, W, _stream()),
            "bf_clip_decode_q16")
    return out


def clip_gather_q16(codes: torch.Tensor, frame_seg: torch.Tensor, seg_lo: torch.Tensor, seg_step: torch.Tensor, idx: torch.Tensor, first_tab: torch.Tensor,
                    T: int, unroll: int, in_table, out_table, Ho: int, Wo: int, augment: Optional[tuple] = None, fluid_tab: Optional[torch.Tensor] = None,
                    file_tab: Optional[torch.Tensor] = None):
    """clip_gather_unroll / clip_gather_augment on a 16-bit store, decoding inside the one launch (bf_clip_gather_q16): -> input clips
    (B, T, Cin, Hc, Wc), target clips (unroll, B, T, Cout, Hc, Wc) and the fluid rows, bit for bit what those give on
    ``clip_decode_q16(codes, ...)``.  ``augment``: None -- the whole Ho x Wo grid, nothing mirrored -- or clip_gather_augment's
    ``(in_odd, out_odd, seed, draw, flip_thr, Hc, Wc, random_y, eval_view)`` under its conventions."""
    nfiles = _q16_tables("clip_gather_q16", codes, frame_seg, seg_lo, seg_step)
    (iid, idf, idv), (oid, odf, odv) = in_table, out_table
    nf, total, H, W = codes.shape
    B = idx.numel()
    if int(unroll) != unroll or unroll < 1:
        raise ValueError(f"clip_gather_q16: unroll {unroll!r} must be an integer >= 1")
    Hc, Wc, aug = Ho, Wo, None
    if augment is not None:
        in_odd, out_odd, seed, draw, flip_thr, Hc, Wc, random_y, eval_view = augment
        if not (1 <= int(Hc) <= Ho and 1 <= int(Wc) <= Wo):
            raise ValueError(f"clip_gather_q16: the window {(Hc, Wc)} must lie inside the output grid {(Ho, Wo)}")
        _check_tensors("clip_gather_q16", codes.device, {"in_odd": (in_odd, (iid.numel(),), torch.int32), "out_odd": (out_odd, (oid.numel(),), torch.int32)})
        signed = lambda v, bits: (v & (2 ** bits - 1)) - (2 ** bits if v & 2 ** (bits - 1) else 0)      # noqa: E731  (the record's signed bit patterns)
        aug = L.ClipAugment(in_odd=_p(in_odd), out_odd=_p(out_odd), seed=signed(int(seed), 64), flip_thr=int(flip_thr), draw=signed(int(draw), 32), Hc=int(Hc),
                            Wc=int(Wc), crop_y=int(bool(random_y)), eval_view=int(bool(eval_view)))
    inp = torch.empty((B, T, iid.numel(), Hc, Wc), dtype=torch.float32, device=codes.device)
    out = torch.empty((int(unroll), B, T, oid.numel(), Hc, Wc), dtype=torch.float32, device=codes.device)
    P = int(fluid_tab.shape[1]) if fluid_tab is not None else 0
    fl = torch.empty((B, P), dtype=torch.float32, device=codes.device) if fluid_tab is not None else None
    job = L.ClipGatherQ16Job(codes=_p(codes), frame_seg=_p(frame_seg), seg_lo=_p(seg_lo), seg_step=_p(seg_step), idx=_p(idx), first_tab=_p(first_tab),
                             in_field=_p(iid), in_diff=_p(idf), in_div=_p(idv), in_out=_p(inp), out_field=_p(oid), out_diff=_p(odf), out_div=_p(odv),
                             out_out=_p(out), fluid_tab=_p(fluid_tab) if fl is not None else None, file_tab=_p(file_tab) if fl is not None else None,
                             fluid_out=_p(fl) if fl is not None else None, field_stride=total * H * W, nframes=total, nsamples=first_tab.numel(),
                             nfiles=nfiles, Cin=iid.numel(), Tin=T, Cout=oid.numel(), Tout=T, unroll=int(unroll), P=P, B=B, H=H, W=W, Ho=Ho, Wo=Wo)
    L.check(L.lib().bf_clip_gather_q16(C.byref(job), C.byref(aug) if aug is not None else None, _stream()), "bf_clip_gather_q16")
    return inp, out, fl


def clip_noise(src: torch.Tensor, sigma: torch.Tensor, sample_ids: Optional[torch.Tensor], draw: int, pass_index: int, seed: int,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = src + sigma[c] * z on contiguous fp32 clips (B, T, C, H, W), z the seeded normals of bf_clip_noise (csrc/noise.hip): a pure
    function of (seed, sample id, draw, pass, element).  sigma [C] fp32 and sample_ids [B] int64 (None: 0 .. B - 1) are device tensors;
    draw / pass_index are taken modulo 2^32 and seed modulo 2^64.  ``out`` may be ``src`` itself (in place); None allocates.  One launch."""
    _require_gpu(src)
    if src.dim() != 5 or src.dtype != torch.float32 or not src.is_contiguous():
        raise L.BubbleformerHipError(f"clip_noise: the clip must be a contiguous fp32 (B, T, C, H, W) tensor, got {src.dtype} {tuple(src.shape)}")
    B, T, Cn, H, W = src.shape
    if out is None:
        out = torch.empty_like(src)
    want = {"sigma": (sigma, (Cn,), torch.float32), "sample_ids": (sample_ids, (B,), torch.int64), "out": (out, tuple(src.shape), torch.float32)}
    _check_tensors("clip_noise", src.device, want, optional=("sample_ids",))
    L.check(L.lib().bf_clip_noise(_p(src), _p(out), _p(sigma), _p(sample_ids), int(seed) & (2 ** 64 - 1), int(draw) & 0xFFFFFFFF,
                                  int(pass_index) & 0xFFFFFFFF, B, T, Cn, H, W, _stream()), "bf_clip_noise")
    return out


def _check_tensors(who: str, device, want: dict, optional=()) -> None:
    """want = {name: (tensor, shape, dtype)}: every tensor contiguous, of that shape and dtype, on ``device``; the names in ``optional`` may be None."""
    for name, (t, shape, dtype) in want.items():
        if t is None and name in optional:
            continue
        if t is None or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != device:
            raise L.BubbleformerHipError(f"{who}: {name} must be a contiguous {dtype} tensor of shape {shape} on {device}")


def _rollout_step_args(who: str, pred: torch.Tensor, frames: torch.Tensor, first: torch.Tensor, step: torch.Tensor, table, steps: int):
    """The per-step rollout bindings' checks of prediction, store, first / step and field table -> their entry points' bf_rollout_step and the stream."""
    _require_gpu(pred)
    if pred.dim() != 5 or pred.dtype != torch.float32 or not pred.is_contiguous():
        raise L.BubbleformerHipError(f"{who}: the prediction must be a contiguous fp32 (B, T, C, H, W) tensor")
    ids, diff, div = table
    nf, total, H, W = frames.shape
    B, T, Cn, Ho, Wo = pred.shape
    _check_tensors(who, pred.device, {"first": (first, (B,), torch.int64), "step": (step, (1,), torch.int32)})
    if frames.dtype != torch.float32 or not frames.is_contiguous() or frames.device != pred.device:
        raise L.BubbleformerHipError(f"{who}: the frames must be a contiguous fp32 (fields, frames, H, W) tensor on {pred.device}")
    if ids.numel() != Cn:
        raise L.BubbleformerHipError(f"{who}: the field table has {ids.numel()} channels, the prediction {Cn}")
    return L.RolloutStep(pred=_p(pred), frames=_p(frames), field_stride=total * H * W, total_frames=total, first=_p(first), step=_p(step), field=_p(ids),
                         diff=_p(diff), div=_p(div), nfields=nf, B=B, T=T, C=Cn, H=H, W=W, Ho=Ho, Wo=Wo, steps=int(steps)), _stream()


def rollout_score_workspace(pred: torch.Tensor) -> torch.Tensor:
    """The fp64 workspace ``rollout_score`` needs for predictions of this shape (allocate once, outside a graph capture)."""
    B, T, Cn, Ho, Wo = pred.shape
    return torch.empty(L.lib().bf_rollout_score_ws_doubles(B, T, Cn, Ho, Wo), dtype=torch.float64, device=pred.device)


def rollout_score(pred: torch.Tensor, frames: torch.Tensor, first: torch.Tensor, step: torch.Tensor, table, sdf_channel: int, steps: int,
                  rel_l2: torch.Tensor, criterion: torch.Tensor, ws: torch.Tensor, eik_pred: Optional[torch.Tensor] = None,
                  eik_tgt: Optional[torch.Tensor] = None, next_in: Optional[torch.Tensor] = None, archive: Optional[torch.Tensor] = None,
                  dx: float = 1.0 / 32) -> None:
    """All scores of one rollout step (bf_rollout_score; include/bubbleformer_hip.h has the contract): pred (B, T, C, Ho, Wo) fp32 against the
    frames ``first[b] + (s + 1) * T + t`` of the store, s = the int32 ``step`` tensor ON THE DEVICE, which the call increments.  Writes row
    s * T + t of rel_l2 (B, steps*T, C), criterion (B, steps), eik_pred / eik_tgt (B, steps*T) (sdf_channel >= 0), and the optional copies
    next_in (like pred) and archive (B, steps*T, C, Ho, Wo).  Allocates nothing: capturable in a HIP graph."""
    rec, stream = _rollout_step_args("rollout_score", pred, frames, first, step, table, steps)
    B, T, Cn, Ho, Wo = pred.shape
    f32 = torch.float32
    _check_tensors("rollout_score", pred.device, {"rel_l2": (rel_l2, (B, steps * T, Cn), f32), "criterion": (criterion, (B, steps), f32),
                   "eik_pred": (eik_pred, (B, steps * T), f32), "eik_tgt": (eik_tgt, (B, steps * T), f32), "next_in": (next_in, (B, T, Cn, Ho, Wo), f32),
                   "archive": (archive, (B, steps * T, Cn, Ho, Wo), f32), "ws": (ws, (ws.numel(),), torch.float64)}, ("eik_pred", "eik_tgt", "next_in", "archive"))
    L.check(L.lib().bf_rollout_score(C.byref(rec), int(sdf_channel), float(dx), _p(rel_l2), _p(criterion), _p(eik_pred), _p(eik_tgt), _p(next_in),
                                     _p(archive), _p(ws), ws.numel(), stream), "bf_rollout_score")


def rollout_heatflux(pred: torch.Tensor, frames: torch.Tensor, first: torch.Tensor, step: torch.Tensor, table, dfun_channel: int, temp_channel: int,
                     heater_temp: torch.Tensor, steps: int, flux_pred: torch.Tensor, flux_tgt: torch.Tensor, x_min: float = -8.0,
                     dx: float = 1.0 / 32, lc: float = 0.0007, conductivity: float = 0.054) -> None:
    """The heat-flux rows of one rollout step (bf_rollout_heatflux; include/bubbleformer_hip.h has the contract): row s * T + t of flux_pred /
    flux_tgt (B, steps*T) from row 0 of the de-normalised prediction and of the stored frame ``first[b] + (s + 1) * T + t``, s = the int32
    ``step`` tensor ON THE DEVICE, which this call only reads -- issue it BEFORE the step's ``rollout_score``.  heater_temp (B,) fp32 on the
    device.  Allocates nothing: capturable in a HIP graph."""
    rec, stream = _rollout_step_args("rollout_heatflux", pred, frames, first, step, table, steps)
    B, T, Cn = pred.shape[:3]
    _check_tensors("rollout_heatflux", pred.device, {"flux_pred": (flux_pred, (B, steps * T), torch.float32), "flux_tgt": (flux_tgt, (B, steps * T), torch.float32),
                                                     "heater_temp": (heater_temp, (B,), torch.float32)})
    if not (0 <= int(dfun_channel) < Cn and 0 <= int(temp_channel) < Cn):
        raise L.BubbleformerHipError(f"rollout_heatflux: channels {dfun_channel} / {temp_channel} are not among the prediction's {Cn}")
    L.check(L.lib().bf_rollout_heatflux(C.byref(rec), int(dfun_channel), int(temp_channel), _p(heater_temp), float(x_min), float(dx), float(lc),
                                        float(conductivity), _p(flux_pred), _p(flux_tgt), stream), "bf_rollout_heatflux")


def kde_kl_workspace(rows: int, n: int, m: int, points: int, device) -> torch.Tensor:
    """The fp64 workspace ``kde_kl`` needs (allocate once, outside a graph capture): O(points) per row, whatever n and m."""
    if int(rows) < 1 or int(n) < 2 or int(m) < 2 or int(points) < 3:
        raise L.BubbleformerHipError(f"kde_kl_workspace: needs rows >= 1, n >= 2, m >= 2, points >= 3 (got {rows}, {n}, {m}, {points})")
    return torch.empty(L.lib().bf_kde_kl_ws_doubles(int(rows), int(n), int(m), int(points)), dtype=torch.float64, device=device)


def kde_kl(p: torch.Tensor, q: torch.Tensor, points: int, eps: float, ws: torch.Tensor, kl: torch.Tensor, x: Optional[torch.Tensor] = None,
           pdf_p: Optional[torch.Tensor] = None, pdf_q: Optional[torch.Tensor] = None) -> None:
    """kl (R,) = KL(p || q) of the Gaussian KDEs of the rows of p (R, n) and q (R, m), fp64 on the device, by Simpson's rule on ``points``
    grid points (bf_kde_kl; include/bubbleformer_hip.h has the contract); optionally the grid and both densities (R, points).  Allocates nothing."""
    _require_gpu(p)
    if p.dim() != 2 or q.dim() != 2 or p.shape[0] != q.shape[0]:
        raise L.BubbleformerHipError(f"kde_kl: p and q must be (R, n) and (R, m), got {tuple(p.shape)} and {tuple(q.shape)}")
    R, n, m = int(p.shape[0]), int(p.shape[1]), int(q.shape[1])
    if n < 2 or m < 2 or int(points) < 3 or R < 1:
        raise L.BubbleformerHipError(f"kde_kl: needs at least 2 samples per set and 3 grid points (n = {n}, m = {m}, points = {points})")
    want = {"p": (p, (R, n)), "q": (q, (R, m)), "kl": (kl, (R,)), "x": (x, (R, points)), "pdf_p": (pdf_p, (R, points)), "pdf_q": (pdf_q, (R, points)),
            "ws": (ws, (ws.numel(),))}
    _check_tensors("kde_kl", p.device, {k: (t, shape, torch.float64) for k, (t, shape) in want.items()}, optional=("x", "pdf_p", "pdf_q"))
    if ws.numel() < L.lib().bf_kde_kl_ws_doubles(R, n, m, int(points)):
        raise L.BubbleformerHipError("kde_kl: the workspace is smaller than kde_kl_workspace(rows, n, m, points)")
    L.check(L.lib().bf_kde_kl(_p(p), _p(q), R, n, m, int(points), float(eps), _p(kl), _p(x), _p(pdf_p), _p(pdf_q), _p(ws), ws.numel(), _stream()),
            "bf_kde_kl")


def bubble_census_workspace(frames: int, H: int, W: int, max_bubbles: int, device) -> torch.Tensor:
    """The workspace ``bubble_census`` (and, with frames = 2 * B * T, ``rollout_bubbles``) needs: allocate once, outside a graph capture.  A frame
    larger than the library supports is refused here, before any launch."""
    nbytes = L.lib().bf_bubble_census_ws_bytes(int(frames), int(H), int(W), int(max_bubbles))
    if nbytes <= 0:
        raise L.BubbleformerHipError(f"bubble_census_workspace: {frames} frames of {H} x {W} with {max_bubbles} records are not supported "
                                     "(every size at least 1, at most 2^24 cells per frame)")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def bubble_census_lds_cells() -> int:
    """Frames of at most this many cells are labelled in LDS, larger ones in the workspace (bf_bubble_census_lds_cells)."""
    return int(L.lib().bf_bubble_census_lds_cells())


def bubble_census(phi: torch.Tensor, connectivity: int, max_bubbles: int, ws: torch.Tensor, count: torch.Tensor, vapour_cells: torch.Tensor,
                  attached: torch.Tensor, area: torch.Tensor, centroid: Optional[torch.Tensor] = None, on_heater: Optional[torch.Tensor] = None,
                  labels: Optional[torch.Tensor] = None) -> None:
    """The connected components of phi > 0 of every frame of phi (F, H, W) fp32 (bf_bubble_census; include/bubbleformer_hip.h has the contract):
    count / vapour_cells / attached (F,) int32, area (F, max_bubbles) int32, and optionally centroid (F, max_bubbles, 2) fp32, on_heater
    (F, max_bubbles) bool and the label image (F, H, W) int32.  Allocates nothing: capturable in a HIP graph."""
    _require_gpu(phi)
    if phi.dim() != 3 or phi.dtype != torch.float32 or not phi.is_contiguous():
        raise L.BubbleformerHipError("bubble_census: phi must be a contiguous fp32 (frames, H, W) tensor")
    F, H, W = phi.shape
    mb = int(max_bubbles)
    i32 = torch.int32
    _check_tensors("bubble_census", phi.device, {"count": (count, (F,), i32), "vapour_cells": (vapour_cells, (F,), i32), "attached": (attached, (F,), i32),
                   "area": (area, (F, mb), i32), "centroid": (centroid, (F, mb, 2), torch.float32), "on_heater": (on_heater, (F, mb), torch.bool),
                   "labels": (labels, (F, H, W), i32), "ws": (ws, (ws.numel(),), torch.uint8)}, ("centroid", "on_heater", "labels"))
    need = L.lib().bf_bubble_census_ws_bytes(F, H, W, mb)
    if need <= 0 or ws.numel() < need:
        raise L.BubbleformerHipError("bubble_census: the workspace is smaller than bubble_census_workspace(frames, H, W, max_bubbles)")
    L.check(L.lib().bf_bubble_census(_p(phi), F, H, W, int(connectivity), mb, _p(count), _p(vapour_cells), _p(attached), _p(area), _p(centroid),
                                     _p(on_heater), _p(labels), _p(ws), ws.numel(), _stream()), "bf_bubble_census")


def rollout_bubbles(pred: torch.Tensor, frames: torch.Tensor, first: torch.Tensor, step: torch.Tensor, table, sdf_channel: int, steps: int,
                    connectivity: int, max_bubbles: int, ws: torch.Tensor, count_pred: torch.Tensor, count_tgt: torch.Tensor, cells_pred: torch.Tensor,
                    cells_tgt: torch.Tensor, attached_pred: torch.Tensor, attached_tgt: torch.Tensor, area_pred: torch.Tensor,
                    area_tgt: torch.Tensor, labels: Optional[torch.Tensor] = None) -> None:
    """The bubble census of one rollout step (bf_rollout_bubbles; include/bubbleformer_hip.h has the contract): row s * T + t of the int32 outputs
    count / cells / attached (B, steps*T) and area (B, steps*T, max_bubbles), for the de-normalised signed-distance channel of the prediction
    (_pred) and for the stored frame ``first[b] + (s + 1) * T + t`` (_tgt), s = the int32 ``step`` tensor ON THE DEVICE, which this call only
    reads -- issue it BEFORE the step's ``rollout_score``.  labels: None, or the ring of ``rollout_bubbles_labelled``.  ws:
    ``bubble_census_workspace(2 * B * T, Ho, Wo, max_bubbles)``.  Allocates nothing."""
    _rollout_census("rollout_bubbles", (pred, frames, first, step, table, steps), sdf_channel, connectivity, max_bubbles, ws,
                    (count_pred, cells_pred, attached_pred, area_pred), (count_tgt, cells_tgt, attached_tgt, area_tgt), labels)


def _census_rows(who: str, device, side: str, lead: tuple, mb: int, count, cells, attached, area, need_cells: bool = True):
    """One side's census tensors, checked -> bf_census_rows; the link calls do not read cells, where need_cells = False lets it be None."""
    i32 = torch.int32
    want = {f"count{side}": (count, lead, i32), f"cells{side}": (cells, lead, i32), f"attached{side}": (attached, lead, i32), f"area{side}": (area, lead + (mb,), i32)}
    _check_tensors(who, device, want, () if need_cells else (f"cells{side}",))
    return L.CensusRows(count=_p(count), cells=_p(cells), attached=_p(attached), area=_p(area))


def _rollout_census(who: str, step_args: tuple, sdf_channel: int, connectivity: int, max_bubbles: int, ws: torch.Tensor, side_pred: tuple, side_tgt: tuple,
                    labels: Optional[torch.Tensor], need_labels: bool = False) -> None:
    """``rollout_bubbles`` and ``rollout_bubbles_labelled``: one entry point, with or without the ring."""
    rec, stream = _rollout_step_args(who, *step_args)
    pred, steps = step_args[0], step_args[-1]
    B, T, Cn, Ho, Wo = pred.shape
    mb = int(max_bubbles)
    census_pred = _census_rows(who, pred.device, "_pred", (B, steps * T), mb, *side_pred)
    census_tgt = _census_rows(who, pred.device, "_tgt", (B, steps * T), mb, *side_tgt)
    _check_tensors(who, pred.device, {"labels": (labels, (2, 2, B, T, Ho, Wo), torch.int32), "ws": (ws, (ws.numel(),), torch.uint8)},
                   () if need_labels else ("labels",))
    if not 0 <= int(sdf_channel) < Cn:
        raise L.BubbleformerHipError(f"{who}: channel {sdf_channel} is not among the prediction's {Cn}")
    need = L.lib().bf_bubble_census_ws_bytes(2 * B * T, Ho, Wo, mb)
    if need <= 0 or ws.numel() < need:
        raise L.BubbleformerHipError(f"{who}: the workspace is smaller than bubble_census_workspace(2 * B * T, Ho, Wo, max_bubbles)")
    L.check(L.lib().bf_rollout_bubbles(C.byref(rec), int(sdf_channel), int(connectivity), mb, C.byref(census_pred), C.byref(census_tgt), _p(labels), _p(ws),
                                       ws.numel(), stream), "bf_rollout_bubbles")


def redistance_workspace(frames: int, H: int, W: int, device) -> torch.Tensor:
    """The workspace ``redistance`` (and, with frames = B * T, ``rollout_redistance``) needs: allocate once, outside a graph capture.  It holds the
    distances of frames that do not fit ``redistance_lds_cells()``; a frame larger than the library supports is refused here, before any launch."""
    nbytes = L.lib().bf_redistance_ws_bytes(int(frames), int(H), int(W))
    if nbytes <= 0:
        raise L.BubbleformerHipError(f"redistance_workspace: {frames} frames of {H} x {W} are not supported (every size at least 1, at most 2^24 cells per frame)")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def redistance_lds_cells() -> int:
    """Frames of at most this many cells are redistanced in LDS, larger ones in the workspace (bf_redistance_lds_cells)."""
    return int(L.lib().bf_redistance_lds_cells())


def redistance(phi: torch.Tensor, dx: float, band: Optional[float], max_rounds: Optional[int], ws: torch.Tensor, out: torch.Tensor,
               rounds: Optional[torch.Tensor] = None, change_rms: Optional[torch.Tensor] = None) -> None:
    """out = the signed distance to the zero level set of every frame of phi (F, H, W) fp32 at spacing dx (bf_redistance;
    include/bubbleformer_hip.h has the contract); out may be phi.  band None: no cap; max_rounds None: H + W.  rounds (F,) int32 and
    change_rms (F,) fp32 are optional.  ws: ``redistance_workspace(F, H, W)``.  Allocates nothing: capturable in a HIP graph."""
    _require_gpu(phi)
    if phi.dim() != 3 or phi.dtype != torch.float32 or not phi.is_contiguous():
        raise L.BubbleformerHipError("redistance: phi must be a contiguous fp32 (frames, H, W) tensor")
    F, H, W = (int(v) for v in phi.shape)
    _check_tensors("redistance", phi.device, {"out": (out, (F, H, W), torch.float32), "rounds": (rounds, (F,), torch.int32),
                   "change_rms": (change_rms, (F,), torch.float32), "ws": (ws, (ws.numel(),), torch.uint8)}, ("rounds", "change_rms"))
    need = L.lib().bf_redistance_ws_bytes(F, H, W)
    if need <= 0 or ws.numel() < need:
        raise L.BubbleformerHipError("redistance: the workspace is smaller than redistance_workspace(frames, H, W)")
    L.check(L.lib().bf_redistance(_p(phi), F, H, W, float(dx), 0.0 if band is None else float(band), 0 if max_rounds is None else int(max_rounds),
                                  _p(out), _p(rounds), _p(change_rms), _p(ws), ws.numel(), _stream()), "bf_redistance")


def rollout_redistance(pred: torch.Tensor, frames: torch.Tensor, first: torch.Tensor, step: torch.Tensor, table, sdf_channel: int, steps: int,
                       dx: float, band: Optional[float], max_rounds: Optional[int], every: int, ws: torch.Tensor,
                       rounds: Optional[torch.Tensor] = None, change_rms: Optional[torch.Tensor] = None) -> None:
    """``redistance`` of the de-normalised signed-distance channel of one rollout step's prediction, written back IN PLACE and renormalised
    (bf_rollout_redistance; include/bubbleformer_hip.h has the contract), on the steps s with (s + 1) % every == 0, s = the int32 ``step`` tensor
    ON THE DEVICE, which this call only reads -- issue it BEFORE every other call of the step.  Row s * T + t of rounds (B, steps*T) int32 and
    change_rms (B, steps*T) fp32 (each optional).  ws: ``redistance_workspace(B * T, Ho, Wo)``.  Allocates nothing."""
    rec, stream = _rollout_step_args("rollout_redistance", pred, frames, first, step, table, steps)
    B, T, Cn, Ho, Wo = pred.shape
    _check_tensors("rollout_redistance", pred.device, {"rounds": (rounds, (B, steps * T), torch.int32), "change_rms": (change_rms, (B, steps * T), torch.float32),
                   "ws": (ws, (ws.numel(),), torch.uint8)}, ("rounds", "change_rms"))
    if not 0 <= int(sdf_channel) < Cn:
        raise L.BubbleformerHipError(f"rollout_redistance: channel {sdf_channel} is not among the prediction's {Cn}")
    need = L.lib().bf_redistance_ws_bytes(B * T, Ho, Wo)
    if need <= 0 or ws.numel() < need:
        raise L.BubbleformerHipError("rollout_redistance: the workspace is smaller than redistance_workspace(B * T, Ho, Wo)")
    L.check(L.lib().bf_rollout_redistance(C.byref(rec), int(sdf_channel), float(dx), 0.0 if band is None else float(band),
                                          0 if max_rounds is None else int(max_rounds), int(every), _p(pred), _p(rounds), _p(change_rms), _p(ws),
                                          ws.numel(), stream), "bf_rollout_redistance")


def bubble_links_workspace(pairs: int, max_bubbles: int, device) -> torch.Tensor:
    """The workspace ``bubble_links`` (and, with pairs = 2 * B * T, ``rollout_bubble_links``) needs: allocate once, outside a graph capture.  It holds
    the overlap tables that do not fit ``bubble_links_lds_entries()``; more records than the library supports are refused here, before any launch."""
    nbytes = L.lib().bf_bubble_links_ws_bytes(int(pairs), int(max_bubbles))
    if nbytes <= 0:
        raise L.BubbleformerHipError(f"bubble_links_workspace: {pairs} pairs with {max_bubbles} records are not supported (at least one pair, "
                                     "1 to 2^15 records per frame)")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def bubble_links_lds_entries() -> int:
    """A pair whose overlap table min(count_a, max_bubbles) x min(count_b, max_bubbles) has at most this many entries keeps it in LDS, a larger
    one in the workspace (bf_bubble_links_lds_entries)."""
    return int(L.lib().bf_bubble_links_lds_entries())


def _link_rows(lead: tuple, mb: int) -> dict:
    """name -> shape of the six outputs of a link call whose pair axes are ``lead``."""
    return {"successor": lead + (mb,), "n_successors": lead + (mb,), "predecessor": lead + (mb,), "n_predecessors": lead + (mb,),
            "departure_area": lead + (mb,), "events": lead + (5,)}


def _link_record(who: str, device, side: str, lead: tuple, mb: int, given: dict):
    """One side's six link tensors (``_link_rows(lead, mb)``), checked -> bf_link_rows."""
    shapes = _link_rows(lead, mb)
    if given.keys() != shapes.keys():
        raise L.BubbleformerHipError(f"{who}: links{side} must hold exactly {sorted(shapes)}")
    _check_tensors(who, device, {f"{k}{side}": (given[k], shape, torch.int32) for k, shape in shapes.items()})
    return L.LinkRows(**{k: _p(given[k]) for k in shapes})


def bubble_links(labels: torch.Tensor, count: torch.Tensor, attached: torch.Tensor, area: torch.Tensor, ws: torch.Tensor, successor: torch.Tensor,
                 n_successors: torch.Tensor, predecessor: torch.Tensor, n_predecessors: torch.Tensor, departure_area: torch.Tensor,
                 events: torch.Tensor) -> None:
    """The links between the consecutive frames of N sequences (bf_bubble_links; include/bubbleformer_hip.h has the contract): labels (N, T, H, W),
    count / attached (N, T) and area (N, T, max_bubbles) int32 as ``bubble_census`` left them -> successor, n_successors, predecessor,
    n_predecessors, departure_area (N, T - 1, max_bubbles) and events (N, T - 1, 5) int32.  T = 1 launches nothing.  ws:
    ``bubble_links_workspace(N * (T - 1), max_bubbles)``.  Allocates nothing: capturable in a HIP graph."""
    _require_gpu(labels)
    i32 = torch.int32
    if labels.dim() != 4 or labels.dtype != i32 or not labels.is_contiguous():
        raise L.BubbleformerHipError("bubble_links: labels must be a contiguous int32 (sequences, T, H, W) tensor")
    if area.dim() != 3:
        raise L.BubbleformerHipError("bubble_links: area must be a (sequences, T, max_bubbles) tensor")
    N, T, H, W = labels.shape
    mb = int(area.shape[-1])
    census = _census_rows("bubble_links", labels.device, "", (N, T), mb, count, None, attached, area, need_cells=False)
    _check_tensors("bubble_links", labels.device, {"ws": (ws, (ws.numel(),), torch.uint8)})
    links = _link_record("bubble_links", labels.device, "", (N, T - 1), mb, dict(successor=successor, n_successors=n_successors, predecessor=predecessor,
                         n_predecessors=n_predecessors, departure_area=departure_area, events=events))
    if N < 1 or T < 1 or H < 1 or W < 1 or mb < 1:
        raise L.BubbleformerHipError(f"bubble_links: needs at least one sequence of at least one frame of at least one cell, got {tuple(labels.shape)}")
    if T == 1:
        return
    need = L.lib().bf_bubble_links_ws_bytes(N * (T - 1), mb)
    if need <= 0 or ws.numel() < need:
        raise L.BubbleformerHipError("bubble_links: the workspace is smaller than bubble_links_workspace(sequences * (T - 1), max_bubbles)")
    L.check(L.lib().bf_bubble_links(_p(labels), C.byref(census), N, T, H, W, mb, C.byref(links), _p(ws), ws.numel(), _stream()), "bf_bubble_links")


def bubble_track_ids(count: torch.Tensor, successor: torch.Tensor, predecessor: torch.Tensor, track_id: torch.Tensor, n_tracks: torch.Tensor) -> None:
    """Track ids of N sequences from their links (bf_bubble_track_ids; include/bubbleformer_hip.h has the contract): count (N, T), successor /
    predecessor (N, T - 1, max_bubbles) int32 -> track_id (N, T, max_bubbles), 0 in unused slots, and n_tracks (N,) int32.  Allocates nothing."""
    _require_gpu(count)
    i32 = torch.int32
    if count.dim() != 2 or track_id.dim() != 3:
        raise L.BubbleformerHipError("bubble_track_ids: count must be (sequences, T) and track_id (sequences, T, max_bubbles)")
    N, T = count.shape
    mb = int(track_id.shape[-1])
    _check_tensors("bubble_track_ids", count.device, {"count": (count, (N, T), i32), "successor": (successor, (N, T - 1, mb), i32),
                   "predecessor": (predecessor, (N, T - 1, mb), i32), "track_id": (track_id, (N, T, mb), i32), "n_tracks": (n_tracks, (N,), i32)})
    if N < 1 or T < 1 or mb < 1:
        raise L.BubbleformerHipError(f"bubble_track_ids: needs at least one sequence, one frame and one record, got {tuple(track_id.shape)}")
    L.check(L.lib().bf_bubble_track_ids(_p(count), _p(successor) if T > 1 else None, _p(predecessor) if T > 1 else None, N, T, mb, _p(track_id),
                                        _p(n_tracks), _stream()), "bf_bubble_track_ids")


def rollout_bubbles_labelled(pred: torch.Tensor, frames: torch.Tensor, first: torch.Tensor, step: torch.Tensor, table, sdf_channel: int, steps: int,
                             connectivity: int, max_bubbles: int, ws: torch.Tensor, count_pred: torch.Tensor, count_tgt: torch.Tensor,
                             cells_pred: torch.Tensor, cells_tgt: torch.Tensor, attached_pred: torch.Tensor, attached_tgt: torch.Tensor,
                             area_pred: torch.Tensor, area_tgt: torch.Tensor, labels: torch.Tensor) -> None:
    """``rollout_bubbles`` that also leaves its label images (bf_rollout_bubbles with the ring): labels (2, 2, B, T, Ho, Wo) int32 is a ring of two
    steps, [0] the prediction and [1] the simulation; step s writes half ``s & 1`` and leaves the other, which ``rollout_bubble_links`` still needs.
    Everything else as ``rollout_bubbles``.  Allocates nothing."""
    _rollout_census("rollout_bubbles_labelled", (pred, frames, first, step, table, steps), sdf_channel, connectivity, max_bubbles, ws,
                    (count_pred, cells_pred, attached_pred, area_pred), (count_tgt, cells_tgt, attached_tgt, area_tgt), labels, need_labels=True)


def rollout_bubble_links(pred: torch.Tensor, frames: torch.Tensor, first: torch.Tensor, step: torch.Tensor, table, steps: int, max_bubbles: int,
                         ws: torch.Tensor, labels: torch.Tensor, count_pred: torch.Tensor, count_tgt: torch.Tensor, attached_pred: torch.Tensor,
                         attached_tgt: torch.Tensor, area_pred: torch.Tensor, area_tgt: torch.Tensor, links_pred: dict, links_tgt: dict) -> None:
    """The links of one rollout step (bf_rollout_bubble_links; include/bubbleformer_hip.h has the contract), on the ring and the census rows the
    step's ``rollout_bubbles_labelled`` wrote: per side and trajectory the pairs that end in a frame of step s = the int32 ``step`` tensor ON THE
    DEVICE, which this call only reads -- issue it after ``rollout_bubbles_labelled`` and BEFORE the step's ``rollout_score``.  links_pred /
    links_tgt: dicts of successor, n_successors, predecessor, n_predecessors, departure_area (B, steps*T - 1, max_bubbles) and events
    (B, steps*T - 1, 5) int32; the pair that ends in frame t of step s is row s * T + t - 1.  ws: ``bubble_links_workspace(2 * B * T, max_bubbles)``.
    A rollout of one frame (steps * T = 1) has no pair and launches nothing.  Allocates nothing."""
    rec, stream = _rollout_step_args("rollout_bubble_links", pred, frames, first, step, table, steps)
    B, T, Cn, Ho, Wo = pred.shape
    mb, dev = int(max_bubbles), pred.device
    _check_tensors("rollout_bubble_links", dev, {"labels": (labels, (2, 2, B, T, Ho, Wo), torch.int32), "ws": (ws, (ws.numel(),), torch.uint8)})
    census_pred = _census_rows("rollout_bubble_links", dev, "_pred", (B, steps * T), mb, count_pred, None, attached_pred, area_pred, need_cells=False)
    census_tgt = _census_rows("rollout_bubble_links", dev, "_tgt", (B, steps * T), mb, count_tgt, None, attached_tgt, area_tgt, need_cells=False)
    rows_pred = _link_record("rollout_bubble_links", dev, "_pred", (B, steps * T - 1), mb, links_pred)
    rows_tgt = _link_record("rollout_bubble_links", dev, "_tgt", (B, steps * T - 1), mb, links_tgt)
    need = L.lib().bf_bubble_links_ws_bytes(2 * B * T, mb)
    if need <= 0 or ws.numel() < need:
        raise L.BubbleformerHipError("rollout_bubble_links: the workspace is smaller than bubble_links_workspace(2 * B * T, max_bubbles)")
    if steps * T < 2:
        return
    L.check(L.lib().bf_rollout_bubble_links(C.byref(rec), mb, _p(labels), C.byref(census_pred), C.byref(census_tgt), C.byref(rows_pred), C.byref(rows_tgt),
                                            _p(ws), ws.numel(), stream), "bf_rollout_bubble_links")


def bubble_match_workspace(pairs: int, max_bubbles: int, device) -> torch.Tensor:
    """The workspace ``bubble_match`` (and, with pairs = B * T, ``rollout_bubble_match``) needs: allocate once, outside a graph capture.  It holds
    every pair's centroid sums and best-partner rows, and the overlap tables that do not fit ``bubble_links_lds_entries()``; more records than the
    library supports are refused here, before any launch."""
    nbytes = L.lib().bf_bubble_match_ws_bytes(int(pairs), int(max_bubbles))
    if nbytes <= 0:
        raise L.BubbleformerHipError(f"bubble_match_workspace: {pairs} pairs with {max_bubbles} records are not supported (at least one pair, "
                                     "1 to 2^15 records per frame)")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _match_rows(lead: tuple, mb: int) -> dict:
    """name -> (shape, dtype) of the six outputs of a match call whose pair axes are ``lead``."""
    i32 = torch.int32
    return {"match_pred": (lead + (mb,), i32), "match_target": (lead + (mb,), i32), "overlap": (lead + (mb,), i32),
            "displacement": (lead + (mb,), torch.float32), "counts": (lead + (6,), i32), "mask": (lead + (2,), i32)}


def _match_record(who: str, device, lead: tuple, mb: int, given: dict):
    """The six match tensors (``_match_rows(lead, mb)``), checked -> bf_match_rows."""
    shapes = _match_rows(lead, mb)
    if given.keys() != shapes.keys():
        raise L.BubbleformerHipError(f"{who}: rows must hold exactly {sorted(shapes)}")
    _check_tensors(who, device, {k: (given[k], shape, dtype) for k, (shape, dtype) in shapes.items()})
    return L.MatchRows(**{k: _p(given[k]) for k in shapes})


def _check_min_iou(who: str, min_iou) -> float:
    if not 0.0 <= float(min_iou) <= 1.0:                    # a NaN fails both comparisons
        raise L.BubbleformerHipError(f"{who}: min_iou must be in [0, 1], got {min_iou!r}")
    return float(min_iou)


def bubble_match(labels_pred: torch.Tensor, labels_tgt: torch.Tensor, count_pred: torch.Tensor, count_tgt: torch.Tensor, attached_pred: torch.Tensor,
                 attached_tgt: torch.Tensor, area_pred: torch.Tensor, area_tgt: torch.Tensor, min_iou: float, ws: torch.Tensor, rows: dict) -> None:
    """Predicted bubbles matched to simulated ones, frame by frame (bf_bubble_match; include/bubbleformer_hip.h has the contract): labels (F, H, W),
    count / attached (F,) and area (F, max_bubbles) int32 of both sides as ``bubble_census`` left them -> rows: a dict of match_pred, match_target,
    overlap (F, max_bubbles) int32, displacement (F, max_bubbles) fp32, counts (F, 6) and mask (F, 2) int32.  ws:
    ``bubble_match_workspace(F, max_bubbles)``.  Allocates nothing: capturable in a HIP graph."""
    _require_gpu(labels_pred)
    i32 = torch.int32
    if labels_pred.dim() != 3 or labels_pred.dtype != i32 or not labels_pred.is_contiguous():
        raise L.BubbleformerHipError("bubble_match: labels_pred must be a contiguous int32 (frames, H, W) tensor")
    if area_pred.dim() != 2:
        raise L.BubbleformerHipError("bubble_match: area_pred must be a (frames, max_bubbles) tensor")
    F, H, W = (int(v) for v in labels_pred.shape)
    mb, dev = int(area_pred.shape[-1]), labels_pred.device
    _check_tensors("bubble_match", dev, {"labels_tgt": (labels_tgt, (F, H, W), i32), "ws": (ws, (ws.numel(),), torch.uint8)})
    census_pred = _census_rows("bubble_match", dev, "_pred", (F,), mb, count_pred, None, attached_pred, area_pred, need_cells=False)
    census_tgt = _census_rows("bubble_match", dev, "_tgt", (F,), mb, count_tgt, None, attached_tgt, area_tgt, need_cells=False)
    record = _match_record("bubble_match", dev, (F,), mb, rows)
    if F < 1 or H < 1 or W < 1 or mb < 1:
        raise L.BubbleformerHipError(f"bubble_match: needs at least one frame of at least one cell and one record, got {tuple(labels_pred.shape)}")
    min_iou = _check_min_iou("bubble_match", min_iou)
    need = L.lib().bf_bubble_match_ws_bytes(F, mb)
    if need <= 0 or ws.numel() < need:
        raise L.BubbleformerHipError("bubble_match: the workspace is smaller than bubble_match_workspace(frames, max_bubbles)")
    L.check(L.lib().bf_bubble_match(_p(labels_pred), _p(labels_tgt), C.byref(census_pred), C.byref(census_tgt), F, H, W, mb, min_iou, C.byref(record),
                                    _p(ws), ws.numel(), _stream()), "bf_bubble_match")


def rollout_bubble_match(pred: torch.Tensor, frames: torch.Tensor, first: torch.Tensor, step: torch.Tensor, table, steps: int, max_bubbles: int,
                         min_iou: float, ws: torch.Tensor, labels: torch.Tensor, count_pred: torch.Tensor, count_tgt: torch.Tensor,
                         attached_pred: torch.Tensor, attached_tgt: torch.Tensor, area_pred: torch.Tensor, area_tgt: torch.Tensor, rows: dict) -> None:
    """The matches of one rollout step (bf_rollout_bubble_match; include/bubbleformer_hip.h has the contract), on the ring and the census rows the
    step's ``rollout_bubbles_labelled`` wrote: the predicted frame (b, t) against the simulated one, s = the int32 ``step`` tensor ON THE DEVICE,
    which this call only reads -- issue it after ``rollout_bubbles_labelled`` and BEFORE the step's ``rollout_score``.  rows: a dict of
    match_pred, match_target, overlap (B, steps*T, max_bubbles) int32, displacement (B, steps*T, max_bubbles) fp32, counts (B, steps*T, 6) and
    mask (B, steps*T, 2) int32; the call writes row s * T + t.  ws: ``bubble_match_workspace(B * T, max_bubbles)``.  Allocates nothing."""
    rec, stream = _rollout_step_args("rollout_bubble_match", pred, frames, first, step, table, steps)
    B, T, Cn, Ho, Wo = pred.shape
    mb, dev = int(max_bubbles), pred.device
    _check_tensors("rollout_bubble_match", dev, {"labels": (labels, (2, 2, B, T, Ho, Wo), torch.int32), "ws": (ws, (ws.numel(),), torch.uint8)})
    census_pred = _census_rows("rollout_bubble_match", dev, "_pred", (B, steps * T), mb, count_pred, None, attached_pred, area_pred, need_cells=False)
    census_tgt = _census_rows("rollout_bubble_match", dev, "_tgt", (B, steps * T), mb, count_tgt, None, attached_tgt, area_tgt, need_cells=False)
    record = _match_record("rollout_bubble_match", dev, (B, steps * T), mb, rows)
    min_iou = _check_min_iou("rollout_bubble_match", min_iou)
    need = L.lib().bf_bubble_match_ws_bytes(B * T, mb)
    if need <= 0 or ws.numel() < need:
        raise L.BubbleformerHipError("rollout_bubble_match: the workspace is smaller than bubble_match_workspace(B * T, max_bubbles)")
    L.check(L.lib().bf_rollout_bubble_match(C.byref(rec), mb, min_iou, _p(labels), C.byref(census_pred), C.byref(census_tgt), C.byref(record), _p(ws),
                                            ws.numel(), stream), "bf_rollout_bubble_match")


_ERROR_ROWS = ("rmse", "max_error", "boundary_rmse", "interface_rmse", "interface_cells", "spectral_error", "spectrum_error", "spectrum_pred",
               "spectrum_target")


def field_errors_workspace(frames: int, H: int, W: int, device) -> torch.Tensor:
    """The workspace ``field_errors`` (and, with frames = B * T * C, ``rollout_errors``) needs: allocate once, outside a graph capture.  It holds the
    fp64 row-to-column intermediate of the transforms; a side above 1024 is refused here, before any launch."""
    nbytes = L.lib().bf_field_errors_ws_bytes(int(frames), int(H), int(W))
    if nbytes <= 0:
        raise L.BubbleformerHipError(f"field_errors_workspace: {frames} frames of {H} x {W} are not supported (at least one frame, sides from 1 to 1024)")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _error_rows(who: str, device, lead: tuple, K: int, rows: dict, ws: torch.Tensor):
    """The nine optional outputs of the error calls, checked -> bf_error_rows."""
    unknown = set(rows) - set(_ERROR_ROWS)
    if unknown:
        raise L.BubbleformerHipError(f"{who}: unknown outputs {sorted(unknown)}")
    f32 = torch.float32
    shapes = {"rmse": (lead, f32), "max_error": (lead, f32), "boundary_rmse": (lead, f32), "interface_rmse": (lead, f32),
              "interface_cells": (lead, torch.int32), "spectral_error": (lead + (3,), f32), "spectrum_error": (lead + (K,), f32),
              "spectrum_pred": (lead + (K,), f32), "spectrum_target": (lead + (K,), f32)}
    want = {k: (rows.get(k), shape, dtype) for k, (shape, dtype) in shapes.items()}
    want["ws"] = (ws, (ws.numel(),), torch.uint8)
    _check_tensors(who, device, want, _ERROR_ROWS)
    return L.ErrorRows(**{k: _p(rows.get(k)) for k in _ERROR_ROWS})


def shell_count(H: int, W: int) -> int:
    """K = isqrt(S * S // 2) + 1 shells for S = min(H, W): every mode of an H x W frame falls in one of them."""
    import math
    S = min(int(H), int(W))
    return math.isqrt(S * S // 2) + 1


def field_errors(pred: torch.Tensor, target: torch.Tensor, sdf: Optional[torch.Tensor], ws: torch.Tensor, interface_radius: int = 1, lo: int = 4,
                 hi: int = 12, want_spectra: bool = True, **rows: Optional[torch.Tensor]) -> None:
    """The error rows of pred against target (F, H, W) fp32 (bf_field_errors; include/bubbleformer_hip.h has the contract); sdf (F, H, W) fp32 in
    physical units or None.  rows: any of rmse, max_error, boundary_rmse, interface_rmse (F,) fp32, interface_cells (F,) int32, spectral_error
    (F, 3), spectrum_error / spectrum_pred / spectrum_target (F, shell_count(H, W)) fp32; what is left out is not computed.  ws:
    ``field_errors_workspace(F, H, W)``.  Allocates nothing: capturable in a HIP graph."""
    _require_gpu(pred)
    if pred.dim() != 3 or pred.dtype != torch.float32 or not pred.is_contiguous():
        raise L.BubbleformerHipError("field_errors: pred must be a contiguous fp32 (frames, H, W) tensor")
    F, H, W = pred.shape
    _check_tensors("field_errors", pred.device, {"target": (target, (F, H, W), torch.float32), "sdf": (sdf, (F, H, W), torch.float32)}, ("sdf",))
    rec = _error_rows("field_errors", pred.device, (F,), shell_count(H, W), rows, ws)
    need = L.lib().bf_field_errors_ws_bytes(F, H, W)
    if need <= 0 or ws.numel() < need:
        raise L.BubbleformerHipError("field_errors: the workspace is smaller than field_errors_workspace(frames, H, W)")
    L.check(L.lib().bf_field_errors(_p(pred), _p(target), _p(sdf), F, H, W, int(interface_radius), int(lo), int(hi), int(bool(want_spectra)),
                                    C.byref(rec), _p(ws), ws.numel(), _stream()), "bf_field_errors")


def rollout_errors(pred: torch.Tensor, frames: torch.Tensor, first: torch.Tensor, step: torch.Tensor, table, sdf_channel: int, steps: int,
                   ws: torch.Tensor, interface_radius: int = 1, lo: int = 4, hi: int = 12, want_spectra: bool = True,
                   **rows: Optional[torch.Tensor]) -> None:
    """The error rows of one rollout step (bf_rollout_errors; include/bubbleformer_hip.h has the contract): rows (b, s * T + t, c) of the outputs
    ``field_errors`` names, here (B, steps*T, C) with the same tails, for the prediction against the stored frame ``first[b] + (s + 1) * T + t``,
    s = the int32 ``step`` tensor ON THE DEVICE, which this call only reads -- issue it BEFORE the step's ``rollout_score``.  The interface mask
    comes from the raw stored frame of ``sdf_channel`` (-1: none).  ws: ``field_errors_workspace(B * T * C, Ho, Wo)``.  Allocates nothing."""
    rec, stream = _rollout_step_args("rollout_errors", pred, frames, first, step, table, steps)
    B, T, Cn, Ho, Wo = pred.shape
    out = _error_rows("rollout_errors", pred.device, (B, steps * T, Cn), shell_count(Ho, Wo), rows, ws)
    if not -1 <= int(sdf_channel) < Cn:
        raise L.BubbleformerHipError(f"rollout_errors: channel {sdf_channel} is not among the prediction's {Cn}")
    need = L.lib().bf_field_errors_ws_bytes(B * T * Cn, Ho, Wo)
    if need <= 0 or ws.numel() < need:
        raise L.BubbleformerHipError("rollout_errors: the workspace is smaller than field_errors_workspace(B * T * C, Ho, Wo)")
    L.check(L.lib().bf_rollout_errors(C.byref(rec), int(sdf_channel), int(interface_radius), int(lo), int(hi), int(bool(want_spectra)), C.byref(out), _p(ws),
                                      ws.numel(), stream), "bf_rollout_errors")


_ENSEMBLE_ROWS = ("mean_rmse", "spread", "crps", "rank_hist", "mean")


def ensemble_workspace(frames: int, members: int, H: int, W: int, device) -> torch.Tensor:
    """The workspace ``ensemble_scores`` (and, with frames = Bt * T * C, ``rollout_ensemble``) needs: allocate once, outside a graph capture.  It
    holds the fp64 and int32 partials of every workgroup; a member count outside 2 .. 32 is refused here, before any launch."""
    nbytes = L.lib().bf_ensemble_scores_ws_bytes(int(frames), int(members), int(H), int(W))
    if nbytes <= 0:
        raise L.BubbleformerHipError(f"ensemble_workspace: {frames} frames of {H} x {W} with {members} members are not supported (2 to 32 members, at "
                                     "least one frame of at least one pixel)")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _ensemble_rows(who: str, device, lead: tuple, members: int, H: int, W: int, rows: dict, ws: torch.Tensor):
    """The outputs of the ensemble calls by name, checked -> bf_ensemble_rows: mean_rmse, spread and crps are required, rank_hist and mean optional."""
    unknown = set(rows) - set(_ENSEMBLE_ROWS)
    if unknown:
        raise L.BubbleformerHipError(f"{who}: unknown outputs {sorted(unknown)}")
    f32 = torch.float32
    shapes = {"mean_rmse": (lead, f32), "spread": (lead, f32), "crps": (lead, f32), "rank_hist": (lead + (members + 1,), torch.int32),
              "mean": (lead + (H, W), f32)}
    want = {k: (rows.get(k), shape, dtype) for k, (shape, dtype) in shapes.items()}
    want["ws"] = (ws, (ws.numel(),), torch.uint8)
    _check_tensors(who, device, want, ("rank_hist", "mean"))
    return L.EnsembleRows(**{k: _p(rows.get(k)) for k in _ENSEMBLE_ROWS})


def ensemble_scores(members: torch.Tensor, target: torch.Tensor, ws: torch.Tensor, fair: bool = False, **rows: Optional[torch.Tensor]) -> None:
    """The statistics across the members of an ensemble, per frame (bf_ensemble_scores; include/bubbleformer_hip.h has the contract): members
    (M, F, H, W) fp32 whose member blocks are contiguous (``members.stride(0)`` may exceed F * H * W: it is the call's member_stride) against target
    (F, H, W) fp32.  rows: mean_rmse, spread, crps (F,) fp32, and optionally rank_hist (F, M + 1) int32 and mean (F, H, W) fp32.  ws:
    ``ensemble_workspace(F, M, H, W)``.  Allocates nothing: capturable in a HIP graph."""
    _require_gpu(members)
    if members.dim() != 4 or members.dtype != torch.float32 or not members[0].is_contiguous() or (members.shape[0] > 1 and members.stride(0) < members[0].numel()):
        raise L.BubbleformerHipError("ensemble_scores: members must be an fp32 (M, frames, H, W) tensor of contiguous member blocks")
    M, F, H, W = members.shape
    _check_tensors("ensemble_scores", members.device, {"target": (target, (F, H, W), torch.float32)})
    rec = _ensemble_rows("ensemble_scores", members.device, (F,), M, H, W, rows, ws)
    need = L.lib().bf_ensemble_scores_ws_bytes(F, M, H, W)
    if need <= 0 or ws.numel() < need:
        raise L.BubbleformerHipError("ensemble_scores: 2 to 32 members, and a workspace of ensemble_workspace(frames, members, H, W)")
    L.check(L.lib().bf_ensemble_scores(_p(members), members.stride(0), _p(target), F, M, H, W, int(bool(fair)), C.byref(rec), _p(ws), ws.numel(),
                                       _stream()), "bf_ensemble_scores")


def rollout_ensemble(pred: torch.Tensor, frames: torch.Tensor, first: torch.Tensor, step: torch.Tensor, table, steps: int, members: int,
                     ws: torch.Tensor, fair: bool = False, **rows: Optional[torch.Tensor]) -> None:
    """The ensemble rows of one rollout step (bf_rollout_ensemble; include/bubbleformer_hip.h has the contract): pred (M * Bt, T, C, Ho, Wo) holds the
    members as row blocks, member-major; rows (b, s * T + t, c) of mean_rmse / spread / crps (Bt, steps*T, C), rank_hist (.., M + 1) and mean
    (.., Ho, Wo) are written against the stored frame ``first[b] + (s + 1) * T + t``, s = the int32 ``step`` tensor ON THE DEVICE, which this call
    only reads -- issue it BEFORE the step's ``rollout_score``.  ws: ``ensemble_workspace(Bt * T * C, M, Ho, Wo)``.  Allocates nothing."""
    rec, stream = _rollout_step_args("rollout_ensemble", pred, frames, first, step, table, steps)
    B, T, Cn, Ho, Wo = pred.shape
    M = int(members)
    if not 2 <= M <= 32 or B % M:
        raise L.BubbleformerHipError(f"rollout_ensemble: {M} members (2 to 32) must divide the prediction's {B} rows")
    Bt = B // M
    out = _ensemble_rows("rollout_ensemble", pred.device, (Bt, steps * T, Cn), M, Ho, Wo, rows, ws)
    need = L.lib().bf_ensemble_scores_ws_bytes(Bt * T * Cn, M, Ho, Wo)
    if need <= 0 or ws.numel() < need:
        raise L.BubbleformerHipError("rollout_ensemble: the workspace is smaller than ensemble_workspace(Bt * T * C, members, Ho, Wo)")
    L.check(L.lib().bf_rollout_ensemble(C.byref(rec), M, int(bool(fair)), C.byref(out), _p(ws), ws.numel(), stream), "bf_rollout_ensemble")


_FLOW_FRAME_ROWS = ("divergence_rms", "kinetic_energy", "enstrophy", "bulk_cells")
_FLOW_PAIR_ROWS = ("transport_rms", "interface_speed_rms", "transport_cells")
_FLOW_ROWS = _FLOW_FRAME_ROWS + _FLOW_PAIR_ROWS


def _flow_rows(who: str, device, frame_lead: tuple, pair_lead: tuple, rows: dict):
    """The seven optional outputs of the flow calls, checked -> bf_flow_rows: the frame rows of shape frame_lead, the pair rows of pair_lead."""
    unknown = set(rows) - set(_FLOW_ROWS)
    if unknown:
        raise L.BubbleformerHipError(f"{who}: unknown outputs {sorted(unknown)}")
    dtype = lambda k: torch.int32 if k.endswith("_cells") else torch.float32
    want = {k: (rows.get(k), frame_lead if k in _FLOW_FRAME_ROWS else pair_lead, dtype(k)) for k in _FLOW_ROWS}
    _check_tensors(who, device, want, _FLOW_ROWS)
    return L.FlowRows(**{k: _p(rows.get(k)) for k in _FLOW_ROWS})


def flow_consistency(sdf: torch.Tensor, velx: torch.Tensor, vely: torch.Tensor, dx: float, dt: float, band: float, interface_radius: int = 1,
                     **rows: Optional[torch.Tensor]) -> None:
    """Do a signed-distance field and a velocity agree with each other (bf_flow_consistency; include/bubbleformer_hip.h has the contract)?  sdf, velx,
    vely (S, T, H, W) fp32 in physical units, H and W from 3 to 1024.  rows: any of divergence_rms, kinetic_energy, enstrophy (S, T) fp32, bulk_cells
    (S, T) int32, transport_rms, interface_speed_rms (S, T - 1) fp32 and transport_cells (S, T - 1) int32, row t - 1 the pair that ends in frame t;
    what is left out is not computed.  No workspace; allocates nothing: capturable in a HIP graph."""
    _require_gpu(sdf)
    if sdf.dim() != 4 or sdf.dtype != torch.float32 or not sdf.is_contiguous():
        raise L.BubbleformerHipError("flow_consistency: sdf must be a contiguous fp32 (sequences, T, H, W) tensor")
    S, T, H, W = (int(v) for v in sdf.shape)
    _check_tensors("flow_consistency", sdf.device, {"velx": (velx, (S, T, H, W), torch.float32), "vely": (vely, (S, T, H, W), torch.float32)})
    rec = _flow_rows("flow_consistency", sdf.device, (S, T), (S, T - 1), rows)
    L.check(L.lib().bf_flow_consistency(_p(sdf), _p(velx), _p(vely), S, T, H, W, float(dx), float(dt), float(band), int(interface_radius), C.byref(rec),
                                        _stream()), "bf_flow_consistency")


def rollout_flow(pred: torch.Tensor, frames: torch.Tensor, first: torch.Tensor, step: torch.Tensor, table, channels, steps: int, dx: float, dt: float,
                 band: float, interface_radius: int, carry: torch.Tensor, rows_pred: dict, rows_target: dict) -> None:
    """The flow-consistency rows of one rollout step (bf_rollout_flow; include/bubbleformer_hip.h has the contract), of the de-normalised prediction
    (rows_pred) and of the stored frames ``first[b] + (s + 1) * T + t`` (rows_target): ``flow_consistency``'s frame rows at row s * T + t of
    (B, steps*T), its pair rows at row s * T + t - 1 of (B, steps*T - 1), s = the int32 ``step`` tensor ON THE DEVICE, which this call only reads --
    issue it BEFORE the step's ``rollout_score`` and after ``rollout_redistance``.  channels = (sdf, velx, vely) among the prediction's channels;
    carry (2, B, 3, Ho, Wo) fp32 hands the step's last predicted frame to the next step's call and belongs to these calls alone.  Allocates nothing."""
    rec, stream = _rollout_step_args("rollout_flow", pred, frames, first, step, table, steps)
    B, T, Cn, Ho, Wo = pred.shape
    _check_tensors("rollout_flow", pred.device, {"carry": (carry, (2, B, 3, Ho, Wo), torch.float32)})
    sides = [_flow_rows("rollout_flow", pred.device, (B, steps * T), (B, steps * T - 1), rows) for rows in (rows_pred, rows_target)]
    sdf_c, velx_c, vely_c = (int(c) for c in channels)
    if not all(0 <= c < Cn for c in (sdf_c, velx_c, vely_c)):
        raise L.BubbleformerHipError(f"rollout_flow: channels {(sdf_c, velx_c, vely_c)} are not among the prediction's {Cn}")
    L.check(L.lib().bf_rollout_flow(C.byref(rec), sdf_c, velx_c, vely_c, float(dx), float(dt), float(band), int(interface_radius), _p(carry),
                                    C.byref(sides[0]), C.byref(sides[1]), stream), "bf_rollout_flow")


def grad_norm_workspace(n: int, device) -> torch.Tensor:
    """The fp64 slab partials of grad_norm_ for a buffer of n elements (at most 1024 doubles)."""
    return torch.empty(int(L.lib().bf_grad_norm_ws_doubles(int(n))), dtype=torch.float64, device=device)


def grad_norm_(grad: torch.Tensor, out: torch.Tensor, max_norm: float, grad_scale: float = 1.0, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[0] = grad_scale * ||grad||_2, out[1] = min(max_norm / (out[0] + 1e-6), 1): the norm and the clip coefficient of
    torch.nn.utils.clip_grad_norm_ over a flat fp32 gradient buffer, left in device memory (`out`: two fp32) for the optimizers'
    ``coef=``.  fp64 sums in a fixed order (csrc/gradclip.hip): the same bits on every call.  ws: grad_norm_workspace(grad.numel(),
    device), allocated per call when None."""
    _require_gpu(grad)
    if grad.dtype != torch.float32 or not grad.is_contiguous() or grad.dim() != 1:
        raise L.BubbleformerHipError("grad_norm_: grad must be a contiguous 1-D torch.float32 tensor")
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != 2 or out.device != grad.device:
        raise L.BubbleformerHipError(f"grad_norm_: out must be a contiguous torch.float32 tensor of 2 elements on {grad.device}")
    if ws is None:
        ws = grad_norm_workspace(grad.numel(), grad.device)
    elif ws.dtype != torch.float64 or not ws.is_contiguous() or ws.device != grad.device:
        raise L.BubbleformerHipError(f"grad_norm_: ws must be a contiguous torch.float64 tensor on {grad.device}")
    L.check(L.lib().bf_grad_norm(_p(grad), grad.numel(), float(grad_scale), float(max_norm), _p(out), _p(ws), ws.numel(), _stream()), "bf_grad_norm")
    return out


def _coef_ptr(coef: Optional[torch.Tensor], p: torch.Tensor, who: str):
    if coef is None:
        return None
    if coef.dtype != torch.float32 or coef.numel() != 1 or coef.device != p.device:
        raise L.BubbleformerHipError(f"{who}: coef must be one torch.float32 element on {p.device} (e.g. grad_norm_'s out[1:])")
    return coef.data_ptr()


def _avg_args(avg: Optional[torch.Tensor], avg_weight: Optional[float], p: torch.Tensor, who: str):
    """None when the call keeps no average; otherwise (avg pointer, weight) for the step record."""
    if avg is None and avg_weight is None:
        return None
    if avg is None or avg_weight is None:
        raise L.BubbleformerHipError(f"{who}: avg and avg_weight go together (got avg={'None' if avg is None else 'a tensor'}, avg_weight={avg_weight!r})")
    if not isinstance(avg, torch.Tensor) or avg.dtype != torch.float32 or avg.device != p.device or avg.numel() != p.numel() or not avg.is_contiguous():
        raise L.BubbleformerHipError(f"{who}: avg must be a contiguous torch.float32 tensor of {p.numel()} elements on {p.device}")
    return _p(avg), float(avg_weight)


class ParamGroupTables:
    """The device side of a step's parameter groups, built once (``param_group_tables``): ``chunk`` (uint8, one group id per 64-element
    chunk of the flat buffer), ``lr_scale`` / ``weight_decay`` (fp32) and ``frozen`` (uint8), one row per group, ``n_groups`` of them, for
    a flat buffer of ``numel`` elements.  What adamw_ / adam_ / lion_ take as ``groups=``, and group_sumsq / group_clip_coef_."""

    def __init__(self, chunk, lr_scale, weight_decay, frozen, n_groups: int, numel: int):
        self.chunk, self.lr_scale, self.weight_decay, self.frozen, self.n_groups, self.numel = chunk, lr_scale, weight_decay, frozen, n_groups, numel


def param_group_tables(chunk_map: torch.Tensor, lr_scale, weight_decay, frozen, numel: int, device) -> ParamGroupTables:
    """Checks a chunk map (uint8, ceil(numel / 64) ids, e.g. utils.param_groups.ResolvedGroups.chunk_map) and the three per-group lists
    against each other on the host -- every id below the number of groups, 1 to 64 groups, scales and decays >= 0: the kernels cannot
    check ids without reading the map -- and puts them on ``device``."""
    if chunk_map is None or lr_scale is None or weight_decay is None or frozen is None:
        raise L.BubbleformerHipError("param_group_tables: the chunk map and the three group tables are required")
    G = len(lr_scale)
    if not 1 <= G <= L.BF_OPT_MAX_GROUPS or len(weight_decay) != G or len(frozen) != G:
        raise L.BubbleformerHipError(f"param_group_tables: {G} / {len(weight_decay)} / {len(frozen)} table rows; there must be 1 to "
                                     f"{L.BF_OPT_MAX_GROUPS} groups, the same number in every table")
    if not all(float(v) >= 0 for v in list(lr_scale) + list(weight_decay)):
        raise L.BubbleformerHipError("param_group_tables: lr_scale and weight_decay must be >= 0")
    cm = torch.as_tensor(chunk_map)
    chunks = (int(numel) + L.BF_OPT_CHUNK - 1) // L.BF_OPT_CHUNK
    if cm.dtype != torch.uint8 or cm.dim() != 1 or cm.numel() != chunks:
        raise L.BubbleformerHipError(f"param_group_tables: the chunk map must be {chunks} uint8 ids (one per {L.BF_OPT_CHUNK} of {int(numel)} elements), "
                                     f"got {tuple(cm.shape)} {cm.dtype}")
    if int(cm.max()) >= G:
        raise L.BubbleformerHipError(f"param_group_tables: the chunk map names group {int(cm.max())}, there are {G}")
    return ParamGroupTables(cm.to(device).contiguous(), torch.tensor([float(v) for v in lr_scale], dtype=torch.float32, device=device),
                            torch.tensor([float(v) for v in weight_decay], dtype=torch.float32, device=device),
                            torch.tensor([int(bool(v)) for v in frozen], dtype=torch.uint8, device=device), G, int(numel))


def _group_args(groups: ParamGroupTables, p: torch.Tensor, who: str):
    """(chunk map, lr_scale, weight_decay, frozen, n_groups) for the step record and the group norms; the map must be the one of p's length."""
    if not isinstance(groups, ParamGroupTables):
        raise L.BubbleformerHipError(f"{who}: groups must be an ops.ParamGroupTables (param_group_tables), got {type(groups).__name__}")
    chunks = (p.numel() + L.BF_OPT_CHUNK - 1) // L.BF_OPT_CHUNK
    if groups.chunk is None or groups.chunk.numel() != chunks or groups.chunk.device != p.device:
        raise L.BubbleformerHipError(f"{who}: the chunk map must hold {chunks} ids on {p.device} for a buffer of {p.numel()} elements"
                                     + ("" if groups.chunk is None else f", it holds {groups.chunk.numel()} on {groups.chunk.device}"))
    tabs = [None if t is None else _p(t) for t in (groups.lr_scale, groups.weight_decay, groups.frozen)]
    return _p(groups.chunk), tabs[0], tabs[1], tabs[2], int(groups.n_groups)


def group_sumsq_workspace(n: int, device) -> torch.Tensor:
    """The fp64 slab partials of group_sumsq for a buffer of n elements (64 per slab, at most 1024 slabs)."""
    return torch.empty(int(L.lib().bf_group_sumsq_ws_doubles(int(n))), dtype=torch.float64, device=device)


def group_sumsq(buf: torch.Tensor, groups: ParamGroupTables, out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[k] = the sum of buf[i]^2 over the elements whose chunk belongs to group k (fp64, n_groups elements on the device; allocated when
    None).  fp64 squares added in a fixed order, no float atomics (csrc/gradclip.hip): the same bits on every call.  ws:
    group_sumsq_workspace(buf.numel(), device), allocated per call when None."""
    _require_gpu(buf)
    if buf.dtype != torch.float32 or not buf.is_contiguous() or buf.dim() != 1:
        raise L.BubbleformerHipError("group_sumsq: buf must be a contiguous 1-D torch.float32 tensor")
    chunk, _, _, _, G = _group_args(groups, buf, "group_sumsq")
    if out is None:
        out = torch.empty(G, dtype=torch.float64, device=buf.device)
    elif out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != G or out.device != buf.device:
        raise L.BubbleformerHipError(f"group_sumsq: out must be a contiguous torch.float64 tensor of {G} elements on {buf.device}")
    if ws is None:
        ws = group_sumsq_workspace(buf.numel(), buf.device)
    elif ws.dtype != torch.float64 or not ws.is_contiguous() or ws.device != buf.device:
        raise L.BubbleformerHipError(f"group_sumsq: ws must be a contiguous torch.float64 tensor on {buf.device}")
    L.check(L.lib().bf_group_sumsq(_p(buf), buf.numel(), chunk, G, _p(out), _p(ws), ws.numel(), _stream()), "bf_group_sumsq")
    return out


def group_clip_coef_(sums: torch.Tensor, groups: ParamGroupTables, out: torch.Tensor, max_norm: float, grad_scale: float = 1.0,
                     group_norm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """grad_norm_'s {norm, coef} from group_sumsq's sums, over the groups that are not frozen -- torch.nn.utils.clip_grad_norm_ over the
    parameters a torch optimizer would hold: out[0] = grad_scale * sqrt(sum of the live groups' sums), out[1] = min(max_norm / (out[0] +
    1e-6), 1).  group_norm (fp32, n_groups elements on the device, optional) receives grad_scale * sqrt(sums[k]) of every group."""
    _require_gpu(sums)
    G = int(groups.n_groups)
    if sums.dtype != torch.float64 or not sums.is_contiguous() or sums.numel() != G:
        raise L.BubbleformerHipError(f"group_clip_coef_: sums must be a contiguous torch.float64 tensor of {G} elements (group_sumsq's)")
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != 2 or out.device != sums.device:
        raise L.BubbleformerHipError(f"group_clip_coef_: out must be a contiguous torch.float32 tensor of 2 elements on {sums.device}")
    if group_norm is not None and (group_norm.dtype != torch.float32 or not group_norm.is_contiguous() or group_norm.numel() != G
                                   or group_norm.device != sums.device):
        raise L.BubbleformerHipError(f"group_clip_coef_: group_norm must be a contiguous torch.float32 tensor of {G} elements on {sums.device}")
    L.check(L.lib().bf_group_clip_coef(_p(sums), None if groups.frozen is None else _p(groups.frozen), G, float(grad_scale), float(max_norm), _p(out),
                                       None if group_norm is None else _p(group_norm), _stream()), "bf_group_clip_coef")
    return out


def _live_ptr(live: Optional[torch.Tensor], p: torch.Tensor, who: str):
    if live is None:
        return None
    if not isinstance(live, torch.Tensor) or live.dtype != torch.int32 or live.numel() != 1 or live.device != p.device:
        raise L.BubbleformerHipError(f"{who}: live must be one torch.int32 element on {p.device} (e.g. step_guard_'s guard[:1])")
    return live.data_ptr()


def _opt_step(who: str, p, g, m, v, step, lr, betas, eps, weight_decay, grad_scale, coef, clip_value, avg, avg_weight, groups, live=None) -> "L.OptStep":
    """The bf_opt_step record of one adamw_ / adam_ / lion_ call, built by field name (lion_: v None, step 0, eps 0)."""
    av = _avg_args(avg, avg_weight, p, who)
    rec = L.OptStep(p=_p(p), g=_p(g), m=_p(m), v=None if v is None else _p(v), coef_dev=_coef_ptr(coef, p, who), n=p.numel(), step=int(step),
                    lr=float(lr), beta1=float(betas[0]), beta2=float(betas[1]), eps=float(eps), wd=float(weight_decay), gscale=float(grad_scale),
                    clip_value=float("inf") if clip_value is None else float(clip_value))
    if av is not None:
        rec.avg, rec.avg_weight = av
    if groups is not None:
        rec.chunk_group, rec.group_lr_scale, rec.group_weight_decay, rec.group_frozen, rec.n_groups = _group_args(groups, p, who)
    if live is not None:
        rec.live_dev = _live_ptr(live, p, who)
    return rec


def lion_(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, lr: float, betas=(0.9, 0.99), weight_decay: float = 0.0,
          grad_scale: float = 1.0, coef: Optional[torch.Tensor] = None, clip_value: Optional[float] = None,
          avg: Optional[torch.Tensor] = None, avg_weight: Optional[float] = None, groups: Optional[ParamGroupTables] = None,
          live: Optional[torch.Tensor] = None) -> None:
    """Fused Lion over flat fp32 buffers (lion_pytorch.Lion semantics, bubbleformer/modules.py:139-140).  coef: one fp32 on the device
    that multiplies grad_scale (grad_norm_'s out[1:]); clip_value: the scaled gradient is clamped to +-clip_value first
    (torch.nn.utils.clip_grad_value_).  Both None: the host-scale kernel.  avg / avg_weight (together or not at all): the same launch
    also moves the fp32 buffer ``avg`` (p's numel and device) towards the new p, avg += avg_weight * (p - avg) with 0 < avg_weight <= 1
    (1 copies p); p and m come out bit for bit as without them (weight_average_ is that update alone).  groups (param_group_tables):
    parameter groups -- an element whose chunk belongs to group k is stepped with lr * lr_scale[k] and weight_decay[k], a frozen group's
    chunks are neither read nor written (p, m, avg keep their bits); the ``weight_decay`` argument is then ignored, every group has its
    own.  live (one int32 on the device, step_guard_'s guard[:1]): the launch reads it first and, where it is 0, reads nothing else and
    writes nothing -- the step is skipped on the device, with no host round trip; where it is not 0 the results are bit for bit those
    without it.  One launch (bf_lion) for every combination of coef / clip_value / avg / groups / live.  None: exactly the kernels
    launched without it."""
    _require_gpu(p)
    rec = _opt_step("lion_", p, g, m, None, 0, lr, betas, 0.0, weight_decay, grad_scale, coef, clip_value, avg, avg_weight, groups, live)
    L.check(L.lib().bf_lion(C.byref(rec), _stream()), "bf_lion")
    _weights_changed()


def adamw_(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: int, lr: float, betas=(0.9, 0.999),
           eps: float = 1e-8, weight_decay: float = 1e-2, grad_scale: float = 1.0, coef: Optional[torch.Tensor] = None,
           clip_value: Optional[float] = None, avg: Optional[torch.Tensor] = None, avg_weight: Optional[float] = None,
           groups: Optional[ParamGroupTables] = None, live: Optional[torch.Tensor] = None) -> None:
    """Fused AdamW over flat fp32 buffers (torch.optim.AdamW semantics, bubbleformer/modules.py:135-136).  coef / clip_value / avg /
    avg_weight / groups / live: see lion_ (bf_adamw; m and v of a frozen chunk, and of a skipped step, keep their bits too)."""
    _require_gpu(p)
    rec = _opt_step("adamw_", p, g, m, v, step, lr, betas, eps, weight_decay, grad_scale, coef, clip_value, avg, avg_weight, groups, live)
    L.check(L.lib().bf_adamw(C.byref(rec), _stream()), "bf_adamw")
    _weights_changed()


def adam_(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: int, lr: float, betas=(0.9, 0.999),
          eps: float = 1e-8, weight_decay: float = 0.0, grad_scale: float = 1.0, coef: Optional[torch.Tensor] = None,
          clip_value: Optional[float] = None, avg: Optional[torch.Tensor] = None, avg_weight: Optional[float] = None,
          groups: Optional[ParamGroupTables] = None, live: Optional[torch.Tensor] = None) -> None:
    """Fused Adam over flat fp32 buffers (torch.optim.Adam semantics, bubbleformer/modules.py:137-138, config/optim_cfg/adam.yaml):
    weight decay is an L2 term added to the gradient before the moments, not AdamW's decoupled decay.  coef / clip_value: see lion_
    (the clamp comes before the L2 term, as clip_grad_value_ before optimizer.step()).  avg / avg_weight / groups: see lion_
    (bf_adam: a group's weight decay is its L2 term).  live: see lion_."""
    _require_gpu(p)
    rec = _opt_step("adam_", p, g, m, v, step, lr, betas, eps, weight_decay, grad_scale, coef, clip_value, avg, avg_weight, groups, live)
    L.check(L.lib().bf_adam(C.byref(rec), _stream()), "bf_adam")
    _weights_changed()


def step_guard_(norm: torch.Tensor, guard: torch.Tensor, step: int) -> torch.Tensor:
    """The device decision whether an optimizer step is taken (bf_step_guard, one tiny launch): ``guard`` (four int32 on the device:
    {live, consecutive, skipped, last_skipped_step}) is updated from ``norm`` (one fp32 on the device: grad_norm_'s or group_clip_coef_'s
    out[:1]) -- live = isfinite(norm); a non-finite norm adds one to consecutive and skipped and records ``step``, a finite one clears
    consecutive.  ``guard[:1]`` is the optimizers' ``live=``.  The norm's fp64 sum of squares is non-finite exactly when some element is."""
    _require_gpu(norm)
    if norm.dtype != torch.float32 or norm.numel() != 1:
        raise L.BubbleformerHipError("step_guard_: norm must be one torch.float32 element (e.g. grad_norm_'s out[:1])")
    if guard.dtype != torch.int32 or not guard.is_contiguous() or guard.numel() != 4 or guard.device != norm.device:
        raise L.BubbleformerHipError(f"step_guard_: guard must be a contiguous torch.int32 tensor of 4 elements on {norm.device}")
    L.check(L.lib().bf_step_guard(norm.data_ptr(), int(step), _p(guard), _stream()), "bf_step_guard")
    return guard


def nonfinite_scan_workspace(n: int, device) -> torch.Tensor:
    """The int64 slab partials of nonfinite_scan for a buffer of n elements (two per slab, at most 1024 slabs)."""
    return torch.empty(int(L.lib().bf_nonfinite_scan_ws_len(int(n))), dtype=torch.int64, device=device)


def nonfinite_scan(buf: torch.Tensor, out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = {index of the first inf / NaN in buf, or -1; how many buf holds} (two int64 on the device, allocated when None) over a flat
    fp32 buffer (bf_nonfinite_scan: grad_norm_'s slabs, integers only, no atomics).  The diagnostic after a skipped step, never part of
    one.  ws: nonfinite_scan_workspace(buf.numel(), device), allocated per call when None."""
    _require_gpu(buf)
    if buf.dtype != torch.float32 or not buf.is_contiguous() or buf.dim() != 1:
        raise L.BubbleformerHipError("nonfinite_scan: buf must be a contiguous 1-D torch.float32 tensor")
    if out is None:
        out = torch.empty(2, dtype=torch.int64, device=buf.device)
    elif out.dtype != torch.int64 or not out.is_contiguous() or out.numel() != 2 or out.device != buf.device:
        raise L.BubbleformerHipError(f"nonfinite_scan: out must be a contiguous torch.int64 tensor of 2 elements on {buf.device}")
    if ws is None:
        ws = nonfinite_scan_workspace(buf.numel(), buf.device)
    elif ws.dtype != torch.int64 or not ws.is_contiguous() or ws.device != buf.device:
        raise L.BubbleformerHipError(f"nonfinite_scan: ws must be a contiguous torch.int64 tensor on {buf.device}")
    L.check(L.lib().bf_nonfinite_scan(_p(buf), buf.numel(), _p(out), _p(ws), ws.numel(), _stream()), "bf_nonfinite_scan")
    return out


def _flat_pair(a: torch.Tensor, b: torch.Tensor, who: str) -> None:
    _require_gpu(a)
    for t in (a, b):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != a.device or t.numel() != a.numel():
            raise L.BubbleformerHipError(f"{who}: both buffers must be contiguous torch.float32 tensors of the same numel on one GPU")


def weight_average_(avg: torch.Tensor, p: torch.Tensor, w: float) -> torch.Tensor:
    """avg += w * (p - avg) over flat fp32 buffers, 0 < w <= 1 (1 copies p): the averaged-weights update of the optimizers' avg= on its
    own, with the same bits (csrc/optim_kernels.h: avg_lerp)."""
    _flat_pair(avg, p, "weight_average_")
    L.check(L.lib().bf_weight_average(_p(avg), _p(p), avg.numel(), float(w), _stream()), "bf_weight_average")
    return avg


def swap_buffers_(a: torch.Tensor, b: torch.Tensor, parameters: bool = False) -> None:
    """Exchanges the contents of two flat fp32 buffers exactly, in one launch (16-byte aligned, same numel, not overlapping).
    parameters=True: one of them backs model parameters, which this writes behind torch's version counters -- the prepared inference
    weights are marked stale (TrainStep.averaged_weights)."""
    _flat_pair(a, b, "swap_buffers_")
    L.check(L.lib().bf_swap_buffers(_p(a), _p(b), a.numel(), _stream()), "bf_swap_buffers")
    if parameters:
        _weights_changed()


# ------------------------------------------------------------------------------------------------ ModernUnet (conv.hip)
# Activations between U-Net layers are channels-last (B, H, W, C) tensors in the compute dtype; the clip and the prediction stay in the
# reference's (B, T, C, H, W) fp32 layout and are read / written in place by the first and last conv.  Weights are re-laid out per call
# as the GEMM operand [kh*kw][C_src][C_dst] in the compute dtype; parameter gradients are fp32 in the reference layout.
GN_GROUPS, GN_EPS = 8, 1e-5


def _csrc(t: Optional[torch.Tensor], C: int = 0, nchw: bool = False) -> Optional[L.ConvSrc]:
    if t is None:
        return None
    return L.ConvSrc(t.data_ptr(), int(C), int(nchw), int(t.dtype == torch.float32))


def _ref(s):
    return None if s is None else C.byref(s)


def _ws(n: int, device, what: str) -> torch.Tensor:
    if n < 0:
        L.check(-1, what)
    return torch.empty(max(int(n), 1), dtype=torch.float32, device=device)


def _conv(dt, geo, s0, s1, w, N, out, pro=L.BF_CONV_PRO_NONE, sc=None, sh=None, bias=None, resid=None, transposed=False):
    L.check(L.lib().bf_conv_fwd(_dt(dt), C.byref(geo), C.byref(s0), _ref(s1), pro, _p(sc), _p(sh), _p(w), N, _p(bias), _ref(resid),
                                C.byref(out), int(transposed), _stream()), "bf_conv_fwd")


def _wgrad(dt, geo, rows, s0, s1, K, dw, pro=L.BF_CONV_PRO_NONE, sc=None, sh=None):
    lib = L.lib()
    M = geo.F * geo.Ho * geo.Wo
    n = lib.bf_conv_wgrad_ws_floats(rows.C, K, M)
    ws = _ws(n, dw.device, "bf_conv_wgrad_ws_floats")
    L.check(lib.bf_conv_wgrad(_dt(dt), C.byref(geo), C.byref(rows), C.byref(s0), _ref(s1), pro, _p(sc), _p(sh), _p(dw), 0, _p(ws), ws.numel(),
                              _stream()), "bf_conv_wgrad")


def _colsum(dt, src, F, H, W, out):
    ws = _ws(64 * src.C, out.device, "bf_conv_colsum")
    L.check(L.lib().bf_conv_colsum(_dt(dt), C.byref(src), F, H, W, _p(out), 0, _p(ws), ws.numel(), _stream()), "bf_conv_colsum")


def _geo(F, Hi, Wi, Ho, Wo, k, stride, pad) -> L.ConvGeo:
    return L.ConvGeo(F, Hi, Wi, Ho, Wo, k, k, stride, pad)


def _wfwd(w, dt):
    """Conv2d weight [Cout][Cin][kh][kw] -> forward GEMM operand [kh*kw][Cin][Cout]."""
    return w.detach().permute(2, 3, 1, 0).to(dt).contiguous()


def _wswap(w, dt):
    """[A][B][kh][kw] -> [kh*kw][A][B]: a Conv2d weight as its data-gradient operand, a ConvTranspose2d weight as its forward one."""
    return w.detach().permute(2, 3, 0, 1).to(dt).contiguous()


def _gn_fwd(dt, x0, C0, x1, C1, B, H, W, gamma, beta):
    """-> (mean, rstd, sc, sh) of GroupNorm(8) over the channel concatenation of x0 and x1."""
    dev = x0.device
    Cin = C0 + C1
    mean = torch.empty(B, GN_GROUPS, dtype=torch.float32, device=dev)
    rstd = torch.empty_like(mean)
    sc = torch.empty(B, Cin, dtype=torch.float32, device=dev)
    sh = torch.empty_like(sc)
    lib = L.lib()
    ws = _ws(lib.bf_gn_ws_floats(B, Cin, GN_GROUPS), dev, "bf_gn_ws_floats")
    L.check(lib.bf_gn_fwd(_dt(dt), C.byref(_csrc(x0, C0)), _ref(_csrc(x1, C1)), B, H, W, GN_GROUPS, _p(_f32c(gamma)), _p(_f32c(beta)), GN_EPS,
                          _p(mean), _p(rstd), _p(sc), _p(sh), _p(ws), _stream()), "bf_gn_fwd")
    return mean, rstd, sc, sh


def _gn_bwd(dt, dA, x0, C0, x1, C1, B, H, W, gamma, stats, add, add_f32_ch, dgamma, dbeta):
    """dA: fp32 [B*H*W][C0+C1] gradient w.r.t. gelu(gn(cat(x0, x1))) -> (dx0, dx1) in the compute dtype, + add."""
    dx0 = torch.empty_like(x0)
    dx1 = torch.empty_like(x1) if x1 is not None else None
    lib = L.lib()
    ws = None
    if gamma is not None:
        ws = _ws(lib.bf_gn_ws_floats(B, C0 + C1, GN_GROUPS), dA.device, "bf_gn_ws_floats")
    mean, rstd, sc, sh = stats if stats is not None else (None,) * 4
    L.check(lib.bf_gn_bwd(_dt(dt), _p(dA), C.byref(_csrc(x0, C0)), _ref(_csrc(x1, C1)), B, H, W, GN_GROUPS, _p(gamma), _p(mean), _p(rstd), _p(sc),
                          _p(sh), _ref(_csrc(add, add_f32_ch)), C.byref(_csrc(dx0, C0)), _ref(_csrc(dx1, C1)), _p(dgamma), _p(dbeta), 0, _p(ws),
                          _stream()), "bf_gn_bwd")
    return dx0, dx1


def _pro(norm: bool):
    return L.BF_CONV_PRO_AFFINE_GELU if norm else L.BF_CONV_PRO_GELU


class _ResBlockFn(torch.autograd.Function):
    """ResidualBlock.forward (bubbleformer/layers/conv_layers.py:41-51) on cat(x, s):
    GN stats -> conv1 (GN affine + GELU prologue) -> GN stats -> conv2 (prologue) + bias + shortcut(x).
    Backward in reverse; the gradient of the skip input s is returned on its own (autograd adds it to the skip tensor's other uses)."""

    @staticmethod
    def forward(ctx, x, s, n1w, n1b, w1, b1, n2w, n2b, w2, b2, scw, scb):
        _require_gpu(x)
        dt = x.dtype
        B, H, W, C0 = x.shape
        C1 = 0 if s is None else s.shape[3]
        Cout = w1.shape[0]
        norm = n1w is not None
        g3 = _geo(B, H, W, H, W, 3, 1, 1)
        st1 = _gn_fwd(dt, x, C0, s, C1, B, H, W, n1w, n1b) if norm else None
        h = torch.empty(B, H, W, Cout, dtype=dt, device=x.device)
        _conv(dt, g3, _csrc(x, C0), _csrc(s, C1), _wfwd(w1, dt), Cout, _csrc(h, Cout), _pro(norm), *(st1[2:] if norm else (None, None)),
              bias=_f32c(b1))
        st2 = _gn_fwd(dt, h, Cout, None, 0, B, H, W, n2w, n2b) if norm else None
        if scw is not None:
            r = torch.empty(B, H, W, Cout, dtype=dt, device=x.device)
            _conv(dt, _geo(B, H, W, H, W, 1, 1, 0), _csrc(x, C0), _csrc(s, C1), _wfwd(scw, dt), Cout, _csrc(r, Cout), bias=_f32c(scb))
        else:
            if C1 or C0 != Cout:
                raise L.BubbleformerHipError("identity shortcut needs in_channels == out_channels")
            r = x
        out = torch.empty(B, H, W, Cout, dtype=dt, device=x.device)
        _conv(dt, g3, _csrc(h, Cout), None, _wfwd(w2, dt), Cout, _csrc(out, Cout), _pro(norm), *(st2[2:] if norm else (None, None)),
              bias=_f32c(b2), resid=_csrc(r, Cout))
        ctx.norm, ctx.has_s, ctx.has_sc = norm, s is not None, scw is not None
        st1 = st1 if norm else ()
        st2 = st2 if norm else ()
        ctx.save_for_backward(x, s if s is not None else x, h, w1, w2, scw if scw is not None else w1, n1w if norm else w1,
                              n2w if norm else w1, *st1, *st2)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, s, h, w1, w2, scw, n1w, n2w, *st = ctx.saved_tensors
        norm = ctx.norm
        s = s if ctx.has_s else None
        dt = x.dtype
        dout = dout.to(dt).contiguous()
        B, H, W, C0 = x.shape
        C1 = 0 if s is None else s.shape[3]
        Cin, Cout = C0 + C1, w1.shape[0]
        dev = x.device
        st1, st2 = (st[:4], st[4:]) if norm else (None, None)
        f32 = dict(dtype=torch.float32, device=dev)
        g3 = _geo(B, H, W, H, W, 3, 1, 1)
        g1 = _geo(B, H, W, H, W, 1, 1, 0)
        # conv2
        dw2 = torch.empty(Cout, 9 * Cout, **f32)
        db2 = torch.empty(Cout, **f32)
        _wgrad(dt, g3, _csrc(dout, Cout), _csrc(h, Cout), None, 9 * Cout, dw2, _pro(norm), *(st2[2:] if norm else (None, None)))
        _colsum(dt, _csrc(dout, Cout), B, H, W, db2)
        dA2 = torch.empty(B * H * W, Cout, **f32)
        _conv(dt, g3, _csrc(dout, Cout), None, _wswap(w2, dt), Cout, _csrc(dA2, Cout), transposed=True)
        dn2w = torch.empty(Cout, **f32) if norm else None
        dn2b = torch.empty(Cout, **f32) if norm else None
        dh, _ = _gn_bwd(dt, dA2, h, Cout, None, 0, B, H, W, n2w if norm else None, st2, None, 0, dn2w, dn2b)
        # shortcut
        dscw = dscb = None
        if ctx.has_sc:
            dscw = torch.empty(Cout, Cin, **f32)
            dscb = torch.empty(Cout, **f32)
            _wgrad(dt, g1, _csrc(dout, Cout), _csrc(x, C0), _csrc(s, C1), Cin, dscw)
            _colsum(dt, _csrc(dout, Cout), B, H, W, dscb)
            dxs = torch.empty(B * H * W, Cin, **f32)
            _conv(dt, g1, _csrc(dout, Cout), None, _wswap(scw, dt), Cin, _csrc(dxs, Cin), transposed=True)
            dscw = dscw.view(Cout, Cin, 1, 1)
        else:
            dxs = dout
        # conv1
        dw1 = torch.empty(Cout, 9 * Cin, **f32)
        db1 = torch.empty(Cout, **f32)
        _wgrad(dt, g3, _csrc(dh, Cout), _csrc(x, C0), _csrc(s, C1), 9 * Cin, dw1, _pro(norm), *(st1[2:] if norm else (None, None)))
        _colsum(dt, _csrc(dh, Cout), B, H, W, db1)
        dA1 = torch.empty(B * H * W, Cin, **f32)
        _conv(dt, g3, _csrc(dh, Cout), None, _wswap(w1, dt), Cin, _csrc(dA1, Cin), transposed=True)
        dn1w = torch.empty(Cin, **f32) if norm else None
        dn1b = torch.empty(Cin, **f32) if norm else None
        dx, ds = _gn_bwd(dt, dA1, x, C0, s, C1, B, H, W, n1w if norm else None, st1, dxs, Cin, dn1w, dn1b)
        dw1 = dw1.view(Cout, 3, 3, Cin).permute(0, 3, 1, 2).contiguous()
        dw2 = dw2.view(Cout, 3, 3, Cout).permute(0, 3, 1, 2).contiguous()
        return dx, ds, dn1w, dn1b, dw1, db1, dn2w, dn2b, dw2, db2, dscw, dscb


def res_block(x, s, n1w, n1b, w1, b1, n2w, n2b, w2, b2, scw, scb):
    """ResidualBlock on cat(x, s) (s may be None); x, s: (B, H, W, C) channels-last in the compute dtype."""
    return _ResBlockFn.apply(x, s, n1w, n1b, w1, b1, n2w, n2b, w2, b2, scw, scb)


class _DownFn(torch.autograd.Function):
    """Downsample: Conv2d(C, C, 3, stride 2, pad 1) (unets.py:37-62).  Data gradient: the 1- / 2-tap phases of the transposed gather."""

    @staticmethod
    def forward(ctx, x, w, b):
        _require_gpu(x)
        dt = x.dtype
        B, H, W, Cc = x.shape
        Ho, Wo = (H + 1) // 2, (W + 1) // 2
        out = torch.empty(B, Ho, Wo, Cc, dtype=dt, device=x.device)
        _conv(dt, _geo(B, H, W, Ho, Wo, 3, 2, 1), _csrc(x, Cc), None, _wfwd(w, dt), Cc, _csrc(out, Cc), bias=_f32c(b))
        ctx.save_for_backward(x, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w = ctx.saved_tensors
        dt = x.dtype
        dout = dout.to(dt).contiguous()
        B, H, W, Cc = x.shape
        Ho, Wo = dout.shape[1:3]
        f32 = dict(dtype=torch.float32, device=x.device)
        dw = torch.empty(Cc, 9 * Cc, **f32)
        db = torch.empty(Cc, **f32)
        _wgrad(dt, _geo(B, H, W, Ho, Wo, 3, 2, 1), _csrc(dout, Cc), _csrc(x, Cc), None, 9 * Cc, dw)
        _colsum(dt, _csrc(dout, Cc), B, Ho, Wo, db)
        dx = torch.empty_like(x)
        _conv(dt, _geo(B, Ho, Wo, H, W, 3, 2, 1), _csrc(dout, Cc), None, _wswap(w, dt), Cc, _csrc(dx, Cc), transposed=True)
        return dx, dw.view(Cc, 3, 3, Cc).permute(0, 3, 1, 2).contiguous(), db


class _UpFn(torch.autograd.Function):
    """Upsample: ConvTranspose2d(C, C, 4, stride 2, pad 1) (unets.py:10-34) as four 2x2-tap parity phases; its data gradient is the
    forward gather with stride 2, its weight gradient the forward-gather weight GEMM with the roles of input and output swapped."""

    @staticmethod
    def forward(ctx, x, w, b):
        _require_gpu(x)
        dt = x.dtype
        B, H, W, Cc = x.shape
        out = torch.empty(B, 2 * H, 2 * W, Cc, dtype=dt, device=x.device)
        _conv(dt, _geo(B, H, W, 2 * H, 2 * W, 4, 2, 1), _csrc(x, Cc), None, _wswap(w, dt), Cc, _csrc(out, Cc), bias=_f32c(b), transposed=True)
        ctx.save_for_backward(x, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w = ctx.saved_tensors
        dt = x.dtype
        dout = dout.to(dt).contiguous()
        B, H, W, Cc = x.shape
        f32 = dict(dtype=torch.float32, device=x.device)
        g = _geo(B, 2 * H, 2 * W, H, W, 4, 2, 1)
        dw = torch.empty(Cc, 16 * Cc, **f32)        # [Cin][(ky, kx, Cout)]
        db = torch.empty(Cc, **f32)
        _wgrad(dt, g, _csrc(x, Cc), _csrc(dout, Cc), None, 16 * Cc, dw)
        _colsum(dt, _csrc(dout, Cc), B, 2 * H, 2 * W, db)
        dx = torch.empty_like(x)
        _conv(dt, g, _csrc(dout, Cc), None, _wfwd(w, dt), Cc, _csrc(dx, Cc))
        return dx, dw.view(Cc, 4, 4, Cc).permute(0, 3, 1, 2).contiguous(), db


class _ProjFn(torch.autograd.Function):
    """image_proj: Conv2d(T*C, hidden, 1) reading the (B, T, C, H, W) fp32 clip in place (channel = t*C + c)."""

    @staticmethod
    def forward(ctx, x, w, b, dt):
        _require_gpu(x)
        x = x.contiguous().float()
        B, T, Cf, H, W = x.shape
        Cin, N = T * Cf, w.shape[0]
        out = torch.empty(B, H, W, N, dtype=dt, device=x.device)
        _conv(dt, _geo(B, H, W, H, W, 1, 1, 0), _csrc(x, Cin, nchw=True), None, _wfwd(w, dt), N, _csrc(out, N), bias=_f32c(b))
        ctx.save_for_backward(x, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w = ctx.saved_tensors
        B, T, Cf, H, W = x.shape
        Cin, N = T * Cf, w.shape[0]
        dt = dout.dtype
        dout = dout.contiguous()
        f32 = dict(dtype=torch.float32, device=x.device)
        g = _geo(B, H, W, H, W, 1, 1, 0)
        dw = torch.empty(N, Cin, **f32)
        db = torch.empty(N, **f32)
        _wgrad(dt, g, _csrc(dout, N), _csrc(x, Cin, nchw=True), None, Cin, dw)
        _colsum(dt, _csrc(dout, N), B, H, W, db)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _conv(dt, g, _csrc(dout, N), None, _wswap(w, dt), Cin, _csrc(dx, Cin, nchw=True), transposed=True)
        return dx, dw.view(N, Cin, 1, 1), db, None


class _FinalFn(torch.autograd.Function):
    """final(gelu(norm(x))) (unets.py:205) writing the (B, T, C_out, H, W) fp32 prediction in place; with ``target`` also the
    relative-L2 loss (LpLoss d=2, p=2, mean B, mean T, sum C; modules.py:50), reduced in a fixed order."""

    @staticmethod
    def forward(ctx, x, target, T, nw, nb, w, b):
        _require_gpu(x)
        dt = x.dtype
        B, H, W, Cc = x.shape
        N = w.shape[0]
        norm = nw is not None
        st = _gn_fwd(dt, x, Cc, None, 0, B, H, W, nw, nb) if norm else None
        pred = torch.empty(B, T, N // T, H, W, dtype=torch.float32, device=x.device)
        _conv(dt, _geo(B, H, W, H, W, 1, 1, 0), _csrc(x, Cc), None, _wfwd(w, dt), N, _csrc(pred, N, nchw=True), _pro(norm),
              *(st[2:] if norm else (None, None)), bias=_f32c(b))
        loss = torch.zeros((), dtype=torch.float32, device=x.device)
        coef = None
        if target is not None:
            target = target.contiguous().float()
            if target.shape != pred.shape:
                raise L.BubbleformerHipError(f"target shape {tuple(target.shape)} != prediction shape {tuple(pred.shape)}")
            coef = torch.empty(B * N, dtype=torch.float32, device=x.device)
            ws = torch.empty(4 * B * N, dtype=torch.float32, device=x.device)
            L.check(L.lib().bf_unet_lploss_fwd(_p(pred), _p(target), B, T, N // T, H * W, _p(loss), _p(coef), _p(ws), _stream()),
                    "bf_unet_lploss_fwd")
        ctx.norm, ctx.fused = norm, target is not None
        ctx.save_for_backward(x, w, nw if norm else w, pred, target if target is not None else pred, coef if coef is not None else pred,
                              *(st if norm else ()))
        ctx.set_materialize_grads(False)
        return pred, loss

    @staticmethod
    def backward(ctx, dpred, dloss):
        x, w, nw, pred, target, coef, *st = ctx.saved_tensors
        norm = ctx.norm
        if ctx.fused and dpred is not None:
            raise L.BubbleformerHipError("a gradient w.r.t. the prediction is not supported beside the fused loss")
        if (dloss if ctx.fused else dpred) is None:
            return (None,) * 7
        dt = x.dtype
        B, H, W, Cc = x.shape
        N = w.shape[0]
        f32 = dict(dtype=torch.float32, device=x.device)
        if ctx.fused:
            dpred = torch.empty_like(pred)
            L.check(L.lib().bf_unet_lploss_bwd(_p(pred), _p(target), _p(coef), _p(dloss.contiguous().float().reshape(1)), B * N, H * W, _p(dpred),
                                               _stream()), "bf_unet_lploss_bwd")
        else:
            dpred = dpred.contiguous().float()
        g = _geo(B, H, W, H, W, 1, 1, 0)
        dw = torch.empty(N, Cc, **f32)
        db = torch.empty(N, **f32)
        _wgrad(dt, g, _csrc(dpred, N, nchw=True), _csrc(x, Cc), None, Cc, dw, _pro(norm), *(st[2:] if norm else (None, None)))
        _colsum(dt, _csrc(dpred, N, nchw=True), B, H, W, db)
        dA = torch.empty(B * H * W, Cc, **f32)
        _conv(dt, g, _csrc(dpred, N, nchw=True), None, _wswap(w, dt), Cc, _csrc(dA, Cc), transposed=True)
        dnw = torch.empty(Cc, **f32) if norm else None
        dnb = torch.empty(Cc, **f32) if norm else None
        dx, _ = _gn_bwd(dt, dA, x, Cc, None, 0, B, H, W, nw if norm else None, st if norm else None, None, 0, dnw, dnb)
        return dx, None, None, dnw, dnb, dw.view(N, Cc, 1, 1), db


def unet_proj(x, w, b, compute_dtype):
    return _ProjFn.apply(x, w, b, compute_dtype)


def unet_down(x, w, b):
    return _DownFn.apply(x, w, b)


def unet_up(x, w, b):
    return _UpFn.apply(x, w, b)


def unet_final(x, T, nw, nb, w, b, target=None):
    """-> (pred (B, T, C, H, W) fp32, loss); only ``loss`` carries gradient when ``target`` is given."""
    return _FinalFn.apply(x, target, T, nw, nb, w, b)


# ------------------------------------------------------------------------------------------------ ClassicUnet (conv.hip + bn.hip)
# A ClassicUnetBlock is conv1 -> BN1 -> GELU -> conv2 -> BN2 -> GELU with bias-free 3x3 convs.  BN1 + GELU is conv2's operand prologue
# (never materialised); BN2 + GELU belongs to the block's consumer: bf_bn_act materialises it (and the 2x2 max pool of an encoder), the
# final 1x1 conv takes it as its prologue.  An activation `a` that feeds another layer's input travels with a gradient PORT: a zero-
# storage fp32 tensor of a's shape whose gradient is the fp32 data gradient the consumer computed for `a` (the skip half of a decoder's
# conv1, an upconv's data gradient).  bf_bn_bwd reads it as it stands, beside the pooled gradient, so the gradient of an encoder output is
# never rounded to the compute dtype and never summed by a PyTorch op.  `bn` below is a BatchNorm2d's (running_mean, running_var,
# num_batches_tracked, eps, momentum, training): training mode normalises with the batch statistics and updates the buffers on the device.


def _check_operands(dev, **named) -> None:
    """Every tensor a launch reads or writes must live on the launching input's GPU: a host (or other-device) address handed to a kernel
    faults.  Checked before the first launch of each classic function, since its convs have no bias to stop them earlier."""
    for name, t in named.items():
        if t is not None and t.device != dev:
            raise L.BubbleformerHipError(f"{name} is on {t.device} but the input is on {dev}: move the model to the input's device")


def _check_act(dt, **named) -> None:
    """Activations the kernels address as dense channels-last (or NCHW) memory: contiguous, in the compute dtype or fp32."""
    for name, t in named.items():
        if t is not None and (not t.is_contiguous() or t.dtype not in (dt, torch.float32)):
            raise L.BubbleformerHipError(f"{name} must be a contiguous {dt} or float32 tensor; got {t.dtype}, strides {t.stride()}")


def _check_bn(dev, C: int, gamma, beta, bn) -> None:
    """A BatchNorm2d's affine parameters and buffers, as bf_bn_fwd / bf_bn_eval read them: C fp32 values each on `dev`, an int64 counter."""
    rm, rv, nbt = bn[:3]
    _check_operands(dev, weight=gamma, bias=beta, running_mean=rm, running_var=rv, num_batches_tracked=nbt)
    for name, t in (("weight", gamma), ("bias", beta), ("running_mean", rm), ("running_var", rv)):
        if t.dtype != torch.float32 or t.numel() != C or not t.is_contiguous():
            raise L.BubbleformerHipError(f"BatchNorm2d {name} must be {C} contiguous fp32 values; got {tuple(t.shape)} {t.dtype}")
    if nbt.dtype != torch.int64 or nbt.numel() != 1:
        raise L.BubbleformerHipError(f"BatchNorm2d num_batches_tracked must be one int64; got {tuple(nbt.shape)} {nbt.dtype}")


def _port(like: torch.Tensor) -> torch.Tensor:
    return torch.empty_strided(like.shape, (0,) * like.dim(), dtype=torch.float32, device=like.device)


def _bn_stats(dt, c, gamma, beta, bn):
    """-> (mean, rstd, sc, sh) of BatchNorm2d over the channels-last conv output c (B, H, W, C); mean / rstd are None in eval mode."""
    rm, rv, nbt, eps, momentum, training = bn
    B, H, W, Cc = c.shape
    dev = c.device
    sc = torch.empty(B, Cc, dtype=torch.float32, device=dev)
    sh = torch.empty_like(sc)
    lib = L.lib()
    if not training:
        L.check(lib.bf_bn_eval(B, Cc, _p(_f32c(gamma)), _p(_f32c(beta)), float(eps), _p(rm), _p(rv), _p(sc), _p(sh), _stream()), "bf_bn_eval")
        return None, None, sc, sh
    mean = torch.empty(Cc, dtype=torch.float32, device=dev)
    rstd = torch.empty_like(mean)
    ws = _ws(lib.bf_bn_ws_floats(B * H * W, Cc), dev, "bf_bn_ws_floats")
    L.check(lib.bf_bn_fwd(_dt(dt), _p(c), B, H * W, Cc, _p(_f32c(gamma)), _p(_f32c(beta)), float(eps), float(momentum), _p(rm), _p(rv), _p(nbt),
                          _p(mean), _p(rstd), _p(sc), _p(sh), _p(ws), _stream()), "bf_bn_fwd")
    return mean, rstd, sc, sh


def _rows_view(g: torch.Tensor):
    """(tensor, row stride) of an fp32 (B, H, W, C) gradient whose pixels are rows of a wider buffer (a channel slice), or contiguous."""
    B, H, W, Cc = g.shape
    s = g.stride()
    if g.dtype == torch.float32 and s[3] == 1 and s[2] >= Cc and s[1] == W * s[2] and s[0] == H * s[1]:
        return g, s[2]
    return g.float().contiguous(), Cc


def _bn_bwd(dt, dA, dP, idx, c, gamma, st):
    """dA: fp32 (B, H, W, C) gradient w.r.t. gelu(bn(c)) or None; dP: gradient of its 2x2 max pool or None -> (dc, dgamma, dbeta)."""
    mean, rstd, sc, sh = st
    B, H, W, Cc = c.shape
    dev = c.device
    lib = L.lib()
    ldA = 0
    if dA is not None:
        dA, ldA = _rows_view(dA)
    if dP is not None:
        dP = dP.to(dt).contiguous()
    dc = torch.empty_like(c)
    dg = torch.empty(Cc, dtype=torch.float32, device=dev)
    db = torch.empty_like(dg)
    ws = _ws(lib.bf_bn_ws_floats(B * H * W, Cc), dev, "bf_bn_ws_floats")
    L.check(lib.bf_bn_bwd(_dt(dt), _p(dA), ldA, 0, _p(dP), _p(idx), _p(c), B, H, W, Cc, _p(_f32c(gamma)), _p(mean), _p(rstd), _p(sc), _p(sh),
                          _p(dc), _p(dg), _p(db), 0, _p(ws), _stream()), "bf_bn_bwd")
    return dc, dg, db


def _eval_bn_backward():
    return L.BubbleformerHipError("backward through an eval-mode BatchNorm2d is not implemented: train in model.train() mode")


class _ClassicConvFn(torch.autograd.Function):
    """conv1 (3x3, no bias) on cat(x0, x1) -> BN1 statistics -> conv2 (3x3, no bias) with BN1 + GELU as its prologue -> c2, the raw
    conv2 output (BN2 + GELU are applied by the consumer).  x0: the (B, T, C, H, W) fp32 clip (nchw) or a channels-last activation;
    x1: the skip activation of a decoder.  Its gradient leaves in fp32 through `port1` when one is given (the U-Net's encoder outputs, read
    in place by bf_bn_bwd), otherwise as x1's own gradient in x1's dtype."""

    @staticmethod
    def forward(ctx, x0, x1, port1, w1, g1, b1, w2, bn1, nchw, dt):
        _require_gpu(x0)
        if nchw:
            B, T, Cf, H, W = x0.shape
            C0 = T * Cf
        else:
            B, H, W, C0 = x0.shape
        C1 = 0 if x1 is None else x1.shape[3]
        Cout = w1.shape[0]
        if w1.shape[1] != C0 + C1:
            raise L.BubbleformerHipError(f"conv1 expects {w1.shape[1]} input channels, got {C0 + C1}")
        _check_operands(x0.device, skip=x1, conv1_weight=w1, conv2_weight=w2)
        _check_act(torch.float32 if nchw else dt, x=x0, skip=x1)
        _check_bn(x0.device, Cout, g1, b1, bn1)
        g3 = _geo(B, H, W, H, W, 3, 1, 1)
        c1 = torch.empty(B, H, W, Cout, dtype=dt, device=x0.device)
        _conv(dt, g3, _csrc(x0, C0, nchw), _csrc(x1, C1), _wfwd(w1, dt), Cout, _csrc(c1, Cout))
        st1 = _bn_stats(dt, c1, g1, b1, bn1)
        c2 = torch.empty_like(c1)
        _conv(dt, g3, _csrc(c1, Cout), None, _wfwd(w2, dt), Cout, _csrc(c2, Cout), L.BF_CONV_PRO_AFFINE_GELU, st1[2], st1[3])
        ctx.nchw, ctx.has_x1, ctx.has_port, ctx.training, ctx.C0, ctx.dt = nchw, x1 is not None, port1 is not None, bn1[5], C0, dt
        ctx.save_for_backward(x0, x1 if x1 is not None else c1, w1, g1, w2, c1, *(st1 if bn1[5] else st1[2:]))
        return c2

    @staticmethod
    def backward(ctx, dc2):
        if not ctx.training:
            raise _eval_bn_backward()
        x0, x1, w1, g1, w2, c1, *st1 = ctx.saved_tensors
        x1 = x1 if ctx.has_x1 else None
        dt, C0, nchw = ctx.dt, ctx.C0, ctx.nchw
        B, H, W, Cout = c1.shape
        C1 = 0 if x1 is None else x1.shape[3]
        Cin = C0 + C1
        f32 = dict(dtype=torch.float32, device=c1.device)
        g3 = _geo(B, H, W, H, W, 3, 1, 1)
        dc2 = dc2.to(dt).contiguous()
        # conv2 (prologue BN1 + GELU) and BN1
        dw2 = torch.empty(Cout, 9 * Cout, **f32)
        _wgrad(dt, g3, _csrc(dc2, Cout), _csrc(c1, Cout), None, 9 * Cout, dw2, L.BF_CONV_PRO_AFFINE_GELU, st1[2], st1[3])
        dA2 = torch.empty(B, H, W, Cout, **f32)
        _conv(dt, g3, _csrc(dc2, Cout), None, _wswap(w2, dt), Cout, _csrc(dA2, Cout), transposed=True)
        dc1, dg1, db1 = _bn_bwd(dt, dA2, None, None, c1, g1, st1)
        del dA2
        # conv1 over cat(x0, x1)
        dw1 = torch.empty(Cout, 9 * Cin, **f32)
        _wgrad(dt, g3, _csrc(dc1, Cout), _csrc(x0, C0, nchw), _csrc(x1, C1), 9 * Cin, dw1)
        dx0 = dx1 = dport = None
        if ctx.needs_input_grad[0]:
            dx0 = torch.empty_like(x0)
            _conv(dt, g3, _csrc(dc1, Cout), None, _wswap(w1[:, :C0], dt), C0, _csrc(dx0, C0, nchw), transposed=True)
        if x1 is not None and (ctx.needs_input_grad[2] if ctx.has_port else ctx.needs_input_grad[1]):
            d1 = torch.empty(B, H, W, C1, **f32) if ctx.has_port else torch.empty_like(x1)
            _conv(dt, g3, _csrc(dc1, Cout), None, _wswap(w1[:, C0:], dt), C1, _csrc(d1, C1), transposed=True)
            dx1, dport = (None, d1) if ctx.has_port else (d1, None)
        dw1 = dw1.view(Cout, 3, 3, Cin).permute(0, 3, 1, 2).contiguous()
        dw2 = dw2.view(Cout, 3, 3, Cout).permute(0, 3, 1, 2).contiguous()
        return dx0, dx1, dport, dw1, dg1, db1, dw2, None, None, None


class _BnActFn(torch.autograd.Function):
    """BN2 + GELU of a block, materialised: a = gelu(bn(c)) and, with pool, p = MaxPool2d(2, 2)(a) -> (a, port[, p]).
    Backward: bf_bn_bwd with the port's fp32 gradient (skip / upconv) and the pooled gradient together."""

    @staticmethod
    def forward(ctx, c, g, b, bn, pool):
        _require_gpu(c)
        dt = c.dtype
        B, H, W, Cc = c.shape
        _check_bn(c.device, Cc, g, b, bn)
        _check_act(dt, c=c)
        st = _bn_stats(dt, c, g, b, bn)
        a = torch.empty_like(c)
        p = idx = None
        if pool:
            p = torch.empty(B, H // 2, W // 2, Cc, dtype=dt, device=c.device)
            idx = torch.empty(B, H // 2, W // 2, Cc, dtype=torch.uint8, device=c.device)
        L.check(L.lib().bf_bn_act(_dt(dt), _p(c), B, H, W, Cc, _p(st[2]), _p(st[3]), _p(a), _p(p), _p(idx), _stream()), "bf_bn_act")
        port = _port(a)
        ctx.training, ctx.pool = bn[5], pool
        ctx.save_for_backward(c, g, *(st if bn[5] else st[2:]), *((idx,) if pool else ()))
        ctx.set_materialize_grads(False)
        return (a, port, p) if pool else (a, port)

    @staticmethod
    def backward(ctx, da, dport, dp=None):
        if not ctx.training:
            raise _eval_bn_backward()
        c, g, *st = ctx.saved_tensors
        idx = st.pop() if ctx.pool else None
        dA = dport
        if da is not None:           # `a` used directly (ClassicUnetBlock.forward outside the U-Net): its gradient is in the compute dtype
            dA = da.float() if dA is None else dA + da.float()
        if dA is None and dp is None:
            return None, None, None, None, None
        dc, dg, db = _bn_bwd(c.dtype, dA, dp, idx, c, g, st)
        return dc, dg, db, None, None


class _UpConv2Fn(torch.autograd.Function):
    """ConvTranspose2d(Cin, Cout, 2, stride 2) (unets.py:252-284): the transposed gather with four parity phases of one tap each.  Its data
    gradient is the forward gather with stride 2, its weight gradient the forward-gather weight GEMM with input and output swapped.  With a
    port, x's gradient leaves in fp32 through the port; without, in x's dtype."""

    @staticmethod
    def forward(ctx, x, port, w, b):
        _require_gpu(x)
        dt = x.dtype
        B, H, W, Cin = x.shape
        Cout = w.shape[1]
        if w.shape[0] != Cin or tuple(w.shape[2:]) != (2, 2):
            raise L.BubbleformerHipError(f"upconv weight {tuple(w.shape)} does not fit {Cin} input channels, kernel 2")
        _check_operands(x.device, upconv_weight=w, upconv_bias=b)
        _check_act(dt, x=x)
        out = torch.empty(B, 2 * H, 2 * W, Cout, dtype=dt, device=x.device)
        _conv(dt, _geo(B, H, W, 2 * H, 2 * W, 2, 2, 0), _csrc(x, Cin), None, _wswap(w, dt), Cout, _csrc(out, Cout), bias=_f32c(b),
              transposed=True)
        ctx.has_port = port is not None
        ctx.save_for_backward(x, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w = ctx.saved_tensors
        dt = x.dtype
        dout = dout.to(dt).contiguous()
        B, H, W, Cin = x.shape
        Cout = w.shape[1]
        f32 = dict(dtype=torch.float32, device=x.device)
        g = _geo(B, 2 * H, 2 * W, H, W, 2, 2, 0)
        dw = torch.empty(Cin, 4 * Cout, **f32)        # [Cin][(ky, kx, Cout)]
        db = torch.empty(Cout, **f32)
        _wgrad(dt, g, _csrc(x, Cin), _csrc(dout, Cout), None, 4 * Cout, dw)
        _colsum(dt, _csrc(dout, Cout), B, 2 * H, 2 * W, db)
        dx = dport = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            d = torch.empty(B, H, W, Cin, **f32) if ctx.has_port else torch.empty_like(x)
            _conv(dt, g, _csrc(dout, Cout), None, _wfwd(w, dt), Cin, _csrc(d, Cin))
            dx, dport = (None, d) if ctx.has_port else (d, None)
        return dx, dport, dw.view(Cin, 2, 2, Cout).permute(0, 3, 1, 2).contiguous(), db


class _ClassicFinalFn(torch.autograd.Function):
    """conv(gelu(bn2(c))) of the last decoder (unets.py:290-319): BN2 statistics, then the 1x1 conv with BN2 + GELU as its prologue writing
    the (B, T, C_out, H, W) fp32 prediction in place; with ``target`` also the fused relative-L2 loss, as _FinalFn."""

    @staticmethod
    def forward(ctx, c, target, T, g, b, bn, w, bias):
        _require_gpu(c)
        dt = c.dtype
        B, H, W, Cc = c.shape
        N = w.shape[0]
        _check_operands(c.device, conv_weight=w, conv_bias=bias, target=target)
        _check_bn(c.device, Cc, g, b, bn)
        _check_act(dt, c=c)
        st = _bn_stats(dt, c, g, b, bn)
        pred = torch.empty(B, T, N // T, H, W, dtype=torch.float32, device=c.device)
        _conv(dt, _geo(B, H, W, H, W, 1, 1, 0), _csrc(c, Cc), None, _wfwd(w, dt), N, _csrc(pred, N, nchw=True), L.BF_CONV_PRO_AFFINE_GELU,
              st[2], st[3], bias=_f32c(bias))
        loss = torch.zeros((), dtype=torch.float32, device=c.device)
        coef = None
        if target is not None:
            target = target.contiguous().float()
            if target.shape != pred.shape:
                raise L.BubbleformerHipError(f"target shape {tuple(target.shape)} != prediction shape {tuple(pred.shape)}")
            coef = torch.empty(B * N, dtype=torch.float32, device=c.device)
            ws = torch.empty(4 * B * N, dtype=torch.float32, device=c.device)
            L.check(L.lib().bf_unet_lploss_fwd(_p(pred), _p(target), B, T, N // T, H * W, _p(loss), _p(coef), _p(ws), _stream()),
                    "bf_unet_lploss_fwd")
        ctx.fused, ctx.training = target is not None, bn[5]
        ctx.save_for_backward(c, g, w, pred, target if target is not None else pred, coef if coef is not None else pred,
                              *(st if bn[5] else st[2:]))
        ctx.set_materialize_grads(False)
        return pred, loss

    @staticmethod
    def backward(ctx, dpred, dloss):
        c, g, w, pred, target, coef, *st = ctx.saved_tensors
        if ctx.fused and dpred is not None:
            raise L.BubbleformerHipError("a gradient w.r.t. the prediction is not supported beside the fused loss")
        if (dloss if ctx.fused else dpred) is None:
            return (None,) * 8
        if not ctx.training:
            raise _eval_bn_backward()
        dt = c.dtype
        B, H, W, Cc = c.shape
        N = w.shape[0]
        f32 = dict(dtype=torch.float32, device=c.device)
        if ctx.fused:
            dpred = torch.empty_like(pred)
            L.check(L.lib().bf_unet_lploss_bwd(_p(pred), _p(target), _p(coef), _p(dloss.contiguous().float().reshape(1)), B * N, H * W, _p(dpred),
                                               _stream()), "bf_unet_lploss_bwd")
        else:
            dpred = dpred.contiguous().float()
        geo = _geo(B, H, W, H, W, 1, 1, 0)
        dw = torch.empty(N, Cc, **f32)
        db = torch.empty(N, **f32)
        _wgrad(dt, geo, _csrc(dpred, N, nchw=True), _csrc(c, Cc), None, Cc, dw, L.BF_CONV_PRO_AFFINE_GELU, st[2], st[3])
        _colsum(dt, _csrc(dpred, N, nchw=True), B, H, W, db)
        dA = torch.empty(B, H, W, Cc, **f32)
        _conv(dt, geo, _csrc(dpred, N, nchw=True), None, _wswap(w, dt), Cc, _csrc(dA, Cc), transposed=True)
        dc, dg, dbn = _bn_bwd(dt, dA, None, None, c, g, st)
        return dc, None, None, dg, dbn, None, dw.view(N, Cc, 1, 1), db


def classic_conv(x0, x1, port1, w1, g1, b1, w2, bn1, compute_dtype, nchw=False):
    """conv1 -> BN1 + GELU -> conv2 of a ClassicUnetBlock -> the raw conv2 output (B, H, W, C) in the compute dtype."""
    return _ClassicConvFn.apply(x0, x1, port1, w1, g1, b1, w2, bn1, bool(nchw), compute_dtype)


def classic_act(c, g, b, bn, pool=False):
    """gelu(bn(c)) -> (a, port) or, with pool, (a, port, maxpool2x2(a))."""
    return _BnActFn.apply(c, g, b, bn, bool(pool))


def unet_upconv2(x, w, b, port=None):
    """ConvTranspose2d(Cin, Cout, kernel 2, stride 2) on a channels-last x -> (B, 2H, 2W, Cout)."""
    return _UpConv2Fn.apply(x, port, w, b)


def classic_final(c, T, g, b, bn, w, bias, target=None):
    """-> (pred (B, T, C, H, W) fp32, loss) of conv(gelu(bn(c))); only ``loss`` carries gradient when ``target`` is given."""
    return _ClassicFinalFn.apply(c, target, T, g, b, bn, w, bias)


# ---------------------------------------------------------------------------- pictures (csrc/render.hip; utils/plot_utils.py is the user's side)
_RENDER_LUTS = {}


def _render_luts(device):
    """The two 256 x 3 colour tables on ``device`` (utils/colormaps.py), uploaded once."""
    key = (device.type, device.index)
    if key not in _RENDER_LUTS:
        from .utils import colormaps
        _RENDER_LUTS[key] = tuple(torch.from_numpy(t.copy()).to(device) for t in (colormaps.BLUES, colormaps.TURBO))
    return _RENDER_LUTS[key]


def render_ranges(frames: torch.Tensor, channels: Sequence[int]) -> torch.Tensor:
    """frames (F, C, H, W) fp32 on the device, channels = (sdf, temperature, velx, vely) with -1 for an absent one -> (3, 5) fp64 on the
    device: {n, sum, sum of squares, min, max} of the signed distance, the temperature and the speed (bf_render_ranges).  Never synchronises."""
    _require_gpu(frames)
    if frames.dim() != 4 or frames.dtype != torch.float32 or not frames.is_contiguous():
        raise L.BubbleformerHipError("render_ranges: the frames must be a contiguous fp32 (F, C, H, W) tensor")
    ch = [int(c) for c in channels]
    if len(ch) != 4 or any(c < -1 or c >= frames.shape[1] for c in ch):
        raise L.BubbleformerHipError(f"render_ranges: channels must be four indices into the {frames.shape[1]} channels, -1 for an absent field")
    Fn, Cn, H, W = frames.shape
    out = torch.empty((3, 5), dtype=torch.float64, device=frames.device)
    ws = torch.empty(L.lib().bf_render_ranges_ws_doubles(), dtype=torch.float64, device=frames.device)
    L.check(L.lib().bf_render_ranges(_p(frames), Fn, Cn, H, W, *ch, _p(out), _p(ws), _stream()), "bf_render_ranges")
    return out


def render_tiles(tiles: Sequence[dict], layout, images: int) -> torch.Tensor:
    """One launch for all images of a call (bf_render_tiles) -> (images, img_h, img_w, 3) uint8 on the device.

    tiles: one dict per description, slot k of an image showing description k % len(tiles): ``kind`` (L.BF_RENDER_*), ``a`` (and ``b`` for a
    speed tile, ``mask`` optionally) fp32 views of shape (images, rounds, H, W) whose last two axes are contiguous, ``range`` two fp64 values
    {vmin, vmax} on the device.  layout: a ``plot_utils.RenderLayout``."""
    g = layout
    rounds, rem = divmod(g.rows * g.cols, len(tiles))
    if not 1 <= len(tiles) <= L.BF_RENDER_MAX_TILES or rem:
        raise L.BubbleformerHipError(f"render_tiles: {len(tiles)} descriptions do not tile {g.rows} x {g.cols} slots")
    device = tiles[0]["a"].device
    desc = (L.RenderTile * len(tiles))()
    for d, t in zip(desc, tiles):
        views = [t["a"], t.get("b"), t.get("mask")]
        for v in views:
            if v is None:
                continue
            _require_gpu(v)
            if (v.dtype != torch.float32 or v.device != device or tuple(v.shape) != (images, rounds, g.H, g.W)
                    or (g.W > 1 and v.stride(3) != 1) or (g.H > 1 and v.stride(2) != g.W)):
                raise L.BubbleformerHipError(f"render_tiles: a field must be an fp32 view of shape {(images, rounds, g.H, g.W)} with contiguous frames on {device}")
        rng = t["range"]
        if rng.dtype != torch.float64 or rng.numel() != 2 or not rng.is_contiguous() or rng.device != device:
            raise L.BubbleformerHipError("render_tiles: a range is two contiguous fp64 values on the fields' device")
        if t["kind"] == L.BF_RENDER_SPEED and views[1] is None:
            raise L.BubbleformerHipError("render_tiles: a speed tile needs both velocity components")
        d.a, d.b, d.mask = _p(views[0]), _p(views[1]), _p(views[2])
        d.frame_stride, d.slot_stride = views[0].stride(0), views[0].stride(1)
        if views[1] is not None and (views[1].stride(0), views[1].stride(1)) != (views[0].stride(0), views[0].stride(1)):
            raise L.BubbleformerHipError("render_tiles: both velocity components must have the same strides")
        if views[2] is not None:
            d.mask_frame_stride, d.mask_slot_stride = views[2].stride(0), views[2].stride(1)
        d.range, d.kind = _p(rng), int(t["kind"])
    geom = L.RenderGeom(g.H, g.W, g.scale, g.rows, g.cols, g.ox, g.oy, g.pitch_x, g.pitch_y, g.bar_dx, g.bar_w, g.img_h, g.img_w, g.stride, float(g.stroke))
    blues, turbo = _render_luts(device)
    out = torch.empty((images, g.img_h, g.img_w, 3), dtype=torch.uint8, device=device)
    L.check(L.lib().bf_render_tiles(desc, len(tiles), C.byref(geom), images, _p(blues), _p(turbo), _p(out), _stream()), "bf_render_tiles")
    return out
