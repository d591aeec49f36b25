"""The reference's criterion and physics penalty as native, differentiable ops (reference: bubbleformer/utils/losses.py).

``LpLoss`` has the reference's constructor, attributes and reduction behaviour; its relative Lp norm per row and the gradient of it run
in csrc/losses.hip (bf_lp_rows_fwd / bf_lp_rows_bwd), the reductions over the leading dims are ordinary torch ops on the small tensor of
per-row ratios.  ``eikonal_loss`` is `physics.eikonal_loss` with a backward (bf_eikonal_bwd).  ``InterfaceLpLoss`` (no reference
program) is the training configuration of LpLoss with a pixel weight around the target's liquid-vapour interface, a weight per field and an
optional Eikonal penalty, forward and backward in their own kernels (bf_wlp_fwd / bf_wlp_bwd).  Inputs are fp32 tensors on the GPU; there
is no CPU path.  ``SpectralLpLoss`` (no reference program) is the same relative L2 taken in Fourier space with a weight per radial shell and
field, on fp32 transforms of its own (csrc/spectral_loss.hip: bf_slp_fwd / bf_slp_bwd).
"""
import math
from typing import List, Union

import torch
import torch.nn as nn

from .. import _lib as L

EIKONAL_DX = 1.0 / 32      # the reference's grid spacing (utils/losses.py:9)


def _require_gpu_f32(t: torch.Tensor, what: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
        raise L.BubbleformerHipError(f"{what} runs only on a ROCm GPU (gfx950): got {where}; there is no CPU fallback")
    if t.dtype != torch.float32:
        raise L.BubbleformerHipError(f"{what} takes fp32 tensors; got {t.dtype}")


def _check_p(p) -> float:
    try:
        v = float(p)
    except (TypeError, ValueError):
        raise NotImplementedError(f"LpLoss: p must be a finite number >= 1; got {p!r}") from None
    if not (math.isfinite(v) and v >= 1.0):
        raise NotImplementedError(f"LpLoss: only finite p >= 1 is implemented natively; got p = {p!r}")
    return v


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _like_offset(t: torch.Tensor) -> torch.Tensor:
    """An uninitialised contiguous fp32 tensor of t's shape at t's offset from a 16-byte boundary, so that the kernels can move t and the
    new tensor with 16-byte accesses together (a contiguous view into a larger tensor need not start on a boundary)."""
    off = (t.data_ptr() % 16) // 4
    if off == 0:
        return torch.empty_like(t)
    return torch.empty(t.numel() + off, dtype=torch.float32, device=t.device)[off:].view(t.shape)


_WS_DOUBLES = {}      # (rows, n) -> bf_lp_rows_ws_doubles


class _LpRowsFn(torch.autograd.Function):
    """(pred, y) -> (sum |pred - y|^p / sum |y|^p)^(1/p) over the last d dims, in the shape of the leading dims."""

    @staticmethod
    def forward(ctx, pred, y, d, p):
        lead, n = pred.shape[:pred.dim() - d], math.prod(pred.shape[pred.dim() - d:])
        rows = math.prod(lead)
        pred, y = pred.contiguous(), y.contiguous()
        lib = L.lib()
        ratio = torch.empty(lead, dtype=torch.float32, device=pred.device)
        nws = _WS_DOUBLES.get((rows, n))
        if nws is None:
            nws = _WS_DOUBLES[(rows, n)] = lib.bf_lp_rows_ws_doubles(rows, n)
        if nws < 0:
            raise L.BubbleformerHipError(f"LpLoss: {rows} rows of {n} elements are out of range")
        buf = torch.empty(2 * rows + nws, dtype=torch.float64, device=pred.device)      # the saved sums, then the call's workspace
        sums = buf[:2 * rows]
        L.check(lib.bf_lp_rows_fwd(pred.data_ptr(), y.data_ptr(), rows, n, p, ratio.data_ptr(), sums.data_ptr(),
                                   sums.data_ptr() + 16 * rows if nws else None, nws, _stream()), "bf_lp_rows_fwd")
        ctx.save_for_backward(pred, y, sums)
        ctx.p = p
        return ratio

    @staticmethod
    def backward(ctx, g):
        pred, y, sums = ctx.saved_tensors
        rows = sums.shape[0] // 2
        g = g.contiguous().float()
        dpred = _like_offset(pred)
        L.check(L.lib().bf_lp_rows_bwd(pred.data_ptr(), y.data_ptr(), g.data_ptr(), sums.data_ptr(), rows, pred.numel() // rows, ctx.p,
                                       dpred.data_ptr(), _stream()), "bf_lp_rows_bwd")
        return dpred, None, None, None


def lp_rows(pred: torch.Tensor, y: torch.Tensor, d: int = 1, p: float = 2) -> torch.Tensor:
    """Relative Lp norm of pred - y over the last d dims (what LpLoss reduces): fp32 GPU tensors of one shape -> the leading dims."""
    p = _check_p(p)
    _require_gpu_f32(pred, "LpLoss")
    _require_gpu_f32(y, "LpLoss")
    if y.requires_grad and torch.is_grad_enabled():
        raise L.BubbleformerHipError("LpLoss: a gradient w.r.t. the target is not implemented (the target must not require grad)")
    if pred.shape != y.shape:
        raise L.BubbleformerHipError(f"LpLoss: prediction {tuple(pred.shape)} and target {tuple(y.shape)} differ in shape")
    if not (isinstance(d, int) and 1 <= d <= pred.dim()):
        raise L.BubbleformerHipError(f"LpLoss: d = {d!r} must be an int between 1 and the {pred.dim()} dims of the input")
    if pred.numel() == 0:
        raise L.BubbleformerHipError("LpLoss: empty input")
    return _LpRowsFn.apply(pred, y, d, p)


class LpLoss(nn.Module):
    """Relative Lp loss on tensors (b, n1, ..., nd) with the reference's interface (utils/losses.py:17-94).

    d: how many trailing dims form one norm; p: the power, any finite value >= 1 (p = inf is not implemented); reduce_dims: the leading
    dims to reduce, an int, a list or None (no reduction); reductions: "sum" / "mean", one for all or one per reduced dim.  Each listed dim
    is reduced with keepdim and the result is squeezed, which also removes a batch dim of size 1, as the reference does."""

    def __init__(self, d: int = 1, p: int = 2, reduce_dims: Union[int, List[int]] = 0, reductions: Union[str, List[str]] = "sum"):
        super().__init__()
        _check_p(p)
        self.d = d
        self.p = p
        self.reduce_dims = [reduce_dims] if isinstance(reduce_dims, int) else reduce_dims
        if self.reduce_dims is not None:      # as in the reference, `reductions` exists only beside reduce_dims
            names = [reductions] * len(self.reduce_dims) if isinstance(reductions, str) else reductions
            for name in names:
                assert name == "sum" or name == "mean"
            self.reductions = names

    def reduce_all(self, x: torch.Tensor) -> torch.Tensor:
        for dim, how in zip(self.reduce_dims, self.reductions):
            x = x.sum(dim=dim, keepdim=True) if how == "sum" else x.mean(dim=dim, keepdim=True)
        return x

    def forward(self, y_pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        ratio = lp_rows(y_pred, y, self.d, self.p)
        if self.reduce_dims is not None:
            ratio = self.reduce_all(ratio).squeeze()
        return ratio


class _EikonalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, phi):
        phi = phi.contiguous()
        H, W = phi.shape[-2:]
        acc = torch.zeros(1, dtype=torch.float64, device=phi.device)
        L.check(L.lib().bf_eikonal_sum(phi.data_ptr(), phi.numel() // (H * W), H, W, EIKONAL_DX, acc.data_ptr(), _stream()), "bf_eikonal_sum")
        ctx.save_for_backward(phi)
        return (acc / phi.numel()).float().squeeze(0)

    @staticmethod
    def backward(ctx, g):
        phi, = ctx.saved_tensors
        H, W = phi.shape[-2:]
        g = g.contiguous().float().reshape(1)
        dphi = torch.empty_like(phi)
        L.check(L.lib().bf_eikonal_bwd(phi.data_ptr(), phi.numel() // (H * W), H, W, EIKONAL_DX, g.data_ptr(), dphi.data_ptr(), _stream()),
                "bf_eikonal_bwd")
        return dphi


def eikonal_loss(phi: torch.Tensor) -> torch.Tensor:
    """phi = SDF tensor (..., H, W) -> mean over all elements of (|grad phi| - 1)^2, gradients as torch.gradient(spacing=1/32, edge_order=1)
    (utils/losses.py:5-15); differentiable.  The value is `physics.eikonal_loss`'s, bit for bit.

    One deliberate difference from autograd of the reference's expression: where |grad phi| is exactly 0 (a flat patch) the reference's
    backward multiplies 0 by inf and turns the whole gradient of the neighbourhood into NaN; here such a cell contributes 0, the limit of
    its contribution along every direction being bounded and the set having measure zero for a real field."""
    _require_gpu_f32(phi, "eikonal_loss")
    if phi.dim() < 2 or phi.numel() == 0:
        raise L.BubbleformerHipError(f"eikonal_loss expects (..., H, W); got {tuple(phi.shape)}")
    return _EikonalFn.apply(phi)


_WLP_WS_DOUBLES = {}      # (frames, C, H, W) -> bf_wlp_ws_doubles


class _InterfaceLpFn(torch.autograd.Function):
    """(pred, y) -> the scalar of InterfaceLpLoss; the criterion keeps the terms the forward left on the device."""

    @staticmethod
    def forward(ctx, pred, y, crit):
        B, T, Cn, H, W = pred.shape
        frames = B * T
        pred, y = pred.contiguous(), y.contiguous()
        lib = L.lib()
        nws = _WLP_WS_DOUBLES.get((frames, Cn, H, W))
        if nws is None:
            nws = _WLP_WS_DOUBLES[(frames, Cn, H, W)] = lib.bf_wlp_ws_doubles(frames, Cn, H, W)
        if nws < 0:
            raise L.BubbleformerHipError(f"InterfaceLpLoss: {frames} frames of {Cn} x {H} x {W} are out of range")
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        terms = torch.empty(1 + Cn, dtype=torch.float32, device=pred.device)
        buf = torch.empty(2 * frames * Cn + nws, dtype=torch.float64, device=pred.device)      # the saved sums, then the call's workspace
        sums = buf[:2 * frames * Cn]
        ctx.args = (frames, Cn, H, W) + crit._abi_args(Cn)
        L.check(lib.bf_wlp_fwd(pred.data_ptr(), y.data_ptr(), *ctx.args, loss.data_ptr(), terms.data_ptr(), sums.data_ptr(),
                               sums.data_ptr() + 16 * frames * Cn, nws, _stream()), "bf_wlp_fwd")
        ctx.save_for_backward(pred, y, sums)
        crit._terms = terms
        return loss

    @staticmethod
    def backward(ctx, g):
        pred, y, sums = ctx.saved_tensors
        g = g.contiguous().float().reshape(1)
        dpred = _like_offset(pred)
        L.check(L.lib().bf_wlp_bwd(pred.data_ptr(), y.data_ptr(), g.data_ptr(), sums.data_ptr(), *ctx.args, dpred.data_ptr(), _stream()), "bf_wlp_bwd")
        return dpred, None, None


class InterfaceLpLoss(nn.Module):
    """The relative L2 of LpLoss's training configuration with every pixel weighted by its distance to the liquid-vapour interface of the
    TARGET frame, a weight per field, and an optional Eikonal penalty on the predicted signed distance -- one native criterion for
    ``TrainStep(criterion=...)`` / ``fit(criterion=...)`` (csrc/losses.hip: bf_wlp_fwd / bf_wlp_bwd; no reference program).

    pred, y: (B, T, C, H, W) fp32 on the GPU in the dataset's normalised units, stored = (x - diff) / div; y never requires a gradient.  With
    phi_t = y[:, :, sdf_channel] * div + diff (the simulated signed distance, in the reference's units, grid spacing dx):
        w        = 1 + gain * max(0, 1 - |phi_t| / band)              a hat of half-width `band` (phi's units) and height `gain` >= 0
        rho      = sqrt(sum_hw w (pred - y)^2 / sum_hw w y^2)         per (b, t, c); one weight map for the C fields of a frame
        L_data   = sum_c field_weights[c] * mean_{b,t} rho[b, t, c]
        L_eik    = eikonal * mean_{b,t,h,w} (|grad (pred[:, :, sdf_channel] * div + diff)| - 1)^2      (torch.gradient, spacing dx)
    and forward returns L_data + L_eik, a scalar fp32 tensor differentiable w.r.t. pred.  gain = 0, unit field weights and eikonal = 0 give
    ``LpLoss(d=2, p=2, reduce_dims=[0, 1, 2], reductions=["mean", "mean", "sum"])``.  A flat cell of the predicted distance contributes 0 to the
    penalty's gradient (see ``eikonal_loss``).

    ``band`` and ``gain`` have no defaults: no value has been validated by a training run.  ``field_terms()`` / ``eikonal_term()`` return the C
    values ``field_weights[c] * mean rho`` and the penalty of the last forward as device tensors (clones; no host synchronisation)."""

    def __init__(self, sdf_channel: int, band: float, gain: float, *, diff: float = 0.0, div: float = 1.0, field_weights=None,
                 eikonal: float = 0.0, dx: float = EIKONAL_DX):
        super().__init__()
        if not (isinstance(sdf_channel, int) and sdf_channel >= 0):
            raise ValueError(f"InterfaceLpLoss: sdf_channel = {sdf_channel!r} must be an int >= 0")
        band, gain, diff, div, eikonal, dx = (float(v) for v in (band, gain, diff, div, eikonal, dx))
        if not (math.isfinite(gain) and gain >= 0.0):
            raise ValueError(f"InterfaceLpLoss: gain = {gain!r} must be finite and >= 0")
        if gain > 0.0 and not (math.isfinite(band) and band > 0.0):
            raise ValueError(f"InterfaceLpLoss: band = {band!r} must be positive and finite (the units of the signed distance)")
        if not (math.isfinite(div) and div != 0.0 and math.isfinite(diff)):
            raise ValueError(f"InterfaceLpLoss: diff = {diff!r}, div = {div!r} must be finite and div not 0")
        if not (math.isfinite(eikonal) and eikonal >= 0.0 and math.isfinite(dx) and dx > 0.0):
            raise ValueError(f"InterfaceLpLoss: eikonal = {eikonal!r} must be finite and >= 0, dx = {dx!r} positive")
        if field_weights is not None:
            field_weights = tuple(float(a) for a in field_weights)
            if not all(math.isfinite(a) and a >= 0.0 for a in field_weights):
                raise ValueError(f"InterfaceLpLoss: field weights {field_weights} must be finite and >= 0")
        self.sdf_channel, self.band, self.gain, self.diff, self.div = sdf_channel, band, gain, diff, div
        self.field_weights, self.eikonal, self.dx = field_weights, eikonal, dx
        self._terms = None

    @classmethod
    def for_dataset(cls, ds, band: float, gain: float, sdf_field: str = "dfun", field_weights=None, eikonal: float = 0.0):
        """The criterion of a normalised dataset (data.BubbleForecast): the channel of ``sdf_field`` among ``ds.output_fields``, its constants
        from ``ds.diff_terms`` / ``ds.div_terms``, dx = ds.downsample_factor / 32; ``field_weights`` a sequence in the order of the output
        fields or a dict by field name (fields it does not name weigh 1)."""
        fields = list(ds.output_fields)
        if sdf_field not in fields:
            raise ValueError(f"InterfaceLpLoss: the dataset's output fields {fields} have no {sdf_field!r}")
        s = fields.index(sdf_field)
        if isinstance(field_weights, dict):
            unknown = [k for k in field_weights if k not in fields]
            if unknown:
                raise ValueError(f"InterfaceLpLoss: field weights name {unknown}, not among the output fields {fields}")
            field_weights = [float(field_weights.get(n, 1.0)) for n in fields]
        try:
            diff, div = float(ds.diff_terms[sdf_field]), float(ds.div_terms[sdf_field])
        except (KeyError, TypeError, ValueError):
            raise ValueError(f"InterfaceLpLoss: the dataset has no normalisation constants for {sdf_field!r} (call normalize() first)") from None
        return cls(s, band, gain, diff=diff, div=div, field_weights=field_weights, eikonal=eikonal,
                   dx=EIKONAL_DX * float(getattr(ds, "downsample_factor", 1)))

    def _abi_args(self, Cn: int):
        a = self.field_weights
        if a is not None and len(a) != Cn:
            raise L.BubbleformerHipError(f"InterfaceLpLoss: {len(a)} field weights for {Cn} fields")
        import ctypes
        arr = (ctypes.c_double * Cn)(*a) if a is not None else None      # read by the library during the call only
        return (self.sdf_channel, self.diff, self.div, self.band, self.gain, arr, self.eikonal, self.dx)

    def forward(self, pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        _require_gpu_f32(pred, "InterfaceLpLoss")
        _require_gpu_f32(y, "InterfaceLpLoss")
        if y.requires_grad and torch.is_grad_enabled():
            raise L.BubbleformerHipError("InterfaceLpLoss: a gradient w.r.t. the target is not implemented (the target must not require grad)")
        if pred.shape != y.shape:
            raise L.BubbleformerHipError(f"InterfaceLpLoss: prediction {tuple(pred.shape)} and target {tuple(y.shape)} differ in shape")
        if pred.dim() != 5:
            raise L.BubbleformerHipError(f"InterfaceLpLoss expects (B, T, C, H, W); got {tuple(pred.shape)}")
        if pred.numel() == 0:
            raise L.BubbleformerHipError("InterfaceLpLoss: empty input")
        if pred.shape[2] <= self.sdf_channel:
            raise L.BubbleformerHipError(f"InterfaceLpLoss: sdf_channel = {self.sdf_channel} lies outside the {pred.shape[2]} fields of {tuple(pred.shape)}")
        return _InterfaceLpFn.apply(pred, y, self)

    def _last(self) -> torch.Tensor:
        if self._terms is None:
            raise L.BubbleformerHipError("InterfaceLpLoss: no forward has run yet")
        return self._terms

    def field_terms(self) -> torch.Tensor:
        """(C,) fp32 on the device: field_weights[c] * mean_{b,t} rho[b, t, c] of the last forward."""
        return self._last()[1:].clone()

    def eikonal_term(self) -> torch.Tensor:
        """The Eikonal penalty of the last forward (0 where eikonal = 0): a 0-dim fp32 tensor on the device."""
        return self._last()[0].clone()


_SLP_WS_BYTES = {}      # (frames, C, H, W) -> bf_slp_ws_bytes


class _SpectralLpFn(torch.autograd.Function):
    """(pred, y) -> the scalar of SpectralLpLoss; the criterion keeps the terms the forward left on the device."""

    @staticmethod
    def forward(ctx, pred, y, crit):
        import ctypes
        B, T, Cn, H, W = pred.shape
        frames = B * T
        pred, y = pred.contiguous(), y.contiguous()
        lib = L.lib()
        nws = _SLP_WS_BYTES.get((frames, Cn, H, W))
        if nws is None:
            nws = _SLP_WS_BYTES[(frames, Cn, H, W)] = lib.bf_slp_ws_bytes(frames, Cn, H, W)
        if nws < 0:
            raise L.BubbleformerHipError(f"SpectralLpLoss: {frames} frames of {Cn} x {H} x {W} are out of range (a side may be at most 1024)")
        table, host = crit._tables(Cn, pred.device)
        a = crit.field_weights
        weights = (ctypes.c_double * Cn)(*a) if a is not None else None      # read by the library during the call only
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        terms = torch.empty(2 * Cn, dtype=torch.float32, device=pred.device)
        sums = torch.empty(2 * frames * Cn, dtype=torch.float64, device=pred.device)
        spec = torch.empty((frames * Cn, H, W // 2 + 1, 2), dtype=torch.float32, device=pred.device)      # the one saved intermediate
        ws = torch.empty(nws, dtype=torch.uint8, device=pred.device)
        L.check(lib.bf_slp_fwd(pred.data_ptr(), y.data_ptr(), frames, Cn, H, W, table.data_ptr(), host, table.shape[1], weights, loss.data_ptr(),
                               terms.data_ptr(), sums.data_ptr(), spec.data_ptr(), ws.data_ptr(), nws, _stream()), "bf_slp_fwd")
        ctx.save_for_backward(spec, sums)
        ctx.args = (frames, Cn, H, W, weights)
        ctx.like = (pred.shape, (pred.data_ptr() % 16) // 4, pred.device)      # the gradient's shape and offset: pred itself is not kept
        crit._terms = terms
        return loss

    @staticmethod
    def backward(ctx, g):
        spec, sums = ctx.saved_tensors
        g = g.contiguous().float().reshape(1)
        shape, off, device = ctx.like
        dpred = torch.empty(math.prod(shape) + off, dtype=torch.float32, device=device)[off:].view(shape)
        L.check(L.lib().bf_slp_bwd(spec.data_ptr(), g.data_ptr(), sums.data_ptr(), *ctx.args, dpred.data_ptr(), _stream()), "bf_slp_bwd")
        return dpred, None, None


class SpectralLpLoss(nn.Module):
    """The relative L2 of LpLoss's training configuration taken in Fourier space, with one weight per radial shell and per field -- a native
    criterion for ``TrainStep(criterion=...)`` / ``fit(criterion=...)`` (csrc/spectral_loss.hip: bf_slp_fwd / bf_slp_bwd; no reference program;
    DESIGN.md section 30).

    pred, y: (B, T, C, H, W) fp32 on the GPU in normalised units; y never requires a gradient.  With E, Y the unnormalised 2-D DFTs of
    pred - y and y, and q(k) the shell of mode k as ``physics.field_errors`` counts it (``physics.shell_count(H, W)`` = K shells; the rows of
    ``spectrum_*`` index the same shells as this table):
        S_e  = sum_k w[c][q(k)] |E_k|^2 / (H W),   S_y the same sum over Y,   rho = sqrt(S_e / S_y)      per (b, t, c)
        L    = sum_c field_weights[c] * mean_{b,t} rho
    ``shell_weights`` is a (C, K) table of weights >= 0 (a (K,) table is broadcast over the fields; a field whose table is all zero is refused).
    w = 1 and unit field weights give ``LpLoss(d=2, p=2, reduce_dims=[0, 1, 2], reductions=["mean", "mean", "sum"])`` up to the transform's
    rounding.  The criterion is bound to the grid whose shell count its table has (``grid=(H, W)``, or the first grid it meets); another grid
    is refused.

    The transforms are fp32, every sum fp64 in a fixed order: two calls give the same bits.  The fp32 noise floor of a transform is about
    eta^2 of a field's TOTAL power, eta = (8 log2(H W) + ...) 2^-24 (7e-6 at 192 x 192): weights whose range approaches 1 / eta^2 make S_y of a
    smooth target noise-dominated.  The forward saves one intermediate for the backward, frames * H * (W/2 + 1) * 8 bytes with frames =
    B * T * C (76 MB at (8, 16, 4, 192, 192)), per pass of an unrolled step.

    ``gain``, ``power`` and ``floor`` of the constructors below have no defaults: no value has been validated by a training run.
    ``field_terms()`` returns the C values ``field_weights[c] * mean rho`` of the last forward, ``plain_terms()`` the same at w = 1 (the plain
    relative L2, for monitoring), as device tensors (clones; no host synchronisation)."""

    def __init__(self, shell_weights, *, field_weights=None, grid=None):
        super().__init__()
        w = torch.as_tensor(shell_weights).detach().to("cpu", torch.float64).contiguous()
        if w.dim() == 1:
            w = w[None]
        if w.dim() != 2 or w.shape[1] == 0 or w.shape[0] == 0:
            raise ValueError(f"SpectralLpLoss: shell weights must be a (K,) or (C, K) table; got {tuple(w.shape)}")
        if not bool((torch.isfinite(w) & (w >= 0)).all()):
            raise ValueError("SpectralLpLoss: shell weights must be finite and >= 0")
        if not bool((w > 0).any(dim=1).all()):
            raise ValueError("SpectralLpLoss: a field's shell weights are all zero")
        if field_weights is not None:
            field_weights = tuple(float(a) for a in field_weights)
            if not all(math.isfinite(a) and a >= 0.0 for a in field_weights):
                raise ValueError(f"SpectralLpLoss: field weights {field_weights} must be finite and >= 0")
            if w.shape[0] not in (1, len(field_weights)):
                raise ValueError(f"SpectralLpLoss: {len(field_weights)} field weights for a table of {w.shape[0]} fields")
        if grid is not None:
            from .physics import shell_count
            grid = (int(grid[0]), int(grid[1]))
            if shell_count(*grid) != w.shape[1]:
                raise ValueError(f"SpectralLpLoss: a {grid[0]} x {grid[1]} grid has {shell_count(*grid)} shells; the table has {w.shape[1]}")
        self.shell_weights, self.field_weights, self.grid = w, field_weights, grid
        self._device_tables = {}      # (device, C) -> ((C, K) fp64 on the device, the same table as a ctypes array); made once, never moved
        self._terms = None

    @classmethod
    def power_law(cls, H: int, W: int, gain: float, power: float, C=None, *, field_weights=None):
        """w[q] = 1 + gain * (q / (K - 1))^power on the shells of an H x W grid, the same for every field (C: the number of rows, None = one
        row that is broadcast).  gain >= 0 and power > 0; neither has a default."""
        from .physics import shell_count
        gain, power = float(gain), float(power)
        if not (math.isfinite(gain) and gain >= 0.0 and math.isfinite(power) and power > 0.0):
            raise ValueError(f"SpectralLpLoss: gain = {gain!r} must be finite and >= 0, power = {power!r} finite and > 0")
        K = shell_count(H, W)
        q = torch.arange(K, dtype=torch.float64) / max(K - 1, 1)
        w = 1.0 + gain * q ** power
        return cls(w if C is None else w[None].repeat(int(C), 1), field_weights=field_weights, grid=(H, W))

    @classmethod
    def from_spectrum(cls, spectrum_target, floor: float, *, field_weights=None, grid=None):
        """Whitening weights from a measured target spectrum P_y (C, K) or (K,) -- the mean over frames of
        ``physics.field_errors(...).spectrum_target``: w[c][q] proportional to 1 / max(P_y[c][q], floor * max_q P_y[c]), scaled so that
        sum_q w P_y = sum_q P_y (a target with that spectrum keeps its S_y).  0 < floor <= 1; it has no default."""
        floor = float(floor)
        if not (math.isfinite(floor) and 0.0 < floor <= 1.0):
            raise ValueError(f"SpectralLpLoss: floor = {floor!r} must lie in (0, 1]")
        P = torch.as_tensor(spectrum_target).detach().to("cpu", torch.float64)
        if P.dim() == 1:
            P = P[None]
        if P.dim() != 2 or not bool((torch.isfinite(P) & (P >= 0)).all()) or not bool((P.amax(dim=1) > 0).all()):
            raise ValueError("SpectralLpLoss: the target spectrum must be a finite (K,) or (C, K) table >= 0 with power in every field")
        w = 1.0 / torch.maximum(P, floor * P.amax(dim=1, keepdim=True))
        w = w * (P.sum(dim=1, keepdim=True) / (w * P).sum(dim=1, keepdim=True))
        return cls(w, field_weights=field_weights, grid=grid)

    def _tables(self, Cn: int, device):
        key = (str(device), Cn)
        got = self._device_tables.get(key)
        if got is None:
            import ctypes
            w = self.shell_weights
            if w.shape[0] not in (1, Cn):
                raise L.BubbleformerHipError(f"SpectralLpLoss: a table of {w.shape[0]} fields for {Cn} fields")
            if self.field_weights is not None and len(self.field_weights) != Cn:
                raise L.BubbleformerHipError(f"SpectralLpLoss: {len(self.field_weights)} field weights for {Cn} fields")
            full = w.expand(Cn, w.shape[1]).contiguous()
            got = self._device_tables[key] = (full.to(device), (ctypes.c_double * full.numel())(*full.flatten().tolist()))
        return got

    def forward(self, pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        _require_gpu_f32(pred, "SpectralLpLoss")
        _require_gpu_f32(y, "SpectralLpLoss")
        if y.requires_grad and torch.is_grad_enabled():
            raise L.BubbleformerHipError("SpectralLpLoss: a gradient w.r.t. the target is not implemented (the target must not require grad)")
        if pred.shape != y.shape:
            raise L.BubbleformerHipError(f"SpectralLpLoss: prediction {tuple(pred.shape)} and target {tuple(y.shape)} differ in shape")
        if pred.dim() != 5:
            raise L.BubbleformerHipError(f"SpectralLpLoss expects (B, T, C, H, W); got {tuple(pred.shape)}")
        if pred.numel() == 0:
            raise L.BubbleformerHipError("SpectralLpLoss: empty input")
        from .physics import shell_count
        H, W = pred.shape[-2:]
        K = self.shell_weights.shape[1]
        if (self.grid is not None and (H, W) != self.grid) or shell_count(H, W) != K:
            bound = f"the {self.grid[0]} x {self.grid[1]} grid" if self.grid is not None else "a grid"
            raise L.BubbleformerHipError(f"SpectralLpLoss: the table is bound to {bound} of {K} shells; got {H} x {W} ({shell_count(H, W)} shells)")
        self._tables(pred.shape[2], pred.device)      # refuses a wrong number of fields before the grid is bound
        if self.grid is None:
            self.grid = (H, W)
        return _SpectralLpFn.apply(pred, y, self)

    def _last(self) -> torch.Tensor:
        if self._terms is None:
            raise L.BubbleformerHipError("SpectralLpLoss: no forward has run yet")
        return self._terms

    def field_terms(self) -> torch.Tensor:
        """(C,) fp32 on the device: field_weights[c] * mean_{b,t} rho[b, t, c] of the last forward."""
        t = self._last()
        return t[:t.numel() // 2].clone()

    def plain_terms(self) -> torch.Tensor:
        """(C,) fp32 on the device: the same terms at w = 1, the plain relative L2 per field of the last forward."""
        t = self._last()
        return t[t.numel() // 2:].clone()
