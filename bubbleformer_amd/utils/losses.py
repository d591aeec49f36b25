"""The reference's criterion and physics penalty as native, differentiable ops (reference: bubbleformer/utils/losses.py).

``LpLoss`` has the reference's constructor, attributes and reduction behaviour; its relative Lp norm per row and the gradient of it run
in csrc/losses.hip (bf_lp_rows_fwd / bf_lp_rows_bwd), the reductions over the leading dims are ordinary torch ops on the small tensor of
per-row ratios.  ``eikonal_loss`` is `physics.eikonal_loss` with a backward (bf_eikonal_bwd).  Inputs are fp32 tensors on the GPU; there
is no CPU path.
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
