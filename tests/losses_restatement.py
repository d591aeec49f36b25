"""Plain-PyTorch restatement of the reference's criterion for the parity tests, written from the maths, in whatever dtype / device the
inputs are in; pinned on the CPU in fp64 by tests/golden/losses.npz (the reference's own results).  The Eikonal residual is
oracle.filmavit_ref.eikonal_loss."""
import torch

from oracle.filmavit_ref import eikonal_loss  # noqa: F401


def lp_rows(pred, y, d=1, p=2):
    """(sum |pred - y|^p / sum |y|^p)^(1/p) over the last d dims."""
    e, t = (pred - y).flatten(-d), y.flatten(-d)
    return (e.abs().pow(p).sum(-1) / t.abs().pow(p).sum(-1)).pow(1.0 / p)


def lp_loss(pred, y, d=1, p=2, reduce_dims=0, reductions="sum"):
    """LpLoss(d, p, reduce_dims, reductions)(pred, y): the per-row ratios, each listed dim summed or averaged in turn, size-1 dims dropped."""
    r = lp_rows(pred, y, d, p)
    if reduce_dims is None:
        return r
    dims = [reduce_dims] if isinstance(reduce_dims, int) else list(reduce_dims)
    hows = [reductions] * len(dims) if isinstance(reductions, str) else list(reductions)
    for dim, how in zip(dims, hows):
        r = r.sum(dim, keepdim=True) if how == "sum" else r.mean(dim, keepdim=True)
    return r.squeeze()
