"""Golden values for utils.losses, generated on the CPU from the reference's own bubbleformer/utils/losses.py.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_losses_golden.py [--reference /path/to/Bubbleformer]

writes tests/golden/losses.npz: seeded fp32 inputs and, from the reference's `LpLoss` run in fp64 on those inputs, the value and
d/dpred of sum(value * weight) (a seeded weight of the value's shape, so that a non-scalar result has every row's gradient pinned) for the
configurations of CONFIGS; and the reference's `eikonal_loss` value and gradient on a non-square field.  The reference file is loaded by
path, without importing its package and without leaving byte code in its checkout."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPE = (2, 3, 4, 8, 12)
# name -> (constructor arguments, batch size taken from the front of the inputs)
CONFIGS = {
    "training": (dict(d=2, p=2, reduce_dims=[0, 1, 2], reductions=["mean", "mean", "sum"]), 2),
    "inference": (dict(d=2, p=2, reduce_dims=[0, 1], reductions=["mean", "mean"]), 2),
    "defaults": (dict(), 2),
    "d3_none": (dict(d=3, reduce_dims=None), 2),
    "p1_mean": (dict(d=2, p=1, reduce_dims=[0, 1, 2], reductions="mean"), 2),
    "p3": (dict(d=2, p=3, reduce_dims=[0, 1, 2], reductions=["mean", "mean", "sum"]), 2),
    "p2_5": (dict(d=2, p=2.5, reduce_dims=[0, 1, 2], reductions=["mean", "mean", "sum"]), 2),
    "squeeze_b1": (dict(d=2, p=2, reduce_dims=[1], reductions="mean"), 1),
}
EIKONAL_SHAPE = (2, 3, 10, 14)


def inputs():
    g = torch.Generator().manual_seed(20240)
    pred = torch.randn(SHAPE, generator=g, dtype=torch.float32)
    y = torch.randn(SHAPE, generator=g, dtype=torch.float32) * 1.5 + 0.25
    yy, xx = torch.meshgrid(torch.arange(EIKONAL_SHAPE[-2], dtype=torch.float64), torch.arange(EIKONAL_SHAPE[-1], dtype=torch.float64), indexing="ij")
    base = torch.sqrt((yy - 4.3) ** 2 + (xx - 6.1) ** 2) / 32 - 0.11          # a signed distance to a circle, in grid units of 1/32
    phi = (base + 0.02 * torch.randn(EIKONAL_SHAPE, generator=g, dtype=torch.float64)).float()
    return pred, y, phi


def weight(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) + 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="checkout of the reference implementation (default: oracle/gen_golden.py's)")
    args = ap.parse_args()
    from oracle import gen_golden
    ref = args.reference or gen_golden.REF
    spec = importlib.util.spec_from_file_location("_reference_losses", os.path.join(ref, "bubbleformer", "utils", "losses.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    pred, y, phi = inputs()
    out = {"pred": pred.numpy(), "y": y.numpy(), "phi": phi.numpy(), "names": np.array(list(CONFIGS))}
    for i, (name, (kw, B)) in enumerate(CONFIGS.items()):
        a = pred[:B].double().requires_grad_(True)
        val = R.LpLoss(**kw)(a, y[:B].double())
        w = weight(val.shape, 700 + i)
        (val * w).sum().backward()
        out[f"{name}/value"], out[f"{name}/weight"], out[f"{name}/dpred"] = val.detach().numpy(), w.numpy(), a.grad.numpy()
        print(f"{name}: value shape {tuple(val.shape)}")
    a = phi.double().requires_grad_(True)
    val = R.eikonal_loss(a)
    val.backward()
    out["eikonal/value"], out["eikonal/dphi"] = val.detach().numpy(), a.grad.numpy()
    assert np.isfinite(out["eikonal/dphi"]).all()
    path = os.path.join(GOLDEN, "losses.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
