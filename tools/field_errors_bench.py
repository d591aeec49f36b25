#!/usr/bin/env python3
"""The error rows of a rollout step (bf_rollout_errors, csrc/spectra.hip), timed on one GPU: prints one JSON object.

  call:     the step call alone at the bench geometry (B = 8 trajectories, T = 16, C = 4, 192 x 192: 512 frames per step), with and without
            the spectra, by device events over back-to-back launches, median of the rounds; and the same rows written in stock torch ops on
            the same GPU: `gather` of the target clips, fp64 casts, `torch.fft.rfft2`, `index_add_` by shell over the weighted half plane,
            two 3 x 3 max-pools for the interface mask.  `agree` is the largest relative gap between the two routes' rows.
  rollout:  ms per step of `evaluate_rollouts` with and without `errors=ErrorSpec()`: FiLMAViT-small bf16, graph, `off` and `on` alternated
            inside every round, the order flipped every round; ms per step is (t(50 steps) - t(10 steps)) / 40 as tools/rollout_eval_bench.py
            defines it.

Usage: python tools/field_errors_bench.py [--rounds R] [--only call|rollout]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEPS, SHORT, T, H, W, NTRAJ = 50, 10, 16, 192, 192, 8


def stock_rows(pred, store, starts, sdf_frames, half_table, weight, K, lo, hi, spectra):
    """The rows of one step in stock torch ops; returns the dict of fp32 rows (interface_cells int32)."""
    tgt = store.gather(starts)[1]
    p, y = pred.double(), tgt.double()
    e = p - y
    e2 = e * e
    out = {"rmse": e2.mean((-1, -2)).sqrt(), "max_error": e.abs().amax((-1, -2))}
    ring = e2[..., 0, :].sum(-1) + e2[..., -1, :].sum(-1) + e2[..., 1:-1, 0].sum(-1) + e2[..., 1:-1, -1].sum(-1)
    out["boundary_rmse"] = (ring / (2 * H + 2 * W - 4)).sqrt()
    vap = (store.frames[0, sdf_frames] > 0).float().unsqueeze(1)                      # (B*T, 1, H, W) raw stored frames
    pool = lambda m: torch.nn.functional.max_pool2d(m, 3, 1, 1)
    mask = ((pool(vap) > 0) & (pool(1 - vap) > 0)).reshape(pred.shape[0], pred.shape[1], 1, H, W)
    cells = mask.sum((-1, -2))
    out["interface_rmse"] = ((e2 * mask).sum((-1, -2)) / cells).sqrt()
    out["interface_cells"] = cells.expand(-1, -1, pred.shape[2]).to(torch.int32)
    if spectra:
        for name, x in (("spectrum_error", e), ("spectrum_pred", p), ("spectrum_target", y)):
            X = torch.fft.rfft2(x)
            power = (X.real ** 2 + X.imag ** 2) * weight
            shells = torch.zeros((x.numel() // (H * W), K), dtype=torch.float64, device=x.device).index_add_(1, half_table, power.reshape(-1, power.shape[-2] * power.shape[-1]))
            out[name] = shells.reshape(x.shape[:-2] + (K,))
        pe = out["spectrum_error"]
        out["spectral_error"] = torch.stack([pe[..., :lo].sum(-1), pe[..., lo:hi].sum(-1), pe[..., hi:].sum(-1)], -1).sqrt()
    return {k: v if v.dtype == torch.int32 else v.float() for k, v in out.items()}


def bench_call(rounds):
    from bubbleformer_amd import ops
    from bubbleformer_amd.utils.rollout import plan_rollouts
    from tests import errors_restatement as R
    from tools.bubble_census_bench import device_time, med
    from tools.rollout_eval_bench import study
    store = study()
    B, C, lo, hi = NTRAJ, 4, 4, 12
    starts = [i * len(store.ds) // NTRAJ for i in range(B)]
    host_first = plan_rollouts(store.ds, starts, STEPS).first
    first = torch.tensor(host_first, dtype=torch.int64, device="cuda")
    pred = (store.gather(starts)[1] + 0.01 * torch.randn((B, T, C, H, W), device="cuda")).contiguous()
    K = R.shell_count(H, W)
    tails = {"spectral_error": (3,), "spectrum_error": (K,), "spectrum_pred": (K,), "spectrum_target": (K,)}
    keys = ("rmse", "max_error", "boundary_rmse", "interface_rmse", "interface_cells", "spectral_error", "spectrum_error", "spectrum_pred", "spectrum_target")
    rows = {k: torch.zeros((B, STEPS * T, C) + tails.get(k, ()), dtype=torch.int32 if k == "interface_cells" else torch.float32, device="cuda") for k in keys}
    ws = ops.field_errors_workspace(B * T * C, H, W, "cuda")
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = {"frames_per_step": B * T * C, "shells": K, "workspace_bytes": ws.numel()}
    for name, spectra in (("with_spectra", True), ("pointwise_only", False)):
        call = lambda: ops.rollout_errors(pred, store.frames, first, counter, store.out_tab, 0, STEPS, ws, 1, lo, hi, spectra, **rows)
        out[f"native_{name}_ms"] = med([device_time(call) * 1e3 for _ in range(rounds)])
    table = torch.from_numpy(R.shell_table(H, W)[:, :W // 2 + 1].reshape(-1).copy()).cuda()
    weight = torch.full((W // 2 + 1,), 2.0, dtype=torch.float64, device="cuda")
    weight[0] = 1.0
    if W % 2 == 0:
        weight[-1] = 1.0
    weight = weight / float(H * W) ** 2
    sdf_frames = torch.tensor([f + T + t for f in host_first for t in range(T)], dtype=torch.int64, device="cuda")
    idx = [s + 0 for s in starts]
    for name, spectra in (("with_spectra", True), ("pointwise_only", False)):
        call = lambda: stock_rows(pred, store, idx, sdf_frames, table, weight, K, lo, hi, spectra)
        out[f"stock_{name}_ms"] = med([device_time(call) * 1e3 for _ in range(rounds)])
    stock = stock_rows(pred, store, idx, sdf_frames, table, weight, K, lo, hi, True)
    gaps = {}
    for k in keys:
        g, w = rows[k][:, :T].double(), stock[k].double()
        gaps[k] = float(((g - w).abs() / w.abs().clamp_min(1e-300)).max()) if k.startswith("spectrum") is False else float(((g - w).abs().sum(-1) / w.sum(-1)).max())
    out["agree"] = {k: float(f"{v:.3e}") for k, v in gaps.items()}
    return out


def bench_rollout(rounds):
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils import ErrorSpec
    from bubbleformer_amd.utils import rollout as Ro
    from oracle import weights as Wt
    from tools.bubble_census_bench import med
    from tools.rollout_eval_bench import CFG, clock, study
    model = get_model("filmavit", time_window=T, drop_path=0.0, compute_dtype=torch.bfloat16, **CFG)
    model.load_state_dict(Wt.generate(Wt.param_shapes(**CFG), seed=42))
    model = model.cuda().eval()
    store = study()
    starts = [i * len(store.ds) // NTRAJ for i in range(NTRAJ)]
    variants = {"off": {}, "on": {"errors": ErrorSpec()}, "on_pointwise_only": {"errors": ErrorSpec(spectra=False)}}
    times = {k: [] for k in variants}
    for r in range(rounds + 1):                                         # round 0 is dropped; the order of the variants flips every round
        for name, kw in (list(variants.items())[::-1] if r % 2 else list(variants.items())):
            run = lambda steps: Ro.evaluate_rollouts(model, store, starts, steps, use_graph=True, **kw)
            pair = (clock(lambda: run(STEPS)), clock(lambda: run(SHORT)))
            if r:
                times[name].append(pair)
    out = {name: {"ms_per_step": med([(a - b) / (STEPS - SHORT) * 1e3 for a, b in times[name]])} for name in variants}
    for name in ("on", "on_pointwise_only"):
        out[f"{name}_marginal_ms_per_step"] = round(out[name]["ms_per_step"]["median"] - out["off"]["ms_per_step"]["median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=("call", "rollout"), default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("field_errors_bench needs a GPU", file=sys.stderr)
        return 1
    out = {"rounds": a.rounds, "geometry": [NTRAJ, T, 4, H, W]}
    if a.only in (None, "call"):
        out["call"] = bench_call(a.rounds)
    if a.only in (None, "rollout"):
        out["rollout"] = bench_rollout(a.rounds)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
