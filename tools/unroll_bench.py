#!/usr/bin/env python3
"""The training step unrolled through k of the model's own predictions, timed on the GPU: prints one JSON object.

FiLMAViT-small (E 384, 6 heads, 12 blocks, stochastic depth 0.2) at the headline shape -- 4 fields, 16 x 192 x 192 clips, batch 8, bf16,
AdamW -- as bench.py runs it.  Versions, each a model and a TrainStep of its own from the same seed:
  k1                     the plain step (unroll_steps = 1)
  k2 / k3                unroll_steps = 2 / 3, gradients through the fed-back predictions (unroll_backprop=True), fused loss
  k2_push / k3_push      the pushforward form (unroll_backprop=False), fused loss
  k2_composed            unroll_steps = 2 through model(x) and criterion = LpLoss(d=2, p=2, mean B, mean T, sum C): the only way to unroll
                         before the last debed stage's backward took both gradient sources
With ``--input-noise STD`` every version named is timed a second time as ``<version>_noise``: the same step with
``input_noise=NoiseSpec(STD)`` (seeded Gaussian noise on the input clip and on every fed-back prediction, one bf_clip_noise launch per
pass, sample ids resident on the device), and "clip_noise" reports the kernel alone on the input clip: microseconds per launch by
device events over 200 back-to-back launches and the rate of its 2 x clip bytes.
With ``--weight-average`` every version named is also timed as ``<version>_avg``: the same step with
``weight_average=AverageSpec("ema", 0.999)`` (the averaged copy of the weights kept inside the optimizer kernel), and "avg_cost_us" is
its median minus the plain version's.
After a warm-up of every version they alternate in rounds of `--reps` back-to-back optimizer steps timed by device events; reported per
version: the median over rounds of the time per step with the minimum and the maximum, and for the unrolled ones the ratio to k x the
k1 step.  "peak_memory_GB" is the process's `max_memory_allocated`: with `--versions <one>` it is that version's (every version named
is resident at once).  "fused_not_slower" holds when the fused k = 2 step's median is at most the composed one's.

Usage: python tools/unroll_bench.py [--rounds R] [--reps K] [--batch B] [--versions k1,k3_push,...] [--input-noise STD] [--weight-average]"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from bench import CFG, DROP_PATH, FIELD_STATS  # noqa: E402

T, H, W = 16, 192, 192
VERSIONS = {"k1": (1, True, False), "k2": (2, True, False), "k2_push": (2, False, False), "k3": (3, True, False), "k3_push": (3, False, False),
            "k2_composed": (2, True, True)}


def clip(B, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(B, T, 4, H, W, device=dev, generator=g)
    for c, (mu, sd) in enumerate(FIELD_STATS):
        x[:, :, c].mul_(sd).add_(mu)
    return x


def base_version(name):
    for suffix in ("_noise", "_avg"):
        if name.endswith(suffix):
            return name[:-len(suffix)]
    return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--versions", default=",".join(VERSIONS))
    ap.add_argument("--input-noise", type=float, default=None, metavar="STD")
    ap.add_argument("--weight-average", action="store_true", help="also time every version with an EMA of the weights kept by the optimizer kernel")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("unroll_bench.py times the step on the GPU: no GPU here, nothing measured")
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.losses import LpLoss
    dev = torch.device("cuda:0")
    x = clip(a.batch, 1, dev)
    ys = torch.stack([clip(a.batch, 2 + j, dev) for j in range(3)])
    fluid = torch.randn(a.batch, CFG["num_fluid_params"], device=dev, generator=torch.Generator(device=dev).manual_seed(9))
    steps = {}
    names = a.versions.split(",")
    if a.input_noise is not None:
        from bubbleformer_amd.utils import NoiseSpec, add_gaussian_noise
        names = [n + suffix for n in names for suffix in ("", "_noise")]
        ids = torch.arange(a.batch, device=dev)
    if a.weight_average:
        from bubbleformer_amd.utils.averaging import AverageSpec
        names = names + [n + "_avg" for n in a.versions.split(",")]
    for name in names:
        noisy, averaged = name.endswith("_noise"), name.endswith("_avg")
        k, backprop, composed = VERSIONS[base_version(name)]
        torch.manual_seed(0)
        model = get_model("filmavit", time_window=T, drop_path=DROP_PATH, compute_dtype=torch.bfloat16, **CFG).to(dev).train()
        crit = LpLoss(d=2, p=2, reduce_dims=[0, 1, 2], reductions=["mean", "mean", "sum"]) if composed else None
        step = TrainStep(model, lr=2.5e-4, weight_decay=1e-2, optimizer="adamw", criterion=crit, unroll_steps=k, unroll_backprop=backprop,
                         input_noise=NoiseSpec(a.input_noise, seed=1) if noisy else None,
                         weight_average=AverageSpec("ema", 0.999) if averaged else None)
        target = ys[0] if k == 1 else ys[:k]
        steps[name] = (lambda s=step, t=target: s(x, fluid, t, sample_ids=ids)) if noisy else (lambda s=step, t=target: s(x, fluid, t))
    for f in steps.values():
        for _ in range(a.warmup):
            loss = f()
        assert torch.isfinite(loss).all()
    torch.cuda.synchronize()
    ms = {n: [] for n in steps}
    for _ in range(a.rounds):
        for n, f in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                f()
            e1.record()
            e1.synchronize()
            ms[n].append(e0.elapsed_time(e1) / a.reps)
    out = {"shape": [a.batch, T, 4, H, W], "dtype": "bf16", "rounds": a.rounds, "reps": a.reps, "peak_memory_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    for n, t in ms.items():
        out[n] = {"ms": round(statistics.median(t), 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3)}
    if a.input_noise is not None:
        for n in a.versions.split(","):
            out[n + "_noise"]["noise_cost_us"] = round(1e3 * (out[n + "_noise"]["ms"] - out[n]["ms"]), 1)
        buf, launches, sig = torch.empty_like(x), 200, torch.full((x.shape[2],), a.input_noise, device=dev)
        for _ in range(10):
            add_gaussian_noise(x, sig, ids, 0, 0, 1, out=buf)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(launches):
            add_gaussian_noise(x, sig, ids, i, 0, 1, out=buf)
        e1.record()
        e1.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / launches
        out["clip_noise"] = {"us_per_launch": round(us, 2), "bytes": 2 * x.numel() * 4, "GB_per_s": round(2 * x.numel() * 4 / us / 1e3, 1)}
    if a.weight_average:
        for n in a.versions.split(","):
            out[n + "_avg"]["avg_cost_us"] = round(1e3 * (out[n + "_avg"]["ms"] - out[n]["ms"]), 1)
    if "k1" in ms:
        for n in ms:
            k = VERSIONS[base_version(n)][0]
            if k > 1:
                out[n]["ratio_to_k_plain_steps"] = round(out[n]["ms"] / (k * out["k1"]["ms"]), 4)
    if "k2" in ms and "k2_composed" in ms:
        out["fused_minus_composed_us"] = round(1e3 * (out["k2"]["ms"] - out["k2_composed"]["ms"]), 1)
        out["checks"] = {"fused_not_slower": out["k2"]["ms"] <= out["k2_composed"]["ms"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
