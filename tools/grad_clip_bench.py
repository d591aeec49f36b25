#!/usr/bin/env python3
"""Gradient-clipping kernels, timed on the GPU: prints one JSON object.

bf_grad_norm (csrc/gradclip.hip: the fp64 fixed-order 2-norm of the flat gradient buffer and the clip coefficient, two launches) and the
three fused optimizers reading that coefficient from device memory (bf_adamw / bf_adam / bf_lion with their record's coef_dev set, with and
without the value clamp: the rows *_dev and *_dev_clamp) beside their host-scale twins (no coefficient, no clamp), all in one run on the flat fp32 buffers TrainStep keeps for
FiLMAViT-small (E 384, 6 heads, 12 blocks; every parameter padded to 64 elements as trainer.FlatParams lays them out).  The kernels
alternate in rounds of `--reps` back-to-back calls timed by device events; reported per kernel: the median over rounds of the time per
call, with the minimum and the maximum, and the bytes it moves per second (the norm reads 4 B per element, AdamW / Adam 28 B, Lion 20 B).

Two conditions are evaluated on the run's own figures and printed under "checks":
  norm_under_adamw     the norm call (n floats read) takes less device time than the AdamW call (4n read, 3n written);
  <opt>_dev_in_spread  each _dev optimizer's median lies within its twin's run-to-run spread (minimum to maximum).

Usage: python tools/grad_clip_bench.py [--rounds R] [--reps K]"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from bubbleformer_amd import _lib as L  # noqa: E402
from bubbleformer_amd.ops import _p, _stream  # noqa: E402
from tools.adam_bench import ADAM, LION, MODELS, flat_sizes, opt_call  # noqa: E402

INF = float("inf")
BYTES = {"grad_norm": 4, "adamw": 28, "adam": 28, "lion": 20}


def time_kernels(n, rounds, reps):
    g = torch.Generator(device="cuda").manual_seed(0)
    p = torch.randn(n, device="cuda", generator=g) * 0.02
    grad = torch.randn(n, device="cuda", generator=g) * 1e-3
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    pair = torch.zeros(2, device="cuda")
    h, st = L.lib(), _stream()
    ws = torch.empty(int(h.bf_grad_norm_ws_doubles(n)), dtype=torch.float64, device="cuda")
    coef = pair[1:].data_ptr()
    steps = {"adamw": lambda **kw: opt_call("bf_adamw", p, grad, m, v, wd=1e-2, **ADAM, **kw), "adam": lambda **kw: opt_call("bf_adam", p, grad, m, v, wd=1e-5, **ADAM, **kw),
             "lion": lambda **kw: opt_call("bf_lion", p, grad, m, **LION, **kw)}
    calls = {"grad_norm": lambda: h.bf_grad_norm(_p(grad), n, 1.0, 1.0, _p(pair), _p(ws), ws.numel(), st)}
    for opt, step in steps.items():          # the _dev rows keep a coefficient that is not null: they time the BF_OPT_DEV kernels
        calls.update({opt: step(), opt + "_dev": step(coef_dev=coef, clip_value=INF), opt + "_dev_clamp": step(coef_dev=coef, clip_value=1e-3)})
    for f in calls.values():                         # warm-up: code objects loaded, buffers touched (the first call leaves a coefficient behind)
        for _ in range(5):
            L.check(f(), "warm-up")
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / reps)
    assert torch.isfinite(p).all() and torch.isfinite(pair).all()
    out = {"grad_norm_slabs": ws.numel()}
    for k, t in ms.items():
        med = statistics.median(t)
        gbs = BYTES[k.split("_dev")[0]] * n / (med * 1e-3) / 1e9
        out[k] = {"ms": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4), "GB_s": round(gbs, 1)}
    checks = {"norm_under_adamw": out["grad_norm"]["ms"] < out["adamw"]["ms"]}
    for k in ("adamw", "adam", "lion"):
        checks[k + "_dev_in_spread"] = out[k]["ms_min"] <= out[k + "_dev"]["ms"] <= out[k]["ms_max"]
    out["checks"] = checks
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/grad_clip_bench.py times GPU kernels: no GPU found"
    params, n = flat_sizes(MODELS["filmavit_small"])
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "model": "filmavit_small", "parameters": params,
           "flat_elements": n}
    res.update(time_kernels(n, args.rounds, args.reps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
