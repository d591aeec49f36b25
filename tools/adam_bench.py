#!/usr/bin/env python3
"""Fused optimizer kernels, timed on the GPU: prints one JSON object.

bf_adam (torch.optim.Adam) against bf_adamw (torch.optim.AdamW) on the flat fp32 buffers TrainStep keeps for FiLMAViT-small
(E 384, 6 heads, 12 blocks) and film_avit_big (E 768, 12 heads, 12 blocks), sized as trainer.FlatParams lays them out (every parameter
padded to 64 elements).  Each step reads p, g, m, v and writes p, m, v: 28 bytes per element.  The two kernels alternate in rounds of
`--reps` back-to-back launches timed by device events; the per-launch time is the median over rounds.  Reported: ms per launch, GB/s,
and the share of the 8.0 TB/s HBM peak (MI355X_MICROARCH: about 6.3 TB/s is achievable by a float4 copy).

Usage: python tools/adam_bench.py [--rounds R] [--reps K]"""
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
from oracle import weights as W  # noqa: E402

MODELS = {
    "filmavit_small": dict(input_fields=4, output_fields=4, patch_size=16, embed_dim=384, num_heads=6, processor_blocks=12, num_fluid_params=9),
    "film_avit_big": dict(input_fields=4, output_fields=4, patch_size=16, embed_dim=768, num_heads=12, processor_blocks=12, num_fluid_params=9),
}
BYTES_PER_ELEMENT = 28
HBM_PEAK = 8.0e12


def flat_sizes(cfg, align=64):
    n = p = 0
    for shape in W.param_shapes(**cfg).values():
        k = 1
        for s in shape:
            k *= s
        p += k
        n += (k + align - 1) // align * align
    return p, n


def time_kernels(n, rounds, reps):
    g = torch.Generator(device="cuda").manual_seed(0)
    p = torch.randn(n, device="cuda", generator=g) * 0.02
    grad = torch.randn(n, device="cuda", generator=g) * 1e-3
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    h, st = L.lib(), _stream()
    calls = {
        "adam": lambda: h.bf_adam(_p(p), _p(grad), _p(m), _p(v), n, 10, 2.5e-4, 0.9, 0.999, 1e-8, 1e-5, 1.0, st),
        "adamw": lambda: h.bf_adamw(_p(p), _p(grad), _p(m), _p(v), n, 10, 2.5e-4, 0.9, 0.999, 1e-8, 1e-2, 1.0, st),
    }
    for f in calls.values():                         # warm-up: code objects loaded, buffers touched
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
    assert torch.isfinite(p).all()
    out = {}
    for k, t in ms.items():
        med = statistics.median(t)
        gbs = BYTES_PER_ELEMENT * n / (med * 1e-3) / 1e9
        out[k] = {"ms": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4), "GB_s": round(gbs, 1),
                  "hbm_peak_share": round(gbs * 1e9 / HBM_PEAK, 3)}
    out["adam_over_adamw"] = round(out["adam"]["ms"] / out["adamw"]["ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/adam_bench.py times GPU kernels: no GPU found"
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "bytes_per_element": BYTES_PER_ELEMENT}
    for name, cfg in MODELS.items():
        params, n = flat_sizes(cfg)
        res[name] = dict(parameters=params, flat_elements=n, **time_kernels(n, args.rounds, args.reps))
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
