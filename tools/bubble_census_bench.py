#!/usr/bin/env python3
"""Bubble census, timed on one GPU: prints one JSON object.

  census:   `bf_bubble_census` alone (ops.bubble_census, outputs and workspace allocated once) by device events over back-to-back launches:
            32 and 256 frames of 192 x 192 (the frame-sides of one rollout step at B = 1 and B = 8: parents in LDS) and 16 frames of
            512 x 512 (BubbleML's full resolution: parents in the workspace), on smooth random fields with a dozen bubbles per frame and on
            white noise (thousands of components per frame) and the worst cases for the union-find (a full frame, a comb, a checkerboard); and, where scipy imports, the route the census
            replaces for the same frames: archive -> host -> `scipy.ndimage.label` frame by frame (copy and labelling timed apart).
  rollout:  the census call of a step alone, and the marginal cost per step of `evaluate_rollouts(bubbles=spec)`: FiLMAViT-small bf16,
            16 x 192 x 192 x 4 clips, B = 1 and 8 trajectories per forward, graph; `off` and `on` alternated inside every round, the order
            flipped every round; ms per step is (t(50 steps) - t(10 steps)) / 40 as tools/rollout_eval_bench.py defines it.

Usage: python tools/bubble_census_bench.py [--rounds R] [--only census|rollout] [--tree CHECKOUT]
(--tree imports bubbleformer_amd from another checkout of this repository: a tree without the feature runs `off` alone, which is how the
default path is timed against the parent commit -- one process per tree, the processes alternated by the caller)."""
import argparse
import inspect
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

STEPS, SHORT, T, H, W, NTRAJ = 50, 10, 16, 192, 192, 8


def med(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min_max": [round(min(v), digits), round(max(v), digits)]}


def device_time(fn, floor_s=0.05):
    """Seconds per call by device events over a window of at least floor_s (after one untimed call)."""
    fn()
    torch.cuda.synchronize()
    reps = 1
    while True:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        t = ev[0].elapsed_time(ev[1]) * 1e-3
        if t >= floor_s:
            return t / reps
        reps = max(reps * 2, int(reps * floor_s / max(t, 1e-6) * 1.2) + 1)


def fields(kind, frames, h, w):
    from tests import bubbles_restatement as R
    if kind == "smooth":
        one = R.smooth_field((min(frames, 8), h, w), seed=1)
        return np.concatenate([one] * (frames // len(one) + 1))[:frames]
    if kind == "noise":                                                 # white noise, as the synthetic study of tools/rollout_eval_bench.py stores
        return np.random.RandomState(3).standard_normal((frames, h, w)).astype(np.float32)
    y, x = np.mgrid[0:h, 0:w]
    mask = {"full": np.ones((h, w), bool), "comb": (x % 2 == 0) | (y == h - 1), "checkerboard": (y + x) % 2 == 0}[kind]
    return np.broadcast_to(np.where(mask, 1.0, -1.0).astype(np.float32), (frames, h, w)).copy()


def bench_census(rounds):
    from bubbleformer_amd import ops
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    out = {"scipy": ndimage is not None, "lds_cells": ops.bubble_census_lds_cells()}
    mb = 256
    for frames, h, w in ((32, H, W), (256, H, W), (16, 512, 512)):
        for kind in ("smooth", "noise", "full", "comb", "checkerboard"):
            host = fields(kind, frames, h, w)
            phi = torch.from_numpy(host).cuda()
            new = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
            count, cells, attached, area = new(frames), new(frames), new(frames), new(frames, mb)
            ws = ops.bubble_census_workspace(frames, h, w, mb, "cuda")
            call = lambda: ops.bubble_census(phi, 4, mb, ws, count, cells, attached, area)
            row = {"us": med([device_time(call) * 1e6 for _ in range(rounds)], 1), "workspace_bytes": ws.numel()}
            row["bubbles_per_frame"] = [int(count.min()), int(count.max())]
            if ndimage is not None and kind == "smooth":
                copy, lab = [], []
                for _ in range(min(rounds, 3)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    on_host = phi.cpu().numpy()
                    t1 = time.perf_counter()
                    counts = [ndimage.label(f > 0)[1] for f in on_host]
                    t2 = time.perf_counter()
                    copy.append((t1 - t0) * 1e6)
                    lab.append((t2 - t1) * 1e6)
                assert counts == count.cpu().tolist()
                row["scipy_route_us"] = {"copy_to_host": med(copy, 1), "label": med(lab, 1)}
            out[f"{frames}x{h}x{w}_{kind}"] = row
    return out


def bench_rollout(rounds):
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils import rollout as Ro
    from oracle import weights as Wt
    from tools.rollout_eval_bench import CFG, clock, study
    model = get_model("filmavit", time_window=T, drop_path=0.0, compute_dtype=torch.bfloat16, **CFG)
    model.load_state_dict(Wt.generate(Wt.param_shapes(**CFG), seed=42))
    model = model.cuda().eval()
    store = study()
    starts = [i * len(store.ds) // NTRAJ for i in range(NTRAJ)]
    has = "bubbles" in inspect.signature(Ro.evaluate_rollouts).parameters
    spec = None
    if has:
        from bubbleformer_amd.utils import BubbleSpec
        spec = BubbleSpec(dx=16 / 192)
    variants = {}
    for B in (1, 8):
        for name, kw in (("off", {}),) + ((("on", {"bubbles": spec}),) if has else ()):
            def run(steps, B=B, kw=kw):
                for k in range(0, NTRAJ, B):
                    Ro.evaluate_rollouts(model, store, starts[k:k + B], steps, use_graph=True, **kw)
            variants[f"B{B}_{name}"] = (B, run)
    times = {k: [] for k in variants}
    for r in range(rounds + 1):                                         # round 0 is dropped; the order of the variants flips every round
        for name, (_, fn) in (list(variants.items())[::-1] if r % 2 else list(variants.items())):
            pair = (clock(lambda: fn(STEPS)), clock(lambda: fn(SHORT)))
            if r:
                times[name].append(pair)
    out = {"has_bubbles": has}
    if has:                                                             # the census call of a step alone, device events
        from bubbleformer_amd import ops
        for B in (1, 8):
            first = torch.tensor(Ro.plan_rollouts(store.ds, starts[:B], STEPS).first, dtype=torch.int64, device="cuda")
            pred = store.gather(starts[:B])[1] + 0.01
            rows = lambda *tail: [torch.empty((B, STEPS * T) + tail, dtype=torch.int32, device="cuda") for _ in range(2)]
            outs = (*rows(), *rows(), *rows(), *rows(spec.max_bubbles))
            counter = torch.zeros(1, dtype=torch.int32, device="cuda")
            ws = ops.bubble_census_workspace(2 * B * T, H, W, spec.max_bubbles, "cuda")
            call = lambda: ops.rollout_bubbles(pred, store.frames, first, counter, store.out_tab, 0, STEPS, 4, spec.max_bubbles, ws, *outs)
            out[f"B{B}_census_call_us"] = med([device_time(call) * 1e6 for _ in range(5)], 2)
            out[f"B{B}_bubbles_per_frame"] = [int(outs[0][:, :T].min()), int(outs[0][:, :T].max()), int(outs[1][:, :T].min()), int(outs[1][:, :T].max())]
    for name, (B, _) in variants.items():
        out[name] = {"ms_per_step": med([(a - b) / (STEPS - SHORT) / (NTRAJ // B) * 1e3 for a, b in times[name]])}
    if has:
        for B in (1, 8):
            on, off = out[f"B{B}_on"]["ms_per_step"], out[f"B{B}_off"]["ms_per_step"]
            out[f"B{B}_marginal_ms_per_step"] = round(on["median"] - off["median"], 4)
            out[f"B{B}_off_spread_ms"] = round(off["min_max"][1] - off["min_max"][0], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=("census", "rollout"), default=None)
    ap.add_argument("--tree", default=None, help="checkout of this repository to import bubbleformer_amd from")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bubble_census_bench needs a GPU", file=sys.stderr)
        return 1
    tree = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, tree)
    out = {"tree": tree, "rounds": a.rounds}
    if a.only in (None, "rollout"):
        out["rollout"] = bench_rollout(a.rounds)
    if a.only in (None, "census"):
        import bubbleformer_amd.ops as ops
        if hasattr(ops, "bubble_census"):
            out["census"] = bench_census(a.rounds)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
