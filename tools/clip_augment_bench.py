#!/usr/bin/env python3
"""`DeviceClipStore.gather` with and without augmentation, timed on one GPU in one process: prints one JSON object.

The bench shape: B 8, T 16, C 4 in and out, 192 x 192 clips (151 MB written per call).  Four cases:
  plain      the plain gather from a 192 x 192 store (bf_clip_gather_batch)
  flip       AugmentSpec(flip_p=0.5) on the same store (bf_clip_gather_augment, no window)
  crop       a 192 x 192 window out of a 512 x 512 store, origins drawn per sample (crop_y="random")
  crop_flip  the window together with flip_p = 0.5
Indices are a device tensor (no host work per call beyond the launch).  Each case's call is captured `--calls` times into one HIP graph
(outputs from the graph's pool), replayed untimed, and then the cases are replayed in turn, `--rounds` rounds, each replay between two
device events: median [min, max] microseconds per call, the ratio of the medians to the plain gather's of the same run, and the rate of the
bytes a call must move (its clips read once and written once).  With the draw a captured graph holds, the plan says how many of the
8 samples are mirrored and how many origins are multiples of 4 (those rows are read 16 bytes at a time).

Usage: python tools/clip_augment_bench.py [--rounds N] [--calls K]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

B, T, FIELDS, OUT = 8, 16, ["dfun", "temperature", "velx", "vely"], 192


def store_of(side, frames, device):
    from bubbleformer_amd.data import BubbleForecast
    g = np.random.default_rng(side)
    traj = {n: g.standard_normal((frames, side, side), dtype=np.float32) + np.float32(k) for k, n in enumerate(FIELDS)}
    ds = BubbleForecast.from_arrays([traj], norm="std", time_window=T, start_time=0)
    store = ds.device_store(device)
    store.normalize()
    return ds, store


def captured(call, calls):
    """A HIP graph of `calls` back-to-back calls (warmed on a side stream first, as capture requires)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = [call() for _ in range(calls)]
    return graph, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--frames", type=int, default=72)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("clip_augment_bench needs a GPU", file=sys.stderr)
        return 1
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bubbleformer_amd.utils import AugmentSpec, augment_plan
    small_ds, small = store_of(OUT, a.frames, "cuda")
    big_ds, big = store_of(512, a.frames, "cuda")
    ids = np.arange(B) * ((len(small_ds) - 1) // (B - 1))
    idx = torch.tensor(ids, dtype=torch.int64, device="cuda")
    draw = 1
    cases = {"plain": (small, None, OUT), "flip": (small, AugmentSpec(flip_p=0.5, seed=3), OUT),
             "crop": (big, AugmentSpec(crop=(OUT, OUT), crop_y="random", seed=3), 512),
             "crop_flip": (big, AugmentSpec(flip_p=0.5, crop=(OUT, OUT), crop_y="random", seed=3), 512)}
    graphs, plans = {}, {}
    for name, (store, spec, side) in cases.items():
        graphs[name] = captured((lambda s=store, sp=spec: s.gather(idx, augment=sp, draw=draw)), a.calls)
        got = graphs[name][1][-1]
        assert tuple(got[0].shape) == tuple(got[1].shape) == (B, T, len(FIELDS), OUT, OUT)
        if spec is not None:
            flip, x0, y0 = augment_plan(spec, ids, draw, side, side)
            plans[name] = {"mirrored": int(flip.sum()), "x0_multiple_of_4": int((x0 % 4 == 0).sum()), "x0": x0.tolist(), "y0": y0.tolist()}
    for graph, _ in graphs.values():
        for _ in range(3):
            graph.replay()
    torch.cuda.synchronize()
    times = {name: [] for name in cases}
    for _ in range(a.rounds):
        for name, (graph, _) in graphs.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            graph.replay()
            ev[1].record()
            torch.cuda.synchronize()
            times[name].append(ev[0].elapsed_time(ev[1]) * 1e3 / a.calls)
    moved = 2.0 * 2 * B * T * len(FIELDS) * OUT * OUT * 4          # two clips, each read once and written once
    out = {"shape": [B, T, len(FIELDS), OUT, OUT], "rounds": a.rounds, "calls_per_replay": a.calls, "bytes_moved": int(moved), "draw": draw}
    base = statistics.median(times["plain"])
    for name, t in times.items():
        med = statistics.median(t)
        out[name] = {"us": round(med, 2), "us_min_max": [round(min(t), 2), round(max(t), 2)], "ratio_to_plain": round(med / base, 3),
                     "TB_per_s": round(moved / med * 1e-6, 3), **({"plan": plans[name]} if name in plans else {})}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
