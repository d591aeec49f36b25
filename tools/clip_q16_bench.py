#!/usr/bin/env python3
"""The clip gather from an fp32 and from a 16-bit (q16) device store, timed on one GPU in one process: prints one JSON object.

The bench shape: B 8, T 16, C 4 in and out, 192 x 192 clips (151 MB written per call).  Two cases, each in both storage forms:
  plain      the plain gather from a 192 x 192 store (fp32: bf_clip_gather_batch; q16: bf_clip_gather_q16)
  crop_flip  a 192 x 192 window out of a 512 x 512 store, origins drawn per sample, with flip_p = 0.5 (fp32: bf_clip_gather_augment)
Both stores of a case hold the same synthetic trajectories; the q16 gather's clips are checked to be bit for bit the fp32 gather's of the
decoded frames before anything is timed.  Indices are a device tensor.  Each case's call is captured `--calls` times into one HIP graph,
replayed untimed, and then the four graphs are replayed in turn, `--rounds` rounds, each replay between two device events: median
[min, max] microseconds per call, the q16 / fp32 ratio of the medians of the same run, and the rate of the bytes a call must move (its
clips read once in the store's form and written once in fp32).  Also: the encode throughput (bf_clip_encode_q16 alone on a resident fp32
chunk, fp32 bytes read per second), the time of a whole q16 fill from host memory, and both stores' resident bytes.

Usage: python tools/clip_q16_bench.py [--rounds N] [--calls K] [--frames F]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

B, T, FIELDS, OUT = 8, 16, ["dfun", "temperature", "velx", "vely"], 192


def dataset_of(side, frames):
    from bubbleformer_amd.data import BubbleForecast
    g = np.random.default_rng(side)
    traj = {n: g.standard_normal((frames, side, side), dtype=np.float32) + np.float32(k) for k, n in enumerate(FIELDS)}
    ds = BubbleForecast.from_arrays([traj], norm="std", time_window=T, start_time=0)
    ds.normalize()
    return ds


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


def timed(fn, repeats):
    """Median microseconds of fn() between two device events."""
    out = []
    for _ in range(repeats):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        out.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--frames", type=int, default=72)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("clip_q16_bench needs a GPU", file=sys.stderr)
        return 1
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bubbleformer_amd import ops
    from bubbleformer_amd.utils import AugmentSpec
    draw = 1
    spec = AugmentSpec(flip_p=0.5, crop=(OUT, OUT), crop_y="random", seed=3)
    out = {"shape": [B, T, len(FIELDS), OUT, OUT], "rounds": a.rounds, "calls_per_replay": a.calls, "draw": draw}
    graphs, alive = {}, []            # a captured graph holds addresses, not references: the stores and indices it reads live as long as it does
    for case, side, aug in (("plain", OUT, None), ("crop_flip", 512, spec)):
        ds = dataset_of(side, a.frames)
        t0 = time.perf_counter()
        q16 = ds.device_store("cuda", storage="q16")
        torch.cuda.synchronize()
        fill = time.perf_counter() - t0
        fp32 = ds.device_store("cuda")
        idx = torch.tensor(np.arange(B) * ((len(ds) - 1) // (B - 1)), dtype=torch.int64, device="cuda")
        got, want = q16.gather(idx, augment=aug, draw=draw), q16.to_fp32().gather(idx, augment=aug, draw=draw)
        assert all(torch.equal(x, y) for x, y in zip(got, want)) and tuple(got[0].shape) == (B, T, len(FIELDS), OUT, OUT)
        out[case] = {"store_side": side, "frames": a.frames, "resident_bytes": {"fp32": fp32.nbytes, "q16": q16.nbytes},
                     "q16_fill_s": round(fill, 3), "q16_staging_frames": q16.staging_frames}
        alive.append((ds, fp32, q16, idx))
        for form, store in (("fp32", fp32), ("q16", q16)):
            graphs[(case, form)] = captured((lambda s=store, sp=aug, i=idx: s.gather(i, augment=sp, draw=draw)), a.calls)
        if case == "crop_flip":                                      # encode alone: one field of the 512 x 512 fp32 store into a code buffer, both resident
            src = fp32.frames[0]
            dst = torch.empty(src.shape, dtype=torch.int16, device="cuda")
            ops.clip_encode_q16(src, dst, -6.0, 65535.0 / 12.0)
            us = timed(lambda: ops.clip_encode_q16(src, dst, -6.0, 65535.0 / 12.0), 20)
            out["encode"] = {"values": src.numel(), "us": round(us, 2), "fp32_GB_per_s": round(src.numel() * 4 / us * 1e-3, 1)}
            del src, dst
    for graph, _ in graphs.values():
        for _ in range(3):
            graph.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, (graph, _) in graphs.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            graph.replay()
            ev[1].record()
            torch.cuda.synchronize()
            times[k].append(ev[0].elapsed_time(ev[1]) * 1e3 / a.calls)
    values = 2 * B * T * len(FIELDS) * OUT * OUT                     # two clips
    for (case, form), t in times.items():
        med = statistics.median(t)
        moved = values * (4 + (4 if form == "fp32" else 2))
        out[case][form] = {"us": round(med, 2), "us_min_max": [round(min(t), 2), round(max(t), 2)], "bytes_moved": moved,
                           "TB_per_s": round(moved / med * 1e-6, 3)}
    for case in ("plain", "crop_flip"):
        out[case]["q16_over_fp32"] = round(out[case]["q16"]["us"] / out[case]["fp32"]["us"], 3)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
