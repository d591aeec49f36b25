#!/usr/bin/env python3
"""`bf_redistance` alone, timed on one GPU: prints one JSON object.

128 frames of two distorted discs (the signed distance to two discs times 1 + 0.8 sin(7 d): the right zero level set, the wrong slopes) at
192 x 192 (the distances live in LDS) and at 384 x 192 (in the workspace), with and without band = 8 dx.  One launch, a workgroup per frame,
outputs and workspace allocated once; the launch is captured in a HIP graph and the time is the median over repeated replays, each between two
device events, after untimed replays.  The pass counts of the frames stand beside it, and the time per pass and cell.

Usage: python tools/redistance_bench.py [--replays N] [--frames F]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

DX = 1.0 / 32


def frames_of(F, H, W):
    """F different two-disc frames: the discs wander with the frame number."""
    y, x = np.mgrid[0:H, 0:W]
    yc, xc = (y + 0.5) * DX, (x + 0.5) * DX
    out = np.empty((F, H, W), np.float32)
    for f in range(F):
        r = 0.17 * min(H, W) * DX
        discs = [((0.27 + 0.001 * f) * W * DX, 0.3 * H * DX, r), (0.7 * W * DX, (0.68 - 0.001 * f) * H * DX, 0.8 * r)]
        d = np.maximum.reduce([rr - np.sqrt((xc - cx) ** 2 + (yc - cy) ** 2) for cx, cy, rr in discs])
        out[f] = d * (1.0 + 0.8 * np.sin(7.0 * d))
    return out


def replay_time(call, replays):
    """Median, minimum and maximum seconds of one replay of the captured call."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(3):
        graph.replay()
    times = []
    for _ in range(replays):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        graph.replay()
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=30)
    ap.add_argument("--frames", type=int, default=128)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("redistance_bench needs a GPU", file=sys.stderr)
        return 1
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bubbleformer_amd import ops
    out = {"frames": a.frames, "replays": a.replays, "lds_cells": ops.redistance_lds_cells()}
    for H, W in ((192, 192), (384, 192)):
        phi = torch.from_numpy(frames_of(a.frames, H, W)).cuda()
        res, rounds, change = torch.empty_like(phi), torch.empty(a.frames, dtype=torch.int32, device="cuda"), torch.empty(a.frames, device="cuda")
        ws = ops.redistance_workspace(a.frames, H, W, "cuda")
        for band in (None, 8 * DX):
            med, lo, hi = replay_time(lambda: ops.redistance(phi, DX, band, None, ws, res, rounds, change), a.replays)
            passes = rounds.float()
            out[f"{H}x{W}_{'band8' if band else 'full'}"] = {
                "path": "lds" if H * W <= out["lds_cells"] else "workspace", "us": round(med * 1e6, 1), "us_min_max": [round(lo * 1e6, 1), round(hi * 1e6, 1)],
                "passes_min_mean_max": [int(passes.min()), round(float(passes.mean()), 1), int(passes.max())],
                "ns_per_pass_and_kilocell": round(med * 1e9 / float(passes.max()) / (H * W / 1000.0), 2)}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
