#!/usr/bin/env python3
"""Bubble tracking, timed on one GPU: prints one JSON object.

  links:    `bf_bubble_links` alone (ops.bubble_links, outputs and workspace allocated once) by device events over back-to-back launches, and in
            the same run the `bf_bubble_census` launch (with label images) of the same frames and the `bf_bubble_track_ids` launch: 256 pairs of
            192 x 192 and 16 pairs of 512 x 512 (every pair a sequence of two frames, the later one the earlier shifted by three cells), on smooth
            random fields with a dozen bubbles per frame (tables in LDS), on white noise (thousands of components, 256 kept: 256 x 256 tables in
            the workspace) and on a full frame (one bubble).
  rollout:  the marginal cost per step of `evaluate_rollouts(bubbles=BubbleSpec(track=True))` against `BubbleSpec()` and against no census:
            FiLMAViT-small bf16, 16 x 192 x 192 x 4 clips, B = 1 and 8 trajectories per forward, graph; the variants alternated inside every
            round, the order flipped every round; ms per step is (t(50 steps) - t(10 steps)) / 40 as tools/rollout_eval_bench.py defines it.

Usage: python tools/bubble_track_bench.py [--rounds R] [--only links|rollout] [--tree CHECKOUT]
(--tree imports bubbleformer_amd from another checkout of this repository: a tree without tracking runs the variants it has, which is how
`off` and `census` are timed against the parent commit -- one process per tree, the processes alternated by the caller)."""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np
import torch

STEPS, SHORT, T, H, W, NTRAJ = 50, 10, 16, 192, 192, 8


def bench_links(rounds):
    from bubbleformer_amd import ops
    from tools.bubble_census_bench import device_time, fields, med
    out = {"lds_entries": ops.bubble_links_lds_entries()}
    mb = 256
    for pairs, h, w in ((256, H, W), (16, 512, 512)):
        for kind in ("smooth", "noise", "full"):
            earlier = fields(kind, pairs, h, w)
            later = np.roll(earlier, (3, 3), axis=(1, 2)) if kind != "noise" else fields(kind, 2 * pairs, h, w)[pairs:]
            phi = torch.from_numpy(np.stack([earlier, later], axis=1)).cuda()          # (pairs, 2, h, w)
            new = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
            count, cells, attached, area, labels = new(pairs, 2), new(pairs, 2), new(pairs, 2), new(pairs, 2, mb), new(pairs, 2, h, w)
            census_ws = ops.bubble_census_workspace(2 * pairs, h, w, mb, "cuda")
            census = lambda: ops.bubble_census(phi.view(2 * pairs, h, w), 4, mb, census_ws, count.view(-1), cells.view(-1), attached.view(-1),
                                               area.view(2 * pairs, mb), None, None, labels.view(2 * pairs, h, w))
            rows = {k: new(*shape) for k, shape in ops._link_rows((pairs, 1), mb).items()}
            ws = ops.bubble_links_workspace(pairs, mb, "cuda")
            links = lambda: ops.bubble_links(labels, count, attached, area, ws, **rows)
            track_id, n_tracks = new(pairs, 2, mb), new(pairs)
            ids = lambda: ops.bubble_track_ids(count, rows["successor"], rows["predecessor"], track_id, n_tracks)
            row = {"census_us": med([device_time(census) * 1e6 for _ in range(rounds)], 1)}
            row["links_us"] = med([device_time(links) * 1e6 for _ in range(rounds)], 1)
            row["track_ids_us"] = med([device_time(ids) * 1e6 for _ in range(rounds)], 1)
            row["links_over_census"] = round(row["links_us"]["median"] / row["census_us"]["median"], 3)
            kept = count.clamp(max=mb)
            row["table_entries"] = [int((kept[:, 0] * kept[:, 1]).min()), int((kept[:, 0] * kept[:, 1]).max())]
            row["events"] = rows["events"].sum(dim=(0, 1)).tolist()
            row["workspace_bytes"] = ws.numel()
            out[f"{pairs}x{h}x{w}_{kind}"] = row
    return out


def bench_rollout(rounds):
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils import BubbleSpec
    from bubbleformer_amd.utils import rollout as Ro
    from oracle import weights as Wt
    from tools.bubble_census_bench import med
    from tools.rollout_eval_bench import CFG, clock, study
    model = get_model("filmavit", time_window=T, drop_path=0.0, compute_dtype=torch.bfloat16, **CFG)
    model.load_state_dict(Wt.generate(Wt.param_shapes(**CFG), seed=42))
    model = model.cuda().eval()
    store = study()
    starts = [i * len(store.ds) // NTRAJ for i in range(NTRAJ)]
    has = "track" in [f.name for f in dataclasses.fields(BubbleSpec)]
    kinds = (("off", {}), ("census", {"bubbles": BubbleSpec(dx=16 / 192)})) + ((("track", {"bubbles": BubbleSpec(dx=16 / 192, track=True)}),) if has else ())
    variants = {}
    for B in (1, 8):
        for name, kw in kinds:
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
    out = {"has_tracking": has}
    for name, (B, _) in variants.items():
        out[name] = {"ms_per_step": med([(a - b) / (STEPS - SHORT) / (NTRAJ // B) * 1e3 for a, b in times[name]])}
    for B in (1, 8):
        off = out[f"B{B}_off"]["ms_per_step"]
        out[f"B{B}_off_spread_ms"] = round(off["min_max"][1] - off["min_max"][0], 4)
        out[f"B{B}_census_marginal_ms_per_step"] = round(out[f"B{B}_census"]["ms_per_step"]["median"] - off["median"], 4)
        if has:
            out[f"B{B}_track_marginal_ms_per_step"] = round(out[f"B{B}_track"]["ms_per_step"]["median"] - out[f"B{B}_census"]["ms_per_step"]["median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=("links", "rollout"), default=None)
    ap.add_argument("--tree", default=None, help="checkout of this repository to import bubbleformer_amd from")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bubble_track_bench needs a GPU", file=sys.stderr)
        return 1
    tree = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, tree)
    out = {"tree": tree, "rounds": a.rounds}
    if a.only in (None, "rollout"):
        out["rollout"] = bench_rollout(a.rounds)
    if a.only in (None, "links"):
        import bubbleformer_amd.ops as ops
        if hasattr(ops, "bubble_links"):
            out["links"] = bench_links(a.rounds)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
