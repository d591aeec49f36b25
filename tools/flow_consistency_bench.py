#!/usr/bin/env python3
"""The flow-consistency rows (bf_flow_consistency / bf_rollout_flow, csrc/flow.hip), timed on one GPU: prints one JSON object.

  call:     the stand-alone call at (8, 16, 192, 192) -- 128 frames, 120 pairs, one workgroup per frame -- on smooth fields with an interface
            through every frame (tests/flow_restatement.fields), by device events over back-to-back launches, median of the rounds, and the bytes
            of the three input fields (each counted once) over that time.  `frame_rows_only` leaves the three pair rows out.
  rollout:  trajectory-steps per second of `evaluate_rollouts_flow` at 8 trajectories per forward with `flow=FlowSpec(dt)`, with `flow=None` and
            with `bubbles=BubbleSpec()` -- the census is a per-frame-workgroup kernel of comparable shape -- FiLMAViT-small bf16, graph, the
            variants alternated inside every round, the order flipped every round; ms per step is (median t(50 steps) - median t(10 steps)) / 40.
            `step_call` under `call` is `ops.rollout_flow` alone on that leg's store, by device events.

Usage: python tools/flow_consistency_bench.py [--rounds R] [--only call|rollout]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEPS, SHORT, T, H, W, NTRAJ = 50, 10, 16, 192, 192, 8
DX, DT = 1.0 / 32, 0.25


def bench_call(rounds):
    from bubbleformer_amd import ops
    from tests import flow_restatement as R
    from tools.bubble_census_bench import device_time, med
    phi, u, v = (torch.from_numpy(a).cuda() for a in R.fields(NTRAJ, T, H, W, np.random.default_rng(5), DX))
    rows = {k: torch.zeros((NTRAJ, T if k in ops._FLOW_FRAME_ROWS else T - 1), dtype=torch.int32 if k.endswith("_cells") else torch.float32, device="cuda")
            for k in ops._FLOW_ROWS}
    nbytes = 3 * 4 * NTRAJ * T * H * W
    out = {"frames": NTRAJ * T, "input_bytes": nbytes}
    for name, keys in (("all_rows", ops._FLOW_ROWS), ("frame_rows_only", ops._FLOW_FRAME_ROWS)):
        call = lambda: ops.flow_consistency(phi, u, v, DX, DT, 3 * DX, 1, **{k: rows[k] for k in keys})
        ms = [device_time(call) * 1e3 for _ in range(rounds)]
        out[f"{name}_ms"] = med(ms)
        out[f"{name}_bytes_per_s"] = float(f"{nbytes / (out[f'{name}_ms']['median'] * 1e-3):.4e}")
    out["bulk_cells_per_frame"] = float(rows["bulk_cells"].float().mean())
    out["band_cells_per_pair"] = float(rows["transport_cells"].float().mean())
    out["step_call"] = bench_step_call(rounds)
    return out


def bench_step_call(rounds):
    """`ops.rollout_flow` alone on the rollout leg's white-noise store: 2 sides x 8 trajectories x 16 frames = 256 workgroups, the counter at step 1
    so that the pairs across the step boundary (carry, stored frame) are taken too."""
    from bubbleformer_amd import ops
    from bubbleformer_amd.utils.rollout import plan_rollouts
    from tools.bubble_census_bench import device_time, med
    from tools.rollout_eval_bench import study
    store = study()
    starts = [i * len(store.ds) // NTRAJ for i in range(NTRAJ)]
    first = torch.tensor(plan_rollouts(store.ds, starts, STEPS).first, dtype=torch.int64, device="cuda")
    pred = (store.gather([s + T for s in starts])[1] + 0.01 * torch.randn((NTRAJ, T, 4, H, W), device="cuda")).contiguous()
    sides = [{k: torch.zeros((NTRAJ, STEPS * T if k in ops._FLOW_FRAME_ROWS else STEPS * T - 1), dtype=torch.int32 if k.endswith("_cells") else torch.float32,
                             device="cuda") for k in ops._FLOW_ROWS} for _ in range(2)]
    carry = torch.zeros((2, NTRAJ, 3, H, W), device="cuda")
    counter = torch.ones(1, dtype=torch.int32, device="cuda")
    call = lambda: ops.rollout_flow(pred, store.frames, first, counter, store.out_tab, (0, 2, 3), STEPS, DX, DT, 3 * DX, 1, carry, sides[0], sides[1])
    return {"workgroups": 2 * NTRAJ * T, "ms": med([device_time(call) * 1e3 for _ in range(rounds)]),
            "bulk_cells_per_frame": float(sides[1]["bulk_cells"][:, T:2 * T].float().mean()),
            "band_cells_per_pair": float(sides[1]["transport_cells"][:, T - 1:2 * T - 1].float().mean())}


def bench_rollout(rounds):
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils import BubbleSpec, FlowSpec
    from bubbleformer_amd.utils import rollout as Ro
    from oracle import weights as Wt
    from tools.bubble_census_bench import med
    from tools.rollout_eval_bench import CFG, clock, study
    model = get_model("filmavit", time_window=T, drop_path=0.0, compute_dtype=torch.bfloat16, **CFG)
    model.load_state_dict(Wt.generate(Wt.param_shapes(**CFG), seed=42))
    model = model.cuda().eval()
    store = study()
    starts = [i * len(store.ds) // NTRAJ for i in range(NTRAJ)]
    variants = {"off": (None, {}), "flow": (FlowSpec(DT), {}), "census": (None, {"bubbles": BubbleSpec()})}
    times = {k: [] for k in variants}
    for r in range(rounds + 1):                                         # round 0 is dropped; the order of the variants flips every round
        for name, (flow, kw) in (list(variants.items())[::-1] if r % 2 else list(variants.items())):
            run = lambda steps: Ro.evaluate_rollouts_flow(model, store, starts, steps, flow, use_graph=True, **kw)
            pair = (clock(lambda: run(STEPS)), clock(lambda: run(SHORT)))
            if r:
                times[name].append(pair)
    # the host now and then holds a call up by seconds, so ms per step is a difference of medians (and of minima), not a median of differences
    out = {}
    for name in variants:
        long, short = med([a for a, _ in times[name]]), med([b for _, b in times[name]])
        ms = (long["median"] - short["median"]) / (STEPS - SHORT) * 1e3
        out[name] = {"t_long_s": long, "t_short_s": short, "ms_per_step": round(ms, 4), "traj_steps_per_s": round(NTRAJ / ms * 1e3, 1),
                     "ms_per_step_from_minima": round((long["min_max"][0] - short["min_max"][0]) / (STEPS - SHORT) * 1e3, 4)}
    for name in ("flow", "census"):
        out[f"{name}_marginal_ms_per_step"] = round(out[name]["ms_per_step"] - out["off"]["ms_per_step"], 4)
        out[f"{name}_marginal_ms_per_step_from_minima"] = round(out[name]["ms_per_step_from_minima"] - out["off"]["ms_per_step_from_minima"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=("call", "rollout"), default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("flow_consistency_bench needs a GPU", file=sys.stderr)
        return 1
    out = {"rounds": a.rounds, "geometry": [NTRAJ, T, H, W]}
    if a.only in (None, "call"):
        out["call"] = bench_call(a.rounds)
    if a.only in (None, "rollout"):
        out["rollout"] = bench_rollout(a.rounds)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
