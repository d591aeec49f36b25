#!/usr/bin/env python3
"""Bubble matching in rollout evaluation, timed on one GPU: prints one JSON object.

Steps per second of `evaluate_rollouts` at 8 trajectories per forward (FiLMAViT-small bf16, 16 x 192 x 192 x 4 clips, graph) three ways:
`BubbleSpec()` (the census alone), `BubbleSpec(track=True)` and `BubbleSpec(track=True, match=True)`.  One process; the variants alternate
inside every round and the order flips every round; round 0 (code objects, first captures) is dropped.  A round clocks three calls of 50
steps and three of 10 steps of every variant, alternated, each call on its own between device synchronisations.  Seconds per step is
(t(50) - t(10)) / 40, as tools/rollout_eval_bench.py defines it, which leaves the set-up of a call (allocation, warm-up, capture) out; a call
now and then takes half a second longer on the host, so the difference is taken between the MEDIANS of the two sets of call times, not per
pair of calls.  Reported per variant: median and range of the call times, steps per second and milliseconds per step from the medians, the
same from the two minima; and the marginal milliseconds per step of tracking and of matching.

Usage: python tools/bubble_match_bench.py [--rounds R]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS, SHORT, T, NTRAJ, REPEATS = 50, 10, 16, 8, 3


def bench(rounds):
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
    specs = {"census": BubbleSpec(dx=16 / 192), "track": BubbleSpec(dx=16 / 192, track=True), "track_match": BubbleSpec(dx=16 / 192, track=True, match=True)}
    run = lambda spec, steps: Ro.evaluate_rollouts(model, store, starts, steps, use_graph=True, bubbles=spec)
    times = {k: {STEPS: [], SHORT: []} for k in specs}
    for r in range(rounds + 1):
        for name in (list(specs)[::-1] if r % 2 else list(specs)):
            for steps in (STEPS, SHORT) * REPEATS:
                s = clock(lambda: run(specs[name], steps))
                if r:
                    times[name][steps].append(s)
    out = {}
    for k, v in times.items():
        long, short = med(v[STEPS]), med(v[SHORT])
        ms = (long["median"] - short["median"]) / (STEPS - SHORT) * 1e3
        floor = (long["min_max"][0] - short["min_max"][0]) / (STEPS - SHORT) * 1e3
        out[k] = {"steps_per_s": round(1e3 / ms, 1), "ms_per_step": round(ms, 4), "ms_per_step_from_minima": round(floor, 4), f"call_s_{STEPS}": long,
                  f"call_s_{SHORT}": short, "calls_timed": len(v[STEPS])}
    out["track_marginal_ms_per_step"] = round(out["track"]["ms_per_step"] - out["census"]["ms_per_step"], 4)
    out["match_marginal_ms_per_step"] = round(out["track_match"]["ms_per_step"] - out["track"]["ms_per_step"], 4)
    report = run(specs["track_match"], 2)                              # what the matched rollout of the study's noise fields holds
    out["counts_sum"] = report.bubble_match_counts.clamp(min=0).sum(dim=(0, 1)).tolist()
    out["trajectories_per_forward"], out["max_bubbles"] = NTRAJ, specs["census"].max_bubbles
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bubble_match_bench needs a GPU", file=sys.stderr)
        return 1
    print(json.dumps({"rounds": a.rounds, "device": torch.cuda.get_device_name(0), "rollout": bench(a.rounds)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
