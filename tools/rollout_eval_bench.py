#!/usr/bin/env python3
"""Rollout evaluation, timed on one GPU: prints one JSON object.

FiLMAViT-small (E 384, 6 heads, 12 blocks, patch 16), bf16, 16 x 192 x 192 x 4 clips, a synthetic in-memory study of 8 trajectories of
16 * 52 frames, 50 autoregressive steps per trajectory.  Variants, alternated inside every round of one process run:

  today:    utils.rollout.autoregressive_rollout(use_graph=True, target_fn=lambda s: store.gather([i + s * T])[1][0]), one trajectory
            after the other (8 calls);
  batched:  utils.rollout.evaluate_rollouts at B = 1, 2, 4, 8 trajectories per forward (8 / B calls), graph and eager.

Every variant rolls the same 8 trajectories out, so the clock (host, device-synchronised) covers 8 * 50 trajectory-steps including each
call's own warm-up forwards and graph capture; `ms_per_step` is the MARGINAL cost of a step, (t(50 steps) - t(10 steps)) / 40, which leaves
those fixed costs out, and `traj_steps_per_s` is its inverse times the trajectories a step carries.  Medians over the rounds, with the
spread.  `scoring` times the scoring call alone with device events: bytes (prediction once + target frames once + copies) over time as a
share of 8 TB/s.

Usage: python tools/rollout_eval_bench.py [--rounds R] [--only today|batched|scoring] [--batches 1,2,4,8] [--graph-only] [--tree CHECKOUT] [--redistance]
(--tree imports bubbleformer_amd from another checkout of this repository, to time `today` on another commit in the same run).
--ensemble 4,16 runs the ensemble measurement instead: per member count M, the step on M * 2 rows with and without EnsembleSpec(M), and the
bf_rollout_ensemble call alone beside bf_rollout_score on the same prediction (device events, bytes over time).
--redistance runs the redistancing measurement instead: the batched graph variant at 8 trajectories per forward with and without
RedistanceSpec(), alternated inside every round, and the passes the correction took (the synthetic study's dfun is noise, nearly all
interface cells: few passes; tools/redistance_bench.py times the kernel on bubble-like frames)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

CFG = dict(input_fields=4, output_fields=4, patch_size=16, embed_dim=384, num_heads=6, processor_blocks=12, num_fluid_params=9)
FIELDS = ("dfun", "temperature", "velx", "vely")
FIELD_STATS = ((-2.37, 1.98), (0.0145, 0.081), (-0.07, 0.49), (0.055, 0.77))       # mean / std of the sample trajectories' fields
T, H, W, NTRAJ, FRAMES, STEPS, SHORT = 16, 192, 192, 8, 16 * 52, 50, 10
HBM_BYTES_PER_S = 8e12


def study():
    from bubbleformer_amd.data import BubbleForecast
    rs = np.random.RandomState(3)
    base = [rs.standard_normal((FRAMES, H, W)).astype(np.float32) for _ in FIELDS]
    trajs = [{n: base[k] * np.float32(sd * (1 + 0.02 * i)) + np.float32(mu) for k, (n, (mu, sd)) in enumerate(zip(FIELDS, FIELD_STATS))}
             for i in range(NTRAJ)]
    fluid = [{"inv_reynolds": 0.0042 * (1 + 0.1 * i), "cpgas": 0.83, "mugas": 0.023, "rhogas": 0.0083, "thcogas": 0.25, "stefan": 0.5298,
              "prandtl": 8.4, "heater": {"nucWaitTime": 0.4, "wallTemp": 1.0 + 0.05 * i}} for i in range(NTRAJ)]
    ds = BubbleForecast.from_arrays(trajs, fluid, norm="std", time_window=T, start_time=0)
    store = ds.device_store("cuda")
    store.normalize()
    return store


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def summary(per_round, trajs_per_step):
    """per_round: [(seconds at STEPS, seconds at SHORT)] for the whole set of NTRAJ trajectories."""
    calls = NTRAJ // trajs_per_step
    ms = [(a - b) / (STEPS - SHORT) / calls * 1e3 for a, b in per_round]
    rate = [trajs_per_step / m * 1e3 for m in ms]
    return {"ms_per_step": round(statistics.median(ms), 4), "ms_per_step_min_max": [round(min(ms), 4), round(max(ms), 4)],
            "traj_steps_per_s": round(statistics.median(rate), 1), "traj_steps_per_s_min_max": [round(min(rate), 1), round(max(rate), 1)],
            "whole_call_s_8x50": round(statistics.median(a for a, _ in per_round), 4)}


def scoring(store, B, reps=20):
    from bubbleformer_amd import ops
    from bubbleformer_amd.utils.rollout import plan_rollouts
    starts = [i * len(store.ds) // NTRAJ for i in range(B)]
    first = torch.tensor(plan_rollouts(store.ds, starts, STEPS).first, dtype=torch.int64, device="cuda")
    pred = store.gather(starts)[1] + 0.01
    new = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    rel, crit, ep, et, nxt = new(B, STEPS * T, 4), new(B, STEPS), new(B, STEPS * T), new(B, STEPS * T), torch.empty_like(pred)
    ws = ops.rollout_score_workspace(pred)
    out = {}
    for name, arch in (("with_next_input", None), ("with_next_input_and_archive", new(B, STEPS * T, 4, H, W))):
        times = []
        for _ in range(3):
            counter = torch.zeros(1, dtype=torch.int32, device="cuda")
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ops.rollout_score(pred, store.frames, first, counter, store.out_tab, 0, STEPS, rel, crit, ws, ep, et, nxt, arch)      # untimed first call
            ev[0].record()
            for _ in range(reps):
                ops.rollout_score(pred, store.frames, first, counter, store.out_tab, 0, STEPS, rel, crit, ws, ep, et, nxt, arch)
            ev[1].record()
            torch.cuda.synchronize()
            times.append(ev[0].elapsed_time(ev[1]) / reps * 1e-3)
        nbytes = pred.numel() * 4 * (3 + (arch is not None))        # prediction read, target frames read, next input written [, archive row written]
        t = statistics.median(times)
        out[name] = {"us": round(t * 1e6, 1), "bytes": nbytes, "TB_per_s": round(nbytes / t / 1e12, 3), "share_of_8TBps": round(nbytes / t / HBM_BYTES_PER_S, 3)}
    return out


def device_time(call, reps=20):
    """Median seconds of `call` over three runs of `reps` back-to-back calls between two device events, after one untimed call."""
    times = []
    for _ in range(3):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        call()
        ev[0].record()
        for _ in range(reps):
            call()
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]) / reps * 1e-3)
    return statistics.median(times)


def ensemble(model, store, M, rounds, Bt=2):
    """The step at M * Bt rows with and without EnsembleSpec(M) (marginal ms per step, as `summary`), and the bf_rollout_ensemble call alone
    beside bf_rollout_score on the same prediction, both with device events: bytes read ((M + 1) * Bt * T * C * H * W * 4: every member once, the
    truth once; the rows written are noise beside them) over time."""
    from bubbleformer_amd import ops
    from bubbleformer_amd.utils import EnsembleSpec
    from bubbleformer_amd.utils import rollout as R
    starts = [i * len(store.ds) // NTRAJ for i in range(Bt)]
    spec = EnsembleSpec(M, 0.05, seed=1)
    variants = {"plain": lambda steps: R.evaluate_rollouts(model, store, starts * M, steps),
                "ensemble": lambda steps: R.evaluate_rollouts(model, store, starts, steps, ensemble=spec)}
    times = {k: [] for k in variants}
    for r in range(rounds + 1):                                         # round 0 is the warm-up and is dropped
        for name, fn in variants.items():
            pair = (clock(lambda: fn(STEPS)), clock(lambda: fn(SHORT)))
            if r:
                times[name].append(pair)
    out = {}
    for name in variants:
        ms = [(a - b) / (STEPS - SHORT) * 1e3 for a, b in times[name]]
        out[name + "_ms_per_step"] = round(statistics.median(ms), 4)
        out[name + "_ms_per_step_min_max"] = [round(min(ms), 4), round(max(ms), 4)]
    B = M * Bt
    first = torch.tensor(plan_rollouts_first(store, starts * M), dtype=torch.int64, device="cuda")
    pred = store.gather(starts * M)[1] + 0.01 * torch.randn(B, T, 4, H, W, device="cuda")
    new = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    rows = {"mean_rmse": new(Bt, STEPS * T, 4), "spread": new(Bt, STEPS * T, 4), "crps": new(Bt, STEPS * T, 4),
            "rank_hist": torch.empty((Bt, STEPS * T, 4, M + 1), dtype=torch.int32, device="cuda")}
    ws = ops.ensemble_workspace(Bt * T * 4, M, H, W, "cuda")
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")            # never advanced: the call only reads it
    t = device_time(lambda: ops.rollout_ensemble(pred, store.frames, first, counter, store.out_tab, STEPS, M, ws, **rows))
    nbytes = (M + 1) * Bt * T * 4 * H * W * 4
    out["rollout_ensemble"] = {"us": round(t * 1e6, 1), "bytes_read": nbytes, "TB_per_s": round(nbytes / t / 1e12, 3)}
    rel, crit, ep, et, nxt = new(B, STEPS * T, 4), new(B, STEPS), new(B, STEPS * T), new(B, STEPS * T), torch.empty_like(pred)
    sws = ops.rollout_score_workspace(pred)

    def score():
        counter.zero_()
        ops.rollout_score(pred, store.frames, first, counter, store.out_tab, 0, STEPS, rel, crit, sws, ep, et, nxt, None)
    t = device_time(score)
    nbytes = pred.numel() * 4 * 3                                         # prediction read, target frames read, next input written
    out["rollout_score_same_run"] = {"us": round(t * 1e6, 1), "bytes": nbytes, "TB_per_s": round(nbytes / t / 1e12, 3), "B": B}
    return out


def redistance(model, store, rounds, B=NTRAJ):
    """evaluate_rollouts(use_graph=True) and evaluate_rollouts_redistanced(RedistanceSpec(), use_graph=True) at B trajectories per forward: marginal ms per step and
    trajectory-steps per second as `summary` gives them, alternated inside every round, and the pass counts of the last corrected run."""
    from bubbleformer_amd.utils import RedistanceSpec
    from bubbleformer_amd.utils import rollout as R
    starts = [i * len(store.ds) // NTRAJ for i in range(NTRAJ)]
    last = {}

    def run(steps, spec):
        for k in range(0, NTRAJ, B):
            if spec is None:
                last["report"] = R.evaluate_rollouts(model, store, starts[k:k + B], steps, use_graph=True)
            else:
                last["report"] = R.evaluate_rollouts_redistanced(model, store, starts[k:k + B], steps, spec, use_graph=True)
    variants = {"without": lambda steps: run(steps, None), "with_redistance": lambda steps: run(steps, RedistanceSpec())}
    times = {k: [] for k in variants}
    for r in range(rounds + 1):                                         # round 0 is the warm-up and is dropped
        for name, fn in variants.items():
            pair = (clock(lambda: fn(STEPS)), clock(lambda: fn(SHORT)))
            if r:
                times[name].append(pair)
    out = {name: summary(times[name], B) for name in variants}
    passes = last["report"].redistance_rounds.float()
    out["passes_mean_max"] = [round(float(passes.mean()), 2), int(passes.max())]
    out["rms_change_mean"] = float(last["report"].redistance_change.mean())
    return out


def plan_rollouts_first(store, starts):
    from bubbleformer_amd.utils.rollout import plan_rollouts
    return plan_rollouts(store.ds, starts, STEPS).first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ensemble", default=None, help="member counts, e.g. 4,16: time the step with and without EnsembleSpec and the ensemble call alone (nothing else runs)")
    ap.add_argument("--redistance", action="store_true", help="time the batched graph variant at 8 trajectories per forward with and without RedistanceSpec() (nothing else runs)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=("today", "batched", "scoring"), default=None)
    ap.add_argument("--batches", default="1,2,4,8", help="trajectories per forward of the batched variants")
    ap.add_argument("--graph-only", action="store_true", help="leave the eager batched variants out (for a kernel-trace profile of one variant)")
    ap.add_argument("--tree", default=None, help="checkout of this repository to import bubbleformer_amd from")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("rollout_eval_bench needs a GPU", file=sys.stderr)
        return 1
    tree = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, tree)
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils import rollout as R
    from oracle import weights as Wt
    model = get_model("filmavit", time_window=T, drop_path=0.0, compute_dtype=torch.bfloat16, **CFG)
    model.load_state_dict(Wt.generate(Wt.param_shapes(**CFG), seed=42))
    model = model.cuda().eval()
    store = study()
    if a.ensemble:
        out = {"tree": tree, "geometry": f"{T}x{H}x{W}x4 bf16 FiLMAViT-small, Bt = 2 trajectories x M members, {STEPS} steps", "rounds": a.rounds}
        for M in [int(m) for m in a.ensemble.split(",")]:
            out[f"M{M}"] = ensemble(model, store, M, a.rounds)
        print(json.dumps(out))
        return 0
    if a.redistance:
        out = {"tree": tree, "geometry": f"{T}x{H}x{W}x4 bf16 FiLMAViT-small, {NTRAJ} trajectories per forward, {STEPS} steps", "rounds": a.rounds}
        out.update(redistance(model, store, a.rounds))
        print(json.dumps(out))
        return 0
    starts = [i * len(store.ds) // NTRAJ for i in range(NTRAJ)]            # the first sample of every trajectory
    variants = {}

    def today(steps):
        for i in starts:
            x, _, fl = store.gather([i])
            R.autoregressive_rollout(model, x[0], steps, fl, use_graph=True, target_fn=lambda s: store.gather([i + s * T])[1][0])

    if a.only in (None, "today"):
        variants["today"] = (1, today)
    if a.only in (None, "batched") and hasattr(R, "evaluate_rollouts"):
        for B in [int(b) for b in a.batches.split(",")]:
            for graph in ((True,) if a.graph_only else (True, False)):
                def batched(steps, B=B, graph=graph):
                    for k in range(0, NTRAJ, B):
                        R.evaluate_rollouts(model, store, starts[k:k + B], steps, use_graph=graph)
                variants[f"batched_B{B}_{'graph' if graph else 'eager'}"] = (B, batched)
    out = {"tree": tree, "geometry": f"{T}x{H}x{W}x4 bf16 FiLMAViT-small, {NTRAJ} trajectories x {STEPS} steps", "rounds": a.rounds}
    times = {k: [] for k in variants}
    for r in range(a.rounds + 1):                                       # round 0 is the process's warm-up and is dropped
        for name, (_, fn) in variants.items():
            pair = (clock(lambda: fn(STEPS)), clock(lambda: fn(SHORT)))
            if r:
                times[name].append(pair)
    for name, (B, _) in variants.items():
        out[name] = summary(times[name], B)
    if "today" in out:
        for name in [k for k in out if k.startswith("batched_")]:
            out[name]["speedup_over_today"] = round(out[name]["traj_steps_per_s"] / out["today"]["traj_steps_per_s"], 3)
    if a.only in (None, "scoring") and hasattr(R, "evaluate_rollouts"):
        out["scoring"] = {f"B{B}": scoring(store, B) for B in (1, 8)}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
