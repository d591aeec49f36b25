#!/usr/bin/env python3
"""Heat-flux evaluation, timed on one GPU: prints one JSON object.

  kde:      `bf_kde_kl` (ops.kde_kl, workspace allocated once) against the same expression in torch on the device (fp64, the points x n
            matrix of each set, row after row) and, where scipy imports, against cell 4 of examples/data_visualization.ipynb on the host
            (R = 1 only, fewer rounds: it takes seconds), at n = m = 800, 6 400 and 102 400 samples, 1000 grid points, R = 1 and 8 rows.
            Device variants are timed with device events over windows of at least 0.3 s after a warm-up, the variants alternated inside
            every round; reported: median and [min, max] of the rounds, fp64 exponentials per second (points * (n + m) * R per call) and the
            peak extra device memory of one call (torch.cuda.max_memory_allocated above the inputs).
  rollout:  the heat-flux call alone (device events over back-to-back launches), and the marginal cost per step of `evaluate_rollouts(heatflux=spec)`: FiLMAViT-small bf16, 16 x 192 x 192 x 4 clips (dx = 16 / 192),
            B = 1 and 8 trajectories per forward, graph; `off` and `on` alternated inside every round; ms per step is
            (t(50 steps) - t(10 steps)) / 40 as tools/rollout_eval_bench.py defines it, so captures and warm-ups drop out.

Usage: python tools/heatflux_eval_bench.py [--rounds R] [--only kde|rollout] [--tree CHECKOUT]
(--tree imports bubbleformer_amd from another checkout of this repository: a tree without the feature runs `off` alone, which is how the
default path is timed against the parent commit -- one process per tree, the processes alternated by the caller)."""
import argparse
import inspect
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

POINTS, EPS = 1000, 1e-10
SIZES, ROWS = (800, 6400, 102400), (1, 8)
STEPS, SHORT, T, H, W, NTRAJ = 50, 10, 16, 192, 192, 8


def med(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min_max": [round(min(v), digits), round(max(v), digits)]}


def sets(R, n, seed=7):
    rs = np.random.RandomState(seed)
    sim = rs.gamma(6.0, 2.0, (R, n)) + 3.0
    model = rs.gamma(5.0, 2.4, (R, n)) + 2.5 + 0.4 * rs.standard_normal((R, n))
    return sim, model


def torch_kl(p, q):
    """The notebook's expression in torch on the device, one row: materialises points x n per set."""
    lo, hi = torch.minimum(p.min(), q.min()), torch.maximum(p.max(), q.max())
    step = (hi - lo) / (POINTS - 1)
    x = lo + torch.arange(POINTS, dtype=torch.float64, device=p.device) * step

    def pdf(s):
        h = s.numel() ** -0.2 * s.std(unbiased=True)
        d = (x[:, None] - s[None, :]) / h
        return torch.exp(-0.5 * d * d).sum(dim=1) / (s.numel() * h * math.sqrt(2 * math.pi))
    dp, dq = pdf(p), pdf(q)
    dq = torch.where(dq == 0, torch.full_like(dq, EPS), dq)
    f = torch.where(dp == 0, torch.zeros_like(dp), dp * torch.log(dp / dq))
    M = POINTS - 1                                                      # an even point count: Simpson on the first 999, then the last interval
    return step / 3 * (f[0] + f[M - 1] + 4 * f[1:M - 1:2].sum() + 2 * f[2:M - 2:2].sum()) + step * (5 * f[-1] + 8 * f[-2] - f[-3]) / 12


def device_time(fn, floor_s=0.3):
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


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def bench_kde(rounds):
    from bubbleformer_amd import ops
    try:
        from scipy.integrate import simpson
        from scipy.stats import gaussian_kde
    except ImportError:
        gaussian_kde = None
    out = {"points": POINTS, "scipy": gaussian_kde is not None}
    for n in SIZES:
        for R in ROWS:
            sim, model = sets(R, n)
            p, q = torch.from_numpy(sim).cuda(), torch.from_numpy(model).cuda()
            kl = torch.empty(R, dtype=torch.float64, device="cuda")
            ws = ops.kde_kl_workspace(R, n, n, POINTS, "cuda")
            hip = lambda: ops.kde_kl(p, q, POINTS, EPS, ws, kl)
            ref = lambda: [torch_kl(p[r], q[r]) for r in range(R)]
            times = {"hip": [], "torch": []}
            for r in range(rounds + 1):                                 # round 0 is dropped
                for name, fn in (("hip", hip), ("torch", ref)):
                    t = device_time(fn)
                    if r:
                        times[name].append(t)
            hip()
            gap = max(abs(float(kl[r]) - float(torch_kl(p[r], q[r]))) for r in range(R))
            exps = POINTS * 2 * n * R
            row = {"kl_row0": float(kl[0]), "hip_minus_torch": gap, "workspace_bytes": ws.numel() * 8}
            for name in times:
                m = med([t * 1e3 for t in times[name]])
                row[name] = {"ms": m, "exp_per_s": round(exps / (m["median"] * 1e-3), -6)}
            row["hip"]["peak_extra_bytes"] = peak_extra(hip) + ws.numel() * 8
            row["torch"]["peak_extra_bytes"] = peak_extra(ref)
            if gaussian_kde is not None and R == 1:
                def host():
                    ks, km = gaussian_kde(sim[0]), gaussian_kde(model[0])
                    x = np.linspace(min(sim[0].min(), model[0].min()), max(sim[0].max(), model[0].max()), POINTS)
                    a, b = ks(x), km(x)
                    b = np.where(b == 0, EPS, b)
                    return simpson(a * np.log(a / b), x)
                ts = []
                for _ in range(min(rounds, 3) if n > 10000 else rounds):
                    t0 = time.perf_counter()
                    v = host()
                    ts.append(time.perf_counter() - t0)
                row["scipy_host"] = {"ms": med([t * 1e3 for t in ts]), "exp_per_s": round(POINTS * 2 * n / statistics.median(ts), -6), "hip_minus_scipy": abs(float(kl[0]) - float(v))}
            out[f"n{n}_R{R}"] = row
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
    has = "heatflux" in inspect.signature(Ro.evaluate_rollouts).parameters
    spec = None
    if has:
        from bubbleformer_amd.utils import HeaterSpec
        spec = HeaterSpec(heater_temp=[1.0 + 0.05 * i for i in range(NTRAJ)], dx=16 / 192)
    variants = {}
    for B in (1, 8):
        for name, kw in (("off", {}),) + ((("on", {"heatflux": spec}),) if has else ()):
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
    out = {"has_heatflux": has}
    if has:                                                             # the heat-flux call alone, device events
        from bubbleformer_amd import ops
        for B in (1, 8):
            first = torch.tensor(Ro.plan_rollouts(store.ds, starts[:B], STEPS).first, dtype=torch.int64, device="cuda")
            pred = store.gather(starts[:B])[1] + 0.01
            fp, ft = (torch.empty(B, STEPS * T, dtype=torch.float32, device="cuda") for _ in range(2))
            heater = torch.ones(B, dtype=torch.float32, device="cuda")
            counter = torch.zeros(1, dtype=torch.int32, device="cuda")
            call = lambda: ops.rollout_heatflux(pred, store.frames, first, counter, store.out_tab, 0, 1, heater, STEPS, fp, ft, spec.x_min, spec.dx, spec.lc, spec.conductivity)
            out[f"B{B}_heatflux_call_us"] = med([device_time(call, 0.05) * 1e6 for _ in range(5)], 2)
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
    ap.add_argument("--only", choices=("kde", "rollout"), default=None)
    ap.add_argument("--tree", default=None, help="checkout of this repository to import bubbleformer_amd from")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("heatflux_eval_bench needs a GPU", file=sys.stderr)
        return 1
    tree = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, tree)
    out = {"tree": tree, "rounds": a.rounds}
    if a.only in (None, "rollout"):
        out["rollout"] = bench_rollout(a.rounds)
    if a.only in (None, "kde"):
        import bubbleformer_amd.ops as ops
        if hasattr(ops, "kde_kl"):
            out["kde"] = bench_kde(a.rounds)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
