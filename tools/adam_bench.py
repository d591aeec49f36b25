#!/usr/bin/env python3
"""Fused optimizer kernels, timed on the GPU: prints one JSON object.

bf_adam (torch.optim.Adam) against bf_adamw (torch.optim.AdamW) on the flat fp32 buffers TrainStep keeps for FiLMAViT-small
(E 384, 6 heads, 12 blocks) and film_avit_big (E 768, 12 heads, 12 blocks), sized as trainer.FlatParams lays them out (every parameter
padded to 64 elements).  Each step reads p, g, m, v and writes p, m, v: 28 bytes per element.  The two kernels alternate in rounds of
`--reps` back-to-back launches timed by device events; the per-launch time is the median over rounds.  Reported: ms per launch, GB/s,
and the share of the 8.0 TB/s HBM peak (MI355X_MICROARCH: about 6.3 TB/s is achievable by a float4 copy).

--average times the averaged-weights step (EMA / SWA) instead, per optimizer (AdamW, Adam, Lion) under the same
protocol: (a) the unchanged plain entry, (b) the _avg entry, which also reads and writes the average (36 bytes per element; Lion 28
against 20), (c) the plain entry followed by bf_weight_average (40; Lion 32, and a second launch).

--groups times the parameter-group launch per optimizer (AdamW, Lion) under the same protocol: (a) the unchanged
ungrouped entry, (b) the _groups entry with every group live -- the table utils.param_groups gives no_weight_decay + layer_decay(0.75) on
the model's parameter names and shapes, (c) the _groups entry with the trunk (blocks.*) frozen.  The grouped launches also read one map
byte per 64 elements; a frozen chunk moves no other byte, so (c) is reported beside the live share of the buffer.

Usage: python tools/adam_bench.py [--rounds R] [--reps K] [--average | --groups]"""
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


def rounds_of(calls, rounds, reps):
    """ms per launch of every call, one list entry per round; the calls alternate inside a round."""
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
    return ms


def summary(t, n, bytes_per_element):
    med = statistics.median(t)
    gbs = bytes_per_element * n / (med * 1e-3) / 1e9
    return {"ms": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4), "GB_s": round(gbs, 1),
            "hbm_peak_share": round(gbs * 1e9 / HBM_PEAK, 3)}


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
    ms = rounds_of(calls, rounds, reps)
    assert torch.isfinite(p).all()
    out = {k: summary(t, n, BYTES_PER_ELEMENT) for k, t in ms.items()}
    out["adam_over_adamw"] = round(out["adam"]["ms"] / out["adamw"]["ms"], 3)
    return out


def time_average(n, rounds, reps):
    """Per optimizer: (a) "plain", (b) "fused" = the _avg entry, (c) "separate" = plain + bf_weight_average; bytes per element are what
    each moves (a: 28 / Lion 20; b: + 8; c: + 12)."""
    g = torch.Generator(device="cuda").manual_seed(0)
    p = torch.randn(n, device="cuda", generator=g) * 0.02
    grad = torch.randn(n, device="cuda", generator=g) * 1e-3
    m, v, a = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    h, st, inf, w = L.lib(), _stream(), float("inf"), 1e-3
    adam_args = lambda wd: (_p(p), _p(grad), _p(m), _p(v), n, 10, 2.5e-4, 0.9, 0.999, 1e-8, wd, 1.0)      # noqa: E731
    lion_args = (_p(p), _p(grad), _p(m), n, 5e-5, 0.9, 0.99, 0.1, 1.0)
    plain = {"adamw": lambda: h.bf_adamw(*adam_args(1e-2), st), "adam": lambda: h.bf_adam(*adam_args(1e-5), st), "lion": lambda: h.bf_lion(*lion_args, st)}
    fused = {"adamw": lambda: h.bf_adamw_avg(*adam_args(1e-2), None, inf, _p(a), w, st), "adam": lambda: h.bf_adam_avg(*adam_args(1e-5), None, inf, _p(a), w, st),
             "lion": lambda: h.bf_lion_avg(*lion_args, None, inf, _p(a), w, st)}
    out = {}
    for opt in ("adamw", "adam", "lion"):
        def separate(f=plain[opt]):
            f()
            return h.bf_weight_average(_p(a), _p(p), n, w, st)
        ms = rounds_of({"plain": plain[opt], "fused": fused[opt], "separate": separate}, rounds, reps)
        base = 20 if opt == "lion" else 28
        res = {"plain": summary(ms["plain"], n, base), "fused": summary(ms["fused"], n, base + 8), "separate": summary(ms["separate"], n, base + 12)}
        res["fused_over_plain"] = round(res["fused"]["ms"] / res["plain"]["ms"], 3)
        res["separate_over_plain"] = round(res["separate"]["ms"] / res["plain"]["ms"], 3)
        res["expected_by_bytes"] = {"fused_over_plain": round((base + 8) / base, 3), "separate_over_plain": round((base + 12) / base, 3)}
        out[opt] = res
    assert torch.isfinite(p).all() and torch.isfinite(a).all()
    return out


def group_tables(cfg, specs_of, weight_decay):
    """ops.ParamGroupTables for the model's flat layout from its parameter names and shapes alone (meta tensors), and the live share."""
    from bubbleformer_amd import ops
    from bubbleformer_amd.utils import param_groups as PG
    named = [(k, torch.empty(shape, device="meta")) for k, shape in W.param_shapes(**cfg).items()]
    offs, n = [], 0
    for _, t in named:
        offs.append(n)
        n += (t.numel() + PG.CHUNK - 1) // PG.CHUNK * PG.CHUNK
    res = PG.resolve(named, specs_of(named), weight_decay)
    cmap = res.chunk_map([k for k, _ in named], offs, n)
    frozen = torch.tensor([t[2] for t in res.table])
    live = 1.0 - float(frozen[cmap.long()].float().mean())
    return ops.param_group_tables(cmap, [t[0] for t in res.table], [t[1] for t in res.table], [t[2] for t in res.table], n, "cuda"), len(res), live


def time_groups(cfg, n, rounds, reps):
    """Per optimizer: "ungrouped" (bf_adamw / bf_lion), "all_live" and "trunk_frozen" (the _groups entry); ms per launch, and each grouped
    launch over the ungrouped one of the same run."""
    from bubbleformer_amd.utils import param_groups as PG
    g = torch.Generator(device="cuda").manual_seed(0)
    p = torch.randn(n, device="cuda", generator=g) * 0.02
    grad = torch.randn(n, device="cuda", generator=g) * 1e-3
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    h, st, inf = L.lib(), _stream(), float("inf")
    out = {}
    for opt, wd, base in (("adamw", 1e-2, 28), ("lion", 0.1, 20)):
        live_t, G_live, _ = group_tables(cfg, lambda named: PG.no_weight_decay() + PG.layer_decay(named, 0.75), wd)
        froz_t, G_froz, share = group_tables(cfg, lambda named: PG.freeze(r"^blocks\."), wd)

        def grouped(t):
            tabs = (_p(t.chunk), _p(t.lr_scale), _p(t.weight_decay), _p(t.frozen), t.n_groups)
            if opt == "adamw":
                return lambda: h.bf_adamw_groups(_p(p), _p(grad), _p(m), _p(v), n, 10, 2.5e-4, 0.9, 0.999, 1e-8, 1.0, None, inf, None, 0.0, *tabs, st)
            return lambda: h.bf_lion_groups(_p(p), _p(grad), _p(m), n, 5e-5, 0.9, 0.99, 1.0, None, inf, None, 0.0, *tabs, st)
        plain = (lambda: h.bf_adamw(_p(p), _p(grad), _p(m), _p(v), n, 10, 2.5e-4, 0.9, 0.999, 1e-8, wd, 1.0, st)) if opt == "adamw" else \
            (lambda: h.bf_lion(_p(p), _p(grad), _p(m), n, 5e-5, 0.9, 0.99, wd, 1.0, st))
        ms = rounds_of({"ungrouped": plain, "all_live": grouped(live_t), "trunk_frozen": grouped(froz_t)}, rounds, reps)
        res = {"ungrouped": summary(ms["ungrouped"], n, base), "all_live": summary(ms["all_live"], n, base),
               "trunk_frozen": summary(ms["trunk_frozen"], int(n * share), base)}
        res["groups_all_live"], res["groups_trunk_frozen"], res["live_share_trunk_frozen"] = G_live, G_froz, round(share, 4)
        res["all_live_over_ungrouped"] = round(res["all_live"]["ms"] / res["ungrouped"]["ms"], 3)
        res["trunk_frozen_over_ungrouped"] = round(res["trunk_frozen"]["ms"] / res["ungrouped"]["ms"], 3)
        out[opt] = res
    assert torch.isfinite(p).all()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--average", action="store_true", help="time the averaged-weights step: plain, fused _avg entry, plain + bf_weight_average")
    ap.add_argument("--groups", action="store_true", help="time the parameter-group launch: ungrouped, every group live, trunk frozen")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/adam_bench.py times GPU kernels: no GPU found"
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "bytes_per_element": BYTES_PER_ELEMENT}
    for name, cfg in MODELS.items():
        params, n = flat_sizes(cfg)
        if args.groups:
            timed = time_groups(cfg, n, args.rounds, args.reps)
        else:
            timed = (time_average if args.average else time_kernels)(n, args.rounds, args.reps)
        res[name] = dict(parameters=params, flat_elements=n, **timed)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
