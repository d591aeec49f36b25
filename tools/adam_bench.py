#!/usr/bin/env python3
"""Fused optimizer kernels, timed on the GPU: prints one JSON object.

bf_adam (torch.optim.Adam) against bf_adamw (torch.optim.AdamW) on the flat fp32 buffers TrainStep keeps for FiLMAViT-small
(E 384, 6 heads, 12 blocks) and film_avit_big (E 768, 12 heads, 12 blocks), sized as trainer.FlatParams lays them out (every parameter
padded to 64 elements).  Each step reads p, g, m, v and writes p, m, v: 28 bytes per element.  The two kernels alternate in rounds of
`--reps` back-to-back launches timed by device events; the per-launch time is the median over rounds.  Reported: ms per launch, GB/s,
and the share of the 8.0 TB/s HBM peak (MI355X_MICROARCH: about 6.3 TB/s is achievable by a float4 copy).

--average times the averaged-weights step (EMA / SWA) instead, per optimizer (AdamW, Adam, Lion) under the same
protocol: (a) the plain step, (b) the step with its record's avg set, which also reads and writes the average (36 bytes per element;
Lion 28 against 20), (c) the plain step followed by bf_weight_average (40; Lion 32, and a second launch).

--groups times the parameter-group launch per optimizer (AdamW, Lion) under the same protocol: (a) the unchanged
ungrouped step, (b) the step with its record's groups set and every group live -- the table utils.param_groups gives no_weight_decay +
layer_decay(0.75) on the model's parameter names and shapes, (c) the grouped step with the trunk (blocks.*) frozen.  The grouped launches also read one map
byte per 64 elements; a frozen chunk moves no other byte, so (c) is reported beside the live share of the buffer.

--guard times the step guard per optimizer (AdamW, Lion) under the same protocol: (a) "unguarded", the launch of a
record without live_dev -- with --parent-lib (a libbubbleformer_hip.so built from the commit before the guard, whose record has no such
member) beside "parent", the same launch from that library, alternating in the same rounds, and the parent's own run-to-run spread
(ms_min .. ms_max over the rounds) is the yardstick for their difference; (b) "guarded_live", the record with live_dev set and the flag 1;
(c) "skipped", the flag 0: the launch reads four bytes and leaves; (d) "norm_and_guard", bf_grad_norm + bf_step_guard, what a step without
clipping by norm adds for the guard (one 4-byte read per element, three tiny launches).

Usage: python tools/adam_bench.py [--rounds R] [--reps K] [--average | --groups | --guard [--parent-lib PATH]]"""
import argparse
import ctypes as C
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


ADAM = dict(step=10, lr=2.5e-4, beta1=0.9, beta2=0.999, eps=1e-8)
LION = dict(lr=5e-5, beta1=0.9, beta2=0.99, wd=0.1)


def opt_call(entry, p, g, m, v=None, **fields):
    """A call of bf_adamw / bf_adam / bf_lion on one bf_opt_step record, built once by field name (gscale 1, no clamp unless `fields` says so)."""
    rec = L.OptStep(**{**dict(p=_p(p), g=_p(g), m=_p(m), v=None if v is None else _p(v), n=p.numel(), gscale=1.0, clip_value=float("inf")), **fields})
    fn, ref, st = getattr(L.lib(), entry), C.byref(rec), _stream()
    return lambda: fn(ref, st)


def group_fields(t):
    return dict(chunk_group=_p(t.chunk), group_lr_scale=_p(t.lr_scale), group_weight_decay=_p(t.weight_decay), group_frozen=_p(t.frozen), n_groups=t.n_groups)


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
    calls = {"adam": opt_call("bf_adam", p, grad, m, v, wd=1e-5, **ADAM), "adamw": opt_call("bf_adamw", p, grad, m, v, wd=1e-2, **ADAM)}
    ms = rounds_of(calls, rounds, reps)
    assert torch.isfinite(p).all()
    out = {k: summary(t, n, BYTES_PER_ELEMENT) for k, t in ms.items()}
    out["adam_over_adamw"] = round(out["adam"]["ms"] / out["adamw"]["ms"], 3)
    return out


def time_average(n, rounds, reps):
    """Per optimizer: (a) "plain", (b) "fused" = the step with avg set, (c) "separate" = plain + bf_weight_average; bytes per element are what
    each moves (a: 28 / Lion 20; b: + 8; c: + 12)."""
    g = torch.Generator(device="cuda").manual_seed(0)
    p = torch.randn(n, device="cuda", generator=g) * 0.02
    grad = torch.randn(n, device="cuda", generator=g) * 1e-3
    m, v, a = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    h, st, w = L.lib(), _stream(), 1e-3
    steps = {"adamw": lambda **kw: opt_call("bf_adamw", p, grad, m, v, wd=1e-2, **ADAM, **kw), "adam": lambda **kw: opt_call("bf_adam", p, grad, m, v, wd=1e-5, **ADAM, **kw),
             "lion": lambda **kw: opt_call("bf_lion", p, grad, m, **LION, **kw)}
    plain = {opt: step() for opt, step in steps.items()}
    fused = {opt: step(avg=_p(a), avg_weight=w) for opt, step in steps.items()}
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
    """Per optimizer: "ungrouped" (bf_adamw / bf_lion), "all_live" and "trunk_frozen" (the same entry with groups); ms per launch, and each grouped
    launch over the ungrouped one of the same run."""
    from bubbleformer_amd.utils import param_groups as PG
    g = torch.Generator(device="cuda").manual_seed(0)
    p = torch.randn(n, device="cuda", generator=g) * 0.02
    grad = torch.randn(n, device="cuda", generator=g) * 1e-3
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    out = {}
    for opt, wd, base in (("adamw", 1e-2, 28), ("lion", 0.1, 20)):
        live_t, G_live, _ = group_tables(cfg, lambda named: PG.no_weight_decay() + PG.layer_decay(named, 0.75), wd)
        froz_t, G_froz, share = group_tables(cfg, lambda named: PG.freeze(r"^blocks\."), wd)

        def step(**kw):
            if opt == "adamw":
                return opt_call("bf_adamw", p, grad, m, v, **{**ADAM, "wd": wd, **kw})
            return opt_call("bf_lion", p, grad, m, **{**LION, "wd": wd, **kw})
        ms = rounds_of({"ungrouped": step(), "all_live": step(**group_fields(live_t)), "trunk_frozen": step(**group_fields(froz_t))}, rounds, reps)
        res = {"ungrouped": summary(ms["ungrouped"], n, base), "all_live": summary(ms["all_live"], n, base),
               "trunk_frozen": summary(ms["trunk_frozen"], int(n * share), base)}
        res["groups_all_live"], res["groups_trunk_frozen"], res["live_share_trunk_frozen"] = G_live, G_froz, round(share, 4)
        res["all_live_over_ungrouped"] = round(res["all_live"]["ms"] / res["ungrouped"]["ms"], 3)
        res["trunk_frozen_over_ungrouped"] = round(res["trunk_frozen"]["ms"] / res["ungrouped"]["ms"], 3)
        out[opt] = res
    assert torch.isfinite(p).all()
    return out


class ParentOptStep(C.Structure):
    """bf_opt_step as it was before live_dev: what a library built from the parent commit reads."""
    _fields_ = [f for f in L.OptStep._fields_ if f[0] != "live_dev"]


def parent_call(lib, entry, p, g, m, v=None, **fields):
    rec = ParentOptStep(**{**dict(p=_p(p), g=_p(g), m=_p(m), v=None if v is None else _p(v), n=p.numel(), gscale=1.0, clip_value=float("inf")), **fields})
    fn, ref, st = getattr(lib, entry), C.byref(rec), C.c_void_p(_stream())
    fn.restype = C.c_int
    return lambda: fn(ref, st)


def time_guard(n, rounds, reps, parent_lib=None):
    """Per optimizer: "unguarded", "guarded_live", "skipped" (ms per launch), "norm_and_guard" (bf_grad_norm + bf_step_guard), and with a
    parent library "parent" with the spread its rounds show; every difference is reported in ms beside that spread."""
    g = torch.Generator(device="cuda").manual_seed(0)
    p = torch.randn(n, device="cuda", generator=g) * 0.02
    grad = torch.randn(n, device="cuda", generator=g) * 1e-3
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    h, st = L.lib(), _stream()
    one, zero = torch.ones(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    pair, guard = torch.zeros(2, device="cuda"), torch.tensor([1, 0, 0, -1], dtype=torch.int32, device="cuda")
    ws = torch.empty(int(h.bf_grad_norm_ws_doubles(n)), dtype=torch.float64, device="cuda")

    def norm_and_guard():
        h.bf_grad_norm(_p(grad), n, 1.0, float("inf"), _p(pair), _p(ws), ws.numel(), st)
        return h.bf_step_guard(_p(pair), 1, _p(guard), st)
    out = {}
    for opt, entry, base, hyper in (("adamw", "bf_adamw", 28, dict(ADAM, wd=1e-2)), ("lion", "bf_lion", 20, LION)):
        bufs = (p, grad, m, v) if opt == "adamw" else (p, grad, m)
        calls = {}
        if parent_lib is not None:
            calls["parent"] = parent_call(parent_lib, entry, *bufs, **hyper)
        calls.update(unguarded=opt_call(entry, *bufs, **hyper), guarded_live=opt_call(entry, *bufs, live_dev=_p(one), **hyper),
                     skipped=opt_call(entry, *bufs, live_dev=_p(zero), **hyper), norm_and_guard=norm_and_guard)
        ms = rounds_of(calls, rounds, reps)
        res = {k: summary(ms[k], n, 4 if k == "norm_and_guard" else base) for k in calls}
        for k in ("GB_s", "hbm_peak_share"):
            res["skipped"].pop(k)                  # a skipped launch moves four bytes
        yard = res.get("parent", res["unguarded"])
        res["spread_ms"] = round(yard["ms_max"] - yard["ms_min"], 4)
        res["spread_of"] = "parent" if "parent" in res else "unguarded"
        if "parent" in res:
            res["unguarded_minus_parent_ms"] = round(res["unguarded"]["ms"] - res["parent"]["ms"], 4)
        res["guarded_live_minus_unguarded_ms"] = round(res["guarded_live"]["ms"] - res["unguarded"]["ms"], 4)
        out[opt] = res
    assert torch.isfinite(p).all() and guard.tolist() == [1, 0, 0, -1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--average", action="store_true", help="time the averaged-weights step: plain, fused (avg set), plain + bf_weight_average")
    ap.add_argument("--groups", action="store_true", help="time the parameter-group launch: ungrouped, every group live, trunk frozen")
    ap.add_argument("--guard", action="store_true", help="time the step guard: unguarded, guarded live, skipped, the norm pass + bf_step_guard")
    ap.add_argument("--parent-lib", default=None, help="--guard: a libbubbleformer_hip.so built from the commit before the guard, timed beside this tree's")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/adam_bench.py times GPU kernels: no GPU found"
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "bytes_per_element": BYTES_PER_ELEMENT}
    parent = None
    if args.guard and args.parent_lib:
        L.lib()                                      # this tree's library first: it binds the HIP runtime both use
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        res["parent_lib"] = os.path.basename(args.parent_lib)
    for name, cfg in MODELS.items():
        params, n = flat_sizes(cfg)
        if args.groups:
            timed = time_groups(cfg, n, args.rounds, args.reps)
        elif args.guard:
            timed = time_guard(n, args.rounds, args.reps, parent)
        else:
            timed = (time_average if args.average else time_kernels)(n, args.rounds, args.reps)
        res[name] = dict(parameters=params, flat_elements=n, **timed)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
