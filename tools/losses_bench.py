#!/usr/bin/env python3
"""utils.losses on the GPU, timed: prints one JSON object.

The native `LpLoss` (csrc/losses.hip) against the same expression in stock torch ops -- what a user of the reference's own LpLoss runs on
this GPU -- at the bench shape (8, 16, 4, 192, 192) fp32: forward + backward of the training configuration (d=2, p=2, mean B, mean T,
sum C), the generic-p case (p = 2.5), short rows (d = 1), and `eikonal_loss` forward + backward on one channel; then one whole training
step of FiLMAViT-small (bf16, batch 8) three ways: the fused TrainStep, TrainStep(criterion=native LpLoss), and the same with the eager
criterion.  One process, device events, every variant warmed; the variants of a group alternate inside a round, a round is `--reps`
back-to-back calls, and the figure is the median with [min, max] over `--rounds` rounds.  Each forward + backward is timed twice: launched
from Python call by call (`*_fwd_bwd`: what a loop that does nothing else sees; with some twenty small launches per call the host can be
the limit for either variant) and as the replay of a graph captured once (`*_fwd_bwd_graph`: the device's time for the same launches,
which is what a training step that keeps the device busy pays).

Algorithmic bytes of LpLoss: the forward reads both tensors (2 x 75.5 MB), the backward reads both and writes the gradient (3 x 75.5 MB).
Both tensors together (151 MB) fit the 256 MiB Infinity Cache and the timed calls repeat on the same buffers, so the rates are those of a
working set that can stay in that cache, not of HBM; in a training step the prediction has just been written and the gradient is read next,
which is the same situation.  `hbm_peak_share` divides by the 8 TB/s HBM figure all the same, as the other tools here do.

`--interface` adds the interface-weighted criterion (utils.losses.InterfaceLpLoss, gain 4, band 0.5 in the units of its SDF channel, field
weights 1 / 0.5 / 2 / 0.25) at the same shape, without and with its Eikonal penalty (2e-3): forward + backward call by call and as a graph
replay, in one group with the native LpLoss of the training configuration (the data term moves LpLoss's bytes, so `*_over_lp_graph` is the
price of the weight) and with the same weighted expression in stock torch ops; and one more whole training step,
TrainStep(criterion=InterfaceLpLoss with the penalty), beside the other three.

`--spectral` adds the shell-weighted spectral criterion (utils.losses.SpectralLpLoss, w = 1 + 100 (q / (K - 1))^2, field weights 1 / 0.5 / 2 /
0.25) at the same shape under the same protocol: forward + backward call by call and as a graph replay, in one group with the native LpLoss
of the training configuration and with the same expression in stock torch ops in fp32 (torch.fft.rfft2, an index by shell, and the irfft2
of its autograd backward: the rocFFT route); and one more whole training step, TrainStep(criterion=SpectralLpLoss), beside the others.
Bytes of the native call: the forward reads both tensors and writes and re-reads both half-spectra (and the error's once more, filtered), the
backward reads the saved half-spectrum and writes the gradient: 2 + 5 x 1.01 + 1.01 + 1 = 9.1 tensors of 75.5 MB.

Usage: python tools/losses_bench.py [--rounds R] [--reps K] [--step-reps K] [--no-step] [--interface] [--spectral]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPE = (8, 16, 4, 192, 192)
HBM_PEAK = 8.0e12
WARMUP_SECONDS = 0.5
TRAINING = dict(d=2, p=2, reduce_dims=[0, 1, 2], reductions=["mean", "mean", "sum"])
SMALL = dict(input_fields=4, output_fields=4, patch_size=16, embed_dim=384, num_heads=6, processor_blocks=12, attn_scale=True, feat_scale=True,
             num_fluid_params=9)


def eager_lp(d, p, reduce_dims, reductions):
    """The criterion in stock torch ops: norms of the flattened difference and target, their quotient, the reductions, squeeze."""
    def f(pred, y):
        r = torch.norm(pred.flatten(-d) - y.flatten(-d), p=p, dim=-1) / torch.norm(y.flatten(-d), p=p, dim=-1)
        for dim, how in zip(reduce_dims, reductions):
            r = r.sum(dim, keepdim=True) if how == "sum" else r.mean(dim, keepdim=True)
        return r.squeeze()
    return f


def eager_eikonal(phi):
    gy, gx = torch.gradient(phi, spacing=1 / 32, dim=(-2, -1), edge_order=1)
    return ((torch.sqrt(gy ** 2 + gx ** 2) - 1.0) ** 2).mean()


INTERFACE = dict(sdf_channel=0, band=0.5, gain=4.0, diff=0.37, div=1.98, field_weights=(1.0, 0.5, 2.0, 0.25))
INTERFACE_EIKONAL = 2e-3


def eager_interface(sdf_channel, band, gain, diff, div, field_weights, eikonal, device):
    """InterfaceLpLoss's expression in stock torch ops: the hat weight from the target, the weighted quotient per row, the field weights, the penalty."""
    a = torch.tensor(field_weights, dtype=torch.float32, device=device)

    def f(pred, y):
        w = (1 + gain * (1 - (y[:, :, sdf_channel] * div + diff).abs() / band).clamp(min=0)).unsqueeze(2)
        rho = ((w * (pred - y) ** 2).sum((-2, -1)) / (w * y ** 2).sum((-2, -1))).sqrt()
        out = (rho.mean((0, 1)) * a).sum()
        return out + eikonal * eager_eikonal(pred[:, :, sdf_channel] * div + diff) if eikonal > 0 else out
    return f


SPECTRAL = dict(gain=100.0, power=2.0, field_weights=(1.0, 0.5, 2.0, 0.25))


def shell_table_half(H, W):
    """(H, W // 2 + 1) int64: the shell of mode (ky, kx <= W / 2), DESIGN.md section 18's rule in Python integers."""
    import math
    S = min(H, W)
    rows = []
    for ky in range(H):
        fy = ky if ky <= H // 2 else ky - H
        rows.append([math.isqrt(S * S * (fy * fy * W * W + fx * fx * H * H) // (H * H * W * W)) for fx in range(W // 2 + 1)])
    return torch.tensor(rows, dtype=torch.int64)


def eager_spectral(shell_weights, field_weights, H, W, device):
    """SpectralLpLoss's expression in stock torch ops, fp32: rfft2, the weight of every mode by an index into the table, the Hermitian half
    counted twice where it is mirrored; autograd's backward runs the irfft2."""
    wm = shell_weights.to(device, torch.float32)[:, shell_table_half(H, W).to(device)]
    kx = torch.arange(W // 2 + 1, device=device)
    wm = wm * torch.where((kx == 0) | (2 * kx == W), 1.0, 2.0).to(torch.float32)
    a = torch.tensor(field_weights, dtype=torch.float32, device=device)

    def f(pred, y):
        E, Y = torch.fft.rfft2(pred - y), torch.fft.rfft2(y)
        se, sy = (wm * (E.real ** 2 + E.imag ** 2)).sum((-2, -1)), (wm * (Y.real ** 2 + Y.imag ** 2)).sum((-2, -1))
        return ((se / sy).sqrt().mean((0, 1)) * a).sum()
    return f


def spectral_criterion():
    from bubbleformer_amd.utils import SpectralLpLoss
    return SpectralLpLoss.power_law(SHAPE[-2], SHAPE[-1], SPECTRAL["gain"], SPECTRAL["power"], C=SHAPE[2], field_weights=SPECTRAL["field_weights"])


def spectral_group(pred, y, rounds, reps):
    from bubbleformer_amd.utils import LpLoss
    crit = spectral_criterion()
    variants = {"lp": LpLoss(**TRAINING), "spectral": crit,
                "eager_spectral": eager_spectral(crit.shell_weights, SPECTRAL["field_weights"], SHAPE[-2], SHAPE[-1], pred.device)}
    calls = {k + "_fwd_bwd": fwd_bwd(c, pred, y) for k, c in variants.items()}
    calls.update({k + "_fwd_bwd_graph": graphed(c, pred, y) for k, c in variants.items()})
    ms = timed(calls, rounds, reps)
    tensor = pred.numel() * 4
    half = (SHAPE[-1] // 2 + 1) * 2 / SHAPE[-1]
    nbytes = {k: (3 + 6 * half) * tensor if "spectral" in k else 5 * tensor for k in calls}
    out = {k: summary(t, nbytes[k]) for k, t in ms.items()}
    out["saved_intermediate_MB"] = round(half * tensor / 1e6, 1)
    med = {k: statistics.median(t) for k, t in ms.items()}
    for tag in ("", "_graph"):
        out[f"spectral_over_lp{tag}"] = round(med[f"spectral_fwd_bwd{tag}"] / med[f"lp_fwd_bwd{tag}"], 3)
        out[f"eager_over_native_spectral{tag}"] = round(med[f"eager_spectral_fwd_bwd{tag}"] / med[f"spectral_fwd_bwd{tag}"], 3)
    return out


def timed(calls, rounds, reps):
    """{name: callable} -> {name: [ms per call, one per round]}, the callables alternating inside every round."""
    t0 = time.perf_counter()                         # warm-up: untimed rounds of every variant for at least half a second (code objects,
    while True:                                      # allocator, and the clocks of a device that was idle: the first timed round of a
        for f in calls.values():                     # process otherwise reads up to twice the steady time for every variant alike)
            for _ in range(reps):
                f()
        torch.cuda.synchronize()
        if time.perf_counter() - t0 >= WARMUP_SECONDS:
            break
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


def summary(t, nbytes=None):
    med = statistics.median(t)
    out = {"us": round(med * 1e3, 2), "us_min": round(min(t) * 1e3, 2), "us_max": round(max(t) * 1e3, 2)}
    if nbytes is not None:
        out.update(algorithmic_MB=round(nbytes / 1e6, 1), TB_s=round(nbytes / (med * 1e-3) / 1e12, 3), hbm_peak_share=round(nbytes / (med * 1e-3) / HBM_PEAK, 3))
    return out


def fwd_bwd(criterion, pred, y):
    def f():
        pred.grad = None
        criterion(pred, y).backward()
    return f


def graphed(criterion, pred, y):
    """forward + backward captured once on one stream (a linear graph); the replay has no host work between the launches."""
    sp = pred.detach().clone().requires_grad_(True)

    def body():
        return torch.autograd.grad(criterion(sp, y), sp)
    body()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = body()
    graph.keep = keep
    return graph.replay


def lp_group(kw, pred, y, rounds, reps, parts=False):
    from bubbleformer_amd.utils import LpLoss
    from bubbleformer_amd.utils.losses import lp_rows
    native, eager = LpLoss(**kw), eager_lp(**kw)
    calls = {"native_fwd_bwd": fwd_bwd(native, pred, y), "eager_fwd_bwd": fwd_bwd(eager, pred, y)}
    calls.update(native_fwd_bwd_graph=graphed(native, pred, y), eager_fwd_bwd_graph=graphed(eager, pred, y))
    tensor = pred.numel() * 4
    nbytes = {k: 5 * tensor for k in calls}
    if parts:
        ratio = lp_rows(pred, y, kw["d"], kw["p"])
        g = torch.full_like(ratio, 1.0 / ratio.numel())

        def fwd():
            with torch.no_grad():
                lp_rows(pred, y, kw["d"], kw["p"])
        calls["native_fwd"] = fwd
        calls["native_bwd"] = lambda: torch.autograd.grad(ratio, pred, g, retain_graph=True)
        nbytes.update(native_fwd=2 * tensor, native_bwd=3 * tensor)
    ms = timed(calls, rounds, reps)
    out = {k: summary(t, nbytes[k]) for k, t in ms.items()}
    for tag in ("", "_graph"):
        n, e = ms["native_fwd_bwd" + tag], ms["eager_fwd_bwd" + tag]
        out["eager_over_native" + tag] = round(statistics.median(e) / statistics.median(n), 3)
        out["intervals_disjoint" + tag] = bool(max(n) < min(e))
    return out


def interface_group(pred, y, rounds, reps):
    from bubbleformer_amd.utils import InterfaceLpLoss, LpLoss
    kw = dict(INTERFACE)
    s, band, gain = kw.pop("sdf_channel"), kw.pop("band"), kw.pop("gain")
    variants = {"lp": LpLoss(**TRAINING), "interface": InterfaceLpLoss(s, band, gain, **kw),
                "interface_eikonal": InterfaceLpLoss(s, band, gain, eikonal=INTERFACE_EIKONAL, **kw),
                "eager_interface": eager_interface(eikonal=0.0, device=pred.device, **INTERFACE),
                "eager_interface_eikonal": eager_interface(eikonal=INTERFACE_EIKONAL, device=pred.device, **INTERFACE)}
    calls = {k + "_fwd_bwd": fwd_bwd(c, pred, y) for k, c in variants.items()}
    calls.update({k + "_fwd_bwd_graph": graphed(c, pred, y) for k, c in variants.items()})
    ms = timed(calls, rounds, reps)
    out = {k: summary(t, 5 * pred.numel() * 4) for k, t in ms.items()}
    med = {k: statistics.median(t) for k, t in ms.items()}
    for tag in ("", "_graph"):
        for k in ("interface", "interface_eikonal"):
            out[f"{k}_over_lp{tag}"] = round(med[f"{k}_fwd_bwd{tag}"] / med[f"lp_fwd_bwd{tag}"], 3)
            out[f"eager_over_native_{k}{tag}"] = round(med[f"eager_{k}_fwd_bwd{tag}"] / med[f"{k}_fwd_bwd{tag}"], 3)
    return out


def step_group(rounds, reps, interface=False, spectral=False):
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils import InterfaceLpLoss, LpLoss
    g = torch.Generator(device="cuda").manual_seed(42)
    x = torch.randn(SHAPE, device="cuda", generator=g)
    y = torch.randn(SHAPE, device="cuda", generator=g)
    c = torch.randn((SHAPE[0], 9), device="cuda", generator=g)
    steps = {}
    legs = [("fused", None), ("native_criterion", LpLoss(**TRAINING)), ("eager_criterion", eager_lp(**TRAINING))]
    if interface:
        kw = dict(INTERFACE)
        legs.append(("interface_criterion", InterfaceLpLoss(kw.pop("sdf_channel"), kw.pop("band"), kw.pop("gain"), eikonal=INTERFACE_EIKONAL, **kw)))
    if spectral:
        legs.append(("spectral_criterion", spectral_criterion()))
    for name, crit in legs:
        torch.manual_seed(0)
        model = get_model("filmavit", time_window=SHAPE[1], drop_path=0.2, compute_dtype=torch.bfloat16, **SMALL).cuda().train()
        step = TrainStep(model, lr=2.5e-4, weight_decay=1e-2, criterion=crit)
        steps[name] = (lambda s=step: s(x, c, y))
    ms = timed(steps, rounds, reps)
    out = {k: {"ms": round(statistics.median(t), 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3)} for k, t in ms.items()}
    out["unfused_price_ms"] = round(statistics.median(ms["native_criterion"]) - statistics.median(ms["fused"]), 3)
    if interface:
        out["interface_price_ms"] = round(statistics.median(ms["interface_criterion"]) - statistics.median(ms["native_criterion"]), 3)
    if spectral:
        out["spectral_price_ms"] = round(statistics.median(ms["spectral_criterion"]) - statistics.median(ms["native_criterion"]), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--step-reps", type=int, default=20, help="training steps per round (a step is tens of milliseconds)")
    ap.add_argument("--no-step", action="store_true", help="skip the whole-training-step comparison")
    ap.add_argument("--interface", action="store_true", help="add the interface-weighted criterion's group and its training-step leg")
    ap.add_argument("--spectral", action="store_true", help="add the shell-weighted spectral criterion's group and its training-step leg")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/losses_bench.py times GPU kernels: no GPU found"
    from bubbleformer_amd.utils import eikonal_loss
    g = torch.Generator(device="cuda").manual_seed(0)
    pred = torch.randn(SHAPE, device="cuda", generator=g).requires_grad_(True)
    y = torch.randn(SHAPE, device="cuda", generator=g) * 1.5 + 0.25
    res = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "rounds": args.rounds, "reps": args.reps,
           "cache_level": "working set 151 MB (226 MB with the gradient) stays within the 256 MiB Infinity Cache between calls"}
    res["training_configuration"] = lp_group(TRAINING, pred, y, args.rounds, args.reps, parts=True)
    res["generic_p_2_5"] = lp_group(dict(TRAINING, p=2.5), pred, y, args.rounds, args.reps)
    res["d1_short_rows"] = lp_group(dict(d=1, p=2, reduce_dims=[0, 1, 2, 3], reductions=["mean", "mean", "sum", "mean"]), pred, y, args.rounds, args.reps)
    phi = (pred.detach()[:, :, 0] * 0.05 + 0.3).contiguous().requires_grad_(True)
    ms = timed({"native_fwd_bwd": fwd_bwd(lambda a, _: eikonal_loss(a), phi, None), "eager_fwd_bwd": fwd_bwd(lambda a, _: eager_eikonal(a), phi, None)},
               args.rounds, args.reps)
    res["eikonal_one_channel"] = {k: summary(t, 3 * phi.numel() * 4) for k, t in ms.items()}
    res["eikonal_one_channel"]["eager_over_native"] = round(statistics.median(ms["eager_fwd_bwd"]) / statistics.median(ms["native_fwd_bwd"]), 3)
    if args.interface:
        res["interface"] = interface_group(pred, y, args.rounds, args.reps)
    if args.spectral:
        res["spectral"] = spectral_group(pred, y, args.rounds, args.reps)
    if not args.no_step:
        del pred, y, phi
        torch.cuda.empty_cache()
        res["train_step_filmavit_small_bf16_b8"] = step_group(args.rounds, args.step_reps, args.interface, args.spectral)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
