#!/usr/bin/env python3
"""Long attention axes, timed on the GPU: prints one JSON object.

  attention: bf_attn_fwd / bf_attn_bwd (bf16, d = 64, 6 heads, contiguous sequences) at L = 32 (the short MFMA kernels) and 48 / 64 / 128
             (csrc/attn_long.hip) with the token count held fixed, per launch (the library's HIP-event timing) and per (token x key);
  native:    one bf16 AdamW training step (TrainStep) of FiLMAViT-small (E 384, 6 heads, 12 blocks) at 16 x 512 x 512, patch 8 (64 x 64
             tokens), batch 1;
  eager:     the same step on the oracle restatement under bf16 autocast with torch.optim.AdamW, as bench.py --eager-gpu-baseline does.

Usage: python tools/long_axes_bench.py [--steps K] [--warmup W] [--skip-eager] [--attention-only | --step-only]"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from bubbleformer_amd import _lib as L  # noqa: E402
from bubbleformer_amd.ops import _dt, _p, _stream  # noqa: E402

CFG = dict(input_fields=4, output_fields=4, patch_size=8, embed_dim=384, num_heads=6, processor_blocks=12, num_fluid_params=9)
T, H, W = 16, 512, 512


def attention(reps):
    h = L.lib()
    heads, d, ntok = 6, 64, 64 * 64 * 16
    E = heads * d
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(ntok, 3 * E, device="cuda", generator=g).bfloat16()
    dout = torch.randn(ntok, E, device="cuda", generator=g).bfloat16()
    out = torch.zeros(ntok, E, device="cuda", dtype=torch.bfloat16)
    dqkv = torch.zeros_like(qkv)
    prm = [torch.ones(d, device="cuda"), torch.zeros(d, device="cuda"), torch.ones(d, device="cuda"), torch.zeros(d, device="cuda"),
           0.1 * torch.randn(32, heads, device="cuda", generator=g), torch.ones(heads, device="cuda")]
    grads = [torch.zeros_like(t) for t in prm]
    ws_floats = 1024 * (4 * 128 + 32 * 16 + 16)
    ws = torch.empty(ws_floats, device="cuda")

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        h.bf_prof_enable(1)
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 14)
        h.bf_prof_report(buf, len(buf))
        h.bf_prof_enable(0)
        return {k: v["ms"] / v["calls"] * 1e3 for k, v in json.loads(buf.value.decode()).items()}

    res = {}
    for Lq in (32, 48, 64, 128):
        geo = (ntok // Lq, Lq, 1, Lq, 0, 1)
        f = lambda: L.check(h.bf_attn_fwd(1, _p(qkv), _p(out), *geo, heads, d, *[_p(t) for t in prm], 1.0, 0, _stream()), "fwd")
        b = lambda: L.check(h.bf_attn_bwd(1, _p(qkv), _p(dout), _p(dqkv), *geo, heads, d, *[_p(t) for t in prm], *[_p(t) for t in grads],
                                          1.0, 0, _p(ws), ws_floats, _stream()), "bwd")
        tf, tb = timed(f)["attn_fwd"], sum(timed(b).values())
        tk = ntok * Lq * heads
        res[f"L{Lq}"] = {"fwd_us": round(tf, 1), "bwd_us": round(tb, 1), "fwd_ps_per_token_key": round(tf * 1e6 / tk, 2),
                         "bwd_ps_per_token_key": round(tb * 1e6 / tk, 2)}
    return res


def batch(seed):
    from oracle import weights as Wt
    x = Wt.synthetic_clip(1, T, CFG["input_fields"], H, W, seed).cuda()
    y = Wt.synthetic_clip(1, T, CFG["output_fields"], H, W, seed + 1).cuda()
    c = Wt.synthetic_fluid_params(1, CFG["num_fluid_params"], seed + 2).cuda()
    return x, c, y


def time_steps(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def native(steps, warmup):
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.trainer import TrainStep
    from oracle import weights as Wt
    m = get_model("filmavit", time_window=T, drop_path=0.0, compute_dtype=torch.bfloat16, **CFG)
    m.load_state_dict(Wt.generate(Wt.param_shapes(**CFG), seed=42))
    m = m.cuda()
    step = TrainStep(m, lr=2.5e-4, weight_decay=1e-2)
    x, c, y = batch(42)
    return {"ms_per_step": round(time_steps(lambda: step(x, c, y), steps, warmup), 2)}


def eager(steps, warmup):
    from oracle import filmavit_ref as R, weights as Wt
    sd = {k: v.cuda().requires_grad_(True) for k, v in Wt.generate(Wt.param_shapes(**CFG), seed=42).items()}
    opt = torch.optim.AdamW(list(sd.values()), lr=2.5e-4, weight_decay=1e-2, fused=True)
    x, c, y = batch(42)

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            pred = R.filmavit_forward(sd, x, c, patch_size=CFG["patch_size"], num_heads=CFG["num_heads"])
        loss = R.lp_loss(pred.float(), y)
        loss.backward()
        opt.step()
    return {"ms_per_step": round(time_steps(step, steps, warmup), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-eager", action="store_true")
    ap.add_argument("--attention-only", action="store_true")
    ap.add_argument("--step-only", action="store_true", help="only the native training step (for a kernel-trace profile of it)")
    a = ap.parse_args()
    out = {} if a.step_only else {"attention_bf16_d64_h6": attention(a.reps)}
    if not a.attention_only:
        out["native_step_16x512x512_p8"] = native(a.steps, a.warmup)
        if not (a.skip_eager or a.step_only):
            out["eager_bf16_autocast_step_16x512x512_p8"] = eager(a.steps, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
