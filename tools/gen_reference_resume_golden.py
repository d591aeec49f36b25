"""Golden checkpoints for resuming a reference training run natively, generated on the CPU from the reference implementation.

    python tools/gen_reference_resume_golden.py [--reference /path/to/Bubbleformer]

writes tests/golden/reference_resume_{adamw,adam}.pt (torch.load(..., weights_only=True) loads them), each holding
  "checkpoint":   a tiny reference FiLMAViT trained 3 steps in fp32 by torch.optim.AdamW / Adam and the reference's CosineWarmupLR
                  (utils/lr_schedulers.py:4-31), stepped per batch as modules.py:132-171 configures them, in the Lightning layout
                  ("model."-prefixed state_dict, optimizer_states, lr_schedulers, global_step, epoch, hyper_parameters as plain dicts);
  "param_names":  the reference's parameter names in optimizer order (`model.parameters()`, modules.py:136-138);
  "batches":      the seeded (x, cond, y) batches of steps 4 and 5;
  "lrs":          the learning rate of steps 4 and 5 and the one after them, from a reference optimizer and scheduler that were
                  rebuilt and given the checkpoint through their own load_state_dict (what a Lightning resume does);
  "params_after": the parameters after those 2 continued reference steps;
  "spec":         model config, batch geometry and the optimizer / scheduler settings."""
import argparse
import copy
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SPEC = dict(B=2, T=2, H=16, W=16, seed=23,
            cfg=dict(input_fields=1, output_fields=1, patch_size=4, embed_dim=32, num_heads=1, processor_blocks=1, num_fluid_params=2),
            warmup_iters=2, max_iters=8, eta_min=1e-6, steps_before=3, steps_after=2)
OPTIM = {"adamw": dict(lr=1e-3, weight_decay=1e-2), "adam": dict(lr=1e-3, weight_decay=1e-5)}


def batch(i):
    from oracle import weights as W
    s, c = SPEC, SPEC["cfg"]
    return (W.synthetic_clip(s["B"], s["T"], c["input_fields"], s["H"], s["W"], 700 + i),
            W.synthetic_fluid_params(s["B"], c["num_fluid_params"], 900 + i),
            W.synthetic_clip(s["B"], s["T"], c["output_fields"], s["H"], s["W"], 800 + i))


def build(ref_models, name, CosineWarmupLR):
    torch.manual_seed(0)
    model = ref_models.get_model("filmavit", time_window=SPEC["T"], drop_path=0.0, **SPEC["cfg"])
    opt_cls = torch.optim.AdamW if name == "adamw" else torch.optim.Adam
    opt = opt_cls(model.parameters(), **OPTIM[name])                    # modules.py:135-138
    sched = CosineWarmupLR(opt, warmup_iters=SPEC["warmup_iters"], max_iters=SPEC["max_iters"], eta_min=SPEC["eta_min"])
    return model, opt, sched


def train_step(model, opt, sched, crit, i):
    x, c, y = batch(i)
    opt.zero_grad()
    crit(model(x, c), y).backward()
    opt.step()
    sched.step()                                                         # interval="step" (modules.py:164-171)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="checkout of the reference implementation (default: oracle/gen_golden.py's)")
    args = ap.parse_args()
    from oracle import gen_golden, weights as W
    if args.reference:
        gen_golden.REF = args.reference
    ref_models, _, LpLoss = gen_golden._import_reference()
    from bubbleformer.utils.lr_schedulers import CosineWarmupLR
    crit = LpLoss(d=2, p=2, reduce_dims=[0, 1, 2], reductions=["mean", "mean", "sum"])       # modules.py:50
    for name in OPTIM:
        model, opt, sched = build(ref_models, name, CosineWarmupLR)
        model.load_state_dict(W.generate(W.param_shapes(**SPEC["cfg"]), seed=SPEC["seed"]))
        for i in range(SPEC["steps_before"]):
            train_step(model, opt, sched, crit, i)
        n = SPEC["steps_before"]
        ckpt = {"epoch": 0, "global_step": n,
                "state_dict": {"model." + k: v.detach().clone() for k, v in model.state_dict().items()},
                "optimizer_states": [copy.deepcopy(opt.state_dict())],
                "lr_schedulers": [copy.deepcopy(sched.state_dict())],
                "hyper_parameters": {"optim_cfg": {"name": name, "params": dict(OPTIM[name])},
                                     "scheduler_cfg": {"name": "cosine_warmup",
                                                       "params": {"warmup_iters": SPEC["warmup_iters"], "eta_min": SPEC["eta_min"]}}}}
        # continue as a Lightning resume does: fresh module, optimizer and scheduler, each given the checkpoint by load_state_dict
        model2, opt2, sched2 = build(ref_models, name, CosineWarmupLR)
        model2.load_state_dict({k[len("model."):]: v for k, v in ckpt["state_dict"].items()})
        opt2.load_state_dict(copy.deepcopy(ckpt["optimizer_states"][0]))
        sched2.load_state_dict(copy.deepcopy(ckpt["lr_schedulers"][0]))
        lrs = []
        for i in range(n, n + SPEC["steps_after"]):
            lrs.append(float(opt2.param_groups[0]["lr"]))
            train_step(model2, opt2, sched2, crit, i)
        lrs.append(float(opt2.param_groups[0]["lr"]))
        out = {"checkpoint": ckpt, "param_names": [k for k, _ in model2.named_parameters()],
               "batches": [dict(zip(("x", "cond", "y"), batch(i))) for i in range(n, n + SPEC["steps_after"])],
               "lrs": lrs, "params_after": {k: p.detach().clone() for k, p in model2.named_parameters()},
               "spec": dict(SPEC, optim=dict(OPTIM[name]))}
        path = os.path.join(GOLDEN, f"reference_resume_{name}.pt")
        torch.save(out, path)
        torch.load(path, weights_only=True)
        print("wrote", path, os.path.getsize(path), "bytes, lrs", lrs)


if __name__ == "__main__":
    main()
