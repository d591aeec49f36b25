"""Golden vectors for the ClassicUnet baseline (unet_classic), generated on the CPU from the reference implementation in fp64.

    python tools/gen_unet_classic_golden.py --reference /path/to/Bubbleformer

writes tests/golden/unet_classic_<config>.npz, in training mode: input, target, prediction, loss and d loss / d input; every parameter
gradient, whole ("g:<name>") or as norm + projections ("n:" / "s:", tools/gen_unet_golden.py's sketch); every BatchNorm buffer after the
forward ("b:<name>").  Then the running statistics are set to seeded non-trivial values ("e:<name>") and the eval-mode prediction of the same
input is stored ("pred_eval").  The fp64 weights are not stored: ``weights(model, seed)`` regenerates them bit for bit.  Also writes
tests/golden/unet_classic_layout.json: the reference state_dict layout at T = 16, 4 fields, hidden 32."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools.gen_unet_golden import SKETCH_MIN, sketch  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")

# name -> model config and problem size; covers hidden 8 and 16, T*fields = 1 and 8, H != W, three frames
CONFIGS = {
    "h8_c1": dict(cfg=dict(time_window=1, input_fields=1, output_fields=1, hidden_channels=8), B=2, H=32, W=48, seed=1),
    "h16_c8": dict(cfg=dict(time_window=2, input_fields=4, output_fields=3, hidden_channels=16), B=2, H=32, W=32, seed=2),
    "h8_c8_b3": dict(cfg=dict(time_window=2, input_fields=4, output_fields=4, hidden_channels=8), B=3, H=16, W=32, seed=3),
}
SHIPPED = dict(time_window=16, input_fields=4, output_fields=4, hidden_channels=32)


def weights(model: torch.nn.Module, seed: int) -> dict:
    """Deterministic fp64 parameters (buffers excluded): convs ~ N(0, 1/fan_in) (a kernel-2 stride-2 transposed conv: fan_in = Cin);
    BatchNorm weight 1 + N(0, 0.1^2), bias N(0, 0.1^2); the final conv's bias N(0, 0.1^2)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, p in model.named_parameters():
        r = torch.randn(p.shape, generator=g, dtype=torch.float64)
        if ".norm" in k:
            out[k] = 1.0 + 0.1 * r if k.endswith("weight") else 0.1 * r
        elif k.endswith("weight"):
            out[k] = r / np.sqrt(p.shape[0] if k.startswith("upconv") else p[0].numel())
        else:
            out[k] = 0.1 * r
    return out


def eval_statistics(model: torch.nn.Module, seed: int) -> dict:
    """Seeded running statistics for the eval-mode check: mean N(0, 0.2^2), var 0.5 + U(0, 1), num_batches_tracked 7."""
    g = torch.Generator().manual_seed(1000 + seed)
    out = {}
    for k, b in model.named_buffers():
        if k.endswith("running_mean"):
            out[k] = 0.2 * torch.randn(b.shape, generator=g, dtype=torch.float64)
        elif k.endswith("running_var"):
            out[k] = 0.5 + torch.rand(b.shape, generator=g, dtype=torch.float64)
        else:
            out[k] = torch.tensor(7, dtype=torch.int64)
    return out


def inputs(spec: dict):
    cfg = spec["cfg"]
    g = torch.Generator().manual_seed(100 + spec["seed"])
    shape = (spec["B"], cfg["time_window"], cfg["input_fields"], spec["H"], spec["W"])
    oshape = (spec["B"], cfg["time_window"], cfg["output_fields"], spec["H"], spec["W"])
    return torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(oshape, generator=g, dtype=torch.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("BUBBLEFORMER_REF"), help="checkout of the reference Bubbleformer")
    args = ap.parse_args()
    import oracle.gen_golden as gg
    if args.reference:
        gg.REF = args.reference
    ref_models, _, LpLoss = gg._import_reference()
    loss_fn = LpLoss(d=2, p=2, reduce_dims=[0, 1, 2], reductions=["mean", "mean", "sum"])
    for name, spec in CONFIGS.items():
        m = ref_models.get_model("unet_classic", **spec["cfg"]).double().train()
        m.load_state_dict(weights(m, spec["seed"]), strict=False)
        x, y = inputs(spec)
        x.requires_grad_(True)
        pred = m(x)
        loss = loss_fn(pred, y)
        loss.backward()
        rec = {"x": x.detach().numpy(), "y": y.numpy(), "pred": pred.detach().numpy(), "loss": np.array(loss.item()), "dx": x.grad.numpy()}
        for k, p in m.named_parameters():
            if p.numel() <= SKETCH_MIN:
                rec["g:" + k] = p.grad.numpy()
            else:
                rec["n:" + k] = np.array(p.grad.norm().item())
                rec["s:" + k] = sketch(k, p.grad).numpy()
        for k, b in m.named_buffers():
            rec["b:" + k] = b.detach().numpy().copy()
        ev = eval_statistics(m, spec["seed"])
        m.load_state_dict(ev, strict=False)
        m.eval()
        with torch.no_grad():
            rec["pred_eval"] = m(x.detach()).numpy()
        for k, b in ev.items():
            rec["e:" + k] = b.numpy()
        path = os.path.join(GOLDEN, f"unet_classic_{name}.npz")
        np.savez_compressed(path, **rec)
        print(name, "params %d" % sum(p.numel() for p in m.parameters()), "loss %.6f" % loss.item(), "%d bytes" % os.path.getsize(path))
    with torch.device("meta"):
        m = ref_models.get_model("unet_classic", **SHIPPED)
    layout = {"config": SHIPPED, "class": type(m).__name__,
              "state_dict": [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()],
              "params": sum(p.numel() for p in m.parameters())}
    with open(os.path.join(GOLDEN, "unet_classic_layout.json"), "w") as f:
        json.dump(layout, f, indent=0)
    print("shipped config: %d parameters, %d state_dict entries" % (layout["params"], len(layout["state_dict"])))


if __name__ == "__main__":
    main()
