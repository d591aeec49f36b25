"""Golden vectors for the ModernUnet baseline (unet_modern), generated on the CPU from the reference implementation in fp64.

    python tools/gen_unet_golden.py --reference /path/to/Bubbleformer

writes tests/golden/unet_modern_<config>.npz: input, target, prediction, loss and d loss / d input in fp64, and every parameter gradient
in fp64 -- whole ("g:<name>") up to SKETCH_MIN elements, above that as its norm ("n:<name>") and SKETCH_ROWS seeded Gaussian projections
("s:<name>", see ``sketch``), which keeps each file under 1 MB.  The fp64 weights are not stored: ``weights(model, seed)`` regenerates them
bit for bit. and tests/golden/unet_modern_layout.json (the reference state_dict layout of the shipped config, hidden 32, ch_mults [1, 2, 2, 4, 4],
at T = 16, 4 fields).  The loss is the reference's LpLoss(d=2, p=2, reduce_dims=[0, 1, 2], reductions=["mean", "mean", "sum"])
(modules.py:50)."""
import argparse
import json
import os
import sys
import zlib

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")

# name -> model config and problem size (kept small: the four files total a few MB)
CONFIGS = {
    "h16_m122": dict(cfg=dict(time_window=2, input_fields=4, output_fields=3, hidden_channels=16, ch_mults=[1, 2, 2], norm=True),
                     B=2, H=24, W=40, seed=1),
    "h16_m122_nonorm": dict(cfg=dict(time_window=2, input_fields=4, output_fields=3, hidden_channels=16, ch_mults=[1, 2, 2], norm=False),
                            B=2, H=24, W=40, seed=2),
    "h8_m12": dict(cfg=dict(time_window=2, input_fields=4, output_fields=3, hidden_channels=8, ch_mults=[1, 2], norm=True),
                   B=2, H=12, W=20, seed=3),
    "h8_m0": dict(cfg=dict(time_window=2, input_fields=4, output_fields=3, hidden_channels=8, ch_mults=[], norm=True),
                  B=2, H=6, W=10, seed=4),
}
SHIPPED = dict(time_window=16, input_fields=4, output_fields=4, hidden_channels=32, ch_mults=[1, 2, 2, 4, 4], norm=True)


def weights(model: torch.nn.Module, seed: int) -> dict:
    """Deterministic fp64 parameters: convs ~ N(0, 1/fan_in); GroupNorm weight 1 + N(0, 0.1^2), bias N(0, 0.1^2)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, p in model.state_dict().items():
        r = torch.randn(p.shape, generator=g, dtype=torch.float64)
        if ".norm" in k or k.startswith("norm"):
            out[k] = 1.0 + 0.1 * r if k.endswith("weight") else 0.1 * r
        elif k.endswith("weight"):
            fan_in = p[0].numel() if "up" not in k or p.dim() != 4 or p.shape[2] != 4 else p.shape[0] * 16
            out[k] = r / np.sqrt(fan_in)
        else:
            out[k] = 0.1 * r
    return out


SKETCH_MIN, SKETCH_ROWS = 4096, 16


def sketch(name: str, g: torch.Tensor) -> torch.Tensor:
    """SKETCH_ROWS projections of the flattened fp64 gradient onto N(0, 1/n) vectors drawn from a generator seeded by the parameter name:
    a wrong gradient (a wrong block of channels included) cannot keep all of them to 1e-12."""
    v = g.detach().double().flatten().cpu()
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    P = torch.randn(SKETCH_ROWS, v.numel(), generator=gen, dtype=torch.float64) / v.numel() ** 0.5
    return P @ v


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
    sys.path.insert(0, REPO)
    import oracle.gen_golden as gg
    if args.reference:
        gg.REF = args.reference
    ref_models, _, LpLoss = gg._import_reference()
    loss_fn = LpLoss(d=2, p=2, reduce_dims=[0, 1, 2], reductions=["mean", "mean", "sum"])
    for name, spec in CONFIGS.items():
        m = ref_models.get_model("unet_modern", **spec["cfg"]).double()
        w = weights(m, spec["seed"])
        m.load_state_dict(w)
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
        np.savez_compressed(os.path.join(GOLDEN, f"unet_modern_{name}.npz"), **rec)
        print(name, "params %d" % sum(p.numel() for p in m.parameters()), "loss %.6f" % loss.item())
    with torch.device("meta"):
        m = ref_models.get_model("unet_modern", **SHIPPED)
    layout = {"config": SHIPPED, "class": type(m).__name__,
              "state_dict": [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()],
              "params": sum(p.numel() for p in m.parameters())}
    with open(os.path.join(GOLDEN, "unet_modern_layout.json"), "w") as f:
        json.dump(layout, f, indent=0)
    print("shipped config: %d parameters" % layout["params"])


if __name__ == "__main__":
    main()
