"""Golden vectors for attention axes longer than 32 tokens, generated on the CPU from the reference implementation.

    python tools/gen_long_axes_golden.py [--reference /path/to/Bubbleformer]

writes
  tests/golden/relpos_tables_long.npz: the reference's T5 bucket tables and bias tensors (positional_encoding.py:50-172) at L = 48, 64,
      100, 128, as oracle/gen_golden.py writes them for L <= 40 (relpos_tables.npz);
  tests/golden/model_long_h36.npz: one FiLMAViT forward + loss + backward in fp64 at a long-axis shape (a 36 x 4 token grid, patch 4), in
      the layout of the model_*.npz files (oracle/gen_golden.py: run_variant), kept small by a single input / output field."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
if REPO not in sys.path:
    sys.path.insert(0, REPO)

LONG_TABLE_L = (48, 64, 100, 128)
# same fields as oracle/gen_golden.py VARIANTS; H = 36 tokens at patch 4 is the long axis
LONG_VARIANT = dict(model="filmavit", B=1, T=2, H=144, W=16, seed=17,
                    cfg=dict(input_fields=1, output_fields=1, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=1, num_fluid_params=4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="checkout of the reference implementation (default: oracle/gen_golden.py's)")
    args = ap.parse_args()
    from oracle import gen_golden
    if args.reference:
        gen_golden.REF = args.reference
    ref_models, ref_layers, LpLoss = gen_golden._import_reference()
    tabs = {}
    torch.manual_seed(5)
    rpb = ref_layers.RelativePositionBias(n_heads=3)
    tabs["emb"] = rpb.relative_attention_bias.weight.detach().numpy()
    for L in LONG_TABLE_L:
        ctx = torch.arange(L)[:, None]
        mem = torch.arange(L)[None, :]
        tabs[f"bucket_{L}"] = rpb._relative_position_bucket(mem - ctx, bidirectional=True, num_buckets=32).numpy()
        tabs[f"bias_{L}"] = rpb(L, L).detach().numpy()
    np.savez_compressed(os.path.join(GOLDEN, "relpos_tables_long.npz"), **tabs)
    np.savez_compressed(os.path.join(GOLDEN, "model_long_h36.npz"), **gen_golden.run_variant("long_h36", LONG_VARIANT, ref_models, LpLoss))
    print("wrote relpos_tables_long.npz, model_long_h36.npz")


if __name__ == "__main__":
    main()
