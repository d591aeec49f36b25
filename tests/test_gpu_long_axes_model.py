"""FiLMAViT / AViT with attention axes longer than 32 tokens (time windows and frame sides up to 128 tokens): the native model against
the oracle restatement run here and against the reference's fp64 golden, the bf16 mode against the fp32 mode, and the runtime paths
(bit-reproducible training step, graphed rollout, TrainStep, the 128-token limit)."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import rel_l2, structurally_zero

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name: model, B, T, pixel H, W, cfg.  Token grids: 12 x 10 at T = 40; 48 x 36; 128 x 4; 40 x 6 with d = 24; 128 x 128 (16384 tokens per
# frame: 512 x 512 at patch 4, the largest frame get_dims admits)
CASES = {
    "t40_12x10": ("filmavit", 1, 40, 48, 40, dict(input_fields=2, output_fields=2, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=1,
                                                   num_fluid_params=4)),
    "t3_48x36_avit": ("avit", 1, 3, 192, 144, dict(input_fields=2, output_fields=2, patch_size=4, embed_dim=64, num_heads=1, processor_blocks=1)),
    "t2_128x4": ("filmavit", 4, 2, 512, 16, dict(input_fields=2, output_fields=2, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=1,
                                                  num_fluid_params=4)),
    "t2_40x6_d24": ("filmavit", 2, 2, 320, 48, dict(input_fields=2, output_fields=2, patch_size=8, embed_dim=96, num_heads=4, processor_blocks=1,
                                                     num_fluid_params=4)),
    "t2_128x128": ("filmavit", 1, 2, 512, 512, dict(input_fields=2, output_fields=2, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=1,
                                                     num_fluid_params=4)),
}


def _data(model, B, T, H, Wd, cfg, seed):
    from oracle import weights as W
    x = W.synthetic_clip(B, T, cfg["input_fields"], H, Wd, seed + 1)
    y = W.synthetic_clip(B, T, cfg["output_fields"], H, Wd, seed + 2)
    c = W.synthetic_fluid_params(B, cfg["num_fluid_params"], seed + 3) if model == "filmavit" else None
    return x, y, c


def _native(model, T, cfg, sd, dtype, x, y, c, drop_path=0.0):
    from bubbleformer_amd.models import get_model
    m = get_model(model, time_window=T, drop_path=drop_path, compute_dtype=dtype, **cfg)
    m.load_state_dict(sd)
    m = m.cuda()
    xg = x.cuda().requires_grad_(True)
    args = (xg, c.cuda(), y.cuda()) if c is not None else (xg, y.cuda())
    loss, pred = m.forward_loss(*args)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss), pred.detach().float().cpu(), xg.grad.cpu(), {k: p.grad.cpu() for k, p in m.named_parameters()}


@pytest.mark.parametrize("name", list(CASES))
def test_long_axes_model_matches_oracle_and_bf16_tracks_fp32(name):
    from oracle import filmavit_ref as R, weights as W
    model, B, T, H, Wd, cfg = CASES[name]
    sd0 = W.generate(W.param_shapes(**cfg), seed=41)
    x0, y0, c0 = _data(model, B, T, H, Wd, cfg, 700)
    # oracle in fp64 on the same fp32 values
    sd = {k: v.double().requires_grad_(True) for k, v in sd0.items()}
    xo = x0.double().requires_grad_(True)
    kw = dict(patch_size=cfg["patch_size"], num_heads=cfg["num_heads"])
    pred_o = R.filmavit_forward(sd, xo, c0.double(), **kw) if model == "filmavit" else R.avit_forward(sd, xo, **kw)
    lo = R.lp_loss(pred_o, y0.double())
    lo.backward()
    l32, p32, dx32, g32 = _native(model, T, cfg, sd0, torch.float32, x0, y0, c0)
    assert abs(l32 - float(lo)) / abs(float(lo)) < 1e-4
    assert rel_l2(p32, pred_o.detach()) < 1e-4
    assert rel_l2(dx32, xo.grad) < 1e-4
    for k in g32:
        if not structurally_zero(k):
            assert rel_l2(g32[k], sd[k].grad) < 1e-4, k
    l16, _, dx16, g16 = _native(model, T, cfg, sd0, torch.bfloat16, x0, y0, c0)
    assert abs(l16 - l32) / abs(l32) < 3e-2
    assert rel_l2(dx16, dx32) < 8e-2
    num = sum(float((g16[k].double() - g32[k].double()).pow(2).sum()) for k in g32)
    den = sum(float(g32[k].double().pow(2).sum()) for k in g32)
    assert (num / den) ** 0.5 < 8e-2, (num / den) ** 0.5
    bad = []
    for k in g32:
        if structurally_zero(k):
            continue
        a, b = g32[k].double().flatten(), g16[k].double().flatten()
        cos = float((a @ b) / (a.norm() * b.norm()).clamp_min(1e-300))
        # the FiLM network's gradient is a sum of a few bf16-rounded per-token terms: 0.93, as test_gpu_parity.py holds it
        if cos < (0.93 if k.startswith("film_embed.") else 0.99):
            bad.append((k, round(cos, 4)))
    assert not bad, bad


def test_long_axes_model_matches_reference_golden():
    """tests/golden/model_long_h36.npz: the reference itself in fp64 (tools/gen_long_axes_golden.py) at a 36-token frame side."""
    from oracle import weights as W
    from tools.gen_long_axes_golden import LONG_VARIANT as spec
    z = np.load(os.path.join(GOLDEN, "model_long_h36.npz"))
    cfg = spec["cfg"]
    sd0 = W.generate(W.param_shapes(**cfg), seed=spec["seed"])
    x, y, c = (torch.from_numpy(z[k]) for k in ("x", "y", "cond"))
    loss, pred, dx, grads = _native(spec["model"], spec["T"], cfg, sd0, torch.float32, x, y, c)
    assert rel_l2(pred, z["pred_f64"]) < 1e-4
    assert abs(loss - float(z["loss_f64"])) / abs(float(z["loss_f64"])) < 1e-4
    assert rel_l2(dx, z["dx_f64"]) < 1e-4
    gscale = max(float(np.linalg.norm(z["grad/" + k])) for k in grads)
    for k, g in grads.items():
        if structurally_zero(k):
            assert float(g.norm()) < 1e-5 * gscale, k
        else:
            assert rel_l2(g, z["grad/" + k]) < 1e-4, k


def test_long_axes_bf16_training_step_is_bit_reproducible():
    """Stochastic depth on and the deferred two-queue backward the trainer uses, FiLMAViT-small at a 36-frame time window (16 x 192 x 192
    frames at patch 16, the geometry of test_gpu_baseline_configs.py: test_training_step_is_bit_reproducible_run_to_run): loss, dx and
    every parameter gradient equal bit for bit run to run."""
    from bubbleformer_amd import ops
    from bubbleformer_amd.models import get_model
    cfg = dict(input_fields=4, output_fields=4, patch_size=16, embed_dim=384, num_heads=6, processor_blocks=2, num_fluid_params=9)
    x0, y0, c0 = _data("filmavit", 1, 36, 192, 192, cfg, 900)

    def once():
        torch.manual_seed(5)
        m = get_model("filmavit", time_window=36, drop_path=0.2, compute_dtype=torch.bfloat16, **cfg).cuda().train()
        x = x0.cuda().requires_grad_(True)
        torch.manual_seed(9)
        ops.set_side_defer(True)
        try:
            loss, _ = m.forward_loss(x, c0.cuda(), y0.cuda())
            loss.backward()
        finally:
            ops.set_side_defer(False)
        torch.cuda.synchronize()
        return float(loss), x.grad.clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}

    l1, d1, g1 = once()
    l2, d2, g2 = once()
    assert l1 == l2 and torch.equal(d1, d2)
    differing = [k for k in g1 if not torch.equal(g1[k], g2[k])]
    assert not differing, differing


def test_long_axes_graphed_rollout_equals_eager():
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils.rollout import autoregressive_rollout
    from oracle import weights as W
    cfg = dict(input_fields=2, output_fields=2, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=1, num_fluid_params=4)
    m = get_model("filmavit", time_window=36, drop_path=0.0, compute_dtype=torch.bfloat16, **cfg)
    m.load_state_dict(W.generate(W.param_shapes(**cfg), seed=3))
    m = m.cuda().eval()
    x, _, c = _data("filmavit", 1, 36, 40, 144, cfg, 950)
    x0, c = x[0].cuda(), c.cuda()
    pg, _ = autoregressive_rollout(m, x0, 2, c, use_graph=True)
    pe, _ = autoregressive_rollout(m, x0, 2, c, use_graph=False)
    torch.cuda.synchronize()
    assert torch.isfinite(pe).all()
    assert torch.equal(pg, pe)


def test_long_axes_train_step_reduces_loss():
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.trainer import TrainStep
    from oracle import weights as W
    cfg = dict(input_fields=2, output_fields=2, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=1, num_fluid_params=4)
    m = get_model("filmavit", time_window=34, drop_path=0.0, compute_dtype=torch.bfloat16, **cfg)
    m.load_state_dict(W.generate(W.param_shapes(**cfg), seed=4))
    m = m.cuda()
    step = TrainStep(m, lr=1e-3)
    x, y, c = (t.cuda() for t in _data("filmavit", 1, 34, 160, 48, cfg, 970))
    losses = [float(step(x, c, y)) for _ in range(6)]
    assert losses[-1] < losses[0] and all(l == l for l in losses), losses


@pytest.mark.parametrize("axis", ["T", "H"])
def test_axis_of_129_tokens_is_refused(axis):
    from bubbleformer_amd import _lib as L
    from bubbleformer_amd.models import get_model
    cfg = dict(input_fields=1, output_fields=1, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=1, num_fluid_params=4)
    T, H = (129, 8) if axis == "T" else (2, 4 * 129)
    m = get_model("filmavit", time_window=T, drop_path=0.0, compute_dtype=torch.float32, **cfg).cuda()
    x, y, c = (t.cuda() for t in _data("filmavit", 1, T, H, 8, cfg, 990))
    with pytest.raises(L.BubbleformerHipError, match="limited to 128 tokens"):
        m.forward_loss(x, c, y)
