"""GPU: the HIP FiLMAViT path (through the nn.Module API -> C ABI) against the oracle and the committed golden
vectors of the real reference: forward, loss, every parameter gradient and dx.

Stated tolerances (relative L2):
  fp32 mode : forward, loss, dx and each gradient family <= 1e-4   (the reference's own fp32-vs-fp64 floor is ~1e-6 / 3e-5)
  bf16 mode : forward <= 3e-2, dx <= 8e-2, ALL parameter gradients taken together <= 8e-2, each family <= 0.5
              (bf16 storage + bf16 MFMA, fp32 accumulate/statistics).  Yardstick: the oracle itself under stock
              torch.autocast(bfloat16) on these O(1)-perturbed tiny models is 1.3e-2..2.2e-2 off on the forward,
              3.8e-2..6.5e-2 on dx, 3e-2..5.6e-2 on the median gradient family and 6e-2..4.4e-1 on the worst one
              (measured in the build container; small-norm families such as FiLM's LayerNorm(9) are rounding-noise
              dominated), so the bf16 bounds are the precision of the format; the per-family 0.5 bound still catches a
              missing or mis-signed term (error >= 1).  The same code is held to 1e-4 in fp32 mode.
Structurally-zero gradients (knorm.bias, mlp.fc2.bias) are compared with an absolute bound.
"""
import numpy as np
import pytest
import torch

from tests.helpers import load_variant, oracle_run, rel_l2, structurally_zero

pytestmark = pytest.mark.gpu

NAMES = ["tiny_d64", "tiny_d24", "tiny_p16", "avit_plain"]
FWD_TOL = {torch.float32: 1e-4, torch.bfloat16: 3e-2}
GRAD_TOL = {torch.float32: 1e-4, torch.bfloat16: 8e-2}


def build_product_model(name, dtype):
    from bubbleformer_amd.models import get_model
    from oracle import weights as W
    spec, z = load_variant(name)
    cfg = dict(spec["cfg"])
    model = get_model(spec["model"], time_window=spec["T"], drop_path=0.0, compute_dtype=dtype, **cfg)
    shapes = W.param_shapes(**cfg)
    assert list(model.state_dict().keys()) == list(shapes.keys())
    model.load_state_dict(W.generate(shapes, seed=spec["seed"]))
    return spec, z, model.cuda()


def run_product(name, dtype, fused_loss):
    spec, z, model = build_product_model(name, dtype)
    x = torch.from_numpy(z["x"]).cuda().requires_grad_(True)
    y = torch.from_numpy(z["y"]).cuda()
    args = (x, torch.from_numpy(z["cond"]).cuda()) if spec["model"] == "filmavit" else (x,)
    if fused_loss:
        loss, pred = model.forward_loss(*args, y)
    else:
        pred = model(*args)
        num = ((pred - y) ** 2).sum(dim=(-1, -2)).sqrt()
        den = (y ** 2).sum(dim=(-1, -2)).sqrt()
        loss = (num / den).mean(0).mean(0).sum()
    loss.backward()
    grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters()}
    return z, pred.detach().cpu(), float(loss), x.grad.detach().cpu(), grads


@pytest.mark.parametrize("fused_loss", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", NAMES)
def test_model_matches_reference_golden(name, dtype, fused_loss):
    z, pred, loss, dx, grads = run_product(name, dtype, fused_loss)
    ft, gt = FWD_TOL[dtype], GRAD_TOL[dtype]
    assert rel_l2(pred, z["pred_f64"]) < ft
    assert abs(loss - float(z["loss_f64"])) / abs(float(z["loss_f64"])) < ft
    assert rel_l2(dx, z["dx_f64"]) < gt
    gscale = max(float(np.linalg.norm(z["grad/" + k])) for k in grads)
    bad = []
    fam_tol = gt if dtype == torch.float32 else 0.5
    num = den = 0.0
    for k, g in grads.items():
        ref = z["grad/" + k]
        num += float((g.double() - torch.from_numpy(ref).double()).pow(2).sum())
        den += float(torch.from_numpy(ref).double().pow(2).sum())
        if structurally_zero(k):
            if float(g.norm()) > (1e-5 if dtype == torch.float32 else 5e-3) * gscale:
                bad.append((k, float(g.norm())))
        else:
            e = rel_l2(g, ref)
            if not e < fam_tol:
                bad.append((k, e))
    assert not bad, bad
    assert (num / den) ** 0.5 < (1e-4 if dtype == torch.float32 else 8e-2), (num / den) ** 0.5


@pytest.mark.parametrize("name", NAMES)
def test_bf16_gradients_track_the_fp32_mode_per_family(name):
    """The throughput mode (bf16 activations, bf16 residual stream) against the parity mode of the SAME kernels on the same inputs:
    every parameter family must point the same way and have the same size -- cosine similarity > 0.99 and relative error < 0.25 per
    family (a mis-scaled or sign-flipped small family -- rel_pos_emb, attn_scale_factor, q/k-norm -- fails this even when its norm is
    tiny next to the projection weights').  Measured on the MI355X: cosine >= 0.9918, error <= 0.225 everywhere except the FiLM
    network of the E = 96 / 18-tokens-per-sample model, whose gradient is a sum of 18 bf16-rounded per-token terms (cosine 0.94-0.97,
    error 0.25-0.42): that family is held to 0.93 / 0.45."""
    _, _, _, dx32, g32 = run_product(name, torch.float32, True)
    _, _, _, dx16, g16 = run_product(name, torch.bfloat16, True)
    bad = []
    for k, a in g32.items():
        if structurally_zero(k):
            continue
        a, b = a.double().flatten(), g16[k].double().flatten()
        cos = float((a @ b) / (a.norm() * b.norm()).clamp_min(1e-300))
        err = float((a - b).norm() / a.norm().clamp_min(1e-300))
        film = k.startswith("film_embed.")
        if cos < (0.93 if film else 0.99) or err > (0.45 if film else 0.25):
            bad.append((k, a.numel(), round(cos, 4), round(err, 3)))
    assert not bad, bad
    a, b = dx32.double().flatten(), dx16.double().flatten()
    assert float((a @ b) / (a.norm() * b.norm())) > 0.995


def test_bf16_training_trajectory_tracks_the_fp32_mode():
    """Eight optimizer steps (fresh input each step, AdamW, cosine warm-up) in the throughput mode against the parity mode from the
    same initial weights: the loss sequences stay within 2 % of each other and the weights within 2 % per large tensor -- the bf16
    residual stream does not drift the optimisation (layer scales at the golden models' O(1) values)."""
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils import CosineWarmupLR
    from oracle import weights as W
    runs = {}
    for dt in (torch.float32, torch.bfloat16):
        spec, z, model = build_product_model("tiny_d64", dt)
        model.train()
        step = TrainStep(model, lr=1e-3, weight_decay=1e-2, scheduler=CosineWarmupLR(1e-3, 2, 20, 1e-6))
        cfg = spec["cfg"]
        losses = []
        for i in range(8):
            x = W.synthetic_clip(spec["B"], spec["T"], cfg["input_fields"], spec["H"], spec["W"], 1000 + i).cuda()
            y = W.synthetic_clip(spec["B"], spec["T"], cfg["output_fields"], spec["H"], spec["W"], 2000 + i).cuda()
            c = W.synthetic_fluid_params(spec["B"], cfg["num_fluid_params"], 3000 + i).cuda()
            losses.append(float(step(x, c, y)))
        runs[dt] = (losses, {k: p.detach().float().cpu().clone() for k, p in model.named_parameters()})
    l32, l16 = runs[torch.float32][0], runs[torch.bfloat16][0]
    assert max(abs(a - b) / abs(a) for a, b in zip(l32, l16)) < 2e-2, (l32, l16)
    for k, p in runs[torch.float32][1].items():
        if p.numel() >= 1024:
            assert rel_l2(runs[torch.bfloat16][1][k], p) < 2e-2, k


@pytest.mark.parametrize("name", ["tiny_d64", "tiny_p16"])
def test_model_matches_oracle_run_on_this_box(name):
    """Same check against the oracle executed here (fp32, CPU) rather than against stored vectors."""
    pred_o, loss_o, dx_o, grads_o = oracle_run(name, torch.float32)
    z, pred, loss, dx, grads = run_product(name, torch.float32, False)
    assert rel_l2(pred, pred_o) < 1e-4
    assert abs(loss - float(loss_o)) / abs(float(loss_o)) < 1e-4
    assert rel_l2(dx, dx_o) < 1e-4
    for k in grads:
        if not structurally_zero(k):
            assert rel_l2(grads[k], grads_o[k]) < 1e-4, k


def test_layer_api_shapes_like_reference_tests():
    """The reference's own shape tests (layers/tests/test_patching.py, models/tests/test_get_model.py) on the HIP path."""
    from bubbleformer_amd.layers import HMLPDebed, HMLPEmbed
    from bubbleformer_amd.models import get_model
    for patch, E in ((4, 192), (8, 384), (16, 192)):
        embed = HMLPEmbed(patch_size=patch, in_channels=4, embed_dim=E, compute_dtype=torch.float32).cuda()
        debed = HMLPDebed(patch_size=patch, out_channels=4, embed_dim=E).cuda()
        x = torch.randn(1, 4, 64, 64, device="cuda")
        y = embed(x)
        zz = debed(y)
        assert y.shape == (1, E, 64 // patch, 64 // patch) and zz.shape == x.shape
    for attn_scale in (True, False):
        for feat_scale in (True, False):
            m = get_model("avit", input_fields=2, output_fields=1, time_window=3, patch_size=8, embed_dim=192, num_heads=4,
                          processor_blocks=2, drop_path=0.0, attn_scale=attn_scale, feat_scale=feat_scale).cuda()
            out = m(torch.randn(2, 3, 2, 64, 64, device="cuda"))
            assert out.shape == (2, 3, 1, 64, 64) and torch.isfinite(out).all()


def test_fused_adamw_matches_torch():
    from bubbleformer_amd import ops
    g = torch.Generator(device="cuda").manual_seed(9)
    n = 10007
    p = torch.randn(n, device="cuda", generator=g)
    ref = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([ref], lr=2.5e-4, weight_decay=1e-2)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in range(1, 4):
        grad = torch.randn(n, device="cuda", generator=g)
        ref.grad = grad.clone()
        opt.step()
        ops.adamw_(p, grad, m, v, step, 2.5e-4)
        assert rel_l2(p.cpu(), ref.detach().cpu()) < 1e-6


def test_direct_gradient_mode_matches_autograd_mode():
    """trainer.TrainStep lets the kernels accumulate straight into the flat gradient buffer; same numbers as autograd."""
    from bubbleformer_amd import ops
    from bubbleformer_amd.trainer import FlatParams
    z, pred, loss, dx, grads = run_product("tiny_d64", torch.float32, True)
    spec, z, model = build_product_model("tiny_d64", torch.float32)
    flat = FlatParams(model)
    slots = {p.data_ptr(): p.grad for p in flat.params}
    seen = []
    ops.set_direct_grad_slots(slots, lambda ptrs: seen.extend(ptrs))
    try:
        x = torch.from_numpy(z["x"]).cuda()
        l2, _ = model.forward_loss(x, torch.from_numpy(z["cond"]).cuda(), torch.from_numpy(z["y"]).cuda())
        l2.backward()
    finally:
        ops.set_direct_grad_slots(None)
    assert sorted(seen) == sorted(slots)            # every parameter reported exactly once
    assert abs(float(l2) - loss) < 1e-6 * abs(loss)
    for (k, p) in model.named_parameters():
        if not structurally_zero(k):
            assert rel_l2(p.grad.cpu(), grads[k]) < 1e-5, k


def test_train_step_reduces_loss():
    from bubbleformer_amd.trainer import TrainStep
    spec, z, model = build_product_model("tiny_d64", torch.bfloat16)
    step = TrainStep(model, lr=1e-3)
    x = torch.from_numpy(z["x"]).cuda()
    c = torch.from_numpy(z["cond"]).cuda()
    y = torch.from_numpy(z["y"]).cuda()
    losses = [float(step(x, c, y)) for _ in range(8)]
    assert losses[-1] < losses[0] and all(l == l for l in losses), losses


@pytest.mark.parametrize("optimizer", ["adamw", "lion"])
def test_training_trajectory_matches_the_oracle_trained_with_torch(optimizer):
    """Eight optimizer steps end to end -- forward, fused loss, backward, fused AdamW / Lion, per-batch cosine warm-up -- in fp32
    against the oracle restatement in fp64 driven by torch.optim.AdamW / the restated Lion rule and the reference's scheduler
    formula, fresh input every step: the loss sequence agrees to 2e-4 and the parameters after the last step to 5e-3 (relative L2
    per tensor).  Adam and sign() turn the rounding noise of a structurally zero gradient into full-size steps, so the two all-zero
    families are skipped and the bound leaves room for the partly-zero ones (the value third of `input_head.bias`: a per-channel
    constant that the InstanceNorm after the attention removes) -- a wrong update direction in a tenth of a tensor would be 3e-2."""
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.lr_schedulers import CosineWarmupLR
    from oracle import filmavit_ref as R, weights as W
    spec, z, model = build_product_model("tiny_d64", torch.float32)
    cfg = spec["cfg"]
    steps, base_lr, wd = 8, (2e-3 if optimizer == "adamw" else 2e-4), 1e-2
    sched = CosineWarmupLR(base_lr, 3, steps, 1e-6)
    step = TrainStep(model, lr=base_lr, weight_decay=wd, optimizer=optimizer, scheduler=sched)
    sd = {k: v.double().requires_grad_(True) for k, v in W.generate(W.param_shapes(**cfg), seed=spec["seed"]).items()}
    opt = torch.optim.AdamW(list(sd.values()), lr=base_lr, weight_decay=wd) if optimizer == "adamw" else None
    mom = {k: torch.zeros_like(v) for k, v in sd.items()}
    kw = dict(patch_size=cfg["patch_size"], num_heads=cfg["num_heads"])
    got, want = [], []
    for i in range(steps):
        x = W.synthetic_clip(spec["B"], spec["T"], cfg["input_fields"], spec["H"], spec["W"], 400 + i)
        y = W.synthetic_clip(spec["B"], spec["T"], cfg["output_fields"], spec["H"], spec["W"], 500 + i)
        c = W.synthetic_fluid_params(spec["B"], cfg["num_fluid_params"], 600 + i)
        got.append(float(step(x.cuda(), c.cuda(), y.cuda())))
        lr = R.cosine_warmup_lr(i, base_lr, 3, steps, 1e-6)
        for v in sd.values():
            v.grad = None
        loss = R.lp_loss(R.filmavit_forward(sd, x.double(), c.double(), **kw), y.double())
        loss.backward()
        want.append(float(loss.detach()))
        with torch.no_grad():
            if optimizer == "adamw":
                for gp in opt.param_groups:
                    gp["lr"] = lr
                opt.step()
            else:
                for k, v in sd.items():
                    R.lion_step(v, v.grad, mom[k], lr, 0.9, 0.99, wd)
    assert np.allclose(got, want, rtol=2e-4), (got, want)
    torch.cuda.synchronize()
    for k, p_ in model.named_parameters():
        if not structurally_zero(k):
            assert rel_l2(p_.detach().cpu(), sd[k].detach()) < 5e-3, k


def test_long_axes_two_block_attention_paths():
    """T = 18, w = 20, h = 3: sequence lengths in (16, 32] take the two-block MFMA attention path in bf16 mode and ragged
    masking in both modes.  fp32 mode vs the oracle run here (1e-4); bf16 mode vs fp32 mode (bf16 bounds)."""
    from bubbleformer_amd.models import get_model
    from oracle import filmavit_ref as R, weights as W
    cfg = dict(input_fields=2, output_fields=2, patch_size=4, embed_dim=64, num_heads=1, processor_blocks=1, num_fluid_params=4)
    B, T, H, Wd = 1, 18, 12, 80
    shapes = W.param_shapes(**cfg)
    sd0 = W.generate(shapes, seed=21)
    x0 = W.synthetic_clip(B, T, 2, H, Wd, 501)
    y0 = W.synthetic_clip(B, T, 2, H, Wd, 502)
    c0 = W.synthetic_fluid_params(B, 4, 503)
    sd = {k: v.clone().requires_grad_(True) for k, v in sd0.items()}
    xo = x0.clone().requires_grad_(True)
    lo = R.lp_loss(R.filmavit_forward(sd, xo, c0, patch_size=4, num_heads=1), y0)
    lo.backward()
    res = {}
    for dt in (torch.float32, torch.bfloat16):
        m = get_model("filmavit", time_window=T, drop_path=0.0, compute_dtype=dt, **cfg)
        m.load_state_dict(sd0)
        m = m.cuda()
        xg = x0.cuda().requires_grad_(True)
        loss, pred = m.forward_loss(xg, c0.cuda(), y0.cuda())
        loss.backward()
        res[dt] = (float(loss), xg.grad.cpu(), {k: p.grad.cpu() for k, p in m.named_parameters()})
    l32, dx32, g32 = res[torch.float32]
    assert abs(l32 - float(lo)) / abs(float(lo)) < 1e-4
    assert rel_l2(dx32, xo.grad) < 1e-4
    for k in g32:
        if not structurally_zero(k):
            assert rel_l2(g32[k], sd[k].grad) < 1e-4, k
    l16, dx16, g16 = res[torch.bfloat16]
    assert abs(l16 - l32) / abs(l32) < 3e-2
    assert rel_l2(dx16, dx32) < 8e-2
    num = sum(float((g16[k].double() - g32[k].double()).pow(2).sum()) for k in g32)
    den = sum(float(g32[k].double().pow(2).sum()) for k in g32)
    assert (num / den) ** 0.5 < 8e-2, (num / den) ** 0.5
    for k in g32:
        if not structurally_zero(k):
            assert rel_l2(g16[k], g32[k]) < 0.5, k


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_stochastic_depth_with_explicit_masks(dtype):
    """DropPath (layers/attention.py:123,309,317): the same explicit per-sample factors through the HIP blocks and the oracle."""
    from bubbleformer_amd.models import get_model
    from oracle import filmavit_ref as R, weights as W
    cfg = dict(input_fields=2, output_fields=2, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=2, num_fluid_params=4)
    B, T, H, Wd = 3, 4, 8, 12
    shapes = W.param_shapes(**cfg)
    sd0 = W.generate(shapes, seed=31)
    x0 = W.synthetic_clip(B, T, 2, H, Wd, 601)
    y0 = W.synthetic_clip(B, T, 2, H, Wd, 602)
    c0 = W.synthetic_fluid_params(B, 4, 603)
    g = torch.Generator().manual_seed(5)
    keep = 0.6
    masks = [[(torch.rand(n, generator=g) < keep).float() / keep for n in (B, B * T, B * T)] for _ in range(2)]
    masks[0][0][0] = 0.0                      # make sure both outcomes occur
    masks[0][0][1] = 1.0 / keep
    # oracle, evaluated in fp64 on the same fp32 values: both sides of a 1e-4 comparison being fp32 would put the oracle's own
    # rounding (up to 3e-5 on cancellation-prone families such as FiLM's LayerNorm(4) bias) inside the tolerance
    od = torch.float64
    sd = {k: v.clone().to(od).requires_grad_(True) for k, v in sd0.items()}
    om = [[mm.to(od) for mm in ms] for ms in masks]
    t = R.embed(sd, "embed.", x0.to(od).reshape(B * T, 2, H, Wd), 4)
    h, w, E = t.shape[1], t.shape[2], t.shape[3]
    t = R.film(sd, "film_embed.", t.reshape(B, T, h, w, E), c0.to(od))
    for i in range(2):
        t = R.temporal_block(sd, f"blocks.{i}.temporal.", t, 2, True, om[i][0])
        t = R.spatial_block(sd, f"blocks.{i}.spatial.", t.reshape(B * T, h, w, E), 2, True, True, om[i][1], om[i][2]).reshape(B, T, h, w, E)
    lo = R.lp_loss(R.debed(sd, "debed.", t.reshape(B * T, h, w, E), 4).reshape(B, T, 2, H, Wd), y0.to(od))
    lo.backward()
    # HIP
    m = get_model("filmavit", time_window=T, drop_path=0.4, compute_dtype=dtype, **cfg)
    m.load_state_dict(sd0)
    m = m.cuda().train()
    tok = m.embed.tokens(x0.cuda(), c0.cuda(), m.film_embed.film_params(), compute_dtype=dtype)
    for i, blk in enumerate(m.blocks):
        tok = blk.temporal.forward_tokens(tok, masks[i][0].cuda())
        tok = blk.spatial.forward_tokens(tok, masks[i][1].cuda(), masks[i][2].cuda())
    loss, _ = m.debed.loss_from_tokens(tok, y0.cuda())
    loss.backward()
    ft, gt = (1e-4, 1e-4) if dtype == torch.float32 else (3e-2, 8e-2)
    assert abs(float(loss) - float(lo)) / abs(float(lo)) < ft
    num = den = 0.0
    for k, p in m.named_parameters():
        ref = sd[k].grad
        num += float((p.grad.cpu().double() - ref.double()).pow(2).sum())
        den += float(ref.double().pow(2).sum())
        if not structurally_zero(k):
            assert rel_l2(p.grad.cpu(), ref) < (gt if dtype == torch.float32 else 0.5), k
    assert (num / den) ** 0.5 < gt


def test_training_mode_draws_masks_and_eval_is_deterministic():
    spec, z, model = build_product_model("tiny_d64", torch.float32)
    for blk in model.blocks:        # the golden models are built with drop_path = 0: give block 1 a rate as the reference's linspace would
        pass
    from bubbleformer_amd.layers.attention import DropPath
    model.blocks[1].temporal.drop_path = DropPath(0.5)
    model.blocks[1].spatial.drop_path = DropPath(0.5)
    x = torch.from_numpy(z["x"]).cuda()
    c = torch.from_numpy(z["cond"]).cuda()
    model.eval()
    a = model(x, c)
    assert rel_l2(a.cpu(), z["pred_f64"]) < 1e-4            # identity in eval mode
    model.train()
    torch.manual_seed(0)
    outs = [model(x, c) for _ in range(4)]
    assert any(rel_l2(o.cpu(), a.cpu()) > 1e-3 for o in outs)   # masks are active in training mode


def test_batched_stage_preparation_is_bit_identical(monkeypatch):
    """bf_prep_stages (all trunk stages' bf16 weight copies, out-projection folds and stochastic-depth tables in one launch per 12
    stages) against the per-stage preparation launches it replaces: same prediction bit for bit in eval and in training mode under a
    fixed seed, same loss, and the prepared records are consumed (nothing left for a later call).  Both arms take the per-stage Python
    path (BF_TRUNK_NATIVE=0): the native trunk call always prepares in batches, so only there does BF_PREP_AHEAD choose between the two
    preparations.  The training-mode run also takes the backward: the operands only it reads (the alpha-scaled out-projection weight,
    the transposed fc2 copy, the stochastic-depth table) are compared through every parameter gradient -- the slab-summed weight
    gradients bit for bit, the rest within four times what two identical runs differ by (the convention of
    test_native_trunk_call_and_folded_slab_sums_change_no_bit)."""
    from bubbleformer_amd import ops
    spec, z, model = build_product_model("tiny_d64", torch.bfloat16)
    from bubbleformer_amd.layers.attention import DropPath
    for blk in model.blocks:
        blk.temporal.drop_path = DropPath(0.3)
        blk.spatial.drop_path = DropPath(0.3)
    x = torch.from_numpy(z["x"]).cuda()
    c = torch.from_numpy(z["cond"]).cuda()
    y = torch.from_numpy(z["y"]).cuda()

    def run(train):
        model.train(train)
        torch.manual_seed(5)
        loss, pred = model.forward_loss(x, c, y)
        assert not ops._LINKS.prepared
        grads = None
        if train:
            model.zero_grad(set_to_none=True)
            loss.backward()
            torch.cuda.synchronize()
            grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        return float(loss), pred.clone(), grads

    monkeypatch.setenv("BF_TRUNK_NATIVE", "0")
    got = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("BF_PREP_AHEAD", mode)
        got[mode] = (run(False), run(True))
    again = run(True)[2]                             # BF_PREP_AHEAD=0 once more: what two identical runs differ by
    for a, b in zip(got["1"], got["0"]):
        assert a[0] == b[0] and torch.equal(a[1], b[1])
    assert got["1"][0][0] != got["1"][1][0]          # the training-mode run really dropped something
    g1, g0 = got["1"][1][2], got["0"][1][2]
    exact = ("input_head.weight", "input_head.bias", "output_head.weight", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
    noise = max(float((g0[k] - again[k]).abs().max()) for k in g0)
    print("run-to-run noise of the parameter gradients: %.3e" % noise)
    assert set(g1) == set(g0) and any(k.startswith("blocks.") and k.endswith(exact) for k in g0)
    for k in g0:
        if k.startswith("blocks.") and k.endswith(exact):
            assert torch.equal(g1[k], g0[k]), k
        else:
            diff = float((g1[k] - g0[k]).abs().max())
            assert diff <= max(noise, 1e-30) * 4 + 1e-12, (k, diff, noise)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bias_type_none_equals_a_zero_table(dtype):
    """bias_type="none" (layers/attention.py:58-59,174-175 of the reference: no bias term): the blocks built that way give what the
    default blocks give with an all-zero embedding table -- which adds exactly 0 to every score -- forward and every gradient; the
    fp32 oracle (zero table) bounds both."""
    from bubbleformer_amd.layers import AttentionBlock, AxialAttentionBlock
    from bubbleformer_amd import ops
    torch.manual_seed(5)
    E, heads = 128, 2
    for cls, shape in ((AttentionBlock, (2, 6, 4, 6, E)), (AxialAttentionBlock, (2, 3, 12, 8, E))):
        rel = cls(E, heads, layer_scale_init_value=0.5).cuda()
        with torch.no_grad():
            for p in rel.parameters():
                p.add_(0.05 * torch.randn_like(p))
            rel.rel_pos_bias.relative_attention_bias.weight.zero_()
        none = cls(E, heads, layer_scale_init_value=0.5, bias_type="none").cuda()
        none.load_state_dict({k: v for k, v in rel.state_dict().items() if "rel_pos_bias" not in k})
        outs = []
        for blk in (rel, none):
            tok = torch.randn(*shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9)).to(dtype).requires_grad_(True)
            out = blk.forward_tokens(tok)
            out.float().square().mean().backward()
            outs.append((out.detach(), tok.grad.detach(), {k: p.grad.detach().clone() for k, p in blk.named_parameters() if "rel_pos_bias" not in k}))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        for k, g in outs[0][2].items():
            if k.endswith("knorm.bias"):      # structurally zero (softmax is shift invariant): rounding noise around 0, summed by float atomics in arrival order
                assert float((outs[1][2][k] - g).abs().max()) < 1e-3 * float(outs[0][2][k.replace("knorm.bias", "knorm.weight")].abs().max()), k
                continue
            assert rel_l2(outs[1][2][k], g) < 1e-5 or float(g.abs().max()) < 1e-9, k


def _stock_init_run(dtype, steps, lr, seed=0, blocks=4, T=8, size=96, batch=2):
    """FiLMAViT with the reference's OWN initialisation (torch defaults per layer type; every layer scale at 1e-6,
    layers/attention.py:30,142) trained for `steps` AdamW steps on fresh synthetic clips; returns the loss sequence, the layer-scale
    vectors (12 branches x 384 channels) after every step and the final parameters."""
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils import CosineWarmupLR
    from oracle import weights as W
    torch.manual_seed(seed)
    cfg = dict(input_fields=4, output_fields=4, patch_size=16, embed_dim=384, num_heads=6, processor_blocks=blocks, num_fluid_params=9)
    model = get_model("filmavit", time_window=T, drop_path=0.0, compute_dtype=dtype, **cfg).cuda().train()
    step = TrainStep(model, lr=lr, weight_decay=1e-2, scheduler=CosineWarmupLR(lr, 5, 200, 1e-6))
    gam = [p for k, p in model.named_parameters() if "gamma" in k]
    losses, traj = [], []
    for i in range(steps):
        x = W.synthetic_clip(batch, T, 4, size, size, 5000 + i).cuda()
        y = W.synthetic_clip(batch, T, 4, size, size, 6000 + i).cuda()
        c = W.synthetic_fluid_params(batch, 9, 7000 + i).cuda()
        losses.append(float(step(x, c, y)))
        traj.append(torch.stack([g.detach().float().flatten() for g in gam]).cpu())
    return losses, torch.stack(traj), {k: p.detach().float().cpu().clone() for k, p in model.named_parameters()}


def test_bf16_training_through_the_layer_scale_dead_zone():
    """The same comparison over 200 steps at lr 3e-3, which takes the layer scales from the stock 1e-6 THROUGH the range where a bf16
    residual stream rounds `gamma * branch` away (below 2^-9 of the stream) and out of it (measured: mean |gamma| 1.6e-2, max 6.7e-2 at
    the end).  If the forward's blindness to small branches mattered for training, the two modes would part here.  Stated bounds: every
    loss within 1 % of the fp32 run's (measured: 0.15 % at worst), every branch's layer-scale vector within 15 % relative L2 at every
    step (measured: 8.9 % at worst, at the end)."""
    l32, g32, _ = _stock_init_run(torch.float32, 200, 3e-3)
    l16, g16, _ = _stock_init_run(torch.bfloat16, 200, 3e-3)
    dev = max(abs(a - b) / abs(a) for a, b in zip(l32, l16))
    rel = (g16[10:] - g32[10:]).norm(dim=2) / g32[10:].norm(dim=2)
    print("loss deviation", round(dev, 5), "gamma: mean |.|", float(g32[-1].abs().mean()), "max", float(g32[-1].abs().max()), "worst rel L2", round(float(rel.max()), 3))
    assert float(g32[-1].abs().mean()) > 5e-3          # the scales really crossed the range
    assert dev < 1e-2 and float(rel.max()) < 0.15, (dev, float(rel.max()))


def test_bf16_training_from_stock_init_tracks_the_fp32_mode():
    """The throughput mode from the reference's stock initialisation, where every branch enters the residual stream through a layer scale
    of 1e-6 (layers/attention.py:30,142): 40 AdamW steps (warm-up 5, lr 1e-3, so that the scales grow by two to three decades inside the
    test) in bf16 against the same kernels in the fp32 parity mode, same seeds and data.  Stated bounds: every loss within 1 % of the
    fp32 run's (measured 0.1 %); from step 10 on (the scales have left their 1e-6 start) each branch's layer-scale VECTOR (384
    channels) within 15 % of the fp32 run's in relative L2 and with cosine similarity > 0.99 (measured: worst 6.3 %, 0.998) -- the
    per-channel scales follow the same trajectories although their gradients are sums of bf16-rounded products -- and the final large
    weight tensors within 5 % (measured: worst 2.05 %).  (The mean over a branch's channels is not a usable yardstick: it crosses zero
    during the run.)  What this does NOT show, and DESIGN.md section 2 states: the residual stream is bf16, so while gamma * branch stays
    under 2^-9 of the stream the forward does not see that branch at all (stock autocast keeps the stream in fp32); the scales still
    learn because their gradient does not pass through the rounded sum."""
    l32, g32, w32 = _stock_init_run(torch.float32, 40, 1e-3)
    l16, g16, w16 = _stock_init_run(torch.bfloat16, 40, 1e-3)
    print("losses fp32", [round(v, 4) for v in l32[::5]], "bf16", [round(v, 4) for v in l16[::5]])
    assert max(abs(a - b) / abs(a) for a, b in zip(l32, l16)) < 1e-2, (l32, l16)
    assert float(g32[-1].abs().mean(1).min()) > 2e-5                  # every branch's scales have left the 1e-6 start by a factor of 20 at least
    rel = (g16[10:] - g32[10:]).norm(dim=2) / g32[10:].norm(dim=2)          # [step][branch]
    cos = torch.nn.functional.cosine_similarity(g16[10:], g32[10:], dim=2)
    print("gamma vectors: rel L2 at the end", [round(float(v), 3) for v in rel[-1]], "worst over steps", round(float(rel.max()), 3),
          "min cosine", round(float(cos.min()), 4))
    assert float(rel.max()) < 0.15 and float(cos.min()) > 0.99, (rel.max(), cos.min())
    worst = max((rel_l2(w16[k], p), k) for k, p in w32.items() if p.numel() >= 4096)
    print("worst large weight tensor", worst)
    assert worst[0] < 5e-2, worst


def test_bf16_training_from_stock_init_at_full_depth_and_bench_geometry():
    """The same comparison where the bench runs: FiLMAViT-small at its full 12 blocks on 16 x 192 x 192 clips (batch 2: the fp32 mode's
    memory), stock initialisation, 30 AdamW steps at lr 1e-3 -- the bf16 residual stream now carries 36 branches, three times the depth
    of the test above.  Stated bounds: every loss within 1 % of the fp32 run's (measured 0.21 %), every layer-scale vector from step 10 on
    within 20 % relative L2 and cosine > 0.98 (measured: worst 9.9 %, 0.995), the final large weight tensors within 5 % (worst 3.9 %,
    blocks.11.spatial.output_head.weight)."""
    kw = dict(blocks=12, T=16, size=192, batch=2)
    l32, g32, w32 = _stock_init_run(torch.float32, 30, 1e-3, **kw)
    l16, g16, w16 = _stock_init_run(torch.bfloat16, 30, 1e-3, **kw)
    dev = max(abs(a - b) / abs(a) for a, b in zip(l32, l16))
    rel = (g16[10:] - g32[10:]).norm(dim=2) / g32[10:].norm(dim=2)
    cos = torch.nn.functional.cosine_similarity(g16[10:], g32[10:], dim=2)
    worst = max((rel_l2(w16[k], p), k) for k, p in w32.items() if p.numel() >= 4096)
    print("losses fp32", [round(v, 4) for v in l32[::5]], "bf16", [round(v, 4) for v in l16[::5]], "worst deviation", round(dev, 5))
    print("gamma vectors (36): worst rel L2", round(float(rel.max()), 3), "min cosine", round(float(cos.min()), 4), "worst large weight", worst)
    assert dev < 1e-2, dev
    assert float(rel.max()) < 0.2 and float(cos.min()) > 0.98, (rel.max(), cos.min())
    assert worst[0] < 5e-2, worst
