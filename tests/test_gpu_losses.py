"""GPU: utils.losses (csrc/losses.hip) -- `LpLoss` and the differentiable `eikonal_loss` against the reference's recorded fp64 results
(tests/golden/losses.npz) and against tests/losses_restatement.py in fp64 on the same fp32 inputs; the drop-in criterion against the fused
loss; a composite criterion against the oracle; TrainStep / fit with a criterion; graph capture.

Bounds come from the arithmetic, not from runs: inputs are fp32, every sum, coefficient and stencil is fp64 and each result is rounded once,
so a value is within a few fp32 ulps (6e-8 each) of the fp64 result of the same inputs and a gradient element within 2-3 ulps: 1e-6 for values
(largest relative error over the elements of the result) and for the relative L2 of gradients, whole and per row; 1e-5 where powf
(about 2 ulp per element) takes part."""
import os

import numpy as np
import pytest
import torch

from tests import losses_restatement as RS
from tests.helpers import load_variant, rel_l2, structurally_zero
from tools.gen_losses_golden import CONFIGS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAINING = dict(d=2, p=2, reduce_dims=[0, 1, 2], reductions=["mean", "mean", "sum"])
BENCH_SHAPE = (8, 16, 4, 192, 192)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "losses.npz")


def _randn(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, generator=g, device=DEV, dtype=torch.float32) * scale + shift


def _value_err(got, want):
    got, want = got.detach().double().cpu(), torch.as_tensor(want).double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(((got - want).abs() / want.abs()).max())


def _row_errs(got, want, d):
    """(relative L2 of the whole gradient, the largest relative L2 of one row's gradient)"""
    e, w = (got.detach().double() - want.double()).flatten(-d), want.double().flatten(-d)
    return float(e.norm() / w.norm()), float((e.norm(dim=-1) / w.norm(dim=-1)).max())


def _weight(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(DEV) + 0.5


def _native(pred, y, kw, w=None):
    from bubbleformer_amd.utils import LpLoss
    a = pred.detach().requires_grad_(True)
    val = LpLoss(**kw)(a, y)
    w = _weight(val.shape, 9) if w is None else w
    (val * w.float()).sum().backward()
    return val.detach(), a.grad, w


def _against_restatement(pred, y, kw, tol):
    val, grad, w = _native(pred, y, kw)
    a = pred.detach().double().requires_grad_(True)
    want = RS.lp_loss(a, y.double(), **kw)
    (want * w.float().double()).sum().backward()
    torch.cuda.synchronize()
    ve, (ge, gr) = _value_err(val, want.detach()), _row_errs(grad, a.grad, kw.get("d", 1))
    print(f"{tuple(pred.shape)} {kw}: value {ve:.2e}, gradient {ge:.2e} (worst row {gr:.2e})")
    assert grad.shape == pred.shape and torch.isfinite(grad).all()
    assert ve <= tol and ge <= tol and gr <= tol, (ve, ge, gr)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_fixture_parity(name):
    z = np.load(FIXTURE)
    kw, B = CONFIGS[name]
    tol = 1e-5 if kw.get("p", 2) == 2.5 else 1e-6
    pred, y = torch.from_numpy(z["pred"])[:B].to(DEV), torch.from_numpy(z["y"])[:B].to(DEV)
    val, grad, _ = _native(pred, y, kw, torch.from_numpy(z[f"{name}/weight"]).to(DEV))
    torch.cuda.synchronize()
    ve, ge = _value_err(val, z[f"{name}/value"]), rel_l2(grad.cpu(), z[f"{name}/dpred"])
    print(f"{name}: value {ve:.2e}, gradient {ge:.2e}")
    assert ve <= tol and ge <= tol, (ve, ge)


@pytest.mark.parametrize("shape,kw", [
    (BENCH_SHAPE, TRAINING),                                                                       # 512 rows of 36,864: long rows in spans
    (BENCH_SHAPE, dict(d=3, p=2, reduce_dims=[0, 1], reductions=["mean", "sum"])),                 # 128 rows of 147,456
    ((4, 5, 4, 512, 512), TRAINING),                                                               # the shipped data configs' clip
    (BENCH_SHAPE, dict(d=1, p=2, reduce_dims=[0, 1, 2, 3], reductions=["mean", "mean", "sum", "mean"])),      # 98,304 rows of 192: part of a wave each
    ((3, 5, 7, 13), dict(d=2, p=2, reduce_dims=[0], reductions="sum")),                            # n = 91: every row starts at another offset
    ((2, 3, 129, 131), dict(d=2, p=2, reduce_dims=None)),                                          # n = 16,899: odd long rows in two spans
    ((2, 3, 97, 131), dict(d=2, p=1, reduce_dims=[1], reductions="mean")),
    ((3, 5, 7, 13), dict(d=2, p=3, reduce_dims=None)),
    ((2, 3, 129, 131), dict(d=2, p=4, reduce_dims=[0, 1], reductions="mean")),
])
def test_regimes_against_restatement(shape, kw):
    _against_restatement(_randn(shape, 1), _randn(shape, 2, 1.5, 0.25), kw, 1e-6)


@pytest.mark.parametrize("shape,kw", [(BENCH_SHAPE, dict(TRAINING, p=2.5)), ((3, 5, 7, 13), dict(d=2, p=2.5, reduce_dims=None)),
                                      ((2, 3, 129, 131), dict(d=2, p=1.5, reduce_dims=[0], reductions="mean"))])
def test_generic_p_against_restatement(shape, kw):
    _against_restatement(_randn(shape, 3), _randn(shape, 4, 1.5, 0.25), kw, 1e-5)


@pytest.mark.parametrize("which", ["both", "prediction", "target"])
@pytest.mark.parametrize("shape,d", [((2, 4, 192, 192), 2), ((6, 16, 192), 1), ((3, 5, 7, 13), 2)])
def test_views_four_bytes_off_a_16_byte_boundary(which, shape, d):
    """Contiguous views one float into their storage: with both inputs at the same offset the kernels keep their 16-byte accesses behind a
    scalar head; with one of them alone they read scalars."""
    n = int(np.prod(shape))

    def make(seed, off, scale, shift):
        t = _randn((n + 4,), seed, scale, shift)[off:off + n].view(shape)
        assert t.is_contiguous() and t.data_ptr() % 16 == 4 * off
        return t
    pred = make(5, 1 if which in ("both", "prediction") else 0, 1.0, 0.0)
    y = make(6, 1 if which in ("both", "target") else 0, 1.5, 0.25)
    _against_restatement(pred, y, dict(d=d, p=2, reduce_dims=[0], reductions="mean"), 1e-6)


@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("shape,d", [((3, 4, 96, 96), 2), ((3, 4, 7, 13), 2)])
def test_edge_rows(p, shape, d):
    from bubbleformer_amd.utils import LpLoss
    y = _randn(shape, 8, 1.5, 0.25)
    pred = _randn(shape, 7)
    pred[1, 2] = y[1, 2]                     # a row without error
    y[2, 0] = 0.0                            # a target row of zeros
    a = pred.detach().requires_grad_(True)
    val = LpLoss(d=d, p=p, reduce_dims=None)(a, y)
    want = RS.lp_rows(pred.double(), y.double(), d, p)
    keep = torch.ones_like(val, dtype=torch.bool)
    keep[2, 0] = False
    (val * keep).sum().backward()            # the zero-target row's gradient is not finite by construction: keep it out of the sum
    torch.cuda.synchronize()
    assert float(val.detach()[1, 2]) == 0.0
    assert torch.isfinite(a.grad[1, 2]).all() and float(a.grad[1, 2].abs().max()) == 0.0
    assert not torch.isfinite(val[2, 0]) and not torch.isfinite(want[2, 0])
    keep[1, 2] = False
    assert _value_err(val[keep], want[keep]) <= 1e-6
    assert torch.isfinite(a.grad[keep]).all()


@pytest.mark.parametrize("kw", [TRAINING, dict(d=1, p=2, reduce_dims=[0, 1, 2, 3], reductions="mean"), dict(TRAINING, p=2.5)])
def test_two_calls_give_the_same_bits(kw):
    pred, y = _randn(BENCH_SHAPE, 10), _randn(BENCH_SHAPE, 11, 1.5, 0.25)
    (v1, g1, w), (v2, g2, _) = _native(pred, y, kw), _native(pred, y, kw)
    torch.cuda.synchronize()
    assert torch.equal(v1, v2) and torch.equal(g1, g2)


# ---------------------------------------------------------------------------------------------------------------- Eikonal
def _smooth_fields(shape, seed):
    """Seeded signed-distance-like fields in the reference's units (grid spacing 1/32): distance to a circle plus a gentle wave."""
    g = torch.Generator().manual_seed(seed)
    H, W = shape[-2:]
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    lead = shape[:-2]
    cy = torch.rand(lead, generator=g, dtype=torch.float64)[..., None, None] * H
    cx = torch.rand(lead, generator=g, dtype=torch.float64)[..., None, None] * W
    r = torch.rand(lead, generator=g, dtype=torch.float64)[..., None, None] * min(H, W) / 3
    phi = (torch.sqrt((yy - cy) ** 2 + (xx - cx) ** 2) - r) / 32 + 0.01 * torch.sin(0.3 * yy + cx) * torch.cos(0.2 * xx + cy)
    return phi.float().to(DEV)


def _eikonal_pair(phi):
    from bubbleformer_amd.utils import eikonal_loss, physics
    a = phi.detach().requires_grad_(True)
    val = eikonal_loss(a)
    (val * 1.75).backward()
    b = phi.detach().double().requires_grad_(True)
    want = RS.eikonal_loss(b)
    (want * 1.75).backward()
    torch.cuda.synchronize()
    assert val.shape == () and val.dtype == torch.float32 and torch.equal(val.detach(), physics.eikonal_loss(phi))
    return a.grad, b.grad


@pytest.mark.parametrize("case", ["fixture", "192x192", "H2", "W2", "2x2", "3x3"])
def test_eikonal_value_and_gradient(case):
    if case == "fixture":
        z = np.load(FIXTURE)
        phi = torch.from_numpy(z["phi"]).to(DEV)
    else:
        shape = {"192x192": (4, 4, 192, 192), "H2": (3, 2, 9), "W2": (3, 9, 2), "2x2": (5, 2, 2), "3x3": (2, 3, 3)}[case]
        phi = _smooth_fields(shape, 20)
    got, want = _eikonal_pair(phi)
    assert got.shape == phi.shape and torch.isfinite(got).all()
    err = rel_l2(got.cpu(), want.cpu())
    print(f"eikonal {case}: gradient {err:.2e}")
    assert err <= 1e-6, err
    if case == "fixture":
        assert rel_l2(got.cpu() / 1.75, z["eikonal/dphi"]) <= 1e-6          # the recorded gradient is that of the bare value


def test_eikonal_flat_patch_contributes_zero_where_autograd_gives_nan():
    phi = _smooth_fields((2, 32, 40), 21)
    phi[0, 10:18, 20:28] = 0.125
    got, want = _eikonal_pair(phi)
    nan = torch.isnan(want)
    inside = torch.zeros_like(nan)
    inside[0, 10:18, 20:28] = True
    assert 0 < int(nan.sum()) <= 64 and not bool((nan & ~inside).any())          # the mask cannot grow to hide a wrong kernel
    assert torch.isfinite(got).all()
    err = rel_l2(got[~nan].cpu(), want[~nan].cpu())
    print(f"eikonal flat patch: {int(nan.sum())} NaN cells in the oracle, gradient elsewhere {err:.2e}")
    assert err <= 1e-6, err


# ---------------------------------------------------------------------------------------------------------------- model + criterion
def _filmavit(name):
    from bubbleformer_amd.models import get_model
    from oracle import weights as W
    spec, z = load_variant(name)
    cfg = dict(spec["cfg"])
    model = get_model(spec["model"], time_window=spec["T"], drop_path=0.0, compute_dtype=torch.float32, **cfg)
    model.load_state_dict(W.generate(W.param_shapes(**cfg), seed=spec["seed"]))
    return spec, z, model.to(DEV)


def _compare_families(got, want, tol, label):
    """Every gradient family of `got` against `want` (relative L2; the structurally zero ones by the absolute bound of test_gpu_parity.py)."""
    gscale = max(float(v.double().norm()) for v in want.values())
    worst, bad = ("", 0.0), []
    for k, g in got.items():
        if structurally_zero(k):
            if float(g.double().norm()) > 1e-5 * gscale:
                bad.append((k, float(g.double().norm())))
            continue
        e = rel_l2(g.cpu(), want[k].cpu())
        worst = max(worst, (k, e), key=lambda kv: kv[1])
        if not e <= tol:
            bad.append((k, e))
    print(f"{label}: worst gradient family {worst[0]} {worst[1]:.2e}")
    assert not bad, bad


@pytest.mark.parametrize("name", ["tiny_d64", "tiny_d24", "tiny_p16"])
def test_dropin_criterion_equals_the_fused_loss(name):
    """LpLoss(training configuration)(model(x, c), y) against model.forward_loss(x, c, y): the same kernels in the same order, differing in
    how d(pred) is rounded.  Measured on the MI355X: loss equal to the bit (tiny_d64, tiny_d24) or 1.2e-7 (tiny_p16), dx 5.2e-7 .. 6.1e-7, worst
    gradient family 2.1e-6 (blocks.0.temporal.rel_pos_bias, tiny_p16); DESIGN.md section 13."""
    from bubbleformer_amd.utils import LpLoss
    out = []
    for fused in (True, False):
        spec, z, model = _filmavit(name)
        x = torch.from_numpy(z["x"]).to(DEV).requires_grad_(True)
        c, y = torch.from_numpy(z["cond"]).to(DEV), torch.from_numpy(z["y"]).to(DEV)
        loss = model.forward_loss(x, c, y)[0] if fused else LpLoss(**TRAINING)(model(x, c), y)
        loss.backward()
        torch.cuda.synchronize()
        out.append((float(loss.detach()), x.grad.clone(), {k: p.grad.clone() for k, p in model.named_parameters()}))
    (lf, dxf, gf), (lc, dxc, gc) = out
    print(f"{name}: loss fused {lf:.9g} criterion {lc:.9g} ({abs(lc - lf) / abs(lf):.2e}), dx {rel_l2(dxc.cpu(), dxf.cpu()):.2e}")
    assert abs(lc - lf) <= 1e-6 * abs(lf)
    assert rel_l2(dxc.cpu(), dxf.cpu()) <= 1e-4
    _compare_families(gc, gf, 1e-4, name)


def test_dropin_criterion_equals_the_fused_loss_unet_classic():
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils import LpLoss
    from tests import unet_classic_restatement as U
    spec, z, p = U.load_golden("h8_c8_b3")
    out = []
    for fused in (True, False):
        m = get_model("unet_classic", compute_dtype=torch.float32, **spec["cfg"])
        m.load_state_dict({k: v.float() for k, v in p.items()}, strict=False)
        m = m.to(DEV)
        x = torch.from_numpy(z["x"]).float().to(DEV).requires_grad_(True)
        y = torch.from_numpy(z["y"]).float().to(DEV)
        loss = m.forward_loss(x, y)[0] if fused else LpLoss(**TRAINING)(m(x), y)
        loss.backward()
        torch.cuda.synchronize()
        out.append((float(loss.detach()), x.grad.clone(), {k: q.grad.clone() for k, q in m.named_parameters()}))
    (lf, dxf, gf), (lc, dxc, gc) = out
    worst = max(((k, rel_l2(gc[k].cpu(), gf[k].cpu())) for k in gf), key=lambda kv: kv[1])
    print(f"unet_classic: loss {abs(lc - lf) / abs(lf):.2e}, dx {rel_l2(dxc.cpu(), dxf.cpu()):.2e}, worst gradient {worst[0]} {worst[1]:.2e}")
    assert abs(lc - lf) <= 1e-6 * abs(lf)
    assert rel_l2(dxc.cpu(), dxf.cpu()) <= 1e-4 and worst[1] <= 1e-4, worst


def test_composite_criterion_against_the_oracle():
    """model + (LpLoss + lambda * eikonal_loss of the de-normalised first channel) + backward in fp32 against the oracle in fp64 with the same
    loss.  lambda = 2e-3 balances the two terms' gradients w.r.t. the prediction (asserted from the oracle), so a dead Eikonal term cannot pass."""
    from bubbleformer_amd.utils import LpLoss, eikonal_loss
    from oracle import filmavit_ref as R, weights as W
    lam, div, diff = 2e-3, 1.98, 2.37
    spec, z, model = _filmavit("tiny_d64")
    cfg = spec["cfg"]
    sd = {k: v.double().requires_grad_(True) for k, v in W.generate(W.param_shapes(**cfg), seed=spec["seed"]).items()}
    xo = torch.from_numpy(z["x"]).double().requires_grad_(True)
    yo, co = torch.from_numpy(z["y"]).double(), torch.from_numpy(z["cond"]).double()
    pred_o = R.filmavit_forward(sd, xo, co, patch_size=cfg["patch_size"], num_heads=cfg["num_heads"], attn_scale=cfg.get("attn_scale", True),
                                feat_scale=cfg.get("feat_scale", True))
    pd = pred_o.detach().requires_grad_(True)
    g_lp, = torch.autograd.grad(R.lp_loss(pd, yo), pd)
    g_eik, = torch.autograd.grad(R.eikonal_loss(pd[:, :, 0] * div - diff), pd)
    ratio = lam * float(g_eik.norm()) / float(g_lp.norm())
    print(f"oracle: |grad lp| {float(g_lp.norm()):.3g}, |grad eik| {float(g_eik.norm()):.3g}, lambda-weighted ratio {ratio:.3g}")
    assert 0.1 <= ratio <= 10.0, ratio
    loss_o = R.lp_loss(pred_o, yo) + lam * R.eikonal_loss(pred_o[:, :, 0] * div - diff)
    loss_o.backward()

    lp = LpLoss(**TRAINING)
    x = torch.from_numpy(z["x"]).to(DEV).requires_grad_(True)
    pred = model(x, torch.from_numpy(z["cond"]).to(DEV))
    loss = lp(pred, torch.from_numpy(z["y"]).to(DEV)) + lam * eikonal_loss(pred[:, :, 0] * div - diff)
    loss.backward()
    torch.cuda.synchronize()
    le, de = abs(float(loss.detach()) - float(loss_o.detach())) / abs(float(loss_o.detach())), rel_l2(x.grad.cpu(), xo.grad)
    print(f"composite: loss {le:.2e}, dx {de:.2e}")
    assert le <= 1e-4 and de <= 1e-4
    _compare_families({k: p.grad for k, p in model.named_parameters()}, {k: v.grad for k, v in sd.items()}, 1e-4, "composite")


def test_train_step_with_criterion_equals_the_fused_step():
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils import LpLoss
    from bubbleformer_amd.utils.lr_schedulers import CosineWarmupLR
    got = []
    for criterion in (None, LpLoss(**TRAINING)):
        spec, z, model = _filmavit("tiny_d64")
        before = torch.cat([p.detach().flatten() for p in model.parameters()]).clone()
        sched = CosineWarmupLR(1e-3, 0, 20, 1e-6)          # no warm-up: the first step already has a learning rate
        kw = {} if criterion is None else dict(criterion=criterion)
        step = TrainStep(model, lr=1e-3, weight_decay=1e-2, optimizer="adamw", scheduler=sched, **kw)
        assert step.criterion is criterion
        lr0 = sched.get_last_lr()[0]
        loss = step(torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["cond"]).to(DEV), torch.from_numpy(z["y"]).to(DEV))
        torch.cuda.synchronize()
        after = torch.cat([p.detach().flatten() for p in model.parameters()])
        assert step.step_no == 1 and sched.get_last_lr()[0] != lr0 and not torch.equal(before, after)
        assert loss.shape == () and not loss.requires_grad
        got.append((float(loss), step.flat.grad.clone()))
    (lf, gf), (lc, gc) = got
    print(f"train step: loss {abs(lc - lf) / abs(lf):.2e}, flat gradient {rel_l2(gc.cpu(), gf.cpu()):.2e}")
    assert abs(lc - lf) <= 1e-6 * abs(lf)
    assert rel_l2(gc.cpu(), gf.cpu()) <= 1e-4


def test_fit_with_criterion_trains_and_validates_on_it():
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.fit import fit, validate
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils import LpLoss
    files = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samples", f"sample_{i}.hdf5") for i in (1, 2)]
    torch.manual_seed(0)
    model = get_model("avit", input_fields=4, output_fields=4, time_window=4, patch_size=8, embed_dim=64, num_heads=2, processor_blocks=2,
                      drop_path=0.0, compute_dtype=torch.float32).cuda()
    tr = BubbleForecast(files[:1], norm="std", time_window=4, start_time=5)
    consts = tr.normalize()
    va = BubbleForecast(files[1:], norm="std", time_window=4, start_time=5)
    va.normalize(*consts)
    calls = []

    def criterion(pred, y, lp=LpLoss(**TRAINING)):
        calls.append(pred.requires_grad)
        return lp(pred, y)
    h = fit(model, tr, va, batch_size=4, max_epochs=2, optimizer="adamw", lr=2e-3, weight_decay=1e-2, warmup_iters=2, eta_min=1e-6,
            limit_train_batches=3, limit_val_batches=2, seed=42, criterion=criterion)
    assert len(h["train_loss"]) == 6 and len(h["val_loss"]) == 2 and np.isfinite(h["train_loss"]).all() and np.isfinite(h["val_loss"]).all()
    assert calls == [True] * 3 + [False] * 2 + [True] * 3 + [False] * 2          # three training batches, two validation batches, twice
    assert h["epoch_train_loss"][1] < h["epoch_train_loss"][0]
    vstore = va.device_store(torch.device(DEV))
    again = validate(model, va, vstore, 4, 2, criterion=criterion)
    fused = validate(model, va, vstore, 4, 2)
    assert again == h["val_loss"][-1]
    assert abs(again - fused) <= 1e-6 * abs(fused), (again, fused)            # the training configuration IS the fused loss


def test_forward_and_backward_capture_into_a_graph():
    from bubbleformer_amd.utils import LpLoss, eikonal_loss
    shape = (2, 4, 4, 96, 96)
    lp = LpLoss(**TRAINING)
    inputs = [(_randn(shape, 30 + i), _randn(shape, 40 + i, 1.5, 0.25)) for i in range(2)]

    def run(pred, y):
        l1 = lp(pred, y)
        l2 = eikonal_loss(pred[:, :, 0].contiguous())
        g1, = torch.autograd.grad(l1, pred)
        g2, = torch.autograd.grad(l2, pred)
        return l1.detach(), l2.detach(), g1, g2
    eager = [tuple(t.clone() for t in run(p.clone().requires_grad_(True), y)) for p, y in inputs]
    sp, sy = inputs[0][0].clone().requires_grad_(True), inputs[0][1].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(sp, sy)
    for (p, y), want in zip(inputs, eager):
        with torch.no_grad():
            sp.copy_(p)
            sy.copy_(y)
        graph.replay()
        torch.cuda.synchronize()
        for got, w in zip(outs, want):
            assert torch.equal(got, w)
