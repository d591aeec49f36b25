"""GPU: utils.losses.SpectralLpLoss (csrc/spectral_loss.hip: bf_slp_fwd / bf_slp_bwd) against tests/spectral_loss_restatement.py in fp64 on the
same fp32 inputs; w = 1 against the native LpLoss; views off a 16-byte boundary; edge rows; bits; graph capture; refusals; the model, TrainStep
and fit with it.

Bounds come from the arithmetic (spectral_loss_restatement.eta / sum_bound / bounds): the transforms are fp32, so a transformed field is
within eta ||x|| of the exact one, eta = (8 max(1, log2(H W)) + P(H) + P(W)) 2^-24; carried through the weighted sum of squares that is
|S - want| <= 2 eta sqrt(want w_max sum x^2) + eta^2 w_max sum x^2, through the quotient and the root the sum of the two relative bounds, through
the filtered inverse 2 eta w_max ||E|| / ||w E|| plus the coefficient's share.  The bounds are not widened to fit; each test prints the worst
ratio of error to bound of its shape.

Inputs (spectral_loss_restatement.make_inputs / weights / field_weights): on every row of a shape with both sides > 2 the restatement gives
S_e(w) / S_e(1) >= 2, S_y(w) / S_y(1) >= 1.25 and a gradient that differs from the one at w = 1 by >= 0.3 relative L2 (asserted here and, on
the CPU, in tests/test_spectral_loss.py), so a dead weight cannot pass."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import spectral_loss_restatement as SR
from tests.errors_restatement import shell_count
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAINING = dict(d=2, p=2, reduce_dims=[0, 1, 2], reductions=["mean", "mean", "sum"])
SCALE = 1.75


@functools.lru_cache(maxsize=None)
def _case(shape):
    """The inputs of a shape on the device and what the restatement gives for them in fp64: computed once, shared, never changed."""
    pred, y = (t.to(DEV) for t in SR.make_inputs(shape))
    w, a = SR.weights(shape[2], shell_count(*shape[-2:])).to(DEV), SR.field_weights(shape[2])
    return (pred, y, w, a) + _restated(pred, y, w, a)


def _restated(pred, y, w, a):
    """fp64 on the device: (loss, field terms, plain terms, S_e, S_y, gradient of SCALE * loss)"""
    p, t = pred.detach().double().requires_grad_(True), y.double()
    terms = SR.field_terms(p, t, w, a)
    grad, = torch.autograd.grad(terms.sum() * SCALE, p)
    se, sy = SR.row_sums(p.detach(), t, w)
    return terms.sum().detach(), terms.detach(), SR.field_terms(p.detach(), t, torch.ones_like(w), a), se, sy, grad


def _criterion(shape, w, a):
    from bubbleformer_amd.utils import SpectralLpLoss
    return SpectralLpLoss(w, field_weights=a, grid=shape[-2:])


def _native(crit, pred, y):
    """(loss, field terms, plain terms, {S_e, S_y} the forward left for the backward, gradient of SCALE * loss)"""
    p = pred.detach().requires_grad_(True)
    val = crit(p, y)
    sums = val.grad_fn.saved_tensors[1].view(*pred.shape[:3], 2)
    (val * SCALE).backward()
    return val.detach(), crit.field_terms(), crit.plain_terms(), sums, p.grad


def _live_weight_conditions(pred, y, w, a, grad):
    if min(pred.shape[-2:]) <= 2:
        return
    p, t, one = pred.double(), y.double(), torch.ones_like(w)
    (se, sy), (se1, sy1) = SR.row_sums(p, t, w), SR.row_sums(p, t, one)
    assert float((se / se1).min()) >= 2.0 and float((sy / sy1).min()) >= 1.25
    g1 = SR.closed_form_gradient(p, t, one, a, g=SCALE)
    assert float((grad - g1).norm() / g1.norm()) >= 0.3


def _compare(label, pred, y, w, got, want):
    """Every figure of one native call against the restatement's, each held to its bound; prints the worst ratio of error to bound."""
    val, terms, plain, sums, grad = got
    wval, wterms, wplain, wse, wsy, wgrad = want
    C = pred.shape[2]
    assert val.shape == () and val.dtype == torch.float32 and terms.shape == (C,) and plain.shape == (C,) and grad.shape == pred.shape
    assert torch.isfinite(grad).all()
    be, by, rel, grel = SR.bounds(pred, y, w)
    _, _, rel1, _ = SR.bounds(pred, y, torch.ones_like(w))
    r_se = float(((sums[..., 0] - wse).abs() / be).max())
    r_sy = float(((sums[..., 1] - wsy).abs() / by).max())
    r_val = float((val.double() - wval).abs() / wval / rel.max())
    r_terms = float(((terms.double() - wterms).abs() / wterms / rel.amax((0, 1))).max())
    r_plain = float(((plain.double() - wplain).abs() / wplain / rel1.amax((0, 1))).max())
    err = ((grad.double() - wgrad).flatten(-2).norm(dim=-1) / wgrad.flatten(-2).norm(dim=-1))
    r_grad = float((err / grel).max())
    print(f"{label}: error / bound: S_e {r_se:.3g}, S_y {r_sy:.3g}, value {r_val:.3g}, field terms {r_terms:.3g}, plain terms {r_plain:.3g}, "
          f"gradient rows {r_grad:.3g} (worst row {float(err.max()):.2e}; eta {SR.eta(*pred.shape[-2:]):.2e})")
    assert max(r_se, r_sy, r_val, r_terms, r_plain, r_grad) <= 1.0, (r_se, r_sy, r_val, r_terms, r_plain, r_grad)


@pytest.mark.parametrize("shape", SR.SHAPES)
def test_value_and_gradient_against_the_restatement(shape):
    pred, y, w, a, *want = _case(shape)
    _live_weight_conditions(pred, y, w, a, want[-1])
    got = _native(_criterion(shape, w, a), pred, y)
    torch.cuda.synchronize()
    _compare(str(shape), pred, y, w, got, want)


def test_views_four_bytes_off_a_16_byte_boundary():
    shape = (1, 2, 2, 12, 20)
    pred0, y0, w, a, *want = _case(shape)

    def shifted(t):
        buf = torch.zeros(t.numel() + 4, dtype=torch.float32, device=DEV)
        v = buf[1:1 + t.numel()].view(shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v
    pred, y = shifted(pred0), shifted(y0)
    got = _native(_criterion(shape, w, a), pred, y)
    torch.cuda.synchronize()
    _compare("one float off", pred, y, w, got, want)
    again = _native(_criterion(shape, w, a), pred0, y0)
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(got, again))            # the same bits at either offset


@pytest.mark.parametrize("shape", [(2, 3, 4, 7, 13), (1, 2, 2, 12, 20), (1, 2, 4, 192, 192)])
def test_unit_weights_are_the_native_training_criterion(shape):
    """w = 1, unit field weights: native LpLoss(training configuration) on the GPU, value to the value bound and gradient to the gradient bound
    (LpLoss itself is within a few fp32 ulps of the fp64 result, far inside either)."""
    from bubbleformer_amd.utils import LpLoss, SpectralLpLoss
    pred, y = (t.to(DEV) for t in SR.make_inputs(shape))
    one = torch.ones(shape[2], shell_count(*shape[-2:]), dtype=torch.float64, device=DEV)
    p = pred.detach().requires_grad_(True)
    want = LpLoss(**TRAINING)(p, y)
    (want * SCALE).backward()
    crit = SpectralLpLoss(one)
    val, terms, plain, _, grad = _native(crit, pred, y)
    torch.cuda.synchronize()
    _, _, rel, grel = SR.bounds(pred, y, one)
    ve = abs(float(val) - float(want.detach())) / float(want.detach())
    err = (grad.double() - p.grad.double()).flatten(-2).norm(dim=-1) / p.grad.double().flatten(-2).norm(dim=-1)
    print(f"{shape} w = 1 against LpLoss: value {ve:.2e} (bound {float(rel.max()):.2e}), gradient rows / bound {float((err / grel).max()):.3g}")
    assert ve <= float(rel.max()) and float((err / grel).max()) <= 1.0 and torch.equal(terms, plain) and crit.grid == shape[-2:]


@pytest.mark.parametrize("shape", [(1, 1, 3, 12, 20), (1, 1, 3, 7, 7)])
def test_edge_rows(shape):
    """One frame, so a field term is one row's ratio: a row without error gives 0 and an exactly zero gradient; a target row of zeros a
    non-finite ratio there and finite ones elsewhere."""
    pred, y = (t.to(DEV) for t in SR.make_inputs(shape))
    pred[0, 0, 1] = y[0, 0, 1]
    y[0, 0, 2] = 0.0
    w, a = SR.weights(3, shell_count(*shape[-2:])).to(DEV), SR.field_weights(3)
    crit = _criterion(shape, w, a)
    p = pred.detach().requires_grad_(True)
    val = crit(p, y)
    terms = crit.field_terms()
    g, = torch.autograd.grad(val, p)
    wterms = SR.field_terms(pred.double(), y.double(), w, a)
    torch.cuda.synchronize()
    assert float(terms[1]) == 0.0 and float(g[0, 0, 1].abs().max()) == 0.0
    assert not torch.isfinite(terms[2]) and not torch.isfinite(wterms[2]) and not torch.isfinite(val)
    assert torch.isfinite(terms[0]) and abs(float(terms[0]) - float(wterms[0])) <= float(SR.bounds(pred, y, w)[2][0, 0, 0]) * float(wterms[0])
    assert torch.isfinite(g[0, 0, 0]).all() and float(g[0, 0, 0].abs().max()) > 0.0


def test_two_calls_give_the_same_bits():
    shape = SR.SHAPES[-1]
    pred, y, w, a, *_ = _case(shape)
    crit = _criterion(shape, w, a)
    one, two = _native(crit, pred, y), _native(crit, pred, y)
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(one, two))


@pytest.mark.parametrize("shape", [(2, 2, 2, 12, 20), (2, 2, 2, 97, 8), (2, 2, 4, 192, 192)])
def test_a_frame_alone_has_the_bits_it_has_in_a_batch(shape):
    pred, y = (t.to(DEV) for t in SR.make_inputs(shape))
    w, a = SR.weights(shape[2], shell_count(*shape[-2:])).to(DEV), SR.field_weights(shape[2])
    crit = _criterion(shape, w, a)
    frames = shape[0] * shape[1]
    _, _, _, sums, grad = _native(crit, pred, y)
    b, t = shape[0] - 1, 1
    _, _, _, s1, g1 = _native(crit, pred[b:b + 1, t:t + 1].contiguous(), y[b:b + 1, t:t + 1].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(sums[b, t], s1[0, 0])
    # the row coefficient alone carries 1 / (B T), here a power of two: the batch's rows times the frame count are the lone frame's rows, bit for bit
    assert frames == 4 and torch.equal(grad[b, t] * frames, g1[0, 0])


def test_forward_and_backward_capture_into_a_graph():
    shape = (2, 2, 2, 64, 64)
    base = tuple(t.to(DEV) for t in SR.make_inputs(shape))
    w, a = SR.weights(shape[2], shell_count(*shape[-2:])).to(DEV), SR.field_weights(shape[2])
    crit = _criterion(shape, w, a)
    inputs = [base, (base[0].flip(0).contiguous() * 1.25, base[1].flip(0).contiguous())]

    def run(pred, y):
        val = crit(pred, y)
        g, = torch.autograd.grad(val, pred)
        return val.detach(), crit.field_terms(), crit.plain_terms(), g
    eager = [tuple(t.clone() for t in run(p.clone().requires_grad_(True), y)) for p, y in inputs]
    assert not torch.equal(eager[0][0], eager[1][0])
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
        for got, w_ in zip(outs, want):
            assert torch.equal(got, w_)


@pytest.mark.parametrize("bad", ["K", "grid", "shape", "dtype", "target_grad", "empty", "4d", "fields", "weights", "cpu", "side"])
def test_refusals(bad):
    from bubbleformer_amd._lib import BubbleformerHipError
    from bubbleformer_amd.utils import SpectralLpLoss
    crit = SpectralLpLoss.power_law(8, 8, 4.0, 2.0, C=3, field_weights=(1.0, 1.0, 1.0))
    pred, y = torch.zeros(1, 2, 3, 8, 8, device=DEV), torch.ones(1, 2, 3, 8, 8, device=DEV)
    match = "SpectralLpLoss"
    if bad == "K":
        pred, y = torch.zeros(1, 2, 3, 16, 16, device=DEV), torch.ones(1, 2, 3, 16, 16, device=DEV)
        match = r"8 x 8 grid of 6 shells; got 16 x 16 \(12 shells\)"
    elif bad == "grid":                     # the same shell count on another grid
        pred, y = torch.zeros(1, 2, 3, 8, 12, device=DEV), torch.ones(1, 2, 3, 8, 12, device=DEV)
        match = "8 x 8 grid of 6 shells; got 8 x 12"
    elif bad == "shape":
        y = y[:, :1]
    elif bad == "dtype":
        pred = pred.half()
    elif bad == "target_grad":
        y.requires_grad_(True)
    elif bad == "empty":
        pred, y = pred[:0], y[:0]
    elif bad == "4d":
        pred, y = pred[0], y[0]
    elif bad == "fields":
        pred, y = pred[:, :, :2].contiguous(), y[:, :, :2].contiguous()
    elif bad == "weights":
        crit = SpectralLpLoss.power_law(8, 8, 4.0, 2.0, field_weights=(1.0, 1.0))
    elif bad == "cpu":
        pred, y = pred.cpu(), y.cpu()
    else:
        crit = SpectralLpLoss(torch.ones(shell_count(8, 1032)))
        pred, y = torch.zeros(1, 1, 1, 8, 1032, device=DEV), torch.ones(1, 1, 1, 8, 1032, device=DEV)
        match = "at most 1024"
    with pytest.raises(BubbleformerHipError, match=match):
        crit(pred, y)


# ---------------------------------------------------------------------------------------------------------------- model + criterion
def test_model_with_the_criterion_against_the_oracle():
    """tiny_d64 + SpectralLpLoss + backward in fp32 against the oracle in fp64 with the restatement as loss, to the project's 1e-4 parity bound."""
    from oracle import filmavit_ref as R, weights as W
    from tests.test_gpu_losses import _compare_families, _filmavit
    spec, z, model = _filmavit("tiny_d64")
    cfg = spec["cfg"]
    sd = {k: v.double().requires_grad_(True) for k, v in W.generate(W.param_shapes(**cfg), seed=spec["seed"]).items()}
    xo = torch.from_numpy(z["x"]).double().requires_grad_(True)
    yo, co = torch.from_numpy(z["y"]).double(), torch.from_numpy(z["cond"]).double()
    shape = tuple(yo.shape)
    w, a = SR.weights(shape[2], shell_count(*shape[-2:])), SR.field_weights(shape[2])
    pred_o = R.filmavit_forward(sd, xo, co, patch_size=cfg["patch_size"], num_heads=cfg["num_heads"], attn_scale=cfg.get("attn_scale", True),
                                feat_scale=cfg.get("feat_scale", True))
    pd = pred_o.detach().requires_grad_(True)
    gw, = torch.autograd.grad(SR.loss(pd, yo, w, a), pd)
    g1, = torch.autograd.grad(SR.loss(pd, yo, torch.ones_like(w), a), pd)
    live = float((gw - g1).norm() / g1.norm())
    print(f"oracle: the weighted criterion's gradient w.r.t. the prediction differs from the plain one's by {live:.3g}")
    assert live >= 0.3, live                          # a dead weight cannot pass
    loss_o = SR.loss(pred_o, yo, w, a)
    loss_o.backward()

    crit = _criterion(shape, w, a)
    x = torch.from_numpy(z["x"]).to(DEV).requires_grad_(True)
    loss = crit(model(x, torch.from_numpy(z["cond"]).to(DEV)), torch.from_numpy(z["y"]).to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    le, de = abs(float(loss.detach()) - float(loss_o.detach())) / abs(float(loss_o.detach())), rel_l2(x.grad.cpu(), xo.grad)
    print(f"model + criterion: loss {le:.2e}, dx {de:.2e}")
    assert le <= 1e-4 and de <= 1e-4
    _compare_families({k: p.grad for k, p in model.named_parameters()}, {k: v.grad for k, v in sd.items()}, 1e-4, "spectral criterion")


def _fit_once():
    """Two training steps through fit on the sample files, at the geometry tests/test_gpu_clip_q16.py pins a loss history at."""
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.fit import fit
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils import SpectralLpLoss
    files = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samples", f"sample_{i}.hdf5") for i in (1, 2)]
    torch.manual_seed(0)
    model = get_model("avit", input_fields=4, output_fields=4, time_window=2, patch_size=8, embed_dim=64, num_heads=2, processor_blocks=1,
                      drop_path=0.0, compute_dtype=torch.float32).cuda()
    tr = BubbleForecast(files[:1], norm="std", time_window=2, start_time=5)
    tr.normalize()
    H, W = tr[0][1].shape[-2:]
    crit = SpectralLpLoss.power_law(H, W, 100.0, 2.0, field_weights=(1.0, 0.5, 2.0, 1.0))
    plain = []

    def log(entry):
        plain.append(crit.plain_terms())
    h = fit(model, tr, None, batch_size=4, max_epochs=1, optimizer="adamw", lr=1e-3, weight_decay=1e-2, warmup_iters=None, limit_train_batches=2,
            seed=42, criterion=crit, log=log)
    torch.cuda.synchronize()
    return h, torch.stack(plain).cpu()


def test_fit_records_the_field_terms_and_repeats_its_history():
    """Two TrainStep(criterion=SpectralLpLoss) steps on the sample files, through fit: hist["field_loss"] holds the per-field terms, they add up
    to the training loss, and a second run gives the same loss, field terms and plain terms at BOTH steps, bit for bit (the second step's
    depend on the first step's update).  The parameters themselves are pinned in the next test."""
    (h1, plain1), (h2, plain2) = _fit_once(), _fit_once()
    assert len(h1["train_loss"]) == 2 and np.isfinite(h1["train_loss"]).all()
    fields, again = (np.asarray(h["field_loss"], dtype=np.float64) for h in (h1, h2))
    assert fields.shape == (2, 4) and np.isfinite(fields).all() and (fields > 0).all()
    err = np.abs(fields.sum(1) - np.asarray(h1["train_loss"])) / np.abs(h1["train_loss"])
    assert err.max() <= 1e-6, err
    assert (fields != plain1.double().numpy()).all()           # the monitoring terms are the plain ratios, not the weighted ones
    assert h1["train_loss"] == h2["train_loss"] and np.array_equal(fields, again) and torch.equal(plain1, plain2)
    assert h1["train_loss"][0] != h1["train_loss"][1]


def test_train_step_with_the_criterion_repeats_to_the_bit():
    """TrainStep(criterion=SpectralLpLoss) at the geometry where the project pins the plain step as bit-reproducible (tests/test_gpu_grad_clip.py:
    _tiny("filmavit_bf16"): 16 x 192 x 192 clips, patch 16, E 384, bf16): two steps, run twice from the same weights -- the losses, the field
    terms, the plain terms, every parameter and both optimizer moments are torch.equal.  The criterion's forward, its backward inside the step,
    the flat gradient buffer and the update all lie on that path."""
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils import SpectralLpLoss
    from tests.test_gpu_grad_clip import _tiny
    runs = []
    for _ in range(2):
        model, data = _tiny("filmavit_bf16")
        crit = SpectralLpLoss.power_law(192, 192, 100.0, 2.0, C=4, field_weights=(1.0, 0.5, 2.0, 1.0))
        step = TrainStep(model, lr=1e-3, weight_decay=1e-2, optimizer="adamw", criterion=crit)
        losses, terms, plain = [], [], []
        for i in range(2):
            losses.append(step(*data(i)))
            terms.append(crit.field_terms())
            plain.append(crit.plain_terms())
        torch.cuda.synchronize()
        runs.append((torch.stack(losses), torch.stack(terms), torch.stack(plain), step.flat.flat.clone(), step.m.clone(), step.v.clone()))
        assert step.step_no == 2 and bool(torch.isfinite(runs[-1][0]).all())
    a, b = runs
    assert not torch.equal(a[0][0], a[0][1]) and float((a[1] - a[2]).abs().min()) > 0.0
    for name, p, q in zip(("losses", "field terms", "plain terms", "parameters", "first moment", "second moment"), a, b):
        assert torch.equal(p, q), name
