"""GPU: utils.losses.InterfaceLpLoss (csrc/losses.hip: bf_wlp_fwd / bf_wlp_bwd) against tests/interface_loss_restatement.py in fp64 on the
same fp32 inputs; its limits against the native LpLoss; views off a 16-byte boundary; edge rows; bits; graph capture; the model, TrainStep and
fit with it.

Bounds come from the arithmetic, as in tests/test_gpu_losses.py: inputs are fp32, every weight, sum, coefficient and stencil is fp64 and each
result is rounded once (the SDF channel's gradient twice: the data term's launch, then the penalty's addition), so a value is within a few
fp32 ulps (6e-8 each) of the fp64 result of the same inputs: 1e-6 for the value, every field term, the gradient's relative L2 and the worst row.

Inputs (interface_loss_restatement.make_inputs, field seed 2, noise seed 1): checked on the CPU at every shape and band used here -- the
smallest share of a frame inside the band is 1.9 % (129 x 131, band 2 cells; the bench shape at band 2 cells has frames at 0.77 %, so it runs
at 4 cells: 1.5 %), the smallest relative difference between a row's weighted and unweighted ratio 4.1e-3 (24 x 24, band 4 cells), and at
eikonal = 2e-3 the penalty's gradient is 0.23 .. 1.6 times the data term's at every shape, so no shape needs a coefficient of its own."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import interface_loss_restatement as IR
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAINING = dict(d=2, p=2, reduce_dims=[0, 1, 2], reductions=["mean", "mean", "sum"])
BENCH_SHAPE = (8, 16, 4, 192, 192)
DIFF, DIV, GAIN, LAM = 0.37, 1.98, 4.0, 2e-3
WEIGHTS = (1.0, 0.5, 2.0, 0.25)
TOL = 1e-6


@functools.lru_cache(maxsize=4)
def _inputs(shape, s, cells):
    pred, y = IR.make_inputs(shape, s, cells / 32, DIFF, DIV)
    return pred.to(DEV), y.to(DEV)


def _criterion(shape, s, cells, lam, **kw):
    from bubbleformer_amd.utils import InterfaceLpLoss
    args = dict(diff=DIFF, div=DIV, field_weights=WEIGHTS[:shape[2]], eikonal=lam)
    args.update(kw)
    return InterfaceLpLoss(s, cells / 32, args.pop("gain", GAIN), **args)


def _native(crit, pred, y, scale=1.75):
    a = pred.detach().requires_grad_(True)
    val = crit(a, y)
    (val * scale).backward()
    return val.detach(), crit.field_terms(), crit.eikonal_term(), a.grad


def _restated(pred, y, s, cells, lam, scale=1.75, gain=GAIN, weights="default"):
    """fp64 on the device: (loss, field terms, penalty, gradient, gradient of the data term alone, of the penalty alone)"""
    a = WEIGHTS[:pred.shape[2]] if weights == "default" else weights
    p, t = pred.detach().double().requires_grad_(True), y.double()
    terms = IR.field_terms(p, t, s, cells / 32, gain, DIFF, DIV, a)
    g_data, = torch.autograd.grad(terms.sum() * scale, p, retain_graph=True)
    eik = IR.eikonal_term(p, s, DIFF, DIV, lam) if lam > 0 else torch.zeros((), dtype=torch.float64, device=pred.device)
    g_eik = torch.autograd.grad(eik * scale, p)[0] if lam > 0 else torch.zeros_like(g_data)
    return (terms.sum() + eik).detach(), terms.detach(), eik.detach(), g_data + g_eik, g_data, g_eik


def _rel(got, want):
    got, want = got.detach().double(), want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(((got - want).abs() / want.abs()).max())


def _row_errs(got, want):
    e, w = (got.detach().double() - want).flatten(-2), want.flatten(-2)
    return float(e.norm() / w.norm()), float((e.norm(dim=-1) / w.norm(dim=-1)).max())


def _live_weight_conditions(pred, y, s, cells):
    """What keeps a dead weight from passing, from the restatement: every frame has >= 1 % of its cells inside the band and (but for the 2 x 2
    frame) a cell outside; every row's weighted ratio differs from its unweighted one by >= 1e-3 relative."""
    share = IR.in_band_share(y, s, cells / 32, DIFF, DIV)
    assert float(share.min()) >= 0.01, float(share.min())
    if y.shape[-2:] != (2, 2):
        assert float(share.max()) < 1.0
    w = IR.weight(y.double(), s, cells / 32, GAIN, DIFF, DIV)
    r_w, r_u = IR.row_ratios(pred.double(), y.double(), w), IR.row_ratios(pred.double(), y.double(), torch.ones_like(w))
    assert float(((r_w - r_u).abs() / r_u).min()) >= 1e-3


def _against_restatement(shape, s, cells, lam):
    pred, y = _inputs(shape, s, cells)
    _live_weight_conditions(pred, y, s, cells)
    want, wterms, weik, wgrad, g_data, g_eik = _restated(pred, y, s, cells, lam)
    if lam > 0:
        ratio = float(g_eik.norm() / g_data.norm())
        print(f"{shape}: |grad penalty| / |grad data| = {ratio:.3g}")
        assert 0.01 <= ratio <= 100.0, ratio              # a dead penalty cannot pass
    val, terms, eik, grad = _native(_criterion(shape, s, cells, lam), pred, y)
    torch.cuda.synchronize()
    assert val.shape == () and val.dtype == torch.float32 and terms.shape == (shape[2],) and eik.shape == ()
    assert grad.shape == pred.shape and torch.isfinite(grad).all()
    ve, te, (ge, gr) = _rel(val, want), _rel(terms, wterms), _row_errs(grad, wgrad)
    ee = _rel(eik, weik) if lam > 0 else float(eik.abs())
    print(f"{shape} s={s} band {cells} cells eikonal {lam}: value {ve:.2e}, field terms {te:.2e}, penalty {ee:.2e}, gradient {ge:.2e} (worst row {gr:.2e})")
    assert ve <= TOL and te <= TOL and ee <= TOL and ge <= TOL and gr <= TOL, (ve, te, ee, ge, gr)


# (shape, SDF channel): ragged short rows with every row at another offset; C = 1 with the whole frame in the band; a narrow frame with s = 1 of 2;
# odd long rows over several spans and Eikonal tiles crossing the 16 x 64 tile edges; whole 16-byte groups in three spans
SMALL = [((2, 3, 4, 7, 13), 0), ((1, 2, 1, 2, 2), 0), ((1, 1, 2, 33, 5), 1), ((2, 2, 3, 129, 131), 2), ((2, 4, 4, 96, 96), 0)]


@pytest.mark.parametrize("lam", [0.0, LAM])
@pytest.mark.parametrize("cells", [2, 4])
@pytest.mark.parametrize("shape,s", SMALL)
def test_value_and_gradient_against_the_restatement(shape, s, cells, lam):
    _against_restatement(shape, s, cells, lam)


@pytest.mark.parametrize("lam", [0.0, LAM])
def test_bench_shape_against_the_restatement(lam):
    _against_restatement(BENCH_SHAPE, 0, 4, lam)


@pytest.mark.parametrize("shape,s", [((2, 3, 4, 7, 13), 0), ((2, 2, 3, 129, 131), 2), ((2, 4, 4, 96, 96), 0)])
def test_without_gain_it_is_the_training_criterion(shape, s):
    """gain = 0, unit weights, no penalty: LpLoss(training configuration), value and gradient; the same again with a gain whose band is narrower
    than every |phi_t|."""
    from bubbleformer_amd.utils import InterfaceLpLoss, LpLoss
    pred, y = _inputs(shape, s, 2)
    a = pred.detach().requires_grad_(True)
    want = LpLoss(**TRAINING)(a, y)
    (want * 1.75).backward()
    narrow = 0.5 * float((y[:, :, s].double() * DIV + DIFF).abs().min())
    assert narrow > 0.0
    for crit in (InterfaceLpLoss(s, 2 / 32, 0.0, diff=DIFF, div=DIV), InterfaceLpLoss(s, narrow, GAIN, diff=DIFF, div=DIV)):
        val, terms, eik, grad = _native(crit, pred, y)
        torch.cuda.synchronize()
        ve, (ge, gr) = _rel(val, want.detach()), _row_errs(grad, a.grad.double())
        print(f"{shape} gain {crit.gain}: value {ve:.2e}, gradient {ge:.2e} (worst row {gr:.2e})")
        assert ve <= TOL and ge <= TOL and gr <= TOL and float(eik) == 0.0


@pytest.mark.parametrize("lam", [0.0, LAM])
@pytest.mark.parametrize("which", ["both", "prediction", "target"])
def test_views_four_bytes_off_a_16_byte_boundary(which, lam):
    """Contiguous views one float into their storage: with both inputs at the same offset the kernels keep their 16-byte accesses behind a
    scalar head; with one of them alone they read scalars."""
    shape, s, cells = (2, 2, 4, 24, 24), 0, 2
    pred0, y0 = _inputs(shape, s, cells)

    def shifted(t, off):
        buf = torch.zeros(t.numel() + 4, dtype=torch.float32, device=DEV)
        v = buf[off:off + t.numel()].view(shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
        return v
    pred = shifted(pred0, 1 if which in ("both", "prediction") else 0)
    y = shifted(y0, 1 if which in ("both", "target") else 0)
    _live_weight_conditions(pred, y, s, cells)
    want, wterms, _, wgrad, _, _ = _restated(pred, y, s, cells, lam)
    val, terms, _, grad = _native(_criterion(shape, s, cells, lam), pred, y)
    torch.cuda.synchronize()
    ve, te, (ge, gr) = _rel(val, want), _rel(terms, wterms), _row_errs(grad, wgrad)
    print(f"{which} eikonal {lam}: value {ve:.2e}, field terms {te:.2e}, gradient {ge:.2e} (worst row {gr:.2e})")
    assert ve <= TOL and te <= TOL and ge <= TOL and gr <= TOL


@pytest.mark.parametrize("shape", [(1, 1, 3, 24, 24), (1, 1, 3, 96, 96), (1, 1, 3, 7, 13)])
def test_edge_rows(shape):
    """One frame, so a field term is one row's ratio: a row without error gives 0 and an exactly zero, finite gradient; a target row of zeros a
    non-finite ratio there and finite ones elsewhere."""
    s, cells = 0, 2
    pred, y = (t.clone() for t in _inputs(shape, s, cells))
    pred[0, 0, 1] = y[0, 0, 1]
    y[0, 0, 2] = 0.0
    crit = _criterion(shape, s, cells, 0.0)
    a = pred.detach().requires_grad_(True)
    val = crit(a, y)
    terms = crit.field_terms()
    g, = torch.autograd.grad(val, a)
    wterms = IR.field_terms(pred.double(), y.double(), s, cells / 32, GAIN, DIFF, DIV, WEIGHTS[:3])
    torch.cuda.synchronize()
    assert float(terms[1]) == 0.0 and torch.isfinite(g[0, 0, 1]).all() and float(g[0, 0, 1].abs().max()) == 0.0
    assert not torch.isfinite(terms[2]) and not torch.isfinite(wterms[2]) and not torch.isfinite(val)
    assert torch.isfinite(terms[0]) and _rel(terms[:1], wterms[:1]) <= TOL
    assert torch.isfinite(g[0, 0, :2]).all() and float(g[0, 0, 0].abs().max()) > 0.0


def test_flat_patch_in_the_predicted_distance_gives_a_finite_gradient():
    """Where |grad phi_p| is exactly 0 autograd of the restatement multiplies 0 by inf; the kernel's cell contributes 0, as eikonal_loss's does."""
    shape, s, cells = (1, 2, 2, 32, 40), 0, 2
    pred, y = (t.clone() for t in _inputs(shape, s, cells))
    pred[0, 0, s, 10:18, 20:28] = 0.125
    want, wterms, weik, wgrad, _, _ = _restated(pred, y, s, cells, LAM)
    val, terms, eik, grad = _native(_criterion(shape, s, cells, LAM), pred, y)
    torch.cuda.synchronize()
    nan = torch.isnan(wgrad)
    inside = torch.zeros_like(nan)
    inside[0, 0, s, 10:18, 20:28] = True
    assert 0 < int(nan.sum()) <= 64 and not bool((nan & ~inside).any())          # the mask cannot grow to hide a wrong kernel
    assert torch.isfinite(grad).all()
    ve, ee, ge = _rel(val, want), _rel(eik, weik), rel_l2(grad[~nan].cpu(), wgrad[~nan].cpu())
    print(f"flat patch: {int(nan.sum())} NaN cells in the restatement's gradient, value {ve:.2e}, penalty {ee:.2e}, gradient elsewhere {ge:.2e}")
    assert ve <= TOL and ee <= TOL and ge <= TOL


def test_two_calls_give_the_same_bits():
    pred, y = _inputs(BENCH_SHAPE, 0, 4)
    crit = _criterion(BENCH_SHAPE, 0, 4, LAM)
    (v1, t1, e1, g1), (v2, t2, e2, g2) = _native(crit, pred, y), _native(crit, pred, y)
    torch.cuda.synchronize()
    assert torch.equal(v1, v2) and torch.equal(t1, t2) and torch.equal(e1, e2) and torch.equal(g1, g2)


def test_the_penalty_alone_has_the_bits_of_eikonal_loss_backward():
    """The penalty's backward and eikonal_loss's backward run one tile body (losses.hip's eik_bwd_tile).  With zero field weights the data term
    writes zeros and the tile adds onto them; with diff = 0, div = 1, eikonal = 1 and the default dx both kernels get inv_dx = 32 exactly and
    scale = 2 g / (B T H W), g = 1: the same bits.  33 x 70 is three tile rows and two tile columns, both with ragged ends."""
    from bubbleformer_amd.utils import InterfaceLpLoss, eikonal_loss
    shape, s = (2, 2, 3, 33, 70), 1
    pred, y = (t.to(DEV) for t in IR.make_inputs(shape, s, 1.0, 0.0, 1.0))
    crit = InterfaceLpLoss(s, band=1.0, gain=0.0, diff=0.0, div=1.0, field_weights=(0, 0, 0), eikonal=1.0)
    a = pred.detach().requires_grad_(True)
    loss = crit(a, y)
    loss.backward()
    phi = pred[:, :, s].detach().clone().requires_grad_(True)
    eikonal_loss(phi).backward()
    torch.cuda.synchronize()
    assert float(phi.grad.abs().max()) > 0.0
    assert torch.equal(a.grad[:, :, s], phi.grad)
    assert float(a.grad[:, :, 0].abs().max()) == 0.0 and float(a.grad[:, :, 2].abs().max()) == 0.0
    assert torch.equal(crit.eikonal_term(), loss.detach())


def test_forward_and_backward_capture_into_a_graph():
    shape, s = (2, 4, 4, 96, 96), 0
    crit = _criterion(shape, s, 2, LAM)
    base = _inputs(shape, s, 2)
    inputs = [base, (base[0].flip(0).contiguous() * 1.25, base[1].flip(0).contiguous())]

    def run(pred, y):
        val = crit(pred, y)
        g, = torch.autograd.grad(val, pred)
        return val.detach(), crit.field_terms(), crit.eikonal_term(), g
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
        for got, w in zip(outs, want):
            assert torch.equal(got, w)


@pytest.mark.parametrize("bad", ["shape", "dtype", "target_grad", "empty", "channel", "4d", "weights"])
def test_refusals(bad):
    from bubbleformer_amd._lib import BubbleformerHipError
    from bubbleformer_amd.utils import InterfaceLpLoss
    crit = InterfaceLpLoss(2, 2 / 32, 4.0, field_weights=(1.0, 1.0, 1.0))
    pred, y = torch.zeros(1, 2, 3, 8, 8, device=DEV), torch.ones(1, 2, 3, 8, 8, device=DEV)
    if bad == "shape":
        y = y[:, :1]
    elif bad == "dtype":
        pred = pred.half()
    elif bad == "target_grad":
        y.requires_grad_(True)
    elif bad == "empty":
        pred, y = pred[:0], y[:0]
    elif bad == "channel":
        pred, y = pred[:, :, :2], y[:, :, :2]
    elif bad == "4d":
        pred, y = pred[0], y[0]
    else:
        pred, y = torch.zeros(1, 2, 4, 8, 8, device=DEV), torch.ones(1, 2, 4, 8, 8, device=DEV)
    with pytest.raises(BubbleformerHipError, match="InterfaceLpLoss"):
        crit(pred, y)


# ---------------------------------------------------------------------------------------------------------------- model + criterion
def test_model_with_the_criterion_against_the_oracle():
    """tiny_d64 + InterfaceLpLoss(eikonal > 0) + backward in fp32 against the oracle in fp64 with the restatement as loss.  The variant's target
    is no signed distance, so the band is 1.0 in its units, which puts a good share of the cells inside; the penalty's share of the gradient is
    asserted from the oracle."""
    from bubbleformer_amd.utils import InterfaceLpLoss
    from oracle import filmavit_ref as R, weights as W
    from tests.test_gpu_losses import _compare_families, _filmavit
    s, band, weights = 0, 1.0, WEIGHTS
    spec, z, model = _filmavit("tiny_d64")
    cfg = spec["cfg"]
    sd = {k: v.double().requires_grad_(True) for k, v in W.generate(W.param_shapes(**cfg), seed=spec["seed"]).items()}
    xo = torch.from_numpy(z["x"]).double().requires_grad_(True)
    yo, co = torch.from_numpy(z["y"]).double(), torch.from_numpy(z["cond"]).double()
    weights = weights[:yo.shape[2]]
    pred_o = R.filmavit_forward(sd, xo, co, patch_size=cfg["patch_size"], num_heads=cfg["num_heads"], attn_scale=cfg.get("attn_scale", True),
                                feat_scale=cfg.get("feat_scale", True))
    share = IR.in_band_share(yo, s, band, DIFF, DIV)
    assert 0.05 <= float(share.min()) and float(share.max()) <= 0.95, (float(share.min()), float(share.max()))
    pd = pred_o.detach().requires_grad_(True)
    g_data, = torch.autograd.grad(IR.field_terms(pd, yo, s, band, GAIN, DIFF, DIV, weights).sum(), pd)
    g_eik, = torch.autograd.grad(IR.eikonal_term(pd, s, DIFF, DIV, LAM), pd)
    ratio = float(g_eik.norm() / g_data.norm())
    print(f"oracle: |grad data| {float(g_data.norm()):.3g}, |grad penalty| {float(g_eik.norm()):.3g}, ratio {ratio:.3g}")
    assert 0.01 <= ratio <= 100.0, ratio
    loss_o = IR.loss(pred_o, yo, s, band, GAIN, DIFF, DIV, weights, LAM)
    loss_o.backward()

    crit = InterfaceLpLoss(s, band, GAIN, diff=DIFF, div=DIV, field_weights=weights, eikonal=LAM)
    x = torch.from_numpy(z["x"]).to(DEV).requires_grad_(True)
    loss = crit(model(x, torch.from_numpy(z["cond"]).to(DEV)), torch.from_numpy(z["y"]).to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    le, de = abs(float(loss.detach()) - float(loss_o.detach())) / abs(float(loss_o.detach())), rel_l2(x.grad.cpu(), xo.grad)
    print(f"model + criterion: loss {le:.2e}, dx {de:.2e}")
    assert le <= 1e-4 and de <= 1e-4
    _compare_families({k: p.grad for k, p in model.named_parameters()}, {k: v.grad for k, v in sd.items()}, 1e-4, "interface criterion")


def test_unrolled_train_step_takes_the_criterion():
    from bubbleformer_amd.trainer import TrainStep
    from tests.test_gpu_losses import _filmavit
    spec, z, model = _filmavit("tiny_d64")
    x, c, y = (torch.from_numpy(z[k]).to(DEV) for k in ("x", "cond", "y"))
    crit = _criterion(tuple(y.shape), 0, 32, LAM)
    step = TrainStep(model, lr=1e-3, weight_decay=1e-2, optimizer="adamw", criterion=crit, unroll_steps=2)
    loss = step(x, c, torch.stack([y, y * 0.5 + 0.1]))
    torch.cuda.synchronize()
    assert step.step_no == 1 and loss.shape == () and bool(torch.isfinite(loss)) and bool(torch.isfinite(step.unroll_losses).all())
    assert bool(torch.isfinite(crit.field_terms()).all()) and float(crit.eikonal_term()) > 0.0


def test_fit_trains_validates_and_records_the_field_terms():
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.fit import fit, validate
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils import InterfaceLpLoss
    files = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samples", f"sample_{i}.hdf5") for i in (1, 2)]
    torch.manual_seed(0)
    model = get_model("avit", input_fields=4, output_fields=4, time_window=4, patch_size=8, embed_dim=64, num_heads=2, processor_blocks=2,
                      drop_path=0.0, compute_dtype=torch.float32).cuda()
    tr = BubbleForecast(files[:1], norm="std", time_window=4, start_time=5)
    consts = tr.normalize()
    va = BubbleForecast(files[1:], norm="std", time_window=4, start_time=5)
    va.normalize(*consts)
    crit = InterfaceLpLoss.for_dataset(tr, 4 / 32, GAIN, field_weights={"temperature": 0.5, "velx": 2.0}, eikonal=LAM)
    assert crit.sdf_channel == list(tr.output_fields).index("dfun") and crit.field_weights == (1.0, 0.5, 2.0, 1.0)
    penalties, logged = [], []

    def log(entry):
        if "train_loss" in entry:
            penalties.append(crit.eikonal_term())           # of the batch just trained on: validation has not run yet
            logged.append(entry["field_loss"])
    h = fit(model, tr, va, batch_size=4, max_epochs=2, optimizer="adamw", lr=2e-3, weight_decay=1e-2, warmup_iters=2, eta_min=1e-6,
            limit_train_batches=3, limit_val_batches=2, seed=42, criterion=crit, log=log)
    assert len(h["train_loss"]) == 6 and len(h["val_loss"]) == 2 and np.isfinite(h["train_loss"]).all() and np.isfinite(h["val_loss"]).all()
    fields = np.asarray(h["field_loss"], dtype=np.float64)
    assert fields.shape == (6, 4) and np.isfinite(fields).all() and (fields > 0).all()
    assert np.array_equal(fields, torch.stack(logged).double().cpu().numpy())
    total = fields.sum(1) + torch.stack(penalties).double().cpu().numpy()
    err = np.abs(total - np.asarray(h["train_loss"])) / np.abs(h["train_loss"])
    print(f"fit: field terms + penalty against the training loss {err.max():.2e}; penalty share {float(torch.stack(penalties).mean()) / np.mean(h['train_loss']):.3g}")
    assert err.max() <= 1e-6 and float(torch.stack(penalties).min()) > 0.0
    vstore = va.device_store(torch.device(DEV))
    assert validate(model, va, vstore, 4, 2, criterion=crit) == h["val_loss"][-1]
