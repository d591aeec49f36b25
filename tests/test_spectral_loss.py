"""CPU: the shell-weighted spectral criterion's definition (tests/spectral_loss_restatement.py) against the plain criterion and its closed-form
gradient; the from_spectrum scaling identity; the mutants the GPU test must be able to see, on the GPU test's own inputs; SpectralLpLoss's
constructors and refusals; bf_slp_fwd / bf_slp_bwd refusing every single defect before any HIP call."""
import ctypes as C
import functools
import os

import pytest
import torch

from tests import losses_restatement as RS
from tests import spectral_loss_restatement as SR
from tests.errors_restatement import shell_count

TRAINING = dict(d=2, p=2, reduce_dims=[0, 1, 2], reductions=["mean", "mean", "sum"])
BIG = [s for s in SR.SHAPES if min(s[-2:]) > 2]


@functools.lru_cache(maxsize=None)
def _case(shape):
    """fp64 (pred, y, w, a) of a shape and the restatement's value and gradient there; computed once, shared, never changed"""
    pred, y = (t.double() for t in SR.make_inputs(shape))
    w, a = SR.weights(shape[2], shell_count(*shape[-2:])), SR.field_weights(shape[2])
    v, g = _grad(lambda p: SR.loss(p, y, w, a), pred)
    return pred, y, w, a, v, g


def _grad(fn, pred):
    p = pred.detach().clone().requires_grad_(True)
    v = fn(p)
    g, = torch.autograd.grad(v, p)
    return v.detach(), g


@pytest.mark.parametrize("shape", [(2, 3, 4, 7, 13), (1, 2, 2, 12, 20), (2, 2, 2, 2, 2), (2, 2, 2, 1, 1)])
def test_unit_weights_are_the_training_criterion(shape):
    pred, y = (t.double() for t in SR.make_inputs(shape))
    w = torch.ones(shape[2], shell_count(*shape[-2:]), dtype=torch.float64)
    got, g1 = _grad(lambda p: SR.loss(p, y, w), pred)
    want, g2 = _grad(lambda p: RS.lp_loss(p, y, **TRAINING), pred)
    assert abs(float(got - want)) <= 1e-12 * abs(float(want))
    assert float((g1 - g2).norm() / g2.norm()) <= 1e-12


@pytest.mark.parametrize("shape", SR.SHAPES[:-1])
def test_closed_form_gradient_is_autograd(shape):
    pred, y, w, a, _, g = _case(shape)
    closed = SR.closed_form_gradient(pred, y, w, a, g=1.75)
    err = float((1.75 * g - closed).abs().max() / g.abs().max())
    assert err <= 1e-12, err


def test_from_spectrum_keeps_the_targets_weighted_power():
    """sum_q w P_y = sum_q P_y per field, w proportional to 1 / max(P_y, floor max P_y)"""
    from bubbleformer_amd.utils import SpectralLpLoss
    g = torch.Generator().manual_seed(5)
    P = torch.rand(3, 12, generator=g, dtype=torch.float64) * torch.logspace(0, -6, 12, dtype=torch.float64)
    crit = SpectralLpLoss.from_spectrum(P, 1e-3)
    w = crit.shell_weights
    assert w.shape == (3, 12) and crit.grid is None
    assert float(((w * P).sum(1) - P.sum(1)).abs().max() / P.sum(1).max()) <= 1e-14
    shape = w * torch.maximum(P, 1e-3 * P.amax(1, keepdim=True))
    assert float((shape / shape[:, :1] - 1).abs().max()) <= 1e-12
    assert float(w[:, -1].min() / w[:, 0].max()) > 100          # the floor binds at the high shells: whitening, not flat
    assert SpectralLpLoss.from_spectrum(P[0], 0.5).shell_weights.shape == (1, 12)
    for bad in (0.0, -1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="floor"):
            SpectralLpLoss.from_spectrum(P, bad)
    with pytest.raises(ValueError, match="spectrum"):
        SpectralLpLoss.from_spectrum(torch.zeros(2, 4), 0.1)


def test_power_law_and_the_constructor():
    from bubbleformer_amd.utils import SpectralLpLoss
    crit = SpectralLpLoss.power_law(12, 20, 100.0, 2.0, C=2, field_weights=(0.5, 2.0))
    K = shell_count(12, 20)
    assert crit.grid == (12, 20) and crit.shell_weights.shape == (2, K) and crit.field_weights == (0.5, 2.0)
    assert torch.equal(crit.shell_weights[0], SR.weights(2, K)[0]) and float(crit.shell_weights[1, -1]) == 101.0
    assert SpectralLpLoss.power_law(1, 1, 3.0, 1.0).shell_weights.tolist() == [[1.0]]
    with pytest.raises(TypeError):
        SpectralLpLoss.power_law(12, 20)                          # gain and power have no defaults
    with pytest.raises(TypeError):
        SpectralLpLoss.from_spectrum(torch.ones(4))               # nor has floor
    for kw in (dict(gain=-1.0, power=2.0), dict(gain=1.0, power=0.0), dict(gain=float("inf"), power=1.0)):
        with pytest.raises(ValueError, match="SpectralLpLoss"):
            SpectralLpLoss.power_law(8, 8, **kw)
    for table in ([1.0, -1.0], [1.0, float("nan")], [[1.0, 1.0], [0.0, 0.0]], [], [[[1.0]]]):
        with pytest.raises(ValueError, match="SpectralLpLoss"):
            SpectralLpLoss(table)
    with pytest.raises(ValueError, match="shells"):
        SpectralLpLoss(torch.ones(4), grid=(16, 16))
    with pytest.raises(ValueError, match="field weights"):
        SpectralLpLoss(torch.ones(2, 4), field_weights=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="field weights"):
        SpectralLpLoss(torch.ones(4), field_weights=(1.0, -1.0))


def test_cpu_tensors_are_refused():
    from bubbleformer_amd._lib import BubbleformerHipError
    from bubbleformer_amd.utils import SpectralLpLoss
    c = SpectralLpLoss.power_law(4, 4, 1.0, 1.0)
    with pytest.raises(BubbleformerHipError, match="SpectralLpLoss"):
        c(torch.zeros(1, 1, 1, 4, 4), torch.zeros(1, 1, 1, 4, 4))
    with pytest.raises(BubbleformerHipError, match="no forward"):
        c.field_terms()
    with pytest.raises(BubbleformerHipError, match="no forward"):
        c.plain_terms()


# ------------------------------------------------------------------------------------------------------- the mutants
def _mutant_applies(mutant, shape):
    """wrong_side is the right table on a square grid; one field has no second table to swap with"""
    if mutant == "wrong_side":
        return shape[-2] != shape[-1]
    if mutant == "tables_swapped":
        return shape[2] > 1
    return True


@pytest.mark.parametrize("shape,mutant", [(s, m) for s in BIG for m in SR.MUTANTS if _mutant_applies(m, s)])
def test_mutants_move_the_result_by_more_than_the_gpu_bound(mutant, shape):
    """A mistake the GPU comparison could not see would be no test of it: on the GPU test's inputs every mutant of the restatement moves the
    loss, or the gradient w.r.t. the prediction, by more than 100 x the bound the kernels are held to at that shape (the worst row's)."""
    pred, y, w, a, v0, g0 = _case(shape)
    _, _, rel, grel = SR.bounds(pred, y, w)
    v1, g1 = _grad(lambda p: SR.loss(p, y, w, a, mutant=mutant), pred)
    dv, dg = abs(float(v1 - v0)) / abs(float(v0)), float((g1 - g0).norm() / g0.norm())
    print(f"{mutant} {shape}: value {dv:.2e} (bound {float(rel.max()):.2e}), gradient {dg:.2e} (bound {float(grel.max()):.2e})")
    assert dv > 100 * float(rel.max()) or dg > 100 * float(grel.max()), (dv, dg)


@pytest.mark.parametrize("shape", BIG)
def test_the_inputs_keep_a_dead_weight_from_passing(shape):
    """The conditions the GPU test asserts from the restatement, here on the CPU: every row's weighted sums are well away from the plain ones and
    so is the gradient."""
    pred, y, w, a, _, g = _case(shape)
    one = torch.ones_like(w)
    (se, sy), (se1, sy1) = SR.row_sums(pred, y, w), SR.row_sums(pred, y, one)
    assert float((se / se1).min()) >= 2.0 and float((sy / sy1).min()) >= 1.25, (float((se / se1).min()), float((sy / sy1).min()))
    _, g1 = _grad(lambda p: SR.loss(p, y, one, a), pred)
    assert float((g - g1).norm() / g1.norm()) >= 0.3


# ------------------------------------------------------------------------------------------------------- the C entries' checks
_BUF = []


def _calls(**kw):
    """(arguments of bf_slp_fwd, of bf_slp_bwd) every check accepts -- aligned host buffers nothing reads but the host table -- with `kw` laid
    over them; a string value moves a pointer by that many bytes."""
    if not _BUF:
        _BUF.append((C.c_char * 8192)())
    p = (C.addressof(_BUF[0]) + 15) // 16 * 16
    a = dict(pred=p, y=p + 512, frames=2, C=2, H=4, W=6, table=p + 1024, host=(1.0, 2.0, 3.0, 0.0, 0.0, 0.5), K=3, weights=(1.0, 0.5), loss=p + 1280,
             terms=p + 1296, sums=p + 1344, spec=p + 2048, ws=p + 4096, ws_bytes=None, g=p + 1312, dpred=p + 1536)
    a.update({k: (a[k] + int(v) if isinstance(v, str) else v) for k, v in kw.items()})
    host = (C.c_double * len(a["host"]))(*a["host"]) if a["host"] is not None else None
    w = (C.c_double * len(a["weights"]))(*a["weights"]) if a["weights"] is not None else None
    fwd = (a["pred"], a["y"], a["frames"], a["C"], a["H"], a["W"], a["table"], host, a["K"], w, a["loss"], a["terms"], a["sums"], a["spec"], a["ws"],
           (1 << 20) if a["ws_bytes"] is None else a["ws_bytes"], None)
    bwd = (a["spec"], a["g"], a["sums"], a["frames"], a["C"], a["H"], a["W"], w, a["dpred"], None)
    return fwd, bwd


_SIZES = "B*T must be 1 .. 2^20, C 1 .. 16, H and W 1 .. 1024"
_BOTH = {
    "sums_null": (dict(sums=None), "null pointer"), "spec_null": (dict(spec=None), "null pointer"),
    "C_zero": (dict(C=0, weights=None), _SIZES), "C_17": (dict(C=17, weights=None), _SIZES), "H_zero": (dict(H=0), _SIZES),
    "W_negative": (dict(W=-4), _SIZES), "W_1025": (dict(W=1025), _SIZES), "H_1025": (dict(H=1025), _SIZES),
    "frames_zero": (dict(frames=0), _SIZES), "frames_huge": (dict(frames=(1 << 20) + 1), _SIZES),
    "field_weight_negative": (dict(weights=(1.0, -0.5)), "field weights must be finite and >= 0"),
    "field_weight_nan": (dict(weights=(float("nan"), 1.0)), "field weights must be finite and >= 0"),
    "sums_off_by_4": (dict(sums="+4"), "misaligned pointer"), "spec_off_by_4": (dict(spec="+4"), "misaligned pointer"),
}
_FWD = {"pred_null": (dict(pred=None), "null pointer"), "y_null": (dict(y=None), "null pointer"), "table_null": (dict(table=None), "null pointer"),
        "host_table_null": (dict(host=None), "null pointer"), "loss_null": (dict(loss=None), "null pointer"), "terms_null": (dict(terms=None), "null pointer"),
        "ws_null": (dict(ws=None), "null pointer"),
        "K_short": (dict(K=2), "K is not the shell count of (H, W)"), "K_long": (dict(K=4, host=(1.0,) * 8), "K is not the shell count of (H, W)"),
        "shell_weight_negative": (dict(host=(1.0, 2.0, -3.0, 0.0, 0.0, 0.5)), "shell weights must be finite and >= 0"),
        "shell_weight_inf": (dict(host=(1.0, float("inf"), 3.0, 0.0, 0.0, 0.5)), "shell weights must be finite and >= 0"),
        "shell_weight_nan": (dict(host=(1.0, 2.0, 3.0, 0.0, float("nan"), 0.5)), "shell weights must be finite and >= 0"),
        "table_all_zero": (dict(host=(1.0, 2.0, 3.0, 0.0, 0.0, 0.0)), "a field's shell weights are all zero"),
        "pred_off_by_2": (dict(pred="+2"), "misaligned pointer"), "y_off_by_2": (dict(y="+2"), "misaligned pointer"),
        "table_off_by_4": (dict(table="+4"), "misaligned pointer"), "ws_off_by_8": (dict(ws="+8"), "misaligned pointer"),
        "terms_off_by_2": (dict(terms="+2"), "misaligned pointer"), "ws_short": (dict(ws_bytes=64), "workspace smaller than bf_slp_ws_bytes")}
_BWD = {"g_null": (dict(g=None), "null pointer"), "dpred_null": (dict(dpred=None), "null pointer"), "dpred_off_by_2": (dict(dpred="+2"), "misaligned pointer"),
        "dpred_inside_spec": (dict(dpred="+768"), "the gradient cannot alias the saved spectrum")}
_CASES = [("bf_slp_fwd", d) for d in sorted({**_BOTH, **_FWD})] + [("bf_slp_bwd", d) for d in sorted({**_BOTH, **_BWD})]


def _lib():
    from bubbleformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.mark.parametrize("name,defect", _CASES)
def test_entry_with_one_defect_is_refused(name, defect):
    """bf_slp_fwd / bf_slp_bwd run every check before any HIP call: no GPU needed.  An otherwise valid call (host buffers nobody reads) with
    exactly one defect is refused under the entry's name and for that defect; no valid call is made here."""
    h = _lib()
    fields, reason = {**_BOTH, **_FWD, **_BWD}[defect]
    fwd, bwd = _calls(**fields)
    assert getattr(h, name)(*(fwd if name == "bf_slp_fwd" else bwd)) != 0
    msg = h.bf_last_error().decode()
    assert (name + ": ") in msg, msg
    assert reason in msg, msg


def test_the_valid_call_of_the_defect_table_passes_the_checks_up_to_the_workspace():
    """The table's base call is valid: with one byte of workspace too few it gets as far as the last check, which names the size."""
    h = _lib()
    need = h.bf_slp_ws_bytes(2, 2, 4, 6)
    assert need > 0 and need % 16 == 0 and h.bf_slp_ws_bytes(0, 2, 4, 6) == -1 and h.bf_slp_ws_bytes(2, 17, 4, 6) == -1 and h.bf_slp_ws_bytes(2, 2, 4, 1025) == -1
    fwd, _ = _calls(ws_bytes=need - 1)
    assert h.bf_slp_fwd(*fwd) != 0 and "workspace smaller" in h.bf_last_error().decode()
