"""GPU: the averaged copy of the weights (EMA / SWA) kept inside the fused optimizer kernels (csrc/optim_kernels.h: the AVG bodies,
bf_adamw / bf_adam / bf_lion with avg, bf_weight_average, bf_swap_buffers), TrainStep(weight_average=...), its averaged_weights()
context, fit and checkpoints, and two data-parallel ranks.

The bound on the average is per element and comes from the arithmetic alone (tests/averaging_restatement.py): the kernel's update is a
subtraction and one fma, two correctly rounded fp32 operations, so |a - restatement| <= 4 * 2^-24 * (|a_prev| + |p_new|) with the fp64
restatement applied to the GPU's own a_prev and p_new."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import averaging_restatement as A
from tests.test_gpu_ddp import _free_port
from tests.test_rollout_eval import FILES

pytestmark = pytest.mark.gpu

OPTS = ("adamw", "adam", "lion")
MODES = {"host": dict(grad_scale=0.25), "coef": dict(grad_scale=0.25, coef=0.5), "clamp": dict(grad_scale=0.25, clip_value=1e-3)}
WEIGHTS = (1.0, 1.0 / 3, 0.1, 1e-3, 1.0)


def _opt_call(opt, p, g, m, v, step, mode, **avg):
    """One launch of the optimizer `opt` in scale mode `mode`; avg = {} is the plain entry."""
    from bubbleformer_amd import ops
    kw = dict(MODES[mode])
    if "coef" in kw:
        kw["coef"] = torch.tensor([kw["coef"]], device="cuda")
    kw.update(avg)
    if opt == "lion":
        ops.lion_(p, g, m, 1e-3, weight_decay=0.1, **kw)
    else:
        getattr(ops, opt + "_")(p, g, m, v, step, 2.5e-4, weight_decay=1e-2, **kw)


def _within_bound(a, a_prev, p_new, w):
    got = a.cpu().numpy().astype(np.float64)
    ap, pn = a_prev.cpu().numpy(), p_new.cpu().numpy()
    err = np.abs(got - A.lerp(ap, pn, w))
    bound = A.lerp_bound(ap, pn)
    worst = float(np.max(err / np.maximum(bound / 4.0, 1e-300))) if err.size else 0.0       # in units of 2^-24 (|a_prev| + |p_new|)
    return bool(np.all(err <= bound)), worst


@pytest.mark.parametrize("n", [3, 4096, 10007])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("opt", OPTS)
def test_fused_average_kernel(opt, mode, n):
    """Five steps with w = 1, 1/3, 0.1, 1e-3, 1 on two buffers: exactly n elements (n = 3: the scalar tail alone; 4096: no tail; 10007: body
    and tail) and the same padded to a multiple of 64 plus 64 zeros, as FlatParams lays it out.  After every step p, m, v equal the plain
    entry's on a copy of the same state bit for bit, the average is within the two-rounding bound of the fp64 restatement (and is p
    itself where w = 1), and the padding of p, m, v and the average is exactly zero."""
    gen = torch.Generator(device="cuda").manual_seed(11)
    padded = (n + 63) // 64 * 64 + 64
    p0 = torch.randn(n, device="cuda", generator=gen)
    bufs = []
    for size in (n, padded):                         # [p, grad, m, v, avg]
        t = [torch.zeros(size, device="cuda") for _ in range(5)]
        t[0][:n] = p0
        t[4][:n] = torch.randn(n, device="cuda", generator=gen)      # an average that is not the parameters
        bufs.append(t)
    worst = 0.0
    for step, w in enumerate(WEIGHTS, start=1):
        grad = torch.randn(n, device="cuda", generator=gen) * 1e-2    # the clamp at 1e-3 (after the scale 0.25) cuts some and leaves some
        for p, g, m, v, a in bufs:
            g[:n] = grad
            twin = [p.clone(), m.clone(), v.clone()]
            a_prev = a.clone()
            _opt_call(opt, twin[0], g, twin[1], twin[2], step, mode)
            _opt_call(opt, p, g, m, v, step, mode, avg=a, avg_weight=w)
            assert torch.equal(p, twin[0]) and torch.equal(m, twin[1]) and torch.equal(v, twin[2]), (step, p.numel())
            assert not torch.equal(p, a_prev)
            ok, units = _within_bound(a, a_prev, p, w)
            worst = max(worst, units)
            assert ok, (step, w, p.numel(), units)
            if w == 1.0:
                assert torch.equal(a, p), (step, p.numel())
            else:
                assert not torch.equal(a, p) and not torch.equal(a, a_prev)
            for t in (p, m, v, a):
                assert not t[n:].any(), (step, p.numel())
    print(f"{opt} {mode} n={n}: worst error {worst:.3f} units of 2^-24 (|a_prev| + |p_new|), bound 4")


@pytest.mark.parametrize("where", [5, 10006])
@pytest.mark.parametrize("opt", OPTS)
def test_nan_reaches_the_average_at_its_element_only(opt, where):
    """A NaN in one gradient element (in the 16-byte body, and in the scalar tail) makes that element of p NaN under AdamW and Adam, and the
    average follows at that element and no other.  Lion takes only the sign of the gradient term, and the sign of a NaN is 0, so there the
    NaN is planted in p itself."""
    n = 10007
    gen = torch.Generator(device="cuda").manual_seed(12)
    p, g, a = (torch.randn(n, device="cuda", generator=gen) for _ in range(3))
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    (p if opt == "lion" else g)[where] = float("nan")
    _opt_call(opt, p, g, m, v, 1, "host", avg=a, avg_weight=0.1)
    want = torch.zeros(n, dtype=torch.bool, device="cuda")
    want[where] = True
    assert torch.equal(torch.isnan(p), want) and torch.equal(torch.isnan(a), want)


@pytest.mark.parametrize("n", [3, 4096, 10007])
def test_weight_average_alone_is_the_fused_update(n):
    """ops.weight_average_ on the (a_prev, p_new, w) of a fused step gives the fused step's average bit for bit, body and tail alike."""
    from bubbleformer_amd import _lib as L, ops
    gen = torch.Generator(device="cuda").manual_seed(13)
    p, a = torch.randn(n, device="cuda", generator=gen), torch.randn(n, device="cuda", generator=gen)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step, w in enumerate(WEIGHTS, start=1):
        g = torch.randn(n, device="cuda", generator=gen)
        alone = a.clone()
        _opt_call("adamw", p, g, m, v, step, "host", avg=a, avg_weight=w)
        assert ops.weight_average_(alone, p, w) is alone
        assert torch.equal(alone, a), (step, w)
    for bad_w in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(L.BubbleformerHipError):
            ops.weight_average_(a, p, bad_w)
    with pytest.raises(L.BubbleformerHipError):
        ops.weight_average_(a, p[:-1], 0.5)


def test_optimizer_average_arguments_are_checked():
    from bubbleformer_amd import _lib as L, ops
    p, g, m, v, a = (torch.zeros(256, device="cuda") for _ in range(5))
    for kw in (dict(avg=a), dict(avg_weight=0.5), dict(avg=a[:-4], avg_weight=0.5), dict(avg=a.double(), avg_weight=0.5), dict(avg=a.cpu(), avg_weight=0.5),
               dict(avg=a, avg_weight=0.0), dict(avg=a, avg_weight=1.5), dict(avg=torch.zeros(257, device="cuda")[1:], avg_weight=0.5)):
        for call in (lambda: ops.adamw_(p, g, m, v, 1, 1e-3, **kw), lambda: ops.adam_(p, g, m, v, 1, 1e-3, **kw), lambda: ops.lion_(p, g, m, 1e-3, **kw)):
            with pytest.raises(L.BubbleformerHipError):
                call()
    assert not p.any() and not a.any()


@pytest.mark.parametrize("n", [3, 4096, 10007])
def test_swap_buffers(n):
    from bubbleformer_amd import _lib as L, ops
    gen = torch.Generator(device="cuda").manual_seed(14)
    a, b = torch.randn(n, device="cuda", generator=gen), torch.randn(n, device="cuda", generator=gen)
    a[0], b[n - 1] = float("nan"), float("-inf")                    # bits, not values, are exchanged
    a0, b0 = a.clone(), b.clone()
    ops.swap_buffers_(a, b)
    assert torch.equal(a.view(torch.int32), b0.view(torch.int32)) and torch.equal(b.view(torch.int32), a0.view(torch.int32))
    ops.swap_buffers_(a, b)
    assert torch.equal(a.view(torch.int32), a0.view(torch.int32)) and torch.equal(b.view(torch.int32), b0.view(torch.int32))
    big = torch.zeros(n + 4, device="cuda")
    for x, y in ((big[1:n + 1], b), (a, big[1:n + 1]), (a, big[:n + 1]), (a, b.double()), (big[:n], big[4:n + 4] if n > 4 else big[:n])):
        with pytest.raises(L.BubbleformerHipError):
            ops.swap_buffers_(x, y)
    assert torch.equal(a.view(torch.int32), a0.view(torch.int32)) and torch.equal(b.view(torch.int32), b0.view(torch.int32))


def test_swap_of_parameter_buffers_marks_prepared_weights_stale():
    from bubbleformer_amd import ops
    a, b = torch.zeros(64, device="cuda"), torch.ones(64, device="cuda")
    before = ops._WEIGHTS_EPOCH[0]
    ops.swap_buffers_(a, b)
    assert ops._WEIGHTS_EPOCH[0] == before
    ops.swap_buffers_(a, b, parameters=True)
    assert ops._WEIGHTS_EPOCH[0] == before + 1


# ------------------------------------------------------------------------------------------------ the step
def _tiny_model(seed=0):
    """The FiLMAViT of tests/test_abi_exports.py::test_no_cpu_fallback."""
    from bubbleformer_amd.models import get_model
    torch.manual_seed(seed)
    return get_model("filmavit", input_fields=4, output_fields=4, time_window=2, patch_size=4, embed_dim=64, num_heads=1, processor_blocks=1,
                     drop_path=0.0, num_fluid_params=9, compute_dtype=torch.float32).cuda().train()


def _tiny_data(i=0):
    g = torch.Generator().manual_seed(70 + i)
    return torch.randn(2, 2, 4, 8, 8, generator=g).cuda(), torch.randn(2, 9, generator=g).cuda(), torch.randn(2, 2, 4, 8, 8, generator=g).cuda()


def _step_kw(opt):
    return dict(optimizer=opt, lr=1e-3, weight_decay=0.1 if opt == "lion" else 1e-2)


def _check_update(step, a_prev, w, what):
    ok, units = _within_bound(step.avg, a_prev, step.flat.flat, w)
    assert ok, (what, units)
    return units


@pytest.mark.parametrize("opt", OPTS)
def test_train_step_keeps_an_ema_and_leaves_the_optimizer_alone(opt):
    """Six steps with AverageSpec("ema", 0.9, start_step=1): flat, m and v are those of a twin step without the average, bit for bit; the
    average after every step is the restated update of the step's own previous average and new parameters (step 1 copies); five updates
    are counted."""
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.averaging import AverageSpec
    spec = AverageSpec("ema", 0.9, start_step=1)
    step, twin = TrainStep(_tiny_model(), weight_average=spec, **_step_kw(opt)), TrainStep(_tiny_model(), **_step_kw(opt))
    assert twin.avg is None and step.avg is not step.flat.flat and torch.equal(step.avg, step.flat.flat) and step.n_averaged == 0
    worst = 0.0
    for i in range(6):
        x, c, y = _tiny_data(i)
        a_prev, n_prev = step.avg.clone(), step.n_averaged
        la, lb = step(x, c, y), twin(x, c, y)
        assert torch.equal(la, lb) and torch.equal(step.flat.flat, twin.flat.flat) and torch.equal(step.m, twin.m), i
        assert opt == "lion" or torch.equal(step.v, twin.v), i
        w = spec.weight(i + 1, n_prev)
        assert w == (1.0 if i == 0 else 1.0 - 0.9)
        worst = max(worst, _check_update(step, a_prev, w, i))
        if i == 0:
            assert torch.equal(step.avg, step.flat.flat)
        else:
            assert not torch.equal(step.avg, step.flat.flat) and not torch.equal(step.avg, a_prev)
    assert step.n_averaged == 5 and step.step_no == 6
    print(f"{opt}: worst update error {worst:.3f} units, bound 4")


def test_train_step_every_second_step_and_accumulation():
    """every=2: the average changes after steps 2, 4, 6 only.  accumulate_grad_batches=2: six calls are three optimizer steps and three
    updates; a call that does not step leaves the average alone."""
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.averaging import AverageSpec
    spec = AverageSpec("ema", 0.9, every=2)
    step = TrainStep(_tiny_model(), weight_average=spec, **_step_kw("adamw"))
    for i in range(6):
        a_prev = step.avg.clone()
        step(*_tiny_data(i))
        if (i + 1) % 2:
            assert torch.equal(step.avg, a_prev), i
        else:
            assert not torch.equal(step.avg, a_prev), i
            _check_update(step, a_prev, 1.0 - 0.9, i)
    assert step.n_averaged == 3
    spec = AverageSpec("ema", 0.9)
    step = TrainStep(_tiny_model(), weight_average=spec, accumulate_grad_batches=2, **_step_kw("adamw"))
    for i in range(6):
        a_prev, f_prev = step.avg.clone(), step.flat.flat.clone()
        step(*_tiny_data(i))
        if (i + 1) % 2:
            assert torch.equal(step.avg, a_prev) and torch.equal(step.flat.flat, f_prev), i
        else:
            assert not torch.equal(step.avg, a_prev), i
            _check_update(step, a_prev, 1.0 - 0.9, i)
    assert step.n_averaged == 3 and step.step_no == 3


def test_train_step_swa_is_the_mean_of_the_snapshots():
    """kind="swa", start_step=1, five steps: the average is the fp64 mean of the four parameter snapshots taken after steps 2 .. 5, within
    the four updates' bounds added up (an update's error is carried on with a factor 1 - w <= 1)."""
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.averaging import AverageSpec
    step = TrainStep(_tiny_model(), weight_average=AverageSpec("swa", start_step=1), **_step_kw("adamw"))
    snaps, bound = [], 0.0
    for i in range(5):
        a_prev = step.avg.clone()
        step(*_tiny_data(i))
        if i >= 1:
            snaps.append(step.flat.flat.cpu().numpy().astype(np.float64))
            bound = bound + A.lerp_bound(a_prev.cpu().numpy(), step.flat.flat.cpu().numpy())
    assert step.n_averaged == 4
    err = np.abs(step.avg.cpu().numpy().astype(np.float64) - np.mean(np.stack(snaps), axis=0))
    print("swa: worst error / bound %.3f" % float(np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound)


# ------------------------------------------------------------------------------------------------ the context
def _fresh_from(sd):
    from bubbleformer_amd.utils.checkpoint import from_reference_state_dict
    fresh = _tiny_model(seed=99)
    fresh.load_state_dict(from_reference_state_dict(sd))
    return fresh.eval()


def _trained_step(steps=3, **kw):
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.averaging import AverageSpec
    step = TrainStep(_tiny_model(), weight_average=AverageSpec("ema", 0.5, start_step=1), **_step_kw("adamw"), **kw)
    for i in range(steps):
        step(*_tiny_data(i))
    return step


def test_averaged_weights_context():
    """Inside, the model computes with the averaged weights (a fresh model loaded from averaged_state_dict() gives the same bits); after,
    the flat buffer and the eval output are those from before -- prepared inference weights that were not re-made would show here.  The
    state dict is the reference's layout, cloned.  Stepping or nesting inside raises, and an exception inside still swaps back."""
    step = _trained_step()
    model = step.model
    x, c, _ = _tiny_data(9)
    flat0, avg0 = step.flat.flat.clone(), step.avg.clone()
    assert not torch.equal(flat0, avg0)
    with torch.no_grad():
        live = model.eval()(x, c).clone()
    sd = step.averaged_state_dict()
    assert list(sd) == ["model." + k for k in model.state_dict()] and all(t.device.type == "cpu" for t in sd.values())
    for (k, p_), o in zip(model.named_parameters(), step.flat.offsets):
        assert torch.equal(sd["model." + k], avg0[o:o + p_.numel()].view(p_.shape).cpu()), k
    fresh = _fresh_from(sd)
    with torch.no_grad():
        want = fresh(x, c).clone()
    assert not torch.equal(want, live)
    with step.averaged_weights() as inside:
        assert inside is model and torch.equal(step.flat.flat, avg0) and torch.equal(step.avg, flat0)
        with torch.no_grad():
            assert torch.equal(model(x, c), want)
        inner = step.averaged_state_dict()                           # still the averaged weights
        assert all(torch.equal(inner[k], sd[k]) for k in sd)
        with pytest.raises(RuntimeError):
            step(*_tiny_data(3))
        with pytest.raises(RuntimeError):
            step.finish_accumulation()
        with pytest.raises(RuntimeError):
            with step.averaged_weights():
                pass
        assert torch.equal(step.flat.flat, avg0)                     # the refused calls changed nothing
    assert torch.equal(step.flat.flat, flat0) and torch.equal(step.avg, avg0)
    with torch.no_grad():
        assert torch.equal(model(x, c), live)
    with pytest.raises(KeyError):
        with step.averaged_weights():
            raise KeyError("inside")
    assert torch.equal(step.flat.flat, flat0) and torch.equal(step.avg, avg0)
    with torch.no_grad():
        assert torch.equal(model(x, c), live)
    model.train()
    step(*_tiny_data(3))                                             # and the step goes on
    assert step.step_no == 4 and step.n_averaged == 3


def test_a_step_without_an_average_has_no_context():
    from bubbleformer_amd.trainer import TrainStep
    step = TrainStep(_tiny_model(), **_step_kw("adamw"))
    with pytest.raises(RuntimeError):
        step.averaged_state_dict()
    with pytest.raises(RuntimeError):
        with step.averaged_weights():
            pass


def _study(T=2):
    """The two sample trajectories at 32 x 32 with a fluid record per file (the conditioned model's 9 parameters)."""
    from bubbleformer_amd.data import BubbleForecast, hdf5_lite
    fields = ["dfun", "temperature", "velx", "vely"]
    trajs = [{k: np.asarray(f[k][...], dtype=np.float32) for k in fields} for f in (hdf5_lite.File(p) for p in FILES)]
    rec = [{"inv_reynolds": 0.0042 + 0.3 * i, "cpgas": 0.83, "mugas": 0.023, "rhogas": 0.0083, "thcogas": 0.25, "stefan": 0.5298 - 0.2 * i,
            "prandtl": 8.4, "heater": {"nucWaitTime": 0.4, "wallTemp": 1.0 + 0.1 * i}} for i in range(2)]
    ds = BubbleForecast.from_arrays(trajs, rec, norm="std", time_window=T, start_time=5, downsample_factor=2)
    ds.normalize()
    return ds


def test_rollout_evaluation_on_the_averaged_weights():
    """One evaluate_rollouts call (1 trajectory, 2 steps) inside the context equals the call on a fresh model holding the averaged
    weights, and differs from the call on the live weights."""
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.averaging import AverageSpec
    from bubbleformer_amd.utils.rollout import evaluate_rollouts
    store = _study().device_store("cuda")
    step = TrainStep(_tiny_model(), weight_average=AverageSpec("ema", 0.5, start_step=1), **_step_kw("adamw"))
    for i in range(3):
        x, y, c = store.gather([3 + i, 11 + i])
        step(x, c, y)
    model = step.model.eval()
    live = evaluate_rollouts(model, store, [4], 2)
    with step.averaged_weights():
        got = evaluate_rollouts(model, store, [4], 2)
    want = evaluate_rollouts(_fresh_from(step.averaged_state_dict()), store, [4], 2)
    assert torch.equal(got.rel_l2, want.rel_l2) and torch.equal(got.criterion, want.criterion)
    assert not torch.equal(got.rel_l2, live.rel_l2)
    again = evaluate_rollouts(model, store, [4], 2)
    assert torch.equal(again.rel_l2, live.rel_l2)


# ------------------------------------------------------------------------------------------------ fit and checkpoints
def _fit_model():
    from bubbleformer_amd.models import get_model
    torch.manual_seed(0)
    return get_model("avit", input_fields=4, output_fields=4, time_window=4, patch_size=8, embed_dim=64, num_heads=1, processor_blocks=1,
                     drop_path=0.0, compute_dtype=torch.float32).cuda()


def test_fit_validates_checkpoints_and_resumes_the_average(tmp_path):
    """fit on the sample trajectories at 32 x 32 (4 x 4 tokens a frame, one block): two validations an epoch, the checkpoint's
    "weight_average", resume, the released file and the three load cases.  Two epochs straight and one epoch plus a resumed second give the
    same bits in the average, the weights and the count.  That needs a training run that repeats itself bit for bit, which this shape
    does (measured: two straight runs agree in every bit); at 64 x 64 with two blocks of two heads the gradients themselves differ in
    their last bits from run to run (5e-7 in the weights after six steps, with or without an average), which is why
    tests/test_fit_loop.py compares its resumed run to 1e-4."""
    import shutil
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.fit import fit
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.averaging import AverageSpec
    from bubbleformer_amd.utils.checkpoint import from_reference_state_dict, load_checkpoint, save_checkpoint
    tr = BubbleForecast(FILES[:1], norm="std", time_window=4, start_time=5, downsample_factor=2)
    consts = tr.normalize()
    va = BubbleForecast(FILES[1:], norm="std", time_window=4, start_time=5, downsample_factor=2)
    va.normalize(*consts)
    spec = AverageSpec("ema", 0.8, start_step=1)
    kw = dict(batch_size=4, max_epochs=2, optimizer="adamw", lr=2e-3, weight_decay=1e-2, warmup_iters=2, eta_min=1e-6, limit_train_batches=3,
              limit_val_batches=2, seed=42, weight_average=spec)
    ck, ck0, events = str(tmp_path / "last.ckpt"), str(tmp_path / "after_epoch0.ckpt"), []

    def log(e):
        events.append(e)
        if e.get("epoch") == 1 and e.get("batch_idx") == 0:          # the file still holds the end-of-epoch-0 state: keep a copy
            shutil.copy(ck, ck0)
    h = fit(_fit_model(), tr, va, checkpoint_path=ck, log=log, **kw)
    assert len(h["val_loss"]) == 2 and len(h["val_loss_avg"]) == 2 and np.isfinite(h["val_loss_avg"]).all()
    assert all(a != b for a, b in zip(h["val_loss"], h["val_loss_avg"]))
    vals = [e for e in events if "val_loss" in e]
    assert [e["val_loss_avg"] for e in vals] == h["val_loss_avg"] and [e["val_loss"] for e in vals] == h["val_loss"]
    saved = torch.load(ck, weights_only=False)
    wa = saved["weight_average"]
    assert {k: wa[k] for k in ("kind", "decay", "warmup", "start_step", "every", "n_averaged")} == dict(
        kind="ema", decay=0.8, warmup=False, start_step=1, every=1, n_averaged=5)
    assert wa["avg"].device.type == "cpu" and wa["avg"].dtype == torch.float32 and len(saved["state_dict"]) == len(_fit_model().state_dict())
    # one epoch, then the second from the end-of-epoch-0 file: the same bits as the uninterrupted run
    ck2 = str(tmp_path / "resumed.ckpt")
    fit(_fit_model(), tr, va, resume_from=ck0, checkpoint_path=ck2, **kw)
    again = torch.load(ck2, weights_only=False)
    assert torch.load(ck0, weights_only=False)["weight_average"]["n_averaged"] == 2
    assert again["weight_average"]["n_averaged"] == 5 and torch.equal(again["weight_average"]["avg"], wa["avg"])
    assert all(torch.equal(again["state_dict"][k], saved["state_dict"][k]) for k in saved["state_dict"])
    # the released file: the averaged weights as the state dict, no training state
    model = _fit_model()
    step = TrainStep(model, optimizer="adamw", weight_average=spec)
    load_checkpoint(ck, model, step)
    assert step.n_averaged == 5 and torch.equal(step.avg.cpu(), wa["avg"]) and not torch.equal(step.avg, step.flat.flat)
    out = str(tmp_path / "averaged.ckpt")
    save_checkpoint(out, model, None, None, step, averaged=True)
    rel = torch.load(out, weights_only=False)
    assert "optimizer_states" not in rel and "lr_schedulers" not in rel and "weight_average" not in rel and rel["global_step"] == 6
    fresh = _fit_model()
    load_checkpoint(out, fresh)
    mine = step.averaged_state_dict()
    assert all(torch.equal(v.cpu(), mine["model." + k]) for k, v in fresh.state_dict().items())
    assert list(from_reference_state_dict(rel["state_dict"])) == list(fresh.state_dict())
    # a file without the key: the average starts from the loaded weights; a step that does not average ignores the key
    load_checkpoint(out, model, step)
    assert step.n_averaged == 0 and torch.equal(step.avg, step.flat.flat)
    plain = TrainStep(_fit_model(), optimizer="adamw")
    load_checkpoint(ck, plain.model, plain)
    assert plain.avg is None and plain.step_no == 6
    wa["avg"] = wa["avg"][:-64]
    short = str(tmp_path / "short.ckpt")
    torch.save(saved, short)
    with pytest.raises(ValueError):
        load_checkpoint(short, model, step)
    with pytest.raises(ValueError):
        save_checkpoint(out, plain.model, None, None, plain, averaged=True)


# ------------------------------------------------------------------------------------------------ two ranks
def _rank_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.averaging import AverageSpec
    step = TrainStep(_tiny_model(seed=5 + rank), weight_average=AverageSpec("ema", 0.9, start_step=1), **_step_kw("adamw"))
    blob = {"avg0": step.avg.cpu(), "flat0": step.flat.flat.cpu(), "flat": [], "avgs": []}
    for i in range(3):
        step(*_tiny_data(10 * rank + i))
        torch.cuda.synchronize()
        blob["flat"].append(step.flat.flat.cpu())
        blob["avgs"].append(step.avg.cpu())
    blob["n_averaged"] = step.n_averaged
    torch.save(blob, out % rank)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_keep_the_same_average(tmp_path):
    """Two ranks (gloo, both on cuda:0) built from different seeds, three steps on different batches: the average starts as rank 0's
    parameters on both, stays identical bit for bit with no collective of its own, and is the restated replay of rank 0's parameter
    snapshots."""
    out = str(tmp_path / "rank%d.pt")
    mp.spawn(_rank_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = torch.load(out % 0), torch.load(out % 1)
    assert torch.equal(r0["avg0"], r0["flat0"]) and torch.equal(r1["avg0"], r0["flat0"])
    assert r0["n_averaged"] == r1["n_averaged"] == 2
    a_prev, n = r0["avg0"], 0
    for i in range(3):
        assert torch.equal(r0["avgs"][i], r1["avgs"][i]) and torch.equal(r0["flat"][i], r1["flat"][i]), i
        w = A.schedule_weight("ema", 0.9, False, 1, 1, i + 1, n)
        n += i >= 1
        ok, units = _within_bound(r0["avgs"][i], a_prev, r0["flat"][i], w)
        assert ok, (i, units)
        a_prev = r0["avgs"][i]
    assert not torch.equal(r0["avgs"][2], r0["flat"][2])
