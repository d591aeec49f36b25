"""GPU: optimizer steps on a non-finite gradient are skipped by a flag the optimizer launch reads on the device.

csrc/optim_kernels.h (the GUARD bodies of bf_adamw / bf_adam / bf_lion), csrc/gradclip.hip (bf_step_guard, bf_nonfinite_scan) against the
integer restatement of tests/step_guard_restatement.py and against the same launches without the flag; TrainStep(step_guard=...), fit() and
the checkpoint's counter.  Every test runs under a watchdog of its own (STEP_LIMIT_S): a test that hangs ends the process instead of
starting the next one."""
import faulthandler
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from tests import step_guard_restatement as R
from tests.helpers import load_variant

pytestmark = pytest.mark.gpu
STEP_LIMIT_S = 240
INF, NAN = float("inf"), float("nan")
SMALL = dict(input_fields=4, output_fields=4, patch_size=16, embed_dim=384, num_heads=6, processor_blocks=12, num_fluid_params=9)
# tail only; one 16-byte sweep and a tail; two slabs of the scan, no tail; past the optimizers' grid cap (256 * 16 workgroups of 256 threads,
# one 16-byte access each): the grid-stride loop takes a second trip, and the tail follows it
SIZES = [3, 67, 4160, 4 * 256 * 4096 + 4 * 1024 + 3]


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def _bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _flag(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------------ 1. the optimizers
def _opt_call(ops, name, bufs, grad, **kw):
    p, m, v, a = bufs
    if "avg_weight" in kw:
        kw["avg"] = a
    if name == "lion":
        ops.lion_(p, grad, m, 1e-3, (0.9, 0.99), 0.1, 0.5, **kw)
    else:
        getattr(ops, name + "_")(p, grad, m, v, 3, 1e-3, (0.9, 0.999), 1e-8, 1e-2, 0.5, **kw)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["adamw", "adam", "lion"])
def test_a_skipped_launch_writes_nothing_and_a_live_one_is_the_old_kernel(name, n):
    """Every scale mode x average x groups: with the flag 0 and a gradient full of NaN and inf, p, m, v and avg keep their bits; with
    the flag 1 they are the bits of the same call without live=."""
    from bubbleformer_amd import ops
    g = torch.Generator(device="cuda").manual_seed(n % 997 + 1)
    rnd = lambda scale: torch.randn(n, device="cuda", generator=g) * scale      # noqa: E731
    start = (rnd(1.0), rnd(0.1), rnd(0.1).abs(), rnd(1.0))
    grad = rnd(1.0)
    poison = torch.full((n,), NAN, device="cuda")
    poison[1::3] = INF
    poison[2::3] = -INF
    chunks = (n + 63) // 64
    groups = ops.param_group_tables((torch.arange(chunks) % 2).to(torch.uint8), [1.0, 0.5], [1e-2, 0.0], [False, True], n, "cuda")      # odd chunks frozen
    coef = torch.tensor([0.5], device="cuda")
    for mode in ({}, {"coef": coef}, {"clip_value": 0.05}):
        for avg in ({}, {"avg_weight": 0.25}):
            for grp in ({}, {"groups": groups}):
                kw = {**mode, **avg, **grp}
                plain = tuple(t.clone() for t in start)
                _opt_call(ops, name, plain, grad, **kw)
                live = tuple(t.clone() for t in start)
                _opt_call(ops, name, live, grad, live=_flag(1), **kw)
                skipped = tuple(t.clone() for t in start)
                _opt_call(ops, name, skipped, poison, live=_flag(0), **kw)
                torch.cuda.synchronize()
                moved = [not _bits(a, b) for a, b in zip(plain, start)]
                assert moved[0] and moved[1] and moved[3] == bool(avg), (kw.keys(), moved)          # the call compared against did step
                for k, (a, b, c) in enumerate(zip(plain, live, skipped)):
                    assert _bits(a, b), (sorted(kw), "live", "pmva"[k])
                    assert _bits(c, start[k]), (sorted(kw), "skipped", "pmva"[k])
    # any non-zero flag is live
    live = tuple(t.clone() for t in start)
    _opt_call(ops, name, live, grad, live=_flag(-5))
    plain = tuple(t.clone() for t in start)
    _opt_call(ops, name, plain, grad)
    assert _bits(live[0], plain[0]) and _bits(live[1], plain[1])


# ------------------------------------------------------------------------------------------------ 2. bf_step_guard
def test_step_guard_record_follows_the_restatement():
    from bubbleformer_amd import ops
    flt_max = float(np.finfo(np.float32).max)
    lives = []
    for x in (1.0, 0.0, flt_max, INF, NAN):
        guard = torch.tensor(R.FRESH, dtype=torch.int32, device="cuda")
        pair = torch.tensor([x, 123.0], device="cuda")
        ops.step_guard_(pair[:1], guard, 5)
        assert tuple(guard.tolist()) == R.guard_update(R.FRESH, x, 5), x
        lives.append(int(guard[0]))
    assert lives == [1, 1, 1, 0, 0]
    guard = torch.tensor(R.FRESH, dtype=torch.int32, device="cuda")
    norms = [2.0, NAN, INF, 0.5, NAN]
    got = []
    for i, x in enumerate(norms):
        ops.step_guard_(torch.tensor([x], device="cuda"), guard, 10 + i)
        got.append(tuple(guard.tolist()))
    assert got == R.guard_run(norms, first_step=10)
    assert [r[1] for r in got] == [0, 1, 2, 0, 1] and [r[2] for r in got] == [0, 1, 2, 2, 3] and [r[3] for r in got] == [-1, 11, 12, 12, 14]


@pytest.mark.parametrize("n", SIZES)
def test_the_norm_is_a_witness_for_every_element(n):
    """One inf or NaN anywhere -- first element, tail, last element -- makes grad_norm_'s norm non-finite, so the guard is not live; a
    finite gradient whose norm exceeds fp32 is skipped too (documented); a finite one of ordinary size is live."""
    from bubbleformer_amd import ops
    base = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    out = torch.zeros(2, device="cuda")

    def live(gradient):
        guard = torch.tensor(R.FRESH, dtype=torch.int32, device="cuda")
        ops.grad_norm_(gradient, out, INF, 1.0)
        ops.step_guard_(out[:1], guard, 1)
        return int(guard[0])
    assert live(base) == 1 and float(out[1]) == 1.0
    for at in sorted({0, n // 2, n - 1}):
        for bad in (NAN, INF, -INF):
            x = base.clone()
            x[at] = bad
            assert live(x) == 0, (at, bad)
    assert live(torch.full((n,), 3e38, device="cuda")) == 0


# ------------------------------------------------------------------------------------------------ 3. bf_nonfinite_scan
SEVERAL_SLABS = 4 * 3072 + 402          # 3172 16-byte groups: four slabs of 1024, the last one short, and a tail of two


@pytest.mark.parametrize("n", SIZES + [SEVERAL_SLABS])
def test_nonfinite_scan_equals_the_restatement(n):
    from bubbleformer_amd import ops
    assert R.slabs(SEVERAL_SLABS) == 4
    base = torch.randn(n, generator=torch.Generator().manual_seed(n % 991)).numpy()
    edge = 4 * R.slab_groups(n)          # the first element of the second slab
    plants = [[], [0], [n - 1], [n // 3, n - 1], [n - 1, n // 3, n // 2]]
    if R.slabs(n) > 1:
        plants += [[edge - 1, edge], [edge], [edge - 1]]
        last = 4 * R.slab_groups(n) * (R.slabs(n) - 1)
        plants += [[last - 1, last]]
    ws = ops.nonfinite_scan_workspace(n, "cuda")
    assert ws.numel() == 2 * R.slabs(n)
    for k, where in enumerate(plants):
        x = base.copy()
        for j, i in enumerate(where):
            x[i] = (np.nan, np.inf, -np.inf)[(j + k) % 3]
        want = R.scan(x)
        assert want == ((min(where), len(set(where))) if where else (-1, 0))
        dev = torch.from_numpy(x).cuda()
        ws.fill_(-7)                     # the result does not depend on what the workspace held
        a = ops.nonfinite_scan(dev, ws=ws)
        b = ops.nonfinite_scan(dev)
        assert tuple(a.tolist()) == want, (n, where)
        assert torch.equal(a, b)
    everything = torch.full((n,), NAN, device="cuda")
    assert tuple(ops.nonfinite_scan(everything).tolist()) == (0, n)


# ------------------------------------------------------------------------------------------------ 4. TrainStep
def _tiny(name="filmavit", B=2):
    """(model, batches) as in test_gpu_grad_clip.py: a tiny model without stochastic depth and a function i -> (x, fluid, y) on the device."""
    from bubbleformer_amd.models import get_model
    from oracle import weights as W
    if name == "filmavit_bf16":          # the one geometry with a bit-reproducible step (test_gpu_baseline_configs.py), two blocks deep
        cfg = dict(SMALL, processor_blocks=2)
        model = get_model("filmavit", time_window=16, drop_path=0.0, compute_dtype=torch.bfloat16, **cfg)
        model.load_state_dict(W.generate(W.param_shapes(**cfg), seed=31))

        def data(i, B=B):
            return (W.synthetic_clip(B, 16, 4, 192, 192, 700 + i).cuda(), W.synthetic_fluid_params(B, 9, 900 + i).cuda(),
                    W.synthetic_clip(B, 16, 4, 192, 192, 800 + i).cuda())
        return model.cuda().train(), data
    if name == "filmavit":
        spec, _ = load_variant("tiny_d64")
        cfg = dict(spec["cfg"])
        model = get_model("filmavit", time_window=spec["T"], drop_path=0.0, compute_dtype=torch.float32, **cfg)
        model.load_state_dict(W.generate(W.param_shapes(**cfg), seed=spec["seed"]))

        def data(i, B=B):
            return (W.synthetic_clip(B, spec["T"], cfg["input_fields"], spec["H"], spec["W"], 700 + i).cuda(),
                    W.synthetic_fluid_params(B, cfg["num_fluid_params"], 900 + i).cuda(),
                    W.synthetic_clip(B, spec["T"], cfg["output_fields"], spec["H"], spec["W"], 800 + i).cuda())
        return model.cuda().train(), data
    from tests import unet_classic_restatement as U
    spec, _, p = U.load_golden("h8_c8_b3")
    cfg = spec["cfg"]
    model = get_model("unet_classic", compute_dtype=torch.float32, **cfg)
    model.load_state_dict({k: v.float() for k, v in p.items()}, strict=False)

    def data(i, B=B):
        g = torch.Generator().manual_seed(40 + i)
        return (torch.randn(B, cfg["time_window"], cfg["input_fields"], spec["H"], spec["W"], generator=g).cuda(), None,
                torch.randn(B, cfg["time_window"], cfg["output_fields"], spec["H"], spec["W"], generator=g).cuda())
    return model.cuda().train(), data


class _Poisoned:
    """LpLoss(pred, y) * poison, poison a device scalar that is 1 or NaN: a NaN gradient through ordinary arithmetic.  ``bad`` lists the
    calls (0-based) that are poisoned, or is True for all of them."""

    def __init__(self, bad=()):
        from bubbleformer_amd.utils.losses import LpLoss
        self.lp = LpLoss(d=2, p=2, reduce_dims=[0, 1, 2], reductions=["mean", "mean", "sum"])
        self.poison = torch.ones((), device="cuda")
        self.bad, self.calls = bad, 0

    def __call__(self, pred, y):
        self.poison.fill_(NAN if self.bad is True or self.calls in self.bad else 1.0)
        self.calls += 1
        return self.lp(pred, y) * self.poison


def _state(step):
    return [t.clone() for t in (step.flat.flat, step.m, step.v, step.avg) if t is not None]


CLIPS = {"none": {}, "norm": dict(gradient_clip_val=1.0), "value": dict(gradient_clip_val=0.01, gradient_clip_algorithm="value")}


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("clip", sorted(CLIPS))
@pytest.mark.parametrize("name", ["filmavit", "unet_classic"])
def test_a_poisoned_step_is_skipped_and_training_goes_on(name, clip, k):
    """Optimizer steps clean, poisoned, clean (k micro-batches each, the poison in the first of its group): the poisoned step leaves
    parameters, moments and average as step 1 left them, is counted, and everything is finite at the end.  Without the guard the same calls
    leave non-finite parameters: the behaviour the guard removes."""
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.averaging import AverageSpec
    from bubbleformer_amd.utils.guard import GuardSpec
    kw = dict(lr=1e-3, weight_decay=1e-2, optimizer="adamw", accumulate_grad_batches=k, weight_average=AverageSpec("ema", 0.9), **CLIPS[clip])
    model, data = _tiny(name)
    crit = _Poisoned(bad=(k,))
    step = TrainStep(model, criterion=crit, step_guard=GuardSpec(), **kw)
    assert (step.guard_norm is None) == (clip == "norm") and tuple(step.guard.tolist()) == R.FRESH
    names = {n for n, _ in model.named_parameters()}
    call = 0
    for _ in range(k):
        step(*data(call)); call += 1
    after_one = _state(step)
    assert step.guard_counts() == {"skipped": 0, "consecutive": 0, "last_skipped_step": -1}
    for _ in range(k):
        step(*data(call)); call += 1
    witness = step.grad_norm if clip == "norm" else step.guard_norm
    assert step.step_no == 2 and not bool(torch.isfinite(witness[0]))
    assert all(torch.equal(a, b) for a, b in zip(_state(step), after_one)) and len(after_one) == 4
    assert step.guard_counts() == {"skipped": 1, "consecutive": 1, "last_skipped_step": 2}
    found = step.diagnose()
    assert found["buffer"] == "gradient" and found["count"] > 0 and found["index"] >= 0
    assert found["parameter"].replace("padding after ", "") in names
    for _ in range(k):
        step(*data(call)); call += 1
    assert step.step_no == 3 and step.guard_counts() == {"skipped": 1, "consecutive": 0, "last_skipped_step": 2}
    assert all(bool(torch.isfinite(t).all()) for t in _state(step))
    assert not torch.equal(step.flat.flat, after_one[0])
    assert step.diagnose() == {"buffer": None, "parameter": None, "index": -1, "count": 0}
    # the same calls without the guard
    model, data = _tiny(name)
    bare = TrainStep(model, criterion=_Poisoned(bad=(k,)), **kw)
    assert bare.guard is None
    for i in range(3 * k):
        bare(*data(i))
    assert not bool(torch.isfinite(bare.flat.flat).all()) and not bool(torch.isfinite(bare.avg).all())
    assert bare.diagnose()["buffer"] == "parameters"


# ------------------------------------------------------------------------------------------------ 5. continuation
@pytest.mark.parametrize("optimizer", ["adamw", "lion"])
def test_training_continues_exactly_as_if_the_skipped_step_had_only_been_counted(optimizer):
    """Where the step is bit-reproducible: clean, poisoned, clean with the guard equals clean batch 1, the host counters advanced by
    hand, clean batch 3 without it -- parameters and moments torch.equal.  The poisoned batch is one whose target holds a NaN: the fused
    loss, hence every gradient, is NaN while the forward pass is the clean one."""
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.guard import GuardSpec
    from bubbleformer_amd.utils.lr_schedulers import CosineWarmupLR

    def make(**kw):
        model, data = _tiny("filmavit_bf16")
        return TrainStep(model, lr=1e-3, weight_decay=1e-2, optimizer=optimizer, scheduler=CosineWarmupLR(1e-3, 2, 10, 1e-6), **kw), data
    step, data = make(step_guard=GuardSpec())
    step(*data(0))
    x, c, y = data(1)
    y[0, 0, 0, 0, 0] = NAN
    loss = step(x, c, y)
    step(*data(2))
    assert not bool(torch.isfinite(loss)) and step.guard_counts() == {"skipped": 1, "consecutive": 0, "last_skipped_step": 2}
    control, data = make()
    control(*data(0))
    control.step_no += 1
    control.scheduler.step()
    control(*data(2))
    torch.cuda.synchronize()
    assert step.step_no == control.step_no == 3
    assert torch.equal(step.flat.flat, control.flat.flat) and torch.equal(step.m, control.m)
    assert (step.v is None and control.v is None) or torch.equal(step.v, control.v)
    assert bool(torch.isfinite(step.flat.flat).all())


# ------------------------------------------------------------------------------------------------ 6. groups
def test_a_nan_in_a_frozen_group_does_not_skip():
    from bubbleformer_amd import ops
    n = 4160
    chunks = (n + 63) // 64
    cmap = (torch.arange(chunks) >= chunks // 2).to(torch.uint8)          # the second half of the buffer is group 1, frozen
    groups = ops.param_group_tables(cmap, [1.0, 1.0], [0.0, 0.0], [False, True], n, "cuda")
    base = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    out = torch.zeros(2, device="cuda")

    def record(at):
        x = base.clone()
        x[at] = NAN
        guard = torch.tensor(R.FRESH, dtype=torch.int32, device="cuda")
        ops.group_clip_coef_(ops.group_sumsq(x, groups), groups, out, INF, 1.0)
        ops.step_guard_(out[:1], guard, 9)
        return tuple(guard.tolist())
    frozen_from = (chunks // 2) * 64
    assert record(frozen_from) == (1, 0, 0, -1) and record(n - 1) == (1, 0, 0, -1)
    assert record(frozen_from - 1) == (0, 1, 1, 9) and record(0) == (0, 1, 1, 9)


def test_train_step_with_groups_guards_on_the_live_groups_only():
    """TrainStep(param_groups=freeze(...), step_guard=...) without norm clipping: the guard's own norm is the one over the groups that
    are not frozen."""
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.guard import GuardSpec
    from bubbleformer_amd.utils.param_groups import freeze
    model, data = _tiny("filmavit")
    step = TrainStep(model, lr=1e-3, optimizer="lion", criterion=_Poisoned(bad=(1,)), param_groups=freeze(r"^blocks\."), step_guard=GuardSpec())
    assert step.groups is not None and step.guard_norm is not None and step.group_grad_norm is None
    step(*data(0))
    before = _state(step)
    step(*data(1))
    assert step.guard_counts() == {"skipped": 1, "consecutive": 1, "last_skipped_step": 2}
    assert all(torch.equal(a, b) for a, b in zip(_state(step), before))
    step(*data(2))
    assert step.guard_counts()["consecutive"] == 0 and bool(torch.isfinite(step.flat.flat).all())


# ------------------------------------------------------------------------------------------------ 7. fit
def _fit_run(tmp=None, **extra):
    from bubbleformer_amd.data.dataset import BubbleForecast
    from bubbleformer_amd.fit import fit
    from bubbleformer_amd.models import get_model
    g = np.random.default_rng(9)
    names = ["dfun", "temperature", "velx", "vely"]
    trajs = [{n: g.standard_normal((L, 16, 32)).astype(np.float32) for n in names} for L in (30, 21)]
    ds = BubbleForecast.from_arrays(trajs, input_fields=names, output_fields=names, norm="std", time_window=2, start_time=1)
    ds.normalize()
    torch.manual_seed(0)
    model = get_model("avit", input_fields=4, output_fields=4, time_window=2, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=1,
                      drop_path=0.0, compute_dtype=torch.float32).cuda()
    events = []
    log = extra.pop("log", events.append)
    hist = fit(model, ds, None, batch_size=4, max_epochs=2, optimizer="adamw", lr=1e-3, weight_decay=1e-2, warmup_iters=2, limit_train_batches=3,
               seed=42, log=log, **extra)
    torch.cuda.synchronize()
    return hist, torch.cat([p.detach().flatten() for p in model.parameters()]).clone(), events, model


def test_fit_marks_the_skipped_step_and_checkpoints_carry_the_count(tmp_path):
    from bubbleformer_amd.utils.guard import GuardSpec
    ck, ck0 = str(tmp_path / "last.ckpt"), str(tmp_path / "after_epoch0.ckpt")
    events = []

    def log(e):
        events.append(e)
        if e.get("epoch") == 1 and e.get("batch_idx") == 0:
            shutil.copy(ck, ck0)
    hist, params, _, _ = _fit_run(criterion=_Poisoned(bad=(2,)), step_guard=GuardSpec(), checkpoint_path=ck, log=log)
    assert hist["skipped"] == [0, 0, 1, 0, 0, 0] and len(hist["guard_norm"]) == 6 and "grad_norm" not in hist
    assert [bool(np.isfinite(v)) for v in hist["guard_norm"]] == [True, True, False, True, True, True]
    assert [bool(np.isfinite(v)) for v in hist["train_loss"]] == [True, True, False, True, True, True]
    assert np.isfinite(hist["epoch_train_loss"]).all()
    assert abs(hist["epoch_train_loss"][0] - np.mean(hist["train_loss"][:2])) <= 1e-6 * abs(hist["epoch_train_loss"][0])
    stepped = [e for e in events if "live" in e]
    assert len(stepped) == 6 and all(e["live"].is_cuda and e["live"].dim() == 0 for e in stepped)
    assert [int(e["live"]) for e in stepped] == [1, 1, 0, 1, 1, 1]
    assert bool(torch.isfinite(params).all())
    assert torch.load(ck0, weights_only=False)["step_guard"] == {"skipped": 1}
    assert torch.load(ck, weights_only=False)["step_guard"] == {"skipped": 1}
    # a resumed run continues the count: epoch 1 again, its second batch poisoned
    ck2 = str(tmp_path / "resumed.ckpt")
    h2, p2, _, _ = _fit_run(criterion=_Poisoned(bad=(1,)), step_guard=GuardSpec(), resume_from=ck0, checkpoint_path=ck2)
    assert h2["skipped"] == [0, 1, 0] and bool(torch.isfinite(p2).all())
    assert torch.load(ck2, weights_only=False)["step_guard"] == {"skipped": 2}
    # a file without the key loads as zero, and a step without a guard ignores the key
    saved = torch.load(ck0, weights_only=False)
    del saved["step_guard"]
    bare = str(tmp_path / "no_key.ckpt")
    torch.save(saved, bare)
    _fit_run(criterion=_Poisoned(), step_guard=GuardSpec(), resume_from=bare, checkpoint_path=ck2)
    assert torch.load(ck2, weights_only=False)["step_guard"] == {"skipped": 0}
    h3, _, _, _ = _fit_run(criterion=_Poisoned(), resume_from=ck0, checkpoint_path=ck2)
    assert "skipped" not in h3 and "step_guard" not in torch.load(ck2, weights_only=False)


def test_fit_stops_a_run_that_only_skips_before_it_writes_a_checkpoint(tmp_path):
    from bubbleformer_amd.utils.guard import GuardSpec
    ck = str(tmp_path / "last.ckpt")
    with pytest.raises(FloatingPointError) as err:
        _fit_run(criterion=_Poisoned(bad=True), step_guard=GuardSpec(max_consecutive=2), checkpoint_path=ck)
    msg = str(err.value)
    from bubbleformer_amd.models import get_model
    names = [n for n, _ in get_model("avit", input_fields=4, output_fields=4, time_window=2, patch_size=4, embed_dim=64, num_heads=2,
                                     processor_blocks=1, drop_path=0.0, compute_dtype=torch.float32).named_parameters()]
    assert "gradient" in msg and any(n in msg for n in names), msg
    assert "streak of 3" in msg
    assert not os.path.exists(ck) and os.listdir(tmp_path) == []
    # max_consecutive=None never raises: the run skips every step, and says so
    hist, params, _, _ = _fit_run(criterion=_Poisoned(bad=True), step_guard=GuardSpec(max_consecutive=None))
    assert hist["skipped"] == [1] * 6 and bool(torch.isfinite(params).all())


def test_fit_without_a_guard_is_the_run_it_was():
    """step_guard=None: the history's keys and values and the parameters of a second plain run (this geometry's step repeats bit for
    bit: test_gpu_unroll_step.py compares two plain runs of it the same way)."""
    h0, p0, e0, _ = _fit_run()
    h1, p1, e1, _ = _fit_run(step_guard=None)
    assert h0.keys() == h1.keys() and "skipped" not in h0 and "guard_norm" not in h0
    assert h0 == h1 and torch.equal(p0, p1)
    assert all("live" not in e for e in e0 + e1)
