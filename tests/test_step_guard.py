"""CPU: the step guard's specification, the restatement the GPU tests compare against, and every refusal the new entry points make before
any HIP call (no GPU needed: host buffers nothing reads)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import step_guard_restatement as R


def _lib():
    from bubbleformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ GuardSpec
def test_guard_spec_validates_its_field():
    from bubbleformer_amd.utils.guard import GuardSpec
    assert GuardSpec().max_consecutive == 16 and GuardSpec(None).max_consecutive is None and GuardSpec(1).max_consecutive == 1
    for bad in (0, -3, 2.0, True, "4"):
        with pytest.raises(ValueError, match="max_consecutive"):
            GuardSpec(bad)
    with pytest.raises(Exception):
        GuardSpec().max_consecutive = 3          # frozen
    s = GuardSpec(2)
    assert [s.tripped(c) for c in (0, 1, 2, 3)] == [False, False, True, True]
    assert not GuardSpec(None).tripped(10 ** 6)


def test_train_step_refuses_what_is_not_a_guard_spec():
    import torch
    from bubbleformer_amd.trainer import TrainStep
    with pytest.raises(ValueError, match="step_guard"):
        TrainStep(torch.nn.Linear(2, 2), step_guard=16)


def test_train_step_without_a_guard_has_no_record():
    import torch
    from bubbleformer_amd.trainer import TrainStep
    step = TrainStep(torch.nn.Linear(3, 2), step_guard=None)
    assert step.guard is None and step.guard_norm is None and step.step_guard is None
    with pytest.raises(RuntimeError, match="no guard"):
        step.guard_counts()


def test_locate_names_parameters_and_their_padding():
    from bubbleformer_amd.utils.guard import locate
    names, offsets, numels = ["a.weight", "a.bias", "b"], [0, 64, 128], [6, 64, 1]
    assert locate(0, names, offsets, numels) == "a.weight" and locate(5, names, offsets, numels) == "a.weight"
    assert locate(6, names, offsets, numels) == "padding after a.weight" and locate(63, names, offsets, numels) == "padding after a.weight"
    assert locate(64, names, offsets, numels) == "a.bias" and locate(127, names, offsets, numels) == "a.bias"
    assert locate(128, names, offsets, numels) == "b" and locate(191, names, offsets, numels) == "padding after b"


# ------------------------------------------------------------------------------------------------ the restatement
def test_restated_record_transitions():
    flt_max = float(np.finfo(np.float32).max)
    assert [R.guard_update(R.FRESH, x, 7)[0] for x in (1.0, 0.0, flt_max, float("inf"), float("nan"))] == [1, 1, 1, 0, 0]
    assert R.guard_update(R.FRESH, 1e39, 7) == (0, 1, 1, 7)          # finite in fp64, inf once rounded to fp32: skipped, as documented
    run = R.guard_run([1.0, float("nan"), float("inf"), 2.0, float("nan")], first_step=10)
    assert [r[1] for r in run] == [0, 1, 2, 0, 1] and [r[2] for r in run] == [0, 1, 2, 2, 3]
    assert [r[3] for r in run] == [-1, 11, 12, 12, 14] and [r[0] for r in run] == [1, 0, 0, 1, 0]


def test_restated_scan_and_slab_rule():
    x = np.arange(10, dtype=np.float32)
    assert R.scan(x) == (-1, 0)
    x[7] = np.inf; x[3] = np.nan; x[9] = -np.inf
    assert R.scan(x) == (3, 3)
    assert R.slabs(3) == 1 and R.slabs(4160) == 2 and R.slab_groups(4160) == 1024
    n = 4 * 256 * 4096 + 4 * 1024 + 3
    assert R.slab_groups(n) == 1280 and R.slabs(n) == 820
    h = _lib()
    for m in (1, 3, 67, 4160, 4 * 3072 + 402, n):
        assert h.bf_nonfinite_scan_ws_len(m) == 2 * R.slabs(m) == 2 * h.bf_grad_norm_ws_doubles(m)
    assert h.bf_nonfinite_scan_ws_len(0) == 0


# ------------------------------------------------------------------------------------------------ refusals before any HIP call
_BUF = (C.c_char * 160)()


def _aligned():
    return (C.addressof(_BUF) + 15) // 16 * 16


def _opt_step(**kw):
    """A bf_opt_step every check accepts (the pattern of test_abi_exports.py), with `kw` over it."""
    from bubbleformer_amd import _lib as L
    p = _aligned()
    good = dict(p=p, g=p + 16, m=p + 32, v=p + 48, coef_dev=p + 64, avg=p + 80, chunk_group=p + 96, group_lr_scale=p + 100, group_weight_decay=p + 104,
                group_frozen=p + 108, live_dev=p + 112, n=4, step=1, n_groups=1, lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8, wd=0.0, gscale=1.0,
                clip_value=float("inf"), avg_weight=0.5)
    return L.OptStep(**{**good, **kw})


@pytest.mark.parametrize("name", ["bf_adamw", "bf_adam", "bf_lion"])
def test_optimizers_refuse_a_misaligned_guard_flag(name):
    h = _lib()
    assert getattr(h, name)(C.byref(_opt_step(live_dev=_aligned() + 114)), None) != 0
    assert (name + ": the guard flag must be 4-byte aligned") in h.bf_last_error().decode(), h.bf_last_error()
    # the flag's check comes after the others: a record with two defects names the earlier one
    assert getattr(h, name)(C.byref(_opt_step(live_dev=_aligned() + 114, n=0)), None) != 0
    assert (name + ": n must be positive") in h.bf_last_error().decode()


def test_step_guard_refuses_null_and_misaligned_pointers():
    h, p = _lib(), _aligned()
    for norm, guard, why in ((None, p + 16, "null pointer"), (p, None, "null pointer"), (p + 2, p + 16, "4-byte aligned"), (p, p + 18, "4-byte aligned")):
        assert h.bf_step_guard(norm, 1, guard, None) != 0
        msg = h.bf_last_error().decode()
        assert "bf_step_guard" in msg and why in msg, msg


def test_nonfinite_scan_refuses_bad_arguments():
    h, p = _lib(), _aligned()
    x, out, ws = p, p + 64, p + 80
    cases = [((None, 8, out, ws, 2), "null pointer"), ((x, 8, None, ws, 2), "null pointer"), ((x, 0, out, ws, 2), "n must be positive"),
             ((x, -4, out, ws, 2), "n must be positive"), ((x, 8, out, None, 2), "workspace"), ((x, 8, out, ws, 1), "workspace"),
             ((x, 4160, out, ws, 3), "workspace"), ((x + 4, 8, out, ws, 2), "16-byte aligned")]
    for args, why in cases:
        assert h.bf_nonfinite_scan(*args, None) != 0, args
        msg = h.bf_last_error().decode()
        assert "bf_nonfinite_scan" in msg and why in msg, (args, msg)


def test_records_built_without_live_have_a_null_flag():
    """ops._opt_step is the one place the wrappers build their record: without live= the member stays NULL, so the launch is the old one."""
    import torch
    from bubbleformer_amd import ops
    t = torch.zeros(8)
    rec = ops._opt_step("adamw_", t, t, t, t, 1, 1e-3, (0.9, 0.999), 1e-8, 0.0, 1.0, None, None, None, None, None)
    assert rec.live_dev is None and rec.n == 8
    flag = torch.ones(1, dtype=torch.int32)
    rec = ops._opt_step("lion_", t, t, t, None, 0, 1e-3, (0.9, 0.99), 0.0, 0.0, 1.0, None, None, None, None, None, live=flag)
    assert rec.live_dev == flag.data_ptr()
    from bubbleformer_amd._lib import BubbleformerHipError
    for bad in (torch.ones(1), torch.ones(2, dtype=torch.int32), 1):
        with pytest.raises(BubbleformerHipError, match="live must be one torch.int32"):
            ops._opt_step("adam_", t, t, t, t, 1, 1e-3, (0.9, 0.999), 1e-8, 0.0, 1.0, None, None, None, None, None, live=bad)


def test_wrappers_have_no_cpu_path():
    import torch
    from bubbleformer_amd import ops
    from bubbleformer_amd._lib import BubbleformerHipError
    with pytest.raises(BubbleformerHipError):
        ops.step_guard_(torch.zeros(1), torch.zeros(4, dtype=torch.int32), 1)
    with pytest.raises(BubbleformerHipError):
        ops.nonfinite_scan(torch.zeros(8))
