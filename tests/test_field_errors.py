"""CPU: the numpy restatement of the error rows checks itself (Parseval, the integer shell table, the shell count), and the new interface
is declared, bound and validated.  tests/test_gpu_field_errors.py holds the kernels to this restatement."""
import inspect
import math

import numpy as np
import pytest

from tests import errors_restatement as R

SHAPES = [(1, 1), (1, 8), (8, 1), (2, 3), (5, 8), (7, 22), (12, 18), (16, 16), (31, 64), (30, 50), (64, 64)]


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_parseval(shape):
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    for x in (R.smooth(H, W, rng), rng.standard_normal((H, W))):
        power = R.shell_power(x)
        assert power.shape == (R.shell_count(H, W),)
        assert abs(power.sum() - np.mean(x * x)) <= 1e-12 * np.mean(x * x)


def test_shell_table_is_the_floored_radius_on_square_frames_and_k_covers_every_mode():
    for n in (1, 2, 3, 7, 16, 31, 64):
        f = np.array([k if k <= n // 2 else k - n for k in range(n)])
        want = np.array([[math.isqrt(int(a * a + b * b)) for b in f] for a in f])
        assert np.array_equal(R.shell_table(n, n), want), n
    for H in range(1, 41):
        for W in range(1, 41):
            table = R.shell_table(H, W)
            assert 0 <= table.min() and table.max() <= R.shell_count(H, W) - 1, (H, W)
            assert table[0, 0] == 0


def test_interface_mask_and_ring():
    sdf = -np.ones((6, 7), np.float32)
    sdf[2, 3] = 1.0
    m = R.interface_mask(sdf, 1)
    assert m.sum() == 9 and m[1:4, 2:5].all()
    assert R.interface_mask(sdf, 2).sum() == 25 and not R.interface_mask(-np.abs(sdf), 1).any()
    sdf[2, 3] = np.nan                                                                # NaN and an exact zero are liquid
    assert not R.interface_mask(sdf, 1).any()
    assert R.ring_mask(1, 5).all() and R.ring_mask(5, 1).all() and R.ring_mask(4, 5).sum() == 14


def test_error_spec_validation():
    from bubbleformer_amd.utils import ErrorSpec, shell_count
    spec = ErrorSpec()
    assert (spec.interface_radius, tuple(spec.bands), spec.spectra, spec.sdf_field) == (1, (4, 12), True, "dfun")
    ErrorSpec(interface_radius=3, bands=(0, 0))
    ErrorSpec(bands=(5, 5), spectra=False)
    for bad in (dict(interface_radius=0), dict(interface_radius=-1), dict(interface_radius=1.5), dict(bands=(5, 4)), dict(bands=(-1, 4)),
                dict(bands=(1, 2, 3)), dict(bands=4)):
        with pytest.raises(ValueError):
            ErrorSpec(**bad)
    assert [shell_count(H, W) for H, W in ((1, 1), (64, 64), (192, 192), (3, 1024), (1024, 1024))] == [1, 46, 136, 3, 725]
    assert all(shell_count(H, W) == R.shell_count(H, W) for H in range(1, 30) for W in range(1, 30))


def test_new_symbols_are_declared_and_bound():
    from bubbleformer_amd import _lib, ops
    h = _lib.lib()
    for name in ("bf_field_errors_ws_bytes", "bf_field_errors", "bf_rollout_errors"):
        assert name in _lib.SIGNATURES and hasattr(h, name)
    assert h.bf_abi_version() == 3
    assert h.bf_field_errors_ws_bytes(0, 8, 8) == 0 and h.bf_field_errors_ws_bytes(1, 8, 1025) == 0 and h.bf_field_errors_ws_bytes(1, 0, 8) == 0
    one, two = h.bf_field_errors_ws_bytes(1, 1024, 1024), h.bf_field_errors_ws_bytes(2, 1024, 1024)
    assert 0 < one < two and one % 16 == 0
    for fn in (ops.field_errors_workspace, ops.field_errors, ops.rollout_errors):
        assert callable(fn)
    with pytest.raises(_lib.BubbleformerHipError):
        ops.field_errors_workspace(1, 8, 2048, "cpu")


def test_evaluate_rollouts_takes_errors_and_the_report_has_the_rows():
    import torch
    from bubbleformer_amd.utils.rollout import RolloutReport, evaluate_rollouts
    assert inspect.signature(evaluate_rollouts).parameters["errors"].default is None
    bare = RolloutReport(torch.zeros(1, 2, 1), torch.zeros(1, 1), None, None, torch.zeros(1, 2, dtype=torch.int64), ["dfun"])
    for key in ("rmse", "max_error", "boundary_rmse", "interface_rmse", "interface_cells", "spectral_error", "spectrum_error", "spectrum_pred",
                "spectrum_target"):
        assert getattr(bare, key) is None, key
    with pytest.raises(ValueError, match="spectra"):
        bare.spectral_ratio()
    bare.spectrum_pred, bare.spectrum_target = torch.full((1, 2, 1, 3), 2.0), torch.full((1, 2, 1, 3), 4.0)
    assert torch.equal(bare.spectral_ratio(), torch.full((1, 2, 1, 3), 0.5)) and RolloutReport.spectrum_pred is None
    assert callable(RolloutReport.spectral_ratio)
