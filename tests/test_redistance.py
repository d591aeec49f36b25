"""CPU: the numpy restatement of redistancing (tests/redistance_restatement.py) against itself and against the properties a
redistanced field must have, and the declarations of the new entry points (include/bubbleformer_hip.h, _lib.SIGNATURES, ops, utils)."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import redistance_restatement as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H0 = 1.0 / 32
SHAPES = [(48, 40), (33, 7), (1, 37), (37, 1), (2, 2)]


@pytest.mark.parametrize("shape", SHAPES + [(24, 24)])
def test_the_two_restatements_agree(shape):
    """Fast sweeping and red-black passes reach the same fixed point: 1e-12 absolute (the values are below 3; fp64 rounding along a chain of at
    most H + W cells is some 1e-14)."""
    H, W = shape
    worst = 0.0
    for name, phi in R.fields(H, W, H0).items():
        for band in (None, 8 * H0):
            a, ra = R.redistance_rb(phi, H0, band)
            b, rb = R.redistance_sweep(phi, H0, band)
            assert (ra > 0) == (rb > 0) and (ra > 0 or ra == rb), (name, band, ra, rb)
            worst = max(worst, float(np.abs(a - b).max()))
            assert np.abs(a - b).max() <= 1e-12, (name, band)
    print(f"{H}x{W}: worst gap between the two restatements {worst:.1e}")


@pytest.mark.parametrize("shape", [(48, 40), (64, 64), (33, 7)])
def test_a_distorted_disc_comes_back_a_signed_distance(shape):
    H, W = shape
    true = R.circles(H, W, H0, R.single_disc(H, W, H0))
    phi = R.distort(true).astype(np.float32)
    d, rounds = R.redistance_rb(phi, H0)
    err = float(np.abs(d - true).max()) / H0
    before, after = R.eikonal_l1(phi, H0), R.eikonal_l1(d, H0)
    moved = float(np.abs(R.crossings(d) - R.crossings(phi)).max())
    print(f"{H}x{W}: max |d - true| {err:.3f} h, Eikonal L1 {before:.3f} -> {after:.3f}, crossings moved by at most {moved:.3f} cell, {rounds} passes")
    assert rounds >= 1
    assert err <= 1.0
    assert after <= 0.05 and after <= 0.1 * before
    assert moved <= 0.1


@pytest.mark.parametrize("shape", SHAPES)
def test_signs_and_interface_cells_are_the_inputs(shape):
    H, W = shape
    for name, phi in R.fields(H, W, H0).items():
        for band in (None, 8 * H0):
            d, rounds = R.redistance_rb(phi, H0, band)
            if rounds > 0:
                assert np.array_equal(np.signbit(d), ~R.vapour(phi)), name
                assert np.array_equal(R.interface_cells(np.where(np.signbit(d), -1.0, 1.0)), R.interface_cells(phi)), name
                assert np.isfinite(d).all() and (band is None or np.abs(d).max() <= 8 * H0), name
            else:
                assert np.array_equal(d, phi.astype(np.float64)), name


def test_status_values():
    H, W = 12, 9
    one_sign = np.full((H, W), -0.3, np.float32)
    for f in (R.redistance_rb, R.redistance_sweep):
        out, rounds = f(one_sign, H0)
        assert rounds == 0 and np.array_equal(out, one_sign)
        out, rounds = f(np.zeros((H, W), np.float32), H0)                   # exact zeros are liquid: one sign
        assert rounds == 0
        for bad in (np.nan, np.inf, -np.inf):
            phi = R.corner(H, W, H0).astype(np.float32)
            phi[5, 4] = bad
            out, rounds = f(phi, H0)
            assert rounds == -1 and np.array_equal(out, phi.astype(np.float64), equal_nan=True)
        phi = R.corner(H, W, H0).astype(np.float32)
        out, rounds = f(phi, H0, None, 3) if f is R.redistance_rb else f(phi, H0, None, 1)
        assert rounds == -2 and np.isfinite(out).all()
        if f is R.redistance_rb:
            assert out[-1, -1] == -(H + W) * H0                             # a cell no pass reached (one pass of four sweeps reaches them all)
        out, rounds = f(phi, H0, 2 * H0, 1)
        assert rounds == -2 and out[-1, -1] == -2 * H0
    assert R.change_rms(one_sign, one_sign) == 0.0


@pytest.mark.parametrize("shape,passes", [((64, 64), 64), ((48, 40), 44), ((96, 24), 60)])
def test_the_corner_frame_needs_half_the_default_limit(shape, passes):
    """One vapour cell in a corner, visited red-black: (H + W) / 2 passes, the worst case found; the default max_rounds = H + W is twice that."""
    H, W = shape
    for dtype in (np.float64, np.float32):
        assert R.redistance_rb(R.corner(H, W, H0).astype(np.float32), H0, dtype=dtype)[1] == passes == (H + W) // 2


NEW = ["bf_redistance_lds_cells", "bf_redistance_ws_bytes", "bf_redistance", "bf_rollout_redistance"]


def _lib_handle():
    from bubbleformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib, _lib.lib()


def test_entry_points_are_declared_and_bound():
    """test_abi_exports.py compares the header, the library and _lib.SIGNATURES as sets; this names the new members of all three, holds every ctypes
    argument list to the header's parameter list type by type, and runs the argument checks that come before any HIP call."""
    import ctypes as C
    _lib, h = _lib_handle()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "bubbleformer_hip.h")).read(), flags=re.S)
    scalar = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float}
    for name in NEW:
        m = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)" % name, txt)
        assert m, name
        assert name in _lib.SIGNATURES and hasattr(h, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is {"int": C.c_int, "int64_t": C.c_int64}[m.group(1)], name
        params = [p.strip() for p in m.group(2).split(",")] if m.group(2).strip() != "void" else []
        assert len(params) == len(args), name
        for p, a in zip(params, args):
            if "*" in p:
                assert a is C.c_void_p or a is C.POINTER(_lib.RolloutStep), (name, p)
            elif p.split()[0] == "bf_stream_t":
                assert a is C.c_void_p, (name, p)
            else:
                assert a is scalar[p.split()[0]], (name, p)
    cells = h.bf_redistance_lds_cells()
    assert 36864 <= cells and cells * 4 < 160 * 1024                        # a 192 x 192 frame fits, with room for the statics
    assert h.bf_redistance_ws_bytes(0, 8, 8) == 0 and h.bf_redistance_ws_bytes(1, 0, 8) == 0 and h.bf_redistance_ws_bytes(1, 4096, 4097) == 0
    assert h.bf_redistance_ws_bytes(3, 8, 8) == 16 and h.bf_redistance_ws_bytes(1, 4096, 4096) == 4 << 24
    side = int(np.sqrt(cells)) + 1
    assert h.bf_redistance_ws_bytes(5, side, side) == 5 * ((4 * side * side + 15) // 16 * 16)
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    assert h.bf_redistance(None, 1, 4, 4, 1.0, 0.0, 0, p, None, None, p, 64, None) != 0
    assert h.bf_last_error().decode().endswith("bf_redistance: null pointer")
    assert h.bf_redistance(p, 1, 4097, 4096, 1.0, 0.0, 0, p, None, None, p, 1 << 40, None) != 0
    assert h.bf_last_error().decode().endswith("bf_redistance: a frame may have at most 2^24 cells")
    side_bytes = h.bf_redistance_ws_bytes(1, side, side)
    assert h.bf_redistance(p, 1, side, side, 1.0, 0.0, 0, p, None, None, p, side_bytes - 1, None) != 0
    assert h.bf_last_error().decode().endswith("bf_redistance: workspace smaller than bf_redistance_ws_bytes")
    assert h.bf_redistance(p, 1, 4, 4, 0.0, 0.0, 0, p, None, None, p, 64, None) != 0
    step = _lib.RolloutStep(pred=p, frames=p, field_stride=64, total_frames=4, first=p, step=p, field=p, diff=p, div=p, nfields=1, B=1, T=2, C=1, H=4, W=4,
                            Ho=4, Wo=4, steps=1)
    for rec, pred in ((None, p), (C.byref(step), None)):
        assert h.bf_rollout_redistance(rec, 0, 1.0, 0.0, 0, 1, pred, None, None, p, 64, None) != 0
        assert h.bf_last_error().decode().endswith("bf_rollout_redistance: null pointer")
    assert h.bf_rollout_redistance(C.byref(step), 0, 1.0, 0.0, 0, 0, p, None, None, p, 64, None) != 0       # every = 0
    assert h.bf_last_error().decode().endswith("bf_rollout_redistance: bad sizes")
    assert h.bf_rollout_redistance(C.byref(step), 1, 1.0, 0.0, 0, 1, p, None, None, p, 64, None) != 0       # channel 1 of 1
    assert h.bf_rollout_redistance(C.byref(step), 0, 1.0, 0.0, 0, 1, p + 16, None, None, p, 64, None) != 0  # not the tensor the record names


def test_python_surface():
    import torch
    from bubbleformer_amd import _lib, ops, utils
    from bubbleformer_amd.utils import physics
    from bubbleformer_amd.utils.rollout import RolloutReport, evaluate_rollouts
    for fn in (ops.redistance, ops.redistance_workspace, ops.redistance_lds_cells, ops.rollout_redistance):
        assert callable(fn)
    assert utils.redistance is physics.redistance and utils.RedistanceSpec is physics.RedistanceSpec
    spec = physics.RedistanceSpec()
    assert (spec.dx, spec.band, spec.max_rounds, spec.every, spec.sdf_field) == (1 / 32, None, None, 1, "dfun")
    assert list(inspect.signature(physics.redistance).parameters) == ["phi", "dx", "band", "max_rounds", "out", "return_status"]
    for bad in (dict(dx=0.0), dict(dx=-1.0), dict(band=0.0), dict(band=-1.0), dict(every=0), dict(every=1.5), dict(max_rounds=0)):
        with pytest.raises(ValueError):
            physics.RedistanceSpec(**bad)
    assert physics.RedistanceSpec(band=0.25, every=3, max_rounds=7).channel(["temperature", "dfun"]) == 1
    with pytest.raises(ValueError):
        spec.channel(["temperature", "velx"])
    from bubbleformer_amd.utils.rollout import evaluate_rollouts_redistanced
    assert list(inspect.signature(evaluate_rollouts_redistanced).parameters) == ["model", "data", "starts", "steps", "redistance", "options"]
    assert "redistance" not in inspect.signature(evaluate_rollouts).parameters      # that list is held as it is (tests/test_ensemble.py)
    with pytest.raises(TypeError):
        evaluate_rollouts_redistanced(None, None, [0], 1, None, no_such_option=1)    # the options are evaluate_rollouts' own
    with pytest.raises(ValueError):
        physics.redistance(torch.zeros(2, 0, 4))                            # a zero-sized axis: refused before any reshape
    assert RolloutReport.redistance_rounds is None and RolloutReport.redistance_change is None
    phi = torch.zeros(1, 4, 4)
    with pytest.raises(_lib.BubbleformerHipError):
        physics.redistance(phi)                                             # no CPU path
    with pytest.raises(_lib.BubbleformerHipError):
        ops.redistance(phi, 1 / 32, None, None, torch.empty(16, dtype=torch.uint8), torch.empty_like(phi))
    with pytest.raises(_lib.BubbleformerHipError):
        ops.redistance_workspace(1, 4096, 4097, "cpu")
    with pytest.raises(ValueError):
        physics.redistance(torch.zeros(4))
    with pytest.raises(ValueError):
        physics.redistance(phi, dx=0.0)
