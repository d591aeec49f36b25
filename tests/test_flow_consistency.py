"""CPU: the flow-consistency rows -- the identities of the numpy restatement tests/flow_restatement.py, the counts on the
sample trajectories, FlowSpec's refusals, the pinned signatures, the report's attributes and methods, the ctypes record, and the refusals the two
entry points make before any HIP call."""
import ctypes as C
import dataclasses
import inspect
import os

import numpy as np
import pytest

from tests import flow_restatement as R
from tests.test_rollout_eval import FILES

DX, DT = 1.0 / 32, 1.0 / 4                           # dyadic, as every coefficient below: every intermediate is exact in fp64


def planar_front(T, H, W, a, b, u0, v0, c):
    """phi = a x + b y - (a u0 + b v0) t + c with x = j dx, y = i dx, t = k dt, carried by the uniform velocity (u0, v0): fp32, exactly."""
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    phi = np.stack([a * (j * DX) + b * (i * DX) - (a * u0 + b * v0) * (k * DT) + c for k in range(T)])
    assert np.array_equal(phi.astype(np.float32).astype(np.float64), phi)
    return phi.astype(np.float32), np.full((T, H, W), u0, dtype=np.float32), np.full((T, H, W), v0, dtype=np.float32)


def solid_body(T, H, W, omega, yc, xc):
    """u = -omega (y - yc), v = omega (x - xc) with x = j dx, y = i dx, and a signed distance that is liquid on the left half: fp32, exactly."""
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    u, v = -omega * (i * DX - yc), omega * (j * DX - xc)
    phi = (j - W // 2) * DX + 0.0 * i
    return tuple(np.broadcast_to(a.astype(np.float32), (T, H, W)).copy() for a in (phi, u, v))


PLANAR = dict(a=0.5, b=-0.25, u0=0.375, v0=1.0, c=-0.25)      # a u0 + b v0 = -0.0625: the front moves, and crosses a 16 x 24 frame
ROTATION = dict(omega=0.75, yc=0.25, xc=0.375)


def test_a_front_carried_by_its_velocity_has_no_residual():
    phi, u, v = planar_front(3, 16, 24, **PLANAR)
    rows = R.sequence_rows(phi, u, v, DX, DT, 3 * DX, 1)
    assert (rows["transport_cells"] > 0).all()
    assert (rows["transport_rms"] == 0.0).all()
    assert (rows["interface_speed_rms"] == abs(PLANAR["a"] * PLANAR["u0"] + PLANAR["b"] * PLANAR["v0"])).all()
    assert (rows["kinetic_energy"] == 0.5 * (PLANAR["u0"] ** 2 + PLANAR["v0"] ** 2)).all() and (rows["enstrophy"] == 0.0).all()
    still = R.sequence_rows(phi, 0 * u, 0 * v, DX, DT, 3 * DX, 1)                       # a velocity that explains nothing: the ratio is 1
    assert np.array_equal(still["transport_rms"], still["interface_speed_rms"])


def test_solid_body_rotation_is_divergence_free_with_enstrophy_two_omega_squared():
    phi, u, v = solid_body(2, 12, 20, **ROTATION)
    rows = R.sequence_rows(phi, u, v, DX, DT, 3 * DX, 1)
    assert (rows["bulk_cells"] == 10 * 9).all()                                        # columns 1 .. 9: column 10 holds phi = 0, which is liquid
    assert (rows["divergence_rms"] == 0.0).all()
    assert (rows["enstrophy"] == 2 * ROTATION["omega"] ** 2).all()


def test_masks_vapour_zero_and_nan():
    """Vapour is phi > 0 alone: a zero and a NaN are liquid; no bulk cell gives a NaN row and a count of 0, and only that row."""
    phi = np.full((5, 6), -1.0, dtype=np.float32)
    phi[2, 2], phi[2, 3] = 0.0, np.nan
    u = np.tile(np.arange(6, dtype=np.float32), (5, 1))
    v = np.zeros((5, 6), dtype=np.float32)
    rows = R.frame_rows(phi, u, v, DX, 1)
    assert rows["bulk_cells"] == 3 * 4 and rows["divergence_rms"] == 1 / DX
    phi[2, 3] = 1.0
    assert R.frame_rows(phi, u, v, DX, 1)["bulk_cells"] == 3
    rows = R.frame_rows(phi, u, v, DX, 3)
    assert rows["bulk_cells"] == 0 and np.isnan(rows["divergence_rms"]) and np.isfinite(rows["kinetic_energy"]) and rows["enstrophy"] == 0.0
    far = R.pair_rows((phi - 9, u, v), (phi - 9, u, v), DX, DT, 3 * DX)
    assert far["transport_cells"] == 0 and np.isnan(far["transport_rms"]) and np.isnan(far["interface_speed_rms"])


@pytest.mark.parametrize("which,band,bulk", [(0, (121, 155), (3203, 3307)), (1, (199, 242), (2857, 3036))])
def test_counts_on_the_sample_trajectories(which, band, bulk):
    """The masks of the two sample files at 64 x 64, dx = 1/32, band = 3 dx, r = 1: never empty, so a masked row over an empty mask cannot pass
    unnoticed."""
    from bubbleformer_amd.data import hdf5_lite
    f = hdf5_lite.File(FILES[which])
    phi, u, v = (np.asarray(f[k][...], dtype=np.float32) for k in ("dfun", "velx", "vely"))
    assert phi.shape[1:] == (64, 64)
    rows = R.sequence_rows(phi, u, v, DX, DT, 3 * DX, 1)
    assert (int(rows["transport_cells"].min()), int(rows["transport_cells"].max())) == band
    assert (int(rows["bulk_cells"].min()), int(rows["bulk_cells"].max())) == bulk
    assert np.isfinite(rows["transport_rms"]).all() and np.isfinite(rows["divergence_rms"]).all()


def test_denormalise_is_an_fp32_product_then_an_fp32_sum():
    x = np.array([0.1, -3.7, 1e-3], dtype=np.float32)
    got = R.denormalise(x, 1.7, 0.3)
    assert got.dtype == np.float32 and np.array_equal(got, (x * np.float32(1.7)).astype(np.float32) + np.float32(0.3))


@pytest.mark.parametrize("kw", [dict(dt=0.0), dict(dt=-1.0), dict(dt=0.25, dx=0.0), dict(dt=0.25, dx=-1 / 32), dict(dt=0.25, band=0.0),
                                dict(dt=0.25, band=-1.0), dict(dt=0.25, interface_radius=0), dict(dt=0.25, interface_radius=1.5)])
def test_flow_spec_refusals(kw):
    from bubbleformer_amd.utils import FlowSpec
    with pytest.raises(ValueError):
        FlowSpec(**kw)


def test_flow_spec():
    from bubbleformer_amd.utils import FlowSpec
    params = inspect.signature(FlowSpec).parameters
    assert list(params) == ["dt", "dx", "band", "interface_radius", "sdf_field", "velx_field", "vely_field"]
    assert params["dt"].default is inspect.Parameter.empty
    with pytest.raises(TypeError):
        FlowSpec()
    spec = FlowSpec(0.25)
    assert spec.dx == 1 / 32 and spec.band is None and spec.band_width() == 3 / 32 and FlowSpec(0.25, band=0.5).band_width() == 0.5
    assert spec.interface_radius == 1 and (spec.sdf_field, spec.velx_field, spec.vely_field) == ("dfun", "velx", "vely")
    with pytest.raises(dataclasses.FrozenInstanceError):
        spec.dt = 1.0
    assert spec.channels(["dfun", "temperature", "velx", "vely"]) == (0, 2, 3)
    assert FlowSpec(0.25, sdf_field="phi").channels(["vely", "velx", "phi"]) == (2, 1, 0)
    for missing in ("dfun", "velx", "vely"):
        with pytest.raises(ValueError, match=repr(missing)):
            spec.channels([f for f in ("dfun", "temperature", "velx", "vely") if f != missing])


def test_signatures():
    from bubbleformer_amd.utils import flow_consistency
    from bubbleformer_amd.utils.rollout import evaluate_rollouts, evaluate_rollouts_flow
    params = inspect.signature(evaluate_rollouts_flow).parameters
    assert list(params) == ["model", "data", "starts", "steps", "flow", "options"] and params["options"].kind is inspect.Parameter.VAR_KEYWORD
    assert params["flow"].default is inspect.Parameter.empty
    assert list(inspect.signature(evaluate_rollouts).parameters) == ["model", "data", "starts", "steps", "use_graph", "sdf_field", "keep_predictions",
                                                                     "heatflux", "bubbles", "errors", "ensemble"]
    params = inspect.signature(flow_consistency).parameters
    assert list(params) == ["sdf", "velx", "vely", "spec"] and params["spec"].kind is inspect.Parameter.KEYWORD_ONLY
    assert params["spec"].default is inspect.Parameter.empty


FLOW_ATTRIBUTES = [f"flow_{name}_{side}" for name in ("divergence", "bulk_cells", "kinetic_energy", "enstrophy", "transport", "interface_speed",
                                                      "transport_cells") for side in ("pred", "target")] + ["flow_dx", "flow_dt"]


def test_report_attributes_and_methods():
    import torch
    from bubbleformer_amd.utils import rollout
    names = [f.name for f in dataclasses.fields(rollout.RolloutReport)]
    assert names[-1] == "bubble_departure_area_target" and not any(n.startswith("flow") for n in names)
    report = rollout.RolloutReport(torch.zeros(1, 2, 1), torch.zeros(1, 1), None, None, torch.zeros(1, 2, dtype=torch.int64), ["dfun"])
    assert sorted(rollout._FLOW_KEYS) == sorted(FLOW_ATTRIBUTES)
    assert all(getattr(report, key) is None for key in FLOW_ATTRIBUTES)
    for method in ("transport_ratio", "energy_drift", "divergence_excess"):
        with pytest.raises(ValueError, match="flow"):
            getattr(report, method)()


def test_cpu_tensors_are_refused():
    import torch
    from bubbleformer_amd import _lib
    from bubbleformer_amd.utils import FlowSpec, flow_consistency
    z = torch.zeros(2, 4, 4)
    with pytest.raises(_lib.BubbleformerHipError):
        flow_consistency(z, z, z, spec=FlowSpec(0.25))
    with pytest.raises(ValueError):
        flow_consistency(z, z, torch.zeros(2, 4, 5), spec=FlowSpec(0.25))


def test_record_mirrors_the_header():
    from bubbleformer_amd import _lib
    from tests.test_abi_exports import _record_fields
    declared = _record_fields("bf_flow_rows")
    assert [n for n, _ in declared] == ["divergence_rms", "kinetic_energy", "enstrophy", "bulk_cells", "transport_rms", "interface_speed_rms",
                                        "transport_cells"]
    assert [(n, t) for n, t in _lib.FlowRows._fields_] == declared
    assert C.sizeof(_lib.FlowRows) == sum(C.sizeof(t) for _, t in declared)


def _library():
    from bubbleformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


_BUF = (C.c_char * 64)()


def _step(**kw):
    from bubbleformer_amd import _lib as L
    p = C.addressof(_BUF)
    return L.RolloutStep(**{**dict(pred=p, frames=p, field_stride=64, total_frames=4, first=p, step=p, field=p, diff=p, div=p, nfields=1, B=1, T=2, C=3,
                                   H=4, W=4, Ho=4, Wo=4, steps=1), **kw})


def test_flow_consistency_refusals_need_no_gpu():
    """Every check comes before the first HIP call: host pointers nothing reads, no GPU."""
    from bubbleformer_amd import _lib as L
    h, p, rows = _library(), C.addressof(_BUF), L.FlowRows()
    call = lambda sdf=p, velx=p, vely=p, T=2, H=4, W=4, dx=DX, dt=DT, band=3 * DX, r=1, rec=C.byref(rows): h.bf_flow_consistency(
        sdf, velx, vely, 1, T, H, W, dx, dt, band, r, rec, None)
    for kw in (dict(rec=None), dict(sdf=None), dict(velx=None), dict(vely=None)):
        assert call(**kw) != 0 and h.bf_last_error().decode().endswith("bf_flow_consistency: null pointer"), kw
    for kw in (dict(H=2), dict(W=2), dict(H=1025), dict(W=1025), dict(H=0), dict(W=-3)):
        assert call(**kw) != 0 and h.bf_last_error().decode().endswith("bf_flow_consistency: H and W must lie in [3, 1024]"), kw
    for kw in (dict(T=0), dict(dx=0.0), dict(dt=0.0), dict(dt=float("nan")), dict(band=0.0), dict(r=0)):
        assert call(**kw) != 0 and "bf_flow_consistency: " in h.bf_last_error().decode(), kw


def test_rollout_flow_refusals_need_no_gpu():
    from bubbleformer_amd import _lib as L
    h, p, rows = _library(), C.addressof(_BUF), L.FlowRows()
    ref = C.byref
    call = lambda step=ref(_step()), ch=(0, 1, 2), carry=p, pred=ref(rows), tgt=ref(rows), dt=DT: h.bf_rollout_flow(
        step, ch[0], ch[1], ch[2], DX, dt, 3 * DX, 1, carry, pred, tgt, None)
    for kw in (dict(step=None), dict(step=ref(_step(pred=None))), dict(carry=None), dict(pred=None), dict(tgt=None)):
        assert call(**kw) != 0 and h.bf_last_error().decode().endswith("bf_rollout_flow: null pointer"), kw
    for kw in (dict(Ho=2, H=2), dict(Wo=2), dict(Ho=1025, H=1025), dict(Wo=1025, W=1025)):
        assert call(step=ref(_step(**{**kw, "field_stride": 1 << 24}))) != 0
        assert h.bf_last_error().decode().endswith("bf_rollout_flow: Ho and Wo must lie in [3, 1024]"), kw
    for ch in ((-1, 1, 2), (0, 3, 2), (0, 1, 3)):
        assert call(ch=ch) != 0 and h.bf_last_error().decode().endswith("must be output channels"), ch
    assert call(dt=0.0) != 0 and "bf_rollout_flow: " in h.bf_last_error().decode()
