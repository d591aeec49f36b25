"""The flow-consistency rows on the GPU (csrc/flow.hip) against the numpy fp64 restatement tests/flow_restatement.py: `flow_consistency` on shapes
from one interior cell to 3 x 1024, the two exact identities on the device, bit determinism, the per-step call `ops.rollout_flow` on the sample
store with its carry across step boundaries, and `evaluate_rollouts_flow` on the tiny conditioned filmavit of test_gpu_field_errors.

The bounds.  Counts and NaN positions are equal.  Every other row is within 2^-23 |want|: the terms of every sum are squares, so the order of an
fp64 sum over at most 2^20 cells moves it by less than 2^-33 relative, and the final rounding to fp32 is 2^-24.  transport_rms gets 2^-48 * scale
on top, scale = the root mean square over the band of |s| + |um dpm/dx| + |vm dpm/dy|: only the residual cancels, and there a contracted
multiply-add may differ by an fp64 ulp of its largest term."""
import functools

import numpy as np
import pytest
import torch

from tests import flow_restatement as R
from tests.test_flow_consistency import DT, DX, PLANAR, ROTATION, planar_front, solid_body
from tests.test_rollout_eval import FILES

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 3), (2, 3, 3), (2, 3, 1024), (3, 5, 8), (5, 30, 50), (2, 64, 64), (2, 193, 67)]
FLOAT_ROWS = ("divergence_rms", "kinetic_energy", "enstrophy", "transport_rms", "interface_speed_rms")
COUNT_ROWS = ("bulk_cells", "transport_cells")
ROWS = FLOAT_ROWS + COUNT_ROWS


def _same(u, v):
    """Equal bits, NaNs included."""
    return u.shape == v.shape and u.dtype == v.dtype and torch.equal(u.contiguous().view(torch.int32), v.contiguous().view(torch.int32))


def _check_rows(got, want, where):
    """got: {row: numpy array off the device}, want: the restatement's arrays of the same shapes -> the worst ratio of an error to its bound."""
    worst = 0.0
    for key in COUNT_ROWS:
        assert np.array_equal(got[key], want[key]), (where, key, got[key], want[key])
    for key in FLOAT_ROWS:
        g, w = got[key].astype(np.float64), np.asarray(want[key], dtype=np.float64)
        assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)), (where, key, g, w)
        bound = 2.0 ** -23 * np.abs(w)
        if key == "transport_rms":
            bound = bound + 2.0 ** -48 * np.asarray(want["scale"], dtype=np.float64)
        ok = ~np.isnan(w)
        err = np.abs(g - w)[ok]
        assert (err <= bound[ok]).all(), (where, key, g, w)
        if ok.any() and (bound[ok] > 0).any():
            worst = max(worst, float((err[bound[ok] > 0] / bound[ok][bound[ok] > 0]).max()))
    return worst


def _device_rows(fc):
    return {key: getattr(fc, key).cpu().numpy() for key in ROWS}


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Three sequences of smooth fields plus a little noise with an interface through every frame, and the restatement's rows per sequence."""
    T, H, W = shape
    f = R.fields(3, T, H, W, np.random.default_rng(1000 * T + 31 * H + W))
    want = [R.sequence_rows(f[0, s], f[1, s], f[2, s], DX, DT, 3 * DX, 1) for s in range(3)]
    return f, {key: np.stack([w[key] for w in want]) for key in ROWS + ("scale",)}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_flow_consistency_against_the_restatement(shape):
    from bubbleformer_amd.utils import FlowSpec, flow_consistency
    T, H, W = shape
    f, want = _case(shape)
    phi, u, v = (torch.from_numpy(a).cuda() for a in f)
    got = flow_consistency(phi, u, v, spec=FlowSpec(DT))
    assert got.divergence_rms.shape == (3, T) and got.transport_rms.shape == (3, T - 1) and got.bulk_cells.dtype == torch.int32
    rows = _device_rows(got)
    worst = _check_rows(rows, want, shape)
    if (H, W) == (3, 3):                            # one interior cell whose window is the frame: no bulk cell, a NaN row
        assert (rows["bulk_cells"] == 0).all() and np.isnan(rows["divergence_rms"]).all()
    else:
        assert (rows["bulk_cells"] > 0).any() and (T == 1 or (rows["transport_cells"] > 0).all())
    print(f"{shape}: worst ratio to the bound {worst:.3f}; bulk cells {rows['bulk_cells'][0].tolist()}, band cells {rows['transport_cells'][0].tolist()}")
    wider = flow_consistency(phi, u, v, spec=FlowSpec(DT, band=5 * DX, interface_radius=2))       # the other arguments reach the kernel
    want2 = [R.sequence_rows(f[0, s], f[1, s], f[2, s], DX, DT, 5 * DX, 2) for s in range(1)]
    _check_rows({key: val[:1] for key, val in _device_rows(wider).items()}, {key: np.stack([w[key] for w in want2]) for key in ROWS + ("scale",)}, shape)


def test_identities_on_the_device():
    """The exact cases of tests/test_flow_consistency.py give exact zeros and exact values on the device too: every intermediate is exact in fp64."""
    from bubbleformer_amd.utils import FlowSpec, flow_consistency
    spec = FlowSpec(DT)
    phi, u, v = (torch.from_numpy(a).cuda() for a in planar_front(3, 16, 24, **PLANAR))
    got = flow_consistency(phi, u, v, spec=spec)
    assert int(got.transport_cells.min()) > 0
    assert bool((got.transport_rms == 0.0).all())
    assert bool((got.interface_speed_rms == abs(PLANAR["a"] * PLANAR["u0"] + PLANAR["b"] * PLANAR["v0"])).all())
    assert bool((got.transport_ratio() == 0.0).all())
    assert bool((got.kinetic_energy == 0.5 * (PLANAR["u0"] ** 2 + PLANAR["v0"] ** 2)).all()) and bool((got.enstrophy == 0.0).all())
    phi, u, v = (torch.from_numpy(a).cuda() for a in solid_body(2, 12, 20, **ROTATION))
    got = flow_consistency(phi, u, v, spec=spec)
    assert bool((got.bulk_cells == 90).all()) and bool((got.divergence_rms == 0.0).all())
    assert bool((got.enstrophy == 2 * ROTATION["omega"] ** 2).all())


@pytest.mark.parametrize("shape", [(3, 5, 8), (5, 30, 50), (2, 193, 67)], ids=lambda s: "x".join(map(str, s)))
def test_determinism_batching_and_null_outputs(shape):
    from bubbleformer_amd import ops
    from bubbleformer_amd.utils import FlowSpec, flow_consistency
    T, H, W = shape
    f, _ = _case(shape)
    phi, u, v = (torch.from_numpy(a).cuda() for a in f)
    spec = FlowSpec(DT)
    a, b = flow_consistency(phi, u, v, spec=spec), flow_consistency(phi, u, v, spec=spec)
    alone = flow_consistency(phi[1:2].clone(), u[1:2].clone(), v[1:2].clone(), spec=spec)
    for key in ROWS:
        assert _same(getattr(a, key), getattr(b, key)), key                              # two calls: the same bits
        assert _same(getattr(a, key)[1:2], getattr(alone, key)), key                    # a sequence alone and in a batch
    # a NaN in one frame's velocity reaches that frame's sums and the pairs it belongs to, and no other row
    u2 = u.clone()
    u2[1, 1] = float("nan")
    c = flow_consistency(phi, u2, v, spec=spec)
    assert bool(torch.isnan(c.kinetic_energy[1, 1])) and bool(torch.isnan(c.enstrophy[1, 1]))
    clean = torch.ones(3, T, dtype=torch.bool, device="cuda")
    clean[1, 1] = False
    for key in ("divergence_rms", "kinetic_energy", "enstrophy", "bulk_cells"):
        assert _same(getattr(c, key)[clean], getattr(a, key)[clean]), key
    clean_pairs = torch.ones(3, T - 1, dtype=torch.bool, device="cuda")
    clean_pairs[1, 0:2] = False                                                          # the pairs (0, 1) and (1, 2)
    for key in ("transport_rms", "interface_speed_rms", "transport_cells"):
        assert _same(getattr(c, key)[clean_pairs], getattr(a, key)[clean_pairs]), key
    assert _same(c.interface_speed_rms, a.interface_speed_rms) and _same(c.transport_cells, a.transport_cells)       # phi alone
    # null members: the others keep their bits, and nothing else is written
    def filled():
        return {key: torch.full((3, T if key in ops._FLOW_FRAME_ROWS else T - 1), -5, dtype=torch.int32 if key.endswith("_cells") else torch.float32,
                                device="cuda") for key in ops._FLOW_ROWS}
    for given in [(key,) for key in ops._FLOW_ROWS] + [("divergence_rms", "transport_cells"), ("bulk_cells", "interface_speed_rms", "enstrophy")]:
        out = filled()
        ops.flow_consistency(phi, u, v, DX, DT, 3 * DX, 1, **{key: out[key] for key in given})
        for key in ops._FLOW_ROWS:
            if key in given:
                assert _same(out[key], getattr(a, key)), (given, key)
            else:
                assert bool((out[key] == -5).all()), (given, key)


def test_bindings_refuse_bad_tensors():
    from bubbleformer_amd import _lib, ops
    z = torch.zeros(1, 2, 4, 4, device="cuda")
    rows = lambda: dict(kinetic_energy=torch.zeros(1, 2, device="cuda"))
    ops.flow_consistency(z, z, z, DX, DT, 3 * DX, 1, **rows())
    for bad in (dict(sdf=z.double()), dict(velx=z[:, :, :, :3]), dict(vely=z.cpu())):
        args = {**dict(sdf=z, velx=z, vely=z), **bad}
        with pytest.raises(_lib.BubbleformerHipError):
            ops.flow_consistency(args["sdf"], args["velx"], args["vely"], DX, DT, 3 * DX, 1, **rows())
    with pytest.raises(_lib.BubbleformerHipError, match="kinetic_energy"):
        ops.flow_consistency(z, z, z, DX, DT, 3 * DX, 1, kinetic_energy=torch.zeros(1, 1, device="cuda"))
    with pytest.raises(_lib.BubbleformerHipError, match="unknown"):
        ops.flow_consistency(z, z, z, DX, DT, 3 * DX, 1, vorticity=torch.zeros(1, 2, device="cuda"))
    with pytest.raises(_lib.BubbleformerHipError, match=r"\[3, 1024\]"):
        ops.flow_consistency(z[:, :, :2].contiguous(), z[:, :, :2].contiguous(), z[:, :, :2].contiguous(), DX, DT, 3 * DX, 1, **rows())


# ---------------------------------------------------------------------------- ops.rollout_flow
CHANNELS = (0, 2, 3)                                 # dfun, velx, vely among the sample store's four output fields


def _rollout_flow(store, pred, starts, s, steps, carry, dx, channels=CHANNELS):
    """One eager `ops.rollout_flow` call with the step counter preset to s, on outputs filled with -5 -> (rows_pred, rows_target, counter)."""
    from bubbleformer_amd import ops
    from bubbleformer_amd.utils.rollout import plan_rollouts
    B, T = pred.shape[:2]
    first = torch.tensor(plan_rollouts(store.ds, starts, steps).first, dtype=torch.int64, device="cuda")
    out = [{key: torch.full((B, steps * T if key in ops._FLOW_FRAME_ROWS else steps * T - 1), -5, dtype=torch.int32 if key.endswith("_cells") else torch.float32,
                            device="cuda") for key in ops._FLOW_ROWS} for _ in range(2)]
    counter = torch.full((1,), s, dtype=torch.int32, device="cuda")
    ops.rollout_flow(pred, store.frames, first, counter, store.out_tab, channels, steps, dx, DT, 3 * dx, 1, carry, out[0], out[1])
    return out[0], out[1], counter


@pytest.mark.parametrize("norm", ["none", "std"])
@pytest.mark.parametrize("factor", [1, 2])
def test_rollout_entry_against_the_restatement(norm, factor):
    """The step call against the restatement: the prediction is the gathered target clip plus a smooth error, de-normalised in np.float32 as the
    kernel does it; the target side is the raw clip `gather` returns from the un-normalised store (the bits the kernel reads).  The carry half is
    written by the call for the step before, and the pair across the boundary is the restatement's on the concatenated frames."""
    from bubbleformer_amd import _lib
    from bubbleformer_amd.data import BubbleForecast
    T, steps, starts = 2, 8, [3, 20, 42 + 10]
    ds = BubbleForecast(FILES, norm=norm, downsample_factor=factor, time_window=T, start_time=5)
    ds.normalize()
    store = ds.device_store("cuda")
    raw = BubbleForecast(FILES, norm="none", downsample_factor=factor, time_window=T, start_time=5)
    raw.normalize()
    raw_store = raw.device_store("cuda")
    hw, dx = 64 // factor, DX * factor
    _, diff, div = (t.cpu().numpy() for t in store.out_tab)
    rng = np.random.default_rng(11 * factor + len(norm))

    def clip(s):
        """Step s: the prediction (device, normalised), its physical (phi, u, v) (B, T, hw, hw) and the simulation's."""
        idx = [st + s * T for st in starts]
        tgt = store.gather(idx)[1]
        err = np.stack([R.smooth(hw, hw, rng) * 0.05 for _ in range(3 * T * 4)]).reshape(3, T, 4, hw, hw)
        pred = (tgt + torch.from_numpy(err.astype(np.float32)).cuda()).contiguous()
        p = pred.cpu().numpy()
        phys = [R.denormalise(p[:, :, c], div[c], diff[c]) for c in CHANNELS]
        sim = raw_store.gather(idx)[1].cpu().numpy()
        return pred, phys, [sim[:, :, c] for c in CHANNELS]

    carry = torch.full((2, 3, 3, hw, hw), -5.0, device="cuda")
    for s in (0, 1, steps - 1):
        before = None
        if s > 0:
            before = clip(s - 1)
            _rollout_flow(store, before[0], starts, s - 1, steps, carry, dx)              # leaves the carry half (s - 1) & 1
        pred, phys, sim = clip(s)
        rows_p, rows_t, counter = _rollout_flow(store, pred, starts, s, steps, carry, dx)
        assert int(counter) == s                                                          # read, never written
        # half s & 1 of the carry: the physical (phi, u, v) of the step's last predicted frame
        assert np.array_equal(carry[s & 1].cpu().numpy(), np.stack([f[:, T - 1] for f in phys], axis=1))
        lead = 0 if s == 0 else T                                                         # frames of the step before, in front
        worst = 0.0
        for side, rows, cur, prev in (("pred", rows_p, phys, before and before[1]), ("target", rows_t, sim, before and before[2])):
            got = {key: v.cpu().numpy() for key, v in rows.items()}
            for b in range(3):
                seq = [np.concatenate([prev[k][b], cur[k][b]]) if s > 0 else cur[k][b] for k in range(3)]
                want = R.sequence_rows(*seq, dx, DT, 3 * dx, 1)
                assert (want["transport_cells"] >= 1).all() and (want["bulk_cells"] >= 1).all(), (side, b, want["transport_cells"])
                pair0 = s * T - 1 if s > 0 else 0                                         # the first pair row of this step
                mine = {key: got[key][b, s * T:(s + 1) * T] for key in R.FRAME_ROWS}
                mine.update({key: got[key][b, pair0:s * T + T - 1] for key in R.PAIR_ROWS})
                ref = {key: want[key][lead:] for key in R.FRAME_ROWS}
                ref.update({key: want[key][lead - 1 if s > 0 else 0:] for key in R.PAIR_ROWS + ("scale",)})
                worst = max(worst, _check_rows(mine, ref, (norm, factor, s, side, b)))
            frames_untouched = torch.ones(steps * T, dtype=torch.bool, device="cuda")
            frames_untouched[s * T:(s + 1) * T] = False
            pairs_untouched = torch.ones(steps * T - 1, dtype=torch.bool, device="cuda")
            pairs_untouched[(s * T - 1 if s > 0 else 0):s * T + T - 1] = False
            for key, v in rows.items():                                                   # only this step's rows
                assert bool((v[:, frames_untouched if key in R.FRAME_ROWS else pairs_untouched] == -5).all()), (side, key)
        print(f"norm {norm} factor {factor} step {s}: worst ratio to the bound {worst:.3f}; band cells pred {rows_p['transport_cells'][:, max(s * T - 1, 0)].tolist()} "
              f"target {rows_t['transport_cells'][:, max(s * T - 1, 0)].tolist()}, bulk cells target {rows_t['bulk_cells'][:, s * T].tolist()}")
        again = _rollout_flow(store, pred, starts, s, steps, carry, dx)
        assert all(_same(again[0][key], rows_p[key]) and _same(again[1][key], rows_t[key]) for key in rows_p)
    for s in (steps, -1):                                                                 # a counter outside [0, steps): nothing written, the carry included
        fresh = torch.full_like(carry, -5.0)
        rows_p, rows_t, counter = _rollout_flow(store, pred, starts, s, steps, fresh, dx)
        assert int(counter) == s and all(bool((v == -5).all()) for v in list(rows_p.values()) + list(rows_t.values()) + [fresh])
    with pytest.raises(_lib.BubbleformerHipError, match="prediction"):
        _rollout_flow(store, pred.double(), starts, 0, steps, carry, dx)
    with pytest.raises(_lib.BubbleformerHipError, match="carry"):
        _rollout_flow(store, pred, starts, 0, steps, carry.double(), dx)
    for channels in ((0, 2, 4), (-1, 2, 3)):
        with pytest.raises(_lib.BubbleformerHipError, match="channels"):
            _rollout_flow(store, pred, starts, 0, steps, carry, dx, channels)


# ---------------------------------------------------------------------------- evaluate_rollouts_flow
FLOW_ROWS = {"flow_divergence": "divergence_rms", "flow_bulk_cells": "bulk_cells", "flow_kinetic_energy": "kinetic_energy", "flow_enstrophy": "enstrophy",
             "flow_transport": "transport_rms", "flow_interface_speed": "interface_speed_rms", "flow_transport_cells": "transport_cells"}
FLOW_KEYS = [f"{name}_{side}" for name in FLOW_ROWS for side in ("pred", "target")]


@functools.lru_cache(maxsize=None)
def _reports():
    """The tiny conditioned filmavit of test_gpu_field_errors._reports on its store (64 x 64, three steps of four frames, three trajectories), with
    the flow rows in a graph, eagerly, for one trajectory alone, with flow=None and with redistancing in front."""
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils import FlowSpec, RedistanceSpec
    from bubbleformer_amd.utils.rollout import evaluate_rollouts_flow
    from oracle import weights as Wt
    from tests.test_gpu_field_errors import _reports as base
    store, starts, steps, _, _, plain, _ = base()
    cfg = dict(input_fields=4, output_fields=4, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=2, num_fluid_params=9)
    model = get_model("filmavit", time_window=4, drop_path=0.0, compute_dtype=torch.float32, **cfg)
    model.load_state_dict(Wt.generate(Wt.param_shapes(**cfg), seed=5))
    model = model.cuda().eval()
    spec = FlowSpec(DT)
    kw = dict(keep_predictions=True)
    graph = evaluate_rollouts_flow(model, store, starts, steps, spec, use_graph=True, **kw)
    eager = evaluate_rollouts_flow(model, store, starts, steps, spec, use_graph=False, **kw)
    single = evaluate_rollouts_flow(model, store, starts[1:2], steps, spec, use_graph=True, **kw)
    none = evaluate_rollouts_flow(model, store, starts, steps, None, use_graph=True, **kw)
    corrected = evaluate_rollouts_flow(model, store, starts, steps, spec, use_graph=True, redistance=RedistanceSpec(), **kw)
    return store, starts, steps, spec, plain, graph, eager, single, none, corrected


def _both_sides(report, store, starts, steps, spec, T=4):
    """`flow_consistency` of the report's de-normalised archive, and of the stored frames behind each trajectory's first input clip."""
    from bubbleformer_amd.utils import flow_consistency
    from bubbleformer_amd.utils.rollout import plan_rollouts
    _, diff, div = store.out_tab
    ch = spec.channels(report.fields)
    phys = [(report.predictions[:, :, c] * div[c] + diff[c]).contiguous() for c in ch]         # fp32 multiply, then add
    first = plan_rollouts(store.ds, starts, steps).first
    rows = [store.fields.index(report.fields[c]) for c in ch]
    sim = [torch.stack([store.frames[r, f + T:f + T + steps * T] for f in first]) for r in rows]
    return flow_consistency(*phys, spec=spec), flow_consistency(*sim, spec=spec)


def test_evaluate_rollouts_flow(tmp_path):
    from tests.test_gpu_rollout_eval import _report_tensors
    store, starts, steps, spec, plain, graph, eager, single, none, corrected = _reports()
    T = 4
    base = _report_tensors(plain)
    assert len(base) == 6 and all(getattr(none, key) is None and getattr(plain, key) is None for key in FLOW_KEYS + ["flow_dx", "flow_dt"])
    for run in (none, graph, eager):                                                      # flow=None is the plain call, and with it nothing else moves
        got = _report_tensors(run)
        assert sorted(got) == sorted(base)
        for k in base:
            assert torch.equal(got[k], base[k]), k
    for key in FLOW_KEYS:
        assert _same(getattr(graph, key), getattr(eager, key)), key                       # graph and eager runs: the same bits
        assert _same(getattr(graph, key)[1:2], getattr(single, key)), key                 # trajectory 1 of B = 3 is the B = 1 run
    assert graph.flow_divergence_pred.shape == (3, steps * T) and graph.flow_transport_target.shape == (3, steps * T - 1)
    assert graph.flow_bulk_cells_pred.dtype == torch.int32 and graph.flow_transport_cells_target.dtype == torch.int32
    assert (graph.flow_dx, graph.flow_dt) == (spec.dx, spec.dt)
    for report in (graph, corrected):                                                     # the same kernel on the same values: equal bits
        want_pred, want_target = _both_sides(report, store, starts, steps, spec)
        for name, member in FLOW_ROWS.items():
            assert _same(getattr(report, name + "_pred"), getattr(want_pred, member)), name
            assert _same(getattr(report, name + "_target"), getattr(want_target, member)), name
    cells = graph.flow_transport_cells_target
    assert 121 <= int(cells.min()) and int(cells.max()) <= 242 and 2857 <= int(graph.flow_bulk_cells_target.min())
    # with redistancing in front the rows are those of the corrected signed distance: the simulation's stay, the prediction's phi rows move
    assert int(corrected.redistance_rounds.min()) >= 1 and not torch.equal(corrected.predictions, graph.predictions)
    assert not _same(corrected.flow_interface_speed_pred, graph.flow_interface_speed_pred)
    for name in FLOW_ROWS:
        assert _same(getattr(corrected, name + "_target"), getattr(graph, name + "_target")), name
    print("transport ratio, prediction", [round(v, 3) for v in graph.transport_ratio()[0][0, :4].tolist()], "simulation",
          [round(v, 3) for v in graph.transport_ratio()[1][0, :4].tolist()], "energy drift", [round(v, 3) for v in graph.energy_drift()[0, :4].tolist()],
          "divergence excess", [round(v, 3) for v in graph.divergence_excess()[0, :4].tolist()])
    ratio_p, ratio_t = graph.transport_ratio()
    assert _same(ratio_p, graph.flow_transport_pred / graph.flow_interface_speed_pred)
    assert _same(ratio_t, graph.flow_transport_target / graph.flow_interface_speed_target)
    assert _same(graph.energy_drift(), graph.flow_kinetic_energy_pred / graph.flow_kinetic_energy_target)
    assert _same(graph.divergence_excess(), graph.flow_divergence_pred / graph.flow_divergence_target)
    for method in ("transport_ratio", "energy_drift", "divergence_excess"):
        with pytest.raises(ValueError):
            getattr(none, method)()
    graph.save(tmp_path / "with.pt")
    none.save(tmp_path / "without.pt")
    with_, without = torch.load(tmp_path / "with.pt"), torch.load(tmp_path / "without.pt")
    assert sorted(set(with_) - set(without)) == sorted(FLOW_KEYS + ["flow_dx", "flow_dt"]) and set(without) <= set(with_)
    for key in FLOW_KEYS:
        assert _same(with_[key], getattr(graph, key)), key
    assert (with_["flow_dx"], with_["flow_dt"]) == (spec.dx, spec.dt)


def test_a_dataset_without_a_velocity_field_is_refused():
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils import FlowSpec
    from bubbleformer_amd.utils.rollout import evaluate_rollouts_flow
    fields = ["dfun", "temperature", "velx"]
    ds = BubbleForecast(FILES[1:], input_fields=fields, output_fields=fields, norm="std", downsample_factor=2, time_window=4, start_time=5)
    ds.normalize()
    model = get_model("avit", time_window=4, drop_path=0.0, input_fields=3, output_fields=3, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=2).cuda().eval()
    with pytest.raises(ValueError, match="vely"):
        evaluate_rollouts_flow(model, ds, [7], 2, FlowSpec(DT))
