"""The error rows on the GPU (csrc/spectra.hip) against the numpy fp64 restatement tests/errors_restatement.py: `field_errors` on every radix
path of the transform, the identities that tie the rows together, determinism, `bf_rollout_errors` on the sample trajectories and
`evaluate_rollouts(errors=ErrorSpec())` against `field_errors` of its own archive."""
import functools

import numpy as np
import pytest
import torch

from tests import errors_restatement as R
from tests.test_rollout_eval import FILES

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 8), (8, 1), (2, 3), (5, 8), (7, 22), (12, 18), (16, 16), (31, 64), (30, 50), (64, 64), (3, 1024), (1024, 3)]
POINTWISE = ("rmse", "max_error", "boundary_rmse", "interface_rmse")
SPECTRA = ("spectrum_error", "spectrum_pred", "spectrum_target")
ROWS = POINTWISE + ("interface_cells", "spectral_error") + SPECTRA


def _same(u, v):
    fill = dict(nan=-7.0, posinf=-8.0, neginf=-9.0)
    return u.shape == v.shape and u.dtype == v.dtype and torch.equal(torch.nan_to_num(u.double(), **fill), torch.nan_to_num(v.double(), **fill))


def _check_frame(got, want, H, W, where):
    """One frame's device rows (numpy, fp32 / int32) against the restatement's; returns the worst shell and band ratio to their bounds."""
    for key in POINTWISE:
        if key not in want:
            continue
        g, w = float(got[key]), float(want[key])
        if np.isnan(w):
            assert np.isnan(g), (where, key, g)
        else:
            assert abs(g - w) <= 2.0 ** -22 * w, (where, key, g, w)
    if "interface_cells" in want:
        assert int(got["interface_cells"]) == want["interface_cells"], (where, int(got["interface_cells"]), want["interface_cells"])
    worst = 0.0
    for key in SPECTRA:
        w, g, total = want[key], got[key].astype(np.float64), want["total"][key]
        if np.isnan(w).any():
            assert np.array_equal(np.isnan(g), np.isnan(w)), (where, key)
            continue
        bound = R.shell_bound(w, total, H, W)
        gap = np.abs(g - w)
        assert (gap <= bound).all(), (where, key, int(np.argmax(gap - bound)), gap.max())
        worst = max(worst, float(np.max(gap[bound > 0] / bound[bound > 0], initial=0.0)))
    w, g = want["spectral_error"], got["spectral_error"].astype(np.float64)
    if np.isnan(w).any():
        assert np.array_equal(np.isnan(g), np.isnan(w)), (where, "spectral_error")
    else:
        for k in range(3):
            bound = R.band_bound(w[k], want["total"]["spectrum_error"], H, W)
            assert abs(g[k] - w[k]) <= bound, (where, "band", k, g[k], w[k])
            worst = max(worst, abs(g[k] - w[k]) / bound if bound > 0 else 0.0)
    return worst


@functools.lru_cache(maxsize=None)
def _case(shape):
    """The six frames of a shape, their device rows and the restatement's: computed once, shared by the tests below and never changed."""
    from bubbleformer_amd.utils import field_errors
    H, W = shape
    pred, target, sdf = R.case_frames(H, W, seed=H * 2048 + W)
    dev = [torch.from_numpy(a).cuda() for a in (pred, target, sdf)]
    got = field_errors(*dev)
    want = [R.field_errors(pred[k], target[k], sdf[k]) for k in range(6)]
    return dev, got, want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_field_errors_against_the_restatement(shape):
    """Pointwise rows to 2^-22 relative (fp64 sums of at most 2^20 terms, one fp32 rounding), integer rows exactly, every shell to one fp32
    rounding plus the normwise FFT bound eta = 64 max(1, log2(H W)) 2^-53 carried through |X|^2, relative to the field's own power; the bands
    to the same carried through the root.  Worst ratio to the bound seen on the MI355X over all shapes: 0.499, the fp32 rounding of the stored
    value, which is half of the bound's first term."""
    H, W = shape
    _, got, want = _case(shape)
    K = R.shell_count(H, W)
    assert got.rmse.shape == (6,) and got.interface_cells.dtype == torch.int32 and got.spectral_error.shape == (6, 3) and got.spectrum_error.shape == (6, K)
    rows = {k: getattr(got, k).cpu().numpy() for k in ROWS}
    worst = 0.0
    for k, name in enumerate(R.CASES):
        worst = max(worst, _check_frame({key: rows[key][k] for key in ROWS}, want[k], H, W, (shape, name)))
    print(f"{H} x {W}: worst ratio of a shell or band error to its bound {worst:.3f}; interface cells {rows['interface_cells'].tolist()}")
    # pred == target: exact zeros in every error row and every shell of the error
    assert all(float(rows[key][3]) == 0.0 for key in ("rmse", "max_error", "boundary_rmse")) and not rows["spectrum_error"][3].any() and not rows["spectral_error"][3].any()
    assert want[3]["interface_cells"] == 0 or float(rows["interface_rmse"][3]) == 0.0
    # a NaN in the frame: NaN in the maximum and the RMSE; no vapour: no interface cells, NaN for their RMSE
    assert np.isnan(rows["max_error"][4]) and np.isnan(rows["rmse"][4])
    assert rows["interface_cells"][5] == 0 and np.isnan(rows["interface_rmse"][5])


@pytest.mark.parametrize("shape", [(5, 8), (30, 50), (64, 64), (3, 1024)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_identities_on_the_device_rows(shape):
    """The shells of the error add up to rmse^2 (Parseval) and so do the squares of the three bands: both to 1e-5 relative, fp32 rows summed in fp64."""
    _, got, _ = _case(shape)
    for k in (0, 1, 2, 5):
        ms = float(got.rmse[k].double() ** 2)
        shells, bands = float(got.spectrum_error[k].double().sum()), float((got.spectral_error[k].double() ** 2).sum())
        assert abs(shells - ms) <= 1e-5 * ms and abs(bands - ms) <= 1e-5 * ms, (shape, k, ms, shells, bands)


@pytest.mark.parametrize("shape", [(7, 22), (30, 50), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_determinism_batching_and_null_outputs(shape):
    from bubbleformer_amd import ops
    from bubbleformer_amd.utils import ErrorSpec, field_errors
    (pred, target, sdf), got, _ = _case(shape)
    again = field_errors(pred, target, sdf)
    for key in ROWS:
        assert _same(getattr(got, key), getattr(again, key)), key                     # two calls: the same bits
    for k in (0, 2, 4):
        alone = field_errors(pred[k], target[k], sdf[k])                               # a frame alone: the bits it has in the batch
        for key in ROWS:
            assert _same(getattr(alone, key), getattr(got, key)[k]), (k, key)
    H, W = shape
    ws = ops.field_errors_workspace(6, H, W, "cuda")
    for keep in (("rmse",), ("spectrum_pred",), ("spectral_error", "interface_cells"), ("max_error", "spectrum_target", "interface_rmse")):
        rows = {key: torch.full_like(getattr(got, key), -3) for key in keep}
        ops.field_errors(pred, target, sdf, ws, **rows)                                # null outputs leave the others as they are
        for key in keep:
            assert _same(rows[key], getattr(got, key)), (keep, key)
    bare = field_errors(pred, target, spec=ErrorSpec(spectra=False))
    assert bare.interface_rmse is None and bare.interface_cells is None and bare.spectrum_error is None and bare.spectral_error is None
    assert _same(bare.rmse, got.rmse) and _same(bare.max_error, got.max_error) and _same(bare.boundary_rmse, got.boundary_rmse)
    wide = field_errors(pred, target, sdf, spec=ErrorSpec(interface_radius=2, bands=(1, 3)))
    for k in range(6):
        want = R.field_errors(pred[k].cpu().numpy(), target[k].cpu().numpy(), sdf[k].cpu().numpy(), r=2, lo=1, hi=3)
        assert int(wide.interface_cells[k]) == want["interface_cells"]
        if k != 4:
            assert np.allclose(wide.spectral_error[k].cpu().numpy(), want["spectral_error"], rtol=1e-6, atol=0)
    assert _same(wide.spectrum_error, got.spectrum_error)
    lead = field_errors(pred.reshape(2, 3, H, W), target.reshape(2, 3, H, W), sdf.reshape(2, 3, H, W))
    assert lead.rmse.shape == (2, 3) and lead.spectrum_pred.shape == (2, 3, R.shell_count(H, W)) and _same(lead.spectrum_pred.reshape(6, -1), got.spectrum_pred)
    assert _same(got.spectral_ratio(), got.spectrum_pred / got.spectrum_target)


def _rollout_errors(store, pred, starts, s, steps, sdf_channel=0):
    """One eager `ops.rollout_errors` call with the step counter preset to s, on outputs filled with -5."""
    from bubbleformer_amd import ops
    from bubbleformer_amd.utils.rollout import plan_rollouts
    B, T, C, Ho, Wo = pred.shape
    first = torch.tensor(plan_rollouts(store.ds, starts, steps).first, dtype=torch.int64, device="cuda")
    K = R.shell_count(Ho, Wo)
    tails = {"spectral_error": (3,), "spectrum_error": (K,), "spectrum_pred": (K,), "spectrum_target": (K,)}
    out = {key: torch.full((B, steps * T, C) + tails.get(key, ()), -5, dtype=torch.int32 if key == "interface_cells" else torch.float32, device="cuda")
           for key in ROWS if sdf_channel >= 0 or not key.startswith("interface")}
    counter = torch.full((1,), s, dtype=torch.int32, device="cuda")
    ops.rollout_errors(pred, store.frames, first, counter, store.out_tab, sdf_channel, steps, ops.field_errors_workspace(B * T * C, Ho, Wo, "cuda"), **out)
    return out, counter


@pytest.mark.parametrize("norm", ["none", "std"])
@pytest.mark.parametrize("factor", [1, 2])
def test_rollout_entry_against_the_restatement(norm, factor):
    """The step call against the restatement on the clips `gather` returns (the target's bits) and on the raw stored signed-distance frames
    (the mask); the prediction is the target plus a smooth error and a little noise.  Every frame of the samples has an interface."""
    from bubbleformer_amd import _lib
    from bubbleformer_amd.data import BubbleForecast
    T, steps, starts = 2, 8, [3, 20, 42 + 10]
    ds = BubbleForecast(FILES, norm=norm, downsample_factor=factor, time_window=T, start_time=5)
    ds.normalize()
    store = ds.device_store("cuda")
    raw = BubbleForecast(FILES, norm="none", downsample_factor=factor, time_window=T, start_time=5)
    raw.normalize()
    raw_store = raw.device_store("cuda")
    hw = 64 // factor
    rng = np.random.default_rng(7 * factor + len(norm))
    for s in (0, steps - 1):
        idx = [st + s * T for st in starts]
        tgt = store.gather(idx)[1]                                                    # (B, T, C, hw, hw): the bits the kernel must read
        sdf = raw_store.gather(idx)[1][:, :, 0].cpu().numpy()
        err = np.stack([R.smooth(hw, hw, rng) * 0.1 + 1e-3 * rng.standard_normal((hw, hw)) for _ in range(3 * T * 4)]).reshape(3, T, 4, hw, hw)
        pred = (tgt + torch.from_numpy(err.astype(np.float32)).cuda()).contiguous()
        out, counter = _rollout_errors(store, pred, starts, s, steps)
        assert int(counter) == s                                                      # read, never written
        rows = {key: v.cpu().numpy() for key, v in out.items()}
        p, y = pred.cpu().numpy(), tgt.cpu().numpy()
        worst = 0.0
        for b in range(3):
            for t in range(T):
                for c in range(4):
                    want = R.field_errors(p[b, t, c], y[b, t, c], sdf[b, t])
                    lo, hi = (415, 790) if factor == 1 else (1, hw * hw)
                    assert lo <= want["interface_cells"] <= hi, (b, t, want["interface_cells"])
                    worst = max(worst, _check_frame({key: rows[key][b, s * T + t, c] for key in ROWS}, want, hw, hw, (norm, factor, s, b, t, c)))
        print(f"norm {norm} factor {factor} step {s}: worst ratio to the bound {worst:.3f}, interface cells {rows['interface_cells'][:, s * T, 0].tolist()}")
        untouched = torch.ones(steps * T, dtype=torch.bool)
        untouched[s * T:(s + 1) * T] = False
        assert all(bool((v[:, untouched.cuda()] == -5).all()) for v in out.values())  # only this step's rows
        again, _ = _rollout_errors(store, pred, starts, s, steps)
        assert all(_same(again[key], out[key]) for key in out)
        none, _ = _rollout_errors(store, pred, starts, s, steps, sdf_channel=-1)      # no signed-distance channel: no interface rows, the rest the same
        assert sorted(none) == sorted(set(ROWS) - {"interface_rmse", "interface_cells"}) and all(_same(none[key], out[key]) for key in none)
    for s in (steps, -1):
        out, counter = _rollout_errors(store, pred, starts, s, steps)                 # a counter outside [0, steps): nothing written
        assert int(counter) == s and all(bool((v == -5).all()) for v in out.values())
    with pytest.raises(_lib.BubbleformerHipError, match="prediction"):
        _rollout_errors(store, pred.double(), starts, 0, steps)


@functools.lru_cache(maxsize=None)
def _reports():
    """The tiny conditioned filmavit of test_gpu_rollout_eval.test_trajectories_do_not_mix on the two sample trajectories (64 x 64, three steps
    of four frames, three trajectories), with the error rows in a graph and eagerly, and without them."""
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils import ErrorSpec
    from bubbleformer_amd.utils.rollout import evaluate_rollouts
    from oracle import weights as Wt
    from tests.test_gpu_rollout_eval import _study
    cfg = dict(input_fields=4, output_fields=4, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=2, num_fluid_params=9)
    model = get_model("filmavit", time_window=4, drop_path=0.0, compute_dtype=torch.float32, **cfg)
    model.load_state_dict(Wt.generate(Wt.param_shapes(**cfg), seed=5))
    model = model.cuda().eval()
    store = _study().device_store("cuda")
    starts, steps = [2, 38 + 9, 20], 3
    graph = evaluate_rollouts(model, store, starts, steps, use_graph=True, keep_predictions=True, errors=ErrorSpec())
    eager = evaluate_rollouts(model, store, starts, steps, use_graph=False, keep_predictions=True, errors=ErrorSpec())
    plain = evaluate_rollouts(model, store, starts, steps, use_graph=True, keep_predictions=True)
    single = evaluate_rollouts(model, store, starts[1:2], steps, use_graph=True, keep_predictions=True, errors=ErrorSpec())
    return store, starts, steps, graph, eager, plain, single


def test_evaluate_rollouts_with_errors(tmp_path):
    from bubbleformer_amd.utils import field_errors
    from bubbleformer_amd.utils.rollout import plan_rollouts
    from tests.test_gpu_rollout_eval import _report_tensors
    store, starts, steps, graph, eager, plain, single = _reports()
    T = 4
    old, old_eager, old_plain = _report_tensors(graph), _report_tensors(eager), _report_tensors(plain)
    assert len(old_plain) == 6 and all(getattr(plain, key) is None for key in ROWS)
    for k in old_plain:
        assert torch.equal(old[k], old_plain[k]) and torch.equal(old_eager[k], old_plain[k]), k    # nothing else moves when the errors are asked for
    for key in ROWS:
        assert _same(getattr(graph, key), getattr(eager, key)), key                                # graph and eager runs: the same bits
        assert _same(getattr(graph, key)[1:2], getattr(single, key)), key                          # trajectory 1 of B = 3 is the B = 1 run
    K = R.shell_count(64, 64)
    assert graph.rmse.shape == (3, steps * T, 4) and graph.spectral_error.shape == (3, steps * T, 4, 3) and graph.spectrum_error.shape == (3, steps * T, 4, K)
    assert graph.interface_cells.dtype == torch.int32
    first = plan_rollouts(store.ds, starts, steps).first
    dfun = store.fields.index("dfun")
    for b, st in enumerate(starts):
        tgt = store.gather([st + s * T for s in range(steps)])[1].reshape(steps * T, 4, 64, 64)
        sdf = store.frames[dfun, first[b] + T:first[b] + T + steps * T].unsqueeze(1).expand(-1, 4, -1, -1)
        want = field_errors(graph.predictions[b], tgt, sdf)
        for key in ROWS:
            assert _same(getattr(graph, key)[b], getattr(want, key)), (b, key)
    cells = graph.interface_cells
    assert 415 <= int(cells.min()) and int(cells.max()) <= 790 and bool((cells == cells[:, :, :1]).all())
    # rmse = rel_l2 * sqrt(mean y^2), and the target's shells add up to mean y^2: 1e-5 relative
    via = graph.rel_l2.double() * graph.spectrum_target.double().sum(-1).sqrt()
    gap = ((graph.rmse.double() - via).abs() / via).max()
    print(f"rmse against rel_l2 * sqrt(sum of the target's shells): {float(gap):.3e} relative; mean spectral ratio of the last shell "
          f"{float(graph.spectral_ratio()[..., -1].mean()):.3e}")
    assert float(gap) <= 1e-5
    assert _same(graph.spectral_ratio(), graph.spectrum_pred / graph.spectrum_target)
    with pytest.raises(ValueError):
        plain.spectral_ratio()
    graph.save(tmp_path / "with.pt")
    plain.save(tmp_path / "without.pt")
    with_, without = torch.load(tmp_path / "with.pt"), torch.load(tmp_path / "without.pt")
    assert sorted(set(with_) - set(without)) == sorted(ROWS) and set(without) <= set(with_)
    for key in ROWS:
        assert _same(with_[key], getattr(graph, key)), key
