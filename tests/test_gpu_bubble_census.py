"""Bubble census on the GPU: `bubble_census` against scipy's label images (tests/golden/bubble_census.npz) and the flood fill of
tests/bubbles_restatement.py, in both storage regimes of the kernel; `bf_rollout_bubbles` against the restatement on the raw target clips
and on pred * div + diff; `evaluate_rollouts(bubbles=...)` against the run without it and against `bubble_census` of its archive.
Integers are compared with ==; a centroid is np.float32(integer sum / area) exactly (exact sums, one fp64 division, one rounding)."""
import functools

import numpy as np
import pytest
import torch

from tests import bubbles_restatement as R
from tests.test_bubble_census import golden, sample_dfun
from tests.test_rollout_eval import FILES

pytestmark = pytest.mark.gpu
NEW_KEYS = ["bubble_area_pred", "bubble_area_target", "bubble_attached_pred", "bubble_attached_target", "bubble_count_pred", "bubble_count_target",
            "vapour_fraction_pred", "vapour_fraction_target"]


def _census(phi, **kw):
    from bubbleformer_amd.utils import bubble_census
    return bubble_census(torch.from_numpy(np.ascontiguousarray(phi)).cuda(), **kw)


def _assert_frame(c, f, mask, conn, mb, what):
    """Frame f of the census c (leading dim = frames) against the flood fill of `mask`."""
    want = R.census(mask, conn, mb)
    got = {k: getattr(c, k)[f].cpu().numpy() for k in ("count", "vapour_cells", "attached", "area", "centroid", "on_heater")}
    for k in ("count", "vapour_cells", "attached"):
        assert int(got[k]) == want[k], (what, k, int(got[k]), want[k])
    assert np.array_equal(got["area"], want["area"]), what
    assert np.array_equal(got["on_heater"], want["on_heater"]), what
    gap = np.abs(got["centroid"].astype(np.float64) - want["centroid"])
    if gap.max() > 0:
        print(f"{what}: worst centroid gap {gap.max():.3e}")
    assert np.array_equal(got["centroid"], want["centroid"]), what
    if c.labels is not None:
        assert np.array_equal(c.labels[f].cpu().numpy(), want["labels"]), what
    return want


@pytest.mark.parametrize("conn", R.CONNECTIVITIES)
def test_synthetic_masks_against_scipy(conn):
    z = golden()
    masks = R.masks()
    phi = np.stack([R.phi_of(m, seed=i) for i, m in enumerate(masks.values())])
    c = _census(phi, connectivity=conn, return_labels=True)
    assert c.labels.shape == (len(masks),) + R.MASK_SHAPE and c.labels.dtype == torch.int32 and c.count.dtype == torch.int32
    assert c.area.shape == (len(masks), 256) and c.centroid.shape == (len(masks), 256, 2) and c.on_heater.dtype == torch.bool
    labels = c.labels.cpu().numpy()
    for f, (name, mask) in enumerate(masks.items()):
        assert np.array_equal(labels[f], z[f"labels/{name}/{conn}"].astype(np.int32)), name          # scipy's numbering, not a permutation of it
        assert int(c.count[f]) == R.MASK_COUNTS[name][conn == 8], name
        _assert_frame(c, f, mask, conn, 256, name)
    if conn == 4:                                                                     # more components than records: the count stays true
        f = list(masks).index("checkerboard")
        assert int(c.count[f]) == 1440 and int(c.vapour_cells[f]) == 1440 and c.area[f].tolist() == [1] * 256
    again = _census(phi, connectivity=conn, return_labels=True)
    for k in ("count", "vapour_cells", "attached", "area", "centroid", "on_heater", "labels"):
        assert torch.equal(getattr(c, k), getattr(again, k)), k                       # two calls, the same bits
    f = list(masks).index("random_0.5")
    alone = _census(phi[f], connectivity=conn, return_labels=True)                    # (H, W): no leading dims
    assert alone.count.dim() == 0 and alone.area.shape == (256,) and alone.labels.shape == R.MASK_SHAPE
    for k in ("count", "vapour_cells", "attached", "area", "centroid", "on_heater", "labels"):
        assert torch.equal(getattr(alone, k), getattr(c, k)[f]), k
    few = _census(phi, connectivity=conn, max_bubbles=3)                              # fewer records: the first three of the same numbering
    assert torch.equal(few.count, c.count) and torch.equal(few.area, c.area[:, :3]) and torch.equal(few.centroid, c.centroid[:, :3])
    assert few.labels is None and torch.equal(few.on_heater, c.on_heater[:, :3])
    frac = c.vapour_fraction()
    cells = c.vapour_cells.cpu().numpy()
    assert frac.dtype == torch.float32 and np.array_equal(frac.cpu().numpy(), (cells / float(40 * 72)).astype(np.float32))
    d = c.equivalent_diameter(dx=1 / 32)
    want = (2 * np.sqrt(c.area.cpu().numpy().astype(np.float64) / 1024 / np.pi))
    assert d.shape == c.area.shape and np.allclose(d.cpu().numpy(), want, rtol=1e-6, atol=0) and bool((d[c.area == 0] == 0).all())


@pytest.mark.parametrize("shape", [(1, 1), (1, 72), (40, 1), (2, 2), (3, 1025)])
def test_thin_frames(shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    masks = [np.ones(shape, bool), np.zeros(shape, bool)] + [rng.random(shape) < p for p in (0.3, 0.6, 0.8)]
    phi = np.stack([R.phi_of(m, seed=i) for i, m in enumerate(masks)])
    for conn in R.CONNECTIVITIES:
        c = _census(phi, connectivity=conn, max_bubbles=16, return_labels=True)
        for f, m in enumerate(masks):
            _assert_frame(c, f, m, conn, 16, (shape, conn, f))


def test_fixture_frames():
    """All 100 frames of the two sample files in one call against scipy's counts, attached counts and areas; a frame alone has the bits it
    has in the batch."""
    z = golden()
    dfun = np.concatenate([sample_dfun(1), sample_dfun(2)])
    assert dfun.shape == (100, 64, 64)
    for conn in R.CONNECTIVITIES:
        c = _census(dfun.reshape(2, 50, 64, 64), connectivity=conn, max_bubbles=32)
        assert c.count.shape == (2, 50) and c.area.shape == (2, 50, 32)
        for k in (1, 2):
            counts, attached, areas = z[f"sample{k}/count/{conn}"], z[f"sample{k}/attached/{conn}"], z[f"sample{k}/areas/{conn}"]
            assert np.array_equal(c.count[k - 1].cpu().numpy(), counts) and np.array_equal(c.attached[k - 1].cpu().numpy(), attached)
            got = c.area[k - 1].cpu().numpy()
            assert np.array_equal(np.sort(got[:, :areas.shape[1]], axis=1), np.sort(areas, axis=1)) and not got[:, areas.shape[1]:].any()
            assert np.array_equal(got[:, :areas.shape[1]], areas)                     # and in scipy's order
            assert np.array_equal(c.vapour_cells[k - 1].cpu().numpy(), (dfun[50 * (k - 1):50 * k] > 0).sum(axis=(1, 2)))
        flat = {k: getattr(c, k).reshape((100,) + getattr(c, k).shape[2:]) for k in ("count", "vapour_cells", "attached", "area", "centroid", "on_heater")}
        for f in (0, 49, 50, 99):
            alone = _census(dfun[f], connectivity=conn, max_bubbles=32)
            for k, v in flat.items():
                assert torch.equal(getattr(alone, k), v[f]), (f, k)
        _assert_frame(type(c)(**{**flat, "shape": (64, 64), "labels": None}), 63, dfun[63] > 0, conn, 32, ("sample frame 63", conn))


def test_both_storage_regimes():
    """The largest frame whose parents live in LDS and the smallest that takes the workspace, blob masks against the flood fill."""
    from bubbleformer_amd import ops
    lds = ops.bubble_census_lds_cells()
    side = int(np.ceil(np.sqrt(lds + 1)))
    width = next((w for w in range(side, 2 * side) if lds % w == 0), side)          # a frame of exactly lds cells where lds has such a divisor
    largest = (lds // width, width)
    assert lds - width < largest[0] * largest[1] <= lds < side * side and (side - 1) * side <= lds
    print(f"LDS limit {lds} cells: largest LDS frame {largest}, smallest workspace frame {(side, side)}")
    for shape in (largest, (side, side)):
        masks = [R.blobs(shape, seed) for seed in (3, 4)]
        phi = np.stack([R.phi_of(m, seed=i) for i, m in enumerate(masks)])
        for conn in R.CONNECTIVITIES:
            c = _census(phi, connectivity=conn, return_labels=True)
            for f, m in enumerate(masks):
                want = _assert_frame(c, f, m, conn, 256, (shape, conn, f))
                assert 3 <= want["count"] <= 256 and want["attached"] >= 1
            alone = _census(phi[1], connectivity=conn, return_labels=True)
            assert torch.equal(alone.labels, c.labels[1]) and torch.equal(alone.centroid, c.centroid[1])


def test_too_large_a_frame_is_refused_before_any_launch():
    from bubbleformer_amd import _lib, ops
    with pytest.raises(_lib.BubbleformerHipError, match="2\\^24"):
        ops.bubble_census_workspace(1, 4096, 4097, 8, "cuda")
    phi = torch.zeros(1, 8, 8, device="cuda")
    new = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
    small = torch.empty(16, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.BubbleformerHipError, match="workspace"):
        ops.bubble_census(phi, 4, 8, small, new(1), new(1), new(1), new(1, 8))
    with pytest.raises(_lib.BubbleformerHipError, match="connectivity"):
        ops.bubble_census(phi, 5, 8, ops.bubble_census_workspace(1, 8, 8, 8, "cuda"), new(1), new(1), new(1), new(1, 8))


def _rollout_bubbles(store, pred, starts, s, steps, conn, mb):
    """One eager `ops.rollout_bubbles` call with the step counter preset to s, on outputs filled with -1."""
    from bubbleformer_amd import ops
    from bubbleformer_amd.utils.rollout import plan_rollouts
    B, T, _, Ho, Wo = pred.shape
    dev = pred.device
    first = torch.tensor(plan_rollouts(store.ds, starts, steps).first, dtype=torch.int64, device=dev)
    fill = lambda *tail: [torch.full((B, steps * T) + tail, -1, dtype=torch.int32, device=dev) for _ in range(2)]
    out = {"count": fill(), "cells": fill(), "attached": fill(), "area": fill(mb)}
    counter = torch.full((1,), s, dtype=torch.int32, device=dev)
    ws = ops.bubble_census_workspace(2 * B * T, Ho, Wo, mb, dev)
    ops.rollout_bubbles(pred, store.frames, first, counter, store.out_tab, 0, steps, conn, mb, ws, *out["count"], *out["cells"], *out["attached"], *out["area"])
    return out, counter


@pytest.mark.parametrize("norm", ["none", "std"])
@pytest.mark.parametrize("factor", [1, 2])
def test_rollout_entry_against_the_restatement(norm, factor):
    """Simulation rows against the flood fill of the raw gathered target clips, prediction rows against the flood fill of pred * div + diff
    formed in torch fp32 (the mask is then decided on identical bits).  The prediction is a smooth random field in physical units."""
    from bubbleformer_amd import _lib
    from bubbleformer_amd.data import BubbleForecast
    T, steps, starts, mb = 2, 8, [3, 20, 42 + 10], 32
    ds = BubbleForecast(FILES, norm=norm, downsample_factor=factor, time_window=T, start_time=5)
    ds.normalize()
    store = ds.device_store("cuda")
    raw = BubbleForecast(FILES, norm="none", downsample_factor=factor, time_window=T, start_time=5)
    raw.normalize()
    raw_store = raw.device_store("cuda")
    _, diff, div = store.out_tab
    hw = 64 // factor
    g = torch.Generator().manual_seed(500 * factor + len(norm))
    pred = torch.randn((3, T, 4, hw, hw), generator=g).cuda()
    field = torch.from_numpy(R.smooth_field((3, T, hw, hw), seed=factor)).cuda()
    pred[:, :, 0] = (field - diff[0]) / div[0]                                        # normalised, so that the physical field is the smooth one
    phys = pred * div.view(1, 1, 4, 1, 1) + diff.view(1, 1, 4, 1, 1)                  # fp32 multiply, then add
    conn = 4 if factor == 1 else 8
    for s in (0, steps - 1):
        out, counter = _rollout_bubbles(store, pred, starts, s, steps, conn, mb)
        assert int(counter) == s                                                      # read, never written
        rows = slice(s * T, (s + 1) * T)
        tgt = raw_store.gather([st + s * T for st in starts])[1]                      # the raw, downsampled target clips
        for side, (name, clip) in enumerate((("pred", phys), ("sim", tgt))):
            masks = clip[:, :, 0].cpu().numpy() > 0
            for b in range(3):
                for t in range(T):
                    want = R.census(masks[b, t], conn, mb)
                    if name == "pred":
                        assert 3 <= want["count"] <= mb and want["attached"] >= 1, (b, t, want["count"], want["attached"])
                    r = s * T + t
                    got = (int(out["count"][side][b, r]), int(out["cells"][side][b, r]), int(out["attached"][side][b, r]))
                    assert got == (want["count"], want["vapour_cells"], want["attached"]), (name, b, t, got)
                    assert np.array_equal(out["area"][side][b, r].cpu().numpy(), want["area"]), (name, b, t)
        untouched = torch.ones(steps * T, dtype=torch.bool)
        untouched[rows] = False
        for pair in out.values():
            for t_ in pair:
                assert bool((t_[:, untouched.cuda()] == -1).all())                    # only this step's rows
        again, _ = _rollout_bubbles(store, pred, starts, s, steps, conn, mb)
        for k in out:
            assert torch.equal(again[k][0], out[k][0]) and torch.equal(again[k][1], out[k][1]), k
    out, counter = _rollout_bubbles(store, pred, starts, steps, steps, conn, mb)       # a counter behind the last row: nothing written
    assert int(counter) == steps and all(bool((t_ == -1).all()) for pair in out.values() for t_ in pair)
    with pytest.raises(_lib.BubbleformerHipError, match="prediction"):
        _rollout_bubbles(store, pred.double(), starts, 0, steps, conn, mb)
    with pytest.raises(_lib.BubbleformerHipError, match="connectivity"):
        _rollout_bubbles(store, pred, starts, 0, steps, 6, mb)


@functools.lru_cache(maxsize=None)
def _reports():
    """The tiny rollout of test_gpu_heatflux_eval (avit, 32 x 32 after downsampling by 2, three steps of four frames) with the census in a
    graph and eagerly, with the heat flux beside it, and that module's runs without the census."""
    from bubbleformer_amd.utils import BubbleSpec
    from bubbleformer_amd.utils.rollout import evaluate_rollouts
    from tests.test_gpu_heatflux_eval import _tiny_model, _tiny_reports
    store, hf_spec, hf_graph, _, plain = _tiny_reports()
    model = _tiny_model()
    spec = BubbleSpec(max_bubbles=24, dx=1 / 2)
    graph = evaluate_rollouts(model, store, [7], 3, use_graph=True, keep_predictions=True, bubbles=spec)
    eager = evaluate_rollouts(model, store, [7], 3, use_graph=False, keep_predictions=True, bubbles=spec)
    both = evaluate_rollouts(model, store, [7], 3, use_graph=True, keep_predictions=True, bubbles=spec, heatflux=hf_spec)
    return store, spec, graph, eager, both, plain, hf_graph


def _tensors(r):
    from tests.test_gpu_heatflux_eval import _tensors as base
    out = base(r)
    if r.bubble_count_pred is not None:
        out.update({k: getattr(r, k) for k in NEW_KEYS})
    return out


def test_evaluate_rollouts_with_bubbles(tmp_path):
    from bubbleformer_amd.utils import bubble_census, kde_kl_divergence
    store, spec, graph, eager, both, plain, hf_graph = _reports()
    a, b, c, d, e = _tensors(graph), _tensors(eager), _tensors(plain), _tensors(both), _tensors(hf_graph)
    assert sorted(a) == sorted(b) and len(a) == 6 + 8 and len(c) == 6 and len(d) == 6 + 2 + 8 and plain.bubble_count_pred is None
    for k in a:
        assert torch.equal(a[k], b[k]), k                                             # graph and eager runs: the same bits
        assert torch.equal(a[k], d[k]), k                                             # the heat flux beside it moves no census row
    for k in c:
        assert torch.equal(a[k], c[k]), k                                             # nothing else moves when the census is asked for
    for k in e:
        assert torch.equal(d[k], e[k]), k                                             # and the census moves no heat-flux row
    assert graph.bubble_count_pred.shape == (1, 12) and graph.bubble_count_pred.dtype == torch.int32 and graph.bubble_area_pred.shape == (1, 12, 24)
    assert graph.vapour_fraction_pred.dtype == torch.float32 and graph.bubble_dx == 0.5 and plain.bubble_dx is None
    _, diff, div = store.out_tab
    phys = graph.predictions[0] * div.view(1, 4, 1, 1) + diff.view(1, 4, 1, 1)        # the de-normalised archive, fp32 multiply then add
    fields = store.fields
    sim = store.frames[fields.index("dfun"), 5 + 7 + 4:5 + 7 + 4 + 12, ::2, ::2]      # file 0, the twelve target frames, nearest-neighbour map of factor 2
    for side, clip in (("pred", phys[:, 0]), ("target", sim)):
        want = bubble_census(clip.contiguous(), connectivity=4, max_bubbles=24)
        assert torch.equal(getattr(graph, f"bubble_count_{side}")[0], want.count) and torch.equal(getattr(graph, f"bubble_attached_{side}")[0], want.attached)
        assert torch.equal(getattr(graph, f"bubble_area_{side}")[0], want.area) and torch.equal(getattr(graph, f"vapour_fraction_{side}")[0], want.vapour_fraction())
        print(f"{side}: bubbles per frame {want.count.tolist()}, on the heater {want.attached.tolist()}")
    assert int(graph.bubble_count_target.min()) >= 1 and int(graph.bubble_count_target.max()) <= 24
    graph.save(tmp_path / "with.pt")
    plain.save(tmp_path / "without.pt")
    with_, without = torch.load(tmp_path / "with.pt"), torch.load(tmp_path / "without.pt")
    assert sorted(without) == ["criterion", "eikonal_pred", "eikonal_target", "fields", "preds", "rel_l2", "timesteps"]
    assert sorted(set(with_) - set(without)) == NEW_KEYS and set(without) <= set(with_)
    for k in NEW_KEYS:
        assert torch.equal(with_[k], getattr(graph, k)), k
    same = lambda u, v: torch.equal(torch.nan_to_num(u, nan=-7.0, posinf=-8.0, neginf=-9.0), torch.nan_to_num(v, nan=-7.0, posinf=-8.0, neginf=-9.0))
    assert same(graph.vapour_drift(), (graph.vapour_fraction_pred - graph.vapour_fraction_target) / graph.vapour_fraction_target)
    sim_d, model_d = graph.bubble_diameters()
    for got, area in ((sim_d, graph.bubble_area_target), (model_d, graph.bubble_area_pred)):
        kept = area[area > 0].float()
        assert got.dim() == 1 and got.dtype == torch.float32 and torch.equal(got, 2.0 * torch.sqrt(kept * (0.5 * 0.5 / np.pi)))
    assert sim_d.numel() == int(graph.bubble_count_target.sum())
    # the rollout's own rows, whatever the tiny model predicts (test_report_helpers_on_known_rows has rows that are known to be populated)
    kl = graph.bubble_size_kl()
    assert kl.dim() == 0 and kl.dtype == torch.float64 and int(graph.bubble_count_pred.max()) <= 24
    by_hand = kde_kl_divergence(sim_d, model_d, 1000) if min(sim_d.numel(), model_d.numel()) >= 2 else torch.full((), float("nan"), dtype=torch.float64, device="cuda")
    assert same(kl, by_hand)
    print(f"bubble-size KL of the tiny rollout {float(kl):.5f}")
    print(f"vapour drift per frame {[f'{v:.3f}' for v in graph.vapour_drift()[0].tolist()]}, {model_d.numel()} predicted / {sim_d.numel()} simulated bubbles")


def test_trajectories_do_not_mix():
    from bubbleformer_amd.utils import BubbleSpec, HeaterSpec
    from bubbleformer_amd.utils.rollout import evaluate_rollouts
    from tests.test_gpu_heatflux_eval import _tiny_model
    store = _reports()[0]
    model = _tiny_model()
    starts, steps = [7, 38 + 9, 20], 2
    kw = dict(bubbles=BubbleSpec(connectivity=8, max_bubbles=24), heatflux=HeaterSpec(heater_temp=(1.0, 1.25), dx=1 / 2))
    batched = _tensors(evaluate_rollouts(model, store, starts, steps, **kw))
    assert len(batched) == 5 + 2 + 8
    for b, st in enumerate(starts):
        single = _tensors(evaluate_rollouts(model, store, [st], steps, **kw))
        for k, v in single.items():
            assert torch.equal(batched[k][b:b + 1], v), (b, k)
    assert not torch.equal(batched["bubble_count_target"][0], batched["bubble_count_target"][1])


def test_report_helpers_on_known_rows():
    """A report built by hand on the device: areas of known sizes, so the diameters, their divergence and the drift are known expressions."""
    from bubbleformer_amd.utils import kde_kl_divergence
    from bubbleformer_amd.utils.rollout import RolloutReport
    rng = np.random.default_rng(11)
    B, F, mb = 2, 6, 8
    area_t = np.zeros((B, F, mb), np.int32)
    area_p = np.zeros((B, F, mb), np.int32)
    count_t, count_p = rng.integers(2, mb + 1, (B, F)), rng.integers(1, mb + 1, (B, F))
    for b in range(B):
        for f in range(F):
            area_t[b, f, :count_t[b, f]] = rng.integers(1, 400, count_t[b, f])
            area_p[b, f, :count_p[b, f]] = rng.integers(1, 900, count_p[b, f])
    dev = lambda a, dtype=torch.int32: torch.from_numpy(np.asarray(a)).to(dtype).cuda()
    frac_t, frac_p = area_t.sum(-1) / 4096.0, area_p.sum(-1) / 4096.0
    z = torch.zeros(B, F, dtype=torch.int32, device="cuda")
    rep = RolloutReport(torch.zeros(B, F, 1).cuda(), torch.zeros(B, 1).cuda(), None, None, torch.zeros(B, F, dtype=torch.int64).cuda(), ["dfun"], None, None, None,
                        dev(count_p), dev(count_t), z, z, dev(frac_p, torch.float32), dev(frac_t, torch.float32), dev(area_p), dev(area_t), 0.25)
    sim, model = rep.bubble_diameters()
    want_sim = (2 * np.sqrt(area_t[area_t > 0].astype(np.float64) * 0.0625 / np.pi))
    want_model = (2 * np.sqrt(area_p[area_p > 0].astype(np.float64) * 0.0625 / np.pi))
    assert sim.shape == (int(count_t.sum()),) and model.shape == (int(count_p.sum()),) and sim.dtype == torch.float32
    assert np.allclose(sim.cpu().numpy(), want_sim, rtol=1e-6, atol=0) and np.allclose(model.cpu().numpy(), want_model, rtol=1e-6, atol=0)     # report order
    assert torch.equal(rep.bubble_diameters(dx=1.0)[0], 2.0 * torch.sqrt(dev(area_t[area_t > 0], torch.float32) * (1.0 / np.pi)))
    kl = rep.bubble_size_kl()
    assert kl.dim() == 0 and kl.dtype == torch.float64 and bool(torch.isfinite(kl)) and float(kl) > 0
    assert torch.equal(kl, kde_kl_divergence(sim, model, 1000)) and torch.equal(rep.bubble_size_kl(points=401), kde_kl_divergence(sim, model, 401))
    assert not torch.equal(kl, rep.bubble_size_kl(points=401))
    drift = rep.vapour_drift()
    assert drift.shape == (B, F) and torch.equal(drift, (rep.vapour_fraction_pred - rep.vapour_fraction_target) / rep.vapour_fraction_target)
    assert np.allclose(drift.cpu().numpy(), (frac_p - frac_t) / frac_t, rtol=1e-5)
    empty = RolloutReport(rep.rel_l2, rep.criterion, None, None, rep.timesteps, ["dfun"], None, None, None, z, dev(count_t), z, z, torch.zeros(B, F).cuda(),
                          rep.vapour_fraction_target, torch.zeros_like(rep.bubble_area_pred), rep.bubble_area_target, 0.25)
    assert empty.bubble_diameters()[1].numel() == 0 and bool(torch.isnan(empty.bubble_size_kl()))      # a model without vapour: NaN, no exception
    assert torch.equal(empty.vapour_drift(), torch.full((B, F), -1.0, device="cuda"))
