"""Bubble matching on the GPU: `bubble_match` against the numpy restatement of tests/match_restatement.py in both storage regimes of the overlap
table, on degenerate, truncated and large frames and at the edge of the IoU bound; `evaluate_rollouts(bubbles=BubbleSpec(match=True))` against
`bubble_match` of its archive and the stored target frames, against the runs without matching, and its report methods against the same
quotients formed on the host.  Integer rows are compared with ==, and so is the displacement (the build's fp64 divide
and root are correctly rounded).  Every case first asserts on the restatement's own output that its input holds what the case is about."""
import functools

import numpy as np
import pytest
import torch

from tests import bubbles_restatement as R
from tests import match_restatement as M
from tests.test_bubble_match import MATCH_KEYS
from tests.test_rollout_eval import FILES

pytestmark = pytest.mark.gpu
CENSUS = tuple(f"{k}_{side}" for side in ("pred", "target") for k in ("count", "attached", "area"))


def _match(phi_p, phi_s, **kw):
    from bubbleformer_amd.utils import bubble_match
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return bubble_match(cuda(phi_p), cuda(phi_s), **kw)


def _assert_rows(got, want, what, index=None):
    """The BubbleMatch `got` (or pair `index` of a batch) against the restatement's stacked rows: every figure exactly."""
    for k in M.ROWS + CENSUS:
        v = getattr(got, k) if index is None else getattr(got, k)[index]
        w = np.asarray(want[k])
        assert v.dtype == (torch.float32 if k == "displacement" else torch.int32), k
        if k == "displacement":
            print(f"{what}: displacement, largest |difference| {np.nanmax(np.abs(v.cpu().numpy().astype(np.float64) - w), initial=0.0):.3g}")
        assert np.array_equal(v.cpu().numpy(), w, equal_nan=True), (what, k)


def _same_bits(a, b, what, index=None):
    for k in M.ROWS + CENSUS:
        u, v = getattr(a, k), getattr(b, k) if index is None else getattr(b, k)[index]
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), (what, k)           # the displacement by its bits


def _fields(pairs, seed=0):
    """[(mask_p, mask_s), ...] of one shape -> (phi_p, phi_s), each (F, H, W) float32."""
    phis = [M.phi_pair(pair, seed=seed + 2 * i) for i, pair in enumerate(pairs)]
    return np.stack([p for p, _ in phis]), np.stack([s for _, s in phis])


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (5, 1)])
def test_degenerate_frames(shape):
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    none, full, dots = np.zeros(shape, bool), np.ones(shape, bool), (y + x) % 2 == 0
    phi_p, phi_s = _fields([(none, none), (full, full), (none, dots), (dots, none), (full, dots), (dots, dots)])
    want = M.match_fields(phi_p, phi_s, max_bubbles=8)
    c = want["counts"]
    assert c[0].tolist() == [0] * 6 and want["mask"][0].tolist() == [0, 0]                           # both sides all liquid
    assert c[1].tolist() == [1, 0, 0, 1, 0, 0] and want["mask"][1].tolist() == [x.size, x.size]      # both all vapour: one heater hit
    assert c[2][0] == 0 and c[2][1] == want["count_target"][2] > 0 and want["count_pred"][2] == 0    # nothing predicted: every bubble a miss
    assert c[3][0] == 0 and c[3][2] == want["count_pred"][3] > 0 and want["count_target"][3] == 0    # nothing simulated: every bubble a false alarm
    assert c[5][0] == want["count_pred"][5] == len(want["tables"][5]) and not want["displacement"][5].any()
    got = _match(phi_p, phi_s, max_bubbles=8)
    assert got.match_pred.shape == (6, 8) and got.counts.shape == (6, 6) and got.mask.shape == (6, 2) and got.displacement.shape == (6, 8)
    _assert_rows(got, want, shape)


def test_table_in_lds():
    """24 x 31, ten predicted and twelve simulated bubbles: a 10 x 12 table, in LDS."""
    from bubbleformer_amd import ops
    phi_p, phi_s = _fields([M.mixed_pair()])
    assert phi_p.shape == (1, 24, 31)
    for conn in R.CONNECTIVITIES:
        want = M.match_fields(phi_p, phi_s, conn)
        table, c = want["tables"][0], dict(zip(M.COUNTS, want["counts"][0].tolist()))
        assert table.shape == (10, 12 if conn == 4 else 11) and table.size <= ops.bubble_links_lds_entries()
        assert min(c["hits"], c["misses"], c["false_alarms"], c["heater_hits"], c["heater_misses"], c["heater_false_alarms"]) >= 1, c
        assert ((table > 0).sum(1) >= 2).any() and ((table > 0).sum(0) >= 2).any()                   # a predicted blob over two bubbles; two inside one
        assert any(row.max() > 0 and (row == row.max()).sum() >= 2 for row in table)                  # a tie
        mp, att_p, att_s = want["match_pred"][0], want["attached_pred"][0], want["attached_target"][0]
        assert any(0 < mp[i] and mp[i] > att_s for i in range(att_p))                                 # on the heater in the prediction only, and matched
        assert len(np.unique(want["displacement"][0])) >= 5
        got = _match(phi_p, phi_s, connectivity=conn)
        _assert_rows(got, want, ("mixed", conn))
    # the methods of the record against the same quotients on the host
    assert np.array_equal(got.iou().cpu().numpy(), M.iou(want), equal_nan=True) and np.isfinite(M.iou(want)).sum() == c["hits"]
    for attached in (False, True):
        for mine, theirs in zip((got.precision(attached), got.recall(attached), got.csi(attached)), M.scores(want["counts"], attached)):
            assert mine.dtype == torch.float32 and np.array_equal(mine.cpu().numpy(), theirs) and np.isfinite(theirs).all()
    assert np.array_equal(got.mask_iou().cpu().numpy(), (want["mask"][:, 0] / want["mask"][:, 1].astype(np.float64)).astype(np.float32))
    mean = (want["displacement"].astype(np.float64).sum(-1) * 0.25 / c["hits"]).astype(np.float32)
    assert np.array_equal(got.centroid_error(0.25).cpu().numpy(), mean)


def test_table_in_the_workspace_and_truncation():
    """34 x 34 isolated cells, 289 a side with 256 records each: a 256 x 256 table, in the workspace; bubbles 257 .. 289 have no record."""
    from bubbleformer_amd import ops
    masks = M.single_cells()
    phi_p, phi_s = _fields([masks])
    want = M.match_fields(phi_p, phi_s, max_bubbles=256)
    assert want["count_pred"][0] == want["count_target"][0] == 289 > 256 and 256 * 256 > ops.bubble_links_lds_entries()
    c = dict(zip(M.COUNTS, want["counts"][0].tolist()))
    assert c["hits"] == 153 and c["misses"] == c["false_alarms"] == 103 and c["heater_hits"] == 17           # the upper half matches cell for cell
    recorded = 2 * 256 - c["hits"]
    assert want["mask"][0].tolist() == [153, 2 * 289 - 153] and want["mask"][0][1] > recorded                # the mask rows count the unrecorded bubbles
    _assert_rows(_match(phi_p, phi_s, max_bubbles=256), want, "single cells")
    few = M.match_fields(phi_p, phi_s, max_bubbles=100)                                                      # 100 x 100: in LDS, the same mask rows
    assert few["mask"][0].tolist() == want["mask"][0].tolist() and few["counts"][0][0] == 100
    _assert_rows(_match(phi_p, phi_s, max_bubbles=100), few, "single cells, 100 records")


def test_threshold_edge():
    phi_p, phi_s = _fields([M.half_iou_pair()])
    above = float(np.nextafter(np.float32(0.5), np.float32(1)))
    at, over = M.match_fields(phi_p, phi_s, max_bubbles=4, min_iou=0.5), M.match_fields(phi_p, phi_s, max_bubbles=4, min_iou=above)
    assert at["overlap"][0].tolist() == [2, 0, 0, 0] and at["area_pred"][0][0] + at["area_target"][0][0] - 2 == 4      # an IoU of exactly 1 / 2
    assert at["counts"][0].tolist() == [1, 0, 0, 0, 0, 0] and over["counts"][0].tolist() == [0, 1, 1, 0, 0, 0] and not over["overlap"].any()
    _assert_rows(_match(phi_p, phi_s, max_bubbles=4, min_iou=0.5), at, "at the bound")
    _assert_rows(_match(phi_p, phi_s, max_bubbles=4, min_iou=above), over, "one ulp above the bound")
    _assert_rows(_match(phi_p, phi_s, max_bubbles=4, min_iou=1.0), over, "min_iou = 1")
    _assert_rows(_match(phi_p, phi_p, max_bubbles=4, min_iou=1.0), M.match_fields(phi_p, phi_p, max_bubbles=4, min_iou=1.0), "identical, min_iou = 1")


def test_large_frame():
    from bubbleformer_amd import ops
    phi_p, phi_s = _fields([M.large_pair()])
    assert phi_p[0].size == 208 * 200 > ops.bubble_census_lds_cells()
    want = M.match_fields(phi_p, phi_s)
    c = dict(zip(M.COUNTS, want["counts"][0].tolist()))
    assert c["hits"] == 4 and c["misses"] == c["false_alarms"] == 1 and c["heater_hits"] == 1 and (want["displacement"][0][:5] > 0).sum() == 4
    _assert_rows(_match(phi_p, phi_s), want, "large")


def test_same_bits_alone_and_in_a_batch():
    """Five 34 x 34 pairs, tables in the workspace and in LDS side by side: two calls give the same bits, and a pair alone the bits it has in the batch."""
    shape = (34, 34)
    cells, none = M.single_cells(), np.zeros(shape, bool)
    pairs = [cells, (R.blobs(shape, 5, 12), R.blobs(shape, 6, 12)), cells[::-1], (none, cells[1]), (R.blobs(shape, 7, 9), cells[0])]
    phi_p, phi_s = _fields(pairs)
    want = M.match_fields(phi_p, phi_s)
    assert want["counts"][1][0] >= 1 and want["counts"][4][0] >= 1 and want["counts"][3].tolist()[:3] == [0, 256, 0]
    assert [t.size > 16384 for t in want["tables"]] == [True, False, True, False, False]
    batch = _match(phi_p, phi_s)
    _assert_rows(batch, want, "batch of five")
    _same_bits(batch, _match(phi_p, phi_s), "two calls")
    for k in range(5):
        _same_bits(_match(phi_p[k], phi_s[k]), batch, ("alone", k), index=k)
    stacked = _match(phi_p.reshape(5, 1, 34, 34), phi_s.reshape(5, 1, 34, 34))                             # leading dims kept
    assert stacked.counts.shape == (5, 1, 6) and torch.equal(stacked.counts[:, 0], batch.counts)


def test_a_census_that_gave_up_and_argument_checks():
    """count = -1 on one side of a pair, written by hand: -1 in every integer row of that pair and NaN in its displacement; the pair beside it as ever."""
    from bubbleformer_amd import _lib, ops
    from bubbleformer_amd.utils import bubble_census
    phi_p, phi_s = _fields([M.mixed_pair(), M.mixed_pair()[::-1]])
    sides = [bubble_census(torch.from_numpy(phi).cuda(), max_bubbles=16, return_labels=True) for phi in (phi_p, phi_s)]
    sides[1].count[0] = -1
    rows = {k: torch.zeros(shape, dtype=dtype, device="cuda") for k, (shape, dtype) in ops._match_rows((2,), 16).items()}
    args = [c.labels for c in sides] + [c.count for c in sides] + [c.attached for c in sides] + [c.area for c in sides]
    ops.bubble_match(*args, 0.0, ops.bubble_match_workspace(2, 16, "cuda"), rows)
    want = M.match_fields(phi_p, phi_s, max_bubbles=16)
    for k in M.INT_ROWS:
        assert bool((rows[k][0] == -1).all()) and np.array_equal(rows[k][1].cpu().numpy(), want[k][1]), k
    assert bool(torch.isnan(rows["displacement"][0]).all()) and np.array_equal(rows["displacement"][1].cpu().numpy(), want["displacement"][1])
    with pytest.raises(_lib.BubbleformerHipError, match="2\\^15"):
        ops.bubble_match_workspace(1, (1 << 15) + 1, "cuda")
    with pytest.raises(_lib.BubbleformerHipError, match="workspace"):
        ops.bubble_match(*args, 0.0, torch.empty(16, dtype=torch.uint8, device="cuda"), rows)
    with pytest.raises(_lib.BubbleformerHipError, match="min_iou"):
        ops.bubble_match(*args, 1.5, ops.bubble_match_workspace(2, 16, "cuda"), rows)
    with pytest.raises(_lib.BubbleformerHipError, match="displacement"):
        ops.bubble_match(*args, 0.0, ops.bubble_match_workspace(2, 16, "cuda"), {**rows, "displacement": rows["overlap"]})
    with pytest.raises(_lib.BubbleformerHipError, match="labels_tgt"):
        ops.bubble_match(args[0], args[1][:, :-1].contiguous(), *args[2:], 0.0, ops.bubble_match_workspace(2, 16, "cuda"), rows)


STARTS, STEPS, SPEC = [7, 38 + 9], 2, dict(max_bubbles=24, dx=1 / 2, min_iou=0.1)


@functools.lru_cache(maxsize=None)
def _reports(factor):
    """A tiny avit rolled out over two trajectories, two steps of four frames, on the sample files downsampled by `factor`: with matching in a
    graph and eagerly, with tracking and matching, with tracking alone and with the census alone."""
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.utils import BubbleSpec
    from bubbleformer_amd.utils.rollout import evaluate_rollouts
    from tests.test_gpu_heatflux_eval import _tiny_model
    ds = BubbleForecast(FILES, norm="std", downsample_factor=factor, time_window=4, start_time=5)
    ds.normalize()
    store = ds.device_store("cuda")
    model = _tiny_model()
    run = lambda graph, **kw: evaluate_rollouts(model, store, STARTS, STEPS, use_graph=graph, keep_predictions=True, bubbles=BubbleSpec(**SPEC, **kw))
    return store, {"graph": run(True, match=True), "eager": run(False, match=True), "both": run(True, track=True, match=True), "track": run(True, track=True),
                   "census": run(True)}


def _tensors(r):
    from tests.test_gpu_bubble_tracks import _tensors as base
    out = base(r)
    if r.bubble_match_counts is not None:
        out.update({k: getattr(r, k).view(torch.int32) for k in MATCH_KEYS})           # the displacement by its bits
    return out


@pytest.mark.parametrize("factor", [1, 2])
def test_evaluate_rollouts_with_matching(factor, tmp_path):
    from bubbleformer_amd.utils import bubble_match
    from bubbleformer_amd.utils.rollout import plan_rollouts
    store, r = _reports(factor)
    t = {name: _tensors(rep) for name, rep in r.items()}
    assert sorted(t["graph"]) == sorted(t["eager"]) and len(t["graph"]) == len(t["census"]) + 6 and len(t["both"]) == len(t["track"]) + 6
    for k in t["graph"]:
        assert torch.equal(t["graph"][k], t["eager"][k]), k                           # graph and eager runs: the same bits
        assert torch.equal(t["graph"][k], t["both"][k]), k                            # tracking beside it moves no match row
    for k in t["track"]:
        assert torch.equal(t["both"][k], t["track"][k]), k                            # matching moves no link row and nothing else of the report
    for k in t["census"]:
        assert torch.equal(t["graph"][k], t["census"][k]), k
    for name in ("track", "census"):                                                  # match=False: no match rows
        assert all(getattr(r[name], k) is None for k in MATCH_KEYS) and not set(MATCH_KEYS) & set(t[name])
    g = r["graph"]
    hw, F = 64 // factor, STEPS * 4
    assert g.bubble_match_pred.shape == (2, F, 24) and g.bubble_match_counts.shape == (2, F, 6) and g.bubble_mask_cells.shape == (2, F, 2)
    assert g.bubble_match_displacement.dtype == torch.float32 and g.bubble_match_displacement.shape == (2, F, 24)
    _, diff, div = store.out_tab
    phys = g.predictions * div.view(1, 1, 4, 1, 1) + diff.view(1, 1, 4, 1, 1)         # the de-normalised archive, fp32 multiply then add
    first = plan_rollouts(store.ds, STARTS, STEPS).first
    sim = torch.stack([store.frames[store.fields.index("dfun"), f0 + 4:f0 + 4 + F, ::factor, ::factor] for f0 in first])     # the raw target frames on the model's grid
    assert sim.shape == (2, F, hw, hw)
    want = bubble_match(phys[:, :, 0].contiguous(), sim.contiguous(), max_bubbles=24, min_iou=0.1)
    host = M.match_fields(phys[:, :, 0].reshape(2 * F, hw, hw).cpu().numpy(), sim.reshape(2 * F, hw, hw).cpu().numpy(), max_bubbles=24, min_iou=0.1)
    counts = host["counts"].reshape(2, F, 6)
    print(f"factor {factor}: hits, misses, false alarms per frame {counts[..., :3].tolist()}")
    assert (host["count_target"] > 0).all() and min(counts[..., q].sum() for q in range(3)) > 0     # hits, misses and false alarms all occur
    for mine, theirs in (("bubble_match_pred", "match_pred"), ("bubble_match_target", "match_target"), ("bubble_match_overlap", "overlap"),
                         ("bubble_match_displacement", "displacement"), ("bubble_match_counts", "counts"), ("bubble_mask_cells", "mask")):
        assert torch.equal(getattr(g, mine).view(torch.int32), getattr(want, theirs).view(torch.int32)), mine
        assert np.array_equal(getattr(g, mine).cpu().numpy().reshape(host[theirs].shape), host[theirs], equal_nan=True), mine
    assert torch.equal(g.bubble_area_pred, want.area_pred) and torch.equal(g.bubble_count_target, want.count_target)
    # the report's methods against the same quotients on the host
    rows = {k: host[k].reshape((2, F) + host[k].shape[1:]) for k in M.ROWS + CENSUS}
    for attached in (False, True):
        for mine, theirs in zip(g.bubble_detection(attached), M.scores(rows["counts"], attached)):
            assert mine.shape == (2, F) and np.array_equal(mine.cpu().numpy(), theirs, equal_nan=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(g.mask_iou().cpu().numpy(), (rows["mask"][..., 0] / rows["mask"][..., 1].astype(np.float64)).astype(np.float32), equal_nan=True)
        assert np.array_equal(g.matched_iou().cpu().numpy(), M.iou(rows), equal_nan=True)
        n = (rows["match_pred"] > 0).sum(-1)
        mean = np.where(n > 0, rows["displacement"].astype(np.float64).sum(-1) * 0.5 / n, np.nan).astype(np.float32)
    assert np.array_equal(g.centroid_error().cpu().numpy(), mean, equal_nan=True) and np.array_equal(g.centroid_error(0.5).cpu().numpy(), mean, equal_nan=True)   # the census' dx
    g.save(tmp_path / "matched.pt")
    r["census"].save(tmp_path / "plain.pt")
    with_, without = torch.load(tmp_path / "matched.pt"), torch.load(tmp_path / "plain.pt")
    assert sorted(set(with_) - set(without)) == MATCH_KEYS and set(without) <= set(with_)


def test_ensemble_rows_follow_the_census_rows():
    """With ensemble=: one row per member trajectory, as the census rows."""
    from bubbleformer_amd.utils import BubbleSpec, EnsembleSpec
    from bubbleformer_amd.utils.rollout import evaluate_rollouts
    from tests.test_gpu_heatflux_eval import _tiny_model
    store, r = _reports(2)
    ens = evaluate_rollouts(_tiny_model(), store, STARTS, STEPS, bubbles=BubbleSpec(**SPEC, match=True), ensemble=EnsembleSpec(2, 0.0))
    assert ens.bubble_match_counts.shape == (4, STEPS * 4, 6) == ens.bubble_count_pred.shape + (6,)
    for m in range(2):                                                                # no noise: every member is the plain run
        assert torch.equal(ens.bubble_match_counts[2 * m:2 * m + 2], r["graph"].bubble_match_counts)
        assert torch.equal(ens.bubble_match_pred[2 * m:2 * m + 2], r["graph"].bubble_match_pred)
