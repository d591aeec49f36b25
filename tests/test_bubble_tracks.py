"""CPU: the bubble links, events and track ids as tests/tracks_restatement.py states them, on the synthetic sequences and on the two sample
files (the event totals below were counted once, from the definitions of DESIGN.md section 17); `BubbleSpec(track=...)`, the tracking
helpers of `RolloutReport` on hand-written rows, and the ABI's declarations.  tests/test_gpu_bubble_tracks.py holds the kernels to the same
restatement."""
import dataclasses
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import bubbles_restatement as R
from tests import tracks_restatement as TR
from tests.test_bubble_census import sample_dfun

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACK_KEYS = ["bubble_departure_area_pred", "bubble_departure_area_target", "bubble_events_pred", "bubble_events_target", "bubble_predecessor_pred",
              "bubble_predecessor_target", "bubble_successor_pred", "bubble_successor_target"]
# (connectivity, max_bubbles, file) -> births, deaths, merges, splits, departures over the file's 49 pairs
FIXTURE_EVENTS = {(4, 256, 1): (10, 8, 28, 22, 3), (4, 256, 2): (20, 8, 39, 27, 3), (8, 256, 1): (6, 5, 35, 32, 1), (8, 256, 2): (14, 5, 38, 30, 5),
                  (4, 8, 1): (26, 22, 24, 19, 2), (4, 8, 2): (46, 34, 35, 23, 1)}


@functools.lru_cache(maxsize=None)
def restated(name, connectivity=4, max_bubbles=256):
    """tracks_restatement.tracks of a named sequence, computed once: "rising", "falling" (its reversal), "dots", "sample1", "sample2"."""
    if name.startswith("sample"):
        return TR.tracks(sample_dfun(int(name[-1])), connectivity, max_bubbles)
    masks = {"rising": TR.rising_discs(), "falling": TR.rising_discs()[::-1], "dots": TR.dense_dots()}[name]
    return TR.tracks(TR.phi_of_sequence(masks), connectivity, max_bubbles)


def _events(t):
    return {i: dict(zip(TR.EVENTS, e.tolist())) for i, e in enumerate(t["events"]) if e.any()}


def test_links_of_a_hand_made_pair():
    la = np.array([[1, 1, 0, 2], [0, 0, 0, 2], [3, 0, 4, 4]], np.int32)
    lb = np.array([[1, 1, 1, 1], [0, 0, 0, 0], [0, 0, 2, 2]], np.int32)
    got = TR.links(la, 4, lb, 2, 2, 1, np.array([2, 2, 1, 2], np.int32), max_bubbles=5)
    assert got["overlap"].tolist() == [[2, 0], [1, 0], [0, 0], [0, 2]]
    assert got["successor"].tolist() == [1, 1, 0, 2, 0] and got["n_successors"].tolist() == [1, 1, 0, 1, 0]
    assert got["predecessor"].tolist() == [1, 4, 0, 0, 0] and got["n_predecessors"].tolist() == [2, 1, 0, 0, 0]
    assert got["events"].tolist() == [0, 1, 1, 0, 0] and not got["departure_area"].any()
    # bubble 4 of a is not attached; with every bubble of a on the heater and none of b, bubbles 1 and 4 depart (2 merged into 1's successor)
    got = TR.links(la, 4, lb, 2, 4, 0, np.array([2, 2, 1, 2], np.int32), max_bubbles=5)
    assert got["departure_area"].tolist() == [2, 0, 0, 2, 0] and got["events"].tolist() == [0, 1, 1, 0, 2]
    tie = TR.links(np.array([[1, 1, 2, 2]], np.int32), 2, np.array([[1, 2, 1, 2]], np.int32), 2, 0, 0, np.array([2, 2], np.int32))
    assert tie["successor"].tolist() == [1, 1] and tie["predecessor"].tolist() == [1, 1] and tie["events"].tolist() == [0, 0, 2, 2, 0]    # ties: the smallest
    cut = TR.links(la, 2, lb, 1, 2, 1, np.array([2, 2], np.int32), max_bubbles=2)                     # labels above ka / kb are liquid
    assert cut["overlap"].tolist() == [[2], [1]] and cut["events"].tolist() == [0, 0, 1, 0, 0]
    ids, n = TR.track_ids([2, 2, 1], np.array([[1, 0], [-1, -1]]), np.array([[1, 0], [-1, -1]]), 2)
    assert ids.tolist() == [[1, 2], [1, 3], [4, 0]] and n == 4                                        # a pair of -1 ends every track


def test_restatement_on_the_rising_discs():
    t = restated("rising")
    assert t["count"].tolist() == [4, 4, 4, 4, 4, 3, 4, 4, 3, 3, 3, 3]
    zero = dict.fromkeys(TR.EVENTS, 0)
    assert _events(t) == {4: {**zero, "deaths": 1, "departures": 1}, 5: {**zero, "births": 1}, 7: {**zero, "merges": 1}}
    assert np.count_nonzero(t["departure_area"]) == 1 and t["departure_area"][4, 0] == t["area"][4, 0] > 0      # the rising disc, bubble 1 of frame 4
    assert t["n_tracks"] == 5 and t["track_id"].max() == 5
    back = restated("falling")
    assert _events(back) == {3: {**zero, "splits": 1}, 5: {**zero, "deaths": 1}, 6: {**zero, "births": 1}} and not back["departure_area"].any()


@pytest.mark.parametrize("key", sorted(FIXTURE_EVENTS))
def test_restatement_on_the_sample_files(key):
    conn, mb, k = key
    t = restated(f"sample{k}", conn, mb)
    assert t["events"].shape == (49, 5) and tuple(t["events"].sum(0)) == FIXTURE_EVENTS[key]
    assert (t["departure_area"] > 0).sum() == FIXTURE_EVENTS[key][4]
    assert t["n_tracks"] == t["track_id"].max() == len(np.unique(t["track_id"][t["track_id"] > 0]))


def test_restatement_on_the_dense_dots():
    t = restated("dots")
    assert t["count"].tolist() == [360, 360] and np.count_nonzero(t["successor"]) == 256 and np.count_nonzero(t["predecessor"]) == 256
    assert t["events"].tolist() == [[0, 0, 0, 0, 0]] and t["n_successors"].max() == 1 and t["n_predecessors"].max() == 1
    assert t["successor"][0].tolist() == list(range(1, 257))


def test_spec_and_exports():
    from bubbleformer_amd import utils
    from bubbleformer_amd.utils import BubbleSpec, BubbleTracks, bubble_tracks, physics
    assert physics.bubble_tracks is bubble_tracks and utils.BubbleTracks is BubbleTracks
    assert BubbleSpec().track is False and BubbleSpec(track=True).track is True
    assert [f.name for f in dataclasses.fields(BubbleSpec)] == ["sdf_field", "connectivity", "max_bubbles", "dx", "track"]
    for bad in (dict(track=1), dict(track="yes"), dict(track=None), dict(track=True, max_bubbles=(1 << 15) + 1), dict(track=True, connectivity=6)):
        with pytest.raises(ValueError):
            BubbleSpec(**bad)
    assert BubbleSpec(max_bubbles=(1 << 15) + 1).track is False                       # the census alone has no such limit
    with pytest.raises(ValueError, match="T, H, W"):
        bubble_tracks(torch.zeros(3, 3))
    with pytest.raises(ValueError, match="connectivity"):
        bubble_tracks(torch.zeros(2, 3, 3), connectivity=5)
    with pytest.raises(ValueError, match="max_bubbles"):
        bubble_tracks(torch.zeros(2, 3, 3), max_bubbles=1 << 16)
    from bubbleformer_amd import _lib
    with pytest.raises(_lib.BubbleformerHipError):                                    # no CPU fallback
        bubble_tracks(torch.zeros(2, 3, 3))


def _report(track, B=2, F=4, mb=3):
    """A census report on CPU rows written by hand; with `track` also link rows with known departures."""
    from bubbleformer_amd.utils.rollout import RolloutReport
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)
    z = torch.zeros(B, F, dtype=torch.int32)
    r = RolloutReport(torch.zeros(B, F, 1), torch.zeros(B, 1), None, None, torch.zeros(B, F, dtype=torch.int64), ["dfun"], None, None, None, z, z, z, z,
                      torch.zeros(B, F), torch.zeros(B, F), torch.zeros(B, F, mb, dtype=torch.int32), torch.zeros(B, F, mb, dtype=torch.int32), 0.5)
    if track:
        r.bubble_departure_area_target = i32([[[4, 0, 0], [0, 0, 0], [0, 16, 0]], [[0, 0, 0], [9, 0, 1], [0, 0, 0]]])
        r.bubble_departure_area_pred = i32([[[0, 0, 0], [0, 0, 0], [0, 0, 0]], [[0, 0, 0], [0, 0, 0], [0, 0, 25]]])
        r.bubble_events_target = i32([[[0, 0, 0, 0, 1], [1, 0, 0, 0, 0], [0, 0, 0, 0, 1]], [[0, 0, 0, 0, 0], [0, 2, 0, 0, 2], [0, 0, 1, 0, 0]]])
        r.bubble_events_pred = i32([[[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]], [[-1, -1, -1, -1, -1], [0, 0, 0, 0, 0], [0, 0, 0, 0, 1]]])
        r.bubble_successor_pred = r.bubble_successor_target = r.bubble_predecessor_pred = r.bubble_predecessor_target = torch.zeros(B, F - 1, mb, dtype=torch.int32)
    return r


def test_report_helpers_and_saved_keys(tmp_path):
    """Fails without the feature: the report has no tracking fields or methods."""
    from bubbleformer_amd.utils.rollout import RolloutReport
    names = [f.name for f in dataclasses.fields(RolloutReport)]
    at = names.index("bubble_dx")
    assert sorted(names[at + 1:]) == TRACK_KEYS                                       # appended behind the census' fields: positional callers keep working
    plain, tracked = _report(False), _report(True)
    for name in TRACK_KEYS:
        assert getattr(plain, name) is None
    for call in (plain.bubble_track_ids, plain.departure_diameters, plain.departure_frequency, plain.departure_diameter_kl):
        with pytest.raises(ValueError, match="track=True"):
            call()
    bare = RolloutReport(torch.zeros(1, 2, 1), torch.zeros(1, 1), None, None, torch.zeros(1, 2, dtype=torch.int64), ["dfun"])
    with pytest.raises(ValueError, match="track=True"):
        bare.departure_frequency()
    sim, model = tracked.departure_diameters()
    want = lambda cells: [float(np.float32(2.0) * np.sqrt(np.float32(c) * np.float32(0.25 / np.pi))) for c in cells]
    assert sim.dtype == torch.float32 and np.allclose(sim.tolist(), want([4, 16, 9, 1]), rtol=1e-6) and np.allclose(model.tolist(), want([25]), rtol=1e-6)
    assert np.allclose(tracked.departure_diameters(dx=1.0)[1].tolist(), [2 * np.sqrt(25 / np.pi)], rtol=1e-6)
    f_sim, f_model = tracked.departure_frequency()
    assert f_sim.dtype == torch.float64 and f_sim.tolist() == [2 / 3, 2 / 3] and f_model.tolist() == [0.0, 0.5]       # an invalid pair (-1) is no pair
    assert bool(torch.isnan(tracked.departure_diameter_kl()))                         # one model departure: no density
    plain.save(tmp_path / "plain.pt")
    tracked.save(tmp_path / "tracked.pt")
    without, with_ = torch.load(tmp_path / "plain.pt"), torch.load(tmp_path / "tracked.pt")
    assert sorted(set(with_) - set(without)) == TRACK_KEYS and set(without) <= set(with_)
    assert not any(k.startswith(("bubble_events", "bubble_successor", "bubble_predecessor", "bubble_departure")) for k in without)
    for k in TRACK_KEYS:
        assert torch.equal(with_[k], getattr(tracked, k)), k


def test_entry_points_are_declared_and_bound():
    from bubbleformer_amd import _lib, ops
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "bubbleformer_hip.h")).read(), flags=re.S)
    assert not re.search(r"\bbf_rollout_bubbles_labelled\b", txt)                     # bf_rollout_bubbles takes the ring itself
    for name in ("bf_bubble_links", "bf_bubble_links_ws_bytes", "bf_bubble_links_lds_entries", "bf_bubble_track_ids", "bf_rollout_bubble_links"):
        assert name in _lib.SIGNATURES, name
        m = re.search(r"\b(?:int|int64_t)\s+%s\s*\((.*?)\)\s*;" % name, txt, flags=re.S)
        assert m, name
        declared = [] if m.group(1).strip() == "void" else m.group(1).split(",")
        assert len(declared) == len(_lib.SIGNATURES[name][1]), name                   # one ctypes entry per declared parameter
    for name in ("bubble_links_workspace", "bubble_links_lds_entries", "bubble_links", "bubble_track_ids", "rollout_bubbles_labelled", "rollout_bubble_links"):
        assert callable(getattr(ops, name)), name


def test_workspace_query():
    """The query needs no GPU: 16 bytes, plus a max_bubbles^2 int32 table per pair when that is more than the LDS budget; 0 out of range."""
    from bubbleformer_amd import _lib
    h = _lib.lib()
    lds = h.bf_bubble_links_lds_entries()
    assert 0 < lds < 256 * 256 and lds * 4 <= 128 * 1024                              # the dense dots (a 256 x 256 table) take the workspace
    side = int(np.sqrt(lds))
    assert h.bf_bubble_links_ws_bytes(7, side) == 16 and h.bf_bubble_links_ws_bytes(7, side + 1) == 16 + 7 * 4 * (side + 1) ** 2
    assert h.bf_bubble_links_ws_bytes(3, 256) == 16 + 3 * 256 * 256 * 4
    assert h.bf_bubble_links_ws_bytes(0, 8) == 0 and h.bf_bubble_links_ws_bytes(1, 0) == 0 and h.bf_bubble_links_ws_bytes(1, (1 << 15) + 1) == 0
    assert h.bf_bubble_links_ws_bytes(1, 1 << 15) == 16 + 4 * (1 << 30)
