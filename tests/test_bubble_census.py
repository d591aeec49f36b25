"""Bubble census, the parts that need no GPU: the flood fill of tests/bubbles_restatement.py against scipy's label images and per-frame figures
(tests/golden/bubble_census.npz, tools/gen_bubble_census_golden.py), the argument checks of `BubbleSpec` / `bubble_census`, a report without
a census, and the declaration of the new entry points."""
import os
import re

import numpy as np
import pytest
import torch

from tests import bubbles_restatement as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


def golden():
    return np.load(os.path.join(GOLDEN, "bubble_census.npz"))


def sample_dfun(k):
    from bubbleformer_amd.data import hdf5_lite
    return np.asarray(hdf5_lite.File(os.path.join(GOLDEN, "samples", f"sample_{k}.hdf5"))["dfun"][:])


def test_restatement_equals_scipy_on_the_masks():
    z = golden()
    assert os.path.getsize(os.path.join(GOLDEN, "bubble_census.npz")) < 200 * 1024
    for name, mask in R.masks().items():
        assert mask.shape == R.MASK_SHAPE
        for ci, conn in enumerate(R.CONNECTIVITIES):
            want = z[f"labels/{name}/{conn}"]
            assert want.dtype == np.int16 and int(want.max()) == R.MASK_COUNTS[name][ci]
            lab, n = R.label(mask, conn)
            assert n == R.MASK_COUNTS[name][ci] and np.array_equal(lab, want), (name, conn)
            phi = R.phi_of(mask)
            assert np.array_equal(phi > 0, mask)                                      # the zeros and the NaN sit among the liquid cells
    assert np.isnan(R.phi_of(R.masks()["alternate_rows"])).sum() == 1 and (R.phi_of(R.masks()["alternate_rows"]) == 0).sum() == 2


def test_restatement_equals_scipy_on_the_sample_frames():
    z = golden()
    ranges = {(1, 4): ((9, 14), (6, 11)), (2, 4): ((13, 21), (5, 12)), (1, 8): ((7, 14), None), (2, 8): ((11, 19), None)}
    for k in (1, 2):
        dfun = sample_dfun(k)
        assert dfun.shape == (50, 64, 64) and not np.any(dfun == 0)
        for conn in R.CONNECTIVITIES:
            counts, attached, areas = z[f"sample{k}/count/{conn}"], z[f"sample{k}/attached/{conn}"], z[f"sample{k}/areas/{conn}"]
            (lo, hi), att = ranges[(k, conn)]
            assert (counts.min(), counts.max()) == (lo, hi) and (att is None or (attached.min(), attached.max()) == att)
            for f in range(0, 50, 7):                                                # every seventh frame: the generator checked them all
                c = R.census(dfun[f] > 0, conn)
                assert c["count"] == counts[f] and c["attached"] == attached[f]
                assert np.array_equal(c["area_all"], areas[f, :counts[f]]) and not areas[f, counts[f]:].any()
                assert c["on_heater"][:c["attached"]].all() and not c["on_heater"][c["attached"]:].any()       # the heater's bubbles come first


def test_census_restatement_records():
    c = R.census(R.masks()["u_around_blob"], 4)
    assert c["count"] == 2 and c["attached"] == 0 and c["area"][:3].tolist() == [21 + 21 + 19, 9, 0]
    assert c["centroid"][1].tolist() == [11.0, 19.0] and c["labels"][5, 30] == 1 and c["labels"][10, 18] == 2
    c = R.census(R.masks()["checkerboard"], 4, max_bubbles=256)
    assert c["count"] == 1440 and c["vapour_cells"] == 1440 and c["area"].tolist() == [1] * 256 and c["attached"] == 36
    assert c["on_heater"][:36].all() and not c["on_heater"][36:].any()


def test_argument_errors():
    from bubbleformer_amd import utils
    from bubbleformer_amd.utils import BubbleCensus, BubbleSpec, bubble_census
    from bubbleformer_amd.utils import physics
    assert physics.BubbleSpec is BubbleSpec and physics.bubble_census is bubble_census and utils.BubbleCensus is BubbleCensus
    spec = BubbleSpec()
    assert (spec.sdf_field, spec.connectivity, spec.max_bubbles, spec.dx) == ("dfun", 4, 256, 1 / 32)
    with pytest.raises(Exception):
        spec.connectivity = 8                                                         # frozen
    for bad in (dict(connectivity=6), dict(connectivity="4"), dict(max_bubbles=0), dict(max_bubbles=2.5), dict(dx=0.0)):
        with pytest.raises(ValueError):
            BubbleSpec(**bad)
    assert BubbleSpec(sdf_field="sdf").channel(["velx", "sdf"]) == 1
    with pytest.raises(ValueError, match="dfun"):
        spec.channel(["temperature", "velx"])
    phi = torch.zeros(2, 3, 3)
    with pytest.raises(ValueError, match="connectivity"):
        bubble_census(phi, connectivity=6)
    with pytest.raises(ValueError, match="max_bubbles"):
        bubble_census(phi, max_bubbles=0)
    with pytest.raises(ValueError, match="H, W"):
        bubble_census(torch.zeros(5))
    area = torch.tensor([[0, 1, 4]], dtype=torch.int32)
    c = BubbleCensus(torch.tensor([2]), torch.tensor([5]), torch.tensor([1]), area, torch.zeros(1, 3, 2), torch.zeros(1, 3, dtype=torch.bool), (3, 5))
    assert c.labels is None and c.vapour_fraction().dtype == torch.float32 and c.vapour_fraction().tolist() == [float(np.float32(5 / 15))]
    d = c.equivalent_diameter(dx=0.5)
    assert d.dtype == torch.float32 and d[0, 0] == 0 and np.allclose(d[0, 1:].numpy(), [2 * np.sqrt(0.25 / np.pi), 2 * np.sqrt(1.0 / np.pi)], rtol=1e-6)
    assert np.allclose(c.equivalent_diameter()[0, 2].item(), 2 * np.sqrt(4 / 1024 / np.pi), rtol=1e-6)


def test_no_cpu_census():
    from bubbleformer_amd import _lib
    from bubbleformer_amd.utils import bubble_census
    with pytest.raises(_lib.BubbleformerHipError):
        bubble_census(torch.zeros(2, 3, 3))


def test_report_without_a_census(tmp_path):
    from bubbleformer_amd.utils.rollout import RolloutReport
    r = RolloutReport(torch.zeros(1, 2, 1), torch.zeros(1, 1), None, None, torch.zeros(1, 2, dtype=torch.int64), ["dfun"])
    new = ("bubble_count_pred", "bubble_count_target", "bubble_attached_pred", "bubble_attached_target", "vapour_fraction_pred",
           "vapour_fraction_target", "bubble_area_pred", "bubble_area_target")
    names = [f.name for f in __import__("dataclasses").fields(RolloutReport)]
    at = names.index("heatflux_target")
    assert tuple(names[at + 1:at + 1 + len(new)]) == new                              # appended after heatflux_target, in this order
    for name in new:
        assert getattr(r, name) is None
    r.save(tmp_path / "plain.pt")
    assert sorted(torch.load(tmp_path / "plain.pt")) == ["criterion", "fields", "rel_l2", "timesteps"]
    for call in (r.vapour_drift, r.bubble_diameters, r.bubble_size_kl):
        with pytest.raises(ValueError, match="BubbleSpec"):
            call()
    frac = torch.tensor([[0.25, 0.5]])
    full = RolloutReport(r.rel_l2, r.criterion, None, None, r.timesteps, ["dfun"], None, None, None, *[torch.zeros(1, 2, dtype=torch.int32)] * 4,
                         frac * 1.5, frac, torch.zeros(1, 2, 4, dtype=torch.int32), torch.zeros(1, 2, 4, dtype=torch.int32))
    assert torch.equal(full.vapour_drift(), torch.tensor([[0.5, 0.5]]))
    full.save(tmp_path / "full.pt")
    assert sorted(set(torch.load(tmp_path / "full.pt")) - {"criterion", "fields", "rel_l2", "timesteps"}) == sorted(new)


def test_entry_points_are_declared_and_bound():
    from bubbleformer_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "bubbleformer_hip.h")).read(), flags=re.S)
    for name in ("bf_bubble_census", "bf_rollout_bubbles", "bf_bubble_census_ws_bytes", "bf_bubble_census_lds_cells"):
        assert name in _lib.SIGNATURES, name
        m = re.search(r"\b(?:int|int64_t)\s+%s\s*\((.*?)\)\s*;" % name, txt, flags=re.S)
        assert m, name
        declared = [] if m.group(1).strip() == "void" else m.group(1).split(",")
        assert len(declared) == len(_lib.SIGNATURES[name][1]), name                   # one ctypes entry per declared parameter
    src = open(os.path.join(REPO, "bubbleformer_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bbubbles\.hip\b", src, flags=re.M)
    csrc = os.path.join(REPO, "bubbleformer_amd", "csrc")
    texts = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip"))}
    for sig in ("float denormalise(", "int nearest_src(", "float clip_norm(", "float eikonal_l1_px("):      # one definition each, in clip_store.h
        assert {f: t.count(sig) for f, t in texts.items() if sig in t} == {"clip_store.h": 1}, sig


def test_makefile_builds_every_hip_file():
    """SRCS names exactly the *.hip files of csrc/: a file that is not listed would be left out of the library without a build error."""
    csrc = os.path.join(REPO, "bubbleformer_amd", "csrc")
    m = re.search(r"^SRCS :=(.*)$", open(os.path.join(csrc, "Makefile")).read(), flags=re.M)
    assert m
    listed = m.group(1).split()
    assert len(listed) == len(set(listed))
    assert sorted(listed) == sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))


def test_workspace_query_and_size_limit():
    """The query needs no GPU: 16 bytes of sums per record and frame, plus the parents when the frame does not fit the LDS; 0 beyond 2^24 cells."""
    from bubbleformer_amd import _lib
    h = _lib.lib()
    lds = h.bf_bubble_census_lds_cells()
    assert 192 * 192 <= lds and lds * 4 < 160 * 1024                                   # the bench geometry is labelled in LDS
    assert h.bf_bubble_census_ws_bytes(3, 64, 64, 256) == 3 * 256 * 16
    side = int(np.ceil(np.sqrt(lds + 1)))
    assert h.bf_bubble_census_ws_bytes(2, side, side, 8) == 2 * (8 * 16 + (side * side * 4 + 15) // 16 * 16)
    assert h.bf_bubble_census_ws_bytes(1, 4096, 4096, 1) > 0 and h.bf_bubble_census_ws_bytes(1, 4096, 4097, 1) == 0
    assert h.bf_bubble_census_ws_bytes(0, 8, 8, 8) == 0 and h.bf_bubble_census_ws_bytes(1, 8, 8, 0) == 0
