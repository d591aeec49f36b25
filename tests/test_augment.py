"""CPU: the mirror / window draw of the clip gather -- utils.augment.augment_plan against its restatement (tests/augment_restatement.py),
its distribution and its separation from the input noise's counters -- and the host side of the feature: AugmentSpec, the signatures, the
two records and the entry point's refusals."""
import ctypes
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest

from tests import augment_restatement as AR
from tests import noise_restatement as NR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = np.arange(4096)
SEEDS = (0, 3, 2 ** 63 + 42)
DRAWS = (0, 1, 5)


def _plan(**kw):
    from bubbleformer_amd.utils import AugmentSpec, augment_plan
    draw, Ho, Wo = kw.pop("draw", 0), kw.pop("Ho", 64), kw.pop("Wo", 64)
    return augment_plan(AugmentSpec(**kw), IDS, draw, Ho, Wo)


# ------------------------------------------------------------------------------------------------ the draw
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("draw", DRAWS)
@pytest.mark.parametrize("crop_y", ["bottom", "random"])
def test_plan_equals_the_restatement(seed, draw, crop_y):
    flip, x0, y0 = _plan(flip_p=0.5, crop=(40, 48), crop_y=crop_y, seed=seed, draw=draw, Ho=64, Wo=64)
    want = AR.decisions(seed, IDS, draw, 0.5, 64, 64, 40, 48, crop_y)
    assert flip.dtype == np.bool_ and flip.shape == x0.shape == y0.shape == (4096,)
    assert flip.tolist() == want[0] and x0.tolist() == want[1] and y0.tolist() == want[2]
    assert 0 <= x0.min() and x0.max() <= 16 and 0 <= y0.min() and y0.max() <= (24 if crop_y == "random" else 0)


def test_plan_counts_ids_and_draws_modulo_2_32_and_takes_any_seed():
    from bubbleformer_amd.utils import AugmentSpec, augment_plan
    spec = AugmentSpec(flip_p=0.3, crop=(5, 7), crop_y="random", seed=-1)
    assert spec.seed == 2 ** 64 - 1
    a = augment_plan(spec, [7, 2 ** 31 + 3, 0], 2 ** 32 - 1, 9, 20)
    b = augment_plan(AugmentSpec(flip_p=0.3, crop=(5, 7), crop_y="random", seed=2 ** 64 - 1), [2 ** 32 + 7, 2 ** 31 + 3, 2 ** 32], 2 ** 33 - 1, 9, 20)
    want = AR.decisions(2 ** 64 - 1, [7, 2 ** 31 + 3, 0], 2 ** 32 - 1, 0.3, 9, 20, 5, 7, "random")
    for got in (a, b):
        assert [v.tolist() for v in got] == [list(w) for w in want]
    flip, x0, y0 = augment_plan(AugmentSpec(flip_p=0.5), [1, 2, 3], 0, 6, 10)          # no crop: the whole grid, origin 0
    assert x0.tolist() == y0.tolist() == [0, 0, 0] and flip.tolist() == AR.decisions(0, [1, 2, 3], 0, 0.5, 6, 10, 6, 10)[0]
    with pytest.raises(ValueError, match="larger"):
        augment_plan(AugmentSpec(crop=(7, 10)), [0], 0, 6, 10)


@pytest.mark.parametrize("draw", DRAWS)
def test_distribution_of_mirrors_and_origins(draw):
    """Seed 3, ids 0 .. 4095: flip_p = 0.5 mirrors 2022 / 2078 / 2012 samples at draws 0 / 1 / 5 and the 17 origins of a 48-wide window on
    a 64-wide grid occur 212 .. 287 times (measured on the host).  Held: 2048 +- 160 (five binomial deviations), 241 +- 90 (six)."""
    flip, x0, y0 = _plan(flip_p=0.5, crop=(48, 48), seed=3, draw=draw)
    counts = np.bincount(x0, minlength=17)
    print("draw", draw, "mirrored", int(flip.sum()), "origin counts", int(counts.min()), "..", int(counts.max()))
    assert abs(int(flip.sum()) - 2048) <= 160
    assert counts.size == 17 and np.all(np.abs(counts - 241) <= 90)
    assert not y0.any()                                                            # crop_y = "bottom" is the default
    assert not _plan(flip_p=0.0, crop=(48, 48), seed=3, draw=draw)[0].any()
    assert _plan(flip_p=1.0, crop=(48, 48), seed=3, draw=draw)[0].all()
    ry = _plan(flip_p=0.5, crop=(48, 48), crop_y="random", seed=3, draw=draw)[2]
    assert np.all(np.abs(np.bincount(ry, minlength=17) - 241) <= 90)


def test_no_counter_block_is_one_the_noise_uses(monkeypatch):
    """Word 0 of an augmentation counter is 0xFFFFFFFF; the noise's is a group number, at most (2^31 - 1 + 3) / 4 - 1 < 2^29 for the largest
    clip bf_clip_noise accepts.  Checked on the blocks both restatements actually hand to Philox, under one seed."""
    seen = []
    real = NR.philox4x32_10

    def spy(counter, key):
        c = [np.asarray(v, dtype=np.uint64) for v in np.broadcast_arrays(*counter)]
        seen.append({tuple(int(v[i]) for v in c) for i in range(c[0].size)})
        return real(counter, key)
    monkeypatch.setattr(NR, "philox4x32_10", spy)
    AR.decisions(3, IDS, 5, 0.5, 64, 64, 48, 48)
    plan_blocks = seen.pop()
    assert plan_blocks == set(AR.counters(IDS, 5)) and all(b[0] == 0xFFFFFFFF and b[3] == 0 for b in plan_blocks)
    for sample, pas in ((0, 0), (5, 0), (4095, 1), (0xFFFFFFFF, 0)):
        NR.normals(3, sample, 5, pas, 2 * 4 * 64 * 64)
        assert not (seen.pop() & plan_blocks)
    assert 0xFFFFFFFF > (2 ** 31 - 1 + 3) // 4 - 1 and (2 ** 31 - 1 + 3) // 4 <= 2 ** 29


# ------------------------------------------------------------------------------------------------ the spec
def test_augment_spec_validation_active_and_eval_view():
    from bubbleformer_amd.utils import AugmentSpec, augment_plan
    from bubbleformer_amd.utils.augment import AugmentSpec as direct
    assert AugmentSpec is direct
    s = AugmentSpec()
    assert (s.flip_p, s.crop, s.crop_y, s.odd_fields, s.seed) == (0.0, None, "bottom", ("velx",), 0) and not s.active
    assert [f.name for f in dataclasses.fields(AugmentSpec)][:5] == ["flip_p", "crop", "crop_y", "odd_fields", "seed"]
    assert AugmentSpec(flip_p=0.25).active and AugmentSpec(crop=(4, 5)).active and AugmentSpec(flip_p=1).flip_p == 1.0
    assert AugmentSpec(crop=[4, 5], odd_fields=["velx", "nope"]).crop == (4, 5)
    assert AugmentSpec(seed=2 ** 64 + 5).seed == 5 and AugmentSpec(seed=-1).seed == 2 ** 64 - 1
    with pytest.raises(dataclasses.FrozenInstanceError):
        s.seed = 1
    for bad in (dict(flip_p=-0.1), dict(flip_p=1.5), dict(flip_p=float("nan")), dict(flip_p="0.5"), dict(flip_p=None), dict(flip_p=True),
                dict(crop=(0, 4)), dict(crop=(4,)), dict(crop=(4, 5, 6)), dict(crop=4), dict(crop=(4.0, 5)), dict(crop=(-1, 3)), dict(crop=(True, 3)),
                dict(crop_y="top"), dict(crop_y=None), dict(odd_fields="velx"), dict(odd_fields=(1,)), dict(seed=1.5), dict(seed=None), dict(seed=True)):
        with pytest.raises(ValueError):
            AugmentSpec(**bad)
    full = AugmentSpec(flip_p=0.5, crop=(4, 5), crop_y="random", seed=9)
    view = full.eval_view()
    assert view.active and view.crop == (4, 5) and view.flip_p == 0.0 and view.seed == 9
    flip, x0, y0 = augment_plan(view, [0, 1, 2 ** 31], 7, 9, 14)                     # never mirrored, centred in x, on row 0, whatever the draw
    assert not flip.any() and x0.tolist() == [(14 - 5) // 2] * 3 and y0.tolist() == [0] * 3
    assert not AugmentSpec(flip_p=0.5).eval_view().active                            # nothing to do without a crop: validation gathers plainly
    assert view.eval_view() == view


def test_signatures_accept_the_new_keywords():
    from bubbleformer_amd import ops
    from bubbleformer_amd.data.dataset import DeviceClipStore
    from bubbleformer_amd.fit import fit, validate
    from bubbleformer_amd.utils import augment_plan
    p = inspect.signature(DeviceClipStore.gather).parameters
    assert list(p) == ["self", "indices", "unroll", "augment", "draw"]
    assert p["unroll"].default is None and p["augment"].default is None and p["draw"].default == 0
    assert inspect.signature(fit).parameters["augment"].default is None
    assert inspect.signature(validate).parameters["augment"].default is None
    assert list(inspect.signature(augment_plan).parameters) == ["spec", "sample_ids", "draw", "Ho", "Wo"]
    assert callable(ops.clip_gather_augment)


def test_cpu_store_refuses_an_active_spec_and_gathers_with_an_inactive_one():
    """A crop larger than the output grid and a CPU store with an active spec raise ValueError before anything native is called; an
    inactive spec goes the plain way, which on a CPU store ends at the library's own refusal exactly as without the argument."""
    from bubbleformer_amd import _lib as L
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.utils import AugmentSpec
    g = np.random.default_rng(0)
    trajs = [{n: g.standard_normal((12, 6, 10)).astype(np.float32) for n in ("dfun", "temperature", "velx", "vely")} for _ in range(2)]
    ds = BubbleForecast.from_arrays(trajs, norm="none", time_window=2, start_time=0)
    ds.normalize()
    store = ds.device_store("cpu")
    with pytest.raises(ValueError, match="CPU store"):
        store.gather([0, 1], augment=AugmentSpec(flip_p=0.5))
    with pytest.raises(ValueError, match="larger"):
        store.gather([0, 1], augment=AugmentSpec(crop=(7, 10)))
    with pytest.raises(ValueError, match="AugmentSpec"):
        store.gather([0, 1], augment=0.5)
    for spec in (None, AugmentSpec(), AugmentSpec(flip_p=0.0)):
        with pytest.raises(L.BubbleformerHipError, match="no CPU fallback"):
            store.gather([0, 1], augment=spec, draw=3)


# ------------------------------------------------------------------------------------------------ the ABI
NEW_RECORDS = {"bf_clip_gather_job": "ClipGatherJob", "bf_clip_augment": "ClipAugment"}


def test_header_declares_the_entry_point():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "bubbleformer_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+bf_clip_gather_augment\s*\(\s*const\s+bf_clip_gather_job\s*\*\s*\w+\s*,\s*const\s+bf_clip_augment\s*\*\s*\w+\s*,\s*bf_stream_t\s+\w+\s*\)\s*;", txt)
    from bubbleformer_amd import _lib
    res, args = _lib.SIGNATURES["bf_clip_gather_augment"]
    assert res is ctypes.c_int and len(args) == 3
    assert args[0]._type_ is _lib.ClipGatherJob and args[1]._type_ is _lib.ClipAugment


@pytest.mark.parametrize("name", sorted(NEW_RECORDS))
def test_new_records_mirror_the_header(name):
    from bubbleformer_amd import _lib
    from tests.test_abi_exports import _record_fields
    rec = getattr(_lib, NEW_RECORDS[name])
    declared = _record_fields(name)
    assert [(n, t) for n, t in rec._fields_] == declared
    assert ctypes.sizeof(rec) == sum(ctypes.sizeof(t) for _, t in declared)


_BUF = []


def _records(**kw):
    """A job and a draw every check accepts -- 16-byte aligned host buffers nothing reads -- with `kw` over their fields."""
    from bubbleformer_amd import _lib as L
    if not _BUF:
        _BUF.append((ctypes.c_char * 80)())
    p = (ctypes.addressof(_BUF[0]) + 15) // 16 * 16
    job = dict(src=p, idx=p, first_tab=p, in_field=p, in_diff=p, in_div=p, in_out=p + 16, out_field=p, out_diff=p, out_div=p, out_out=p + 32,
               fluid_tab=None, file_tab=None, fluid_out=None, field_stride=12 * 6 * 10, nframes=12, nsamples=9, Cin=1, Tin=2, Cout=1, Tout=2, unroll=1,
               P=0, B=1, H=6, W=10, Ho=6, Wo=10)
    aug = dict(in_odd=p, out_odd=p, seed=3, flip_thr=2 ** 31, draw=0, Hc=4, Wc=5, crop_y=0, eval_view=0)
    job.update({k: v for k, v in kw.items() if k in job})
    aug.update({k: v for k, v in kw.items() if k in aug})
    return L.ClipGatherJob(**job), L.ClipAugment(**aug)


@pytest.mark.parametrize("defect,reason", [
    (None, "null pointer"), ("no_job", "null pointer"), ("no_draw", "null pointer"), (dict(src=None), "null pointer"), (dict(in_odd=None), "null pointer"),
    (dict(out_odd=None), "null pointer"), (dict(Hc=7), "the window must be 1 .. Ho by 1 .. Wo"), (dict(Wc=11), "the window must be 1 .. Ho by 1 .. Wo"),
    (dict(Hc=0), "the window must be 1 .. Ho by 1 .. Wo"), (dict(Wc=0), "the window must be 1 .. Ho by 1 .. Wo"), (dict(unroll=0), "bad unroll count or frame count"),
    (dict(Ho=7), "bad sizes"), (dict(flip_thr=2 ** 32 + 1), "bad flip threshold, crop_y or eval_view")],
    ids=lambda v: "-".join(f"{k}_{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_entry_point_refuses_null_records_and_windows_larger_than_the_grid(defect, reason):
    """Every check of bf_clip_gather_augment comes before any HIP call: no GPU needed, and no valid call is made here."""
    from bubbleformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    h = _lib.lib()
    job, aug = _records(**(defect if isinstance(defect, dict) else {}))
    j = None if defect in (None, "no_job") else ctypes.byref(job)
    a = None if defect in (None, "no_draw") else ctypes.byref(aug)
    assert h.bf_clip_gather_augment(j, a, None) != 0
    assert h.bf_last_error().decode().endswith("bf_clip_gather_augment: " + reason), h.bf_last_error()
