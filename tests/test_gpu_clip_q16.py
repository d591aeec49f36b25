"""GPU: the 16-bit device clip store (csrc/clip_store_q16.hip).  The codes and the decode are held to the numpy
restatement (tests/clip_q16_restatement.py) bit for bit; the gather is held, bit for bit, to the EXISTING fp32 kernels on the decoded frames
(``store.to_fp32().gather``); the statistics to the fp32 store's; and fit() with ``train_storage="q16"`` to fit() on the decoded frames.

Two datasets: the two 50 x 64 x 64 sample files (rows of whole quads: the 8-byte loads), and two in-memory files of 9 and 7 frames at
6 x 10 (a width that is no multiple of 4: the scalar loads and the ragged last quad).  Every store is filled with staging_frames = 7, which
divides neither 50 nor 9: those segments have chunk seams and a short last chunk, and the 7-frame file is one whole chunk."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import clip_q16_restatement as QR

pytestmark = pytest.mark.gpu

FIELDS = ["dfun", "temperature", "velx", "vely"]
SAMPLES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samples")
FILES = [os.path.join(SAMPLES, f"sample_{i}.hdf5") for i in (1, 2)]
FLUID = {"inv_reynolds": 0.0042, "cpgas": 0.83, "mugas": 0.023, "rhogas": 0.0083, "thcogas": 0.25, "stefan": 0.5, "prandtl": 8.4,
         "heater": {"nucWaitTime": 0.4, "wallTemp": 1.0}}
KINDS = ["samples", "ragged"]


def _ragged_arrays():
    g = np.random.default_rng(610)
    return [{n: (g.standard_normal((frames, 6, 10)) * (0.5 + k + 3 * fi) + (1.5 - k) * 0.8 + 0.3 - 40 * fi).astype(np.float32) for k, n in enumerate(FIELDS)}
            for fi, frames in enumerate((9, 7))]                     # the second file on another scale and offset: a wrong file's scale shows


def _dataset(kind, factor=1):
    from bubbleformer_amd.data import BubbleForecast
    if kind == "samples":
        ds = BubbleForecast(FILES, norm="std", downsample_factor=factor, time_window=2, start_time=5)
    else:
        ds = BubbleForecast.from_arrays(_ragged_arrays(), [dict(FLUID, stefan=0.5 + i) for i in range(2)], norm="std", downsample_factor=factor, time_window=2,
                                        start_time=0)
    ds.normalize()                                                   # the host path: the same constants whichever store is built next
    return ds


def _originals(ds):
    """One {field: [frames][H][W] fp32} per file, as the fill reads them."""
    return [{n: np.array(f[n][...], dtype=np.float32) for n in FIELDS} for f in ds.data]


@functools.lru_cache(maxsize=None)
def _stores(kind, factor=1):
    """(dataset, its q16 store filled through 7-frame staging buffers, the fp32 store of the decoded frames)."""
    ds = _dataset(kind, factor)
    q = ds.device_store("cuda", storage="q16", staging_frames=7)
    return ds, q, q.to_fp32()


@pytest.fixture(scope="module", autouse=True)
def _release_the_shared_stores():
    """The stores are built once and shared by this file's tests; the tests that run after it get their device memory back."""
    yield
    _stores.cache_clear()


@functools.lru_cache(maxsize=None)
def _restated(kind):
    """The restatement's store of the dataset: (codes, lo, hi, step, frame_seg), computed once."""
    return QR.store(_originals(_dataset(kind)), sorted(FIELDS))


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def _spec(**kw):
    from bubbleformer_amd.utils import AugmentSpec
    return AugmentSpec(**kw)


def _plan(spec, ids, draw, grid):
    from bubbleformer_amd.utils import augment_plan
    flip, x0, y0 = augment_plan(spec, ids, draw, *grid)
    return flip.tolist(), x0.tolist(), y0.tolist()


def _grid(kind, factor=1):
    h, w = (64, 64) if kind == "samples" else (6, 10)
    return (h // factor, w // factor) if factor > 1 else (h, w)


def _window(kind, ragged_width=False):
    """A crop for the dataset: whole quads (the sample files: 8-byte loads where x0 is a multiple of 4) or a width that is no multiple of 4."""
    if kind == "samples":
        return (40, 30) if ragged_width else (40, 32)
    return (4, 5) if ragged_width else (3, 4)


# ------------------------------------------------------------------------------------------------ codes and decode
@pytest.mark.parametrize("kind", KINDS)
def test_device_codes_are_the_restatements(kind):
    ds, q, _ = _stores(kind)
    codes, lo, hi, step, seg = _restated(kind)
    assert q.storage == "q16" and q.staging_frames == 7 and q.fields == sorted(FIELDS)
    got = q.codes.cpu().numpy().view(np.uint16)
    assert got.shape == codes.shape and np.array_equal(got, codes)
    assert np.array_equal(q.seg_lo.cpu().numpy(), lo) and np.array_equal(q.seg_step.cpu().numpy(), step) and np.array_equal(q.frame_seg.cpu().numpy(), seg)
    other = ds.device_store("cuda", storage="q16", staging_frames=3 if kind == "ragged" else 50)      # other seams, a chunk that is a whole file: the same codes
    assert torch.equal(other.codes, q.codes)


@pytest.mark.parametrize("kind", KINDS)
def test_decode_is_the_restatements_and_within_the_bound_of_the_originals(kind):
    ds, q, dec = _stores(kind)
    codes, lo, hi, step, seg = _restated(kind)
    from bubbleformer_amd.data import DeviceClipStore
    assert type(dec) is DeviceClipStore and dec.storage == "fp32" and dec.frames.dtype == torch.float32 and dec.frames.shape == q.codes.shape
    got = dec.frames.cpu().numpy()
    assert np.array_equal(got, QR.decode_store(codes, lo, step, seg))
    worst = 0.0
    for fi, traj in enumerate(_originals(ds)):
        a, b = int(q.frame0[fi]), int(q.frame0[fi + 1])
        for ci, n in enumerate(sorted(FIELDS)):
            err = float(np.abs(got[ci, a:b].astype(np.float64) - traj[n].astype(np.float64)).max())
            limit = QR.bound(lo[ci, fi], hi[ci, fi], step[ci, fi])
            worst = max(worst, err / limit)
            assert err <= limit, (n, fi, err, limit)
            assert np.array_equal(got[ci, a:b][traj[n] == lo[ci, fi]], traj[n][traj[n] == lo[ci, fi]])      # lo decodes exactly
    print(kind, "worst error / bound %.3f" % worst)


def test_a_constant_segment_decodes_exactly():
    from bubbleformer_amd.data import BubbleForecast
    trajs = _ragged_arrays()
    trajs[1]["velx"] = np.full_like(trajs[1]["velx"], np.float32(-2.75))
    ds = BubbleForecast.from_arrays(trajs, norm="none", time_window=2, start_time=0)
    ds.normalize()
    q = ds.device_store("cuda", storage="q16", staging_frames=4)
    ci = sorted(FIELDS).index("velx")
    assert float(q.seg_step[ci, 1]) == 0.0 and not q.codes[ci, 9:].any()
    assert torch.equal(q.to_fp32().frames[ci, 9:].cpu(), torch.from_numpy(trajs[1]["velx"]))


# ------------------------------------------------------------------------------------------------ the gather against the fp32 kernels
@pytest.mark.parametrize("kind", KINDS)
def test_plain_and_unrolled_gathers_are_the_fp32_kernels_on_the_decoded_frames(kind):
    ds, q, dec = _stores(kind)
    ids = [0, len(ds) - 1, 5, len(ds) // 2, 3]                                       # both files
    _same(q.gather(ids), dec.gather(ids))
    pool = ds.unrollable(2)
    ids2 = [pool[0], pool[-1], pool[len(pool) // 2]]
    got = q.gather(ids2, unroll=2)
    _same(got, dec.gather(ids2, unroll=2))
    assert got[1].shape[:2] == (2, 3) and got[1][1].is_contiguous()
    _same(q.gather(ids2, unroll=1), dec.gather(ids2, unroll=1))
    _same(q.gather(ids), q.gather(ids))                                              # two calls: the same bits
    if kind == "ragged":                                                             # the plain gather is also the restatement's, composed from its own decode
        codes, lo, hi, step, seg = _restated(kind)
        first = [int(q.frame0[fi]) + st for fi, st in (ds.locate(i) for i in ids)]
        for clip, t0, tab in ((0, 0, q.in_tab), (1, 2, q.out_tab)):
            want = QR.gather(codes, lo, step, seg, first, t0, 2, tab[0].tolist(), tab[1].cpu().numpy(), tab[2].cpu().numpy(), 6, 10)
            assert np.array_equal(q.gather(ids)[clip].cpu().numpy(), want)
        assert q.gather(ids)[2].shape == (5, 9) and torch.equal(q.gather(ids)[2], dec.gather(ids)[2])      # the fluid rows


@pytest.mark.parametrize("kind", KINDS)
def test_device_indices_out_of_range_are_clamped_as_the_fp32_gather_clamps_them(kind):
    ds, q, dec = _stores(kind)
    n = len(ds)
    idx = torch.tensor([-3, 10 ** 6, 5, n - 1, 0], device="cuda")
    _same(q.gather(idx), dec.gather(idx))
    _same(q.gather(idx), q.gather([0, n - 1, 5, n - 1, 0]))
    _same(q.gather(idx, unroll=2), dec.gather(idx, unroll=2))
    with pytest.raises(IndexError):
        q.gather([0, n])
    with pytest.raises(IndexError):
        q.gather([n - 1], unroll=2)


@pytest.mark.parametrize("kind", KINDS)
def test_unrolled_targets_that_run_into_the_next_file_take_its_scale(kind):
    """The last sample of file 0 as a DEVICE index with unroll = 3: its later target clips are the next file's first frames, which decode
    under the next file's scale (the frame read chooses it, not the sample's file); the store's last sample runs into the last frame."""
    ds, q, dec = _stores(kind)
    last0 = ds._per_traj()[0] - 1
    idx = torch.tensor([last0, len(ds) - 1, 0], device="cuda")
    got, want = q.gather(idx, unroll=3), dec.gather(idx, unroll=3)
    _same(got, want)
    first = int(q.frame0[0]) + ds.locate(last0)[1]
    frames = [first + 2 + t for t in range(6)]                                       # the six target frames of that sample
    assert frames[1] == int(q.frame0[1]) - 1 and frames[2] == int(q.frame0[1])       # clip 0 ends file 0; clips 1 and 2 are file 1's
    ids, diff, div = q.out_tab
    for t, fr in enumerate(frames):
        for c in range(4):
            assert torch.equal(got[1][t // 2, 0, t % 2, c].cpu(), (dec.frames[int(ids[c]), fr].cpu() - diff[c].cpu()) / div[c].cpu())
    ci = int(ids[0])
    assert float(q.seg_step[ci, 0]) != float(q.seg_step[ci, 1]) and float(q.seg_lo[ci, 0]) != float(q.seg_lo[ci, 1])      # the two scales do differ


@pytest.mark.parametrize("kind", KINDS)
def test_downsampled_gathers(kind):
    ds, q, dec = _stores(kind, 2)
    ids = [0, len(ds) - 1, 7]
    got = q.gather(ids)
    assert got[0].shape[-2:] == _grid(kind, 2)
    _same(got, dec.gather(ids))
    _same(q.gather(ids[:2] if kind == "ragged" else ids, unroll=1), dec.gather(ids[:2] if kind == "ragged" else ids, unroll=1))
    spec = _spec(flip_p=0.5, crop=(3, 3) if kind == "ragged" else (20, 12), crop_y="random", seed=3)
    _same(q.gather(ids, augment=spec, draw=2), dec.gather(ids, augment=spec, draw=2))


@pytest.mark.parametrize("kind", KINDS)
def test_mirrored_and_unmirrored_samples(kind):
    ds, q, dec = _stores(kind)
    spec = _spec(flip_p=0.5, seed=3)
    ids = list(range(len(ds)))[:24]
    draw = next(d for d in range(64) if 2 <= sum(_plan(spec, ids, d, _grid(kind))[0]) <= len(ids) - 2)      # mirrored and unmirrored samples in one batch
    flip = _plan(spec, ids, draw, _grid(kind))[0]
    got = q.gather(ids, augment=spec, draw=draw)
    _same(got, dec.gather(ids, augment=spec, draw=draw))
    vx = FIELDS.index("velx")
    plain = q.gather(ids)
    b = flip.index(True)
    assert torch.equal(got[0][b, :, 0], torch.flip(plain[0][b, :, 0], dims=[-1])) and not torch.equal(got[0][b, :, vx], torch.flip(plain[0][b, :, vx], dims=[-1]))
    pool = ds.unrollable(2)[:8]
    _same(q.gather(pool, unroll=2, augment=spec, draw=1), dec.gather(pool, unroll=2, augment=spec, draw=1))


@pytest.mark.parametrize("ragged_width", [False, True], ids=["whole_quads", "ragged_width"])
@pytest.mark.parametrize("kind", KINDS)
def test_windows_at_odd_and_aligned_origins(kind, ragged_width):
    """A crop whose batch holds an odd x0 beside one that is a multiple of 4 (picked from the plan), mirrored and unmirrored samples, with
    whole quads (at the sample files' aligned origins: the 8-byte loads, read back to front when mirrored) and with a width that is no
    multiple of 4."""
    ds, q, dec = _stores(kind)
    window, grid = _window(kind, ragged_width), _grid(kind)
    assert (window[1] % 4 != 0) == ragged_width
    spec = _spec(flip_p=0.5, crop=window, crop_y="random", seed=3)
    ids = list(range(len(ds)))[:16]
    draw = next(d for d in range(256) if (lambda flip, x0, y0: any(v % 2 for v in x0) and any(v % 4 == 0 and f for v, f in zip(x0, flip)) and
                                          any(v % 4 == 0 and not f for v, f in zip(x0, flip)) and max(y0) > 0)(*_plan(spec, ids, d, grid)))
    got = q.gather(ids, augment=spec, draw=draw)
    assert got[0].shape == (len(ids), 2, 4) + window and got[0].is_contiguous()
    _same(got, dec.gather(ids, augment=spec, draw=draw))
    _same(q.gather(ids, augment=_spec(crop=window, seed=3), draw=draw), dec.gather(ids, augment=_spec(crop=window, seed=3), draw=draw))      # no mirror


@pytest.mark.parametrize("kind", KINDS)
def test_eval_view(kind):
    ds, q, dec = _stores(kind)
    view = _spec(flip_p=0.5, crop=_window(kind), crop_y="random", seed=9).eval_view()
    ids = [0, len(ds) - 1, 4]
    got = q.gather(ids, augment=view, draw=5)
    _same(got, dec.gather(ids, augment=view, draw=5))
    _same(got, q.gather(ids, augment=view, draw=77))                                 # nothing is drawn
    inactive = _spec(flip_p=0.5).eval_view()
    _same(q.gather(ids, augment=inactive), q.gather(ids))


# ------------------------------------------------------------------------------------------------ statistics
def _stat_terms(ds):
    """Per (field, file) of the ORIGINAL values, in fp64 on the host: n, sum |x| and sum x^2."""
    trajs = _originals(ds)
    n = np.array([[t[f].size for t in trajs] for f in sorted(FIELDS)], dtype=np.float64)
    a1 = np.array([[np.abs(t[f].astype(np.float64)).sum() for t in trajs] for f in sorted(FIELDS)])
    a2 = np.array([[(t[f].astype(np.float64) ** 2).sum() for t in trajs] for f in sorted(FIELDS)])
    return n, a1, a2


@pytest.mark.parametrize("kind", KINDS)
def test_statistics_are_the_fp32_stores(kind):
    """The statistics taken chunk by chunk during the fill against the fp32 store's one launch over the same (original) values: min and max
    equal; the sums differ by the order of an fp64 sum only, |d sum| <= n 2^-52 sum|x| and |d sum x^2| <= n 2^-52 sum x^2."""
    from bubbleformer_amd.data import BubbleForecast
    ds = _dataset(kind)
    q = ds.device_store("cuda", storage="q16", staging_frames=7)
    f = ds.device_store("cuda")
    (sq, nq), (sf, nf) = q._segment_stats(), f._segment_stats()
    n, a1, a2 = _stat_terms(ds)
    assert np.array_equal(nq, nf) and np.array_equal(nq, n)
    assert np.array_equal(sq[..., 2], sf[..., 2]) and np.array_equal(sq[..., 3], sf[..., 3])
    print(kind, "d sum / bound %.2e" % float((np.abs(sq[..., 0] - sf[..., 0]) / (n * 2.0 ** -52 * a1)).max()),
          "d sum x^2 / bound %.2e" % float((np.abs(sq[..., 1] - sf[..., 1]) / (n * 2.0 ** -52 * a2)).max()))
    assert np.all(np.abs(sq[..., 0] - sf[..., 0]) <= n * 2.0 ** -52 * a1) and np.all(np.abs(sq[..., 1] - sf[..., 1]) <= n * 2.0 ** -52 * a2)
    assert np.array_equal(sq[..., 2], [[t[name].min() for t in _originals(ds)] for name in sorted(FIELDS)])      # of the originals, not of the decoded values


@pytest.mark.parametrize("norm", ["std", "minmax", "tanh"])
def test_normalize_and_field_std_agree_with_the_fp32_store(norm):
    """minmax / tanh read min and max alone: equal constants.  std: with ds = n 2^-52 sum|x| and ds2 = n 2^-52 sum x^2 (the sums' bounds),
    |d mean| <= ds / n, |d var| <= ds2 / n + 2 |mean| ds / n + (ds / n)^2 and |d std| <= |d var| / std (d sqrt(v) = dv / (2 sqrt v), the
    factor 2 left as room for the second order); the dataset's constants are means over the files, so the largest file's figure holds them."""
    from bubbleformer_amd.data import BubbleForecast
    make = lambda: BubbleForecast(FILES, norm=norm, time_window=2, start_time=5)      # noqa: E731
    dq, df = make(), make()
    q, f = dq.device_store("cuda", storage="q16", staging_frames=7), df.device_store("cuda")
    (diff_q, div_q), (diff_f, div_f) = q.normalize(), f.normalize()
    assert dq.diff_terms is diff_q and sorted(diff_q) == sorted(FIELDS)
    if norm != "std":
        assert diff_q == diff_f and div_q == div_f
    n, a1, a2 = _stat_terms(df)
    sf, _ = f._segment_stats()
    mean = sf[..., 0] / n
    std = np.sqrt(sf[..., 1] / n - mean ** 2)
    d_mean = 2.0 ** -52 * a1
    d_std = (2.0 ** -52 * a2 + 2 * np.abs(mean) * d_mean + d_mean ** 2) / std
    for ci, name in enumerate(sorted(FIELDS)):
        if norm == "std":
            print(name, "d diff %.2e (bound %.2e)" % (abs(diff_q[name] - diff_f[name]), d_mean[ci].max()), "d div %.2e (bound %.2e)" % (abs(div_q[name] - div_f[name]), d_std[ci].max()))
            assert abs(diff_q[name] - diff_f[name]) <= d_mean[ci].max() and abs(div_q[name] - div_f[name]) <= d_std[ci].max()
    if norm != "std":
        assert torch.equal(q.in_tab[1], f.in_tab[1]) and torch.equal(q.in_tab[2], f.in_tab[2])      # the fp32 tables the kernels read
    sq_, sf_ = q.field_std(), f.field_std()
    pooled = np.sqrt(sf[..., 1].sum(axis=1) / n.sum(axis=1) - (sf[..., 0].sum(axis=1) / n.sum(axis=1)) ** 2)
    for ci, name in enumerate(sorted(FIELDS)):
        pm = abs(sf[ci, :, 0].sum() / n[ci].sum())
        dm = 2.0 ** -52 * a1[ci].sum()
        room = (2.0 ** -52 * a2[ci].sum() + 2 * pm * dm + dm ** 2) / pooled[ci] / float(div_f[name])
        room += sf_[name] * (d_std[ci].max() / float(div_f[name]) + 2.0 ** -51)      # the two stores' div constants, and the quotient's own rounding
        assert abs(sq_[name] - sf_[name]) <= room, (name, sq_[name], sf_[name], room)


# ------------------------------------------------------------------------------------------------ residency
def test_resident_bytes_and_the_fills_peak():
    ds = _dataset("samples")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()                                             # allocated bytes, not reserved ones: what the caching allocator keeps does not count
    before = torch.cuda.memory_allocated()
    q = ds.device_store("cuda", storage="q16", staging_frames=7)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    values = 4 * 100 * 64 * 64
    assert q.codes.element_size() == 2 and q.codes.numel() == values
    staging = 7 * 64 * 64 * 4
    print("resident", q.nbytes, "fill peak above the start", peak, "allowed", q.nbytes + 2 * staging + (1 << 20))
    assert q.nbytes >= 2 * values and peak <= q.nbytes + 2 * staging + (1 << 20)
    f = ds.device_store("cuda")
    assert f.nbytes == 4 * values and q.nbytes < 0.51 * f.nbytes
    assert not hasattr(q, "frames")
    big = ds.device_store("cuda", storage="q16")                                     # the default: 64 MB's worth of frames, held to the longest file
    assert big.staging_frames == 50 and torch.equal(big.codes, q.codes)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="staging_frames"):
            ds.device_store("cuda", storage="q16", staging_frames=bad)


# ------------------------------------------------------------------------------------------------ training and evaluation
def _model():
    from bubbleformer_amd.models import get_model
    torch.manual_seed(0)
    return get_model("avit", input_fields=4, output_fields=4, time_window=2, patch_size=8, embed_dim=64, num_heads=2, processor_blocks=1, drop_path=0.0,
                     compute_dtype=torch.float32).cuda()


def _fit(train_set, **kw):
    from bubbleformer_amd.fit import fit
    hist = fit(_model(), train_set, None, batch_size=4, max_epochs=1, optimizer="adamw", lr=1e-3, weight_decay=1e-2, warmup_iters=None, limit_train_batches=3,
               seed=42, **kw)
    torch.cuda.synchronize()
    return hist


def test_fit_on_q16_is_fit_on_the_decoded_frames(tmp_path):
    """The training step is bit-reproducible and the q16 gather has the bits of the fp32 gather of the decoded frames: the same loss history."""
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.utils import AugmentSpec
    ds, q, dec = _stores("samples")
    frames = dec.frames.cpu().numpy()
    order = sorted(FIELDS)
    decoded = BubbleForecast.from_arrays([{n: frames[order.index(n), int(q.frame0[fi]):int(q.frame0[fi + 1])] for n in FIELDS} for fi in range(2)],
                                         norm="std", time_window=2, start_time=5)
    decoded.normalize(ds.diff_terms, ds.div_terms)
    ck = str(tmp_path / "q16.ckpt")
    a = _fit(ds, train_storage="q16", checkpoint_path=ck, hyper_parameters={"model_cfg": {"name": "avit"}})
    b = _fit(decoded)
    assert a["train_loss"] == b["train_loss"] and len(a["train_loss"]) == 3 and np.isfinite(a["train_loss"]).all()
    assert a["train_storage"] == "q16" and b["train_storage"] == "fp32"
    hp = torch.load(ck, map_location="cpu", weights_only=False)["hyper_parameters"]
    assert hp["train_storage"] == "q16" and hp["model_cfg"] == {"name": "avit"} and "normalization_constants" in hp
    assert a["train_loss"] != _fit(ds)["train_loss"]                                # the originals are other values
    spec = AugmentSpec(flip_p=0.5, crop=(48, 32), seed=3)
    assert _fit(ds, train_storage="q16", augment=spec, unroll_steps=2)["train_loss"] == _fit(decoded, augment=spec, unroll_steps=2)["train_loss"]


def test_fit_with_the_default_storage_is_the_call_without_the_keyword():
    ds = _dataset("samples")
    absent = _fit(ds)
    assert _fit(ds, train_storage="fp32") == absent and absent["train_storage"] == "fp32"
    with pytest.raises(ValueError, match="'fp32' or 'q16'"):
        _fit(ds, train_storage="fp16")


def test_rollout_evaluation_refuses_a_q16_store_and_runs_on_to_fp32():
    from bubbleformer_amd.utils.rollout import evaluate_rollouts, evaluate_rollouts_redistanced, render_rollouts
    ds, q, dec = _stores("samples")
    model = _model().eval()
    for call in (lambda: evaluate_rollouts(model, q, [3], 2), lambda: evaluate_rollouts_redistanced(model, q, [3], 2, None)):
        with pytest.raises(ValueError, match=r"'q16'.*to_fp32\(\)"):
            call()
    rep = evaluate_rollouts(model, q.to_fp32(), [3], 2, keep_predictions=True)
    assert rep.rel_l2.shape[:2] == (1, 4) and torch.isfinite(rep.rel_l2).all()
    with pytest.raises(ValueError, match=r"'q16'.*to_fp32\(\)"):
        render_rollouts(rep, q, [3], "unused")
