"""GPU: the renderer (csrc/render.hip, utils/plot_utils.py) against the numpy restatement tests/render_restatement.py, byte for byte.

The only pixels set aside are those of a speed tile whose fp64 distance to an arrow stroke lies within 1e-6 px of the stroke's half-width;
each test asserts on the restatement that they are at most 0.1 % of a tile before it compares (the seeded fields give none)."""
import os

import numpy as np
import pytest
import torch

from tests import render_restatement as R
from tests.test_render import GOLDEN, SCALES, SHAPES, _luts

pytestmark = pytest.mark.gpu

FILES = [os.path.join(GOLDEN, "samples", f"sample_{i}.hdf5") for i in (1, 2)]
FIELDS = ["dfun", "temperature", "velx", "vely"]
_SAMPLES = {}


def _sample(i):
    """(50, 4, 64, 64) fp32 of one sample file, read once."""
    if i not in _SAMPLES:
        from bubbleformer_amd.data import hdf5_lite
        f = hdf5_lite.File(FILES[i])
        _SAMPLES[i] = np.ascontiguousarray(np.stack([np.asarray(f[k][...], dtype=np.float32) for k in FIELDS], axis=1))
        _SAMPLES[i].flags.writeable = False
    return _SAMPLES[i]


def _spec(s, stride=8):
    from bubbleformer_amd.utils.plot_utils import RenderSpec
    return RenderSpec(scale=s, stride=stride)


def _assert_images_equal(got, want, band, tile_pixels, what):
    """Every byte outside the arrow band; the band itself at most 0.1 % of a tile (asserted first, on the restatement alone)."""
    print(f"{what}: {int(band.sum())} band pixels of {tile_pixels} per tile")
    assert band.sum() <= 1e-3 * tile_pixels, what
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    bad = (got != want).any(axis=-1) & ~band
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())


def _fields(rng, frames, H, W, lo, hi):
    """Seeded fp32 fields over a little more than [lo, hi], with the range ends, values just beyond them, NaN and both infinities put in."""
    x = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), (frames, H, W)).astype(np.float32)
    special = np.float32([lo, hi, np.nextafter(np.float32(hi), np.float32(np.inf)), np.nextafter(np.float32(lo), np.float32(-np.inf)), np.nan, np.inf,
                          -np.inf, hi + 100.0, lo - 100.0])
    flat = x.reshape(-1)
    at = rng.permutation(flat.size)[:len(special)]
    flat[at] = special[:len(at)] if flat.size >= len(special) else special[rng.permutation(len(special))[:len(at)]]
    return x


@pytest.mark.parametrize("shape", SHAPES)
def test_tiles_exact_bytes(shape):
    """A signed-distance tile (Blues, outline) beside a temperature tile (turbo) for every scale, 1 - 3 frames per launch; one scale also
    with vmax == vmin.  Colour, outline, bar and gutter: every byte."""
    from bubbleformer_amd import _lib as L, ops
    H, W = shape
    luts = _luts()
    for k, s in enumerate(SCALES):
        frames = 1 + (k + H) % 3
        rng = np.random.default_rng(1000 * H + 10 * W + s)
        sdf = _fields(rng, frames, H, W, -0.5, 0.75)
        temp = _fields(rng, frames, H, W, 0.1, 0.9)
        ranges = [(-0.5, 0.75), (0.1, 0.9) if s != 3 else (0.4, 0.4)]
        lay = _spec(s).layout(H, W, 1, 2)
        dev = [torch.from_numpy(a).cuda().unsqueeze(1) for a in (sdf, temp)]
        rng_dev = torch.tensor(ranges, dtype=torch.float64).cuda()
        got = ops.render_tiles([{"kind": L.BF_RENDER_SDF, "a": dev[0], "range": rng_dev[0]}, {"kind": L.BF_RENDER_TEMP, "a": dev[1], "range": rng_dev[1]}],
                               lay, frames)
        rl = R.layout(H, W, s, 1, 2)
        for f in range(frames):
            want, band = R.compose([(R.SDF, sdf[f], None, None, *ranges[0]), (R.TEMP, temp[f], None, None, *ranges[1])], rl, luts)
            _assert_images_equal(got[f], want, band, H * W * s * s, f"{shape} s={s} frame {f}")


ARROW_CASES = [((5, 8), 3, 2, "mixed"), ((5, 8), 5, 1, "mixed"), ((7, 22), 5, 3, "mixed"), ((16, 16), 2, 8, "mixed"), ((31, 64), 1, 8, "mixed"),
               ((64, 64), 2, 8, "mixed"), ((16, 16), 2, 8, "vapour"), ((5, 8), 3, 40, "mixed"), ((16, 16), 3, 20, "mixed"), ((1, 1), 5, 1, "mixed")]


@pytest.mark.parametrize("shape,s,stride,mask_kind", ARROW_CASES)
def test_arrows(shape, s, stride, mask_kind):
    """Speed tiles with arrows, two frames: velocities from well below to above vmax, some anchors exactly zero, NaN and infinite; a mask
    that hides some anchors ("vapour": all of them, so no arrow is left); a stride whose anchors all lie outside the field (40) and one
    larger than the field with its anchor inside (20)."""
    from bubbleformer_amd import _lib as L, ops
    H, W = shape
    rng = np.random.default_rng(7 * H + W + 100 * s + stride)
    u = rng.normal(0, 0.6, (2, H, W)).astype(np.float32)
    v = rng.normal(0, 0.6, (2, H, W)).astype(np.float32)
    flat_u, flat_v = u.reshape(-1), v.reshape(-1)
    for k, (a, b) in enumerate([(0.0, 0.0), (np.nan, 0.3), (np.inf, 0.1), (2.5, -3.7)]):
        at = rng.integers(0, flat_u.size)
        flat_u[at], flat_v[at] = a, b
    mask = np.ones((2, H, W), dtype=np.float32) if mask_kind == "vapour" else rng.normal(0, 1, (2, H, W)).astype(np.float32)
    vrange = (0.0, 1.0)
    lay = _spec(s, stride).layout(H, W, 1, 1)
    dev = [torch.from_numpy(a).cuda().unsqueeze(1) for a in (u, v, mask)]
    got = ops.render_tiles([{"kind": L.BF_RENDER_SPEED, "a": dev[0], "b": dev[1], "mask": dev[2], "range": torch.tensor(vrange, dtype=torch.float64).cuda()}], lay, 2)
    rl = R.layout(H, W, s, 1, 1, stride)
    whites = 0
    for f in range(2):
        want, band = R.compose([(R.SPEED, u[f], v[f], mask[f], *vrange)], rl, _luts())
        d = R.arrow_distance(u[f], v[f], mask[f], s, stride, vrange[1])
        whites += int((d <= rl["stroke"]).sum())
        _assert_images_equal(got[f], want, band, H * W * s * s, f"{shape} s={s} stride={stride} frame {f}")
    print("arrow pixels:", whites)
    if mask_kind == "vapour" or stride == 40:
        assert whites == 0
    elif H >= 5:
        assert whites > 0


def _range_bounds(x):
    """See test_ranges' docstring -> (relative bound of the mean's error against |mean| + sigma, relative bound of the std's error)."""
    n = x.size
    u = 2.0 ** -53
    gamma = n * u
    A, Q, S1 = np.abs(x).sum(), (x * x).sum(), x.sum()
    mean = S1 / n
    M = Q - S1 * S1 / n
    d_mean = gamma * A / n + u * abs(mean)
    d_M = gamma * Q + 2 * abs(S1) * gamma * A / n + 4 * u * Q
    return d_mean, 0.5 * d_M / M + 2 * u if M > 0 else np.inf


@pytest.mark.parametrize("case", ["sample_0", "sample_1", "one_cell", "nan", "skipped"])
def test_ranges(case):
    """bf_render_ranges against numpy fp64.  n, min and max are exact.  With u = 2^-53 and gamma = n u, a sum of n fp64 terms in any fixed order
    is within gamma * sum |term| of the exact one, so |S1' - S1| <= gamma A (A = sum |x|) and |S2' - S2| <= gamma Q (Q = sum x^2); numpy's own
    pairwise sums are far inside the same bounds, which therefore also hold between the two.  What plot_bubbleml derives from them:
      mean' = S1' / n:                     |mean' - mean| <= gamma A / n + u |mean|
      M' = S2' - S1'^2 / n = (n - 1) var:  |M' - M| <= gamma Q + 2 |S1| gamma A / n + 4 u Q   (the square, the quotient, the difference and
                                           the second-order term, each at most u Q since S1^2 / n <= Q)
      std' = sqrt(M' / (n - 1)):           |std' - std| / std <= |M' - M| / (2 M) + 2 u
    For the cases here |mean| <= 10 sigma, which keeps Q / M <= 101 n / (n - 1); the test checks on numpy's values that the std's bound is
    below 1e-9 relative, then holds the device's mean and std to the bounds."""
    from bubbleformer_amd import ops
    from bubbleformer_amd.utils.plot_utils import reference_ranges
    channels = (0, 1, 2, 3)
    if case.startswith("sample"):
        x = _sample(int(case[-1])).copy()
    elif case == "one_cell":
        x = np.float32([[[[-0.25]], [[1.5]], [[3.0]], [[-4.0]]]])
    elif case == "nan":
        x = np.random.default_rng(5).normal(1.0, 2.0, (3, 4, 7, 22)).astype(np.float32)
        x[1, 0, 2, 3] = x[2, 2, 0, 0] = np.nan
    else:
        x = np.random.default_rng(6).normal(1.0, 2.0, (2, 3, 5, 8)).astype(np.float32)        # odd plane size: the scalar path; no y velocity
        channels = (2, -1, 1, -1)
    got = ops.render_ranges(torch.from_numpy(x).cuda(), channels).cpu().numpy()
    want = R.ranges(x, channels)
    assert got.shape == (3, 5)
    assert np.array_equal(got[:, 0], want[:, 0]) and np.array_equal(got[:, 3:], want[:, 3:]), (got, want)           # n, min, max: exact
    if case == "skipped":
        assert got[1].tolist() == [0, 0, 0, np.inf, -np.inf] and got[2].tolist() == [0, 0, 0, np.inf, -np.inf] and got[0, 0] == 80
    if case == "nan":
        assert np.isnan(got[0, 1:3]).all() and np.isnan(got[2, 1:3]).all() and np.isfinite(got[:, 3:]).all() and np.isfinite(got[1]).all()
    series = (x[:, channels[0]].astype(np.float64), x[:, channels[1]].astype(np.float64) if channels[1] >= 0 else None,
              R.speed(x[:, channels[2]], x[:, channels[3]]) if channels[3] >= 0 else None)
    for q, xs in enumerate(series):
        if xs is None or np.isnan(xs).any():
            continue
        n = xs.size
        gamma = n * 2.0 ** -53
        assert abs(got[q, 1] - want[q, 1]) <= gamma * np.abs(xs).sum() and abs(got[q, 2] - want[q, 2]) <= gamma * (xs * xs).sum(), (case, q)
        if n < 2:
            assert reference_ranges(got)[q] is not None and all(np.isnan(v) for v in reference_ranges(got)[q])      # no std of one value
            continue
        mean, std = xs.mean(), xs.std(ddof=1)
        d_mean, rel_std = _range_bounds(xs)
        print(f"{case} quantity {q}: |mean| / sigma = {abs(mean) / std:.3f}, bounds {d_mean:.2e} (mean), {rel_std:.2e} relative (std)")
        assert abs(mean) <= 10 * std and rel_std < 1e-9
        got_mean = got[q, 1] / n
        got_std = np.sqrt((got[q, 2] - got[q, 1] ** 2 / n) / (n - 1))
        assert abs(got_mean - mean) <= 2 * d_mean and abs(got_std - std) <= 2 * rel_std * std, (case, q)      # twice: numpy's own values carry the same bound
        assert reference_ranges(got)[q] == (round(float(got_mean - 3 * got_std), 2), round(float(got_mean + 3 * got_std), 2))


def _clips(kind):
    """(pred, target) (F, 4, H, W), scale, stride, ranges."""
    if kind == "sample":
        x = _sample(0)
        target = x[20:23].copy()
        pred = (x[21:24] * np.float32(0.97)).astype(np.float32)
        return pred, target, 1, 8, [(-0.3, 0.25), (0.0, 0.9), (0.0, 0.6)]
    H, W, s, stride = (5, 8, 3, 2) if kind == "5x8" else (16, 16, 2, 8)
    rng = np.random.default_rng(H)
    target, pred = (rng.normal(0.2, 0.7, (2, 4, H, W)).astype(np.float32) for _ in range(2))
    pred[0, 1, 0, 0], pred[1, 2, 1, 1] = np.nan, np.inf
    return pred, target, s, stride, [(-1.0, 1.5), (-0.8, 1.2), (0.0, 1.1)]


@pytest.mark.parametrize("kind", ["5x8", "16x16", "sample"])
def test_panels(kind):
    """Whole 2 x 3 images: the simulation on top, the prediction below, both rows' arrows hidden by the SIMULATION's vapour.  Two runs give
    the same bytes; a second channel order and a missing field give the matching columns."""
    from bubbleformer_amd.utils.plot_utils import render_panels
    pred, target, s, stride, ranges = _clips(kind)
    spec = _spec(s, stride)
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(target).cuda()
    got = render_panels(p, t, ranges, spec)
    again = render_panels(p, t, torch.tensor(ranges, dtype=torch.float64), spec)
    assert torch.equal(got, again)
    F, _, H, W = pred.shape
    rl = R.layout(H, W, s, 2, 3, stride)
    assert got.shape == (F, rl["img_h"], rl["img_w"], 3) and got.dtype == torch.uint8
    for f in range(F):
        want, band = R.panel(pred[f], target[f], ranges, rl, _luts())
        _assert_images_equal(got[f], want, band, H * W * s * s, f"{kind} frame {f}")
    if kind == "16x16":
        perm = [3, 0, 2, 1]                                    # channels elsewhere, and no temperature: two columns
        got2 = render_panels(p[:, perm], t[:, perm], ranges, spec, channels=(1, None, 2, 0))
        rl2 = R.layout(H, W, s, 2, 2, stride)
        for f in range(F):
            want, band = R.panel(pred[f][perm], target[f][perm], ranges, rl2, _luts(), channels=(1, -1, 2, 0))
            _assert_images_equal(got2[f], want, band, H * W * s * s, f"{kind} permuted frame {f}")


@pytest.mark.parametrize("T", [1, 4])
def test_strips(T):
    """The three wandb_*_plotter strips of T sample frames, scaled to their own minimum and maximum on the device, and once with a given range."""
    from bubbleformer_amd.utils.plot_utils import sdf_strip, temp_strip, vel_strip
    x = _sample(1)[30:30 + T]
    dev = torch.from_numpy(x.copy()).cuda()
    spec = _spec(1)
    rl = R.layout(64, 64, 1, 1, T)
    for name, fn, frames, dframes, kind in (("sdf", sdf_strip, x[:, 0], dev[:, 0], R.SDF), ("temp", temp_strip, x[:, 1], dev[:, 1], R.TEMP),
                                            ("vel", vel_strip, x[:, 2:4], dev[:, 2:4], R.SPEED)):
        got = fn(dframes, spec=spec)
        assert torch.equal(got, fn(dframes, spec=spec))
        want, band = R.strip(frames, kind, None, rl, _luts())
        _assert_images_equal(got, want, band, 64 * 64, f"{name} strip T={T}")
        want, band = R.strip(frames, kind, (0.05, 0.4), rl, _luts())
        _assert_images_equal(fn(dframes, (0.05, 0.4), spec), want, band, 64 * 64, f"{name} strip T={T} with a range")
    with pytest.raises(ValueError):
        vel_strip(dev[:, 0])


def _stamped(images, layout, cols, first, ranges):
    from bubbleformer_amd.utils.plot_utils import panel_titles, stamp_labels
    out = images.cpu().numpy().copy()
    for k in range(out.shape[0]):
        stamp_labels(out[k], layout, panel_titles(cols, first + k), [ranges[q] for _ in range(2) for q in cols])
    return out


def test_plot_bubbleml_end_to_end(tmp_path):
    from bubbleformer_amd.utils.plot_utils import RenderSpec, plot_bubbleml, reference_ranges, render_panels
    from bubbleformer_amd.utils.png import read_png
    from bubbleformer_amd.utils.rollout import relative_l2_per_frame
    x = _sample(0)
    target = torch.from_numpy(x[10:14].copy()).cuda()
    pred = torch.from_numpy((x[11:15] * np.float32(1.02)).astype(np.float32)).cuda()
    steps = torch.arange(15, 19)
    res = plot_bubbleml(pred, target, steps, tmp_path, apng=True, chunk=3)
    want_ranges = reference_ranges(R.ranges(x[10:14], (0, 1, 2, 3)))
    assert res["ranges"] == want_ranges and all(np.isfinite(v) for r in want_ranges for v in r)
    assert sorted(os.listdir(tmp_path / "plots")) == ["0000.png", "0001.png", "0002.png", "0003.png", "rollout.png"]
    spec = RenderSpec()
    layout = spec.layout(64, 64, 2, 3)
    want = _stamped(render_panels(pred, target, want_ranges, spec), layout, [0, 1, 2], 0, want_ranges)
    plain = render_panels(pred, target, want_ranges, spec).cpu().numpy()
    assert (want != plain).any(axis=-1).sum() > 6 * 50                     # the glyphs are there
    for k in range(4):
        assert np.array_equal(read_png(tmp_path / "plots" / f"{k:04d}.png"), want[k]), k
    frames = read_png(tmp_path / "plots" / "rollout.png", all_frames=True)
    assert len(frames) == 4 and all(np.array_equal(a, b) for a, b in zip(frames, want))
    rows = (tmp_path / "relative_l2_error.csv").read_text().strip().split("\n")
    assert rows[0].split(",")[0] == "timestep" and len(rows) == 5
    table = np.array([[float(v) for v in r.split(",")] for r in rows[1:]])
    assert table[:, 0].tolist() == [15, 16, 17, 18]
    assert np.array_equal(table[:, 1:].astype(np.float32), relative_l2_per_frame(pred, target).cpu().numpy())
    given = plot_bubbleml(pred, target, steps, tmp_path / "given", vmin=(-1, 0, 0), vmax=(1, 1, 2))
    assert given["ranges"] == [(-1.0, 1.0), (0.0, 1.0), (0.0, 2.0)] and len(given["files"]) == 4
    bad = target.clone()
    bad[0, 1, 0, 0] = float("nan")
    with pytest.raises(ValueError, match="temperature"):
        plot_bubbleml(pred, bad, steps, tmp_path / "bad")


def _tiny_model():
    from bubbleformer_amd.models import get_model
    from oracle import weights as Wt
    cfg = dict(input_fields=4, output_fields=4, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=2)
    model = get_model("avit", time_window=4, drop_path=0.0, **cfg)
    model.load_state_dict(Wt.generate(Wt.param_shapes(**cfg), seed=3))
    return model.cuda()


def test_render_rollouts(tmp_path):
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.utils.plot_utils import RenderSpec, render_panels
    from bubbleformer_amd.utils.png import read_png
    from bubbleformer_amd.utils.rollout import evaluate_rollouts, render_rollouts
    model = _tiny_model().eval()
    ds = BubbleForecast(FILES, norm="std", downsample_factor=2, time_window=4, start_time=5)
    ds.normalize()
    store = ds.device_store("cuda")
    starts, steps = [7, 38 + 3], 2
    report = evaluate_rollouts(model, store, starts, steps, keep_predictions=True)
    out = render_rollouts(report, store, starts, tmp_path)
    assert sorted(out) == [0, 1]
    for b in range(2):
        assert sorted(os.listdir(tmp_path / f"traj_{b}" / "plots")) == [f"{k:04d}.png" for k in range(8)]
        assert (tmp_path / f"traj_{b}" / "relative_l2_error.csv").exists()
    b, k = 1, 5                                                   # frame 1 of step 1 of trajectory 1
    target = store.gather([starts[b] + 4])[1][0]
    spec = RenderSpec()
    ranges = out[b]["ranges"]
    want = _stamped(render_panels(report.predictions[b, k:k + 1], target[1:2], ranges, spec), spec.layout(32, 32, 2, 3), [0, 1, 2], k, ranges)[0]
    assert np.array_equal(read_png(tmp_path / "traj_1" / "plots" / "0005.png"), want)
    only = render_rollouts(report, store, starts, tmp_path / "one", trajectories=[1])
    assert sorted(only) == [1] and os.listdir(tmp_path / "one") == ["traj_1"]
    with pytest.raises(ValueError, match="keep_predictions"):
        render_rollouts(evaluate_rollouts(model, store, starts, steps), store, starts, tmp_path / "none")
    with pytest.raises(ValueError, match="trajectories"):
        render_rollouts(report, store, [7, 38 + 4], tmp_path / "other")


def test_fit_writes_the_validation_strips(tmp_path):
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.fit import fit
    from bubbleformer_amd.utils.png import read_png
    tr = BubbleForecast(FILES[:1], norm="std", downsample_factor=2, time_window=4, start_time=5)
    tr.normalize()
    va = BubbleForecast(FILES[1:], norm="std", downsample_factor=2, time_window=4, start_time=5)
    va.normalize(tr.diff_terms, tr.div_terms)
    kw = dict(batch_size=2, max_epochs=1, optimizer="adamw", lr=1e-3, weight_decay=1e-2, warmup_iters=None, limit_train_batches=1, limit_val_batches=1)
    before = set(os.listdir(tmp_path))
    fit(_tiny_model(), tr, va, **kw)
    assert set(os.listdir(tmp_path)) == before
    panels = tmp_path / "panels"
    fit(_tiny_model(), tr, va, panel_dir=str(panels), **kw)
    assert sorted(os.listdir(panels)) == sorted(f"epoch_0_{n}_{side}.png" for n in ("sdf", "temp", "vel") for side in ("target", "pred"))
    from bubbleformer_amd.utils.plot_utils import RenderSpec
    lay = RenderSpec().layout(32, 32, 1, 4)
    for name in os.listdir(panels):
        img = read_png(panels / name)
        assert img.shape == (lay.img_h, lay.img_w, 3) and len(np.unique(img.reshape(-1, 3), axis=0)) > 16
    nosdf = BubbleForecast(FILES[1:], input_fields=FIELDS[1:], output_fields=FIELDS[1:], norm="std", downsample_factor=2, time_window=4, start_time=5)
    from bubbleformer_amd.fit import write_validation_strips
    x = torch.from_numpy(_sample(1)[5:9, 1:, ::2, ::2].copy()).cuda()
    files = write_validation_strips(str(tmp_path / "nosdf"), 3, list(nosdf.output_fields), x, x)
    assert sorted(os.path.basename(f) for f in files) == ["epoch_3_temp_pred.png", "epoch_3_temp_target.png", "epoch_3_vel_pred.png", "epoch_3_vel_target.png"]
