"""GPU: the seeded mirror and window of the device clip gather (bf_clip_gather_augment) -- bit for bit against the plain gather put through
the host plan (utils.augment.augment_plan, itself held to tests/augment_restatement.py on the CPU), its purity, the unrolled layout, and
fit() with ``augment``.

Every comparison is torch.equal: the kernel forms clip_norm on the stored value (negated for an odd field of a mirrored sample), which is
the expression the plain gather forms on a dataset whose odd fields were negated on the host."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FIELDS = ["dfun", "temperature", "velx", "vely"]
SIZES = [(8, 8, 1), (6, 10, 1), (9, 14, 2)]            # the 16-byte row path; W no multiple of 4; a 4 x 7 output grid through the nearest-neighbour map
WINDOWS = [(4, 5), (3, 3)]
FLUID = {"inv_reynolds": 0.0042, "cpgas": 0.83, "mugas": 0.023, "rhogas": 0.0083, "thcogas": 0.25, "stefan": 0.5, "prandtl": 8.4,
         "heater": {"nucWaitTime": 0.4, "wallTemp": 1.0}}


def _arrays(H, W, negate_velx):
    g = np.random.default_rng(100 * H + W)
    trajs = []
    for _ in range(2):
        t = {n: (g.standard_normal((12, H, W)) * (0.5 + k) + (1.5 - k) * 0.8 + 0.3).astype(np.float32) for k, n in enumerate(FIELDS)}      # non-zero means
        if negate_velx:
            t["velx"] = -t["velx"]
        trajs.append(t)
    return trajs


@functools.lru_cache(maxsize=None)
def _stores(H, W, f, in_fields=None, out_fields=None, fluid=False):
    """(dataset, its device store, the store of the same data with velx negated on the host, normalised with the FIRST dataset's constants)."""
    from bubbleformer_amd.data import BubbleForecast
    kw = dict(norm="std", time_window=2, start_time=0, downsample_factor=f, input_fields=list(in_fields or FIELDS), output_fields=list(out_fields or FIELDS))
    fl = [dict(FLUID, stefan=0.5 + i) for i in range(2)] if fluid else None
    ds = BubbleForecast.from_arrays(_arrays(H, W, False), fl, **kw)
    diff, div = ds.normalize()
    assert all(abs(diff[n]) > 0.05 for n in ds.fields)
    neg = BubbleForecast.from_arrays(_arrays(H, W, True), fl, **kw)
    neg.normalize(diff, div)
    return ds, ds.device_store("cuda"), neg.device_store("cuda")


def _grid(H, W, f):
    return (H // f, W // f) if f > 1 else (H, W)


def _spec(**kw):
    from bubbleformer_amd.utils import AugmentSpec
    return AugmentSpec(**kw)


def _plan(spec, ids, draw, grid):
    from bubbleformer_amd.utils import augment_plan
    flip, x0, y0 = augment_plan(spec, ids, draw, *grid)
    return flip.tolist(), x0.tolist(), y0.tolist()


def _expected(plain, negated, plan, window, batch_dim=0):
    """The plain gather put through the host plan: per sample the window of `plain` (of `negated` when mirrored), mirrored in x."""
    flip, x0, y0 = plan
    hc, wc = window
    rows = []
    for b in range(len(flip)):
        src = (negated if flip[b] else plain).select(batch_dim, b)[..., y0[b]:y0[b] + hc, x0[b]:x0[b] + wc]
        rows.append(torch.flip(src, dims=[-1]) if flip[b] else src)
    return torch.stack(rows, dim=batch_dim)


def _pick_draw(spec, ids, grid, ok):
    """The first draw whose plan satisfies `ok` -- picked from the plan, not hoped for."""
    return next(d for d in range(256) if ok(*_plan(spec, ids, d, grid)))


# ------------------------------------------------------------------------------------------------ 1. off is plain
@pytest.mark.parametrize("H,W,f", SIZES)
def test_off_is_the_plain_gather(H, W, f, monkeypatch):
    from bubbleformer_amd import ops
    ds, store, _ = _stores(H, W, f)
    ids = [0, 5, 17, 9]
    plain, plain2 = store.gather(ids), store.gather([0, 5, 11], unroll=2)
    monkeypatch.setattr(ops, "clip_gather_augment", lambda *a, **k: (_ for _ in ()).throw(AssertionError("an inactive spec launched the augmenting gather")))
    for spec in (_spec(), _spec(flip_p=0.0), _spec(flip_p=0, seed=9, crop_y="random"), _spec(flip_p=0.5).eval_view()):
        got = store.gather(ids, augment=spec, draw=3)
        assert all(torch.equal(a, b) for a, b in zip(got, plain))
        got2 = store.gather([0, 5, 11], unroll=2, augment=spec, draw=3)
        assert all(torch.equal(a, b) for a, b in zip(got2, plain2))
    with pytest.raises(AssertionError, match="inactive"):
        store.gather(ids, augment=_spec(flip_p=0.5))


@pytest.mark.parametrize("H,W,f", SIZES)
def test_a_window_of_the_whole_grid_without_a_mirror_is_the_plain_gather(H, W, f):
    """The new kernel itself on the identity: crop = the whole output grid, flip_p = 0."""
    ds, store, _ = _stores(H, W, f)
    ids = list(range(len(ds)))
    got = store.gather(ids, augment=_spec(crop=_grid(H, W, f), crop_y="random", seed=5), draw=2)
    assert all(torch.equal(a, b) for a, b in zip(got, store.gather(ids)))


# ------------------------------------------------------------------------------------------------ 2. mirror
@pytest.mark.parametrize("H,W,f", SIZES)
def test_mirror_is_the_flipped_gather_of_the_negated_velx(H, W, f):
    ds, store, neg = _stores(H, W, f)
    ids = [0, 5, 17, 9, 12]
    got = store.gather(ids, augment=_spec(flip_p=1.0, seed=3), draw=4)
    want = neg.gather(ids)
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.equal(a, torch.flip(b, dims=[-1]))
    vx = FIELDS.index("velx")
    assert not torch.equal(got[0][:, :, vx], torch.flip(store.gather(ids)[0], dims=[-1])[:, :, vx])          # the sign is there ...
    same = store.gather(ids, augment=_spec(flip_p=1.0, odd_fields=(), seed=3), draw=4)                       # ... and odd_fields = () leaves it alone
    for a, b in zip(same, store.gather(ids)):
        assert torch.equal(a, torch.flip(b, dims=[-1]))
    unknown = store.gather(ids, augment=_spec(flip_p=1.0, odd_fields=("velx", "no_such_field"), seed=3), draw=4)
    assert all(torch.equal(a, b) for a, b in zip(unknown, got))


@pytest.mark.parametrize("H,W,f", SIZES)
def test_mirror_with_velx_among_the_outputs_only(H, W, f):
    fields = (("dfun", "temperature"), ("velx", "dfun", "vely"))
    ds, store, neg = _stores(H, W, f, *fields)
    ids = [3, 16, 8]
    got = store.gather(ids, augment=_spec(flip_p=1.0), draw=1)
    want = neg.gather(ids)
    assert got[0].shape[2] == 2 and got[1].shape[2] == 3
    for a, b in zip(got, want):
        assert torch.equal(a, torch.flip(b, dims=[-1]))
    assert torch.equal(got[0], torch.flip(store.gather(ids)[0], dims=[-1]))            # no odd field among the inputs


# ------------------------------------------------------------------------------------------------ 3. window
@pytest.mark.parametrize("crop_y", ["bottom", "random"])
@pytest.mark.parametrize("window", WINDOWS + [(4, 4)])
@pytest.mark.parametrize("H,W,f", SIZES)
def test_window_is_the_slice_of_the_plain_gather_at_the_planned_origin(H, W, f, window, crop_y):
    """(4, 4) at W = 8 has origins that are multiples of 4 (16-byte reads) beside ones that are not; the draw is chosen from the plan so that
    the batch holds an odd x0 (and, where the grid leaves room, a y0 > 0 under crop_y = "random")."""
    ds, store, neg = _stores(H, W, f)
    grid = _grid(H, W, f)
    ids = list(range(len(ds)))
    spec = _spec(crop=window, crop_y=crop_y, seed=3)
    room_y = crop_y == "random" and grid[0] > window[0]
    draw = _pick_draw(spec, ids, grid, lambda flip, x0, y0: any(v % 2 for v in x0) and any(v % 4 == 0 for v in x0) and (not room_y or max(y0) > 0))
    plan = _plan(spec, ids, draw, grid)
    assert not any(plan[0]) and (crop_y == "random" or not any(plan[2]))
    got, plain = store.gather(ids, augment=spec, draw=draw), store.gather(ids)
    for a, b in zip(got, plain):
        assert a.shape == b.shape[:3] + window and a.is_contiguous()
        assert torch.equal(a, _expected(b, b, plan, window))


# ------------------------------------------------------------------------------------------------ 4. both
@pytest.mark.parametrize("crop_y", ["bottom", "random"])
@pytest.mark.parametrize("window", WINDOWS + [(4, 4)])
@pytest.mark.parametrize("H,W,f", SIZES)
def test_mirror_and_window_together_follow_the_plan_per_sample(H, W, f, window, crop_y):
    ds, store, neg = _stores(H, W, f)
    grid = _grid(H, W, f)
    spec = _spec(flip_p=0.5, crop=window, crop_y=crop_y, seed=3)
    flip = _plan(spec, list(range(len(ds))), 6, grid)[0]
    ids = [i for i in range(len(ds)) if flip[i]][:3] + [i for i in range(len(ds)) if not flip[i]][:3]
    plan = _plan(spec, ids, 6, grid)
    assert any(plan[0]) and not all(plan[0])                                         # mirrored and unmirrored samples in one batch
    got = store.gather(ids, augment=spec, draw=6)
    for a, p, n in zip(got, store.gather(ids), neg.gather(ids)):
        assert torch.equal(a, _expected(p, n, plan, window))


# ------------------------------------------------------------------------------------------------ 5. pure function
@pytest.mark.parametrize("H,W,f", SIZES)
def test_a_samples_clip_depends_on_seed_sample_and_draw_alone(H, W, f):
    ds, store, _ = _stores(H, W, f)
    grid = _grid(H, W, f)
    spec = _spec(flip_p=0.5, crop=(3, 3), crop_y="random", seed=11)
    s, draw = 7, 2
    alone = store.gather([s], augment=spec, draw=draw)
    five = store.gather([1, 4, s, 16, 2], augment=spec, draw=draw)
    moved = store.gather([s, 1, 4, 16, s], augment=spec, draw=draw)
    on_device = store.gather(torch.tensor([2, s], device="cuda"), augment=spec, draw=draw)
    for k in range(2):
        assert torch.equal(five[k][2], alone[k][0]) and torch.equal(moved[k][0], alone[k][0]) and torch.equal(moved[k][4], alone[k][0])
        assert torch.equal(on_device[k][1], alone[k][0]) and torch.equal(on_device[k][0], five[k][4])
    assert all(torch.equal(a, b) for a, b in zip(store.gather([1, 4, s, 16, 2], augment=spec, draw=draw), five))      # two calls: the same bits
    ids = list(range(len(ds)))
    base = store.gather(ids, augment=spec, draw=draw)
    other_draw = _pick_draw(spec, ids, grid, lambda *p: p != _plan(spec, ids, draw, grid))
    assert other_draw != draw and not torch.equal(store.gather(ids, augment=spec, draw=other_draw)[0], base[0])
    other_seed = next(sd for sd in range(12, 64) if _plan(_spec(flip_p=0.5, crop=(3, 3), crop_y="random", seed=sd), ids, draw, grid) != _plan(spec, ids, draw, grid))
    assert not torch.equal(store.gather(ids, augment=_spec(flip_p=0.5, crop=(3, 3), crop_y="random", seed=other_seed), draw=draw)[0], base[0])
    assert all(torch.equal(a, b) for a, b in zip(store.gather(ids, augment=spec, draw=draw + 2 ** 32), base))           # draws count modulo 2^32
    # device indices out of range are clamped as in the plain gather: the clamped index is the sample, and its id
    n = len(ds)
    clamped = store.gather(torch.tensor([-3, 10 ** 6, 5], device="cuda"), augment=spec, draw=draw)
    assert all(torch.equal(a, b) for a, b in zip(clamped, store.gather([0, n - 1, 5], augment=spec, draw=draw)))
    with pytest.raises(IndexError):
        store.gather([0, n], augment=spec)
    with pytest.raises(ValueError, match="larger"):
        store.gather([0], augment=_spec(crop=(grid[0] + 1, 3)))


# ------------------------------------------------------------------------------------------------ 6. unroll
@pytest.mark.parametrize("mode", ["mirror", "window", "both"])
@pytest.mark.parametrize("H,W,f", SIZES)
def test_unrolled_clips_share_the_samples_decision(H, W, f, mode):
    """unroll = 2 on a conditioned dataset: the input clip and both target clips of a sample under its one decision, (k, B, T, C, Hc, Wc),
    and the fluid rows of the plain gather."""
    ds, store, neg = _stores(H, W, f, fluid=True)
    grid = _grid(H, W, f)
    window = grid if mode == "mirror" else (3, 3)
    spec = _spec(flip_p={"mirror": 1.0, "window": 0.0, "both": 0.5}[mode], crop=None if mode == "mirror" else window, crop_y="random", seed=3)
    pool = ds.unrollable(2)
    flip = _plan(spec, pool, 1, grid)[0]
    ids = ([i for i, fl in zip(pool, flip) if fl][:2] + [i for i, fl in zip(pool, flip) if not fl][:2]) if mode == "both" else [pool[0], pool[-1], pool[5]]
    plan = _plan(spec, ids, 1, grid)
    assert mode != "both" or (any(plan[0]) and not all(plan[0]))
    inp, tgt, fl = store.gather(ids, unroll=2, augment=spec, draw=1)
    p_inp, p_tgt, p_fl = store.gather(ids, unroll=2)
    n_inp, n_tgt, _ = neg.gather(ids, unroll=2)
    assert inp.shape == (len(ids), 2, 4) + window and tgt.shape == (2, len(ids), 2, 4) + window and tgt[1].is_contiguous()
    assert torch.equal(inp, _expected(p_inp, n_inp, plan, window))
    assert torch.equal(tgt, _expected(p_tgt, n_tgt, plan, window, batch_dim=1))
    assert torch.equal(fl, p_fl) and fl.shape == (len(ids), 9) and (mode == "both" or not torch.equal(fl[0], fl[1]))      # rows of both files
    one = store.gather(ids, augment=spec, draw=1)                                  # without unroll: the same input clip and first target clip
    assert torch.equal(one[0], inp) and torch.equal(one[1], tgt[0]) and torch.equal(one[2], fl)
    with pytest.raises(IndexError):
        store.gather([len(ds) - 1], unroll=2, augment=spec)


# ------------------------------------------------------------------------------------------------ 7. the loop
SAMPLES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samples")
_DEFAULT = object()


def _sets():
    from bubbleformer_amd.data import BubbleForecast
    files = [os.path.join(SAMPLES, f"sample_{i}.hdf5") for i in (1, 2)]
    tr = BubbleForecast(files, norm="std", time_window=2, start_time=5)
    diff, div = tr.normalize()
    va = BubbleForecast(files[:1], norm="std", time_window=2, start_time=30)
    va.normalize(diff, div)
    return tr, va


def _fit(max_epochs=2, augment=_DEFAULT, seed=3, resume_from=None, checkpoint=None, val=False, **kw):
    """tests/test_gpu_noise.py's loop -- the tiny avit (patch 8), three batches of four clips of the two 64 x 64 sample files per epoch, a
    constant learning rate -- with ``augment``; _DEFAULT = AugmentSpec(flip_p=0.5, crop=(48, 32), seed=seed), "absent" = no keyword."""
    from bubbleformer_amd.fit import fit
    from bubbleformer_amd.models import get_model
    tr, va = _sets()
    torch.manual_seed(0)
    model = get_model("avit", input_fields=4, output_fields=4, time_window=2, patch_size=8, embed_dim=64, num_heads=2, processor_blocks=1,
                      drop_path=0.0, compute_dtype=torch.float32).cuda()
    if augment is _DEFAULT:
        augment = _spec(flip_p=0.5, crop=(48, 32), seed=seed)
    if augment != "absent":
        kw["augment"] = augment
    hist = fit(model, tr, va if val else None, batch_size=4, max_epochs=max_epochs, optimizer="adamw", lr=1e-3, weight_decay=1e-2, warmup_iters=None,
               limit_train_batches=3, limit_val_batches=2, seed=42, resume_from=resume_from, checkpoint_path=checkpoint, **kw)
    torch.cuda.synchronize()
    return hist


def test_fit_with_augment_repeats_resumes_and_depends_on_the_seed(tmp_path):
    a, b = _fit(), _fit()
    assert a == b and len(a["train_loss"]) == 6 and np.isfinite(a["train_loss"]).all()
    ck = str(tmp_path / "epoch0.ckpt")
    first = _fit(max_epochs=1, checkpoint=ck)
    second = _fit(resume_from=ck)
    resumed = torch.tensor(first["train_loss"] + second["train_loss"])
    assert torch.equal(resumed, torch.tensor(a["train_loss"])), (resumed, a["train_loss"])
    assert _fit(seed=4)["train_loss"] != a["train_loss"]


def test_fit_without_augment_is_the_call_without_the_keyword():
    absent = _fit(augment="absent")
    assert _fit(augment=None) == absent and _fit(augment=_spec()) == absent
    assert _fit()["train_loss"] != absent["train_loss"]


def test_fit_with_augment_composes_with_unroll_noise_and_validation():
    from bubbleformer_amd.utils import NoiseSpec
    kw = dict(unroll_steps=2, input_noise=NoiseSpec(0.01, relative=True, seed=5))
    a, b = _fit(max_epochs=1, **kw), _fit(max_epochs=1, **kw)
    assert a == b and np.isfinite(a["train_loss"]).all() and np.isfinite(a["unroll_loss"]).all() and len(a["unroll_loss"]) == 3
    va, vb = _fit(max_epochs=1, val=True), _fit(max_epochs=1, val=True)
    assert va == vb and len(va["val_loss"]) == 1 and np.isfinite(va["val_loss"]).all()
    flip_only = _fit(max_epochs=1, val=True, augment=_spec(flip_p=0.5, seed=3))      # no crop: validation is gathered plainly, at 64 x 64
    assert np.isfinite(flip_only["val_loss"]).all() and flip_only["val_loss"] != va["val_loss"]
