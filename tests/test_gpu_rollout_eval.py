"""Batched on-device rollout evaluation on the GPU: the scoring kernel (`bf_rollout_score`) against fp64 restatements and against the
clips `DeviceClipStore.gather` returns, `evaluate_rollouts` against today's one-trajectory loop, against the reference's own rollouts
(tests/golden/rollout_eval.npz, tools/gen_rollout_eval_golden.py) and against itself at other batch sizes."""
import os

import numpy as np
import pytest
import torch

from tests.test_rollout_eval import FILES, GOLDEN, golden_dataset

pytestmark = pytest.mark.gpu
ALL = ["dfun", "temperature", "velx", "vely"]


def _score(store, pred, starts, s, steps, sdf=0, copies=True):
    """One eager `ops.rollout_score` call with the step counter preset to s; returns every output."""
    from bubbleformer_amd import ops
    from bubbleformer_amd.utils.rollout import plan_rollouts
    B, T, C, Ho, Wo = pred.shape
    dev = pred.device
    first = torch.tensor(plan_rollouts(store.ds, starts, steps).first, dtype=torch.int64, device=dev)
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    out = dict(rel_l2=new(B, steps * T, C), criterion=new(B, steps), eik_pred=new(B, steps * T), eik_tgt=new(B, steps * T),
               next_in=new(B, T, C, Ho, Wo) if copies else None, archive=new(B, steps * T, C, Ho, Wo) if copies else None)
    counter = torch.full((1,), s, dtype=torch.int32, device=dev)
    ops.rollout_score(pred, store.frames, first, counter, store.out_tab, sdf, steps, out["rel_l2"], out["criterion"], ops.rollout_score_workspace(pred),
                      out["eik_pred"], out["eik_tgt"], out["next_in"], out["archive"])
    out["counter"] = counter
    return out


def _rel_err(got, want):
    return float(((got.double() - want).abs() / want.abs()).max())


@pytest.mark.parametrize("norm", ["none", "std"])
@pytest.mark.parametrize("factor", [1, 2])
def test_scoring_kernel_against_fp64(norm, factor):
    """rel_l2 / criterion: relative error at most 2^-22 against torch fp64 on the gathered clips -- the kernel's inputs are the same fp32
    bits, its arithmetic is fp64 (summation-order error at most N * 2^-53 < 1e-10 for N <= 512^2) and one fp32 rounding follows.  Eikonal
    rows: rtol 2e-6 (test_physics_kernels_match_reference_values' figure for this score) against the fp64 restatement of the notebook's
    score on the torch-built physical field, and against physics.eikonal_l1_per_frame of the same fields."""
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.utils import physics
    from oracle import filmavit_ref as R
    T, steps, starts = 2, 8, [3, 20, 42 + 10]
    ds = BubbleForecast(FILES, norm=norm, downsample_factor=factor, time_window=T, start_time=5)
    ds.normalize()
    store = ds.device_store("cuda")
    raw = BubbleForecast(FILES, norm="none", downsample_factor=factor, time_window=T, start_time=5)
    raw.normalize()
    raw_store = raw.device_store("cuda")
    _, diff, div = store.out_tab
    hw = 64 // factor
    g = torch.Generator().manual_seed(100 * factor + len(norm))
    pred = torch.randn((3, T, 4, hw, hw), generator=g).cuda()
    for s in (0, 7):
        o = _score(store, pred, starts, s, steps)
        idx = [st + s * T for st in starts]
        tgt = store.gather(idx)[1].double()
        num = ((pred.double() - tgt) ** 2).sum(dim=(-1, -2))
        ratio = (num / (tgt ** 2).sum(dim=(-1, -2))).sqrt()                          # (B, T, C)
        rows = slice(s * T, (s + 1) * T)
        e1, e2 = _rel_err(o["rel_l2"][:, rows], ratio), _rel_err(o["criterion"][:, s], ratio.mean(dim=1).mean(dim=1))
        print(f"norm {norm} factor {factor} step {s}: rel_l2 {e1:.3e} criterion {e2:.3e} (bound {2.0 ** -22:.3e})")
        assert e1 <= 2.0 ** -22 and e2 <= 2.0 ** -22
        phi_p = pred[:, :, 0] * div[0] + diff[0]                                     # fp32 multiply, then add: the physical field
        phi_t = raw_store.gather(idx)[1][:, :, 0].contiguous()                       # the raw, downsampled frames
        for name, phi in (("eik_pred", phi_p), ("eik_tgt", phi_t)):
            got = o[name][:, rows].cpu().numpy().reshape(-1)
            want = R.eikonal_l1_per_frame(phi.reshape(-1, hw, hw).double().cpu()).numpy()
            old = physics.eikonal_l1_per_frame(phi.reshape(-1, hw, hw).contiguous()).cpu().numpy()
            print(f"  {name}: against fp64 {np.max(np.abs(got - want) / np.abs(want)):.3e}, against bf_eikonal_l1_frames {np.max(np.abs(got - old) / np.abs(old)):.3e}")
            assert np.allclose(got, want, rtol=2e-6, atol=0) and np.allclose(got, old, rtol=2e-6, atol=0)
        untouched = torch.ones(steps * T, dtype=torch.bool)
        untouched[rows] = False
        assert torch.isnan(o["rel_l2"][:, untouched.cuda()]).all()                   # only this step's rows are written
    none = _score(store, pred, starts, 0, steps, sdf=-1, copies=False)               # no signed-distance channel, no copies
    assert torch.isnan(none["eik_pred"]).all() and torch.equal(none["rel_l2"][:, :T], _score(store, pred, starts, 0, steps)["rel_l2"][:, :T])


@pytest.mark.parametrize("factor", [1, 2])
def test_targets_are_the_stores_and_copies_are_exact(factor):
    from bubbleformer_amd.data import BubbleForecast
    T, steps, starts, s = 2, 6, [0, 30, 42 + 25], 3
    ds = BubbleForecast(FILES, norm="std", downsample_factor=factor, time_window=T, start_time=5)
    ds.normalize()
    store = ds.device_store("cuda")
    pred = store.gather([st + s * T for st in starts])[1]
    a, b = _score(store, pred, starts, s, steps), _score(store, pred, starts, s, steps)
    rows = slice(s * T, (s + 1) * T)
    assert torch.equal(a["rel_l2"][:, rows], torch.zeros_like(a["rel_l2"][:, rows]))         # the target has the bits gather() returns
    assert torch.equal(a["criterion"][:, s], torch.zeros(3, device="cuda"))
    assert torch.equal(a["next_in"], pred) and torch.equal(a["archive"][:, rows], pred)
    assert int(a["counter"]) == s + 1
    for k in ("rel_l2", "criterion", "eik_pred", "eik_tgt", "next_in", "archive"):           # NaN marks rows no call wrote
        assert torch.equal(torch.nan_to_num(a[k], nan=-7.0), torch.nan_to_num(b[k], nan=-7.0)), k
    assert torch.equal(a["eik_pred"][:, rows].isfinite(), torch.ones(3, T, dtype=torch.bool, device="cuda"))
    past = _score(store, pred, starts, steps, steps)                                  # a counter behind the last row: nothing written, counter kept
    assert int(past["counter"]) == steps and torch.isnan(past["rel_l2"]).all() and torch.isnan(past["next_in"]).all()


def test_the_three_step_calls_read_the_same_store_frame():
    """`rollout_score`, `rollout_heatflux` and `rollout_bubbles` of one step all report on the stored frame clamp(first[b] + (s + 1) * T + t,
    0, total - 1), computed here in Python, including starts that need the clamp at either end of the store (`plan_rollouts` refuses those,
    so no other test gets there), with a channel that is not its own field id, at full resolution and through `nearest_src`.  A synthetic
    store inside a larger buffer: an unclamped index would read allocated memory and show up as a wrong value."""
    from bubbleformer_amd import ops
    from bubbleformer_amd.utils import physics
    from tests import heatflux_restatement as H_
    nf, total, H, W, C, T, steps, B, mb = 3, 12, 6, 10, 2, 2, 3, 3, 32
    margin = (steps + 1) * T * H * W                                                  # floats: a multiple of 4, so the store stays 16-byte aligned
    g = torch.Generator().manual_seed(7)
    flat = torch.randn(2 * margin + nf * total * H * W, generator=g).cuda()
    frames = flat[margin:margin + nf * total * H * W].view(nf, total, H, W)
    frames[0] += 3.0                                                                  # the temperature field: heater_temp - temp does not vanish
    assert frames.is_contiguous() and frames.data_ptr() % 16 == 0
    dev = frames.device
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    table = (i32([2, 0]), f32([0.3, -0.2]), f32([1.7, 0.6]))                         # channel 0 = field 2 (signed distance), channel 1 = field 0 (temperature)
    identity = (i32([0, 1, 2]), f32([0.0, 0.0, 0.0]), f32([1.0, 1.0, 1.0]))
    first_host = [-5, 3, total - 1]                                                   # clamped at 0, in range, clamped at total - 1
    first = torch.tensor(first_host, dtype=torch.int64, device=dev)
    temps = [1.0, 1.3, 1.15]
    heater = f32(temps)
    for Ho, Wo in ((6, 10), (3, 5)):
        spec = physics.HeaterSpec(1.0, x_min=-8.0, dx=16.0 / Wo)
        for s in (0, steps - 1):
            e = [[min(max(first_host[b] + (s + 1) * T + t, 0), total - 1) for t in range(T)] for b in range(B)]
            if s == 0:
                assert e[0][0] == 0 and e[2] == [total - 1] * T and e[1] == [3 + T, 3 + T + 1]      # both clamps and an in-range start are in play
            gather = lambda tab: torch.stack([torch.cat([ops.clip_gather(frames, torch.tensor([e[b][t]], dtype=torch.int64, device=dev), 0, 1, tab, Ho, Wo)[0]
                                                         for t in range(T)]) for b in range(B)])
            pred, raw = gather(table), gather(identity)                               # (B, T, C, Ho, Wo) normalised, (B, T, nf, Ho, Wo) as stored
            rows = slice(s * T, (s + 1) * T)
            counter = lambda: torch.full((1,), s, dtype=torch.int32, device=dev)
            nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
            # the scoring call: a prediction that IS the gathered frames e scores exactly 0, and is copied exactly
            rel, crit, ep, et, nxt, arch = nan(B, steps * T, C), nan(B, steps), nan(B, steps * T), nan(B, steps * T), nan(B, T, C, Ho, Wo), nan(B, steps * T, C, Ho, Wo)
            ops.rollout_score(pred, frames, first, counter(), table, 0, steps, rel, crit, ops.rollout_score_workspace(pred), ep, et, nxt, arch)
            print(f"{Ho}x{Wo} step {s}: frames {e}, rel_l2 max {float(rel[:, rows].max()):.3e}")
            assert torch.equal(rel[:, rows], torch.zeros_like(rel[:, rows]))
            assert torch.equal(nxt, pred) and torch.equal(arch[:, rows], pred)
            # the heat-flux call: its simulation rows against bf_heatflux_rows of the same raw frames
            fp, ft = nan(B, steps * T), nan(B, steps * T)
            ops.rollout_heatflux(pred, frames, first, counter(), table, 0, 1, heater, steps, fp, ft, x_min=spec.x_min, dx=spec.dx, lc=spec.lc,
                                 conductivity=spec.conductivity)
            liquid, vapour = H_.heater_cells(raw[:, :, 2, 0].cpu().numpy(), spec.x_min, spec.dx)
            assert liquid > 0 and vapour > 0, (liquid, vapour)                        # otherwise the mask is not exercised
            want = torch.stack([physics.heatflux_series(raw[b, :, 2].contiguous(), raw[b, :, 0].contiguous(), temps[b], spec) for b in range(B)])
            got = ft[:, rows]
            diff = (got.double() - want.double()).abs()                                # a heater row without a liquid cell has flux 0 on both sides
            print(f"{Ho}x{Wo} step {s}: flux_tgt worst relative error {float((diff / want.double().abs())[want != 0].max()):.2e} (bound 2e-6), "
                  f"bit-equal {torch.equal(got, want)}, {liquid} liquid / {vapour} vapour cells")
            assert bool(want.isfinite().all()) and bool((want != 0).any()) and bool((diff <= 2e-6 * want.double().abs()).all())
            # the census call: its simulation side against bf_bubble_census of the same raw frames
            bub = {k: [torch.full((B, steps * T) + tail, -9, dtype=torch.int32, device=dev) for _ in range(2)]
                   for k, tail in (("count", ()), ("cells", ()), ("attached", ()), ("area", (mb,)))}
            ops.rollout_bubbles(pred, frames, first, counter(), table, 0, steps, 4, mb, ops.bubble_census_workspace(2 * B * T, Ho, Wo, mb, dev),
                                *bub["count"], *bub["cells"], *bub["attached"], *bub["area"])
            census = physics.bubble_census(raw[:, :, 2], connectivity=4, max_bubbles=mb)
            print(f"{Ho}x{Wo} step {s}: bubbles per target frame {census.count.tolist()}")
            assert int(census.count.min()) > 0
            for k, want_k in (("count", census.count), ("cells", census.vapour_cells), ("attached", census.attached), ("area", census.area)):
                assert torch.equal(bub[k][1][:, rows], want_k), k


def _report_tensors(r):
    out = {"rel_l2": r.rel_l2, "criterion": r.criterion, "timesteps": r.timesteps}
    if r.eikonal_pred is not None:
        out["eikonal_pred"], out["eikonal_target"] = r.eikonal_pred, r.eikonal_target
    if r.predictions is not None:
        out["predictions"] = r.predictions
    return out


def test_one_trajectory_equals_todays_loop(tmp_path):
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils.rollout import autoregressive_rollout, evaluate_rollouts, relative_l2_per_step
    from oracle import weights as Wt
    cfg = dict(input_fields=4, output_fields=4, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=2)
    model = get_model("avit", time_window=4, drop_path=0.0, **cfg)
    model.load_state_dict(Wt.generate(Wt.param_shapes(**cfg), seed=3))
    model = model.cuda().eval()
    ds = BubbleForecast(FILES, norm="std", downsample_factor=2, time_window=4, start_time=5)
    ds.normalize()
    store = ds.device_store("cuda")
    start, steps = 7, 3
    x0 = store.gather([start])[0][0]
    tg = [store.gather([start + s * 4])[1][0] for s in range(steps)]
    pg, eg = autoregressive_rollout(model, x0, steps, use_graph=True, target_fn=lambda s: tg[s])
    pe, _ = autoregressive_rollout(model, x0, steps, use_graph=False)
    rg = evaluate_rollouts(model, store, [start], steps, use_graph=True, keep_predictions=True)
    re_ = evaluate_rollouts(model, ds, [start], steps, use_graph=False, keep_predictions=True)      # a BubbleForecast: its own device store
    assert rg.predictions.shape == (1, steps * 4, 4, 32, 32) and rg.fields == ALL
    assert torch.equal(rg.predictions[0], pg) and torch.equal(re_.predictions[0], pe) and torch.equal(pg, pe)
    a, b = _report_tensors(rg), _report_tensors(re_)
    assert sorted(a) == sorted(b) and len(a) == 6
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for s in range(steps):                                                            # the scalar today's loop reports, from the per-field curves
        assert float(rg.criterion[0, s]) == pytest.approx(float(eg[s]), rel=1e-5)
        assert float(rg.rel_l2[0, s * 4:(s + 1) * 4].mean()) == pytest.approx(float(relative_l2_per_step(pg[s * 4:(s + 1) * 4], tg[s])), rel=1e-5)
    assert rg.timesteps.tolist() == [list(range(5 + 7 + 4, 5 + 7 + 4 + 12))]
    no_sdf = evaluate_rollouts(model, store, [start], 1, sdf_field=None)
    assert no_sdf.eikonal_pred is None and no_sdf.eikonal_target is None and no_sdf.predictions is None
    assert torch.equal(no_sdf.rel_l2, rg.rel_l2[:, :4])
    rg.save(tmp_path / "report.pt")
    saved = torch.load(tmp_path / "report.pt")
    assert sorted(saved) == ["criterion", "eikonal_pred", "eikonal_target", "fields", "preds", "rel_l2", "timesteps"]
    assert torch.equal(saved["preds"], rg.predictions) and saved["fields"] == ALL


def test_batched_rollouts_match_the_reference_rollouts():
    """The reference's evaluation of both sample trajectories (fp64 run) against one batched fp32 run on the device: every entry of every
    report tensor within max(2e-5, 4 * field_drift_f32[step]) relative, the rule of test_native_rollout_matches_the_reference_rollout with
    the drift the reference's own fp32 run shows for that trajectory.  No entry is left out."""
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils.rollout import evaluate_rollouts
    from oracle import weights as W
    from oracle.gen_golden import ROLLOUT
    z = np.load(os.path.join(GOLDEN, "rollout_eval.npz"))
    old = np.load(os.path.join(GOLDEN, "rollout.npz"))
    T, steps, cfg = ROLLOUT["T"], ROLLOUT["steps"], ROLLOUT["cfg"]
    model = get_model(ROLLOUT["model"], time_window=T, drop_path=0.0, compute_dtype=torch.float32, **cfg)
    model.load_state_dict(W.generate(W.param_shapes(**cfg), seed=ROLLOUT["seed"]))
    model = model.cuda().eval()
    ds = golden_dataset(z)
    rep = evaluate_rollouts(model, ds, [int(i) for i in z["starts"]], steps)
    assert rep.fields == [str(n) for n in z["fields"]] and rep.rel_l2.shape == (2, steps * T, 4)
    for b in range(2):
        tol = np.maximum(2e-5, 4 * z[f"field_drift_f32/{b}"])
        frame_tol = np.repeat(tol, T)
        assert rep.timesteps[b].tolist() == list(range(5 + T, 5 + T + steps * T))
        for name, got, per in (("rel_l2", rep.rel_l2[b], frame_tol[:, None]), ("criterion", rep.criterion[b], tol),
                               ("eikonal_pred", rep.eikonal_pred[b], frame_tol), ("eikonal_target", rep.eikonal_target[b], frame_tol)):
            want = z[f"{name}_f64/{b}"]
            err = np.abs(got.cpu().numpy().astype(np.float64) - want) / np.abs(want)
            print(f"trajectory {b} {name}: worst share of the allowance {np.max(err / per):.3f} (step-1 error {err.reshape(steps, -1)[0].max():.2e})")
            assert got.shape == want.shape and np.all(err <= per), (b, name)
    err = np.abs(rep.criterion[0].cpu().numpy().astype(np.float64) - old["criterion_f64"]) / old["criterion_f64"]
    assert np.all(err <= np.maximum(2e-5, 4 * old["field_drift_f32"]))


def _study(fluid_order=(0, 1)):
    """The two sample trajectories in memory with a different fluid record per file."""
    from bubbleformer_amd.data import BubbleForecast, hdf5_lite
    trajs = [{k: np.asarray(f[k][...], dtype=np.float32) for k in ALL} for f in (hdf5_lite.File(p) for p in FILES)]
    rec = [{"inv_reynolds": 0.0042 + 0.3 * i, "cpgas": 0.83, "mugas": 0.023, "rhogas": 0.0083, "thcogas": 0.25, "stefan": 0.5298 - 0.2 * i,
            "prandtl": 8.4, "heater": {"nucWaitTime": 0.4, "wallTemp": 1.0 + 0.1 * i}} for i in range(2)]
    ds = BubbleForecast.from_arrays(trajs, [rec[i] for i in fluid_order], norm="std", time_window=4, start_time=5)
    ds.normalize()
    return ds


def _assert_trajectory_equals(batched, b, single):
    for k, v in _report_tensors(single).items():
        assert torch.equal(_report_tensors(batched)[k][b:b + 1], v), k


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_trajectories_do_not_mix(dtype):
    """Trajectory b of a B = 3 run against the B = 1 run from the same sample, a conditioned model with one fluid record per file.  The
    eval kernels reduce per frame / per token row in an order that does not depend on the batch, so the runs are bit-identical."""
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils.rollout import evaluate_rollouts
    from oracle import weights as Wt
    cfg = dict(input_fields=4, output_fields=4, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=2, num_fluid_params=9)
    model = get_model("filmavit", time_window=4, drop_path=0.0, compute_dtype=dtype, **cfg)
    model.load_state_dict(Wt.generate(Wt.param_shapes(**cfg), seed=5))
    model = model.cuda().eval()
    store = _study().device_store("cuda")
    starts, steps = [2, 38 + 9, 20], 3                                               # files 0, 1, 0 (38 samples per file at T = 4)
    assert [store.ds.locate(i)[0] for i in starts] == [0, 1, 0]
    batched = evaluate_rollouts(model, store, starts, steps, keep_predictions=True)
    singles = [evaluate_rollouts(model, store, [st], steps, keep_predictions=True) for st in starts]
    for b, single in enumerate(singles):
        d = (batched.predictions[b] - single.predictions[0]).double()
        print(f"{dtype} trajectory {b}: predictions differ by {float(d.norm() / single.predictions[0].double().norm()):.3e} relative L2, "
              f"bit-identical {torch.equal(batched.predictions[b], single.predictions[0])}")
    for b, single in enumerate(singles):
        _assert_trajectory_equals(batched, b, single)
    # the check above sees a fluid row in the wrong place: the same start on a study whose files carry each other's fluid records
    swapped = evaluate_rollouts(model, _study((1, 0)).device_store("cuda"), [starts[0]], steps, keep_predictions=True)
    with pytest.raises(AssertionError):
        _assert_trajectory_equals(batched, 0, swapped)


def test_classic_unet_goes_through_the_same_function():
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils.rollout import evaluate_rollouts
    torch.manual_seed(11)
    model = get_model("unet_classic", time_window=4, input_fields=4, output_fields=4, hidden_channels=8, compute_dtype=torch.float32).cuda().eval()
    store = _study().device_store("cuda")
    starts, steps = [2, 38 + 9, 20], 3
    batched = evaluate_rollouts(model, store, starts, steps, use_graph=True, keep_predictions=True)
    assert batched.predictions.shape == (3, steps * 4, 4, 64, 64) and bool(torch.isfinite(batched.rel_l2).all())
    for b, st in enumerate(starts):
        single = evaluate_rollouts(model, store, [st], steps, use_graph=True, keep_predictions=True)
        d = (batched.predictions[b] - single.predictions[0]).double()
        print(f"unet_classic trajectory {b}: predictions differ by {float(d.norm() / single.predictions[0].double().norm()):.3e} relative L2")
        _assert_trajectory_equals(batched, b, single)
    with pytest.raises(ValueError, match="time_window"):
        evaluate_rollouts(get_model("unet_classic", time_window=3, input_fields=4, output_fields=4, hidden_channels=8).cuda(), store, [0], 1)
