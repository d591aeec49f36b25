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
