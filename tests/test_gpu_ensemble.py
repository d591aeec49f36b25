"""The ensemble rows on the GPU (csrc/ensemble.hip) against the numpy fp64 restatement tests/ensemble_restatement.py: `ensemble_scores` on both
sides of every template boundary and on every load path, determinism, and `evaluate_rollouts(ensemble=EnsembleSpec(...))` against
`ensemble_scores` of its own archive, the plain call and smaller ensembles."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import ensemble_restatement as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS = [2, 3, 5, 8, 9, 16, 17, 32]                   # both sides of the kernel's extents 4, 8, 16, 32
FLOAT_ROWS = ("mean_rmse", "spread", "crps")
ROWS = FLOAT_ROWS + ("rank_hist", "mean")


def _quads():
    """The 4-pixel groups a workgroup takes before a frame is shared, from the kernel's own constant."""
    src = open(os.path.join(REPO, "bubbleformer_amd", "csrc", "ensemble.hip")).read()
    return int(re.search(r"constexpr int ENS_QUADS = (\d+)", src).group(1))


def _shapes():
    """2 x 2: one 4-group; 5 x 7: ragged, no aligned row; 1 x 64: one row of 16-byte groups; 17 rows of width W = 1 (mod 4) with one group more than
    a workgroup's share (two workgroups, the second nearly idle, every row ends ragged); a 16-byte-aligned frame of three workgroups."""
    q = _quads()
    wq = q // 17 + 1                                     # 17 * wq groups: just above q
    above = (17, 4 * wq - 3)
    assert q < 17 * wq <= q + 17 and above[1] % 4 == 1
    side = 4 * int(np.ceil(np.sqrt(2 * q * 4 + 1) / 4))  # side^2 / 4 groups: above 2 q
    assert 2 * q < side * side // 4 <= 3 * q
    return [(2, 2), (5, 7), (1, 64), above, (side, side)]


def _run(x, y, fair=False, stride_pad=0):
    """`ops.ensemble_scores` on numpy members (M, F, H, W) / target (F, H, W); stride_pad floats between the member blocks."""
    from bubbleformer_amd import ops
    M, F, H, W = x.shape
    if stride_pad:
        big = torch.full((M, F * H * W + stride_pad), float("nan"), device="cuda")
        big[:, :F * H * W] = torch.from_numpy(x.reshape(M, -1)).cuda()
        xm = big[:, :F * H * W].view(M, F, H, W)
        assert xm.stride(0) == F * H * W + stride_pad
    else:
        xm = torch.from_numpy(x).cuda()
    new = lambda dtype, *shape: torch.full(shape, -5, dtype=dtype, device="cuda")
    rows = {"mean_rmse": new(torch.float32, F), "spread": new(torch.float32, F), "crps": new(torch.float32, F),
            "rank_hist": new(torch.int32, F, M + 1), "mean": new(torch.float32, F, H, W)}
    ops.ensemble_scores(xm, torch.from_numpy(y).cuda(), ops.ensemble_workspace(F, M, H, W, "cuda"), fair, **rows)
    return rows


@functools.lru_cache(maxsize=None)
def _reference(kind, M, F, shape, fair=False):
    """One case's inputs and the restatement's rows and bounds: computed once, shared by the tests below and never changed."""
    x, y = R.case(kind, M, F, shape[0], shape[1], seed=1000 * M + 10 * shape[1] + F + R.KINDS.index(kind))
    return (x, y) + R.ensemble_rows(x, y, fair)


def _check(got, want, bounds, where):
    worst = 0.0
    for key in FLOAT_ROWS + ("mean",):
        g, w, b = got[key].cpu().numpy().astype(np.float64), want[key], bounds[key]
        gap = np.abs(g - w)
        print(f"{where} {key}: worst gap {gap.max():.3e}, its bound {b.reshape(-1)[np.argmax(gap)]:.3e}")
        assert (gap <= b).all(), (where, key, float(gap.max()), float(b.reshape(-1)[np.argmax(gap - b)]))
        worst = max(worst, float(np.max(gap[b > 0] / b[b > 0], initial=0.0)))
    assert np.array_equal(got["rank_hist"].cpu().numpy(), want["rank_hist"]), where
    return worst


@pytest.mark.parametrize("M", MEMBERS)
def test_ensemble_scores_against_the_restatement(M):
    """Every output within its bound (one fp32 rounding of the value plus the fp64 re-ordering terms of tests/ensemble_restatement.py), the rank
    histogram exactly: on every frame shape, for 3 frames and for 1, standard-normal inputs, the cancellation case 1e4 + 1e-2 z, equal members
    (spread exactly 0, mass in bins 0 and M only), a truth that ties with a member on half the pixels, and member blocks further apart than
    dense (a stride that is no multiple of 4: the 4-byte loads)."""
    worst = 0.0
    for shape in _shapes():
        for kind, F, pad in (("normal", 3, 0), ("normal", 1, 0), ("offset", 3, 0), ("equal", 3, 0), ("ties", 3, 0), ("normal", 3, 8), ("normal", 3, 3)):
            x, y, want, bounds = _reference(kind, M, F, shape)
            got = _run(x, y, stride_pad=pad)
            worst = max(worst, _check(got, want, bounds, (M, shape, kind, F, pad)))
            if kind == "equal":
                assert not got["spread"].any() and not got["rank_hist"][:, 1:M].any()
                assert torch.equal(got["mean"], torch.from_numpy(x[0]).cuda())
            assert int(got["rank_hist"].sum()) == F * shape[0] * shape[1]
    print(f"M = {M}: worst ratio of an error to its bound {worst:.3f}")


@pytest.mark.parametrize("M", [3, 16, 17])
def test_same_bits_on_every_call_and_the_fair_weight(M):
    from bubbleformer_amd import ops
    from bubbleformer_amd.utils import ensemble_scores
    shape = _shapes()[3]
    x, y, want, bounds = _reference("normal", M, 3, shape)
    first, again = _run(x, y), _run(x, y)
    for key in ROWS:
        assert torch.equal(first[key], again[key]), key                                   # two calls: the same bits
    padded = _run(x, y, stride_pad=8)
    for key in ROWS:
        assert torch.equal(first[key], padded[key]), key                                  # the member stride changes no bit
    for f in range(3):
        alone = _run(x[:, f:f + 1].copy(), y[f:f + 1])                                   # a frame alone: the bits it has in the batch
        for key in ROWS:
            assert torch.equal(alone[key][0], first[key][f]), (f, key)
    # fair: only the CRPS moves, by the pair term times (M / (M - 1) - 1), the pair term from the restatement
    fair = _run(x, y, fair=True)
    _, _, want_fair, bounds_fair = _reference("normal", M, 3, shape, True)
    _check(fair, want_fair, bounds_fair, (M, "fair"))
    for key in ("mean_rmse", "spread", "rank_hist", "mean"):
        assert torch.equal(first[key], fair[key]), key
    assert np.allclose(want_fair["pair"], want["pair"] * M / (M - 1), rtol=1e-15, atol=0)
    moved = (first["crps"].double() - fair["crps"].double()).cpu().numpy()
    assert (np.abs(moved - want["pair"] / (M - 1)) <= bounds["crps"] + bounds_fair["crps"]).all()
    # the public function: leading dims, optional outputs, the same kernel
    xm = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2, 3))).cuda()           # (F, M, H, W)
    pub = ensemble_scores(xm, torch.from_numpy(y).cuda(), return_mean=True)
    assert pub.members == M and pub.rank_hist.dtype == torch.int32
    for key in ROWS:
        assert torch.equal(getattr(pub, key), first[key]), key
    bare = ensemble_scores(xm.reshape(3, 1, M, *shape), torch.from_numpy(y).cuda().reshape(3, 1, *shape), rank_histogram=False)
    assert bare.rank_hist is None and bare.mean is None and bare.crps.shape == (3, 1) and torch.equal(bare.crps.reshape(3), first["crps"])
    assert torch.equal(pub.spread_skill(), pub.spread * float(np.sqrt((M + 1) / M)) / pub.mean_rmse)
    # rows left out are not written, the others as before
    keep = {k: torch.full_like(first[k], -3) for k in FLOAT_ROWS}
    ops.ensemble_scores(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), ops.ensemble_workspace(3, M, *shape, "cuda"), **keep)
    assert all(torch.equal(keep[k], first[k]) for k in FLOAT_ROWS)
    from bubbleformer_amd import _lib
    with pytest.raises(_lib.BubbleformerHipError):
        ops.ensemble_scores(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), ops.ensemble_workspace(3, M, *shape, "cuda"), crps=keep["crps"])


# ---------------------------------------------------------------------------------------------------------------- evaluate_rollouts
T, STEPS, STARTS, M_ENS = 2, 2, [3, 27 + 5], 3


@functools.lru_cache(maxsize=None)
def _study(side, factor):
    """Two synthetic trajectories (30 and 21 frames of side x side) with fluid parameters, normalised, and their device store."""
    from bubbleformer_amd.data.dataset import BubbleForecast, FLUID_PARAM_KEYS
    g = np.random.default_rng(9 + side)
    names = ["dfun", "temperature", "velx", "vely"]
    yy, xx = np.meshgrid(np.linspace(0, 2 * np.pi, side), np.linspace(0, 2 * np.pi, side), indexing="ij")
    trajs = []
    for L in (30, 21):
        phase = g.uniform(0, 2 * np.pi, size=(len(names), 1, 1, 1))
        t = np.arange(L)[None, :, None, None] * 0.2
        fields = np.sin(yy + phase + t) * np.cos(2 * xx - phase + 0.5 * t) + 0.05 * g.standard_normal((len(names), L, side, side))
        trajs.append({n: fields[i].astype(np.float32) for i, n in enumerate(names)})
    fp = [dict({k: float(g.standard_normal()) for k in FLUID_PARAM_KEYS}, heater={"nucWaitTime": 0.1 * (i + 1), "wallTemp": 90.0 + i}) for i in range(2)]
    ds = BubbleForecast.from_arrays(trajs, fluid_params=fp, input_fields=names, output_fields=names, norm="std", time_window=T, start_time=0,
                                    downsample_factor=factor)
    ds.normalize()
    return ds.device_store("cuda")


@functools.lru_cache(maxsize=None)
def _model():
    from bubbleformer_amd.models import get_model
    from oracle import weights as Wt
    cfg = dict(input_fields=4, output_fields=4, patch_size=4, embed_dim=64, num_heads=1, processor_blocks=1, num_fluid_params=9)
    model = get_model("filmavit", time_window=T, drop_path=0.0, compute_dtype=torch.float32, **cfg)
    model.load_state_dict(Wt.generate(Wt.param_shapes(**cfg), seed=5))
    return model.cuda().eval()


@functools.lru_cache(maxsize=None)
def _report(side=16, factor=1, members=M_ENS, starts=tuple(STARTS), graph=True, std=0.05, **spec):
    from bubbleformer_amd.utils import EnsembleSpec
    from bubbleformer_amd.utils.rollout import evaluate_rollouts
    ens = EnsembleSpec(members, std, seed=7, **spec) if members else None
    return evaluate_rollouts(_model(), _study(side, factor), list(starts), STEPS, use_graph=graph, keep_predictions=True, ensemble=ens)


PLAIN_ROWS = ("rel_l2", "criterion", "eikonal_pred", "eikonal_target", "predictions")
ENS_ROWS = ("ensemble_mean_rmse", "ensemble_spread", "ensemble_crps", "ensemble_rank_hist")


def _against_ensemble_scores(report, store, starts, keep_mean):
    """The report's ensemble rows are `ensemble_scores` of its own kept members against the targets `clip_gather` returns: the same bits."""
    from bubbleformer_amd import ops
    from bubbleformer_amd.utils import ensemble_scores
    from bubbleformer_amd.utils.rollout import plan_rollouts
    M, Bt = report.ensemble_members, len(starts)
    members = report.by_member(report.predictions)                                        # (M, Bt, steps*T, C, Ho, Wo)
    assert members.shape[:3] == (M, Bt, STEPS * T)
    Ho, Wo = members.shape[-2:]
    first = torch.tensor(plan_rollouts(store.ds, starts, STEPS).first, dtype=torch.int64, device="cuda")
    targets = ops.clip_gather(store.frames, first, T, STEPS * T, store.out_tab, Ho, Wo)   # the frames behind the first input clip
    want = ensemble_scores(members.permute(1, 2, 3, 0, 4, 5).contiguous(), targets, return_mean=keep_mean)
    for key in ENS_ROWS:
        got = getattr(report, key)
        assert got.shape == getattr(want, key[9:]).shape and torch.equal(got, getattr(want, key[9:])), key
    assert report.ensemble_rank_hist.dtype == torch.int32 and report.ensemble_rank_hist.shape == (Bt, STEPS * T, 4, M + 1)
    assert bool((report.ensemble_rank_hist.sum(-1) == Ho * Wo).all())
    if keep_mean:
        assert torch.equal(report.ensemble_mean, want.mean)
        exact = members.double().mean(0)                                                  # one fp32 rounding of the fp64 mean of the kept members
        assert bool(((report.ensemble_mean.double() - exact).abs() <= 2.0 ** -24 * exact.abs() + 2.0 ** -50 * members.double().abs().mean(0)).all())
    else:
        assert report.ensemble_mean is None
    return want


def test_evaluate_rollouts_member_0_is_the_plain_call_and_the_rows_are_ensemble_scores():
    ens, plain = _report(keep_mean=True), _report(members=0)
    Bt = len(STARTS)
    assert ens.ensemble_members == M_ENS and ens.rel_l2.shape == (M_ENS * Bt, STEPS * T, 4) and ens.timesteps.shape == (M_ENS * Bt, STEPS * T)
    for key in PLAIN_ROWS:                                                                # control: member 0 is the unperturbed rollout
        assert torch.equal(ens.by_member(getattr(ens, key))[0], getattr(plain, key)), key
    assert torch.equal(ens.timesteps[:Bt], plain.timesteps) and torch.equal(ens.timesteps[Bt:2 * Bt], plain.timesteps)
    assert not torch.equal(ens.by_member(ens.predictions)[1], plain.predictions)          # the others are perturbed
    _against_ensemble_scores(ens, _study(16, 1), STARTS, True)
    assert bool((ens.ensemble_spread > 0).all()) and bool((ens.ensemble_crps > 0).all())
    M = M_ENS
    assert torch.equal(ens.spread_skill(), ens.ensemble_spread * float(np.sqrt((M + 1) / M)) / ens.ensemble_mean_rmse)
    hist = ens.rank_histogram()
    assert hist.shape == (Bt, 4, M + 1) and hist.dtype == torch.int64 and bool((hist.sum(-1) == STEPS * T * 256).all())
    for key in ("ensemble_members",) + ENS_ROWS + ("ensemble_mean",):                     # without the spec: none of the new attributes
        assert getattr(plain, key) is None, key
    with pytest.raises(ValueError, match="ensemble"):
        plain.spread_skill()


def test_evaluate_rollouts_graph_and_eager_give_the_same_bits():
    graph, eager = _report(keep_mean=True), _report(graph=False, keep_mean=True)
    for key in PLAIN_ROWS + ENS_ROWS + ("ensemble_mean",):
        assert torch.equal(getattr(graph, key), getattr(eager, key)), key


def test_evaluate_rollouts_noise_is_a_pure_function_of_seed_sample_and_member():
    """Member 1 of the M = 3 run is member 1 of an M = 2 run, and of a run on one of the trajectories alone: neither M, Bt nor the other
    trajectories of the call reach the noise (or the rows: they do not mix)."""
    Bt = len(STARTS)
    ens, two, one = _report(keep_mean=True), _report(members=2), _report(starts=(STARTS[1],))
    for key in PLAIN_ROWS:
        full = ens.by_member(getattr(ens, key))
        assert torch.equal(full[1], two.by_member(getattr(two, key))[1]), key
        assert torch.equal(full[1, 1:2], one.by_member(getattr(one, key))[1]), key
        assert torch.equal(full[2, 1:2], one.by_member(getattr(one, key))[2]), key
    for key in ENS_ROWS:                                                                  # a trajectory's ensemble rows: the same alone and in a batch
        assert torch.equal(getattr(ens, key)[1:2], getattr(one, key)), key
    other = _report(control=False)                                                        # without a control member 0 is perturbed too, the rest as before
    assert not torch.equal(other.by_member(other.predictions)[0], ens.by_member(ens.predictions)[0])
    assert torch.equal(other.by_member(other.predictions)[1:], ens.by_member(ens.predictions)[1:])


def test_evaluate_rollouts_without_noise_has_no_spread():
    calm, plain = _report(std=0.0), _report(members=0)
    members = calm.by_member(calm.predictions)
    for m in range(M_ENS):
        assert torch.equal(members[m], plain.predictions), m
    assert not calm.ensemble_spread.any()                                                 # exactly 0
    assert not calm.ensemble_rank_hist[..., 1:M_ENS].any()
    fair = _report(fair=True, rank_histogram=False)
    ens = _report(keep_mean=True)
    assert fair.ensemble_rank_hist is None and torch.equal(fair.ensemble_spread, ens.ensemble_spread) and bool((fair.ensemble_crps < ens.ensemble_crps).all())


def test_evaluate_rollouts_downsampled_store_relative_noise_render_and_save(tmp_path):
    """32 x 32 frames at downsample_factor 2 (the truth read through the nearest-neighbour map, 4-byte loads), noise relative to the fields' deviation."""
    from bubbleformer_amd.utils.rollout import render_rollouts
    store = _study(32, 2)
    report = _report(side=32, factor=2, relative=True)
    assert report.predictions.shape == (M_ENS * 2, STEPS * T, 4, 16, 16)
    _against_ensemble_scores(report, store, STARTS, False)
    out = render_rollouts(report, store, list(STARTS) * M_ENS, tmp_path, trajectories=[1, 2 * len(STARTS)])
    assert sorted(out) == [1, 4]
    for b in (1, 4):
        assert sorted(os.listdir(tmp_path / f"traj_{b}" / "plots")) == [f"{k:04d}.png" for k in range(STEPS * T)]
        assert (tmp_path / f"traj_{b}" / "relative_l2_error.csv").exists()
    report.save(tmp_path / "with.pt")
    _report(members=0).save(tmp_path / "without.pt")
    with_, without = torch.load(tmp_path / "with.pt"), torch.load(tmp_path / "without.pt")
    assert sorted(set(with_) - set(without)) == sorted(("ensemble_members",) + ENS_ROWS) and with_["ensemble_members"] == M_ENS
    for key in ENS_ROWS:
        assert torch.equal(with_[key], getattr(report, key)), key


def test_register_audit_lists_the_ensemble_kernels_without_spills():
    from tests.test_ensemble import KERNELS, audited_ensemble_kernels
    mine = audited_ensemble_kernels()
    assert sorted(mine) == sorted(KERNELS)
    for name, k in mine.items():
        assert k.get("vgpr_spill", 0) == 0 and k.get("scratch", 0) == 0, (name, k)
