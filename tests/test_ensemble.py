"""CPU: the ensemble rows' restatement agrees with itself, EnsembleSpec validates, the bf_ensemble_rows record mirrors the header, the two entry
points refuse null records before any HIP call, evaluate_rollouts keeps its signature, and the member-major plan is M equal blocks."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import ensemble_restatement as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("ensemble_kernel<4>", "ensemble_kernel<8>", "ensemble_kernel<16>", "ensemble_kernel<32>", "ensemble_finish_kernel")


@pytest.mark.parametrize("M", [2, 3, 8, 17, 32])
@pytest.mark.parametrize("fair", [False, True])
def test_pairwise_crps_equals_the_sorted_form_in_fp64(M, fair):
    for kind in ("normal", "ties"):
        x, y = R.case(kind, M, 2, 5, 7, seed=M)
        rows, bounds = R.ensemble_rows(x, y, fair)
        for f in range(2):
            want = R.crps_sorted(x[:, f], y[f], fair)
            assert abs(rows["crps"][f] - want) <= 1e-13 * (abs(want) + rows["pair"][f]), (kind, f, rows["crps"][f], want)
    # the cancellation case: the two forms still agree in fp64 (to the digits the sorted form keeps: its terms are 1e6 times their sum there)
    x, y = R.case("offset", M, 1, 5, 7, seed=M)
    rows, _ = R.ensemble_rows(x, y, fair)
    assert abs(rows["crps"][0] - R.crps_sorted(x[:, 0], y[0], fair)) <= 1e-7 * rows["pair"][0]


@pytest.mark.parametrize("M", [2, 5, 32])
def test_restatement_on_equal_members_and_histogram_mass(M):
    x, y = R.case("equal", M, 3, 5, 7, seed=3)
    rows, bounds = R.ensemble_rows(x, y)
    assert not rows["spread"].any() and not rows["pair"].any()
    mae = np.abs(x[0].astype(np.float64) - y).reshape(3, -1).mean(1)
    assert np.allclose(rows["crps"], mae, rtol=1e-14, atol=0)
    assert not rows["rank_hist"][:, 1:M].any() and (rows["rank_hist"].sum(1) == 35).all()
    assert np.array_equal(rows["mean"], x[0].astype(np.float64))
    for kind in R.KINDS:
        x, y = R.case(kind, M, 2, 4, 9, seed=11)
        rows, bounds = R.ensemble_rows(x, y)
        assert (rows["rank_hist"].sum(1) == 36).all() and rows["rank_hist"].shape == (2, M + 1)
        assert all((bounds[k] >= 0).all() for k in bounds)
        if kind != "equal":                         # the bound of every row stays near one fp32 rounding of it: the offset costs the pairwise form nothing
            assert (bounds["crps"] <= 1.001 * R.U32 * np.abs(rows["crps"]) + 1e-10 * (np.abs(rows["crps"]) + rows["pair"])).all(), kind
    x, y = R.case("ties", M, 1, 8, 8, seed=5)
    tied = (x[:, 0] == y[0]).any(0)
    assert 16 <= tied.sum() <= 48                   # about half the pixels
    rows, _ = R.ensemble_rows(x, y)
    assert rows["rank_hist"][0, M] <= (~tied).sum()             # a pixel whose truth equals a member cannot have all M members below it


def test_fair_weight_is_the_pair_term_times_m_over_m_minus_1():
    x, y = R.case("normal", 5, 2, 6, 6, seed=1)
    plain, _ = R.ensemble_rows(x, y)
    fair, _ = R.ensemble_rows(x, y, fair=True)
    assert np.allclose(fair["pair"], plain["pair"] * 5 / 4, rtol=1e-15, atol=0)
    assert np.allclose(plain["crps"] - fair["crps"], plain["pair"] / 4, rtol=1e-12, atol=0)
    for key in ("mean_rmse", "spread", "mean", "rank_hist"):
        assert np.array_equal(plain[key], fair[key])


def test_ensemble_spec_validates():
    from bubbleformer_amd.utils import EnsembleSpec
    spec = EnsembleSpec(4, 0.1)
    assert (spec.members, spec.std, spec.relative, spec.seed, spec.control, spec.fair, spec.rank_histogram, spec.keep_mean) == (
        4, 0.1, False, 0, True, False, True, False)
    assert EnsembleSpec(2, (0.1, 0, 0.2)).std == (0.1, 0.0, 0.2) and EnsembleSpec(32, 0).std == 0.0
    assert EnsembleSpec(3, 0.5).sigma(2) == [0.5, 0.5] and EnsembleSpec(3, (1.0, 2.0), relative=True).sigma(2, [0.5, 0.25]) == [0.5, 0.5]
    with pytest.raises(dataclass_frozen_error()):
        spec.members = 5
    for bad in (dict(members=1), dict(members=33), dict(members=True), dict(members=4.0), dict(std=-0.1), dict(std=True), dict(std=(0.1, -1)),
                dict(std=float("nan")), dict(std="0.1"), dict(relative=1), dict(seed=True), dict(seed=1.5), dict(control=1), dict(fair=0),
                dict(rank_histogram=None), dict(keep_mean="no")):
        with pytest.raises(ValueError, match="EnsembleSpec"):
            EnsembleSpec(**{**dict(members=4, std=0.1), **bad})
    with pytest.raises(ValueError):
        EnsembleSpec(3, (0.1, 0.2)).sigma(4)
    with pytest.raises(ValueError):
        EnsembleSpec(3, 0.1, relative=True).sigma(4)


def dataclass_frozen_error():
    import dataclasses
    return dataclasses.FrozenInstanceError


def _record_fields(name):
    """[(field, ctypes type)] of `typedef struct name { ... } name;` as the header declares it: a pointer is a c_void_p, int64_t a c_int64, int32_t /
    int a c_int32; a declaration may name several fields (`float *a, *b;`: the star belongs to the declarator)."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "bubbleformer_hip.h")).read(), flags=re.S)
    m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), txt, flags=re.S)
    assert m, name
    scalars = {"int64_t": C.c_int64, "int32_t": C.c_int32, "int": C.c_int32}
    fields = []
    for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
        base, rest = re.match(r"(?:const\s+)?(\w+)\s*(.*)$", decl, flags=re.S).groups()
        for d in rest.split(","):
            fields.append((d.replace("*", "").strip(), C.c_void_p if "*" in d else scalars[base]))
    return fields


def test_ensemble_rows_record_mirrors_the_header():
    from bubbleformer_amd import _lib
    declared = _record_fields("bf_ensemble_rows")
    assert [n for n, _ in declared] == ["mean_rmse", "spread", "crps", "rank_hist", "mean"]
    assert [(n, t) for n, t in _lib.EnsembleRows._fields_] == declared
    assert C.sizeof(_lib.EnsembleRows) == sum(C.sizeof(t) for _, t in declared) == 40
    for name in ("bf_ensemble_scores_ws_bytes", "bf_ensemble_scores", "bf_rollout_ensemble"):
        assert name in _lib.SIGNATURES


def _lib_handle():
    from bubbleformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib, _lib.lib()


@pytest.mark.parametrize("name", ["bf_ensemble_scores", "bf_rollout_ensemble"])
def test_null_record_and_null_member_are_refused(name):
    """A NULL record, and a record whose mean_rmse is NULL, are the call's null pointer: both return at the first check, before any HIP call."""
    L, h = _lib_handle()
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    step = L.RolloutStep(pred=p, frames=p, field_stride=64, total_frames=4, first=p, step=p, field=p, diff=p, div=p, nfields=1, B=2, T=2, C=1, H=4, W=4,
                         Ho=4, Wo=4, steps=1)
    for rows in (None, L.EnsembleRows(mean_rmse=None, spread=p, crps=p), L.EnsembleRows(mean_rmse=p, spread=None, crps=p),
                 L.EnsembleRows(mean_rmse=p, spread=p, crps=None)):
        rec = rows if rows is None else C.byref(rows)
        if name == "bf_ensemble_scores":
            rc = h.bf_ensemble_scores(p, 16, p, 1, 2, 4, 4, 0, rec, p, 1 << 20, None)
        else:
            rc = h.bf_rollout_ensemble(C.byref(step), 2, 0, rec, p, 1 << 20, None)
        assert rc != 0 and h.bf_last_error().decode().endswith(name + ": null pointer"), h.bf_last_error()
    assert h.bf_rollout_ensemble(None, 2, 0, C.byref(L.EnsembleRows(mean_rmse=p, spread=p, crps=p)), p, 1 << 20, None) != 0
    assert h.bf_last_error().decode().endswith("bf_rollout_ensemble: null pointer")


def test_size_errors_name_the_function():
    L, h = _lib_handle()
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    rows = L.EnsembleRows(mean_rmse=p, spread=p, crps=p)
    for members, stride in ((1, 16), (33, 16), (2, 15)):
        assert h.bf_ensemble_scores(p, stride, p, 1, members, 4, 4, 0, C.byref(rows), p, 1 << 20, None) != 0
        assert "bf_ensemble_scores: bad sizes" in h.bf_last_error().decode()
    assert h.bf_ensemble_scores(p, 16, p, 1, 2, 4, 4, 0, C.byref(rows), p, 8, None) != 0          # a workspace too small
    assert "bf_ensemble_scores: the workspace" in h.bf_last_error().decode()
    for B, members in ((3, 2), (2, 1), (66, 33)):                                                # B % members != 0, and members outside 2 .. 32
        step = L.RolloutStep(pred=p, frames=p, field_stride=64, total_frames=4, first=p, step=p, field=p, diff=p, div=p, nfields=1, B=B, T=2, C=1, H=4,
                             W=4, Ho=4, Wo=4, steps=1)
        assert h.bf_rollout_ensemble(C.byref(step), members, 0, C.byref(rows), p, 1 << 20, None) != 0
        assert "bf_rollout_ensemble: bad sizes" in h.bf_last_error().decode()
    assert h.bf_ensemble_scores_ws_bytes(1, 1, 4, 4) == 0 and h.bf_ensemble_scores_ws_bytes(1, 33, 4, 4) == 0 and h.bf_ensemble_scores_ws_bytes(0, 2, 4, 4) == 0
    assert h.bf_ensemble_scores_ws_bytes(3, 5, 4, 4) == (3 * (32 + 6 * 4) + 15) // 16 * 16 and h.bf_ensemble_scores_ws_bytes(1, 2, 2, 2) % 16 == 0
    assert h.bf_abi_version() == 3


def test_ensemble_scores_has_no_cpu_path():
    import torch
    from bubbleformer_amd import _lib
    from bubbleformer_amd.utils import ensemble_scores
    with pytest.raises(_lib.BubbleformerHipError):
        ensemble_scores(torch.zeros(3, 4, 4), torch.zeros(4, 4))


def test_evaluate_rollouts_keeps_the_parents_signature():
    from bubbleformer_amd.utils.rollout import RolloutReport, evaluate_rollouts
    import dataclasses
    params = inspect.signature(evaluate_rollouts).parameters
    assert list(params) == ["model", "data", "starts", "steps", "use_graph", "sdf_field", "keep_predictions", "heatflux", "bubbles", "errors", "ensemble"]
    assert [params[k].default for k in list(params)[4:]] == [True, "dfun", False, None, None, None, None]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(params)[4:])
    names = [f.name for f in dataclasses.fields(RolloutReport)]
    assert names[-1] == "bubble_departure_area_target" and not any(n.startswith("ensemble") for n in names)
    report = RolloutReport(None, None, None, None, None, [])
    for key in ("ensemble_members", "ensemble_mean_rmse", "ensemble_spread", "ensemble_crps", "ensemble_rank_hist", "ensemble_mean"):
        assert getattr(report, key) is None
    for call in (report.spread_skill, report.rank_histogram, lambda: report.by_member(None)):
        with pytest.raises(ValueError, match="ensemble"):
            call()


def test_member_major_plan_is_m_equal_blocks():
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.utils.rollout import plan_rollouts
    names = ["dfun", "temperature", "velx", "vely"]
    trajs = [{n: np.zeros((L, 4, 4), np.float32) for n in names} for L in (30, 21)]
    ds = BubbleForecast.from_arrays(trajs, input_fields=names, output_fields=names, norm="none", time_window=2, start_time=0)
    starts, M, steps = [3, 27 + 5], 3, 2
    one, all_ = plan_rollouts(ds, starts, steps), plan_rollouts(ds, list(starts) * M, steps)
    assert all_.first == one.first * M and all_.files == one.files * M
    assert all_.timesteps.shape == (M * 2, steps * 2)
    for m in range(M):
        assert (all_.timesteps[m * 2:(m + 1) * 2] == one.timesteps).all()


def audited_ensemble_kernels():
    """tools/register_audit.py's rows of csrc/ensemble.hip by kernel name (the build leaves the compiler's remarks beside the objects)."""
    from bubbleformer_amd import _lib
    from tools import register_audit
    if not os.path.exists(os.path.join(register_audit.BUILD, "ensemble.remarks")):
        _lib.build()
    rows, bad, warn, missing = register_audit.audit()
    assert "ensemble" not in register_audit.counted_wait_files()
    return {k["kernel"]: k for k in rows if k["file"] == "ensemble"}


def test_register_audit_lists_the_ensemble_kernels_without_spills():
    mine = audited_ensemble_kernels()
    assert sorted(mine) == sorted(KERNELS)
    for name, k in mine.items():
        assert k.get("vgpr_spill", 0) == 0 and k.get("scratch", 0) == 0, (name, k)
        assert k["vgpr"] <= 256 and k["occ"] >= 2, (name, k)
