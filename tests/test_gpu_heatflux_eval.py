"""Heat-flux evaluation on the GPU: `bf_rollout_heatflux` against the fp64 restatement and the reference's own rows
(tests/golden/heatflux_eval.npz, tools/gen_heatflux_golden.py), `evaluate_rollouts(heatflux=...)` against the run without it and against
`heatflux_series` of its archive, and `bf_kde_kl` against cell 4 of examples/data_visualization.ipynb executed by the generator."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import heatflux_restatement as H
from tests.test_rollout_eval import FILES, GOLDEN

pytestmark = pytest.mark.gpu
ALL = ["dfun", "temperature", "velx", "vely"]
U = 2.0 ** -53


def _golden():
    return np.load(os.path.join(GOLDEN, "heatflux_eval.npz"))


def test_heatflux_series_matches_the_reference_rows():
    """rtol 2e-6: test_physics_kernels_match_reference_values' figure for this expression (fp32 difference, fp64 sum, one fp32 rounding)."""
    from bubbleformer_amd.utils import HeaterSpec, heatflux_series, physics
    z = _golden()
    dfun, temp = (torch.from_numpy(a).cuda() for a in H.flux_fields())
    for k, ht in enumerate(H.HEATER_TEMPS):
        rows = heatflux_series(dfun, temp, ht)
        assert rows.shape == (3,) and rows.dtype == torch.float32
        err = np.abs(rows.cpu().numpy().astype(np.float64) - z[f"flux/{k}"]) / z[f"flux/{k}"]
        print(f"heater {ht}: worst relative error {err.max():.2e} (bound 2e-6)")
        assert np.all(err <= 2e-6)
        mean, mx = physics.heatflux(dfun, temp, ht)
        assert torch.equal(rows.mean(), mean) and torch.equal(rows.max(), mx)
        assert torch.equal(rows, heatflux_series(dfun, temp, ht, HeaterSpec(ht)))
    with pytest.raises(ValueError, match="columns"):
        heatflux_series(dfun[:, :, :256], temp[:, :, :256], 1.0)
    # another conductivity scales the rows
    twice = heatflux_series(dfun, temp, 1.0, HeaterSpec(1.0, conductivity=0.108))
    assert np.allclose(twice.cpu().numpy(), 2 * heatflux_series(dfun, temp, 1.0).cpu().numpy(), rtol=1e-6)


def _heatflux(store, pred, starts, s, steps, heater, spec_kw):
    """One eager `ops.rollout_heatflux` call with the step counter preset to s, on NaN-filled outputs."""
    from bubbleformer_amd import ops
    from bubbleformer_amd.utils.rollout import plan_rollouts
    B, T = pred.shape[:2]
    dev = pred.device
    first = torch.tensor(plan_rollouts(store.ds, starts, steps).first, dtype=torch.int64, device=dev)
    fp, ft = (torch.full((B, steps * T), float("nan"), dtype=torch.float32, device=dev) for _ in range(2))
    counter = torch.full((1,), s, dtype=torch.int32, device=dev)
    ops.rollout_heatflux(pred, store.frames, first, counter, store.out_tab, 0, 1, heater, steps, fp, ft, **spec_kw)
    return fp, ft, counter


@pytest.mark.parametrize("norm", ["none", "std"])
@pytest.mark.parametrize("factor", [1, 2])
def test_heatflux_kernel_against_fp64(norm, factor):
    """Simulation rows against the restatement on the raw gathered clips, prediction rows against the restatement on pred * div + diff
    formed in fp32 with the kernel's two roundings (the liquid mask is then decided on identical bits), rtol 2e-6."""
    from bubbleformer_amd import _lib
    from bubbleformer_amd.data import BubbleForecast
    T, steps, starts = 2, 8, [3, 20, 42 + 10]
    ds = BubbleForecast(FILES, norm=norm, downsample_factor=factor, time_window=T, start_time=5)
    ds.normalize()
    store = ds.device_store("cuda")
    raw = BubbleForecast(FILES, norm="none", downsample_factor=factor, time_window=T, start_time=5)
    raw.normalize()
    raw_store = raw.device_store("cuda")
    _, diff, div = store.out_tab
    hw = 64 // factor
    kw = dict(x_min=-8.0, dx=factor / 4, lc=0.0007, conductivity=0.054)
    g = torch.Generator().manual_seed(300 * factor + len(norm))
    pred = torch.randn((3, T, 4, hw, hw), generator=g).cuda()
    temps = [1.0, 1.3, 1.15]
    heater = torch.tensor(temps, dtype=torch.float32, device="cuda")
    for s in (0, steps - 1):
        fp, ft, counter = _heatflux(store, pred, starts, s, steps, heater, kw)
        assert int(counter) == s                                                     # read, never written
        rows = slice(s * T, (s + 1) * T)
        tgt = raw_store.gather([st + s * T for st in starts])[1]                     # the raw, downsampled target clips
        phys = pred * div.view(1, 1, 4, 1, 1) + diff.view(1, 1, 4, 1, 1)             # fp32 multiply, then add
        for name, got, clip in (("sim", ft, tgt), ("pred", fp, phys)):
            d_row, t_row = clip[:, :, 0, 0].cpu().numpy(), clip[:, :, 1, 0].cpu().numpy()      # (B, T, W): row 0 of dfun and temperature
            liquid, vapour = H.heater_cells(d_row, kw["x_min"], kw["dx"])
            assert liquid > 0 and vapour > 0, (name, liquid, vapour)                 # otherwise the mask is not exercised
            want = np.stack([H.heatflux_rows(d_row[b], t_row[b], temps[b], **kw) for b in range(3)])
            g_ = got[:, rows].cpu().numpy().astype(np.float64)
            err = np.abs(g_ - want) / np.abs(want)
            print(f"norm {norm} factor {factor} step {s} {name}: worst relative error {err.max():.2e} (bound 2e-6), {liquid} liquid / {vapour} vapour cells")
            assert np.all(np.abs(want) > 0) and np.all(err <= 2e-6)
        untouched = torch.ones(steps * T, dtype=torch.bool)
        untouched[rows] = False
        assert torch.isnan(fp[:, untouched.cuda()]).all() and torch.isnan(ft[:, untouched.cuda()]).all()      # only this step's rows
        again = _heatflux(store, pred, starts, s, steps, heater, kw)
        assert torch.equal(again[0][:, rows], fp[:, rows]) and torch.equal(again[1][:, rows], ft[:, rows])
    fp, ft, counter = _heatflux(store, pred, starts, steps, steps, heater, kw)       # a counter behind the last row: nothing written
    assert int(counter) == steps and torch.isnan(fp).all() and torch.isnan(ft).all()
    with pytest.raises(_lib.BubbleformerHipError, match="heater_temp"):
        _heatflux(store, pred, starts, 0, steps, heater[:2].contiguous(), kw)
    with pytest.raises(_lib.BubbleformerHipError, match="prediction"):
        _heatflux(store, pred.double(), starts, 0, steps, heater, kw)


def _tiny_model():
    from bubbleformer_amd.models import get_model
    from oracle import weights as Wt
    cfg = dict(input_fields=4, output_fields=4, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=2)
    model = get_model("avit", time_window=4, drop_path=0.0, **cfg)
    model.load_state_dict(Wt.generate(Wt.param_shapes(**cfg), seed=3))
    return model.cuda().eval()


@functools.lru_cache(maxsize=None)
def _tiny_reports():
    """The rollout of test_one_trajectory_equals_todays_loop (tiny avit, 32 x 32 after downsampling by 2, three steps of four frames), with the
    heat flux in a graph and eagerly, and without it."""
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.utils import HeaterSpec
    from bubbleformer_amd.utils.rollout import evaluate_rollouts
    model = _tiny_model()
    ds = BubbleForecast(FILES, norm="std", downsample_factor=2, time_window=4, start_time=5)
    ds.normalize()
    store = ds.device_store("cuda")
    spec = HeaterSpec(heater_temp=1.1, dx=1 / 2)
    graph = evaluate_rollouts(model, store, [7], 3, use_graph=True, keep_predictions=True, heatflux=spec)
    eager = evaluate_rollouts(model, store, [7], 3, use_graph=False, keep_predictions=True, heatflux=spec)
    plain = evaluate_rollouts(model, store, [7], 3, use_graph=True, keep_predictions=True)
    return store, spec, graph, eager, plain


def _tensors(r):
    from tests.test_gpu_rollout_eval import _report_tensors
    out = _report_tensors(r)
    if r.heatflux_pred is not None:
        out["heatflux_pred"], out["heatflux_target"] = r.heatflux_pred, r.heatflux_target
    return out


def test_evaluate_rollouts_with_heatflux(tmp_path):
    from bubbleformer_amd.utils import heatflux_series
    from bubbleformer_amd.utils.rollout import evaluate_rollouts
    store, spec, graph, eager, plain = _tiny_reports()
    a, b, c = _tensors(graph), _tensors(eager), _tensors(plain)
    assert sorted(a) == sorted(b) and len(a) == 8 and len(c) == 6 and plain.heatflux_pred is None and plain.heatflux_target is None
    for k in a:
        assert torch.equal(a[k], b[k]), k                                            # graph and eager runs: the same bits
    for k in c:
        assert torch.equal(a[k], c[k]), k                                            # nothing else moves when the heat flux is asked for
    assert graph.heatflux_pred.shape == (1, 12) and graph.heatflux_pred.dtype == torch.float32 and bool(torch.isfinite(graph.heatflux_pred).all())
    _, diff, div = store.out_tab
    phys = graph.predictions[0] * div.view(1, 4, 1, 1) + diff.view(1, 4, 1, 1)       # the de-normalised archive, fp32 multiply then add
    want = heatflux_series(phys[:, 0].contiguous(), phys[:, 1].contiguous(), 1.1, spec)
    gap = (graph.heatflux_pred[0] - want).abs()
    print(f"heatflux_pred against heatflux_series of the archive: worst gap {float(gap.max()):.2e} on rows of size {float(want.abs().max()):.2e} (rtol 2e-6)")
    assert bool((gap <= 2e-6 * want.abs()).all())
    raw_rows = store.frames[:, 5 + 7 + 4:5 + 7 + 4 + 12, ::2, ::2]                    # file 0, the twelve target frames, nearest-neighbour map of factor 2
    fields = store.fields
    sim = heatflux_series(raw_rows[fields.index("dfun")].contiguous(), raw_rows[fields.index("temperature")].contiguous(), 1.1, spec)
    assert bool(((graph.heatflux_target[0] - sim).abs() <= 2e-6 * sim.abs()).all()) and bool((sim != 0).all())
    graph.save(tmp_path / "with.pt")
    plain.save(tmp_path / "without.pt")
    with_, without = torch.load(tmp_path / "with.pt"), torch.load(tmp_path / "without.pt")
    assert sorted(without) == ["criterion", "eikonal_pred", "eikonal_target", "fields", "preds", "rel_l2", "timesteps"]
    assert sorted(set(with_) - set(without)) == ["heatflux_pred", "heatflux_target"] and set(without) <= set(with_)
    assert torch.equal(with_["heatflux_pred"], graph.heatflux_pred) and torch.equal(with_["heatflux_target"], graph.heatflux_target)
    graph.save_heatfluxes(tmp_path / "heatfluxes.pt")
    hf = torch.load(tmp_path / "heatfluxes.pt")
    assert sorted(hf) == ["model_hf", "sim_hf"]
    for key, src in (("sim_hf", graph.heatflux_target), ("model_hf", graph.heatflux_pred)):
        assert hf[key].device.type == "cpu" and hf[key].dtype == torch.float32 and hf[key].dim() == 1 and torch.equal(hf[key], src.reshape(-1).cpu())
    model = _tiny_model()
    with pytest.raises(ValueError, match="pressure"):
        evaluate_rollouts(model, store, [7], 1, heatflux=type(spec)(1.1, dx=1 / 2, temperature_field="pressure"))      # not an output field
    with pytest.raises(ValueError, match="columns"):
        evaluate_rollouts(model, store, [7], 1, heatflux=type(spec)(1.1))             # the default dx on a 32-column frame
    with pytest.raises(ValueError, match="2 files"):
        evaluate_rollouts(model, store, [7], 1, heatflux=type(spec)((1.0, 1.1, 1.2), dx=1 / 2))


def test_report_heatflux_kl_is_the_divergence_of_its_rows():
    from bubbleformer_amd.utils import kde_kl_divergence
    from bubbleformer_amd.utils.rollout import RolloutReport
    _, _, graph, _, _ = _tiny_reports()
    case = H.KL_CASES[0]
    sets = [H.kl_sets(case, seed) for seed in (21, 22, 23)]                           # a report whose rows are flux-shaped sets, three trajectories
    sim = torch.from_numpy(np.stack([s for s, _ in sets])).float().cuda()
    model = torch.from_numpy(np.stack([m for _, m in sets])).float().cuda()
    made = RolloutReport(graph.rel_l2, graph.criterion, None, None, graph.timesteps, graph.fields, None, model, sim)
    for rep in (graph, made):
        same = lambda a, b: torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))
        per = rep.heatflux_kl()
        B = rep.heatflux_pred.shape[0]
        assert per.shape == (B,) and per.dtype == torch.float64
        for b in range(B):
            assert same(per[b], kde_kl_divergence(rep.heatflux_target[b], rep.heatflux_pred[b]))
        pooled = rep.heatflux_kl(pooled=True)
        assert pooled.dim() == 0 and same(pooled, kde_kl_divergence(rep.heatflux_target.reshape(-1), rep.heatflux_pred.reshape(-1)))
        assert same(rep.heatflux_kl(points=400)[0], kde_kl_divergence(rep.heatflux_target[0], rep.heatflux_pred[0], points=400))
        print("heat-flux KL per trajectory", [f"{v:.5f}" for v in per.tolist()], "pooled", f"{float(pooled):.5f}")
    assert bool(torch.isfinite(made.heatflux_kl()).all()) and float(made.heatflux_kl(pooled=True)) > 0


def test_reference_geometry_targets_match_the_reference_rows():
    """Two 512 x 512 trajectories at the reference's constants (default spec), one heater temperature per file: every simulated row against
    the row the reference's `heatflux` gave for that frame, rtol 2e-6."""
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils import HeaterSpec
    from bubbleformer_amd.utils.rollout import evaluate_rollouts
    from oracle import weights as Wt
    z = _golden()
    T, steps = 2, 2
    ds = BubbleForecast.from_arrays(H.synthetic_study(), norm="none", time_window=T, start_time=0)
    ds.normalize()
    per_file = H.STUDY_FRAMES - 2 * T + 1
    assert len(ds) == 2 * per_file
    cfg = dict(input_fields=4, output_fields=4, patch_size=16, embed_dim=64, num_heads=1, processor_blocks=1)
    model = get_model("avit", time_window=T, drop_path=0.0, **cfg)
    model.load_state_dict(Wt.generate(Wt.param_shapes(**cfg), seed=9))
    rep = evaluate_rollouts(model.cuda().eval(), ds, [0, per_file], steps, heatflux=HeaterSpec(heater_temp=H.STUDY_HEATER_TEMPS))
    assert rep.heatflux_target.shape == (2, steps * T) and rep.heatflux_pred.shape == (2, steps * T) and rep.predictions is None
    assert rep.timesteps.tolist() == [list(range(T, T + steps * T))] * 2
    for b in range(2):
        want = z[f"study_flux/{b}"][T:T + steps * T]
        err = np.abs(rep.heatflux_target[b].cpu().numpy().astype(np.float64) - want) / want
        print(f"file {b}: worst relative error of a simulated row {err.max():.2e} (bound 2e-6)")
        assert err.shape == (steps * T,) and np.all(err <= 2e-6)
    assert bool(torch.isfinite(rep.heatflux_pred).all())


def test_trajectories_do_not_mix():
    """Row b of a B = 3 run against the B = 1 run from the same sample (conditioned model, one heater temperature per file); the same start on
    a spec whose files carry each other's temperatures differs."""
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils import HeaterSpec
    from bubbleformer_amd.utils.rollout import evaluate_rollouts
    from oracle import weights as Wt
    from tests.test_gpu_rollout_eval import _study
    cfg = dict(input_fields=4, output_fields=4, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=2, num_fluid_params=9)
    model = get_model("filmavit", time_window=4, drop_path=0.0, compute_dtype=torch.float32, **cfg)
    model.load_state_dict(Wt.generate(Wt.param_shapes(**cfg), seed=5))
    model = model.cuda().eval()
    store = _study().device_store("cuda")
    starts, steps = [2, 38 + 9, 20], 3                                               # files 0, 1, 0
    spec = HeaterSpec(heater_temp=(1.0, 1.25), dx=1 / 4)
    batched = evaluate_rollouts(model, store, starts, steps, heatflux=spec)
    for b, st in enumerate(starts):
        single = evaluate_rollouts(model, store, [st], steps, heatflux=spec)
        for k, v in _tensors(single).items():
            assert torch.equal(_tensors(batched)[k][b:b + 1], v), (b, k)
    swapped = evaluate_rollouts(model, store, [starts[0]], steps, heatflux=HeaterSpec(heater_temp=(1.25, 1.0), dx=1 / 4))
    assert torch.equal(swapped.rel_l2, batched.rel_l2[:1])
    assert not torch.equal(swapped.heatflux_pred, batched.heatflux_pred[:1]) and not torch.equal(swapped.heatflux_target, batched.heatflux_target[:1])
    kl = batched.heatflux_kl()
    assert kl.shape == (3,)
    print("per-trajectory heat-flux KL of the sample rollouts:", [f"{v:.4f}" for v in kl.tolist()], "pooled", f"{float(batched.heatflux_kl(pooled=True)):.4f}")


def test_kde_kl_matches_the_notebook():
    """Allowance for the divergence: (max(n, m) + 4096) * 2^-53 * (A + 2), A = the integral of |integrand|.  To first order |df| <= e |f| + 2 e p
    when both densities carry relative error e, and a density integrates to at most 1; e bounds one density value: a sum of <= n non-negative
    fp64 terms in any order (n * 2^-53), each an exp good to a few ulp of an argument (magnitude <= 745) a few ulp off (inside 4096 * 2^-53).
    Densities: rtol 1e-9 where the golden density exceeds 1e-250 (chosen: six orders above fp64 noise, four below the smallest formula slip
    worth catching).  The returned kl against Simpson's rule on the returned arrays: points * 2^-53 * A."""
    from bubbleformer_amd.utils import kde_kl_divergence
    z = _golden()
    for case in H.KL_CASES:
        n = case["name"]
        sim, model = H.kl_sets(case, int(z[f"seed/{n}"]))
        want, A = float(z[f"kl/{n}"]), float(z[f"A/{n}"])
        kl, x, p, q = kde_kl_divergence(torch.from_numpy(sim).cuda(), torch.from_numpy(model).cuda(), points=case["points"], return_pdfs=True)
        assert kl.dim() == 0 and kl.dtype == torch.float64 and x.shape == p.shape == q.shape == (case["points"],)
        allow = (max(case["n"], case["m"]) + 4096) * U * (A + 2)
        print(f"{n}: KL {float(kl):.12f} (notebook {want:.12f}), off by {abs(float(kl) - want):.2e} = {abs(float(kl) - want) / allow:.4f} of the allowance {allow:.2e}")
        assert abs(float(kl) - want) <= allow
        x_, p_, q_ = x.cpu().numpy(), p.cpu().numpy(), q.cpu().numpy()
        ref_x = z[f"x/{n}"]                                                          # i * step + lo: one rounding each, of numbers no larger than the grid's ends
        assert np.abs(x_ - ref_x).max() <= 4 * U * max(abs(ref_x[0]), abs(ref_x[-1])) and x_[0] == ref_x[0] and x_[-1] == ref_x[-1]
        print(f"  grid: {int((x_ != ref_x).sum())} of {case['points']} points differ from np.linspace's bits, by at most {np.abs(x_ - ref_x).max():.1e}")
        for name, got, ref in (("sim", p_, z[f"pdf_sim/{n}"]), ("model", q_, z[f"pdf_model/{n}"])):
            big = ref > 1e-250
            worst = np.max(np.abs(got - ref)[big] / ref[big])
            print(f"  {name} density: worst relative error {worst:.2e} over {int(big.sum())} points (bound 1e-9), exact zeros {int((got == 0).sum())} / {int((ref == 0).sum())}")
            assert worst <= 1e-9 and np.array_equal(got == 0, ref == 0)
        host = H.simpson_uniform(H.kl_integrand(p_, q_), (x_[-1] - x_[0]) / (case["points"] - 1))
        assert abs(float(kl) - host) <= case["points"] * U * A, (float(kl), host)
        assert torch.equal(kl, kde_kl_divergence(torch.from_numpy(sim).cuda(), torch.from_numpy(model).cuda(), points=case["points"]))      # two calls, the same bits
    assert int((z["pdf_model/exact_zero"] == 0).sum()) > 100


def test_kde_kl_inputs_batches_graphs_and_edges():
    from bubbleformer_amd import _lib
    from bubbleformer_amd.utils import kde_kl_divergence
    case = H.KL_CASES[0]
    sets = [H.kl_sets(case, seed) for seed in (11, 12, 13)]
    p = torch.from_numpy(np.stack([s for s, _ in sets])).cuda()
    q = torch.from_numpy(np.stack([m for _, m in sets])).cuda()
    # fp32 input is converted to fp64: equal to the same values passed as fp64
    assert torch.equal(kde_kl_divergence(p[0].float(), q[0].float()), kde_kl_divergence(p[0].float().double(), q[0].float().double()))
    # three rows at once: each equal to the row alone, densities included
    kl, x, dp, dq = kde_kl_divergence(p, q, return_pdfs=True)
    assert kl.shape == (3,) and x.shape == (3, 1000)
    for r in range(3):
        one = kde_kl_divergence(p[r], q[r], return_pdfs=True)
        for got, alone in zip((kl[r], x[r], dp[r], dq[r]), one):
            assert torch.equal(got, alone), r
    assert len({float(v) for v in kl}) == 3
    # an even number of grid points takes the last-interval rule
    even = kde_kl_divergence(p[0], q[0], points=400, return_pdfs=True)
    host = H.simpson_uniform(H.kl_integrand(even[2].cpu().numpy(), even[3].cpu().numpy()), float(even[1][-1] - even[1][0]) / 399)
    want, _, _, _, A = H.kde_kl(sets[0][0], sets[0][1], 400)
    assert abs(float(even[0]) - host) <= 400 * U * A and abs(float(even[0]) - want) <= (800 + 4096) * U * (A + 2)
    # captured in a graph and replayed
    eager = kde_kl_divergence(p, q)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        kde_kl_divergence(p, q)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = kde_kl_divergence(p, q)
    for _ in range(2):
        out.fill_(-1.0)
        graph.replay()
        assert torch.equal(out, eager)
    # a set without variance has no bandwidth: NaN (scipy raises)
    flat = torch.full((800,), 3.0, dtype=torch.float64, device="cuda")
    assert bool(torch.isnan(kde_kl_divergence(flat, q[0]))) and bool(torch.isnan(kde_kl_divergence(p[0], flat)))
    assert bool(torch.isfinite(kde_kl_divergence(p[0], q[0])))
    # two sets 60 apart: the notebook's expression is NaN (0 * -inf); here the integrand is 0 where the simulated density is
    rs = np.random.RandomState(5)
    a, b = rs.standard_normal(300), rs.standard_normal(200) + 60.0
    want, _, wp, wq, A = H.kde_kl(a, b, 500)
    got, _, gp, gq = kde_kl_divergence(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), points=500, return_pdfs=True)
    assert (wp == 0).any() and bool((gp == 0).any())
    print(f"60 apart: KL {float(got):.6f} against the restatement's {want:.6f}, off by {abs(float(got) - want):.2e} of {(300 + 4096) * U * (A + 2):.2e}")
    assert np.isfinite(float(got)) and abs(float(got) - want) <= (300 + 4096) * U * (A + 2)
    # refusals on the host
    for bad in ((p[0, :1], q[0]), (p[0], q[0, :1])):
        with pytest.raises(ValueError):
            kde_kl_divergence(*bad)
    with pytest.raises(ValueError):
        kde_kl_divergence(p[0], q[0], points=2)
    with pytest.raises(ValueError):
        kde_kl_divergence(p, q[:2])
    with pytest.raises(_lib.BubbleformerHipError):
        kde_kl_divergence(p[0].cpu(), q[0].cpu())
