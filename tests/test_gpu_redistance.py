"""Redistancing on the GPU (csrc/redistance.hip) against the numpy fp64 restatement tests/redistance_restatement.py: every test field at the edge
shapes and on both sides of the LDS / workspace threshold, the status values, the invariants, and `evaluate_rollouts_redistanced(..., RedistanceSpec())`
against `redistance` of the model's own outputs.

Tolerance against fp64: 8 * 2^-24 * (H + W) * max(d_max, h) absolute per cell -- a handful of correctly rounded fp32 operations per update (fast-math,
contraction and the approximate divide are off for this kernel), carried along a dependency chain of at most H + W cells; interface cells, which
have no chain, 16 * 2^-24 * h.  A wrong neighbour, a missed cell or an early stop is at least 1e-3 h away.

The pass count is compared with the red-black restatement run in the kernel's own fp32 operations: whether a pass "changed a cell" can hinge on
a last-place difference between two upwind paths, which fp64 and fp32 resolve differently (on the CPU: 26 fp64 against 24 fp32 passes on the
64 x 64 disc, 10 against 9 on the banded 48 x 40 disc), so the fp64 count is asserted only on the corner field, whose single source leaves no
such ties, and printed elsewhere."""
import functools

import numpy as np
import pytest
import torch

from tests import redistance_restatement as R

pytestmark = pytest.mark.gpu
H0 = 1.0 / 32
SHAPES = [(48, 40), (33, 7), (1, 37), (37, 1), (2, 2)]


def _run(phi, band=None, max_rounds=None, dx=H0):
    """One call on a numpy (H, W) or (F, H, W) field -> (out, rounds, change_rms) as numpy."""
    from bubbleformer_amd.utils import redistance
    out, rounds, change = redistance(torch.from_numpy(np.ascontiguousarray(phi, dtype=np.float32)).cuda(), dx, band, max_rounds, return_status=True)
    return out.cpu().numpy(), rounds.cpu().numpy(), change.cpu().numpy()


def _check(name, phi, band, got, rounds, change):
    """The result of one frame against the restatement; returns the worst gaps as fractions of their bounds."""
    H, W = phi.shape
    want, passes = R.redistance_rb(phi, H0, band)
    want32, passes32 = R.redistance_rb(phi, H0, band, dtype=np.float32)
    assert int(rounds) == passes32, (name, band, int(rounds), passes32, passes)
    if passes <= 0:
        assert np.array_equal(got, phi) and float(change) == 0.0
        return 0.0, 0.0, passes, passes32
    tol = 8 * 2.0 ** -24 * (H + W) * max(float(np.abs(want).max()), H0)
    gap = np.abs(got.astype(np.float64) - want)
    iface = R.interface_cells(phi)
    assert gap.max() <= tol, (name, band, float(gap.max()), tol)
    assert gap[iface].max() <= 16 * 2.0 ** -24 * H0, (name, band, float(gap[iface].max()))
    assert np.array_equal(np.signbit(got), ~R.vapour(phi)), name
    assert np.array_equal(R.interface_cells(np.where(np.signbit(got), -1.0, 1.0)), iface), name
    rms = R.change_rms(got, phi)
    assert abs(float(change) - rms) <= 1e-6 * rms, (name, float(change), rms)
    if not np.array_equal(got, want32):
        print(f"    {name} band {band}: {int((got != want32).sum())} cells differ from the fp32 restatement's bits")
    return float(gap.max() / tol), float(gap[iface].max() / (16 * 2.0 ** -24 * H0)), passes, passes32


@pytest.mark.parametrize("band", [None, 8 * H0])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_field_against_the_restatement(shape, band):
    H, W = shape
    fields = R.fields(H, W, H0)
    got, rounds, change = _run(np.stack(list(fields.values())), band)
    for k, (name, phi) in enumerate(fields.items()):
        cell, iface, p64, p32 = _check(name, phi, band, got[k], rounds[k], change[k])
        print(f"  {H}x{W} {name} band {band}: worst gap {cell:.3f} of the bound, interface {iface:.3f} of its bound, passes {int(rounds[k])} (fp64 restatement {p64})")
        if name == "corner":
            assert int(rounds[k]) == p64


def test_both_sides_of_the_lds_threshold():
    """The largest square frame whose distances live in LDS and the smallest that takes the workspace: the corner field (the longest chain, and
    the worst pass count: (H + W) / 2) and the two-disc field."""
    from bubbleformer_amd import ops
    cells = ops.redistance_lds_cells()
    side = int(np.sqrt(cells))
    assert side * side <= cells < (side + 1) * (side + 1)
    for n in (side, side + 1):
        frames = {"corner": R.corner(n, n, H0).astype(np.float32), "two_discs": R.distort(R.circles(n, n, H0, R.two_discs(n, n, H0))).astype(np.float32)}
        got, rounds, change = _run(np.stack(list(frames.values())))
        for k, (name, phi) in enumerate(frames.items()):
            cell, iface, p64, p32 = _check(name, phi, None, got[k], rounds[k], change[k])
            print(f"  {n}x{n} ({'LDS' if n * n <= cells else 'workspace'}) {name}: worst gap {cell:.3f} of the bound, interface {iface:.3f}, passes {int(rounds[k])} (fp64 {p64})")
        assert int(rounds[0]) == n == R.redistance_rb(frames["corner"], H0)[1]


def test_status_values():
    H, W = 48, 40
    one = np.full((H, W), -0.3, np.float32)
    one[3, 5] = 0.0                                                         # an exact zero is liquid too
    out, rounds, change = _run(one)
    assert int(rounds) == 0 and np.array_equal(out, one) and float(change) == 0.0
    for bad in (np.nan, np.inf):
        phi = R.fields(H, W, H0)["disc"].copy()
        phi[17, 23] = bad
        out, rounds, change = _run(phi)
        assert int(rounds) == -1 and np.array_equal(out.view(np.uint32), phi.view(np.uint32)) and float(change) == 0.0
    corner = R.corner(H, W, H0).astype(np.float32)
    out, rounds, change = _run(corner, max_rounds=3)
    want, passes = R.redistance_rb(corner, H0, None, 3)                     # the same visiting order: the values three passes reach
    assert int(rounds) == -2 == passes and np.isfinite(out).all()
    assert np.abs(out - want).max() <= 8 * 2.0 ** -24 * (H + W) * float(np.abs(want).max())
    assert out[-1, -1] == -(H + W) * H0
    out, rounds, _ = _run(corner, band=2 * H0, max_rounds=1)               # the cap reaches every cell in the first pass, which is not quiet
    assert int(rounds) == -2 and out[-1, -1] == -2 * H0
    out, rounds, _ = _run(corner, max_rounds=(H + W) // 2)
    assert int(rounds) == (H + W) // 2                                      # exactly enough passes: the last one is the quiet one


def test_same_bits_in_place_twice_and_alone():
    from bubbleformer_amd import ops
    from bubbleformer_amd.utils import redistance
    H, W = 48, 40
    fields = R.fields(H, W, H0)
    batch = torch.from_numpy(np.stack(list(fields.values()))).cuda()
    first, rounds, change = redistance(batch, return_status=True)
    again, rounds2, change2 = redistance(batch, return_status=True)
    assert torch.equal(first, again) and torch.equal(rounds, rounds2) and torch.equal(change, change2)
    for k in range(batch.shape[0]):
        alone, r1, c1 = redistance(batch[k], return_status=True)
        assert alone.shape == (H, W) and r1.shape == () and torch.equal(alone, first[k]) and int(r1) == int(rounds[k]) and float(c1) == float(change[k])
    aliased = batch.clone()
    ret = redistance(aliased, out=aliased)
    assert ret is aliased and torch.equal(aliased, first)
    lead = redistance(batch.view(1, 5, 1, H, W))
    assert lead.shape == (1, 5, 1, H, W) and torch.equal(lead.view(5, H, W), first)
    strided = redistance(batch.transpose(1, 2))                             # the wrapper makes its own contiguous copy
    assert strided.shape == (5, W, H)
    n = int(np.sqrt(ops.redistance_lds_cells())) + 1
    big = torch.from_numpy(np.stack([R.distort(R.circles(n, n, H0, R.two_discs(n, n, H0))), R.walls(n, n, H0)]).astype(np.float32)).cuda()
    a, b = redistance(big), redistance(big)
    assert torch.equal(a, b) and torch.equal(redistance(big[1]), a[1])      # the workspace path likewise


def test_refusals():
    from bubbleformer_amd import _lib, ops
    from bubbleformer_amd.utils import redistance
    phi = torch.zeros(2, 8, 8, device="cuda")
    ws = ops.redistance_workspace(2, 8, 8, "cuda")
    out = torch.empty_like(phi)
    E = _lib.BubbleformerHipError
    with pytest.raises(E):
        ops.redistance(phi.transpose(1, 2), H0, None, None, ws, out)
    with pytest.raises(E):
        ops.redistance(phi.double(), H0, None, None, ws, out)
    with pytest.raises(E):
        ops.redistance(phi.cpu(), H0, None, None, ws, out)
    with pytest.raises(E):
        ops.redistance(phi, H0, None, None, ws, out.double())
    with pytest.raises(E):
        ops.redistance(phi, H0, None, None, ws, out, rounds=torch.empty(2, device="cuda"))
    with pytest.raises(E):
        ops.redistance(phi, H0, None, None, ws[:8], out)
    with pytest.raises(E):
        redistance(phi.double())
    with pytest.raises(E):
        redistance(phi.cpu())
    with pytest.raises(E):
        redistance(phi, out=out.transpose(1, 2))
    n = int(np.sqrt(ops.redistance_lds_cells())) + 1
    with pytest.raises(E):
        ops.redistance(torch.zeros(1, n, n, device="cuda"), H0, None, None, ws, torch.zeros(1, n, n, device="cuda"))     # the LDS-sized workspace


# ---------------------------------------------------------------------------- evaluate_rollouts_redistanced
START, STEPS, T, DX = 7, 3, 4, 1.0 / 32                                      # the spacing the Eikonal rows use


def _tensors(r):
    from tests.test_gpu_heatflux_eval import _tensors as base
    out = base(r)
    if r.redistance_rounds is not None:
        out["redistance_rounds"], out["redistance_change"] = r.redistance_rounds, r.redistance_change
    return out


@functools.lru_cache(maxsize=None)
def _reports():
    """The tiny rollout of test_gpu_heatflux_eval (avit, 32 x 32 after downsampling by 2, norm="std", three steps of four frames): plain, and with
    redistancing in a graph, eagerly and on every second step."""
    from bubbleformer_amd.utils import RedistanceSpec
    from bubbleformer_amd.utils.rollout import evaluate_rollouts_redistanced
    from tests.test_gpu_heatflux_eval import _tiny_model, _tiny_reports
    store, _, _, _, plain = _tiny_reports()
    model = _tiny_model()
    kw = dict(keep_predictions=True)
    spec = RedistanceSpec(dx=DX)
    graph = evaluate_rollouts_redistanced(model, store, [START], STEPS, spec, use_graph=True, **kw)
    eager = evaluate_rollouts_redistanced(model, store, [START], STEPS, spec, use_graph=False, **kw)
    second = evaluate_rollouts_redistanced(model, store, [START], STEPS, RedistanceSpec(dx=DX, every=2, band=4 * DX), use_graph=True, **kw)
    none = evaluate_rollouts_redistanced(model, store, [START], STEPS, None, use_graph=True, **kw)
    return store, model, plain, none, graph, eager, second


def test_none_changes_nothing_and_graph_equals_eager():
    store, model, plain, none, graph, eager, second = _reports()
    a, b = _tensors(plain), _tensors(none)
    assert sorted(a) == sorted(b) and len(a) == 6 and none.redistance_rounds is None and none.redistance_change is None
    for k in a:
        assert torch.equal(a[k], b[k]), k
    g, e = _tensors(graph), _tensors(eager)
    assert sorted(g) == sorted(e) and len(g) == 8
    for k in g:
        assert torch.equal(g[k], e[k]), k
    assert graph.redistance_rounds.shape == (1, STEPS * T) and graph.redistance_rounds.dtype == torch.int32
    assert graph.redistance_change.shape == (1, STEPS * T) and graph.redistance_change.dtype == torch.float32
    assert int(graph.redistance_rounds.min()) >= 1 and float(graph.redistance_change.min()) > 0.0
    assert not torch.equal(graph.predictions, plain.predictions)
    print("passes per frame", graph.redistance_rounds[0].tolist(), "rms change", [round(v, 4) for v in graph.redistance_change[0].tolist()])


@pytest.mark.parametrize("which", ["every_step", "every_second_step"])
def test_the_archive_is_the_redistanced_model_output(which):
    """Step s of the archive: the model's output on the previous archive clip (the gathered input for s = 0), its sdf channel de-normalised,
    redistanced and renormalised on the steps the spec names -- bit for bit, all channels."""
    from bubbleformer_amd.utils import redistance
    store, model, plain, none, graph, eager, second = _reports()
    report, every, band = (graph, 1, None) if which == "every_step" else (second, 2, 4 * DX)
    _, diff, div = store.out_tab
    sdf = report.fields.index("dfun")
    clip = store.gather([START])[0]
    for s in range(STEPS):
        rows = slice(s * T, (s + 1) * T)
        with torch.no_grad():
            out = model(clip).float().contiguous()
        want = out.clone()
        if (s + 1) % every == 0:
            phys = out[:, :, sdf] * div[sdf] + diff[sdf]                     # fp32 multiply, then add
            d, rounds, change = redistance(phys.contiguous(), DX, band, return_status=True)
            assert int(rounds.min()) >= 1
            want[:, :, sdf] = (d - diff[sdf]) / div[sdf]
            assert torch.equal(report.redistance_rounds[:, rows], rounds) and torch.equal(report.redistance_change[:, rows], change)
            assert not torch.equal(want[:, :, sdf], out[:, :, sdf])
        else:
            assert int(report.redistance_rounds[:, rows].abs().max()) == 0 and float(report.redistance_change[:, rows].abs().max()) == 0.0
        got = report.predictions[:, rows]
        for c in range(want.shape[2]):
            assert torch.equal(got[:, :, c], want[:, :, c]), (s, report.fields[c])
        clip = got.contiguous()


def test_the_scores_see_the_corrected_prediction():
    """eikonal_pred is bf_rollout_score's own evaluation of the score, eikonal_l1_per_frame is bf_eikonal_l1_frames': two kernels, not the same
    bits.  2e-6 relative is the figure the existing tests hold this pair to (tests/test_rollout_physics.py, test_scoring_kernel_against_fp64)."""
    from bubbleformer_amd.utils import physics
    store, model, plain, none, graph, eager, second = _reports()
    _, diff, div = store.out_tab
    sdf = graph.fields.index("dfun")
    phys = (graph.predictions[0, :, sdf] * div[sdf] + diff[sdf]).contiguous()
    want = physics.eikonal_l1_per_frame(phys)
    gap = ((graph.eikonal_pred[0] - want).abs() / want.abs()).max()
    print(f"eikonal_pred against eikonal_l1_per_frame of the corrected archive: {float(gap):.2e} relative; "
          f"uncorrected {plain.eikonal_pred[0].tolist()[:4]} -> corrected {graph.eikonal_pred[0].tolist()[:4]}")
    assert torch.allclose(graph.eikonal_pred[0], want, rtol=2e-6, atol=0)    # test_scoring_kernel_against_fp64's figure for this score
    assert torch.equal(graph.eikonal_target, plain.eikonal_target)


def test_with_bubbles_and_an_ensemble():
    from bubbleformer_amd.utils import BubbleSpec, EnsembleSpec, RedistanceSpec, bubble_census
    from bubbleformer_amd.utils.rollout import evaluate_rollouts_redistanced
    store, model = _reports()[:2]
    spec = BubbleSpec(max_bubbles=24, dx=1 / 2)
    M = 2
    rep = evaluate_rollouts_redistanced(model, store, [START, 20], 2, RedistanceSpec(dx=DX), keep_predictions=True, bubbles=spec,
                                        ensemble=EnsembleSpec(M, 0.05, seed=7))
    assert rep.redistance_rounds.shape == (M * 2, 2 * T) and int(rep.redistance_rounds.min()) >= 1
    assert rep.by_member(rep.redistance_rounds).shape == (M, 2, 2 * T) and rep.ensemble_spread.shape[0] == 2
    _, diff, div = store.out_tab
    sdf = rep.fields.index("dfun")
    phys = rep.predictions[:, :, sdf] * div[sdf] + diff[sdf]
    want = bubble_census(phys.contiguous(), connectivity=4, max_bubbles=24)
    assert torch.equal(rep.bubble_count_pred, want.count) and torch.equal(rep.bubble_attached_pred, want.attached)
    assert torch.equal(rep.bubble_area_pred, want.area) and torch.equal(rep.vapour_fraction_pred, want.vapour_fraction())


def test_a_dataset_without_the_field_is_refused():
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.utils import RedistanceSpec
    from bubbleformer_amd.utils.rollout import evaluate_rollouts_redistanced
    from tests.test_gpu_render import FIELDS
    from tests.test_rollout_eval import FILES
    from bubbleformer_amd.models import get_model
    nosdf = BubbleForecast(FILES[1:], input_fields=FIELDS[1:], output_fields=FIELDS[1:], norm="std", downsample_factor=2, time_window=4, start_time=5)
    nosdf.normalize()
    model = get_model("avit", time_window=4, drop_path=0.0, input_fields=3, output_fields=3, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=2).cuda().eval()
    with pytest.raises(ValueError):
        evaluate_rollouts_redistanced(model, nosdf.device_store("cuda"), [3], 1, RedistanceSpec())
