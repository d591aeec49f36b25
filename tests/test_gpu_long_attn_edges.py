"""Long-axis attention (33 <= L <= 128: csrc/attn_long.hip) through the C ABI, every output held per element to the fp64 reference and
the derived bound of tests/attn_bounds.py (modes LONG_BF16 / LONG_FP32).  The harness is test_gpu_attn_edges.py's `Call`: outputs written
with accumulate = 0 start as NaN; every token buffer carries sentinel tokens, every parameter-gradient buffer and the workspace sentinel
floats, that must come back bit-unchanged; the inputs must come back bit-unchanged too.  out_scale is passed as the fp32 value the kernel
receives (0.37 is not a power of two: the staged dO out_scale is then a rounded operand).

Which case reaches which branch of attn_long.hip:

  test_every_instantiation      GO(NA) for NA = 3 .. 8 in both dtypes, L on both sides of every multiple of 16 (LP and NA change), the four
                                geometries in turn, a full workspace (attn_long_ws_reduce) alternating with ws = NULL (atomics).
  test_head_dim_edges           d below one 16-column slice (8; 4, 12 in fp32), 8- and 4-wide tail slices (24, 40, 72, 120; 12, 20), whole
                                slices, at L = 40 (d > LP from 72 on) and L = 100 (d < LP up to 72); d = LP and d = LP + chunk, where the
                                backward's plane pitch goes from LDM to d + 1; L = d = 128, the largest LDS plan; L = 80 at d = 64 / 128 (the
                                backward's dynamic LDS crosses 64 KB only for d > LP) and L = 96 / 112 (the forward's crosses it).
  test_heads                    1, 3 and 16 heads, 16 with emb and demb (a_emb's pitch of 16) at the smallest d.
  test_parameter_variants       emb / hscale absent and present (dhscale is passed without hscale and must stay zero), out_scale 0.5, 1.0
                                and 0.37, accumulate 1 in the forward and the backward on prefilled buffers.
  test_raw_pair_of_passes       accumulate 2 then 5 (forward 0 then 1) against the fp64 axial pair with the long axis on H, on W and on both;
                                the short pass of a mixed pair runs in attn_mfma.hip and is held to the short mode's bound.
  test_raw_modes_refused        2 and 5 in fp32 and at d % 32 != 0: an error, nothing written.
  test_forward_persistent       more than 2048 problems: the forward's grid cap, every workgroup's second problem.
  test_backward_persistent      700 problems (512 workgroups, a ragged second round) and 1104 (some workgroups take three), both dtypes,
                                through workspace rows and through atomics.
  test_workspace_variants       full rows, k = 1 and 3 rows (k workgroups loop over all problems), a workspace smaller than one row (the
                                fallback to atomics) and ws = NULL: out / dqkv bit-identical across all, parameter sums within
                                param_total's reordering allowance of each other and within their bounds, the workspace paths bit-identical
                                run to run.  The workspace is NaN-filled beforehand.
  test_hard_inputs              the short suite's peaked (scores +-30) and offset (rows 48 .. 150) inputs at L = 100 and 128.
  test_refusals                 L = 129, d = 136, 17 heads, d off the 16-byte chunk: check_geo returns before any launch; nothing written.
  test_zz_worst_ratios          prints the worst |got - ref| / bnd per (mode, output) seen so far (pytest -s); complete only when the whole
                                file runs in one process, in file order.
"""
import collections

import numpy as np
import pytest
import torch

from tests import attn_bounds as AB
from tests.test_gpu_attn_edges import AX_NAMES, Call, plain_outputs, same_bits

pytestmark = pytest.mark.gpu

WORST = collections.defaultdict(float)  # (mode, output) -> worst ratio seen
BF16, FP32 = torch.bfloat16, torch.float32
DT = pytest.mark.parametrize("dtype", [BF16, FP32], ids=["bf16", "fp32"])
FULL = 512                              # workspace rows: LONG_BWD_GRID, one per workgroup whatever the problem count


def f32(x):
    return float(np.float32(x))


def mode_of(dtype):
    return AB.LONG_BF16 if dtype == BF16 else AB.LONG_FP32


def hold(res, got, tag, what):
    """Every output of `res` ({name: (ref, bnd)}) against got[name]; records the worst ratios."""
    for k, (ref, bnd) in res.items():
        names = {4: ("sequence", "head", "row", "channel"), 3: ("token", "head", "channel"), 2: ("bucket", "head"), 1: ("index",)}[ref.dim()]
        w = AB.check(got[k], ref, bnd, f"{what}: {k}", names)
        key = (tag, "dhscale" if k.startswith("dhscale") else k)
        WORST[key] = max(WORST[key], w)
        print(f"{what} [{tag}] {k}: worst ratio {w:.3g}")


def run_long(L, d, heads, geo, N, dtype, with_emb=True, with_hs=True, out_scale=0.5, seed=0, ws_rows=FULL, kind="plain", accumulate=False,
             with_bwd=True):
    assert geo[1] == L and L > 32
    c = Call(N, heads, d, dtype, seed, kind)
    old_o, old_d = c.prefill(seed + 1) if accumulate else (None, None)
    os_ = f32(out_scale)
    c.fwd(geo, with_emb, with_hs, os_, int(accumulate))
    if with_bwd:
        c.bwd(geo, with_emb, with_hs, os_, int(accumulate), ws_rows=ws_rows)
    c.untouched()
    c.reorder = {}
    res = AB.plain(c.qkv[:N], c.dout[:N] if with_bwd else None, geo, heads, d, c.prm, with_emb, with_hs, os_, mode_of(dtype),
                   None if old_o is None else old_o[:N], None if old_d is None else old_d[:N], c.reorder)
    hold(res, plain_outputs(c, geo, with_bwd), "long bf16" if dtype == BF16 else "long fp32", f"L={L} d={d} heads={heads}")
    if with_bwd and not with_hs:
        assert float(c.grads[5].abs().max()) == 0.0, "dhscale without hscale must stay zero"
    return c


def small_geo(kind, L):
    """six sequences (four contiguous ones): with 2 heads at most 12 problems"""
    return AB.geometry(kind, L, n_outer=2, inner=3)


KINDS = ("contig", "temporal", "W", "H")
EVERY_L = (33, 47, 48, 49, 63, 64, 65, 80, 81, 96, 97, 111, 112, 113, 127, 128)


@DT
@pytest.mark.parametrize("i", range(len(EVERY_L)), ids=[f"L{L}" for L in EVERY_L])
def test_every_instantiation(i, dtype):
    L = EVERY_L[i]
    geo, N = small_geo(KINDS[i % 4], L)
    run_long(L, 64, 2, geo, N, dtype, i % 5 != 1, i % 3 != 2, (0.5, 1.0, 0.37)[i % 3], 2000 + i, ws_rows=None if i % 2 else FULL)


HEAD_DIMS = [(BF16, d, L) for d in (8, 24, 32, 40, 72, 120, 128) for L in (40, 100)] + [(FP32, d, L) for d in (4, 12, 20, 64, 128) for L in (40, 100)]
HEAD_DIMS += [(t, d, L) for t in (BF16, FP32) for d, L in ((64, 64), (72, 64), (128, 128), (64, 80), (128, 80), (64, 96), (64, 112))]
HEAD_DIMS += [(FP32, 68, 64)]           # d = LP + the fp32 chunk


@pytest.mark.parametrize("dtype,d,L", HEAD_DIMS, ids=[f"{'bf16' if t == BF16 else 'fp32'}-d{d}-L{L}" for t, d, L in HEAD_DIMS])
def test_head_dim_edges(dtype, d, L):
    geo, N = small_geo(KINDS[(d // 4 + L) % 4], L)
    run_long(L, d, 2, geo, N, dtype, True, True, 0.37 if d % 16 else 0.5, 2100 + d + L, ws_rows=FULL if (d // 8) % 2 else None)


@DT
@pytest.mark.parametrize("heads,L", [(1, 40), (3, 50), (16, 33), (16, 113)])
def test_heads(heads, L, dtype):
    d = (8 if dtype == BF16 else 4) if heads == 16 else 32
    nseq = 2 if heads == 16 else 4
    run_long(L, d, heads, (nseq, L, 1, L, 0, 1), nseq * L, dtype, True, True, 0.5, 2200 + heads + L, ws_rows=FULL if L == 33 else None)


VARIANTS = [  # emb, hscale, out_scale, accumulate
    (False, False, 1.0, False), (True, False, 0.37, False), (False, True, 0.5, False), (True, True, 0.37, True), (False, False, 0.37, True),
    (True, True, 1.0, True),
]


@DT
@pytest.mark.parametrize("i", range(len(VARIANTS)))
def test_parameter_variants(i, dtype):
    with_emb, with_hs, out_scale, acc = VARIANTS[i]
    L, d = (49, 72, 100)[i % 3], (32, 24)[i % 2] if dtype == BF16 else (32, 20)[i % 2]
    geo, N = small_geo(KINDS[(i + 1) % 4], L)
    run_long(L, d, 2, geo, N, dtype, with_emb, with_hs, out_scale, 2300 + i, ws_rows=None if i % 2 else FULL, accumulate=acc)


def pair_modes(h, w):
    return (AB.LONG_BF16 if w > 32 else AB.MFMA, AB.LONG_BF16 if h > 32 else AB.MFMA)


@pytest.mark.parametrize("h,w,d,heads", [(40, 12, 32, 2), (12, 64, 64, 2), (33, 48, 128, 1), (40, 12, 128, 1), (12, 64, 32, 2), (33, 48, 64, 2)])
def test_raw_pair_of_passes(h, w, d, heads):
    """Forward accumulate 0 then 1, backward accumulate 2 then 5, against the fp64 gradient of the sum of both passes through the shared
    q / k LayerNorm.  (40, 12): the long axis is H, the W pass runs in attn_mfma.hip; (12, 64): the reverse; (33, 48): both long."""
    Fr = 1
    c = Call(Fr * h * w, heads, d, BF16, 2400 + h + w + d, nhs=2)
    gW, gH = AB.axial_geos(Fr, h, w)
    c.fwd(gW, acc=0, hs_i=0)
    c.fwd(gH, acc=1, hs_i=1)
    c.bwd(gW, acc=2, hs_i=0, ws_rows=FULL)
    c.bwd(gH, acc=5, hs_i=1, ws_rows=None)
    c.untouched()
    N = c.N
    res = AB.axial_pair(c.qkv[:N], c.dout[:N], Fr, h, w, heads, d, c.prm, pair_modes(h, w))
    got = {"out": c.out[:N].view(N, heads, d), **{n: c.dqkv[:N].view(N, heads, 3, d)[:, :, i] for i, n in enumerate(("dq", "dk", "dv"))}}
    got.update(dict(zip(AX_NAMES, c.grads)))
    hold(res, got, "long bf16 pair" if min(h, w) > 32 else "long + short pair", f"axial pair {h}x{w} d={d}")


def refused(c, geo, acc=0, fwd=True, heads=None, d=None):
    """The entry points return an error for these arguments before any launch (check_geo / BF_REQUIRE in attn.hip) and write nothing."""
    from bubbleformer_amd import _lib as L
    from bubbleformer_amd.ops import _dt, _p, _stream
    heads, d = heads or c.heads, d or c.d
    par = [_p(t) for t in c.prm[:6]]
    if fwd:
        assert L.lib().bf_attn_fwd(_dt(c.dtype), _p(c.qkv), _p(c.out), *geo, heads, d, *par, 0.5, 0, _stream()) != 0
    assert L.lib().bf_attn_bwd(_dt(c.dtype), _p(c.qkv), _p(c.dout), _p(c.dqkv), *geo, heads, d, *par, *[_p(t) for t in c.grads[:6]], 0.5, acc,
                               None, 0, _stream()) != 0
    c.untouched()
    assert torch.isnan(c.out.float()).all() and torch.isnan(c.dqkv.float()).all(), "a refused call wrote an output"
    assert all(float(g.abs().max()) == 0.0 for g in c.grads), "a refused call wrote a parameter gradient"


@pytest.mark.parametrize("dtype,d", [(FP32, 64), (BF16, 40), (BF16, 72)], ids=["fp32-d64", "bf16-d40", "bf16-d72"])
@pytest.mark.parametrize("acc", [2, 5])
def test_raw_modes_refused(dtype, d, acc):
    L = 40
    refused(Call(2 * L, 2, d, dtype, 2500), (2, L, 1, L, 0, 1), acc=acc, fwd=False)


def test_forward_persistent():
    """go_fwd_long launches at most 2048 workgroups: 137 sequences x 16 heads = 2192 problems, 144 workgroups take a second one."""
    L, d, heads, nseq = 33, 8, 16, 137
    assert nseq * heads > 2048
    run_long(L, d, heads, (nseq, L, 1, L, 0, 1), nseq * L, BF16, seed=2600, with_bwd=False)
    run_long(L, 4, heads, (nseq, L, 1, L, 0, 1), nseq * L, FP32, seed=2601, with_bwd=False)


@DT
@pytest.mark.parametrize("nseq,heads,ws_rows", [(100, 7, FULL), (69, 16, None)], ids=["700", "1104"])
def test_backward_persistent(nseq, heads, ws_rows, dtype):
    """LONG_BWD_GRID = 512 workgroups: 700 problems leave 188 workgroups a second one; 1104 give every workgroup two and 80 a third.  What a
    workgroup keeps in LDS between its problems (s_emb, s_stat, the a_ln / a_emb / a_hs sums) is then part of every checked output."""
    L, d = 33, 8
    assert nseq * heads > 512 and (nseq * heads) % 512
    run_long(L, d, heads, (nseq, L, 1, L, 0, 1), nseq * L, dtype, seed=2700 + heads, ws_rows=ws_rows)


@DT
@pytest.mark.parametrize("L,d,heads,nseq", [(40, 32, 3, 4), (81, 24, 2, 5), (33, 8, 16, 40)], ids=["12", "10", "640"])
def test_workspace_variants(L, d, heads, nseq, dtype):
    if dtype == FP32 and d == 24:
        d = 20
    geo, args = (nseq, L, 1, L, 0, 1), dict(seed=2800 + L)
    full = run_long(L, d, heads, geo, nseq * L, dtype, ws_rows=FULL, **args)
    again = run_long(L, d, heads, geo, nseq * L, dtype, ws_rows=FULL, **args)
    runs = {"full again": again}
    for k in (1, 3):
        runs[f"{k} rows"] = run_long(L, d, heads, geo, nseq * L, dtype, ws_rows=k, **args)
    runs["3 rows again"] = run_long(L, d, heads, geo, nseq * L, dtype, ws_rows=3, **args)
    runs["less than a row"] = run_long(L, d, heads, geo, nseq * L, dtype, ws_rows=0, **args)       # a workspace pointer with no room: atomics
    runs["no workspace"] = run_long(L, d, heads, geo, nseq * L, dtype, ws_rows=None, **args)
    for name, c in runs.items():
        assert same_bits(c.out, full.out) and same_bits(c.dqkv, full.dqkv), name
        for n, x, y in zip(AB.NAMES, c.grads, full.grads):
            AB.check(x, y.double(), full.reorder[n], f"{n}: {name} against full rows", ("bucket", "head") if n == "demb" else ("index",))
    for a, b in ((full, again), (runs["3 rows"], runs["3 rows again"])):
        for x, y in zip(a.grads, b.grads):
            assert same_bits(x, y), "parameter gradients through the workspace must not depend on the run"


@DT
@pytest.mark.parametrize("kind", ["peaked", "offset"])
@pytest.mark.parametrize("L,d", [(100, 64), (128, 32)])
def test_hard_inputs(kind, L, d, dtype):
    geo, N = small_geo("temporal", L)
    run_long(L, d, 2, geo, N, dtype, seed=2900 + L, kind=kind)


@DT
@pytest.mark.parametrize("what", ["L129", "d136", "heads17", "chunk"])
def test_refusals(what, dtype):
    L, d, heads = 40, 32, 2
    c = Call(140, 17, 136, dtype, 3000)         # buffers larger than anything the refused arguments describe
    if what == "L129":
        L = 129
    elif what == "d136":
        d = 136
    elif what == "heads17":
        heads = 17
    else:
        d = 36 if dtype == BF16 else 34
    refused(c, (1, L, 1, L, 0, 1), heads=heads, d=d)


def test_zz_worst_ratios():
    """Asserts nothing (every ratio was asserted <= 1 where it was measured): prints the summary DESIGN.md quotes.  It reads what the tests
    above left in WORST, so it is complete only when the whole file runs in one process."""
    for (tag, name), w in sorted(WORST.items()):
        print(f"worst |got - ref| / bnd  {tag:18s} {name:10s} {w:.3g}")
