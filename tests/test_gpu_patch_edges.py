"""GPU: the patch-stage streaming kernels at their edges, every output element held to the per-element bound of tests/patch_bounds.py,
through the C ABI: bf_gather_gemm, bf_gather_gemm_rebuilt, bf_scatter_gemm (+ bf_in_stats_merge_slices on its partials),
bf_gather_wgrad, bf_gather_wgrad_rebuilt, bf_embed_tail_bwd, bf_debed_last, bf_debed_last_bwd, bf_debed_last_bwd_norm, bf_embed_first.

One tile in all; 16-row blocks that wrap image rows; several tiles per wave (the frame count is computed from the device's CU count so
that tiles just exceed one or two full grids, five tiles per frame so that runs straddle frames under clearly different affines);
weight-gradient runs of one, two and three steps and slab counts either side of the reduce kernel's unrolled loop; the last-stage
kernels either side of 16 and 64 groups per frame in every channel count; tail_plan's every tiles-per-wave value and the prime count;
frame counts either side of the 16-deep frame loop; cancelling and badly scaled inputs; refusals that write nothing.  The kernels carry
no per-path profiler names, so each case asserts the path it expects from patch_bounds' restated dispatch arithmetic before it judges
the output.  Operands come from seeded CPU generators, every output buffer has a NaN tail behind it, the fp64 references are computed
on the device.  The last test prints the worst |got - ref| / bound of each area."""
import functools

import pytest
import torch

from bubbleformer_amd import _lib as L
from tests import norm_bounds as NB
from tests import patch_bounds as PB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
TAIL = 64
NAN = float("nan")
C0 = 96
WORST = {}


def _note(area, ratio, case):
    if ratio >= WORST.get(area, (-1.0, ""))[0]:
        WORST[area] = (ratio, case)


def _randn(*shape, scale=1.0, shift=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=F32) * scale + shift


def _rand(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=F32)


def _dev(t, dt=None):
    return None if t is None else (t if dt is None else t.to(dt)).to(DEV).contiguous()


def _buf(shape, dt=F32, init=None):
    """-> (view of `shape`, whole buffer): NaN (or `init`) followed by a NaN tail no kernel may touch."""
    n = 1
    for s in shape:
        n *= s
    b = torch.full((n + TAIL,), NAN, dtype=dt, device=DEV)
    if init is not None:
        b[:n] = init.reshape(-1).to(dt).to(DEV)
    return b[:n].view(shape), b


def _tail(b, what):
    torch.cuda.synchronize()
    assert torch.isnan(b[-TAIL:].float()).all(), (what, "wrote past its extent")


def _untouched(b, what):
    torch.cuda.synchronize()
    assert torch.isnan(b.float()).all(), (what, "a refused call wrote")


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _tables(Fr, C, seed):
    """Every frame its own affine, far from its neighbours'."""
    return 0.5 + _rand(Fr, C, seed=seed), _randn(Fr, C, scale=0.3, seed=seed + 1)


@functools.lru_cache(maxsize=2)
def _big_map(Fr, gh, gw, seed):
    return _dev(_randn(Fr, 2 * gh, 2 * gw, C0, seed=seed), BF16)


def _frames_for(rounds, tpf):
    """The frame count at which tiles = F * tpf just exceeds `rounds - 1` full grids of 2 * CUs * 4 waves."""
    return (rounds - 1) * 2 * _cus() * PB.GW // tpf + 2 if rounds > 1 else None


def _assert_split(Fr, gh, gw, rounds, straddle):
    tiles, tpf = Fr * gh * gw // 32, gh * gw // 32
    got = PB.wave_split(tiles, _cus())
    assert got[0] == rounds, (tiles, _cus(), got)
    runs = [r for r in PB.wave_runs(tiles, _cus()) if r[1] > r[0]]
    assert max(e - b for b, e in runs) == rounds
    if rounds == 1:
        assert got[1] == tiles                                   # fewer tiles than a full grid's waves: one wave per tile
    if straddle:
        assert any(e - b >= 2 and b // tpf != (e - 1) // tpf for b, e in runs), "no run holds two tiles of different frames"


# ---------------------------------------------------------------------------------------------------- gather GEMM
def run_gather(Fr, gh, gw, form, w_kn, rounds=1, straddle=False, hard=None, seed=0):
    lib = L.lib()
    _assert_split(Fr, gh, gw, rounds, straddle)
    P, shape = Fr * gh * gw, (Fr, 2 * gh, 2 * gw, C0)
    what = f"gather {form} kn{w_kn} F{Fr} {gh}x{gw} {hard or ''}"
    W = _randn(96, 4 * C0, scale=1 / 16, seed=seed + 1)                                # [n][(q, c)]
    sc, sh = _tables(Fr, C0, seed + 2)
    if form == "rebuilt":
        pt = _dev(_randn(Fr * 4 * gh * gw, 16, shift=0.2, seed=seed), BF16)
        w0 = _randn(C0, 16, scale=1 / 3, seed=seed + 4)
        if hard == "clamp":
            w0 = w0 * 4
        if hard == "spread":
            w0[5] *= 1e3
        w0 = _dev(w0, BF16)
    else:
        m = _big_map(Fr, gh, gw, seed) if rounds > 1 else _dev(_randn(*shape, seed=seed), BF16)
        if hard == "clamp":                                      # arguments of the GELU polynomial either side of its clamp at |z| = 4
            m = (m.float() * 4).to(BF16)
        if hard == "spread":                                     # one channel 10^3 against its neighbours inside one 8-channel group
            m = m.clone()
            m[..., 5] = (m[..., 5].float() * 1e3).to(BF16)
    if hard == "zero_row":
        W[7] = 0.0
    Wd = _dev(W, BF16)
    wdev = Wd.t().contiguous() if w_kn else Wd
    scd, shd = _dev(sc), _dev(sh)
    out, ob = _buf((P, 96), BF16)
    if form == "rebuilt":
        rc = lib.bf_gather_gemm_rebuilt(1, _p(pt), _p(w0), _p(wdev), w_kn, _p(scd), _p(shd), _p(out), Fr, gh, gw, C0, 96, _stream())
        y, ey = PB.rebuilt(pt, w0)
        a, ea = PB.pro_operand(y.reshape(shape), scd, shd, ev=ey.reshape(shape))
    else:
        tab = (scd, shd) if form == "gelu" else (None, None)
        rc = lib.bf_gather_gemm(1, _p(m), _p(wdev), w_kn, _p(tab[0]), _p(tab[1]), _p(out), Fr, gh, gw, C0, 96, _stream())
        a, ea = PB.pro_operand(m, *tab)
    L.check(rc, what)
    ref, bnd = PB.gather(a, ea, Wd, gh, gw)
    r = PB.check(out, ref, bnd, what, ("row", "col"))
    _tail(ob, what)
    if hard == "zero_row":
        assert float(out[:, 7].float().abs().max()) == 0.0
    return r


SMALL = [(1, 2, 16), (2, 4, 40), (2, 4, 8), (3, 6, 16)]          # one tile in all; a 16-row block wraps an image row; a tile spans four rows


@pytest.mark.parametrize("Fr,gh,gw", SMALL)
@pytest.mark.parametrize("form", ["plain", "gelu", "rebuilt"])
@pytest.mark.parametrize("w_kn", [0, 1])
def test_gather_small_geometry(Fr, gh, gw, form, w_kn):
    _note(f"gather ({form})", run_gather(Fr, gh, gw, form, w_kn, seed=Fr + gw), f"F{Fr} {gh}x{gw} kn{w_kn}")


@pytest.mark.parametrize("form", ["plain", "gelu", "rebuilt"])
@pytest.mark.parametrize("w_kn", [0, 1])
def test_gather_two_tiles_per_wave_across_frames(form, w_kn):
    Fr = _frames_for(2, 5)
    _note(f"gather ({form}), several tiles per wave", run_gather(Fr, 4, 40, form, w_kn, rounds=2, straddle=True, seed=3), f"F{Fr} kn{w_kn}")


def test_gather_three_tiles_per_wave():
    Fr = _frames_for(3, 5)
    _note("gather (plain), several tiles per wave", run_gather(Fr, 4, 40, "plain", 1, rounds=3, straddle=True, seed=4), f"F{Fr} rounds 3")


@pytest.mark.parametrize("form", ["plain", "gelu", "rebuilt"])
@pytest.mark.parametrize("hard", ["clamp", "spread", "zero_row"])
def test_gather_hard_inputs(form, hard):
    _note(f"gather ({form}), hard inputs", run_gather(3, 4, 40, form, 0, hard=hard, seed=9), hard)


def test_gather_refusals_write_nothing():
    lib = L.lib()
    m = _dev(_randn(2, 8, 32, C0, seed=1), BF16)
    W = _dev(_randn(96, 384, seed=2), BF16)
    out, ob = _buf((2 * 4 * 16, 96), BF16)
    pt, w0 = _dev(_randn(2 * 8 * 32, 16, seed=3), BF16), _dev(_randn(C0, 16, seed=4), BF16)
    sc, sh = (_dev(t) for t in _tables(2, C0, 5))
    assert lib.bf_gather_gemm(0, _p(m), _p(W), 0, None, None, _p(out), 2, 4, 16, C0, 96, _stream()) == 1               # fp32
    assert lib.bf_gather_gemm(1, _p(m), _p(W), 0, None, None, _p(out), 2, 4, 16, 64, 96, _stream()) == 1               # C0 != 96
    assert lib.bf_gather_gemm(1, _p(m), _p(W), 0, None, None, _p(out), 2, 3, 5, C0, 96, _stream()) == 1                # gh * gw % 32
    assert lib.bf_gather_gemm_rebuilt(0, _p(pt), _p(w0), _p(W), 0, _p(sc), _p(sh), _p(out), 2, 4, 16, C0, 96, _stream()) == 1
    assert lib.bf_gather_gemm_rebuilt(1, _p(pt), _p(w0), _p(W), 0, _p(sc), _p(sh), _p(out), 2, 3, 5, C0, 96, _stream()) == 1
    _untouched(ob, "gather refusals")


# ---------------------------------------------------------------------------------------------------- scatter GEMM
def run_scatter(Fr, gh, gw, pro, w_kn, with_part, rounds=1, straddle=False, hard=None, seed=0):
    lib = L.lib()
    _assert_split(Fr, gh, gw, rounds, straddle)
    P, S4, nsl = Fr * gh * gw, 4 * gh * gw, gh * gw // 32
    what = f"scatter pro{int(pro)} kn{w_kn} part{int(with_part)} F{Fr} {gh}x{gw} {hard or ''}"
    a = _randn(P, 96, seed=seed)
    if hard == "clamp":
        a = a * 4
    if hard == "spread":
        a[:, 5] *= 1e3
    W = _randn(4 * C0, 96, scale=1 / 8, seed=seed + 1)                                  # [(q, c)][k]
    if hard == "zero_row":
        W[C0 + 7] = 0.0
    if hard == "offset":                                         # every output far from zero: t2 - t1 mu of the partials cancels
        a = a.abs() + 1.0
        W = W.abs()
    ad, Wd = _dev(a, BF16), _dev(W, BF16)
    wdev = Wd.t().contiguous() if w_kn else Wd
    sc, sh = (_dev(t) for t in _tables(Fr, 96, seed + 2))
    tab = (sc, sh) if pro else (None, None)
    fmap, mb = _buf((Fr, 2 * gh, 2 * gw, C0), BF16)
    nws = max(int(lib.bf_in_ws_floats(1, Fr, S4, C0)), 2 * Fr * C0 * (1 + nsl))
    ws, wb = _buf((nws,))
    part = ws[2 * Fr * C0:]
    L.check(lib.bf_scatter_gemm(1, _p(ad), _p(wdev), w_kn, _p(tab[0]), _p(tab[1]), _p(fmap), _p(part) if with_part else None, Fr, gh, gw, 96, C0, _stream()), what)
    oa, ea = PB.pro_operand(ad.reshape(Fr, gh * gw, 96), *tab)
    ref, bnd = PB.scatter(oa.reshape(P, 96), ea.reshape(P, 96), Wd, Fr, gh, gw)
    r = PB.check(fmap, ref, bnd, what, ("frame", "y", "x", "channel"))
    _tail(mb, what)
    _tail(wb, what)
    if not with_part:
        assert torch.isnan(ws).all(), (what, "wrote partials nobody asked for")
        return r, None, None
    # the partials of each 128-pixel tile and the merged statistics, judged against the map as the kernel stored it
    got = part[:Fr * nsl * C0 * 2].view(Fr, nsl, C0, 2)
    assert torch.isnan(part[Fr * nsl * C0 * 2:]).all()
    want = PB.slice_partials(PB.scatter_tiles(fmap.double(), gh, gw), pow2=True)
    names = ("frame", "tile", "channel")
    rp = max(PB.check(got[..., 0], *want["mean"], what + " slice mean", names), PB.check(got[..., 1], *want["m2"], what + " slice m2", names))
    rm = None
    if lib.bf_in_ws_floats(1, Fr, S4, C0) >= 2 * Fr * C0 * (1 + nsl):
        w_, b_ = 1 + _randn(C0, scale=0.1, seed=seed + 5), _randn(C0, scale=0.1, seed=seed + 6)
        outs = [_buf((Fr, C0)) for _ in range(4)]
        wd, bd = _dev(w_), _dev(b_)
        L.check(lib.bf_in_stats_merge_slices(1, Fr, S4, C0, 128, _p(wd), _p(bd), None, 1, None, *[_p(o[0]) for o in outs], _p(ws), _stream()), "merge")
        st = NB.merge(got[..., 0].cpu(), got[..., 1].cpu(), 128, S4, w_, b_)
        rm = max(NB.check(o[0], *st[k], f"{what} merged {k}", ("frame", "channel")) for o, k in zip(outs, ("mean", "rstd", "sc", "sh")))
        for o in outs:
            _tail(o[1], what + " merged")
    return r, rp, rm


def _note_scatter(area, res, case):
    for tag, r in zip(("", ", slice partials", ", merged statistics"), res):
        if r is not None:
            _note("scatter" + area + tag, r, case)


@pytest.mark.parametrize("Fr,gh,gw", SMALL + [(2, 8, 16)])      # 8 x 16: 512 fine pixels, the shortest frame bf_in_stats slices
@pytest.mark.parametrize("pro", [False, True])
@pytest.mark.parametrize("w_kn", [0, 1])
def test_scatter_small_geometry(Fr, gh, gw, pro, w_kn):
    _note_scatter("", run_scatter(Fr, gh, gw, pro, w_kn, True, seed=Fr + gw), f"F{Fr} {gh}x{gw} pro{int(pro)} kn{w_kn}")
    _note_scatter("", run_scatter(Fr, gh, gw, pro, w_kn, False, seed=Fr + gw), f"F{Fr} {gh}x{gw} pro{int(pro)} kn{w_kn} no partials")


@pytest.mark.parametrize("pro,w_kn", [(False, 1), (True, 0)])
def test_scatter_two_tiles_per_wave_across_frames(pro, w_kn):
    Fr = _frames_for(2, 5)
    _note_scatter(", several tiles per wave", run_scatter(Fr, 4, 40, pro, w_kn, True, rounds=2, straddle=True, seed=5), f"F{Fr} pro{int(pro)}")


@pytest.mark.parametrize("pro", [False, True])
@pytest.mark.parametrize("hard", ["clamp", "spread", "zero_row", "offset"])
def test_scatter_hard_inputs(pro, hard):
    _note_scatter(", hard inputs", run_scatter(2, 8, 16, pro, 0, True, hard=hard, seed=13), f"{hard} pro{int(pro)}")


def test_scatter_refusals_write_nothing():
    lib = L.lib()
    a, W = _dev(_randn(2 * 4 * 16, 96, seed=1), BF16), _dev(_randn(384, 96, seed=2), BF16)
    fmap, mb = _buf((2, 8, 32, C0), BF16)
    part, pb = _buf((2 * 2 * C0 * 2,))
    assert lib.bf_scatter_gemm(0, _p(a), _p(W), 0, None, None, _p(fmap), _p(part), 2, 4, 16, 96, C0, _stream()) == 1    # fp32
    assert lib.bf_scatter_gemm(1, _p(a), _p(W), 0, None, None, _p(fmap), _p(part), 2, 4, 16, 96, 64, _stream()) == 1    # C0 != 96
    assert lib.bf_scatter_gemm(1, _p(a), _p(W), 0, None, None, _p(fmap), _p(part), 2, 4, 16, 64, C0, _stream()) == 1    # K != 96
    assert lib.bf_scatter_gemm(1, _p(a), _p(W), 0, None, None, _p(fmap), _p(part), 2, 3, 5, 96, C0, _stream()) == 1     # gh * gw % 32
    _untouched(mb, "scatter refusals")
    _untouched(pb, "scatter refusals")


# ---------------------------------------------------------------------------------------------------- gather wgrad
def run_wgrad(Fr, gh, gw, form, tr, r_div, seed=0):
    """r_div: the runs per frame wanted, forced through the workspace size; None: the preferred launch."""
    lib = L.lib()
    P, tpf, shape = Fr * gh * gw, gh * gw // 32, (Fr, 2 * gh, 2 * gw, C0)
    nws = PB.wgrad_ws_floats(Fr, gh, gw) if r_div is None else Fr * PB.SLAB * r_div
    assert lib.bf_gather_wgrad_ws_floats(Fr, gh, gw) == PB.wgrad_ws_floats(Fr, gh, gw)
    rpf = PB.wgrad_runs(Fr, tpf, nws)
    assert rpf == (r_div or PB.wgrad_runs(Fr, tpf)) and rpf >= 1
    steps, slabs = tpf // rpf, Fr * rpf
    what = f"wgrad {form} tr{tr} F{Fr} {gh}x{gw} steps{steps} slabs{slabs}"
    coarse = _dev(_randn(P, 96, seed=seed + 1), BF16)
    sc, sh = (_dev(t) for t in _tables(Fr, 96, seed + 2))
    tab, none = (sc, sh), (None, None)
    ws, wb = _buf((nws,))
    out, ob = _buf((96, 384) if tr else (384, 96))
    if form == "rebuilt":
        pt, w0 = _dev(_randn(P * 4, 16, shift=0.2, seed=seed), BF16), _dev(_randn(C0, 16, scale=1 / 3, seed=seed + 4), BF16)
        call = lambda o, n: lib.bf_gather_wgrad_rebuilt(1, _p(pt), _p(w0), _p(coarse), _p(sc), _p(sh), _p(o), tr, Fr, gh, gw, C0, 96, _p(ws), n, _stream())
        y, ey = PB.rebuilt(pt, w0)
        a, ea = PB.pro_operand(y.reshape(shape), sc, sh, ev=ey.reshape(shape))
    else:
        fine = _dev(_randn(*shape, seed=seed), BF16)
        ft, ct = (tab if form == "fine" else none), (tab if form == "coarse" else none)
        call = lambda o, n: lib.bf_gather_wgrad(1, _p(fine), _p(coarse), _p(ft[0]), _p(ft[1]), _p(ct[0]), _p(ct[1]), _p(o), tr, Fr, gh, gw, C0, 96, _p(ws), n, _stream())
        a, ea = PB.pro_operand(fine, *ft)
    L.check(call(out, nws), what)
    b, eb = PB.pro_operand(coarse.reshape(Fr, gh * gw, 96), *(tab if form == "coarse" else none))
    ref, bnd = PB.wgrad(PB.gather_rows(a, gh, gw), PB.gather_rows(ea, gh, gw), b.reshape(P, 96), eb.reshape(P, 96), steps, slabs)
    r = PB.check(out.t() if tr else out, ref, bnd, what, ("qc", "k"))
    _tail(ob, what)
    _tail(wb, what)
    out2, ob2 = _buf(tuple(out.shape))
    L.check(call(out2, nws), what)
    torch.cuda.synchronize()
    assert torch.equal(out, out2), (what, "two runs differ")
    return r, call


FORMS = [("plain", 0), ("fine", 1), ("coarse", 0), ("rebuilt", 1), ("plain", 1), ("fine", 0)]


@pytest.mark.parametrize("form,tr", FORMS)
@pytest.mark.parametrize("r_div", [6, 3, 2])
def test_wgrad_steps_per_run(form, tr, r_div):
    """Six tiles per frame in runs of one, two and three 32-row steps: both coarse-tile buffers and the prefetch."""
    r, _ = run_wgrad(2, 4, 48, form, tr, r_div, seed=r_div)
    _note(f"wgrad ({form})", r, f"steps {6 // r_div} tr{tr}")


@pytest.mark.parametrize("Fr,gh,gw,r_div,slabs", [(1, 2, 16, 1, 1), (2, 4, 48, 2, 4), (10, 4, 48, 6, 60), (61, 4, 16, 1, 61), (65, 2, 16, 1, 65),
                                                  (43, 4, 48, 3, 129)])
def test_wgrad_slab_counts(Fr, gh, gw, r_div, slabs):
    """Either side of gather_wgrad_reduce_kernel's unrolled loop (r + 60 < rows) and its four-lane tail."""
    assert Fr * r_div == slabs
    for form, tr in FORMS[:4]:
        r, _ = run_wgrad(Fr, gh, gw, form, tr, r_div, seed=slabs)
        _note(f"wgrad ({form})", r, f"slabs {slabs}")


def test_wgrad_cap_on_workgroups():
    """103 frames of five tiles: five runs per frame would be 515 workgroups, above the cap of 512, so the preferred launch is one run of
    five steps per frame."""
    assert PB.wgrad_runs(103, 5) == 1 and PB.wgrad_runs(102, 5) == 5
    r, _ = run_wgrad(103, 4, 40, "fine", 1, None, seed=8)
    _note("wgrad (fine)", r, "103 frames, capped")


def test_wgrad_refusals_write_nothing():
    lib = L.lib()
    Fr, gh, gw = 2, 4, 16
    fine, coarse = _dev(_randn(Fr, 2 * gh, 2 * gw, C0, seed=1), BF16), _dev(_randn(Fr * gh * gw, 96, seed=2), BF16)
    sc, sh = (_dev(t) for t in _tables(Fr, 96, 3))
    nws = PB.wgrad_ws_floats(Fr, gh, gw)
    ws, wb = _buf((nws,))
    out, ob = _buf((384, 96))
    tail = (Fr, gh, gw, C0, 96, _p(ws))
    assert lib.bf_gather_wgrad(0, _p(fine), _p(coarse), None, None, None, None, _p(out), 0, *tail, nws, _stream()) == 1                       # fp32
    assert lib.bf_gather_wgrad(1, _p(fine), _p(coarse), None, None, None, None, _p(out), 0, *tail, Fr * PB.SLAB - 1, _stream()) == 1          # no slab per frame
    assert lib.bf_gather_wgrad(1, _p(fine), _p(coarse), _p(sc), _p(sh), _p(sc), _p(sh), _p(out), 0, *tail, nws, _stream()) == 1               # both sides
    assert lib.bf_gather_wgrad(1, _p(fine), _p(coarse), None, None, None, None, _p(out), 0, Fr, 3, 5, C0, 96, _p(ws), nws, _stream()) == 1    # gh * gw % 32
    assert lib.bf_gather_wgrad(1, _p(fine), _p(coarse), None, None, None, None, _p(out), 0, Fr, gh, gw, 64, 96, _p(ws), nws, _stream()) == 1  # C0 != 96
    _untouched(ob, "wgrad refusals")
    _untouched(wb, "wgrad refusals")


# ---------------------------------------------------------------------------------------------------- last-stage kernels
GEOM = {1: (1, 16), 15: (5, 48), 16: (8, 32), 17: (17, 16), 63: (21, 48), 64: (32, 32), 65: (65, 16), 129: (43, 48)}      # groups -> (h, w)
LAST = [(g, Ci, (i + j) % 4 + 1) for i, g in enumerate(GEOM) for j, Ci in enumerate((32, 64, 96, 128))]


def _last(groups, Ci, Co, seed):
    h, w = GEOM[groups]
    Fr = 2
    s = PB.dl_split(h, w)
    assert s["groups"] == groups and s["waves"] == -(-groups // 16) and s["wgs"] == -(-groups // 64)
    d = dict(Fr=Fr, h=h, w=w, Ci=Ci, Co=Co, P=Fr * h * w, S=h * w, split=s)
    wc = torch.zeros(Ci, 16)
    wc[:, :4 * Co] = _randn(Ci, 4 * Co, scale=Ci ** -0.5, seed=seed)
    d["wc"] = _dev(wc, BF16)
    shp = (Fr, Co, 2 * h, 2 * w)
    d["y"], d["pred"], d["dpred"] = _dev(_randn(*shp, seed=seed + 1)), _dev(_randn(*shp, seed=seed + 2)), _dev(_randn(*shp, scale=0.3, seed=seed + 3))
    d["coef"], d["gs"] = _dev(0.5 + _rand(Fr, Co, seed=seed + 4)), _dev(torch.tensor([0.7]))
    return d


def _limbs(buf):
    out = torch.zeros(buf.shape[:-1], dtype=torch.float64, device=buf.device)
    for k in range(buf.shape[-1]):
        out += buf[..., k].double() * 2.0 ** (48 * k) * PB.LIMB_UNIT
    return out


@pytest.mark.parametrize("groups,Ci,Co", LAST)
def test_debed_last(groups, Ci, Co):
    lib = L.lib()
    assert L.BF_LOSS_LIMBS == PB.LOSS_LIMBS
    d = _last(groups, Ci, Co, seed=groups + Ci)
    Fr, h, w, P = d["Fr"], d["h"], d["w"], d["P"]
    what = f"debed_last groups{groups} Ci{Ci} Co{Co}"
    act = _dev(_randn(P, Ci, seed=groups), BF16)
    sc, sh = (_dev(t) for t in _tables(Fr, Ci, Ci))
    pred, pb = _buf((Fr, Co, 2 * h, 2 * w))
    nl = Fr * Co * 2 * L.BF_LOSS_LIMBS
    lb = torch.zeros(nl + TAIL, dtype=torch.int64, device=DEV)
    lb[nl:] = -7
    L.check(lib.bf_debed_last(1, _p(act), _p(sc), _p(sh), _p(d["wc"]), _p(pred), _p(d["y"]), _p(lb), Fr, Ci, Co, h, w, 16, _stream()), what)
    ref, bnd = PB.debed_last(act, sc, sh, d["wc"], Fr, Co, h, w)
    _note("debed_last pred", PB.check(pred, ref, bnd, what), what)
    _tail(pb, what)
    assert bool((lb[nl:] == -7).all()), (what, "wrote past the loss limbs")
    v = _limbs(lb[:nl].view(Fr, Co, 2, L.BF_LOSS_LIMBS))
    want = PB.loss_limbs(pred, d["y"], h, w)
    _note("debed_last loss limbs", max(PB.check(v[..., 0], *want["num"], what + " num", ("frame", "channel")),
                                        PB.check(v[..., 1], *want["den"], what + " den", ("frame", "channel"))), what)
    pred2, pb2 = _buf((Fr, Co, 2 * h, 2 * w))                    # without a target: the same prediction, bit for bit
    L.check(lib.bf_debed_last(1, _p(act), _p(sc), _p(sh), _p(d["wc"]), _p(pred2), None, None, Fr, Ci, Co, h, w, 16, _stream()), what)
    _tail(pb2, what)
    assert torch.equal(pred, pred2)


def _sources(d, mode):
    """-> (the five source arguments, patch_bounds.dpm's keywords)."""
    if mode == "given":
        return (_p(d["dpred"]), None, None, None, None), dict(dpred=d["dpred"])
    kw = dict(pred=d["pred"], y=d["y"], coef=d["coef"], gscale=d["gs"])
    if mode == "fused":
        return (None, _p(d["pred"]), _p(d["y"]), _p(d["coef"]), _p(d["gs"])), kw
    return (_p(d["dpred"]), _p(d["pred"]), _p(d["y"]), _p(d["coef"]), _p(d["gs"])), dict(dpred=d["dpred"], **kw)


@pytest.mark.parametrize("groups,Ci,Co", LAST)
def test_debed_last_bwd_and_with_the_norm_in_front(groups, Ci, Co):
    """The three gradient sources; dpm of both entry points bit-identical; dact and dx judged on the kernel's own dpm; a workspace of
    exactly 2 F Ci (1 + slices) floats, the last slice ragged unless groups is a multiple of 16; priors in d_in_w / d_in_b, and both NULL."""
    lib = L.lib()
    d = _last(groups, Ci, Co, seed=groups + Ci + 1)
    Fr, h, w, P, S = d["Fr"], d["h"], d["w"], d["P"], d["S"]
    nsl = d["split"]["slices"]
    assert nsl == -(-S // 256) and d["split"]["last_rows"] == S - 256 * (nsl - 1)
    ymap = _dev(_randn(P, Ci, scale=1.5, shift=0.2, seed=groups + 2), BF16)
    yf = ymap.float().view(Fr, S, Ci)
    mean, rstd = yf.mean(1).contiguous(), (yf.var(1, unbiased=False) + 1e-5).rsqrt().contiguous()
    in_w, in_b = _dev(1 + _randn(Ci, scale=0.2, seed=Ci)), _dev(_randn(Ci, scale=0.3, seed=Ci + 1))
    nws = 2 * Fr * Ci * (1 + nsl)
    for mode in ("given", "fused", "both"):
        what = f"debed_last_bwd {mode} groups{groups} Ci{Ci} Co{Co}"
        src, kw = _sources(d, mode)
        dpm, db = _buf((P, 16), BF16)
        dact, ab = _buf((P, Ci), BF16)
        L.check(lib.bf_debed_last_bwd(1, *src, _p(d["wc"]), _p(dpm), _p(dact), Fr, Ci, Co, h, w, 16, _stream()), what)
        ref, err = PB.dpm(h, w, **kw)
        if mode == "given":
            assert float(err.max()) == 0.0
        _note(f"dpm ({mode})", PB.check(dpm, ref, err, what + " dpm", ("row", "n")), what)
        _note("debed_last_bwd dact", PB.check(dact, *PB.rank16(dpm, d["wc"]), what + " dact", ("row", "channel")), what)
        _tail(db, what)
        _tail(ab, what)
        # ... with the InstanceNorm + GELU in front
        prior = mode != "fused"
        dpm2, db2 = _buf((P, 16), BF16)
        dx, xb = _buf((P, Ci), BF16)
        ws, wb = _buf((nws,))
        dw, dwb = _buf((Ci,), init=torch.full((Ci,), 2.0))
        dbi, dbb = _buf((Ci,), init=torch.full((Ci,), -1.0))
        args = (_p(d["wc"]), _p(dpm2), _p(ymap), _p(mean), _p(rstd), _p(in_w), _p(in_b), _p(dx), _p(dw) if prior else None, _p(dbi) if prior else None)
        L.check(lib.bf_debed_last_bwd_norm(1, *src, *args, Fr, Ci, Co, h, w, 16, _p(ws), nws, _stream()), what + " norm")
        torch.cuda.synchronize()
        assert torch.equal(dpm, dpm2), (what, "dpm differs between the two entry points")
        want = PB.debed_last_bwd_norm(dpm2, d["wc"], ymap, mean, rstd, in_w, in_b, Fr)
        _note("debed_last_bwd_norm dx", PB.check(dx, *want["dx"], what + " dx", ("row", "channel")), what)
        tot = ws[:2 * Fr * Ci].view(Fr, Ci, 2)
        _note("debed_last_bwd_norm sums", max(PB.check(tot[..., 0], *want["s1"], what + " s1", ("frame", "channel")),
                                               PB.check(tot[..., 1], *want["s2"], what + " s2", ("frame", "channel"))), what)
        for b in (db2, xb, wb, dwb, dbb):
            _tail(b, what + " norm")
        if prior:
            cpu = lambda pr: tuple(t.cpu() for t in pr)
            pg = NB.param_grads(cpu(want["s1"]), cpu(want["s2"]), in_w.cpu(), in_b.cpu(), prior=dict(dw=torch.full((Ci,), 2.0), db=torch.full((Ci,), -1.0)), gelu=True)
            _note("debed_last_bwd_norm d_in_w / d_in_b", max(NB.check(dw, *pg["dw"], what + " dw", ("channel",)), NB.check(dbi, *pg["db"], what + " db", ("channel",))), what)
        else:
            assert bool((dw == 2.0).all()) and bool((dbi == -1.0).all())
    # refusals: fp32, Np != 16, w % 16, a workspace one float short
    dpm, db = _buf((P, 16), BF16)
    dx, xb = _buf((P, Ci), BF16)
    ws, wb = _buf((nws,))
    src, _ = _sources(d, "given")
    args = (_p(d["wc"]), _p(dpm), _p(ymap), _p(mean), _p(rstd), _p(in_w), _p(in_b), _p(dx), None, None)
    assert lib.bf_debed_last_bwd(0, *src, _p(d["wc"]), _p(dpm), _p(dx), Fr, Ci, Co, h, w, 16, _stream()) == 1
    assert lib.bf_debed_last_bwd(1, *src, _p(d["wc"]), _p(dpm), _p(dx), Fr, Ci, Co, h, w, 24, _stream()) == 1
    assert lib.bf_debed_last_bwd(1, *src, _p(d["wc"]), _p(dpm), _p(dx), Fr, Ci, Co, h * 2, w // 2 + 4, 16, _stream()) == 1
    assert lib.bf_debed_last_bwd_norm(0, *src, *args, Fr, Ci, Co, h, w, 16, _p(ws), nws, _stream()) == 1
    assert lib.bf_debed_last_bwd_norm(1, *src, *args, Fr, Ci, Co, h, w, 16, _p(ws), nws - 1, _stream()) == 1
    for b in (db, xb, wb):
        _untouched(b, "last-stage refusals")


def test_debed_last_refusals_write_nothing():
    lib = L.lib()
    d = _last(17, 64, 3, seed=5)
    Fr, h, w = d["Fr"], d["h"], d["w"]
    act = _dev(_randn(d["P"], 64, seed=1), BF16)
    sc, sh = (_dev(t) for t in _tables(Fr, 64, 2))
    pred, pb = _buf((Fr, 3, 2 * h, 2 * w))
    a = (_p(act), _p(sc), _p(sh), _p(d["wc"]), _p(pred), None, None)
    assert lib.bf_debed_last(0, *a, Fr, 64, 3, h, w, 16, _stream()) == 1               # fp32
    assert lib.bf_debed_last(1, *a, Fr, 64, 3, h, w, 24, _stream()) == 1               # Np != 16
    assert lib.bf_debed_last(1, *a, Fr, 64, 5, h, w, 16, _stream()) == 1               # Co > 4
    assert lib.bf_debed_last(1, *a, Fr, 48, 3, h, w, 16, _stream()) == 1               # Ci % 32
    assert lib.bf_debed_last(1, *a, Fr, 64, 3, h * 2, w // 2, 16, _stream()) == 1      # w % 16
    _untouched(pb, "debed_last refusals")


@pytest.mark.parametrize("groups,C,cin", LAST)
def test_embed_first(groups, C, cin):
    """patches to the bit, y0 on the kernel's own patches, the 256-row slice partials (the last one ragged) on the kernel's own y0 and
    merged; y0 = NULL with the partials, and the partials NULL with y0, change no bit of what is left."""
    lib = L.lib()
    h2, w2 = GEOM[groups]
    Fr, S, P = 2, h2 * w2, 2 * h2 * w2
    nsl = PB.dl_split(h2, w2)["slices"]
    what = f"embed_first groups{groups} C{C} cin{cin}"
    x = _dev(_randn(Fr, cin, 2 * h2, 2 * w2, shift=0.5, seed=groups + C))
    wc = torch.zeros(C, 16)
    wc[:, :4 * cin] = _randn(C, 4 * cin, scale=0.5, seed=C)
    wc = _dev(wc, BF16)
    nws = max(int(lib.bf_in_ws_floats(1, Fr, S, C)), 2 * Fr * C * (1 + nsl))
    ws, wb = _buf((nws,))
    part = ws[2 * Fr * C:]
    pt, ptb = _buf((P, 16), BF16)
    y0, yb = _buf((P, C), BF16)
    L.check(lib.bf_embed_first(1, _p(x), _p(wc), _p(pt), _p(y0), Fr, C, cin, h2, w2, 16, _p(part), _stream()), what)
    ref, err = PB.dpm(h2, w2, dpred=x)
    assert float(err.max()) == 0.0
    _note("embed_first patches", PB.check(pt, ref, err, what + " patches", ("row", "k")), what)
    _note("embed_first y0", PB.check(y0, *PB.rank16(pt, wc), what + " y0", ("row", "channel")), what)
    got = part[:Fr * nsl * C * 2].view(Fr, nsl, C, 2)
    want = PB.sliced(y0.double().view(Fr, S, C), 256, pow2=False)
    names = ("frame", "slice", "channel")
    _note("embed_first slice partials", max(PB.check(got[..., 0], *want["mean"], what + " slice mean", names),
                                             PB.check(got[..., 1], *want["m2"], what + " slice m2", names)), what)
    for b in (wb, ptb, yb):
        _tail(b, what)
    assert torch.isnan(ws[:2 * Fr * C]).all() and torch.isnan(part[Fr * nsl * C * 2:]).all()
    if lib.bf_in_ws_floats(1, Fr, S, C) >= 2 * Fr * C * (1 + nsl):
        w_, b_ = 1 + _randn(C, scale=0.1, seed=C + 5), _randn(C, scale=0.1, seed=C + 6)
        outs = [_buf((Fr, C)) for _ in range(4)]
        wd, bd = _dev(w_), _dev(b_)
        L.check(lib.bf_in_stats_merge_slices(1, Fr, S, C, 256, _p(wd), _p(bd), None, 1, None, *[_p(o[0]) for o in outs], _p(ws), _stream()), "merge")
        st = NB.merge(got[..., 0].cpu(), got[..., 1].cpu(), 256, S, w_, b_)
        _note("embed_first merged statistics", max(NB.check(o[0], *st[k], f"{what} merged {k}", ("frame", "channel")) for o, k in zip(outs, ("mean", "rstd", "sc", "sh"))), what)
    pt2, ptb2 = _buf((P, 16), BF16)
    ws2, wb2 = _buf((nws,))
    L.check(lib.bf_embed_first(1, _p(x), _p(wc), _p(pt2), None, Fr, C, cin, h2, w2, 16, _p(ws2[2 * Fr * C:]), _stream()), what + " y0 = NULL")
    torch.cuda.synchronize()
    assert torch.equal(pt, pt2) and torch.equal(ws2[2 * Fr * C:][:Fr * nsl * C * 2], part[:Fr * nsl * C * 2])
    pt3, ptb3 = _buf((P, 16), BF16)
    y3, yb3 = _buf((P, C), BF16)
    L.check(lib.bf_embed_first(1, _p(x), _p(wc), _p(pt3), _p(y3), Fr, C, cin, h2, w2, 16, None, _stream()), what + " no partials")
    torch.cuda.synchronize()
    assert torch.equal(pt, pt3) and torch.equal(y0, y3)
    for b in (ptb2, wb2, ptb3, yb3):
        _tail(b, what)
    # refusals
    y4, yb4 = _buf((P, C), BF16)
    pt4, ptb4 = _buf((P, 16), BF16)
    assert lib.bf_embed_first(0, _p(x), _p(wc), _p(pt4), _p(y4), Fr, C, cin, h2, w2, 16, None, _stream()) == 1
    assert lib.bf_embed_first(1, _p(x), _p(wc), _p(pt4), _p(y4), Fr, C, cin, h2, w2, 24, None, _stream()) == 1
    _untouched(yb4, "embed_first refusals")
    _untouched(ptb4, "embed_first refusals")


# ---------------------------------------------------------------------------------------------------- embed tail
def run_tail(Fr, gh1, gw1, C1, stored, hard=None, seed=0):
    lib = L.lib()
    S1, S0 = gh1 * gw1, 4 * gh1 * gw1
    tpw, cpf = PB.tail_plan(S1)
    nws = PB.tail_ws_floats(Fr, gh1, gw1)
    assert lib.bf_embed_tail_ws_floats(Fr, gh1, gw1, C0, 16) == nws > 0
    what = f"embed_tail F{Fr} {gh1}x{gw1} C1 {C1} {'stored' if stored else 'rebuilt'} tpw{tpw} cpf{cpf} {hard or ''}"
    pt = _randn(Fr * S0, 16, shift=0.3, seed=seed)
    w0 = _randn(C0, 16, scale=1 / 3, seed=seed + 1)
    dy1 = _randn(Fr * S1, C1, seed=seed + 3)
    if hard == "flat_channel":                                   # a channel of (near) zero variance: rstd = eps^-1/2
        pt[:, 15] = 1.0
        w0[5] = 0.0
        w0[5, 15] = 0.5
    if hard == "cancel":                                         # G, t1 P1 and t2 PX nearly cancel: patch rows far from zero, almost one dy1 row
        pt = pt + 2.0
        dy1 = _randn(1, C1, seed=seed + 3) + 0.05 * dy1
    pt, w0, dy1 = _dev(pt, BF16), _dev(w0, BF16), _dev(dy1, BF16)
    w1 = _dev(_randn(C1, 4 * C0, scale=1 / 8, seed=seed + 2), BF16)
    in_w, in_b = _dev(1 + _randn(C0, scale=0.2, seed=seed + 4)), _dev(_randn(C0, scale=0.3, seed=seed + 5))
    y0 = (pt.float() @ w0.float().t()).to(BF16)                  # what bf_embed_first stores
    yf = y0.float().view(Fr, S0, C0)
    mean, rstd = yf.mean(1).contiguous(), (yf.var(1, unbiased=False) + 1e-5).rsqrt().contiguous()
    sc = (rstd * in_w).contiguous()
    sh = (in_b - mean * sc).contiguous()
    ws, wb = _buf((nws,))
    dwp, pb = _buf((C0, 16))
    dw, dwb = _buf((C0,), init=torch.full((C0,), 2.0))
    db, dbb = _buf((C0,), init=torch.full((C0,), -1.0))
    a = [_p(t) for t in (dy1, w1, y0 if stored else None, pt, w0, sc, sh, mean, rstd, in_w)]
    L.check(lib.bf_embed_tail_bwd(1, *a, _p(dwp), _p(dw), _p(db), Fr, gh1, gw1, C1, C0, 16, _p(ws), nws, _stream()), what)
    pri = dict(prior_w=torch.full((C0,), 2.0), prior_b=torch.full((C0,), -1.0))
    want = PB.embed_tail(dy1, w1, pt, w0, sc, sh, mean, rstd, in_w, Fr, gh1, gw1, y0=y0 if stored else None, **pri)
    r = PB.check(dwp, *want["dwprep"], what + " dwprep", ("channel", "k"))
    rp = max(PB.check(dw, *want["d_in_w"], what + " d_in_w", ("channel",)), PB.check(db, *want["d_in_b"], what + " d_in_b", ("channel",)))
    for b in (wb, pb, dwb, dbb):
        _tail(b, what)
    dwp2, pb2 = _buf((C0, 16))
    L.check(lib.bf_embed_tail_bwd(1, *a, _p(dwp2), None, None, Fr, gh1, gw1, C1, C0, 16, _p(ws), nws, _stream()), what)
    torch.cuda.synchronize()
    assert torch.equal(dwp, dwp2), (what, "two runs differ")
    dwp3, pb3 = _buf((C0, 16))
    assert lib.bf_embed_tail_bwd(1, *a, _p(dwp3), None, None, Fr, gh1, gw1, C1, C0, 16, _p(ws), nws - 1, _stream()) == 1
    _untouched(pb3, what + " one float short")
    return r, rp


TAIL_GEOM = {1: (8, 16), 2: (8, 32), 4: (8, 64), 5: (20, 32), 6: (16, 48), 7: (14, 64)}      # S1 / 128 -> (gh1, gw1)
TAIL_PLAN = {1: (1, 1), 2: (2, 1), 4: (4, 1), 5: (5, 1), 6: (6, 1), 7: (1, 7)}


@pytest.mark.parametrize("n", sorted(TAIL_GEOM))
@pytest.mark.parametrize("C1", [96, 192])
@pytest.mark.parametrize("stored", [True, False])
def test_embed_tail_every_plan(n, C1, stored):
    gh1, gw1 = TAIL_GEOM[n]
    assert PB.tail_plan(gh1 * gw1) == TAIL_PLAN[n]
    for Fr in (2, 3):                                            # 4 F cpf workgroups: a multiple of 8 (remapped block index) and not
        assert (4 * Fr * TAIL_PLAN[n][1]) % 8 == (0 if Fr == 2 else 4)
        r, rp = run_tail(Fr, gh1, gw1, C1, stored, seed=n + Fr)
        _note("embed_tail dwprep", r, f"S1 {128 * n} F{Fr} C1 {C1} stored{int(stored)}")
        _note("embed_tail d_in_w / d_in_b", rp, f"S1 {128 * n} F{Fr} C1 {C1} stored{int(stored)}")


@pytest.mark.parametrize("Fr", [1, 15, 16, 17, 35])
@pytest.mark.parametrize("stored", [True, False])
def test_embed_tail_frame_loop(Fr, stored):
    """Either side of embed_tail_sum_kernel's 16-deep frame loop (r + 16 <= F)."""
    r, rp = run_tail(Fr, 8, 16, 96, stored, seed=Fr)
    _note("embed_tail dwprep", r, f"F{Fr} stored{int(stored)}")
    _note("embed_tail d_in_w / d_in_b", rp, f"F{Fr} stored{int(stored)}")


@pytest.mark.parametrize("hard", ["flat_channel", "cancel"])
@pytest.mark.parametrize("stored", [True, False])
def test_embed_tail_hard_inputs(hard, stored):
    r, rp = run_tail(3, 8, 32, 96, stored, hard=hard, seed=17)
    _note("embed_tail dwprep, hard inputs", r, f"{hard} stored{int(stored)}")
    _note("embed_tail d_in_w / d_in_b, hard inputs", rp, f"{hard} stored{int(stored)}")


def test_embed_tail_refusals_write_nothing():
    lib = L.lib()
    Fr, gh1, gw1 = 2, 8, 16
    nws = PB.tail_ws_floats(Fr, gh1, gw1)
    t = lambda *s: _dev(_randn(*s, seed=1), BF16)
    dy1, w1, y0, pt, w0 = t(Fr * 128, 96), t(96, 384), t(Fr * 512, C0), t(Fr * 512, 16), t(C0, 16)
    f = [_dev(_randn(Fr, C0, seed=2)) for _ in range(4)] + [_dev(_randn(C0, seed=3))]
    ws, wb = _buf((nws,))
    dwp, pb = _buf((C0, 16))
    a = [_p(x) for x in (dy1, w1, y0, pt, w0, *f)]
    assert lib.bf_embed_tail_bwd(0, *a, _p(dwp), None, None, Fr, gh1, gw1, 96, C0, 16, _p(ws), nws, _stream()) == 1          # fp32
    assert lib.bf_embed_tail_bwd(1, *a, _p(dwp), None, None, Fr, gh1, gw1, 128, C0, 16, _p(ws), nws, _stream()) == 1         # C1
    assert lib.bf_embed_tail_bwd(1, *a, _p(dwp), None, None, Fr, gh1, gw1, 96, 64, 16, _p(ws), nws, _stream()) == 1          # C0
    assert lib.bf_embed_tail_bwd(1, *a, _p(dwp), None, None, Fr, gh1, gw1, 96, C0, 24, _p(ws), nws, _stream()) == 1          # Kp
    assert lib.bf_embed_tail_bwd(1, *a, _p(dwp), None, None, Fr, gh1 + 8, gw1 + 8, 96, C0, 16, _p(ws), nws, _stream()) == 1  # gw1 % 16
    assert lib.bf_embed_tail_bwd(1, *a, _p(dwp), None, None, Fr, 6, 16, 96, C0, 16, _p(ws), nws, _stream()) == 1             # gh1 * gw1 % 128
    _untouched(pb, "embed_tail refusals")
    _untouched(wb, "embed_tail refusals")


# ---------------------------------------------------------------------------------------------------- report
def test_report_worst_ratios(capsys):
    """Last in the module: prints the worst |got - ref| / bound of each area the tests above reached (all are <= 1, or they failed)."""
    assert all(r <= 1.0 for r, _ in WORST.values())
    with capsys.disabled():
        print("\nworst |got - ref| / bound per area:")
        for area, (r, case) in sorted(WORST.items()):
            print(f"  {area:46s} {r:.3e}  ({case})")
