"""GPU: the InstanceNorm kernels of norm.hip and the InReduceJob reduction of param_reduce.h at their edges, every output element held
to the per-element bound of tests/norm_bounds.py, through the C ABI (bf_in_stats, bf_in_bwd, bf_affine_apply, bf_colsum,
bf_in_stats_merge_slices) in both dtypes.

Frame lengths either side of every dispatch threshold of both geometries (row groups, the register cache, one backward slice, 5 and 9
slices with a ragged last one), channel counts from one chunk to 288, ws = NULL (the atomic parameter gradients below the cached length,
the uncached <T, false> kernels above it), the FiLM arguments (g, gb, gdiv with a ragged last group, dg / dgb alone and together, priors
in all four), enough frames for the eight-deep batch loop of in_reduce_block and its redo pass, cancelling and badly scaled inputs,
argument refusals, and sentinel tails behind every output and behind a workspace of exactly bf_in_ws_floats floats.  The kernels carry no
per-variant profiler names, so each case states the path it expects from the geometry constants written out below, and asserts that
norm_bounds' restated slice_cfg and the library's own bf_in_ws_floats (which is 2 F C (1 + slices) on the sliced path) agree with it.
The last test prints the worst |got - ref| / bound of each area."""
import pytest
import torch

from bubbleformer_amd import _lib as L
from tests import norm_bounds as NB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
DTS = [F32, BF16]
TAIL = 64
NAN = float("nan")
WORST = {}
# norm.hip: (row groups, cached rows) of the one-workgroup kernels; (statistics slice, backward slice) per geometry
RG = {F32: 16, BF16: 32}
CACHED = {F32: 96, BF16: 192}
SLICE = {(F32, False): (96, 384), (BF16, False): (192, 768), (F32, True): (48, 192), (BF16, True): (96, 384)}


def _note(area, dt, ratio, case):
    area = f"{area}, {'bf16' if dt == BF16 else 'fp32'}"
    if ratio >= WORST.get(area, (-1.0, ""))[0]:
        WORST[area] = (ratio, case)


def _randn(*shape, scale=1.0, shift=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift


def _st(t, dt):
    return t.to(dt).double()


def _dti(dt):
    return L.BF_DTYPE_BF16 if dt == BF16 else L.BF_DTYPE_F32


def _buf(n, dt=F32, init=None):
    """n elements (NaN, or `init`) followed by a NaN tail no kernel may touch."""
    b = torch.full((n + TAIL,), NAN, dtype=dt, device=DEV)
    if init is not None:
        b[:n] = init.reshape(-1).to(dt).to(DEV)
    return b


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _tail(b, n, what):
    assert torch.isnan(b[n:].float()).all(), (what, "wrote past its extent")


def _expect(dt, S, C, ws=True):
    """The path a shape must take, from the constants above -> (kind, wide, statistics slices, backward slices); checked against the
    restatement and, through the workspace size, against the library's own slice_cfg."""
    bf = dt == BF16
    wide = C % 96 == 0
    srows, brows = SLICE[(dt, wide)]
    if S <= CACHED[dt]:
        exp = ("cached", False, 0, 0)
    elif not ws:
        exp = ("uncached", False, 0, 0)
    else:
        exp = ("sliced", wide, -(-S // srows), -(-S // brows))
    p = NB.path(bf, S, C, ws)
    assert (p["kind"], p["wide"], p["stat_slices"], p["bwd_slices"]) == exp, (dt, S, C, ws, p, exp)
    nsl = -(-S // srows) if S > CACHED[dt] else 0
    for Fr in (1, 3):
        n = L.lib().bf_in_ws_floats(_dti(dt), Fr, S, C)
        assert n == 2 * Fr * C * (1 + nsl) == NB.ws_floats(bf, Fr, S, C), (dt, S, C, n)
    return exp


def _film(Fr, gdiv, C, seed, with_gb=True):
    ng = -(-Fr // gdiv)
    g = _randn(ng, C, scale=0.3, shift=1.0, seed=seed).float()
    return g, (_randn(ng, C, scale=0.5, seed=seed + 1).float() if with_gb else None)


def _exp_g(g, gdiv, Fr):
    return None if g is None else g[torch.arange(Fr) // gdiv]


def _dev(t):
    return None if t is None else t.to(DEV)


# ---------------------------------------------------------------------------------------------------- runners
def run_stats(dt, Fr, S, C, kind, ws=True, film="none", gdiv=1, x=None, seed=0):
    """One bf_in_stats call against the bound -> worst ratio.  kind: the path the case is about ("cached" | "uncached" | "sliced")."""
    h = L.lib()
    exp = _expect(dt, S, C, ws)
    assert exp[0] == kind, (dt, S, C, ws, "takes", exp, "not", kind)
    what = f"stats {dt} F{Fr} S{S} C{C} {exp} ws{int(ws)} {film} gdiv{gdiv}"
    x = _st(_randn(Fr, S, C, scale=1.5, shift=0.3, seed=seed) if x is None else x, dt)
    w, b = _randn(C, scale=0.4, shift=1.0, seed=seed + 1).float(), _randn(C, scale=0.5, seed=seed + 2).float()
    g, gb = _film(Fr, gdiv, C, seed + 3, film == "g+gb") if film != "none" else (None, None)
    xd, wd, bd, gd, gbd = (_dev(t) for t in (x.to(dt), w, b, g, gb))
    outs = {k: _buf(Fr * C) for k in ("mean", "rstd", "sc", "sh")}
    nws = h.bf_in_ws_floats(_dti(dt), Fr, S, C)
    wsb = _buf(nws) if ws else None
    L.check(h.bf_in_stats(_dti(dt), _p(xd), Fr, S, C, _p(wd), _p(bd), _p(gd), gdiv, _p(gbd), _p(outs["mean"]), _p(outs["rstd"]), _p(outs["sc"]),
                          _p(outs["sh"]), _p(wsb), _stream()), "bf_in_stats")
    torch.cuda.synchronize()
    ref = NB.in_stats(x, w, b, _exp_g(g, gdiv, Fr), _exp_g(gb, gdiv, Fr), SLICE[(dt, exp[1])][0] if kind == "sliced" else None)
    worst = {}
    for k, o in outs.items():
        worst[k] = NB.check(o[:Fr * C].view(Fr, C), *ref[k], f"{what} {k}", ("frame", "channel"))
        _tail(o, Fr * C, f"{what} {k}")
    if ws:
        _tail(wsb, nws, what + " workspace")
    return worst, what


def _note_stats(area, dt, res):
    worst, what = res
    for k, r in worst.items():
        _note(f"{area} {k}", dt, r, what)


def run_bwd(dt, Fr, S, C, kind, ws=True, with_g=False, gdiv=1, gelu=False, with_add=False, want=("dw", "db"), x=None, dy=None, wscale=1.0,
            seed=0, twice=False):
    """One bf_in_bwd call (given fp32 statistics, nonzero priors in every requested gradient) against the bound -> {output: worst ratio}."""
    h = L.lib()
    bf = dt == BF16
    exp = _expect(dt, S, C, ws)
    assert exp[0] == kind, (dt, S, C, ws, "takes", exp, "not", kind)
    what = f"bwd {dt} F{Fr} S{S} C{C} {exp} ws{int(ws)} g{int(with_g)} gdiv{gdiv} gelu{int(gelu)} add{int(with_add)} {'+'.join(want)}"
    x = _st(_randn(Fr, S, C, scale=1.5, shift=0.3, seed=seed) if x is None else x, dt)
    dy = _st(_randn(Fr, S, C, seed=seed + 1) if dy is None else dy, dt)
    add = _st(_randn(Fr, S, C, seed=seed + 2), dt) if with_add else None
    w, b = (_randn(C, scale=0.4, shift=1.0, seed=seed + 3) * wscale).float(), _randn(C, scale=0.5, seed=seed + 4).float()
    mean = x.mean(1).float()
    rstd = ((x.var(1, unbiased=False) + NB.EPS) ** -0.5).float()
    g = _film(Fr, gdiv, C, seed + 5, False)[0] if with_g else None
    ng = -(-Fr // gdiv)
    prior = {k: _randn(*((C,) if k in ("dw", "db") else (ng, C)), seed=seed + 6 + i).float() for i, k in enumerate(("dw", "db", "dg", "dgb")) if k in want}
    xd, dyd, addd = (_dev(None if t is None else t.to(dt)) for t in (x, dy, add))
    md, rd, wd, bd, gd = (_dev(t) for t in (mean, rstd, w, b, g))
    nws = h.bf_in_ws_floats(_dti(dt), Fr, S, C)
    ref = NB.in_bwd(dy, x, mean, rstd, w, b, _exp_g(g, gdiv, Fr), add, gelu, bf, exp[3])
    pg = NB.param_grads(ref["s1"], ref["s2"], w, b, g, gdiv, prior, gelu)

    def once():
        dx = _buf(Fr * S * C, dt)
        o = {k: _buf(prior[k].numel(), F32, prior[k]) for k in want}
        wsb = _buf(nws) if ws else None
        L.check(h.bf_in_bwd(_dti(dt), _p(dyd), _p(xd), _p(addd), _p(dx), Fr, S, C, _p(md), _p(rd), _p(wd), _p(bd), _p(gd), gdiv, int(gelu),
                            _p(o.get("dw")), _p(o.get("db")), _p(o.get("dg")), _p(o.get("dgb")), _p(wsb), _stream()), "bf_in_bwd")
        torch.cuda.synchronize()
        _tail(dx, Fr * S * C, what + " dx")
        for k in want:
            _tail(o[k], prior[k].numel(), f"{what} {k}")
        if ws:
            _tail(wsb, nws, what + " workspace")
        return dx, o

    dx, o = once()
    worst = {"dx": NB.check(dx[:Fr * S * C].view(Fr, S, C), *ref["dx"], what + " dx", ("frame", "row", "channel"))}
    for k in want:
        worst[k] = NB.check(o[k][:prior[k].numel()], *pg[k], f"{what} {k}", ("group", "channel"))
    if twice:
        dx2, o2 = once()
        assert torch.equal(dx[:Fr * S * C], dx2[:Fr * S * C])
        for k in want:
            assert torch.equal(o[k][:prior[k].numel()], o2[k][:prior[k].numel()]), (what, k, "differs from run to run")
    return worst, what


def _note_bwd(area, dt, res, ws=True):
    worst, what = res
    for k, r in worst.items():
        _note(f"{area} dx" if k == "dx" else f"param grads ({'workspace' if ws else 'atomic'}) {k}", dt, r, what)


def s_edges(dt, wide):
    srows, brows = SLICE[(dt, wide)]
    rg, cached = RG[dt], CACHED[dt]
    return [1, rg - 1, rg, rg + 1, cached, cached + 1, brows + 1, 4 * srows + 5, 8 * srows + 1, 4 * brows + 7, 8 * brows + 1]


# ---------------------------------------------------------------------------------------------------- S and C edges
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C", [40, 96, 192])
def test_stats_frame_length_edges(dt, C):
    """1, RG - 1, RG, RG + 1 rows; the cached length and one more (two slices, or three in the wide geometry, the last of one row); one
    backward slice + 1; 5 and 9 slices of either kind with a ragged last one (the 4-lane merge loops take a second and a third turn)."""
    wide = C % 96 == 0
    for S in s_edges(dt, wide):
        kind = "cached" if S <= CACHED[dt] else "sliced"
        Fr = 3 if S <= 1000 else 2
        _note_stats(f"stats ({kind}{', wide' if wide and kind == 'sliced' else ''})", dt, run_stats(dt, Fr, S, C, kind, seed=S))
        if S > CACHED[dt] and S <= 1000:
            _note_stats("stats (uncached, ws = NULL)", dt, run_stats(dt, Fr, S, C, "uncached", ws=False, seed=S))
    srows = SLICE[(dt, wide)][0]
    assert _expect(dt, CACHED[dt] + 1, C)[2] == (3 if wide else 2) and (CACHED[dt] + 1) % srows == 1
    assert _expect(dt, 4 * srows + 5, C)[2] == 5 and _expect(dt, 8 * srows + 1, C)[2] == 9


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C", [40, 96, 192])
@pytest.mark.parametrize("gelu", [False, True])
def test_bwd_frame_length_edges(dt, C, gelu):
    wide = C % 96 == 0
    for S in s_edges(dt, wide):
        kind = "cached" if S <= CACHED[dt] else "sliced"
        Fr = 3 if S <= 1000 else 2
        r = run_bwd(dt, Fr, S, C, kind, gelu=gelu, with_add=S % 2 == 1, seed=S)
        _note_bwd(f"bwd ({kind}{', wide' if wide and kind == 'sliced' else ''})", dt, r)
        if S <= 1000:
            r = run_bwd(dt, Fr, S, C, "cached" if S <= CACHED[dt] else "uncached", ws=False, gelu=gelu, with_add=S % 2 == 0, seed=S)
            _note_bwd(f"bwd ({'cached' if S <= CACHED[dt] else 'uncached'}, ws = NULL)", dt, r, ws=False)
    brows = SLICE[(dt, wide)][1]
    assert _expect(dt, brows + 1, C)[3] == 2 and _expect(dt, 4 * brows + 7, C)[3] == 5 and _expect(dt, 8 * brows + 1, C)[3] == 9


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C", ["chunk", 40, 64, 72, 96, 192, 288])
def test_channel_count_edges(dt, C):
    """One chunk, a partly filled block, whole blocks, 72 (a second block of one / two chunk lanes), and the multiples of 96."""
    C = (8 if dt == BF16 else 4) if C == "chunk" else C
    for S, kind in ((37, "cached"), (CACHED[dt] + 5, "sliced")):
        _note_stats(f"stats ({kind})", dt, run_stats(dt, 3, S, C, kind, film="g+gb", gdiv=2, seed=C))
        _note_bwd(f"bwd ({kind})", dt, run_bwd(dt, 3, S, C, kind, with_g=True, gdiv=2, gelu=True, with_add=True, seed=C))
        k2 = "cached" if kind == "cached" else "uncached"
        _note_stats(f"stats ({k2}, ws = NULL)", dt, run_stats(dt, 3, S, C, k2, ws=False, seed=C + 1))
        _note_bwd(f"bwd ({k2}, ws = NULL)", dt, run_bwd(dt, 3, S, C, k2, ws=False, with_g=True, gdiv=2, want=("dw", "db", "dg", "dgb"), seed=C + 1), ws=False)


# ---------------------------------------------------------------------------------------------------- FiLM arguments
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("gdiv", [1, 2, 5])
def test_stats_film_arguments(dt, gdiv):
    """g alone and g + gb; 5 frames in groups of 2 leave a ragged last group."""
    for film in ("g", "g+gb"):
        for S, kind in ((37, "cached"), (CACHED[dt] + 5, "sliced")):
            _note_stats(f"stats ({kind})", dt, run_stats(dt, 5, S, 72, kind, film=film, gdiv=gdiv, seed=gdiv))
        _note_stats("stats (uncached, ws = NULL)", dt, run_stats(dt, 5, CACHED[dt] + 5, 72, "uncached", ws=False, film=film, gdiv=gdiv, seed=gdiv))


WANTS = [("dg",), ("dgb",), ("dg", "dgb"), ("dw", "db", "dg", "dgb"), ("dw", "dg"), ("dw", "db")]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("gdiv", [1, 2, 5])
@pytest.mark.parametrize("ws", [True, False])
def test_bwd_film_arguments(dt, gdiv, ws):
    """dg / dgb each alone, together, with and without dw / db, every one on nonzero prior contents; with and without `add`; on the
    workspace path the grouped reduction (one workgroup per group, workgroup row 0 redoing dw / db over all frames), without one the
    float atomics."""
    for i, want in enumerate(WANTS):
        for S, kind in ((37, "cached"), (CACHED[dt] + 5, "sliced" if ws else "uncached")):
            r = run_bwd(dt, 5, S, 72, kind, ws=ws, with_g=True, gdiv=gdiv, with_add=i % 2 == 0, want=want, seed=10 * gdiv + i)
            _note_bwd(f"bwd ({kind})", dt, r, ws)
    for S, kind in ((37, "cached"), (CACHED[dt] + 5, "sliced" if ws else "uncached")):
        r = run_bwd(dt, 5, S, 72, kind, ws=ws, with_g=True, gdiv=gdiv, gelu=True, with_add=True, want=("dw", "db"), seed=gdiv)
        _note_bwd(f"bwd ({kind})", dt, r, ws)
        r = run_bwd(dt, 5, S, 72, kind, ws=ws, with_g=False, gdiv=gdiv, want=("dw", "db", "dg", "dgb"), seed=gdiv)      # g = NULL, groups asked for
        _note_bwd(f"bwd ({kind})", dt, r, ws)


# ---------------------------------------------------------------------------------------------------- many frames
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Fr,gdiv,want", [(130, 1, ("dw", "db")), (250, 120, ("dw", "db", "dg", "dgb")), (130, 3, ("dw", "db", "dg", "dgb")),
                                          (250, 120, ("dg",))])
def test_many_frames(dt, Fr, gdiv, want):
    """in_reduce_block with 16 frame lanes: 130 frames ungrouped are one eight-deep batch (lanes 0 and 1) plus a tail; groups of 120, 120
    and 10 send a grouped workgroup through the batch loop and workgroup row 0 through the redo pass over all 250 frames; groups of 3 are
    44 workgroup rows of a tail alone.  Fixed order: two runs agree bit for bit.  The atomic path is held to the same bound."""
    with_g = gdiv > 1
    r = run_bwd(dt, Fr, 4, 72, "cached", with_g=with_g, gdiv=gdiv, want=want, seed=Fr + gdiv, twice=True)
    _note_bwd("bwd (many frames)", dt, r)
    r = run_bwd(dt, Fr, 4, 72, "cached", ws=False, with_g=with_g, gdiv=gdiv, want=want, seed=Fr + gdiv)
    _note_bwd("bwd (many frames, ws = NULL)", dt, r, ws=False)


# ---------------------------------------------------------------------------------------------------- hard inputs
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", ["large_mean", "constant", "scales"])
def test_stats_hard_inputs(dt, kind):
    """|mean| / std of 1000 (fp32) or 33 (bf16), where sh loses ~ u |mean| / std by construction; a channel of variance 0 (rstd =
    eps^-1/2); channels six decades apart inside one chunk."""
    Fr, C = 3, 72
    for S, path, ws in ((60, "cached", True), (CACHED[dt] + 7, "sliced", True), (CACHED[dt] + 7, "uncached", False)):
        if kind == "large_mean":
            x = _randn(Fr, S, C, scale=1.0, shift=1000.0, seed=1) if dt == F32 else _randn(Fr, S, C, scale=3.0, shift=100.0, seed=1)
        elif kind == "constant":
            x = _randn(Fr, S, C, seed=2)
            x[:, :, 3] = 0.7
            x[:, :, 64] = -3.0
        else:
            x = _randn(Fr, S, C, seed=3) * (10.0 ** torch.linspace(-3, 3, C, dtype=torch.float64)[torch.randperm(C, generator=torch.Generator().manual_seed(4))])
        res = run_stats(dt, Fr, S, C, path, ws=ws, film="g+gb", gdiv=2, x=x, seed=5)
        _note_stats(f"stats hard inputs ({kind})", dt, res)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", ["dy_const", "dy_xhat", "clamp"])
def test_bwd_hard_inputs(dt, kind):
    """dy constant over a frame (dx cancels to ~0 through s1), dy proportional to xhat (through s2), GELU arguments either side of the
    polynomial's clamp at |z| = 4."""
    Fr, C = 3, 72
    for S, path, ws in ((60, "cached", True), (CACHED[dt] + 7, "sliced", True), (CACHED[dt] + 7, "uncached", False)):
        x = _st(_randn(Fr, S, C, scale=1.5, shift=0.3, seed=7), dt)
        xh = (x - x.mean(1, keepdim=True)) * (x.var(1, unbiased=False, keepdim=True) + NB.EPS) ** -0.5
        if kind == "dy_const":
            dy = _randn(Fr, 1, C, seed=8).expand(Fr, S, C).contiguous()
        elif kind == "dy_xhat":
            dy = xh * 0.5
        else:
            dy = None
        r = run_bwd(dt, Fr, S, C, path, ws=ws, gelu=kind == "clamp", wscale=2.5 if kind == "clamp" else 1.0, x=x, dy=dy, seed=7)
        _note_bwd(f"bwd hard inputs ({kind})", dt, r, ws)


# ---------------------------------------------------------------------------------------------------- merge of given partials
@pytest.mark.parametrize("dt,C", [(F32, 40), (BF16, 96)])
@pytest.mark.parametrize("rows", [128, 256])
def test_merge_slices_of_given_partials(dt, C, rows):
    """bf_in_stats_merge_slices on partials the test wrote in the documented layout ({mean, M2} pairs at ws + 2 F C, [frame][slice][C]),
    a ragged last slice, g and gb given; workspace of exactly bf_in_ws_floats floats."""
    h = L.lib()
    Fr, gdiv = 3, 2
    S = 5 * rows + 9
    N = -(-S // rows)
    assert _expect(dt, S, C)[0] == "sliced" and N > 4
    pm, pq = _randn(Fr, N, C, scale=0.2, shift=0.5, seed=1).float(), (_randn(Fr, N, C, seed=2).abs() * rows).float()
    w, b = _randn(C, shift=1.0, scale=0.3, seed=3).float(), _randn(C, seed=4).float()
    g, gb = _film(Fr, gdiv, C, 5)
    nws = h.bf_in_ws_floats(_dti(dt), Fr, S, C)
    assert nws >= 2 * Fr * C * (1 + N)
    wsb = _buf(nws)
    wsb[2 * Fr * C:2 * Fr * C * (1 + N)] = torch.stack([pm, pq], -1).reshape(-1).to(DEV)
    outs = {k: _buf(Fr * C) for k in ("mean", "rstd", "sc", "sh")}
    wd, bd, gd, gbd = (_dev(t) for t in (w, b, g, gb))
    rc = h.bf_in_stats_merge_slices(_dti(dt), Fr, S, C, rows, _p(wd), _p(bd), _p(gd), gdiv, _p(gbd), _p(outs["mean"]), _p(outs["rstd"]),
                                    _p(outs["sc"]), _p(outs["sh"]), _p(wsb), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    ref = NB.merge(pm, pq, rows, S, w, b, _exp_g(g, gdiv, Fr), _exp_g(gb, gdiv, Fr))
    for k, o in outs.items():
        _note(f"merge of given partials {k}", dt, NB.check(o[:Fr * C].view(Fr, C), *ref[k], f"merge {dt} rows{rows} {k}", ("frame", "channel")), f"rows{rows}")
        _tail(o, Fr * C, f"merge {k}")
    _tail(wsb, nws, "merge workspace")


def test_merge_slices_declines_more_slices_than_the_workspace_holds():
    """bf16, 40 channels: the workspace is sized for 192-row slices; 400 rows in 128-row slices are four where it holds three."""
    h = L.lib()
    Fr, S, C = 2, 400, 40
    wsb = _buf(h.bf_in_ws_floats(L.BF_DTYPE_BF16, Fr, S, C), init=torch.zeros(1))
    outs = [_buf(Fr * C) for _ in range(4)]
    w = torch.ones(C, device=DEV)
    rc = h.bf_in_stats_merge_slices(L.BF_DTYPE_BF16, Fr, S, C, 128, _p(w), _p(w), None, 1, None, *[_p(o) for o in outs], _p(wsb), _stream())
    torch.cuda.synchronize()
    assert rc == 1
    assert all(torch.isnan(o).all() for o in outs)


# ---------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("dt", DTS)
def test_channel_counts_off_the_chunk_are_refused(dt):
    """C = 12 (bf16) / 6 (fp32) is an error for all five entry points, on the one-workgroup and the sliced paths, and writes nothing;
    so is dg / dgb behind a GELU, whose group gradients the kernels' two sums do not give."""
    h = L.lib()
    C = 12 if dt == BF16 else 6
    Fr = 2
    for S in (20, CACHED[dt] + 5):
        n = Fr * S * C
        xd = torch.ones(n + 64, dtype=dt, device=DEV)
        v = torch.ones(Fr * C + 64, device=DEV)
        outs = [_buf(Fr * C) for _ in range(4)]
        wsb = _buf(4 * Fr * C * (2 + S // 48))
        big = _buf(n, dt)
        grads = [_buf(Fr * C) for _ in range(4)]
        for use_ws in (wsb, None):
            assert h.bf_in_stats(_dti(dt), _p(xd), Fr, S, C, _p(v), _p(v), None, 1, None, *[_p(o) for o in outs], _p(use_ws), _stream()) < 0
            assert h.bf_in_bwd(_dti(dt), _p(xd), _p(xd), None, _p(big), Fr, S, C, _p(v), _p(v), _p(v), _p(v), None, 1, 0, *[_p(o) for o in grads],
                               _p(use_ws), _stream()) < 0
        assert h.bf_in_stats_merge_slices(_dti(dt), Fr, S, C, 128, _p(v), _p(v), None, 1, None, *[_p(o) for o in outs], _p(wsb), _stream()) < 0
        assert h.bf_affine_apply(_dti(dt), _p(xd), None, _p(v), _p(v), _p(big), Fr * S, S, C, _stream()) < 0
        assert h.bf_colsum(_dti(dt), _p(xd), Fr * S, C, None, _p(outs[0]), _stream()) < 0
        # a chunk-multiple C, but the group gradients behind a GELU
        C2 = 8
        assert h.bf_in_bwd(_dti(dt), _p(xd), _p(xd), None, _p(big), Fr, S, C2, _p(v), _p(v), _p(v), _p(v), None, 1, 1, None, None, _p(grads[2]),
                           _p(grads[3]), _p(wsb), _stream()) < 0
        torch.cuda.synchronize()
        for o in outs + grads + [wsb, big]:
            assert torch.isnan(o.float()).all(), "a refused call wrote to an output"


# ---------------------------------------------------------------------------------------------------- apply
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("resid", [False, True])
@pytest.mark.parametrize("sh", [False, True])
def test_affine_apply(dt, resid, sh):
    h = L.lib()
    Fr, S, C = 3, 37, 72
    z, r = _st(_randn(Fr, S, C, seed=1), dt), _st(_randn(Fr, S, C, seed=2), dt)
    sc, shv = _randn(Fr, C, shift=1.0, scale=0.3, seed=3).float(), _randn(Fr, C, seed=4).float()
    out = _buf(Fr * S * C, dt)
    zd, rd, scd, shd = _dev(z.to(dt)), _dev(r.to(dt)), _dev(sc), _dev(shv)
    L.check(h.bf_affine_apply(_dti(dt), _p(zd), _p(rd) if resid else None, _p(scd), _p(shd) if sh else None, _p(out), Fr * S, S, C, _stream()), "bf_affine_apply")
    torch.cuda.synchronize()
    ref = NB.affine_apply(z, sc, shv if sh else None, r if resid else None, dt == BF16)
    _note("apply", dt, NB.check(out[:Fr * S * C].view(Fr, S, C), *ref, f"apply {dt} resid{resid} sh{sh}", ("frame", "row", "channel")), f"resid{resid} sh{sh}")
    _tail(out, Fr * S * C, "apply")


@pytest.mark.parametrize("dt", DTS)
def test_affine_apply_grid_stride_wraps(dt):
    """The grid is capped at 4096 workgroups of 256 threads: 256 frames of 4099 one-chunk rows are 768 chunks more, so the first 768
    threads take a second turn."""
    h = L.lib()
    C = 8 if dt == BF16 else 4
    Fr, S = 256, 4099
    assert Fr * S > 4096 * 256 and Fr * S < 4096 * 256 + 4096
    z, r = _st(_randn(Fr, S, C, seed=1), dt), _st(_randn(Fr, S, C, seed=2), dt)
    sc, shv = _randn(Fr, C, shift=1.0, scale=0.3, seed=3).float(), _randn(Fr, C, seed=4).float()
    out = _buf(Fr * S * C, dt)
    zd, rd, scd, shd = _dev(z.to(dt)), _dev(r.to(dt)), _dev(sc), _dev(shv)
    L.check(h.bf_affine_apply(_dti(dt), _p(zd), _p(rd), _p(scd), _p(shd), _p(out), Fr * S, S, C, _stream()), "bf_affine_apply")
    torch.cuda.synchronize()
    ref = NB.affine_apply(z, sc, shv, r, dt == BF16)
    _note("apply", dt, NB.check(out[:Fr * S * C].view(Fr, S, C), *ref, f"apply wrap {dt}", ("frame", "row", "channel")), "grid-stride wrap")
    _tail(out, Fr * S * C, "apply wrap")


# ---------------------------------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("nrows,C,split", [(5, 72, (64, 1)), (63, 72, (64, 1)), (130, 72, (64, 3)), (20000, 72, (64, 313)), (70000, "chunk", (69, 1015))])
def test_colsum(dt, nrows, C, split):
    """Fewer rows than a block takes, a ragged last block (130 = 2 * 64 + 2), more than 64 rows per block; scale given and NULL; a
    nonzero prior."""
    h = L.lib()
    C = (8 if dt == BF16 else 4) if C == "chunk" else C
    assert NB.colsum_split(nrows, C) == split
    x = _st(_randn(nrows, C, shift=0.2, seed=nrows), dt)
    xd = _dev(x.to(dt))
    scale, prior = _randn(C, seed=1).float(), _randn(C, seed=2).float()
    for sc in (None, scale):
        out = _buf(C, F32, prior)
        scd = _dev(sc)
        L.check(h.bf_colsum(_dti(dt), _p(xd), nrows, C, _p(scd), _p(out), _stream()), "bf_colsum")
        torch.cuda.synchronize()
        _note("colsum", dt, NB.check(out[:C], *NB.colsum(x, sc, prior), f"colsum {dt} {nrows}x{C} scale{sc is not None}", ("channel",)), f"{nrows}x{C}")
        _tail(out, C, "colsum")


# ---------------------------------------------------------------------------------------------------- the wrappers
def test_kernels_wrappers_take_priors_and_group_gradients():
    """kernels.in_stats(use_ws=) and kernels.in_bwd(dw=, db=, dg=, dgb=): the tensors given are accumulated into; the defaults return what
    they returned before (fresh dw / db, no group gradients)."""
    from bubbleformer_amd import kernels as K
    Fr, S, C, gdiv = 5, 37, 72, 2
    x, dy = _randn(Fr, S, C, seed=1).float(), _randn(Fr, S, C, seed=2).float()
    w, b = _randn(C, shift=1.0, scale=0.3, seed=3).float(), _randn(C, seed=4).float()
    g = _film(Fr, gdiv, C, 5, False)[0]
    xd, dyd, wd, bd, gd = (_dev(t) for t in (x, dy, w, b, g))
    mean, rstd, _, _ = K.in_stats(xd, Fr, S, C, wd, bd, use_ws=False)
    m2, r2, _, _ = K.in_stats(xd, Fr, S, C, wd, bd)
    assert torch.equal(mean, m2) and torch.equal(rstd, r2)
    prior = {k: _randn(*((C,) if k in ("dw", "db") else (3, C)), seed=6 + i).float() for i, k in enumerate(("dw", "db", "dg", "dgb"))}
    o = {k: _dev(v.clone()) for k, v in prior.items()}
    dx, dw, db = K.in_bwd(dyd, xd, Fr, S, C, mean, rstd, wd, bd, g=gd, gdiv=gdiv, **o)
    assert dw is o["dw"] and db is o["db"]
    ref = NB.in_bwd(dy, x, mean.cpu(), rstd.cpu(), w, b, _exp_g(g, gdiv, Fr))
    pg = NB.param_grads(ref["s1"], ref["s2"], w, b, g, gdiv, prior)
    NB.check(dx, *ref["dx"], "wrapper dx", ("frame", "row", "channel"))
    for k in o:
        NB.check(o[k], *pg[k], "wrapper " + k, ("group", "channel"))
    dx0, dw0, db0 = K.in_bwd(dyd, xd, Fr, S, C, mean, rstd, wd, bd, g=gd, gdiv=gdiv)
    pg0 = NB.param_grads(ref["s1"], ref["s2"], w, b, g, gdiv)
    assert torch.equal(dx0, dx)
    NB.check(dw0, *pg0["dw"], "wrapper default dw", ("channel",))
    NB.check(db0, *pg0["db"], "wrapper default db", ("channel",))


# ---------------------------------------------------------------------------------------------------- report
def test_report_worst_ratios(capsys):
    """Last in the module: prints the worst |got - ref| / bound of each area the tests above reached (all are <= 1, or they failed)."""
    assert all(r <= 1.0 for r, _ in WORST.values())
    with capsys.disabled():
        print("\nworst |got - ref| / bound per area:")
        for area, (r, case) in sorted(WORST.items()):
            print(f"  {area:52s} {r:.3e}  ({case})")
