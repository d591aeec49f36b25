"""GPU: the BatchNorm2d / GELU / max-pool kernels of bn.hip at their edges, every output element held to the per-element bound of
tests/bn_bounds.py, through the C ABI (bf_bn_fwd, bf_bn_eval, bf_bn_act, bf_bn_bwd, bf_bn_ws_floats) in both dtypes.

Pixel counts from 2 to 263169 and channel counts from 1 to 512: idle channel lanes (CW > C), a second channel block of one channel, the
`want` cap on the slab count, used < slabs (coef lives behind the slabs that are written, the workspace is sized by all of them), the
second trip of slab_sums (more than 256 slabs), a last slab shorter than the row threads, odd frames whose partial windows are activated
but not pooled; running statistics given and NULL; dA alone, dP alone, both, dA as a channel slice of a wider NaN-filled buffer (offA = 5,
ldA = C + 7, the base pointer passed), accumulate = 1 on nonzero priors and 0 on NaN priors, index bytes from the forward and hand-made;
badly scaled, constant, tying and cancelling inputs; NaN and +inf in pool windows; the eval affine; refusals that write nothing; NaN tails
behind every float output, a fixed byte behind idx, and a workspace of exactly bf_bn_ws_floats floats.  The kernels carry no per-path
profiler names, so each case states the (slabs, used, pixels in the last slab) it expects and asserts bn_bounds' restatement and the
library's own bf_bn_ws_floats against it.  The last test prints the worst |got - ref| / bound of each area."""
import math

import pytest
import torch

from bubbleformer_amd import _lib as L
from tests import bn_bounds as BB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
DTS = [F32, BF16]
TAIL = 64
NAN = float("nan")
IDX_FILL = 0xA5
MOM = 0.1
WORST = {}
NAMES4 = ("frame", "y", "x", "channel")

# (B, H, W, C) -> (slabs, used, pixels in the last slab), and what the shape is there for
PLAN = {
    (1, 1, 2, 1): (1, 1, 2),              # the smallest training input: n / (n - 1) = 2
    (1, 2, 2, 33): (1, 1, 4),             # the smallest pooled frame; CW = 64, 31 channel lanes idle
    (2, 5, 7, 3): (1, 1, 70),             # odd frame, CW = 4 > C
    (3, 5, 7, 20): (3, 3, 35),            # odd frame, CW = 32 > C, three slabs
    (1, 3, 107, 64): (20, 19, 15),        # used < slabs
    (1, 65, 67, 64): (272, 257, 3),       # second trip of slab_sums; the last slab has 3 pixels for 4 row threads
    (1, 65, 67, 65): (272, 257, 3),       # the same with a second channel block of one channel (gx = 2)
    (1, 65, 67, 512): (256, 242, 17),     # the `want` cap: 2048 / 8 channel blocks
    (1, 513, 513, 1): (257, 257, 769),    # one channel, 256 row threads, second trip
}


def _note(area, dt, ratio, case):
    area = f"{area}, {'bf16' if dt == BF16 else 'fp32'}"
    if ratio >= WORST.get(area, (-1.0, ""))[0]:
        WORST[area] = (ratio, case)


def _dti(dt):
    return L.BF_DTYPE_BF16 if dt == BF16 else L.BF_DTYPE_F32


def _buf(n, dt=F32, init=None):
    """n elements (NaN, or `init`) followed by a NaN tail no kernel may touch."""
    b = torch.full((n + TAIL,), NAN, dtype=dt, device=DEV)
    if init is not None:
        b[:n] = init.reshape(-1).to(dt).to(DEV)
    return b


def _ibuf(n):
    return torch.full((n + TAIL,), IDX_FILL, dtype=torch.uint8, device=DEV)


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _tail(b, n, what):
    if b.dtype == torch.uint8:
        assert bool((b[n:] == IDX_FILL).all()), (what, "wrote past its extent")
    else:
        assert torch.isnan(b[n:].float()).all(), (what, "wrote past its extent")


def _untouched(bufs, what):
    torch.cuda.synchronize()
    for b in bufs:
        ok = bool((b == IDX_FILL).all()) if b.dtype == torch.uint8 else bool(torch.isnan(b.float()).all())
        assert ok, (what, "a refused call wrote to an output")


def _expect(shape):
    """The plan a shape must take -> bn_bounds.plan(), checked against the table above and the library's own workspace size."""
    B, H, W, C = shape
    M = B * H * W
    p = BB.plan(M, C)
    if shape in PLAN:
        assert (p["slabs"], p["used"], p["last"]) == PLAN[shape], (shape, p)
    n = L.lib().bf_bn_ws_floats(M, C)
    assert n == 4 * p["slabs"] * C + 2 * C == BB.ws_floats(M, C), (shape, n)
    return p


def _dev(t, dt=None):
    return None if t is None else (t if dt is None else t.to(dt)).to(DEV)


# ---------------------------------------------------------------------------------------------------- runners
def run_fwd(dt, x, gamma, beta, running=True, seed=0, what=""):
    """One bf_bn_fwd call against the bound -> (the kernel's fp32 mean / rstd / sc / sh (C,) on the host, {output: worst ratio})."""
    h = L.lib()
    B, H, W, C = x.shape
    M = B * H * W
    _expect(tuple(x.shape))
    what = f"fwd {dt} {tuple(x.shape)} running{int(running)} {what}"
    xd, gd, bd = _dev(x, dt), _dev(gamma), _dev(beta)
    rm = BB.randn(C, scale=0.5, seed=seed + 300).float() if running else None
    rv = (BB.randn(C, seed=seed + 301).abs() + 0.5).float() if running else None
    o = dict(mean=_buf(C), rstd=_buf(C), sc=_buf(B * C), sh=_buf(B * C))
    rmb, rvb = (_buf(C, F32, rm), _buf(C, F32, rv)) if running else (None, None)
    nbt = torch.tensor([5, -77], dtype=torch.int64, device=DEV) if running else None
    nws = h.bf_bn_ws_floats(M, C)
    ws = _buf(nws)
    L.check(h.bf_bn_fwd(_dti(dt), _p(xd), B, H * W, C, _p(gd), _p(bd), BB.EPS32, MOM, _p(rmb), _p(rvb), _p(nbt), _p(o["mean"]), _p(o["rstd"]),
                        _p(o["sc"]), _p(o["sh"]), _p(ws), _stream()), "bf_bn_fwd")
    torch.cuda.synchronize()
    ref = BB.stats(xd.double(), gamma, beta, rm, rv, BB.EPS32, MOM)
    worst = {}
    for k in ("mean", "rstd", "sc", "sh"):
        worst[k] = BB.check(o[k][:C], *ref[k], f"{what} {k}", ("channel",))
    for k in ("sc", "sh"):
        fr = o[k][:B * C].view(B, C)
        assert bool((fr == fr[0]).all()), (what, k, "differs from frame to frame")
        _tail(o[k], B * C, f"{what} {k}")
    _tail(o["mean"], C, what + " mean"), _tail(o["rstd"], C, what + " rstd"), _tail(ws, nws, what + " workspace")
    if running:
        worst["rm"] = BB.check(rmb[:C], *ref["rm"], what + " running_mean", ("channel",))
        worst["rv"] = BB.check(rvb[:C], *ref["rv"], what + " running_var", ("channel",))
        _tail(rmb, C, what + " running_mean"), _tail(rvb, C, what + " running_var")
        assert nbt.tolist() == [6, -77], (what, "num_batches_tracked", nbt.tolist())
    for k, r in worst.items():
        _note({"rm": "running_mean", "rv": "running_var"}.get(k, k), dt, r, what)
    return tuple(o[k][:C].cpu() for k in ("mean", "rstd", "sc", "sh")), worst


def run_act(dt, x, sc, sh, pool, what="", finite=True):
    """One bf_bn_act call: `a` against the bound, p / idx exactly F.max_pool2d's on the stored a -> (a, p, idx) on the host."""
    h = L.lib()
    B, H, W, C = x.shape
    n, Hp, Wp = B * H * W * C, H // 2, W // 2
    npool = B * Hp * Wp * C
    what = f"act {dt} {tuple(x.shape)} pool{int(pool)} {what}"
    xd = _dev(x, dt)
    scd, shd = _dev(sc.repeat(B)), _dev(sh.repeat(B))
    a = _buf(n, dt)
    p, idx = (_buf(npool, dt), _ibuf(npool)) if pool else (None, None)
    L.check(h.bf_bn_act(_dti(dt), _p(xd), B, H, W, C, _p(scd), _p(shd), _p(a), _p(p), _p(idx), _stream()), "bf_bn_act")
    torch.cuda.synchronize()
    ref, bnd = BB.act(xd.double(), sc, sh, dt == BF16)
    got = a[:n].view(B, H, W, C)
    if not finite:                                          # NaN / inf elements are compared by class, the rest by bound
        g64 = got.double()
        assert torch.equal(torch.isnan(g64), torch.isnan(ref)) and torch.equal(g64 == float("inf"), ref == float("inf")), what
        assert not bool((g64 == float("-inf")).any()) and not bool((ref == float("-inf")).any())
        bad = ~torch.isfinite(ref)
        assert int(bad.sum()) > 0
        got, ref, bnd = torch.where(bad, 0.0, g64), torch.where(bad, 0.0, ref), torch.where(bad, 1.0, bnd)
    _note("a", dt, BB.check(got, ref, bnd, what, NAMES4), what)
    _tail(a, n, what + " a")
    ac = a[:n].view(B, H, W, C).cpu()
    if not pool:
        return ac, None, None
    pw, iw = BB.pool_of_stored(ac)
    pc, ic = p[:npool].view(B, Hp, Wp, C).cpu(), idx[:npool].view(B, Hp, Wp, C).cpu()
    assert torch.equal(torch.isnan(pc.double()), torch.isnan(pw)), what
    assert torch.equal(torch.nan_to_num(pc.double(), nan=0.0), torch.nan_to_num(pw, nan=0.0)), (what, "p is not the maximum of the stored a")
    assert torch.equal(ic, iw), (what, "idx is not F.max_pool2d's window position", int((ic != iw).sum()))
    _tail(p, npool, what + " p"), _tail(idx, npool, what + " idx")
    return ac, pc, ic


def run_bwd(dt, x, gamma, st, dA=None, dP=None, idx=None, sliced=False, prior=None, what=""):
    """One bf_bn_bwd call against the bound.  st: the given fp32 (mean, rstd, sc, sh); sliced: dA is passed as the base pointer of a wider
    NaN-filled buffer with offA = 5, ldA = C + 7; prior: (dgamma, dbeta) for accumulate = 1, None for accumulate = 0 on NaN contents.
    -> (dx, dgamma, dbeta) device tensors."""
    h = L.lib()
    B, H, W, C = x.shape
    M = B * H * W
    n = M * C
    _expect(tuple(x.shape))
    what = (f"bwd {dt} {tuple(x.shape)} dA{int(dA is not None)} dP{int(dP is not None)} offA{BB.OFFA if sliced else 0} "
            f"acc{int(prior is not None)} {what}")
    xd, gd = _dev(x, dt), _dev(gamma)
    B_ = st[2].numel() // C
    md, rd, scd, shd = (_dev(t) for t in st)
    if B_ == 1:
        scd, shd = scd.repeat(B), shd.repeat(B)
    dAd, ldA, offA = None, C, 0
    if dA is not None:
        if sliced:
            dAd, ldA, offA = _dev(BB.wide(dA)), C + BB.PADA, BB.OFFA
        else:
            dAd = _dev(dA, F32)
    dPd, idxd = _dev(dP, dt), _dev(idx)
    dx = _buf(n, dt)
    dg, db = (_buf(C, F32, prior[0]), _buf(C, F32, prior[1])) if prior is not None else (_buf(C), _buf(C))
    nws = h.bf_bn_ws_floats(M, C)
    ws = _buf(nws)
    L.check(h.bf_bn_bwd(_dti(dt), _p(dAd), ldA, offA, _p(dPd), _p(idxd), _p(xd), B, H, W, C, _p(gd), _p(md), _p(rd), _p(scd), _p(shd), _p(dx), _p(dg),
                        _p(db), int(prior is not None), _p(ws), _stream()), "bf_bn_bwd")
    torch.cuda.synchronize()
    ref = BB.bwd(_dev(dA), None if dP is None else dPd.double(), idxd, xd.double(), gamma, *st, *(prior or (None, None)), bf16=dt == BF16)
    _note("dx", dt, BB.check(dx[:n].view(B, H, W, C), *ref["dx"], what + " dx", NAMES4), what)
    _note("dgamma", dt, BB.check(dg[:C], *ref["dgamma"], what + " dgamma", ("channel",)), what)
    _note("dbeta", dt, BB.check(db[:C], *ref["dbeta"], what + " dbeta", ("channel",)), what)
    _tail(dx, n, what + " dx"), _tail(dg, C, what + " dgamma"), _tail(db, C, what + " dbeta"), _tail(ws, nws, what + " workspace")
    return dx[:n], dg[:C], db[:C]


def _chain(dt, x, gamma, beta, seed=0, what="", dA=None, dP=None):
    """Forward with the running statistics, activation + pool (index bytes for the backward), backward with both gradients."""
    B, H, W, C = x.shape
    st, _ = run_fwd(dt, x, gamma, beta, True, seed, what)
    a, p, idx = run_act(dt, x, st[2], st[3], True, what)
    dA0, dP0 = BB.grads(B, H, W, C, dt == BF16, seed)
    dA, dP = dA0 if dA is None else dA(st), dP0 if dP is None else dP(st)
    run_bwd(dt, x, gamma, st, dA, dP, idx, what=what)
    return st, idx


# ---------------------------------------------------------------------------------------------------- edge shapes
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", list(PLAN))
def test_edge_shapes(dt, shape):
    """Every entry point on every plan of the table: statistics with and without the running pair; the activation without and with the
    pool (odd H / W: partial windows activated but not pooled; 2100 and 720 elements are no multiple of 256); the backward with dA alone,
    dP alone, both, dA as a channel slice at offA = 5, accumulate = 1 on nonzero priors (every other call: accumulate = 0 on NaN)."""
    B, H, W, C = shape
    bf = dt == BF16
    x, gamma, beta, dA, dP = BB.edge_input(shape, bf)
    st, _ = run_fwd(dt, x, gamma, beta, True, C)
    st2, _ = run_fwd(dt, x, gamma, beta, False, C)
    assert all(torch.equal(u, v) for u, v in zip(st, st2))
    run_act(dt, x, st[2], st[3], False)
    run_bwd(dt, x, gamma, st, dA)
    run_bwd(dt, x, gamma, st, dA, sliced=True, prior=BB.priors(C))
    if H < 2 or W < 2:
        return
    a, p, idx = run_act(dt, x, st[2], st[3], True)
    run_bwd(dt, x, gamma, st, None, dP, idx)
    run_bwd(dt, x, gamma, st, dA, dP, idx)
    run_bwd(dt, x, gamma, st, dA, dP, idx, sliced=True, prior=BB.priors(C, 1))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [(3, 5, 7, 20), (2, 4, 6, 33)])
def test_hand_made_index_bytes(dt, shape):
    """The routing apart from the forward: random index bytes, which need not name a maximum."""
    B, H, W, C = shape
    x = BB.stored(BB.randn(B, H, W, C, scale=1.5, shift=0.3, seed=9), dt == BF16)
    gamma, beta = BB.params(C, 9)
    st = BB.given_stats(x, gamma, beta)
    dA, dP = BB.grads(B, H, W, C, dt == BF16, 9)
    idx = torch.randint(0, 4, dP.shape, generator=torch.Generator().manual_seed(9), dtype=torch.uint8)
    run_bwd(dt, x, gamma, st, None, dP, idx, what="hand-made idx")
    run_bwd(dt, x, gamma, st, dA, dP, idx, what="hand-made idx")


# ---------------------------------------------------------------------------------------------------- value cases
VSHAPES = [(3, 5, 7, 20), (1, 65, 67, 64)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", VSHAPES)
@pytest.mark.parametrize("kind", ["large_mean", "constant", "scales", "ties"])
def test_value_cases(dt, shape, kind):
    """|mean| / std = 1000 (fp32; 33 in bf16, the largest ratio its 8 bits store distinctly); a constant channel (var = 0 exactly, rstd =
    eps32^-1/2) beside near-constant ones; channels six decades apart in one channel block; constant 2x2 windows (every maximum a tie,
    won by the window's first element)."""
    B, H, W, C = shape
    x = BB.value_input(kind, B, H, W, C, dt == BF16, 0)
    gamma, beta = BB.params(C, 0)
    st, idx = _chain(dt, x, gamma, beta, 0, kind)
    if kind == "constant":
        assert float(st[1][3]) == BB.f32(1.0 / math.sqrt(BB.EPS32)), float(st[1][3])
    if kind == "ties":
        assert bool((idx == 0).all())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", VSHAPES)
@pytest.mark.parametrize("kind", ["dA_const", "dP_xhat", "gelu_range"])
def test_bwd_value_cases(dt, shape, kind):
    """dA constant over all pixels (g - mean(g) cancels where gelu' is flat); dP proportional to xhat; GELU arguments from below -6 to
    above 6 (gamma scaled by 3)."""
    B, H, W, C = shape
    bf = dt == BF16
    x = BB.value_input("plain", B, H, W, C, bf, 4)
    gamma, beta = BB.params(C, 4, gscale=3.0 if kind == "gelu_range" else 1.0)
    dA = (lambda st: torch.full((B, H, W, C), 0.75, dtype=torch.float64)) if kind == "dA_const" else None
    dP = None
    if kind == "dP_xhat":
        dP = lambda st: BB.stored(0.5 * ((x - st[0].double()) * st[1].double())[:, 0:2 * (H // 2):2, 0:2 * (W // 2):2], bf)
    st, _ = _chain(dt, x, gamma, beta, 4, kind, dA, dP)
    if kind == "gelu_range":
        z = x * st[2].double() + st[3].double()
        assert float(z.min()) < -6 and float(z.max()) > 6


@pytest.mark.parametrize("dt", DTS)
def test_act_nan_and_inf_in_pool_windows(dt):
    """bf_bn_act alone with given sc / sh, so that no statistic is poisoned: a NaN at each of the four window positions, two NaNs in one
    window (the later one wins), a +inf.  `a` is NaN / inf exactly where the fp64 GELU of the same affine is; p and idx follow
    F.max_pool2d on the stored a."""
    B, H, W, C = 2, 6, 9, 20
    x = BB.stored(BB.randn(B, H, W, C, seed=5), dt == BF16)
    sc, sh = BB.randn(C, scale=0.3, shift=1.0, seed=6).abs().float() + 0.1, BB.randn(C, scale=0.5, seed=7).float()
    for k, (y, xx) in enumerate(((0, 0), (0, 3), (3, 0), (3, 3))):            # window positions 0, 1, 2, 3
        x[0, y, xx, k] = NAN
    x[1, 2, 4, 5], x[1, 3, 5, 5] = NAN, NAN                                    # positions 0 and 3 of one window
    x[1, 2, 4, 6], x[1, 3, 4, 6] = NAN, NAN                                    # positions 0 and 2
    x[1, 0, 1, 7] = float("inf")
    x[0, 5, 8, 8] = NAN                                                        # in the partial column: activated, not pooled
    a, p, idx = run_act(dt, x, sc, sh, True, "NaN / inf", finite=False)
    assert [int(idx[0, 0, 0, 0]), int(idx[0, 0, 1, 1]), int(idx[0, 1, 0, 2]), int(idx[0, 1, 1, 3])] == [0, 1, 2, 3]
    assert int(idx[1, 1, 2, 5]) == 3 and int(idx[1, 1, 2, 6]) == 2 and int(idx[1, 0, 0, 7]) == 1
    assert bool(torch.isnan(p[1, 1, 2, 5])) and float(p[1, 0, 0, 7]) == float("inf") and bool(torch.isnan(a[0, 5, 8, 8]))
    run_act(dt, x, sc, sh, False, "NaN / inf", finite=False)


# ---------------------------------------------------------------------------------------------------- eval
@pytest.mark.parametrize("B,C", [(1, 1), (3, 37), (2, 128), (3, 200)])
def test_eval_affine(B, C):
    """B * C below, at and above one 256-thread block; a channel with running_var = 0."""
    h = L.lib()
    gamma, beta = BB.params(C, C)
    rm, rv = BB.randn(C, scale=0.5, seed=1).float(), (BB.randn(C, seed=2).abs() + 0.5).float()
    rv[C // 2] = 0.0
    sc, sh = _buf(B * C), _buf(B * C)
    gd, bd, rmd, rvd = (_dev(t) for t in (gamma, beta, rm, rv))
    L.check(h.bf_bn_eval(B, C, _p(gd), _p(bd), BB.EPS32, _p(rmd), _p(rvd), _p(sc), _p(sh), _stream()), "bf_bn_eval")
    torch.cuda.synchronize()
    ref = BB.eval_affine(gamma, beta, rm, rv)
    for k, o in (("sc", sc), ("sh", sh)):
        fr = o[:B * C].view(B, C)
        assert bool((fr == fr[0]).all())
        _note("eval " + k, F32, BB.check(fr[0], *ref[k], f"eval B{B} C{C} {k}", ("channel",)), f"B{B} C{C}")
        _tail(o, B * C, "eval " + k)


# ---------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("dt", DTS)
def test_refusals_write_nothing(dt):
    h = L.lib()
    B, H, W, C = 2, 4, 6, 8
    M = B * H * W
    d = _dti(dt)
    x = torch.ones(M * C + TAIL, dtype=dt, device=DEV)
    v = torch.ones(B * C + TAIL, device=DEV)
    wideA = torch.ones(M * (C + BB.PADA) + TAIL, device=DEV)
    nbt = torch.zeros(2, dtype=torch.int64, device=DEV)
    o = [_buf(B * C) for _ in range(8)]                      # mean, rstd, sc, sh, rm, rv, dgamma, dbeta
    ws = _buf(h.bf_bn_ws_floats(M, C))
    big, pool, idx = _buf(M * C, dt), _buf(M * C // 4, dt), _ibuf(M * C // 4)
    idx_in = torch.zeros(M * C // 4 + TAIL, dtype=torch.uint8, device=DEV)

    def fwd(dtype=d, B_=B, HW=H * W, rm=o[4], rv=o[5]):
        return h.bf_bn_fwd(dtype, _p(x), B_, HW, C, _p(v), _p(v), BB.EPS32, MOM, _p(rm), _p(rv), _p(nbt), *[_p(t) for t in o[:4]], _p(ws), _stream())

    def act(dtype=d, H_=H, W_=W, p=pool, i=idx):
        return h.bf_bn_act(dtype, _p(x), B, H_, W_, C, _p(v), _p(v), _p(big), _p(p), _p(i), _stream())

    def bwd(dtype=d, dA=wideA, ldA=C, offA=0, dP=x, i=idx_in):
        return h.bf_bn_bwd(dtype, _p(dA), ldA, offA, _p(dP), _p(i), _p(x), B, H, W, C, _p(v), _p(v), _p(v), _p(v), _p(v), _p(big), _p(o[6]), _p(o[7]), 0,
                           _p(ws), _stream())

    assert fwd(B_=1, HW=1) != 0, "M = 1"
    assert fwd(rv=None) != 0 and fwd(rm=None) != 0, "one of the running pair"
    assert fwd(dtype=7) != 0 and act(dtype=7) != 0 and bwd(dtype=7) != 0, "dtype"
    assert act(H_=1, W_=M // B) != 0 and act(H_=M // B, W_=1) != 0, "a pool with H = 1 or W = 1"
    assert act(i=None) != 0 and act(p=None) != 0, "p and idx go together"
    assert bwd(dA=None, dP=None) != 0, "no incoming gradient"
    assert bwd(ldA=C + BB.PADA, offA=BB.PADA + 1) != 0 and bwd(ldA=C - 1) != 0, "ldA < offA + C"
    assert bwd(ldA=C + BB.PADA, offA=-1) != 0, "offA < 0"
    assert bwd(i=None) != 0, "dP without idx"
    _untouched(o + [ws, big, pool, idx], f"{dt}")
    assert nbt.tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------------- reruns
@pytest.mark.parametrize("dt", DTS)
def test_reruns_agree_bit_for_bit(dt):
    """No float atomics anywhere: the (1, 65, 67, 65) forward and backward (272 slabs, two channel blocks) run twice give the same bits."""
    B, H, W, C = shape = (1, 65, 67, 65)
    assert _expect(shape)["gx"] == 2
    x = BB.stored(BB.randn(B, H, W, C, scale=1.5, shift=0.3, seed=11), dt == BF16)
    gamma, beta = BB.params(C, 11)
    st1, _ = run_fwd(dt, x, gamma, beta, True, 11)
    st2, _ = run_fwd(dt, x, gamma, beta, True, 11)
    assert all(torch.equal(u, v) for u, v in zip(st1, st2))
    a, p, idx = run_act(dt, x, st1[2], st1[3], True)
    dA, dP = BB.grads(B, H, W, C, dt == BF16, 11)
    r1 = run_bwd(dt, x, gamma, st1, dA, dP, idx)
    r2 = run_bwd(dt, x, gamma, st1, dA, dP, idx)
    assert all(torch.equal(u, v) for u, v in zip(r1, r2)), "the backward differs from run to run"


# ---------------------------------------------------------------------------------------------------- report
def test_report_worst_ratios(capsys):
    """Last in the module: prints the worst |got - ref| / bound of each area the tests above reached (all are <= 1, or they failed)."""
    assert all(r <= 1.0 for r, _ in WORST.values())
    with capsys.disabled():
        print("\nworst |got - ref| / bound per area:")
        for area, (r, case) in sorted(WORST.items()):
            print(f"  {area:28s} {r:.3e}  ({case})")
