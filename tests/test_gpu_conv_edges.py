"""GPU: the raw conv.hip bindings at their edge shapes, every output held to the per-element bound of tests/conv_bounds.py.

Forward and transposed gathers at 1x1 / tiny / odd frames and empty parity phases, ragged row and column tiles, two channel-concatenated
sources split across k-runs and taps, the GroupNorm + GELU prologue with per-frame scale / shift, bias + residual epilogues, the nchw
fp32 first / last-layer paths, weight gradients down to many slabs with a partial last one, column sums, the accumulate = 1 flags of the
C ABI, and GroupNorm statistics / backward at fewer pixels than slices and across the source boundary.  fp32 and bf16 throughout."""
import ctypes as ct

import pytest
import torch
import torch.nn.functional as F

from bubbleformer_amd import _lib as L
from tests import conv_bounds as CB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTS = [torch.float32, torch.bfloat16]
WORST = {}                                              # area -> (worst ratio, case)


@pytest.fixture(scope="module", autouse=True)
def _report(request):
    yield
    cap = request.config.pluginmanager.get_plugin("capturemanager")
    if WORST and cap is not None:
        with cap.global_and_fixture_disabled():
            print("\nworst |got - ref| / bound per area:")
            for area, (r, case) in sorted(WORST.items()):
                print(f"  {area:28s} {r:.3e}  ({case})")


def _note(area, ratio, case):
    if ratio >= WORST.get(area, (-1.0, ""))[0]:
        WORST[area] = (ratio, case)


def _randn(*shape, scale=1.0, shift=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift


def _st(t, dt):
    """Exact stored values of t in dtype dt (fp64)."""
    return t.to(dt).double()


def _dev(t, dt, nchw=False):
    """fp64 NCHW -> device tensor in dt, channels-last unless nchw."""
    return (t if nchw else t.permute(0, 2, 3, 1)).to(dt).contiguous().to(DEV)


def _back(t, nchw=False):
    torch.cuda.synchronize()
    return (t if nchw else t.permute(0, 3, 1, 2)).double().cpu()


def _nan(shape, dt):
    return torch.full(shape, float("nan"), dtype=dt, device=DEV)


def _ops():
    from bubbleformer_amd import ops
    return ops


def _sc_sh(Fr, Cin, seed):
    """fp32 GroupNorm-prologue scale / shift that differ per frame (a frame mix-up inside a row tile changes the result)."""
    sc = _randn(Fr, Cin, scale=0.3, shift=1.0, seed=seed).float()
    sh = _randn(Fr, Cin, scale=0.5, seed=seed + 1).float()
    return sc, sh


def run_conv(dt, Fr, Hi, Wi, Ho, Wo, k, s, p, C0, C1, N, pro=CB.PRO_NONE, transposed=False, bias=False, resid=False, src_nchw=False,
             out="dt", seed=0):
    """One bf_conv_fwd call against the bound.  out: "dt" (channels-last in the compute dtype), "f32" (channels-last fp32, the dA
    path) or "nchw" (fp32 (F, N, H, W), the last layer).  -> worst ratio."""
    ops = _ops()
    bf = dt == torch.bfloat16
    Cin = C0 + C1
    sdt = torch.float32 if src_nchw else dt
    x0 = _st(_randn(Fr, C0, Hi, Wi, scale=1.5, shift=0.3, seed=seed), sdt)
    x1 = _st(_randn(Fr, C1, Hi, Wi, seed=seed + 1), dt) if C1 else None
    sc, sh = _sc_sh(Fr, Cin, seed + 2) if pro == CB.PRO_AFFINE_GELU else (None, None)
    wshape = (Cin, N, k, k) if transposed else (N, Cin, k, k)
    w = _st(_randn(*wshape, scale=(k * k * Cin) ** -0.5, seed=seed + 3), dt)
    wg = w.permute(2, 3, 0, 1) if transposed else w.permute(2, 3, 1, 0)
    b = _randn(N, scale=0.5, seed=seed + 4).float() if bias else None
    r = _st(_randn(Fr, N, Ho, Wo, seed=seed + 5), dt) if resid else None
    odt = dt if out == "dt" else torch.float32
    o = _nan((Fr, N, Ho, Wo) if out == "nchw" else (Fr, Ho, Wo, N), odt)
    x0g = _dev(x0, sdt, src_nchw)
    x1g = _dev(x1, dt) if C1 else None
    rg = _dev(r, dt) if resid else None
    ops._conv(dt, ops._geo(Fr, Hi, Wi, Ho, Wo, k, s, p), ops._csrc(x0g, C0, src_nchw), ops._csrc(x1g, C1), wg.to(dt).contiguous().to(DEV), N,
              ops._csrc(o, N, out == "nchw"), pro, sc.to(DEV) if sc is not None else None, sh.to(DEV) if sh is not None else None,
              b.to(DEV) if bias else None, ops._csrc(rg, N), transposed)
    got = _back(o, out == "nchw")
    a, ea = CB.operand(torch.cat([x0] + ([x1] if C1 else []), 1), pro, sc, sh, bf)
    fn = CB.conv_transposed if transposed else CB.conv_fwd
    ref, bnd = fn(a, ea, w, s, p, Ho, Wo, bias=b, resid=r, out_bf16=bf and out == "dt")
    return CB.check(got, ref, bnd, f"conv {'T' if transposed else 'F'} {dt} F{Fr} {Hi}x{Wi}->{Ho}x{Wo} k{k}s{s}p{p} C{C0}+{C1} N{N}")


def _ho(H, k, s, p):
    return (H + 2 * p - k) // s + 1


FWD_GEOS = [(k, s, p, H, W) for (k, s, p) in [(1, 1, 0), (3, 1, 1)] for (H, W) in [(1, 1), (2, 2), (3, 5)]] + \
           [(3, 2, 1, H, W) for (H, W) in [(1, 1), (2, 2), (1, 7), (3, 5), (7, 6)]]


# ---------------------------------------------------------------------------------------------------- forward gather
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("k,s,p,H,W", FWD_GEOS)
def test_forward_geometry(dt, k, s, p, H, W):
    """GN + GELU prologue, bias and residual at every forward geometry; 33 input channels, a ragged 65-column output."""
    r = run_conv(dt, 2, H, W, _ho(H, k, s, p), _ho(W, k, s, p), k, s, p, 33, 0, 65, CB.PRO_AFFINE_GELU, bias=True, resid=True, seed=H * 7 + W)
    _note("forward geometry", r, f"{dt} k{k}s{s} {H}x{W}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Cin", [1, 3, 33])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
def test_forward_channels(dt, Cin, N):
    r = run_conv(dt, 2, 3, 5, 3, 5, 3, 1, 1, Cin, 0, N, CB.PRO_GELU, bias=True, seed=Cin * 131 + N)
    _note("channels", r, f"{dt} Cin{Cin} N{N}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C0,C1", [(1, 7), (5, 12), (12, 20)])
@pytest.mark.parametrize("pro", [CB.PRO_NONE, CB.PRO_GELU, CB.PRO_AFFINE_GELU])
def test_two_sources(dt, C0, C1, pro):
    """(5, 12): a k-run of 8 crosses the tap boundary at 17 and the source boundary at 5 of the next tap."""
    r = run_conv(dt, 3, 4, 5, 4, 5, 3, 1, 1, C0, C1, 24, pro, bias=True, seed=C0 * 17 + pro)
    _note("two sources", r, f"{dt} {C0}+{C1} pro{pro}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Fr,H,W", [(7, 3, 3), (4, 4, 4), (5, 13, 1)])
def test_rows_and_frames(dt, Fr, H, W):
    """M = 63 / 64 / 65 output rows; at 7 frames of 3x3 one 64-row tile spans all 7 frames, each with its own sc / sh."""
    r = run_conv(dt, Fr, H, W, H, W, 3, 1, 1, 8, 0, 16, CB.PRO_AFFINE_GELU, resid=True, seed=Fr * 100 + H)
    _note("rows", r, f"{dt} M{Fr * H * W}")


@pytest.mark.parametrize("dt", DTS)
def test_nchw_paths(dt):
    """The first layer reads the (B, T*C, H, W) fp32 clip in place (rounded to bf16 in bf16 mode); the last writes fp32 (B, N, H, W)
    behind its prologue; the data gradients write fp32 channels-last (dA) and read / write the nchw fp32 tensors."""
    cases = [
        dict(Fr=2, Hi=5, Wi=7, Ho=5, Wo=7, k=1, s=1, p=0, C0=64, C1=0, N=65, src_nchw=True, bias=True),               # image_proj
        dict(Fr=2, Hi=5, Wi=7, Ho=5, Wo=7, k=3, s=1, p=1, C0=4, C1=0, N=16, src_nchw=True),                          # classic conv1
        dict(Fr=2, Hi=5, Wi=7, Ho=5, Wo=7, k=1, s=1, p=0, C0=16, C1=0, N=64, pro=CB.PRO_AFFINE_GELU, out="nchw", bias=True),   # final
        dict(Fr=2, Hi=5, Wi=7, Ho=5, Wo=7, k=3, s=1, p=1, C0=24, C1=0, N=40, transposed=True, out="f32"),             # dA
        dict(Fr=2, Hi=5, Wi=7, Ho=5, Wo=7, k=1, s=1, p=0, C0=64, C1=0, N=16, transposed=True, src_nchw=True, out="f32"),  # final dA
        dict(Fr=2, Hi=5, Wi=7, Ho=5, Wo=7, k=1, s=1, p=0, C0=65, C1=0, N=64, transposed=True, out="nchw"),            # d clip
    ]
    for i, c in enumerate(cases):
        r = run_conv(dt, seed=300 + i, **c)
        _note("nchw paths", r, f"{dt} case {i}")


# ---------------------------------------------------------------------------------------------------- transposed gather
TR_GEOS = [
    # (Hi, Wi, Ho, Wo, k, s, p, what)
    (1, 1, 2, 2, 4, 2, 1, "upsample 1x1"), (1, 3, 2, 6, 4, 2, 1, "upsample 1x3"), (3, 5, 6, 10, 4, 2, 1, "upsample 3x5"),
    (1, 1, 2, 2, 2, 2, 0, "upconv2 1x1"), (3, 5, 6, 10, 2, 2, 0, "upconv2 3x5"),
    (3, 5, 3, 5, 3, 1, 1, "dgrad 3x3 s1"), (1, 1, 1, 1, 3, 1, 1, "dgrad 3x3 s1 1x1"),
    (4, 3, 7, 6, 3, 2, 1, "dgrad 3x3 s2 odd"), (1, 4, 1, 7, 3, 2, 1, "dgrad 3x3 s2 Ho=1"), (1, 1, 2, 2, 3, 2, 1, "dgrad 3x3 s2 2x2"),
    (1, 1, 1, 1, 3, 2, 1, "dgrad 3x3 s2 1x1"), (3, 5, 3, 5, 1, 1, 0, "dgrad 1x1"),
]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Hi,Wi,Ho,Wo,k,s,p,what", TR_GEOS)
def test_transposed(dt, Hi, Wi, Ho, Wo, k, s, p, what):
    """ConvTranspose2d k4 s2 p1 / k2 s2 p0 with bias, and data gradients (odd Ho; Ho = 1 leaves a parity phase empty) into fp32 dA."""
    up = what.startswith("up")
    r = run_conv(dt, 2, Hi, Wi, Ho, Wo, k, s, p, 33, 0, 65 if up else 40, transposed=True, bias=up, resid=up, out="dt" if up else "f32",
                 seed=Hi * 11 + Ho + k)
    _note("transposed", r, f"{dt} {what}")


# ---------------------------------------------------------------------------------------------------- weight gradient
def run_wgrad(dt, Fr, Hi, Wi, Ho, Wo, k, s, p, C0, C1, R, pro=CB.PRO_NONE, rows_nchw=False, accumulate=False, seed=0):
    ops = _ops()
    bf = dt == torch.bfloat16
    Cin, K = C0 + C1, k * k * (C0 + C1)
    x0 = _st(_randn(Fr, C0, Hi, Wi, scale=1.5, shift=0.3, seed=seed), dt)
    x1 = _st(_randn(Fr, C1, Hi, Wi, seed=seed + 1), dt) if C1 else None
    sc, sh = _sc_sh(Fr, Cin, seed + 2) if pro == CB.PRO_AFFINE_GELU else (None, None)
    rdt = torch.float32 if rows_nchw else dt
    rows = _st(_randn(Fr, R, Ho, Wo, seed=seed + 3), rdt)
    prior = _randn(R, K, seed=seed + 4).float() if accumulate else None
    dw = prior.clone().to(DEV) if accumulate else _nan((R, K), torch.float32)
    geo = ops._geo(Fr, Hi, Wi, Ho, Wo, k, s, p)
    keep = [_dev(rows, rdt, rows_nchw), _dev(x0, dt), _dev(x1, dt) if C1 else None]   # _csrc holds raw pointers only
    rs, s0, s1 = ops._csrc(keep[0], R, rows_nchw), ops._csrc(keep[1], C0), ops._csrc(keep[2], C1)
    scd, shd = (sc.to(DEV), sh.to(DEV)) if sc is not None else (None, None)
    if accumulate:
        lib = L.lib()
        n = lib.bf_conv_wgrad_ws_floats(R, K, Fr * Ho * Wo)
        ws = torch.empty(n, dtype=torch.float32, device=DEV)
        L.check(lib.bf_conv_wgrad(ops._dt(dt), ct.byref(geo), ct.byref(rs), ct.byref(s0), ops._ref(s1), pro, ops._p(scd), ops._p(shd),
                                  ops._p(dw), 1, ops._p(ws), ws.numel(), ops._stream()), "bf_conv_wgrad")
    else:
        ops._wgrad(dt, geo, rs, s0, s1, K, dw, pro, scd, shd)
    torch.cuda.synchronize()
    a, ea = CB.operand(torch.cat([x0] + ([x1] if C1 else []), 1), pro, sc, sh, bf)
    ref, bnd = CB.conv_wgrad(CB.rnd16(rows) if bf else rows, a, ea, k, s, p, prior=prior.double() if accumulate else None)
    return CB.check(dw.cpu(), ref, bnd, f"wgrad {dt} F{Fr} {Hi}x{Wi}->{Ho}x{Wo} k{k}s{s}p{p} C{C0}+{C1} R{R} acc{int(accumulate)}",
                    ("r", "k"))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("k,s,p,H,W", FWD_GEOS)
def test_wgrad_geometry(dt, k, s, p, H, W):
    """Every forward geometry, plain (one source) and with the prologue on two sources; R = 65 (ragged row tile)."""
    Ho, Wo = _ho(H, k, s, p), _ho(W, k, s, p)
    r1 = run_wgrad(dt, 2, H, W, Ho, Wo, k, s, p, 33, 0, 65, seed=H * 5 + W)
    r2 = run_wgrad(dt, 3, H, W, Ho, Wo, k, s, p, 5, 12, 65, CB.PRO_AFFINE_GELU, seed=H * 5 + W + 50)
    _note("wgrad geometry", max(r1, r2), f"{dt} k{k}s{s} {H}x{W}")


@pytest.mark.parametrize("dt", DTS)
def test_wgrad_special(dt):
    cases = [
        dict(Fr=2, Hi=6, Wi=10, Ho=3, Wo=5, k=4, s=2, p=1, C0=24, C1=0, R=33),                       # Upsample's weight gradient
        dict(Fr=2, Hi=6, Wi=10, Ho=3, Wo=5, k=2, s=2, p=0, C0=24, C1=0, R=33),                       # classic upconv's
        dict(Fr=4, Hi=61, Wi=67, Ho=61, Wo=67, k=3, s=1, p=1, C0=8, C1=0, R=8),                      # 64 slabs, the last 220 of 256 pixels
        dict(Fr=2, Hi=5, Wi=7, Ho=5, Wo=7, k=1, s=1, p=0, C0=16, C1=0, R=64, pro=CB.PRO_AFFINE_GELU, rows_nchw=True),   # final layer
        dict(Fr=3, Hi=4, Wi=5, Ho=4, Wo=5, k=3, s=1, p=1, C0=12, C1=20, R=16, pro=CB.PRO_GELU, accumulate=True),
        dict(Fr=4, Hi=61, Wi=67, Ho=61, Wo=67, k=3, s=1, p=1, C0=8, C1=0, R=8, accumulate=True),
    ]
    M, K = 4 * 61 * 67, 72
    chunk, slabs = CB.wgrad_split(8, K, M)
    assert slabs > 1 and M % chunk != 0
    for i, c in enumerate(cases):
        r = run_wgrad(dt, seed=400 + i, **c)
        _note("wgrad special", r, f"{dt} case {i}")


# ---------------------------------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Fr,H,W,C,nchw,acc", [
    (1, 3, 5, 65, False, False),      # M = 15 < 64: one-row chunks
    (1, 1, 1, 3, False, False),
    (3, 17, 19, 130, False, False),
    (2, 5, 7, 64, True, False),       # fp32 nchw dpred
    (2, 3, 5, 65, False, True),
    (3, 17, 19, 8, True, True),
])
def test_colsum(dt, Fr, H, W, C, nchw, acc):
    ops = _ops()
    sdt = torch.float32 if nchw else dt
    x = _st(_randn(Fr, C, H, W, shift=0.2, seed=Fr * 7 + C), sdt)
    prior = _randn(C, seed=5).float() if acc else None
    out = prior.clone().to(DEV) if acc else _nan((C,), torch.float32)
    xg = _dev(x, sdt, nchw)                          # _csrc holds a raw pointer only
    src = ops._csrc(xg, C, nchw)
    if acc:
        ws = torch.empty(64 * C, dtype=torch.float32, device=DEV)
        L.check(L.lib().bf_conv_colsum(ops._dt(dt), ct.byref(src), Fr, H, W, ops._p(out), 1, ops._p(ws), ws.numel(), ops._stream()),
                "bf_conv_colsum")
    else:
        ops._colsum(dt, src, Fr, H, W, out)
    torch.cuda.synchronize()
    ref, bnd = CB.colsum(x, prior.double() if acc else None)
    r = CB.check(out.cpu(), ref, bnd, f"colsum {dt} F{Fr} {H}x{W} C{C} acc{int(acc)}", ("channel",))
    _note("column sums", r, f"{dt} M{Fr * H * W} C{C} acc{int(acc)}")


# ---------------------------------------------------------------------------------------------------- GroupNorm
GN_CASES = [(1, 1, 1, 40, 0), (3, 2, 3, 40, 0), (2, 1, 1, 12, 28), (3, 2, 3, 12, 28), (2, 5, 7, 8, 0), (1, 1, 1, 8, 0), (3, 3, 4, 16, 0)]
E53 = 2.0 ** -53


def _gn_case(dt, Fr, H, W, C0, C1, seed):
    x0 = _st(_randn(Fr, C0, H, W, scale=2.0, shift=1.0, seed=seed), dt)
    x1 = _st(_randn(Fr, C1, H, W, scale=0.5, shift=-0.5, seed=seed + 1), dt) if C1 else None
    gamma = _randn(C0 + C1, scale=0.2, shift=1.0, seed=seed + 2).float()
    beta = _randn(C0 + C1, scale=0.2, seed=seed + 3).float()
    return x0, x1, gamma, beta


def gn_stats_bounds(x, gamma, beta, G=8, eps=float(torch.tensor(1e-5, dtype=torch.float32))):
    """fp64 GroupNorm statistics of the stored x (F, C, H, W) and the bounds of bf_gn_fwd's fp32 results: fp64 sums of n terms (tree
    order; gamma_n in fp64), mean / rstd rounded once to fp32, sc = fl(gamma*rstd), sh = fl(beta - fl(mean*sc)) (contracted or not).
    eps is the fp32 value the C ABI receives."""
    Fr, Cn = x.shape[:2]
    xg = x.reshape(Fr, G, -1)
    n = xg.shape[2]
    g64 = (n + 4) * E53
    mu = xg.mean(2)
    var = (xg * xg).mean(2) - mu * mu
    e_mu = g64 * xg.abs().mean(2)
    e_var = 2 * g64 * (xg * xg).mean(2) + 2 * mu.abs() * e_mu
    rstd = 1 / torch.sqrt(var.clamp_min(0) + eps)
    e_r = rstd * (0.5 * e_var / (var.clamp_min(0) + eps) + 4 * E53) * 1.01
    b_mean = e_mu + CB.U32 * mu.abs()
    b_rstd = e_r + CB.U32 * rstd
    rep = lambda t: t.repeat_interleave(Cn // G, 1)
    ga, be = gamma.double()[None], beta.double()[None]
    sc = ga * rep(rstd)
    b_sc = ga.abs() * rep(b_rstd) + CB.U32 * sc.abs()
    sh = be - rep(mu) * sc
    b_sh = rep(b_mean) * sc.abs() + rep(mu.abs()) * b_sc + CB.U32 * (rep(mu).abs() * sc.abs() + sh.abs())
    return (mu, rstd, sc, sh), (b_mean, b_rstd, b_sc, b_sh)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Fr,H,W,C0,C1", GN_CASES)
def test_group_norm_stats(dt, Fr, H, W, C0, C1):
    """HW = 1 and 6 (fewer pixels than the 32 slices), 8 channels (one per group), groups straddling C0 = 12 of 40, 3 frames."""
    ops = _ops()
    x0, x1, gamma, beta = _gn_case(dt, Fr, H, W, C0, C1, seed=Fr * 31 + H * W + C0)
    got = ops._gn_fwd(dt, _dev(x0, dt), C0, _dev(x1, dt) if C1 else None, C1, Fr, H, W, gamma.to(DEV), beta.to(DEV))
    torch.cuda.synchronize()
    x = torch.cat([x0] + ([x1] if C1 else []), 1)
    refs, bnds = gn_stats_bounds(x, gamma, beta)
    worst = 0.0
    for name, g, rf, bd in zip(("mean", "rstd", "sc", "sh"), got, refs, bnds):
        worst = max(worst, CB.check(g.cpu(), rf, bd, f"gn {name} {dt} F{Fr} {H}x{W} C{C0}+{C1}", ("frame", "group/channel")))
    _note("groupnorm stats", worst, f"{dt} F{Fr} {H}x{W} C{C0}+{C1}")


def _rel16(got, want, tol, what):
    """rel-L2 over the whole tensor and every block of 16 channels (dim 1); an exactly-zero reference block is held to tol absolute."""
    got, want = got.double().cpu(), want.double().cpu()
    assert torch.isfinite(got).all(), what
    worst = 0.0
    for c0 in range(0, want.shape[1], 16):
        g, w = got[:, c0:c0 + 16], want[:, c0:c0 + 16]
        e = float((g - w).norm() / w.norm()) if w.abs().max() > 1e-9 else float(g.abs().max())
        assert e <= tol, (what, "channels %d.." % c0, e)
        worst = max(worst, e)
    return worst


def _group_norm(x, gamma, beta, G=8, eps=1e-5):
    """GroupNorm written out (F.group_norm refuses groups of one value, the 8-channel 1x1 case)."""
    xg = x.reshape(x.shape[0], G, -1)
    mu = xg.mean(2, keepdim=True)
    xh = ((xg - mu) / torch.sqrt(((xg - mu) ** 2).mean(2, keepdim=True) + eps)).view_as(x)
    return xh * gamma[None, :, None, None] + beta[None, :, None, None]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Fr,H,W,C0,C1", [c for c in GN_CASES if c[1] * c[2] * c[3] > 8])
@pytest.mark.parametrize("norm", [True, False])
def test_group_norm_backward(dt, Fr, H, W, C0, C1, norm):
    """GELU' folded in, dx split into both sources plus an fp32 `add` (the shortcut's data gradient); without a norm, GELU alone.
    Not at one value per group (8 channels, 1x1): there x*sc and sh cancel to beta with rstd = eps^-1/2, so the fp32 prologue input
    carries ~|x sc| / |beta| ~ 1e3 ulps -- a property of the sc / sh form that the conv bound's |v sc| + |sh| term covers and a fixed
    rel-L2 does not.  Its statistics are checked above."""
    ops = _ops()
    Cn = C0 + C1
    x0, x1, gamma, beta = _gn_case(dt, Fr, H, W, C0, C1, seed=Fr * 37 + H * W + C0)
    dA = _randn(Fr, Cn, H, W, seed=7).float().double()
    add = _randn(Fr, Cn, H, W, scale=0.3, seed=8).float().double()
    x0g, x1g = _dev(x0, dt), (_dev(x1, dt) if C1 else None)
    stats = ops._gn_fwd(dt, x0g, C0, x1g, C1, Fr, H, W, gamma.to(DEV), beta.to(DEV)) if norm else None
    dg = _nan((Cn,), torch.float32) if norm else None
    db = _nan((Cn,), torch.float32) if norm else None
    dx0, dx1 = ops._gn_bwd(dt, _dev(dA, torch.float32).reshape(-1, Cn), x0g, C0, x1g, C1, Fr, H, W, gamma.to(DEV) if norm else None, stats,
                           _dev(add, torch.float32), Cn, dg, db)
    torch.cuda.synchronize()
    xr = torch.cat([x0] + ([x1] if C1 else []), 1).requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.gelu(_group_norm(xr, gr, br) if norm else xr)
    y.backward(dA)
    tol = 1e-5 if dt == torch.float32 else 1e-2
    dx = torch.cat([_back(dx0)] + ([_back(dx1)] if C1 else []), 1)
    what = f"gn bwd {dt} F{Fr} {H}x{W} C{C0}+{C1} norm{int(norm)}"
    worst = _rel16(dx, xr.grad + add, tol, what + " dx")
    if norm:
        worst = max(worst, _rel16(dg.cpu()[None], gr.grad[None], tol, what + " dgamma"), _rel16(db.cpu()[None], br.grad[None], tol, what + " dbeta"))
    _note("groupnorm backward (rel-L2)", worst, f"{dt} F{Fr} {H}x{W} C{C0}+{C1} norm{int(norm)}")
