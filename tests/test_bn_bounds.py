"""CPU: pins tests/bn_bounds.py.  An fp32 / fp64 emulation of the arithmetic of bn.hip's kernels (slab statistics and finalize, the eval
affine, GELU with and without the pool, the backward's partial sums, parameter gradients and apply) in two slab orders -- the slabs as
bn_slabs cuts them, row threads then an LDS halving tree, then slab_sums' strided trips and its tree; and one plain sequential sum -- must
fall inside the bound in both dtypes; the closed-form backward must equal fp64 autograd through F.batch_norm(training) -> F.gelu ->
F.max_pool2d at exact statistics; the emulation with one defect each must be rejected on the inputs tests/test_gpu_bn_edges.py uses; and
the restated host code is pinned to the plan table of the edge shapes."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import bn_bounds as BB
from tests.test_gemm_bounds import fma32

F32, BF16 = torch.float32, torch.bfloat16
DTS = [F32, BF16]
ORDERS = ["slabs", "seq"]
CS32, C032 = BB.f32(0.70710678118654752440), BB.f32(0.39894228040143267794)

# (B, H, W, C): (slabs, used, pixels in the last slab) -- computed from the formulas of bn.hip
PLAN = {(1, 1, 2, 1): (1, 1, 2), (1, 2, 2, 33): (1, 1, 4), (2, 5, 7, 3): (1, 1, 70), (3, 5, 7, 20): (3, 3, 35), (1, 3, 107, 64): (20, 19, 15),
        (1, 65, 67, 64): (272, 257, 3), (1, 65, 67, 65): (272, 257, 3), (1, 65, 67, 512): (256, 242, 17), (1, 513, 513, 1): (257, 257, 769)}


# ---------------------------------------------------------------------------------------------------- emulation
def gelu_erff32(t):
    return 0.5 * t * (1.0 + torch.erf(t * CS32))


def dgelu_erff32(t):
    return 0.5 * (1.0 + torch.erf(t * CS32)) + t * C032 * torch.exp(-0.5 * t * t)


def _halve(acc, dim_len):
    o = dim_len // 2
    while o >= 1:
        acc = acc[..., :o, :] + acc[..., o:2 * o, :]
        o //= 2
    return acc[..., 0, :]


def slab_reduce(t, order, mutant=None):
    """Sum t (M, C) fp64 over M.  "seq": row after row.  "slabs": bn_stats_kernel / bn_bwd_partial_kernel (row thread rl takes pixels
    rl, rl + rows, ... of its slab, then tree_rows), then slab_sums (thread z takes slabs z, z + 256, ..., then the tree over 256)."""
    M, C = t.shape
    if order == "seq":
        acc = torch.zeros(C, dtype=torch.float64)
        for i in range(M):
            acc = acc + t[i]
        return acc
    p = BB.plan(M, C)
    chunk, used, rows = p["chunk"], p["used"], p["rows"]
    t = torch.cat([t, torch.zeros(used * chunk - M, C, dtype=torch.float64)]).reshape(used, chunk, C)
    q = -(-chunk // rows)
    t = torch.cat([t, torch.zeros(used, q * rows - chunk, C, dtype=torch.float64)], 1).reshape(used, q, rows, C)
    acc = torch.zeros(used, rows, C, dtype=torch.float64)
    for i in range(q):
        acc = acc + t[:, i]
    part = _halve(acc, rows)                               # (used, C): the workspace
    if mutant == "drop_last_slab":
        part = part[:-1]
    if mutant == "first_trip_only":
        part = part[:BB.BN_THREADS]
    trips = -(-part.shape[0] // BB.BN_THREADS)
    part = torch.cat([part, torch.zeros(trips * BB.BN_THREADS - part.shape[0], C, dtype=torch.float64)]).reshape(trips, BB.BN_THREADS, C)
    acc = torch.zeros(BB.BN_THREADS, C, dtype=torch.float64)
    for i in range(trips):
        acc = acc + part[i]
    return _halve(acc, BB.BN_THREADS)


def emu_fwd(x, gamma, beta, rm=None, rv=None, eps32=BB.EPS32, mom=0.1, order="slabs", mutant=None):
    C = x.shape[-1]
    xf = x.float().double().reshape(-1, C)
    n = float(xf.shape[0])
    s1, s2 = slab_reduce(xf, order, mutant), slab_reduce(xf * xf, order, mutant)
    mu = s1 / n
    var = (s2 / n - mu * mu).clamp_min(0.0)
    m = mu.float()
    eps = 1e-5 if mutant == "eps_literal" else eps32
    r = (1.0 / torch.sqrt((var * n / (n - 1.0) if mutant == "unbiased_rstd" else var) + eps)).float()
    a = gamma * r
    out = dict(mean=m, rstd=r, sc=a, sh=beta - m * a)
    if rm is not None:
        mom32 = torch.tensor(mom, dtype=F32)
        unb = (var if mutant == "biased_running" else var * n / (n - 1.0)).float()
        out["rm"] = mom32 * m + (1.0 - mom32) * rm
        out["rv"] = mom32 * unb + (1.0 - mom32) * rv
    return out


def emu_eval(gamma, beta, rm, rv, eps32=BB.EPS32):
    r = (1.0 / torch.sqrt(rv.double() + eps32)).float()
    a = gamma * r
    return dict(sc=a, sh=beta - rm * a)


def emu_act(x, sc, sh, dt, pool=False, mutant=None):
    """-> a, or (a, p, idx) with the kernel's rule: a later element wins only if strictly greater or NaN."""
    t = fma32(x.float(), sc, sh)
    if mutant == "double_round":
        t = t.to(dt).float()
    a = gelu_erff32(t).to(dt)
    if not pool:
        return a
    Hp, Wp = a.shape[1] // 2, a.shape[2] // 2
    af = a.float()
    best = af[:, 0:2 * Hp:2, 0:2 * Wp:2]
    bi = torch.zeros_like(best, dtype=torch.uint8)
    for j in range(1, 4):
        v = af[:, j >> 1:2 * Hp:2, j & 1:2 * Wp:2]
        take = ((v >= best) if mutant == "tie_last" else (v > best)) | torch.isnan(v)
        best = torch.where(take, v, best)
        bi = torch.where(take, torch.full_like(bi, j), bi)
    return a, best.to(dt), bi


def emu_route(dP, idx, B, H, W, mutant=None):
    """bn_grad_in's index arithmetic, pixel by pixel -> (M, C) fp32."""
    C = dP.shape[-1]
    Hp, Wp = H // 2, W // 2
    m = torch.arange(B * H * W)
    f, r = m // (H * W), m % (H * W)
    y, xx = r // W, r % W
    ok = ((y >> 1) < Hp) & ((xx >> 1) < Wp)
    o = (f * Hp + (y >> 1)) * Wp + (xx >> 1)
    if mutant == "partial_windows":                        # no guard: the partial windows read the neighbouring entries
        ok = torch.ones_like(ok)
        o = o % (B * Hp * Wp)
    o = torch.where(ok, o, torch.zeros_like(o))
    pos = ((y & 1) << 1) | (xx & 1)
    take = ok[:, None] & (idx.reshape(-1, C)[o].long() == pos[:, None])
    return torch.where(take, dP.float().reshape(-1, C)[o], torch.zeros(()))


def emu_bwd(dAw, offA, dP, idx, x, gamma, mean, rstd, sc, sh, dt, order="slabs", prior=None, mutant=None):
    """dAw: the wide fp32 buffer (B, H, W, ld) or None, read at channel offA; prior: (dgamma, dbeta) for accumulate = 1, None for 0."""
    B, H, W, C = x.shape
    M = B * H * W
    xf = x.float().reshape(M, C)
    g = torch.zeros(M, C)
    if dAw is not None:
        o = 0 if mutant == "offA_ignored" else offA
        g = dAw.reshape(M, -1)[:, o:o + C].float().clone()
    if dP is not None:
        g = g + emu_route(dP, idx, B, H, W, mutant)
    if mutant != "no_dgelu":
        g = g * dgelu_erff32(fma32(xf, sc, sh))
    xh = (xf - mean) * rstd
    s1, s2 = slab_reduce(g.double(), order), slab_reduce(g.double() * xh.double(), order)
    p = BB.plan(M, C)
    ws = torch.full((BB.ws_floats(M, C),), float("nan"))
    off = BB.coef_offset(M, C)
    ws[off:off + 2 * C] = torch.stack([(s1 / M).float(), (s2 / M).float()], -1).reshape(-1)
    roff = 2 * p["slabs"] * C * 2 if mutant == "coef_at_slabs" else off
    coef = ws[roff:roff + 2 * C].reshape(C, 2)
    db, dg = s1.float(), s2.float()
    if prior is not None and mutant != "acc_overwrite":
        dg, db = prior[0] + dg, prior[1] + db
    inner = g - coef[:, 0] if mutant == "no_s2" else g - coef[:, 0] - xh * coef[:, 1]
    if mutant == "double_round":
        inner = inner.to(dt).float()
    dx = ((gamma * rstd) * inner).to(dt)
    return dict(dx=dx.reshape(B, H, W, C), dgamma=dg, dbeta=db)


# ---------------------------------------------------------------------------------------------------- helpers
def _check_fwd(got, ref, what):
    return max(BB.check(got[k], *ref[k], f"{what} {k}", ("channel",)) for k in ref)


def _check_bwd(got, ref, what):
    w = BB.check(got["dx"], *ref["dx"], what + " dx", ("frame", "y", "x", "channel"))
    return max(w, BB.check(got["dgamma"], *ref["dgamma"], what + " dgamma", ("channel",)),
               BB.check(got["dbeta"], *ref["dbeta"], what + " dbeta", ("channel",)))


def _rejected(fn):
    with pytest.raises(AssertionError, match="exceeds the bound|non-finite output"):
        fn()


def _running(C, seed):
    return BB.randn(C, scale=0.5, seed=seed + 300).float(), (BB.randn(C, seed=seed + 301).abs() + 0.5).float()


def _bwd_case(shape, dt, kind="edge", seed=0, gscale=1.0):
    """The GPU test's operands: its edge-shape inputs, or one of its value cases -> x, gamma, the given statistics, dA, dP."""
    B, H, W, C = shape
    bf = dt == BF16
    if kind == "edge":
        x, gamma, beta, dA, dP = BB.edge_input(shape, bf)
        return x, gamma, BB.given_stats(x, gamma, beta), dA, dP
    x = BB.value_input(kind, B, H, W, C, bf, seed)
    gamma, beta = BB.params(C, seed, gscale)
    st = BB.given_stats(x, gamma, beta)
    dA, dP = BB.grads(B, H, W, C, bf, seed)
    return x, gamma, st, dA, dP


# ---------------------------------------------------------------------------------------------------- restated host code
def test_plan_table():
    for (B, H, W, C), (slabs, used, last) in PLAN.items():
        p = BB.plan(B * H * W, C)
        assert (p["slabs"], p["used"], p["last"]) == (slabs, used, last), ((B, H, W, C), p)
        assert BB.ws_floats(B * H * W, C) == 4 * slabs * C + 2 * C
        assert BB.coef_offset(B * H * W, C) + 2 * C <= BB.ws_floats(B * H * W, C)
    assert [BB.chan_width(c) for c in (1, 2, 3, 20, 33, 64, 65, 512)] == [1, 2, 4, 32, 64, 64, 64, 64]
    assert BB.plan(4355, 65)["gx"] == 2 and BB.plan(4355, 512)["gx"] == 8 and BB.plan(4, 33)["CW"] == 64
    assert BB.plan(4355, 64)["rows"] == 4 and BB.plan(4355, 64)["last"] < 4            # a last slab shorter than the row threads
    assert BB.plan(263169, 1)["rows"] == 256 and BB.plan(263169, 1)["used"] > 256      # the second trip of slab_sums


def test_eps_and_lipschitz_constants():
    assert BB.EPS32 != 1e-5 and abs(BB.EPS32 - 1e-5) < 1e-5 * BB.U32
    x = torch.linspace(-8, 8, 1600001, dtype=torch.float64)
    d2 = torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi) * (2 - x * x)
    assert float(d2.abs().max()) < BB.L_DGELU
    d = BB.dgelu_erff(x)[0]
    assert float(((d[1:] - d[:-1]) / (x[1:] - x[:-1])).abs().max()) < BB.L_DGELU and float(d.abs().max()) < BB.L_GELU


def test_fp32_evaluation_of_dgelu_erff_is_inside_its_bound():
    x = torch.linspace(-14, 14, 400001, dtype=torch.float64).float()
    d, e = BB.dgelu_erff(x.double())
    assert float(((dgelu_erff32(x).double() - d).abs() / e).max()) <= 1.0
    a, e = BB.act(x, torch.ones(1), torch.zeros(1))
    assert float(((gelu_erff32(x).double() - a).abs() / e.clamp_min(1e-300)).max()) <= 1.0


# ---------------------------------------------------------------------------------------------------- emulations stay inside
SHAPES = [(1, 1, 2, 1), (1, 2, 2, 33), (2, 5, 7, 3), (3, 5, 7, 20), (1, 3, 107, 64), (1, 65, 67, 65)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", SHAPES)
def test_fwd_emulation_inside(dt, order, shape):
    B, H, W, C = shape
    x = BB.stored(BB.randn(B, H, W, C, scale=1.5, shift=0.3, seed=C), dt == BF16)
    gamma, beta = BB.params(C, C)
    rm, rv = _running(C, C)
    _check_fwd(emu_fwd(x, gamma, beta, rm, rv, order=order), BB.stats(x, gamma, beta, rm, rv), f"fwd {dt} {order} {shape}")
    _check_fwd(emu_fwd(x, gamma, beta, order=order), BB.stats(x, gamma, beta), f"fwd {dt} {order} {shape} no running")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind", ["large_mean", "constant", "scales", "ties"])
def test_fwd_value_cases_inside(dt, order, kind):
    B, H, W, C = 3, 5, 7, 20
    x = BB.value_input(kind, B, H, W, C, dt == BF16, 1)
    gamma, beta = BB.params(C, 1)
    rm, rv = _running(C, 1)
    ref = BB.stats(x, gamma, beta, rm, rv)
    _check_fwd(emu_fwd(x, gamma, beta, rm, rv, order=order), ref, f"fwd {kind} {dt} {order}")
    if kind == "constant":
        assert float((ref["rstd"][0][3] - BB.EPS32 ** -0.5).abs()) < 1e-9
        assert float(ref["rstd"][1][3]) <= 2.0 ** -16 * (1 + 1e-3)                   # half an ulp at 316.2


def test_eval_emulation_inside():
    C = 37
    gamma, beta = BB.params(C, 2)
    rm, rv = _running(C, 2)
    rv[4] = 0.0
    ref = BB.eval_affine(gamma, beta, rm, rv)
    got = emu_eval(gamma, beta, rm, rv)
    for k in ("sc", "sh"):
        BB.check(got[k], *ref[k], "eval " + k, ("channel",))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [(1, 2, 2, 33), (3, 5, 7, 20), (1, 3, 107, 64)])
@pytest.mark.parametrize("kind", ["plain", "ties"])
def test_act_and_pool_emulation_inside(dt, shape, kind):
    B, H, W, C = shape
    x = BB.value_input(kind, B, H, W, max(C, 20), dt == BF16, 3)[..., :C].contiguous()
    gamma, beta = BB.params(C, 3, gscale=2.5)
    _, _, sc, sh = BB.given_stats(x, gamma, beta)
    a, p, idx = emu_act(x, sc, sh, dt, pool=True)
    BB.check(a, *BB.act(x, sc, sh, dt == BF16), f"act {dt} {shape}", ("frame", "y", "x", "channel"))
    assert torch.equal(emu_act(x, sc, sh, dt), a)
    pw, iw = BB.pool_of_stored(a)
    assert torch.equal(p.double(), pw) and torch.equal(idx, iw)
    if kind == "ties":
        assert bool((idx == 0).all())


@pytest.mark.parametrize("dt", DTS)
def test_pool_rule_with_nan_and_inf(dt):
    """The kernel's rule (a later element wins if strictly greater or NaN) is F.max_pool2d's: a NaN at each position, two in a window
    (the later one wins), a +inf."""
    B, H, W, C = 1, 4, 7, 6
    x = BB.stored(BB.randn(B, H, W, C, seed=5), dt == BF16)
    for k, (y, xx) in enumerate(((0, 0), (0, 3), (3, 0), (3, 3))):
        x[0, y, xx, k] = float("nan")
    x[0, 0, 4, 4], x[0, 1, 5, 4], x[0, 2, 1, 5] = float("nan"), float("nan"), float("inf")
    a, p, idx = emu_act(x, torch.ones(C), torch.zeros(C), dt, pool=True)
    pw, iw = BB.pool_of_stored(a)
    assert torch.equal(torch.isnan(p.double()), torch.isnan(pw)) and torch.equal(torch.nan_to_num(p.double()), torch.nan_to_num(pw))
    assert torch.equal(idx, iw)
    assert [int(idx[0, 0, 0, 0]), int(idx[0, 0, 1, 1]), int(idx[0, 1, 0, 2]), int(idx[0, 1, 1, 3]), int(idx[0, 0, 2, 4])] == [0, 1, 2, 3, 3]
    assert float(p[0, 1, 0, 5]) == float("inf") and int(idx[0, 1, 0, 5]) == 1


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", SHAPES[1:])
def test_bwd_emulation_inside(dt, order, shape):
    """dA alone, dP alone, both; dA as a channel slice (offA = 5, ldA = C + 7); accumulate = 1 on nonzero priors; hand-made index bytes."""
    B, H, W, C = shape
    x = BB.stored(BB.randn(B, H, W, C, scale=1.5, shift=0.3, seed=C), dt == BF16)
    gamma, beta = BB.params(C, C)
    st = BB.given_stats(x, gamma, beta)
    dA, dP = BB.grads(B, H, W, C, dt == BF16, C)
    idx = torch.randint(0, 4, dP.shape, generator=torch.Generator().manual_seed(C), dtype=torch.uint8)
    prior = (BB.randn(C, seed=7).float(), BB.randn(C, seed=8).float())
    for a_, p_, pr in ((dA, None, None), (None, dP, None), (dA, dP, None), (dA, dP, prior)):
        got = emu_bwd(None if a_ is None else BB.wide(a_), BB.OFFA, p_, idx, x, gamma, *st, dt, order, pr)
        ref = BB.bwd(a_, p_, idx, x, gamma, *st, *(pr or (None, None)), bf16=dt == BF16)
        _check_bwd(got, ref, f"bwd {dt} {order} {shape} dA{a_ is not None} dP{p_ is not None} acc{pr is not None}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind", ["dA_const", "dP_xhat", "gelu_range", "ties", "large_mean", "scales"])
def test_bwd_value_cases_inside(dt, order, kind):
    shape = (3, 5, 7, 20)
    xkind = kind if kind in ("ties", "large_mean", "scales") else "plain"
    x, gamma, st, dA, dP = _bwd_case(shape, dt, xkind, seed=0 if xkind == kind else 4, gscale=3.0 if kind == "gelu_range" else 1.0)
    a, p, idx = emu_act(x, st[2], st[3], dt, pool=True)
    if kind == "dA_const":
        dA = torch.full_like(dA, 0.75)
    if kind == "dP_xhat":
        xh = (x - st[0].double()) * st[1].double()
        dP = BB.stored(0.5 * xh[:, 0:4:2, 0:6:2], dt == BF16)
    if kind == "gelu_range":
        z = x * st[2].double() + st[3].double()
        assert float(z.min()) < -6 and float(z.max()) > 6
    got = emu_bwd(dA.float(), 0, dP, idx, x, gamma, *st, dt, order)
    _check_bwd(got, BB.bwd(dA, dP, idx, x, gamma, *st, bf16=dt == BF16), f"bwd {kind} {dt} {order}")


# ---------------------------------------------------------------------------------------------------- the reference is the gradient
@pytest.mark.parametrize("shape", [(2, 5, 7, 3), (2, 4, 6, 5)])
def test_closed_form_equals_autograd(shape):
    B, H, W, C = shape
    x, dA = BB.randn(B, H, W, C, scale=1.5, shift=0.3, seed=1), BB.randn(B, H, W, C, seed=2)
    dP = BB.randn(B, H // 2, W // 2, C, seed=3)
    gamma, beta = BB.randn(C, scale=0.4, shift=1.0, seed=4), BB.randn(C, scale=0.5, seed=5)
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    a = F.gelu(F.batch_norm(xr.permute(0, 3, 1, 2), None, None, gr, br, training=True, eps=BB.EPS32))
    p, iw = F.max_pool2d(a, 2, 2, return_indices=True)
    ((a * dA.permute(0, 3, 1, 2)).sum() + (p * dP.permute(0, 3, 1, 2)).sum()).backward()
    idx = BB.window_pos(iw, W).permute(0, 2, 3, 1).to(torch.uint8)
    xm = x.reshape(-1, C)
    mean, rstd = xm.mean(0), (xm.var(0, unbiased=False) + BB.EPS32) ** -0.5
    sc = gamma * rstd
    ref = BB.bwd(dA, dP, idx, x, gamma, mean, rstd, sc, beta - mean * sc)
    rel = lambda u, v: float((u - v).norm() / v.norm())
    assert rel(ref["dx"][0], xr.grad) < 1e-12 and rel(ref["dgamma"][0], gr.grad) < 1e-12 and rel(ref["dbeta"][0], br.grad) < 1e-12


# ---------------------------------------------------------------------------------------------------- mutants are rejected
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mutant", ["biased_running", "unbiased_rstd"])
def test_mutant_unbiased_factor(dt, mutant):
    """n / (n - 1) belongs in running_var and nowhere else; at 105 pixels it is 1 % of the variance."""
    C = 20
    x, gamma, beta, _, _ = BB.edge_input((3, 5, 7, C), dt == BF16)
    rm, rv = _running(C, C)
    ref = BB.stats(x, gamma, beta, rm, rv)
    _check_fwd(emu_fwd(x, gamma, beta, rm, rv), ref, "good")
    _rejected(lambda: _check_fwd(emu_fwd(x, gamma, beta, rm, rv, mutant=mutant), ref, mutant))
    M = 4355
    assert M / (M - 1.0) - 1 > 100 * BB.U32                                                  # and still visible at the large shape


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [(3, 5, 7, 20), (1, 65, 67, 64)])
def test_mutant_eps_literal(dt, shape):
    """1e-5 for its fp32 value moves rstd by 1.26e-8 relative where var << eps: a fifth of u, seen only because rstd is held to half an
    ulp of its binade.  The constant channel and the near-constant ones between them must catch it."""
    B, H, W, C = shape
    x = BB.value_input("constant", B, H, W, C, dt == BF16, 0)
    gamma, beta = BB.params(C, 0)
    ref = BB.stats(x, gamma, beta)
    _check_fwd(emu_fwd(x, gamma, beta), ref, "good")
    _rejected(lambda: _check_fwd(emu_fwd(x, gamma, beta, mutant="eps_literal"), ref, "eps literal"))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mutant,shape", [("drop_last_slab", (1, 3, 107, 64)), ("drop_last_slab", (1, 65, 67, 64)),
                                          ("first_trip_only", (1, 65, 67, 64)), ("first_trip_only", (1, 65, 67, 65))])
def test_mutant_slab_sums(dt, mutant, shape):
    x, gamma, beta, _, _ = BB.edge_input(shape, dt == BF16)
    ref = BB.stats(x, gamma, beta)
    _check_fwd(emu_fwd(x, gamma, beta), ref, "good")
    _rejected(lambda: _check_fwd(emu_fwd(x, gamma, beta, mutant=mutant), ref, mutant))


@pytest.mark.parametrize("dt", DTS)
def test_mutant_coef_behind_all_slabs(dt):
    """used = 19 of 20 slabs: coef lives behind the 19 that are written."""
    shape = (1, 3, 107, 64)
    x, gamma, st, dA, dP = _bwd_case(shape, dt)
    assert BB.coef_offset(321, 64) < 2 * 20 * 64 * 2
    ref = BB.bwd(dA, None, None, x, gamma, *st, bf16=dt == BF16)
    _check_bwd(emu_bwd(dA.float(), 0, None, None, x, gamma, *st, dt), ref, "good")
    _rejected(lambda: _check_bwd(emu_bwd(dA.float(), 0, None, None, x, gamma, *st, dt, mutant="coef_at_slabs"), ref, "coef"))


@pytest.mark.parametrize("dt", DTS)
def test_mutant_tie_routed_to_the_last_element(dt):
    shape = (3, 5, 7, 20)
    x, gamma, st, dA, dP = _bwd_case(shape, dt, "ties")
    a, p, idx = emu_act(x, st[2], st[3], dt, pool=True)
    a2, p2, idx2 = emu_act(x, st[2], st[3], dt, pool=True, mutant="tie_last")
    assert torch.equal(idx, BB.pool_of_stored(a)[1]) and not torch.equal(idx2, idx) and torch.equal(p2, p)
    ref = BB.bwd(None, dP, idx, x, gamma, *st, bf16=dt == BF16)
    _check_bwd(emu_bwd(None, 0, dP, idx, x, gamma, *st, dt), ref, "good")
    _rejected(lambda: _check_bwd(emu_bwd(None, 0, dP, idx2, x, gamma, *st, dt), ref, "tie last"))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [(3, 5, 7, 20), (1, 65, 67, 64)])
@pytest.mark.parametrize("mutant", ["partial_windows", "no_s2", "no_dgelu", "offA_ignored", "acc_overwrite"])
def test_mutant_backward(dt, shape, mutant):
    x, gamma, st, dA, dP = _bwd_case(shape, dt)
    a, p, idx = emu_act(x, st[2], st[3], dt, pool=True)
    prior = BB.priors(shape[3], 1)
    ref = BB.bwd(dA, dP, idx, x, gamma, *st, *prior, bf16=dt == BF16)
    _check_bwd(emu_bwd(BB.wide(dA), BB.OFFA, dP, idx, x, gamma, *st, dt, prior=prior), ref, "good")
    _rejected(lambda: _check_bwd(emu_bwd(BB.wide(dA), BB.OFFA, dP, idx, x, gamma, *st, dt, prior=prior, mutant=mutant), ref, mutant))


def test_mutant_bf16_rounded_twice():
    """The GELU argument (act) or the bracket of dx rounded to bf16 before the last operation and again at the store."""
    shape = (1, 65, 67, 64)
    x, gamma, st, dA, dP = _bwd_case(shape, BF16)
    ref = BB.act(x, st[2], st[3], True)
    BB.check(emu_act(x, st[2], st[3], BF16), *ref, "act", ("frame", "y", "x", "channel"))
    _rejected(lambda: BB.check(emu_act(x, st[2], st[3], BF16, mutant="double_round"), *ref, "act twice", ("frame", "y", "x", "channel")))
    ref = BB.bwd(dA, None, None, x, gamma, *st, bf16=True)
    _check_bwd(emu_bwd(dA.float(), 0, None, None, x, gamma, *st, BF16), ref, "good")
    _rejected(lambda: _check_bwd(emu_bwd(dA.float(), 0, None, None, x, gamma, *st, BF16, mutant="double_round"), ref, "dx twice"))
