"""CPU: pins tests/norm_bounds.py.  An fp32 emulation of the InstanceNorm kernels' arithmetic (statistics in one workgroup and sliced +
merged, the apply, the backward in both of its forms, the parameter-gradient reductions with and without a workspace, the column sums)
in two accumulation orders must fall inside the bound for every mode and both store types; the same emulation with one defect each of
the kind these kernels can have must be rejected; the closed-form backward reference must equal fp64 autograd at exact statistics; and
the restated host code is pinned to the geometry table of norm.hip."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_bounds as GB
from tests import norm_bounds as NB
from tests.test_gemm_bounds import dgelu32, fma32

F32, BF16 = torch.float32, torch.bfloat16
DTS = [F32, BF16]
ORDERS = ["tree", "seq"]


def _randn(*shape, scale=1.0, shift=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift


def _st(t, dt):
    return t.to(dt).double()


# ---------------------------------------------------------------------------------------------------- fp32 emulation
def sum32(t, order, rg):
    """Sum t (..., n, C) over n in fp32.  fp64 terms (exact products of fp32 values) are rounded once into the accumulator: an fma.
    "tree": lane r takes rows r, r + rg, ... in order, then the lanes meet in a halving tree (reduce_rows); "seq": row after row."""
    n, C = t.shape[-2:]
    lead = t.shape[:-2]
    if order == "tree":
        q = -(-n // rg)
        t = torch.cat([t, torch.zeros(*lead, q * rg - n, C, dtype=t.dtype)], -2).reshape(*lead, q, rg * C)
    acc = torch.zeros(*lead, t.shape[-1], dtype=F32)
    for i in range(t.shape[-2]):
        acc = (acc.double() + t[..., i, :].double()).float()
    if order == "tree":
        acc = acc.reshape(*lead, rg, C)
        s = rg // 2
        while s > 0:
            acc = acc[..., :s, :] + acc[..., s:2 * s, :]
            s //= 2
        acc = acc[..., 0, :]
    return acc


def emu_moments(x, order, rg, fused, n=None, one_pass=False):
    """One workgroup's two passes over x (..., rows, C) fp32, dividing by n (default: the rows present)."""
    n = n or x.shape[-2]
    mu = sum32(x, order, rg) / n
    if one_pass:
        return mu, (sum32(x * x, order, rg) / n - mu * mu) * n
    d = x - mu.unsqueeze(-2)
    return mu, sum32(d.double() * d.double() if fused else d * d, order, rg)


def emu_stats(x, w, b, g=None, gdiv=1, gb=None, order="tree", rg=16, slices=None, mutant=None):
    """in_stats_kernel (slices None) or in_stats_slice_kernel + in_stats_merge_kernel; g / gb (groups, C) as the kernel indexes them."""
    Fr, S, C = x.shape
    x = x.float()
    if slices is None:
        mu, q = emu_moments(x, order, rg, True, one_pass=mutant == "one_pass")
    else:
        ms, qs, ns = [], [], []
        for s0 in range(0, S, slices):
            n = min(slices, S - s0)
            xs = x[:, s0:s0 + n]
            if mutant == "drop_last_row" and n < slices:
                xs = xs[:, :n - 1]
            m_i, q_i = emu_moments(xs, order, rg, False, n=n)
            ms.append(m_i), qs.append(q_i), ns.append(float(slices if mutant == "weight_rows" else n))
        ms, qs = torch.stack(ms, 1), torch.stack(qs, 1)                  # (F, N, C)
        nn = torch.tensor(ns, dtype=F32).view(1, -1, 1)
        if mutant == "div_by_slices":
            mu = sum32(ms, order, 4) / len(ns)
        else:
            mu = sum32(ms * nn, order, 4) / S
        dm = ms - mu[:, None]
        q = sum32(qs if mutant == "no_between" else qs + dm * dm * nn, order, 4)
    v = q / S if mutant == "no_eps" else q / S + NB.EPS
    r = v.rsqrt()
    a = r * w
    s0 = fma32(-mu, a, b) if slices is None else b - mu * a
    if g is not None:
        fi = torch.arange(Fr)
        gi = fi % gdiv if mutant == "g_mod" else fi // gdiv
        a = a * g[gi]
        s0 = s0 * g[gi]
        if gb is not None and mutant != "no_gb":
            s0 = s0 + gb[gi]
    return dict(mean=mu, rstd=r, sc=a, sh=s0)


def emu_apply(z, sc, sh, resid, dt, mutant=None):
    t = fma32(z.float(), sc[:, None], sh[:, None] if sh is not None else torch.zeros(()))
    if mutant == "double_round":
        t = t.to(dt).float()
    if resid is not None:
        t = t + resid.float()
    return t.to(dt)


def emu_bwd(dy, x, mean, rstd, w, b, g=None, gdiv=1, add=None, gelu=False, dt=F32, order="tree", rg=16, slice_rows=None, ws=True,
            prior=None, want=("dw", "db", "dg", "dgb"), mutant=None):
    """in_bwd_kernel (slice_rows None) or the sliced three-launch form, then in_reduce_block (ws) or the float atomics."""
    Fr, S, C = x.shape
    bf = dt == BF16
    dy, x = dy.float(), x.float()
    mu, rs = mean[:, None], rstd[:, None]
    xh = (x - mu) * rs
    dd = dy * dgelu32(xh * w + b, bf) if (gelu and mutant != "no_dgelu") else dy
    gf = torch.ones(Fr, C) if g is None else g[torch.arange(Fr) // gdiv]
    if slice_rows is None:
        s1, s2 = sum32(dd, order, rg), sum32(dd * xh, order, rg)
        inner = dd - s1[:, None] / S if mutant == "no_s2" else dd - (s1[:, None] + xh * s2[:, None]) / S
    else:
        p1 = torch.stack([sum32(dd[:, s0:s0 + slice_rows], order, rg) for s0 in range(0, S, slice_rows)], 1)
        p2 = torch.stack([sum32((dd * xh)[:, s0:s0 + slice_rows], order, rg) for s0 in range(0, S, slice_rows)], 1)
        s1, s2 = sum32(p1, order, 4), sum32(p2, order, 4)
        inner = dd - (s1 / S)[:, None] if mutant == "no_s2" else dd - (s1 / S)[:, None] - xh * (s2 / S)[:, None]
    t = rs * w * gf[:, None] * inner
    if add is not None:
        t = t + add.float()
    out = dict(dx=t.to(dt))
    prior = prior or {}
    grp = torch.arange(Fr) // gdiv
    ng = int(grp.max()) + 1
    pr = lambda k, shape: prior[k].clone() if k in prior else torch.zeros(shape)
    gdb = torch.ones(Fr, C) if mutant == "db_no_g" else gf
    bterm = torch.zeros(C) if mutant == "dg_no_b" else b
    if ws:
        out["dw"] = pr("dw", C) + sum32(gf * s2, order, 16)
        out["db"] = pr("db", C) + sum32(gdb * s1, order, 16)
        dg, dgb = pr("dg", (ng, C)), pr("dgb", (ng, C))
        for k in range(ng):
            S1, S2 = sum32(s1[grp == k], order, 16), sum32(s2[grp == k], order, 16)
            dg[k] += w * S2 + bterm * S1
            dgb[k] += S1
    else:
        dw, db, dg, dgb = pr("dw", C), pr("db", C), pr("dg", (ng, C)), pr("dgb", (ng, C))
        for f in (range(Fr) if order == "seq" else reversed(range(Fr))):      # atomics land in any order
            dw += gf[f] * s2[f]
            db += gdb[f] * s1[f]
            dg[grp[f]] += w * s2[f] + bterm * s1[f]
            dgb[grp[f]] += s1[f]
        out["dw"], out["db"] = dw, db
    out["dg"], out["dgb"] = dg, dgb
    return out


def emu_colsum(x, scale, prior, order):
    rpb, nblk = NB.colsum_split(*x.shape)
    out = prior.clone() if prior is not None else torch.zeros(x.shape[1])
    for k in (range(nblk) if order == "seq" else reversed(range(nblk))):
        part = sum32(x[k * rpb:(k + 1) * rpb].float(), order, 16)
        out += part * scale if scale is not None else part
    return out


# ---------------------------------------------------------------------------------------------------- cases
def _film(Fr, gdiv, C, seed, with_gb=True):
    ng = -(-Fr // gdiv)
    g = _randn(ng, C, scale=0.3, shift=1.0, seed=seed).float()
    return g, (_randn(ng, C, scale=0.5, seed=seed + 1).float() if with_gb else None)


def _stats_case(dt, S, C=16, Fr=5, scale=1.5, shift=0.3, seed=0):
    x = _st(_randn(Fr, S, C, scale=scale, shift=shift, seed=seed), dt)
    return x, _randn(C, scale=0.4, shift=1.0, seed=seed + 1).float(), _randn(C, scale=0.5, seed=seed + 2).float()


def _check_stats(got, ref, what):
    return max(NB.check(got[k], *ref[k], f"{what} {k}", ("frame", "channel")) for k in ("mean", "rstd", "sc", "sh"))


def _exp(g, gdiv, Fr):
    return None if g is None else g[torch.arange(Fr) // gdiv]


# ---------------------------------------------------------------------------------------------------- emulations stay inside
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("S,slices", [(1, None), (37, None), (96, None), (97, 96), (250, 48), (430, 48)])
@pytest.mark.parametrize("film", ["none", "g", "g+gb"])
def test_stats_emulation_inside(dt, order, S, slices, film):
    Fr, gdiv = 5, 2
    for shift, scale in ((0.3, 1.5), (100.0, 3.0)):
        x, w, b = _stats_case(dt, S, shift=shift, scale=scale, seed=S)
        g, gb = _film(Fr, gdiv, 16, 7, film == "g+gb") if film != "none" else (None, None)
        got = emu_stats(x, w, b, g, gdiv, gb, order, 16, slices)
        ref = NB.in_stats(x, w, b, _exp(g, gdiv, Fr), _exp(gb, gdiv, Fr), slices)
        _check_stats(got, ref, f"stats {dt} {order} S{S} slices{slices} {film} shift{shift}")


@pytest.mark.parametrize("order", ORDERS)
def test_stats_constant_channel_inside(order):
    """Variance 0: rstd = eps^-1/2 to within the rounding of the mean (a sum of equal values is not exact)."""
    for dt, c in ((F32, 0.7), (BF16, 3.0)):
        x = torch.full((3, 50, 8), c, dtype=torch.float64)
        x = _st(x, dt)
        w, b = torch.ones(8), torch.zeros(8)
        ref = NB.in_stats(x, w, b)
        _check_stats(emu_stats(x, w, b, order=order), ref, f"constant {dt}")
        assert float((ref["rstd"][0] - NB.EPS ** -0.5).abs().max()) < 1e-9


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("rows", [128, 256])
def test_merge_of_given_partials_inside(order, rows):
    Fr, S, C, gdiv = 3, 3 * rows + 7, 16, 2
    N = -(-S // rows)
    pm, pq = _randn(Fr, N, C, scale=0.2, shift=0.5, seed=1).float(), (_randn(Fr, N, C, seed=2).abs() * rows).float()
    w, b = _randn(C, shift=1.0, scale=0.3, seed=3).float(), _randn(C, seed=4).float()
    g, gb = _film(Fr, gdiv, C, 5)
    nn = torch.tensor([min(rows, S - i * rows) for i in range(N)], dtype=F32).view(1, -1, 1)
    mu = sum32(pm * nn, order, 4) / S
    dm = pm - mu[:, None]
    q = sum32(pq + dm * dm * nn, order, 4)
    r = (q / S + NB.EPS).rsqrt()
    a = r * w
    s0 = b - mu * a
    gi = torch.arange(Fr) // gdiv
    got = dict(mean=mu, rstd=r, sc=a * g[gi], sh=s0 * g[gi] + gb[gi])
    _check_stats(got, NB.merge(pm, pq, rows, S, w, b, g[gi], gb[gi]), f"merge rows{rows} {order}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("resid", [False, True])
@pytest.mark.parametrize("sh", [False, True])
def test_apply_emulation_inside(dt, resid, sh):
    Fr, S, C = 3, 20, 16
    z, r = _st(_randn(Fr, S, C, seed=1), dt), _st(_randn(Fr, S, C, seed=2), dt)
    sc, shv = _randn(Fr, C, shift=1.0, scale=0.3, seed=3).float(), _randn(Fr, C, seed=4).float()
    got = emu_apply(z, sc, shv if sh else None, r if resid else None, dt)
    NB.check(got, *NB.affine_apply(z, sc, shv if sh else None, r if resid else None, dt == BF16), "apply", ("frame", "row", "channel"))


def _bwd_case(dt, S, C=16, Fr=5, seed=0, stats_exact=False, zscale=1.0):
    x = _st(_randn(Fr, S, C, scale=1.5, shift=0.3, seed=seed), dt)
    dy, add = _st(_randn(Fr, S, C, seed=seed + 1), dt), _st(_randn(Fr, S, C, seed=seed + 2), dt)
    w, b = (_randn(C, scale=0.4, shift=1.0, seed=seed + 3) * zscale).float(), _randn(C, scale=0.5, seed=seed + 4).float()
    mean = x.mean(1)
    rstd = (x.var(1, unbiased=False) + NB.EPS) ** -0.5
    if not stats_exact:
        mean, rstd = mean.float(), rstd.float()
    return x, dy, add, w, b, mean, rstd


def _check_bwd(got, ref, pg, what, want=("dw", "db", "dg", "dgb")):
    worst = NB.check(got["dx"], *ref["dx"], what + " dx", ("frame", "row", "channel"))
    for k in want:
        worst = max(worst, NB.check(got[k], *pg[k], f"{what} {k}", ("group", "channel")))
    return worst


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("S,slice_rows", [(1, None), (37, None), (430, None), (430, 192)])
@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("ws", [False, True])
def test_bwd_emulation_inside(dt, order, S, slice_rows, gelu, ws):
    Fr, C = 5, 16
    x, dy, add, w, b, mean, rstd = _bwd_case(dt, S, seed=S)
    for gdiv, with_g, with_add in ((1, False, False), (2, True, True), (Fr, True, False)):
        g, _ = _film(Fr, gdiv, C, 9, False) if with_g else (None, None)
        prior = {k: _randn(*((C,) if k in ("dw", "db") else (-(-Fr // gdiv), C)), seed=20 + i).float() for i, k in enumerate(("dw", "db", "dg", "dgb"))}
        got = emu_bwd(dy, x, mean, rstd, w, b, g, gdiv, add if with_add else None, gelu, dt, order, 16, slice_rows, ws, prior)
        ns = 0 if slice_rows is None else -(-S // slice_rows)
        ref = NB.in_bwd(dy, x, mean, rstd, w, b, _exp(g, gdiv, Fr), add if with_add else None, gelu, dt == BF16, ns)
        _check_bwd(got, ref, NB.param_grads(ref["s1"], ref["s2"], w, b, g, gdiv, prior, gelu), f"bwd {dt} {order} S{S} sl{slice_rows} gelu{gelu} ws{ws} gdiv{gdiv}",
                   ("dw", "db") if gelu else ("dw", "db", "dg", "dgb"))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("order", ORDERS)
def test_bwd_cancelling_inputs_inside(dt, order):
    """dy constant over a frame (dx cancels through s1), dy proportional to xhat (through s2), GELU arguments on both sides of |z| = 4."""
    Fr, S, C = 3, 60, 16
    x, dy, add, w, b, mean, rstd = _bwd_case(dt, S, seed=3)
    xh = (x - mean.double()[:, None]) * rstd.double()[:, None]
    for name, d, gelu, zs in (("const", torch.ones_like(dy) * 0.75, False, 1.0), ("xhat", _st(xh * 0.5, dt), False, 1.0), ("clamp", dy, True, 2.5)):
        x, _, _, w, b, mean, rstd = _bwd_case(dt, S, seed=3, zscale=zs)
        got = emu_bwd(d, x, mean, rstd, w, b, gelu=gelu, dt=dt, order=order)
        ref = NB.in_bwd(d, x, mean, rstd, w, b, gelu=gelu, bf16=dt == BF16)
        _check_bwd(got, ref, NB.param_grads(ref["s1"], ref["s2"], w, b), f"bwd {name} {dt}")
        if name != "clamp":
            assert float(ref["dx"][0].abs().max()) < 1e-2 * float(d.abs().max()), "the case does not cancel"
        else:
            z = xh * w.double() + b.double()
            assert float(z.abs().max()) > 4.5 and float((z.abs() < 4).double().mean()) > 0.3


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("nrows", [5, 700, 70000])
def test_colsum_emulation_inside(dt, order, nrows):
    C = 8
    x = _st(_randn(nrows, C, shift=0.2, seed=nrows), dt)
    scale, prior = _randn(C, seed=1).float(), _randn(C, seed=2).float()
    for sc, pr in ((None, None), (scale, prior)):
        NB.check(emu_colsum(x, sc, pr, order), *NB.colsum(x, sc, pr), f"colsum {dt} {nrows}", ("channel",))


# ---------------------------------------------------------------------------------------------------- the reference is the gradient
@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("gdiv", [0, 1, 2, 5])
def test_closed_form_equals_autograd(gelu, gdiv):
    """Exact fp64 statistics: dx, dw, db, dg, dgb of the closed form against autograd of F.instance_norm [+ F.gelu] [* g + gb].  Behind a
    GELU the group gradients are not made of the kernels' two sums (dg = sum dy gelu(z)): bf_in_bwd refuses that combination and the
    closed form has no dg / dgb to compare."""
    Fr, S, C = 5, 23, 8
    x, dy, add, w, b, mean, rstd = _bwd_case(torch.float64, S, C, Fr, seed=1, stats_exact=True)
    w, b = w.double(), b.double()
    g = _randn(-(-Fr // gdiv), C, shift=1.0, scale=0.3, seed=2) if gdiv else None
    ref = NB.in_bwd(dy, x, mean, rstd, w, b, _exp(g, gdiv, Fr) if gdiv else None, None, gelu, False)
    pg = NB.param_grads(ref["s1"], ref["s2"], w, b, g, gdiv or 1, gelu=gelu)
    assert ("dg" in pg) == (not gelu)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    gr = g.clone().requires_grad_(True) if gdiv else None
    gbr = torch.zeros_like(g).requires_grad_(True) if gdiv else None
    y = F.instance_norm(xr.permute(0, 2, 1), weight=wr, bias=br, eps=NB.EPS).permute(0, 2, 1)
    if gelu:
        y = F.gelu(y)
    if gdiv:
        gi = torch.arange(Fr) // gdiv
        y = y * gr[gi][:, None] + gbr[gi][:, None]
    (y * dy).sum().backward()
    pairs = [("dx", ref["dx"][0], xr.grad), ("dw", pg["dw"][0], wr.grad), ("db", pg["db"][0], br.grad)]
    if gdiv and not gelu:
        pairs += [("dg", pg["dg"][0], gr.grad), ("dgb", pg["dgb"][0], gbr.grad)]
    for name, a, e in pairs:
        assert NB.rel_l2(a, e) < 1e-12, (name, NB.rel_l2(a, e))


def test_gelu_second_derivative_is_pinned():
    """L_DGELU bounds the slope of gelu' -- exactly 2 phi(0) at 0 -- and of the polynomial form bf16 kernels evaluate."""
    x = torch.linspace(-8, 8, 1600001, dtype=torch.float64)
    d2 = torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi) * (2 - x * x)
    assert abs(float(d2.abs().max()) - 2 / math.sqrt(2 * math.pi)) < 1e-12 and 2 / math.sqrt(2 * math.pi) < NB.L_DGELU
    p = GB.dgelu_poly(x)[0]
    slope = ((p[1:] - p[:-1]) / (x[1:] - x[:-1])).abs().max()
    assert float(slope) < NB.L_DGELU, float(slope)


# ---------------------------------------------------------------------------------------------------- mutants are rejected
def _rejected(fn):
    with pytest.raises(AssertionError, match="exceeds the bound"):
        fn()


def test_mutant_one_pass_variance():
    x, w, b = _stats_case(F32, 60, shift=300.0, scale=1.0, seed=1)                       # |mean| / std = 300
    ref = NB.in_stats(x, w, b)
    _check_stats(emu_stats(x, w, b), ref, "two-pass")
    _rejected(lambda: _check_stats(emu_stats(x, w, b, mutant="one_pass"), ref, "one-pass"))


def test_mutant_eps_left_out():
    x = torch.full((2, 40, 8), 0.5, dtype=torch.float64)
    x[:, :, 1:] = _randn(2, 40, 7, scale=1e-4, seed=1).float().double()                   # small-variance channels beside the constant one
    w, b = torch.ones(8), torch.zeros(8)
    ref = NB.in_stats(x, w, b)
    _check_stats(emu_stats(x, w, b), ref, "with eps")
    got = emu_stats(x, w, b, mutant="no_eps")
    got = {k: torch.nan_to_num(v, nan=0.0, posinf=3e38, neginf=-3e38) for k, v in got.items()}
    _rejected(lambda: _check_stats(got, ref, "no eps"))


@pytest.mark.parametrize("mutant", ["drop_last_row", "weight_rows", "div_by_slices", "no_between"])
@pytest.mark.parametrize("dt", DTS)
def test_mutant_sliced_statistics(mutant, dt):
    """Two full slices and a ragged one of 5 rows, slice means that differ (a drift along the frame)."""
    S, rows = 2 * 48 + 5, 48
    x, w, b = _stats_case(dt, S, seed=2)
    x = _st(x + torch.linspace(-1, 1, S, dtype=torch.float64)[None, :, None], dt)
    ref = NB.in_stats(x, w, b, slices=rows)
    _check_stats(emu_stats(x, w, b, slices=rows), ref, "sliced")
    _rejected(lambda: _check_stats(emu_stats(x, w, b, slices=rows, mutant=mutant), ref, mutant))


@pytest.mark.parametrize("mutant", ["g_mod", "no_gb"])
def test_mutant_film_indexing(mutant):
    Fr, gdiv = 5, 2
    x, w, b = _stats_case(F32, 30, seed=3)
    g, gb = _film(Fr, gdiv, 16, 4)
    ref = NB.in_stats(x, w, b, _exp(g, gdiv, Fr), _exp(gb, gdiv, Fr))
    _check_stats(emu_stats(x, w, b, g, gdiv, gb), ref, "film")
    _rejected(lambda: _check_stats(emu_stats(x, w, b, g, gdiv, gb, mutant=mutant), ref, mutant))


@pytest.mark.parametrize("mutant,key", [("no_s2", "dx"), ("no_dgelu", "dx"), ("dg_no_b", "dg"), ("db_no_g", "db")])
@pytest.mark.parametrize("dt", DTS)
def test_mutant_backward(mutant, key, dt):
    Fr, gdiv, S = 5, 2, 40
    x, dy, add, w, b, mean, rstd = _bwd_case(dt, S, seed=5)
    g, _ = _film(Fr, gdiv, 16, 6, False)
    gelu = key == "dx"
    ref = NB.in_bwd(dy, x, mean, rstd, w, b, _exp(g, gdiv, Fr), add, gelu, dt == BF16)
    pg = NB.param_grads(ref["s1"], ref["s2"], w, b, g, gdiv, gelu=gelu)
    pg["dx"] = ref["dx"]
    names = ("frame", "row", "channel") if key == "dx" else ("group", "channel")
    NB.check(emu_bwd(dy, x, mean, rstd, w, b, g, gdiv, add, gelu, dt)[key], *pg[key], "good", names)
    _rejected(lambda: NB.check(emu_bwd(dy, x, mean, rstd, w, b, g, gdiv, add, gelu, dt, mutant=mutant)[key], *pg[key], mutant, names))


def test_mutant_bf16_rounded_twice():
    """t rounded to bf16 before the residual add and again after it: up to two bf16 half-ulps where the bound allows one."""
    Fr, S, C = 3, 200, 16
    z, r = _st(_randn(Fr, S, C, seed=1), BF16), _st(_randn(Fr, S, C, seed=2), BF16)
    sc, sh = _randn(Fr, C, shift=1.0, scale=0.3, seed=3).float(), _randn(Fr, C, seed=4).float()
    ref = NB.affine_apply(z, sc, sh, r, True)
    NB.check(emu_apply(z, sc, sh, r, BF16), *ref, "apply", ("frame", "row", "channel"))
    _rejected(lambda: NB.check(emu_apply(z, sc, sh, r, BF16, mutant="double_round"), *ref, "double round", ("frame", "row", "channel")))


# ---------------------------------------------------------------------------------------------------- restated host code
def test_geometry_table():
    """norm.hip: MAXR = 6, 16-byte chunks.  (lanes, row groups), cached rows, statistics slice, backward slice."""
    table = {(False, False): ((16, 16), 96, 96, 384), (True, False): ((8, 32), 192, 192, 768),
             (False, True): ((24, 8), 96, 48, 192), (True, True): ((12, 16), 192, 96, 384)}
    for (bf, wide), (lr, cached, srows, brows) in table.items():
        C = 96 if wide else 64
        assert NB.geo(bf, wide)[1:] == lr
        for S in (cached, cached + 1):
            c = NB.slice_cfg(bf, S, C)
            assert (c["cached"], c["rows"], c["wide"], c["sliced"]) == (cached, srows, wide, S > cached)
        p = NB.path(bf, cached + 1, C)
        assert (p["kind"], p["stat_rows"], p["bwd_rows"], p["stat_slices"], p["bwd_slices"]) == ("sliced", srows, brows, 3 if wide else 2, 1)
        assert NB.path(bf, cached + 1, C, ws=False)["kind"] == "uncached" and NB.path(bf, cached, C)["kind"] == "cached"
        assert NB.path(bf, brows + 1, C)["bwd_slices"] == 2
        assert NB.ws_floats(bf, 3, cached, C) == 2 * 3 * C
        assert NB.ws_floats(bf, 3, 5 * srows + 1, C) == 2 * 3 * C * 7
    assert NB.colsum_split(63, 72) == (64, 1) and NB.colsum_split(130, 72) == (64, 3) and NB.colsum_split(70000, 8) == (69, 1015)
