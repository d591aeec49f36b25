"""Per-element error bounds for the InstanceNorm family of csrc/norm.hip (statistics one-workgroup / sliced + merge, affine apply,
backward one-workgroup / sliced, column sums) and the InReduceJob half of csrc/param_reduce.h.

Given the exact (fp64) values a kernel reads, each function returns the fp64 reference `ref` and an elementwise bound `bnd` such that a
correct kernel satisfies |got - ref| <= bnd everywhere.  `check`, `gamma`, `rnd16`, `U32`, `U16`, `rel_l2` are conv_bounds'; the GELU
forms and their evaluation bounds are gemm_bounds'.  u = 2^-24; gamma_n = n u / (1 - n u) bounds a sum of n terms in ANY order (Higham,
Accuracy and Stability of Numerical Algorithms, Thm 3.1), so the row-group strided loads, the lane permutes, the LDS trees, the 4-lane
slice merges, the 16-lane frame sums and the float atomics are all covered by the term count alone.  Every constant is derived here
from the kernels' rounding points; none is fitted to GPU output.  Statistics and parameter gradients are stored in fp32, which the value
already is: no store rounding.  dx and the apply output are rounded to the activation type: |rnd(v) - ref| <= (1 + u_out) |v - ref| +
u_out |ref| with u_out = 2^-8 for bf16; an fp32 store is exact.

Statistics (`in_stats`; in_stats_kernel, in_stats_slice_kernel + in_stats_merge_kernel).  Per (frame, channel), S rows:
  mean.  mh = fl(fl(sum x) / S): |mh - m| <= e_mu = (1 + u) gamma_S sum|x| / S + u |m|.
  second moment.  The kernel sums fl(x - mh)^2.  With the exact identity sum (x - mh)^2 = M2 + S (mh - m)^2 the mean's own error is
    carried, not ignored: Q = sum (x - mh)^2 <= M2 + S e_mu^2.  Each d = fl(x - mh) carries one relative rounding, d * d one more (an
    fma rounds less: the unfused form is charged), the sum gamma_S; every term is non-negative, so the computed value is within
    gamma_{S+3} Q of Q:  e_M2 = S e_mu^2 + gamma_{S+3} (M2 + S e_mu^2).
  rstd.  v = fl(fl(q / S) + eps), eps the fp32 value of 1e-5: e_v = e_M2 / S + u M2 / S + u v (times 1 + 2^-10 for the second-order
    terms).  r = rsqrtf(v).  v^-1/2 is monotone, so the exact inverse root of the computed v lies in [(v + e_v)^-1/2, (v - e_v)^-1/2]
    (to first order d r / r = -1/2 d v / v; the interval form stays valid where e_v is not small beside v, a constant channel of large
    value).  The computed q is >= 0, so v >= eps (1 - 2u) whatever e_v says.  rsqrtf itself: no document shipped with the toolchain
    states its accuracy under the default flags.  ASSUMED: within 1 ulp, E_RSQ = 2u relative -- the figure AMD's CDNA instruction-set
    guides give for v_rsq_f32 (as gemm_bounds assumes for __expf and the reciprocal).
  sc = fl(fl(r w) g): e_a = e_r |w| + u |r w|, then e_a |g| + u |a g|.
  sh.  The one-workgroup kernel computes fmaf(-mu, a, b), the merge kernel b - mu * a, contracted or not.  One bound charges the
    unfused form, u |mu a| + u (|mu a| + |b|), plus the carried |a| e_mu + |mu| e_a + e_mu e_a.  Then s g + gb the same way
    (gb absent: the add of an exact zero is not charged).  Where |mean| / std is large this term is ~ u |mean| / std in absolute
    size while sh itself may cancel to O(1): the bound follows the magnitudes, not the result.
  sliced (`slices=` rows per slice; `slice_cfg` restates the host's choice).  Slice i of n_i rows gives mh_i and q_i exactly as above
    (with n_i for S).  The merge computes mu = fl(sum fl(mh_i n_i) / S): e_mu = (1 + u) (sum n_i e_i + gamma_{N+1} sum n_i (|m_i| +
    e_i)) / S + u |m| over N slices.  The merged second moment is sum_i (q_i + n_i (mh_i - mu)^2); with exact slice values this is the
    identity M2 = sum (M2_i + n_i (m_i - m)^2).  dm_i = fl(mh_i - mu) is within e_d = (e_i + e_mu) (1 + u) + u |m_i - m| of m_i - m;
    dm^2 n_i rounds twice; the term and the N-term sum round N + 2 times more; all terms are non-negative:
      e_M2 = sum_i [e_qi + n_i (2 |m_i - m| e_d + e_d^2)] + gamma_{N+4} sum_i [M2_i + e_qi + n_i (|m_i - m| + e_d)^2].
    `merge` takes slice partials as exact inputs (bf_in_stats_merge_slices, whose partials another kernel wrote): e_i = e_qi = 0.

  carried input (`ex`, one-workgroup form; tests/frame_bounds.py: a norm behind a product that is never stored).  Rows within ex of x
    have their mean within mean(ex) of m and -- centring being an orthogonal projection -- sqrt(M2) within ||ex||_2, so M2 moves by at
    most 2 sqrt(M2) ||ex|| + ||ex||^2; the roundings above are then charged on the rows as carried (|x| + ex, M2 plus that).

Apply (`affine_apply`).  t = fmaf(z, sc, sh): u |t|; + resid: u (|t| + |resid|); store.

Backward (`in_bwd`; in_bwd_kernel, in_bwd_slice_kernel + in_slice_sum_kernel, in_reduce_block).  mean and rstd are the GIVEN fp32
values, exact inputs; the reference is the closed form of the kernel header in fp64 (with inexact statistics that, not autograd, is what
a correct kernel computes; tests/test_norm_bounds.py proves it equals autograd at exact statistics).
  xh = fl(fl(x - mu) rs): e_xh = 2u |xh| (1 + 2^-10).
  GELU argument z = fl(fl(xh w) + b), charged unfused: e_z = e_xh |w| + u |xh w| + u (|xh w| + |b|).  dgelu_t<T>(z): the evaluation
    bound of gemm_bounds.dgelu (polynomial form for bf16, A&S for fp32) plus L_DGELU e_z.  |gelu''(x)| = |phi(x) (2 - x^2)| is largest
    at 0: 2 phi(0) = 0.79788; L_DGELU = 0.80 (the CPU test pins the exact figure and the polynomial form's own slope below it).
    dyn = fl(dy d): e_dyn = |dy| e_d + u |dyn|.  Without GELU dyn = dy, exact.
  s1 = sum dyn, s2 = sum fl(dyn xh): e_s1 = sum e_dyn + gamma_n sum (|dyn| + e_dyn); e_s2 likewise on the products with their carried
    operand errors, n + 1 for the product's rounding.  n = S rows, plus the slice count on the sliced path.
  A gradient that is itself within e_dy of dy (`e_dy`; a fused producer's fp32 accumulator) starts e_dyn at e_dy (behind a GELU: plus
    e_dy (|d| + e_d)); everything below carries it.
  dx.  The one-workgroup kernel forms dyn - (s1 + xh s2) / S (4 roundings), the sliced kernel dyn - s1/S - xh (s2/S) (5).  Each
    rounding is charged u on the magnitude sum Mg = |dyn| + |s1| / S + |xh s2| / S plus the carried error E, not on the cancelled
    result: E_I = E + 5u (Mg + E), E = e_dyn + e_s1 / S + (e_xh |s2| + |xh| e_s2 + e_xh e_s2) / S.  Then P = rs w g and P I: k = 2
    (3 with g) relative roundings, gamma_k |P| (|I| + E_I).  + add: u (|v| + |add| + e).  Store.
  dw = prior + sum_f g s2, db = prior + sum_f g s1: the product, the frames in any order (16 frame lanes in fixed order on the workspace
    path, float atomics without one) and the prior: gamma_{frames+2} on sum_f |g| (|s| + e_s) + |prior|, plus the carried sum |g| e_s.
  dg[group] = prior + sum_{f in group} (w s2 + b s1), dgb = prior + sum s1: the gradients of y = (xhat w + b) g + gb.  (Behind a GELU
    they would be sum dy gelu(z) and sum dy, which the kernels' two sums do not give: bf_in_bwd refuses dg / dgb with gelu.)  The
    workspace path sums the frames, then forms w S2 + b S1; the atomic path forms w s2 + b s1 per frame and adds atomically.  Either
    way a value passes at most n_f + 2 roundings: gamma_{n_f+4} on sum_f (|w s2| + |b s1|) + |prior| covers both.  dgb: gamma_{n_f+1}.

Column sums (`colsum`; colsum_kernel).  out[c] = prior + scale[c] sum_rows x: a block sums its rows (rows per block as bf_colsum sizes
them), scales once, and the blocks meet the prior in float atomics: n = rows per block + blocks + 1, the form of conv_bounds.colsum.
"""
import math

import torch

from tests.conv_bounds import U16, U32, check, gamma, rel_l2, rnd16  # noqa: F401  (re-exported to the tests)
from tests import gemm_bounds as GB

EPS = GB.f32(1e-5)            # BF_IN_EPS as the kernel holds it
E_RSQ = 2 * U32               # ASSUMED: rsqrtf (v_rsq_f32) within 1 ulp
L_DGELU = 0.80                # >= max |gelu''| = 2 phi(0) = 0.79788...
O2 = GB.O2
MAXR, BREP = 6, 4             # norm.hip: rows a thread keeps; batches per backward slice


# ---------------------------------------------------------------------------------------------------- restated host code
def geo(bf16, wide=False):
    """(chunk, chunk lanes per row, row groups) of Geo<T, CPB, NT>: 64 channels x 256 threads, or 96 x 192 (wide)."""
    ch = 8 if bf16 else 4
    cpb, nt = (96, 192) if wide else (64, 256)
    lc = cpb // ch
    return ch, lc, nt // lc


def slice_cfg(bf16, S, C):
    """norm.hip slice_cfg(): dict(sliced, wide, rows (of a statistics slice), cached (rows of the one-workgroup register cache))."""
    cached = geo(bf16)[2] * MAXR
    wide = C % 96 == 0
    return dict(sliced=S > cached, wide=wide, rows=geo(bf16, True)[2] * MAXR if wide else cached, cached=cached)


def ws_floats(bf16, frames, S, C):
    """bf_in_ws_floats()."""
    c = slice_cfg(bf16, S, C)
    return 2 * frames * C * ((1 + -(-S // c["rows"])) if c["sliced"] else 1)


def path(bf16, S, C, ws=True):
    """Which kernels bf_in_stats / bf_in_bwd run -> dict(kind = "cached" | "uncached" | "sliced", wide, stat_rows, stat_slices,
    bwd_rows, bwd_slices); the slice figures are 0 off the sliced path."""
    c = slice_cfg(bf16, S, C)
    if not c["sliced"]:
        return dict(kind="cached", wide=False, stat_rows=0, stat_slices=0, bwd_rows=0, bwd_slices=0)
    if not ws:
        return dict(kind="uncached", wide=False, stat_rows=0, stat_slices=0, bwd_rows=0, bwd_slices=0)
    return dict(kind="sliced", wide=c["wide"], stat_rows=c["rows"], stat_slices=-(-S // c["rows"]), bwd_rows=c["rows"] * BREP,
                bwd_slices=-(-S // (c["rows"] * BREP)))


def colsum_split(nrows, C):
    """(rows per block, blocks) of bf_colsum."""
    cb = -(-C // 64)
    rpb = max(64, (nrows * cb + 1023) // 1024)
    return rpb, -(-nrows // rpb)


# ---------------------------------------------------------------------------------------------------- statistics
def _moments(x, ex=None):
    """x (..., n, C) -> exact mean, M2, the mean's error bound and the second moment's, for one workgroup's two passes.  ex: elementwise
    bound on a deviation the kernel's rows carry from x (None: they are x)."""
    n = x.shape[-2]
    m = x.mean(-2)
    M2 = ((x - m.unsqueeze(-2)) ** 2).sum(-2)
    if ex is None:
        e_m = (1 + U32) * gamma(n) * x.abs().sum(-2) / n + U32 * m.abs()
        e_q = n * e_m ** 2 + gamma(n + 3) * (M2 + n * e_m ** 2)
        return m, M2, e_m, e_q
    dm = ex.sum(-2) / n                                   # the rows' own mean moves by at most this
    d2 = (ex ** 2).sum(-2).sqrt()
    dM2 = 2 * M2.sqrt() * d2 + d2 ** 2                    # centring is an orthogonal projection: |sqrt M2' - sqrt M2| <= ||ex||
    e_r = (1 + U32) * gamma(n) * (x.abs() + ex).sum(-2) / n + U32 * (m.abs() + dm)      # the roundings, on the rows as carried
    e_q = n * e_r ** 2 + gamma(n + 3) * (M2 + dM2 + n * e_r ** 2)
    return m, M2, e_r + dm, e_q + dM2


def _merge(mi, ei, qi, eqi, ni, S):
    """Slice values mi / qi (N, F, C) with their bounds and row counts ni (N,) -> merged (m, M2, e_mu, e_M2)."""
    N = mi.shape[0]
    nn = ni.double().view(-1, 1, 1)
    m = (nn * mi).sum(0) / S
    e_mu = (1 + U32) * ((nn * ei).sum(0) + gamma(N + 1) * (nn * (mi.abs() + ei)).sum(0)) / S + U32 * m.abs()
    D = (mi - m).abs()
    M2 = (qi + nn * D ** 2).sum(0)
    e_d = (ei + e_mu) * (1 + U32) + U32 * D
    e_M2 = (eqi + nn * (2 * D * e_d + e_d ** 2)).sum(0) + gamma(N + 4) * (qi + eqi + nn * (D + e_d) ** 2).sum(0)
    return m, M2, e_mu, e_M2


def _finish_stats(m, M2, e_mu, e_M2, S, w, b, g, gb):
    w, b = w.double(), b.double()
    v = M2 / S + EPS
    e_v = O2 * (e_M2 / S + U32 * M2 / S + U32 * v)
    r = v ** -0.5
    r_hi = (v - e_v).clamp_min(EPS * (1 - 2 * U32)) ** -0.5
    r_lo = (v + e_v) ** -0.5
    e_r = torch.maximum(r_hi - r, r - r_lo) + E_RSQ * r_hi
    a = r * w
    e_a = O2 * (e_r * w.abs() + U32 * a.abs())
    s = b - m * a
    e_s = O2 * (a.abs() * e_mu + m.abs() * e_a + e_mu * e_a + U32 * (m * a).abs() + U32 * ((m * a).abs() + b.abs()))
    if g is not None:
        g = g.double()
        e_a = O2 * (e_a * g.abs() + U32 * (a * g).abs())
        a = a * g
        e_s = e_s * g.abs() + U32 * (s * g).abs()
        s = s * g
        if gb is not None:
            e_s = e_s + U32 * (s.abs() + gb.double().abs())
            s = s + gb.double()
        e_s = O2 * e_s
    return dict(mean=(m, e_mu), rstd=(r, e_r), sc=(a, e_a), sh=(s, e_s))


def in_stats(x, w, b, g=None, gb=None, slices=None, ex=None):
    """x (F, S, C) exact stored values; w / b (C,) fp32; g / gb (F, C) fp32, already expanded per frame (g[f // gdiv]); slices: rows per
    slice on the sliced path, None for one workgroup per frame; ex (F, S, C), one-workgroup form only: the rows the kernel sums are within
    ex of x (a producer's error carried in; absent: they are x) -> {"mean" | "rstd" | "sc" | "sh": (ref, bnd)}, each (F, C)."""
    x = x.double()
    S = x.shape[1]
    assert ex is None or slices is None
    if slices is None:
        m, M2, e_mu, e_M2 = _moments(x, None if ex is None else ex.double())
    else:
        parts = [_moments(x[:, s0:s0 + slices]) for s0 in range(0, S, slices)]
        ni = torch.tensor([min(slices, S - s0) for s0 in range(0, S, slices)])
        mi, qi, ei, eqi = (torch.stack([p[k] for p in parts]) for k in range(4))
        m, M2, e_mu, e_M2 = _merge(mi, ei, qi, eqi, ni, S)
    return _finish_stats(m, M2, e_mu, e_M2, S, w, b, g, gb)


def merge(part_m, part_q, rows, S, w, b, g=None, gb=None):
    """bf_in_stats_merge_slices on partials a producer wrote: part_m / part_q (F, N, C) the fp32 slice means and centred second moments
    as stored (exact inputs), slices of `rows` rows, the last one ragged."""
    N = part_m.shape[1]
    ni = torch.tensor([min(rows, S - i * rows) for i in range(N)])
    mi, qi = part_m.double().transpose(0, 1), part_q.double().transpose(0, 1)
    z = torch.zeros_like(mi)
    return _finish_stats(*_merge(mi, z, qi, z, ni, S), S, w, b, g, gb)


# ---------------------------------------------------------------------------------------------------- apply
def _store(v, e, bf16):
    return (v, (1 + U16) * e + U16 * v.abs()) if bf16 else (v, e)


def affine_apply(z, sc, sh=None, resid=None, bf16=False):
    """z / resid (F, S, C) exact; sc / sh (F, C) fp32 -> (ref, bnd)."""
    t = z.double() * sc.double()[:, None]
    if sh is not None:
        t = t + sh.double()[:, None]
    e = U32 * t.abs()
    if resid is not None:
        e = e + U32 * (t.abs() + e + resid.double().abs())
        t = t + resid.double()
    return _store(t, e, bf16)


# ---------------------------------------------------------------------------------------------------- backward
def in_bwd(dy, x, mean, rstd, w, b, g=None, add=None, gelu=False, bf16=False, nslices=0, e_dy=None):
    """dy / x / add (F, S, C) exact; mean / rstd (F, C) the given fp32 statistics; w / b (C,); g (F, C) already expanded per frame.
    nslices: backward slices on the sliced path, 0 otherwise.  e_dy (F, S, C): the gradient the kernel holds is within e_dy of dy (a fused
    producer's accumulator; absent: it is dy).
    -> {"dx": (ref, bnd) (F, S, C), "s1" | "s2": (ref, bnd) (F, C) the per-frame sums the parameter gradients are made of}."""
    dy, x = dy.double(), x.double()
    S = x.shape[1]
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    w, b = w.double(), b.double()
    xh = (x - mu) * rs
    e_xh = 2 * U32 * xh.abs() * O2
    if gelu:
        z = xh * w + b
        e_z = e_xh * w.abs() + U32 * (xh * w).abs() + U32 * ((xh * w).abs() + b.abs())
        d, e_d = GB.dgelu(z, bf16)
        e_d = e_d + L_DGELU * e_z
        dyn = dy * d
        e_dyn = dy.abs() * e_d + U32 * dyn.abs()
        if e_dy is not None:
            e_dyn = e_dyn + e_dy.double() * (d.abs() + e_d) * (1 + U32)
    else:
        dyn, e_dyn = dy, (torch.zeros_like(dy) if e_dy is None else e_dy.double())
    n = S + nslices
    s1 = dyn.sum(1)
    e_s1 = e_dyn.sum(1) + gamma(n) * (dyn.abs() + e_dyn).sum(1)
    p = dyn * xh
    e_p = e_dyn * xh.abs() + dyn.abs() * e_xh + e_dyn * e_xh
    s2 = p.sum(1)
    e_s2 = e_p.sum(1) + gamma(n + 1) * (p.abs() + e_p).sum(1)
    a1, a2 = s1[:, None], s2[:, None]
    I = dyn - a1 / S - xh * a2 / S
    Mg = dyn.abs() + a1.abs() / S + (xh * a2).abs() / S
    E = e_dyn + e_s1[:, None] / S + (e_xh * a2.abs() + xh.abs() * e_s2[:, None] + e_xh * e_s2[:, None]) / S
    E_I = E + 5 * U32 * (Mg + E)
    P = rs * w
    k = 2
    if g is not None:
        P, k = P * g.double()[:, None], 3
    v = P * I
    e = P.abs() * E_I + gamma(k) * P.abs() * (I.abs() + E_I)
    if add is not None:
        e = e + U32 * (v.abs() + add.double().abs() + e)
        v = v + add.double()
    return dict(dx=_store(v, e, bf16), s1=(s1, e_s1), s2=(s2, e_s2))


def param_grads(s1, s2, w, b, g=None, gdiv=1, prior=None, gelu=False):
    """s1 / s2: the (ref, bnd) pairs of in_bwd; g (groups, C) as the kernel indexes it (g[f // gdiv]); prior: {"dw" | "db" | "dg" | "dgb":
    fp32 contents before the call} (absent: zero) -> {"dw" | "db" (C,), "dg" | "dgb" (groups, C): (ref, bnd)}.  Behind a GELU the group
    gradients are sum dy gelu(z) and sum dy, which s1 / s2 (sums of dy gelu'(z)) do not give: bf_in_bwd refuses that combination and no
    dg / dgb is returned for it."""
    (s1, e1), (s2, e2) = s1, s2
    Fr, C = s1.shape
    w, b = w.double(), b.double()
    prior = prior or {}
    grp = torch.arange(Fr) // gdiv
    ng = int(grp.max()) + 1
    gf = torch.ones(Fr, C, dtype=torch.float64) if g is None else g.double()[grp]
    out = {}
    for name, s, e in (("dw", s2, e2), ("db", s1, e1)):
        p = prior.get(name)
        pr = torch.zeros(C, dtype=torch.float64) if p is None else p.double()
        carried = (gf.abs() * e).sum(0)
        out[name] = ((gf * s).sum(0) + pr, carried + gamma(Fr + 2) * ((gf.abs() * (s.abs() + e)).sum(0) + pr.abs()))

    def by_group(t):
        return torch.zeros(ng, C, dtype=torch.float64).index_add_(0, grp, t)

    if gelu:
        return out
    nf = min(gdiv, Fr)
    p = prior.get("dg")
    pr = torch.zeros(ng, C, dtype=torch.float64) if p is None else p.double()
    carried = by_group(w.abs() * e2 + b.abs() * e1)
    mag = by_group((w * s2).abs() + (b * s1).abs())
    out["dg"] = (by_group(w * s2 + b * s1) + pr, carried + gamma(nf + 4) * (mag + carried + pr.abs()))
    p = prior.get("dgb")
    pr = torch.zeros(ng, C, dtype=torch.float64) if p is None else p.double()
    out["dgb"] = (by_group(s1) + pr, by_group(e1) + gamma(nf + 1) * (by_group(s1.abs() + e1) + pr.abs()))
    return out


# ---------------------------------------------------------------------------------------------------- column sums
def colsum(x, scale=None, prior=None):
    """x (nrows, C) exact; scale / prior (C,) fp32 -> (ref, bnd) of shape (C,)."""
    x = x.double()
    rpb, nblk = colsum_split(x.shape[0], x.shape[1])
    sc = torch.ones(x.shape[1], dtype=torch.float64) if scale is None else scale.double()
    pr = torch.zeros(x.shape[1], dtype=torch.float64) if prior is None else prior.double()
    ref = sc * x.sum(0) + pr
    return ref, gamma(rpb + nblk + 1) * (sc.abs() * x.abs().sum(0) + pr.abs())
