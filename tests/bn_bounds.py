"""Per-element error bounds for csrc/bn.hip: BatchNorm2d batch statistics with the running update (bf_bn_fwd), the eval affine (bf_bn_eval),
GELU and GELU + 2x2 max-pool (bf_bn_act), and the BatchNorm backward with the routed pool gradient (bf_bn_bwd).

Given the exact (fp64) values a kernel reads, each function returns the fp64 reference `ref` and an elementwise bound `bnd` such that a
correct kernel satisfies |got - ref| <= bnd everywhere.  `check`, `gamma`, `rnd16`, `U32`, `U16` are conv_bounds'; `O2` (1 + 2^-10, the
second-order terms), `f32` and `L_GELU` are gemm_bounds'; `L_DGELU` is norm_bounds'.  u = 2^-24, u64 = 2^-53.  gamma_n bounds a sum of n
terms in ANY order (Higham, Accuracy and Stability of Numerical Algorithms, Thm 3.1), so the row-thread strided loads, the LDS trees over
the rows, the per-thread strided slab sums and the tree over the 256 slab lanes are covered by the term count alone; `g64(n)` is the
same with u64, for the kernels' fp64 sums.  Every constant is derived here from the kernels' rounding points; none is fitted to GPU
output.  The functions run on whatever device their arguments live on.

GELU forms.  bn.hip evaluates gelu_erff / dgelu_erff of bf_common.h (libm erff and expf) in BOTH dtypes -- not the A&S erf_fast or the
polynomial forms that gemm_bounds bounds.
  gelu_erff(t) = 0.5f * t * (1 + erff(t * c)).  conv_bounds derives its bound for the conv prologue, C_PRO u (T + |a|) with T = |x sc| +
    |sh| the magnitude of the fma's terms (meaningful where they cancel); it is taken from there.
  dgelu_erff(x) = 0.5f * (1 + erff(x * c)) + (x * c0) * expf((-0.5f * x) * x), c0 = fp32(1 / sqrt(2 pi)).  On the same lines:
    - x * c carries 2u relative (the product and the constant); erf' |z| <= 0.484, so erf moves by <= 0.97 u.  erff is within 2 ulp
      (HIP's documented bound), ulp(erf) <= 2u: 4u.  1 + erf rounds once: u |1 + erf|.  The factor 0.5 is exact and halves all of it:
      e_cdf = 0.5 (4.97 u + u |1 + erf|).
    - the exponent y = 0.5 x^2 is formed with one rounding (-0.5f * x is exact), which moves exp(-y) by y u relative.  expf itself: no
      document shipped with the toolchain states its accuracy.  ASSUMED: within 1 ulp, 2u relative (the figure HIP's math API table
      gives, as gemm_bounds assumes for __expf).  x * c0 rounds twice (the constant, the product), the product with the exponential once:
      |x pdf| (y + 5) u.  Where the exponential is subnormal (|x| > 13) it may flush: at most 2^-126 |x|.
    - the sum rounds once: u |d|.
  An argument that itself carries an error adds L_GELU (1.14 >= max |gelu'|) or L_DGELU (0.80 >= max |gelu''| = 2 phi(0)) times it.

Statistics (`stats`; bn_stats_kernel + bn_finalize_kernel).  Per channel over n = M pixels.  The partial sums are fp64 sums of the fp32
values and of their squares (exact in fp64: 48 bits):  |s1 - S1| <= g64(n) sum|x|,  |s2 - S2| <= g64(n) sum x^2.
  mu = s1 / n:  e_mu = g64(n) sum|x| / n + u64 |mu|.
  var = fmax(s2 / n - mu * mu, 0), the one-pass form in fp64: the quotient, the square (2 |mu| e_mu + u64 mu^2) and the difference each
    round on the magnitudes, not on the cancelled result:  e_var = g64(n) S2 / n + 2 |mu| e_mu + e_mu^2 + 2 u64 (S2 / n + mu^2).  The
    exact variance is >= 0, so the clamp only moves the computed value towards it.  The reference is the two-pass variance in fp64.
  mean = fp32(mu): e_m = e_mu + u |mu|.
  rstd = fp32(1 / sqrt(var + (double)eps)), eps the fp32 value of 1e-5 -- which is what the reference adds, not the literal.  v^-1/2 is
    monotone: the exact inverse root of the computed v lies in [(v + e_v)^-1/2, (v - e_v)^-1/2], and the computed v is >= eps (1 - u64)
    whatever e_v says (norm_bounds' interval form; e_v is not small beside v in a near-constant channel of large value).  sqrt and the
    division are correctly rounded in fp64 (2 u64), and the one fp32 rounding is to nearest: at most half an ulp OF ITS BINADE,
    2^(e - 25) for a value in [2^(e-1), 2^e) -- the form that is tight enough to tell eps from the literal 1e-5 (1.26e-8 relative in
    rstd, a fifth of u).
  sc = a = fl(gamma r): e_a = |gamma| e_r + u |a|.
  sh = b = beta - m * a, contracted or not: charged unfused, u |m a| + u (|m a| + |beta|), plus the carried |a| e_m + |m| e_a + e_m e_a.
    Where |mean| / std is large this is ~ u |mean| / std while sh itself may cancel to O(1): the bound follows the magnitudes.
  sc / sh are written once per frame from the same registers: the tests assert the frames bit-identical, not by bound.
  running_mean = momentum * m + (1.0f - momentum) * rm in fp32: the reference takes the fp32 value of momentum, the fp32 difference
    1.0f - momentum and rm as they are, and charges the two products and the sum unfused (u |p1| + u |p2| + u (|p1| + |p2|)) plus
    momentum e_m.  running_var likewise on (float)(var * n / (n - 1)): e = e_var n / (n - 1) + (2 u64 + u) |.|.

Eval affine (`eval_affine`; bn_eval_kernel).  The same two lines from the running statistics, which are exact inputs: r = fp32(1 /
sqrt((double)rv + (double)eps)) is half an ulp of its binade plus 3 u64; a and b as above with e_m = 0.

Activation (`act`; bn_act_kernel, bn_act_pool_kernel).  t = fmaf(x, sc, sh) with the GIVEN fp32 sc / sh, gelu_erff, the store:
(1 + u_out) C_PRO u (T + |a|) + u_out |a|, u_out = 2^-8 for bf16; an fp32 store is exact.  The pool has no bound: p must equal the maximum
of the kernel's own stored `a` over each full window and idx the window position F.max_pool2d(return_indices=True) gives on those stored
values -- ties to the first position in row-major window order, a NaN replacing the running maximum (`pool_of_stored`).

Backward (`bwd`; bn_bwd_partial_kernel, bn_bwd_param_kernel, bn_bwd_apply_kernel).  mean, rstd, sc, sh are the GIVEN fp32 values and idx
the given bytes; the reference is the closed form of the kernel header in fp64 (tests/test_bn_bounds.py proves it equals autograd at
exact statistics).
  z = fmaf(x, sc, sh): e_z = u |z|.  d = dgelu_erff(z): its evaluation bound plus L_DGELU e_z.
  gin = dA + routed dP (`route`): one rounding where both are present, exact otherwise.  g = fl(gin d): e_g = |gin| e_d + e_gin (|d| +
    e_d) + u |g|.
  xh = fl(fl(x - mean) rstd): e_xh = 2u |xh| (1 + 2^-10).
  s1 = sum g in fp64, s2 = sum (double)g * xh (the product of two fp32 values is exact in fp64): e_s1 = sum e_g + g64(n) sum (|g| + e_g),
    e_s2 = sum e_p + g64(n) sum (|p| + e_p) with e_p = e_g |xh| + |g| e_xh + e_g e_xh.
  dbeta = fp32(s1), dgamma = fp32(s2): one rounding each; accumulate = 1 adds the prior with one more, u (|prior| + |s| + e).
    accumulate = 0 overwrites: the prior (NaN in the tests) must not show.
  coef = {fp32(s1 / M), fp32(s2 / M)}: e_c = e_s / M + (u + u64) |s / M|.
  dx = fl(fl(gamma r) fl(fl(g - c0) - fl(xh c1))): three roundings inside, each charged on Mg = |g| + |c0| + |xh c1| plus the carried
    error E = e_g + e_c0 + e_xh |c1| + |xh| e_c1 + e_xh e_c1, not on the cancelled result: E_I = E + 3u (Mg + E).  Then P = gamma r and
    P I: gamma_2 |P| (|I| + E_I).  Then the store.
"""
import math

import torch
import torch.nn.functional as F

from tests.conv_bounds import C_PRO, U16, U32, check, gamma, rnd16  # noqa: F401  (re-exported to the tests)
from tests.gemm_bounds import L_GELU, O2, f32  # noqa: F401
from tests.norm_bounds import L_DGELU

U64 = 2.0 ** -53
EPS32 = f32(1e-5)             # nn.BatchNorm2d's eps as the float argument of bf_bn_fwd / bf_bn_eval holds it
E_EXP = 2 * U32               # ASSUMED: expf within 1 ulp
BN_THREADS, BN_TARGET_WGS = 256, 2048


def g64(n):
    return n * U64 / (1.0 - n * U64)


# ---------------------------------------------------------------------------------------------------- restated host code
def chan_width(C):
    w = 1
    while w < C and w < 64:
        w <<= 1
    return w


def bn_slabs(M, C):
    CW = chan_width(C)
    gx, rows = -(-C // CW), BN_THREADS // CW
    want, most = -(-BN_TARGET_WGS // gx), M // (4 * rows)
    return max(1, min(want, most))


def plan(M, C):
    """-> dict(CW, gx, rows, slabs, chunk, used, last): the launch geometry of bf_bn_fwd / bf_bn_bwd; `used` slabs of `chunk` pixels are
    launched, the last of `last` pixels."""
    CW = chan_width(C)
    slabs = bn_slabs(M, C)
    chunk = -(-M // slabs)
    used = -(-M // chunk)
    return dict(CW=CW, gx=-(-C // CW), rows=BN_THREADS // CW, slabs=slabs, chunk=chunk, used=used, last=M - (used - 1) * chunk)


def ws_floats(M, C):
    """bf_bn_ws_floats(): slabs * C * 2 doubles of slab partials, then C * 2 floats of coef."""
    return 2 * bn_slabs(M, C) * C * 2 + 2 * C


def coef_offset(M, C):
    """Float offset of coef in the workspace: behind the `used` slabs that are written, not behind all `slabs`."""
    return 2 * plan(M, C)["used"] * C * 2


# ---------------------------------------------------------------------------------------------------- rounding helpers
def half_ulp32(v):
    """Half an fp32 ulp of the binade of v: the most a round-to-nearest fp32 conversion of v moves it (normal range)."""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 25)


def _store(v, e, bf16):
    return (v, (1 + U16) * e + U16 * v.abs()) if bf16 else (v, e)


def dgelu_erff(x):
    """dgelu_erff of bf_common.h -> (exact gelu', bound on its fp32 evaluation at the exact argument x)."""
    y = 0.5 * x * x
    erf = torch.erf(x / math.sqrt(2.0))
    xp = x * torch.exp(-y) / math.sqrt(2 * math.pi)
    d = 0.5 * (1 + erf) + xp
    e_cdf = 0.5 * (4.97 * U32 + U32 * (1 + erf).abs())
    e_xp = xp.abs() * (y * U32 + E_EXP + 3 * U32) + 2.0 ** -126 * x.abs()
    return d, (e_cdf + e_xp + U32 * d.abs()) * O2


# ---------------------------------------------------------------------------------------------------- statistics
def _affine(g, b, m, e_m, r, e_r):
    a = g * r
    e_a = O2 * (g.abs() * e_r + U32 * a.abs())
    ma = (m * a).abs()
    s = b - m * a
    e_s = O2 * (a.abs() * e_m + m.abs() * e_a + e_m * e_a + U32 * ma + U32 * (ma + b.abs()))
    return (a, e_a), (s, e_s)


def _running(mom, new, e_new, old):
    """momentum * new + (1.0f - momentum) * old in fp32, `new` an fp32 value within e_new of its reference (its own rounding included)."""
    m32 = f32(mom)
    om = f32(1.0 - m32)                                   # 1.0f - momentum: one fp32 rounding of an exact fp64 difference
    p1, p2 = m32 * new, om * old
    return p1 + p2, O2 * (m32 * e_new + U32 * p1.abs() + U32 * p2.abs() + U32 * (p1.abs() + p2.abs()))


def stats(x, gamma_, beta, rm=None, rv=None, eps32=EPS32, momentum=0.1):
    """x (..., C) the exact stored values; gamma_ / beta / rm / rv (C,) fp32; eps32 / momentum the float arguments as Python floats
    -> {"mean" | "rstd" | "sc" | "sh" [| "rm" | "rv"]: (ref, bnd)}, each (C,)."""
    x = x.double().reshape(-1, x.shape[-1])
    n = x.shape[0]
    g, b = gamma_.double().to(x.device), beta.double().to(x.device)
    mu = x.mean(0)
    var = ((x - mu) ** 2).mean(0)
    S2n = (x * x).mean(0)
    e_mu = g64(n) * x.abs().mean(0) + U64 * mu.abs()
    e_var = g64(n) * S2n + 2 * mu.abs() * e_mu + e_mu ** 2 + 2 * U64 * (S2n + mu * mu)
    e_m = e_mu + U32 * mu.abs()
    v = var + eps32
    e_v = e_var + U64 * v
    r = v ** -0.5
    r_hi = (v - e_v).clamp_min(eps32 * (1 - U64)) ** -0.5
    r_lo = (v + e_v) ** -0.5
    e_r = torch.maximum(r_hi - r, r - r_lo) + half_ulp32(r_hi) + 4 * U64 * r_hi
    sc, sh = _affine(g, b, mu, e_m, r, e_r)
    out = dict(mean=(mu, e_m), rstd=(r, e_r), sc=sc, sh=sh)
    if rm is not None:
        out["rm"] = _running(momentum, mu, e_m, rm.double().to(x.device))
        unb = var * n / (n - 1.0)
        e_unb = e_var * n / (n - 1.0) + (2 * U64 + U32) * unb + O2 * U32 * e_var
        out["rv"] = _running(momentum, unb, e_unb, rv.double().to(x.device))
    return out


def eval_affine(gamma_, beta, rm, rv, eps32=EPS32):
    """-> {"sc" | "sh": (ref, bnd)}, each (C,), from the running statistics (exact fp32 inputs)."""
    g, b, m, v = gamma_.double(), beta.double(), rm.double(), rv.double() + eps32
    r = v ** -0.5
    e_r = half_ulp32(r) + 4 * U64 * r
    sc, sh = _affine(g, b, m, torch.zeros_like(m), r, e_r)
    return dict(sc=sc, sh=sh)


# ---------------------------------------------------------------------------------------------------- activation and pool
def act(x, sc, sh, bf16=False):
    """x (..., C) exact; sc / sh (C,) the given fp32 values -> (ref, bnd) of a = gelu(x sc + sh) as stored."""
    x = x.double()
    s, h = sc.double().to(x.device), sh.double().to(x.device)
    t, T = x * s + h, (x * s).abs() + h.abs()
    a = F.gelu(t)
    return _store(a, C_PRO * U32 * (T + a.abs()), bf16)


def window_pos(iw, W):
    """F.max_pool2d's flat H * W indices -> the kernel's window position byte (dy << 1 | dx)."""
    return (((iw // W) & 1) << 1) | ((iw % W) & 1)


def pool_of_stored(a):
    """a (B, H, W, C) the kernel's own stored activations -> (p, idx) (B, H/2, W/2, C) as F.max_pool2d(2, 2) gives them: exact."""
    W = a.shape[2]
    pw, iw = F.max_pool2d(a.double().permute(0, 3, 1, 2), 2, 2, return_indices=True)
    return pw.permute(0, 2, 3, 1), window_pos(iw, W).permute(0, 2, 3, 1).to(torch.uint8)


# ---------------------------------------------------------------------------------------------------- backward
def route(dP, idx, H, W):
    """dP / idx (B, H/2, W/2, C) -> (the pooled gradient at the pixel each index byte names, zero elsewhere and on the partial windows of
    an odd frame (B, H, W, C); the mask of the pixels that received one)."""
    B, Hp, Wp, C = dP.shape
    out = torch.zeros(B, H, W, C, dtype=torch.float64, device=dP.device)
    hit = torch.zeros(B, H, W, C, dtype=torch.bool, device=dP.device)
    for j in range(4):
        sel = idx.to(dP.device) == j
        out[:, j >> 1:2 * Hp:2, j & 1:2 * Wp:2] = torch.where(sel, dP.double(), torch.zeros_like(out[:, :1, :1, :1]))
        hit[:, j >> 1:2 * Hp:2, j & 1:2 * Wp:2] = sel
    return out, hit


def bwd(dA, dP, idx, x, gamma_, mean, rstd, sc, sh, prior_dgamma=None, prior_dbeta=None, bf16=False):
    """dA (B, H, W, C) the exact fp32 gradient or None; dP / idx (B, H/2, W/2, C) or None; x (B, H, W, C) exact; gamma_ / mean / rstd / sc /
    sh (C,) the given values; priors (C,): the contents an accumulate = 1 call adds to (None: accumulate = 0)
    -> {"dx": (ref, bnd) (B, H, W, C), "dgamma" | "dbeta": (ref, bnd) (C,)}."""
    x = x.double()
    dev = x.device
    B, H, W, C = x.shape
    n = B * H * W
    g_, mu, rs, s, h = (t.double().to(dev) for t in (gamma_, mean, rstd, sc, sh))
    z = x * s + h
    d, e_d = dgelu_erff(z)
    e_d = e_d + L_DGELU * U32 * z.abs()
    gin = torch.zeros_like(x) if dA is None else dA.double().to(dev)
    e_gin = torch.zeros_like(x)
    if dP is not None:
        r_, hit = route(dP.to(dev), idx, H, W)
        gin = gin + r_
        if dA is not None:
            e_gin = U32 * gin.abs() * hit
    g = gin * d
    e_g = O2 * (gin.abs() * e_d + e_gin * (d.abs() + e_d) + U32 * g.abs())
    xh = (x - mu) * rs
    e_xh = 2 * U32 * xh.abs() * O2
    red = (0, 1, 2)
    s1 = g.sum(red)
    e_s1 = e_g.sum(red) + g64(n) * (g.abs() + e_g).sum(red)
    p = g * xh
    e_p = e_g * xh.abs() + g.abs() * e_xh + e_g * e_xh
    s2 = p.sum(red)
    e_s2 = e_p.sum(red) + g64(n) * (p.abs() + e_p).sum(red)
    out = {}
    for name, sv, ev, prior in (("dbeta", s1, e_s1, prior_dbeta), ("dgamma", s2, e_s2, prior_dgamma)):
        e = ev + U32 * sv.abs()
        if prior is not None:
            pr = prior.double().to(dev)
            e = e + U32 * (pr.abs() + sv.abs() + e)
            sv = sv + pr
        out[name] = (sv, e)
    c0, c1 = s1 / n, s2 / n
    e_c0, e_c1 = e_s1 / n + (U32 + U64) * c0.abs(), e_s2 / n + (U32 + U64) * c1.abs()
    I = g - c0 - xh * c1
    Mg = g.abs() + c0.abs() + (xh * c1).abs()
    E = e_g + e_c0 + e_xh * c1.abs() + xh.abs() * e_c1 + e_xh * e_c1
    E_I = E + 3 * U32 * (Mg + E)
    P = g_ * rs
    v = P * I
    out["dx"] = _store(v, P.abs() * E_I + gamma(2) * P.abs() * (I.abs() + E_I), bf16)
    return out


# ---------------------------------------------------------------------------------------------------- the inputs of the value cases
def randn(*shape, scale=1.0, shift=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift


def stored(t, bf16):
    return t.to(torch.bfloat16 if bf16 else torch.float32).double()


OFFA, PADA = 5, 7                         # the dA slice of the offA cases: channels [5, 5 + C) of rows of C + 7 floats


def params(C, seed=0, gscale=1.0):
    """gamma, beta (C,) fp32."""
    return (randn(C, scale=0.4, shift=1.0, seed=seed + 100) * gscale).float(), randn(C, scale=0.5, seed=seed + 101).float()


def given_stats(x, gamma_, beta, eps32=EPS32):
    """fp32 mean / rstd / sc / sh (C,) of x (..., C) as a forward would hand them to bf_bn_bwd (rounded from fp64; exact inputs there)."""
    x = x.double().reshape(-1, x.shape[-1])
    mean = x.mean(0).float()
    rstd = ((x.var(0, unbiased=False) + eps32) ** -0.5).float()
    sc = gamma_ * rstd
    return mean, rstd, sc, beta - mean * sc


def grads(B, H, W, C, bf16, seed=0):
    """dA (B, H, W, C) fp32 and dP (B, H/2, W/2, C) in the stored type, as fp64."""
    return randn(B, H, W, C, seed=seed + 200).float().double(), stored(randn(B, H // 2, W // 2, C, seed=seed + 201), bf16)


def wide(dA):
    """dA as channels [OFFA, OFFA + C) of a NaN-filled fp32 buffer with rows of C + PADA floats."""
    w = torch.full((*dA.shape[:-1], dA.shape[-1] + PADA), float("nan"), dtype=torch.float32)
    w[..., OFFA:OFFA + dA.shape[-1]] = dA.float()
    return w


def priors(C, seed=0):
    """Nonzero (dgamma, dbeta) contents for an accumulate = 1 call."""
    return randn(C, seed=seed + 400).float(), randn(C, seed=seed + 401).float()


def edge_input(shape, bf16):
    """The operands of the edge-shape cases -> (x, gamma, beta, dA, dP), seeded by the channel count."""
    B, H, W, C = shape
    x = stored(randn(B, H, W, C, scale=1.5, shift=0.3, seed=C), bf16)
    return (x, *params(C, C), *grads(B, H, W, C, bf16, C))


NEAR_CONST = (2, 5, 7, 11, 13, 17)       # channels of the "constant" case whose variance is far below eps (channel 3 is exactly constant)


def value_input(kind, B, H, W, C, bf16, seed=0):
    """The activations of the value cases, shared by the GPU test and the CPU test that rejects the mutants on them, rounded to the
    stored type.  C >= 20.
      plain        N(0.3, 1.5^2)
      large_mean   |mean| / std = 1000 in fp32; bf16 has 8 bits, so the largest ratio it stores distinctly is ~33 (100 +- 3: spacing 0.5)
      constant     channel 3 constant (variance exactly 0, rstd = eps32^-1/2); the NEAR_CONST channels two-valued, 2^-6 and 2^-6 +
                   k 2^-12: var from eps / 670 to eps / 19, where the fp32 value of eps and the literal 1e-5 differ in rstd
      scales       channels six decades apart inside one channel block
      ties         constant 2x2 windows: every maximum is a tie
    """
    if kind == "plain":
        x = randn(B, H, W, C, scale=1.5, shift=0.3, seed=seed)
    elif kind == "large_mean":
        x = randn(B, H, W, C, scale=3.0, shift=100.0, seed=seed) if bf16 else randn(B, H, W, C, scale=1.0, shift=1000.0, seed=seed)
    elif kind == "constant":
        x = randn(B, H, W, C, scale=1.5, shift=0.3, seed=seed)
        x[..., 3] = 0.03125
        odd = (torch.arange(B * H * W).reshape(B, H, W) % 2).double()
        for k, c in enumerate(NEAR_CONST):
            x[..., c] = 2.0 ** -6 + odd * (k + 1) * 2.0 ** -12        # both values are bf16 numbers; var = ((k + 1) 2^-13)^2 (1 - 1/n^2)
    elif kind == "scales":
        perm = torch.randperm(C, generator=torch.Generator().manual_seed(seed + 1))
        x = randn(B, H, W, C, seed=seed) * (10.0 ** torch.linspace(-3, 3, C, dtype=torch.float64)[perm])
    elif kind == "ties":
        x = randn(B, (H + 1) // 2, (W + 1) // 2, C, scale=1.5, shift=0.3, seed=seed).repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W]
    else:
        raise ValueError(kind)
    return stored(x.contiguous(), bf16)
