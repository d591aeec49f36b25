"""Per-element error bounds for the trunk GEMM family: csrc/gemm.hip (tile kernel), gemm_stream.hip, gemm_tokred.hip, the plain
frame-pair path of gemm_frame.hip and the shared epilogue of gemm_common.h.

Given the exact (fp64) values a kernel reads -- its stored operands as dense [outer][k] matrices, the fp32 prologue tables expanded to
the same shape, the fp32 epilogue vectors, `aux`, the prior contents of an accumulated output -- the functions below return the fp64
reference `ref` and an elementwise bound `bnd` such that a correct kernel satisfies |got - ref| <= bnd everywhere.  `check` and `rel_l2`
are conv_bounds'.  u = 2^-24 is the fp32 unit roundoff; every constant below is derived here and none is fitted to GPU output.

Operand (`operand()`; gemm.hip StagerFixed::commit).  Without a prologue the stored value is the operand: exact.  With one the kernel
computes t = v * sc + sh in fp32 and does not force an fma: two roundings, |dt| <= u |v sc| + u |t| <= 2 u T with T = |v sc| + |sh|
(sh == NULL: one rounding, u |t|; BF_PRO_GELU: t = v, exact).  BF_PRO_AFFINE_GELU / BF_PRO_GELU then apply gelu_t<T> (below); in bf16
mode the result is rounded to bf16 (RNE) and so is the reference's: rounding is monotone, so the kernel's operand lies in
[rnd(a - eps), rnd(a + eps)] and the operand error is the larger distance from rnd(a) to either end (conv_bounds.operand's
construction).  The prologue applies to valid elements only: padded rows and the zero-filled K tail are exact zeros and contribute
nothing, so the caller passes the valid [outer][K] matrix alone.

GELU forms.  bf16 kernels evaluate the polynomials phi_fast / dgelu_fast of bf_common.h: `phi_poly` / `dgelu_poly` restate them in
fp64 (coefficients and the clamp at |x| = 4 copied; tests/test_gemm_bounds.py pins them against the exact functions), so the bound
covers only the fp32 evaluation.  That is not a fixed number of ulps (gelu' cancels near |x| = 4: 0.5 + x r(x^2) with x r ~ -0.5), so
it is bounded per element by the running Horner error of Higham, Accuracy and Stability of Numerical Algorithms, Alg. 5.1 (two
roundings per step; a contracted fma rounds once and is covered), plus the rounding of the argument x^2 carried through |r'|, plus one
rounding each for x * r, 0.5 + ., and gelu's x * Phi.  fp32 kernels evaluate erf_fast (Abramowitz & Stegun 7.1.26) inside gelu_f /
dgelu_f; the reference is the exact erf and the bound takes the formula's error E_AS = 1.5e-7 (A&S; measured 1.39e-7 on [-8, 8]) plus
its evaluation: the same running Horner error for the quintic in t, t = rcp(1 + p|x c|) carrying 6u relative (the argument's 2u, product, sum, and
the reciprocal's 2u), and exp carrying (3y + 2)u relative at argument -y (two roundings forming y, the log2 e scaling inside __expf, the
exponential itself).  No ROCm document shipped with the toolchain states the accuracy of __expf and __builtin_amdgcn_rcpf; ASSUMED: both
(v_exp_f32, v_rcp_f32) are within 1 ulp = 2u relative, the figure of AMD's CDNA instruction-set guides.  An input that itself carries
an error et (the prologue's t, the epilogue's v) adds L_GELU * et, L_GELU = 1.14 >= max |gelu'| (1.1289 exact; the polynomial form's
own derivative is pinned below 1.14 in the CPU test).

Sum.  n products accumulated in fp32 in any order are within gamma_n sum |a||b| of the exact dot product, gamma_n = n u / (1 - n u)
(Higham Thm 3.1); bf16 products are exact in fp32.  n is K plus one per K-slice / slab (split-K atomics in any order, the tokred slab
sums in slice order) plus one for the prior value of an accumulating output.  The column sums (bf_gemm's colsum, tokred's) are the same
form with b = 1.  Operand errors enter as ea |b| + |a| eb + ea eb.

Epilogue (`epilogue()`).  The tile kernel (gemm_common.h epilogue_rows) rounds four times: v1 = fmaf(acc + bias, cs, ch) (the add, then
the fma), v2 = v1 * rs, v3 = v2 + aux or v2 * gelu'(aux), then the store.  The streaming and pair kernels (epi_lin / epi_lin_add) fuse
the last product and sum into one fma, which rounds once where the tile kernel rounds twice.  One bound covers both: each rounding is
charged u times the sum of magnitudes of the value it rounds (u (|S| + |bias|), u (|v0 cs| + |ch|), u |v2|, u (|v2| + |aux|)), a fused
step is charged as if unfused, and a step that multiplies by an absent 1 or adds an absent 0 is exact and not charged.  The error of
each stage is carried forward multiplied by |cs|, |rs|, |gelu'|.  Terms of order u^2 (a rounding applied to a value that already
carries an error) are covered by the factor 1 + 2^-10: every carried error here is below 2^-10 of the magnitudes it is charged on.
gelu_out is gelu_t<T> of the fp32 v3 before its store rounding: bounded from v3 and its error as above, then rounded to the output type.

Store.  |rnd(v) - ref| <= (1 + u_out) |v - ref| + u_out |ref|; u_out = 2^-24 for fp32 stores, BF_OUT_STORE_F32 and the fp32 atomics,
2^-8 for bf16 stores (conv_bounds' figures).
"""
import math

import torch

from tests.conv_bounds import U16, U32, check, gamma, rel_l2, rnd16  # noqa: F401  (re-exported to the tests)

PRO_NONE, PRO_AFFINE, PRO_AFFINE_GELU, PRO_GELU = 0, 1, 2, 3      # L.BF_PRO_*
AUX_NONE, AUX_ADD, AUX_DGELU = 0, 1, 2                            # L.BF_AUX_*
L_GELU = 1.14
E_AS = 1.5e-7
O2 = 1.0 + 2.0 ** -10

# bf_common.h phi_fast / dgelu_fast: coefficients of r(u), u = x^2, highest power first
PHI_C = (-1.520480094e-09, 1.180964698e-07, -4.014221545e-06, 7.960997465e-05, -1.041295800e-03, 9.641715296e-03, -6.614117438e-02,
         3.988329119e-01)
DGELU_C = (9.387459194e-10, -7.941240515e-08, 2.950722870e-06, -6.380590451e-05, 8.975979855e-04, -8.669717964e-03, 5.833777581e-02,
           -2.646917422e-01, 7.975648121e-01)
# bf_common.h erf_fast: poly(t) = t * q(t), q's coefficients highest power first; P_AS the A&S p
AS_C = (1.061405429, -1.453152027, 1.421413741, -0.284496736, 0.254829592)
P_AS = 0.3275911


def f32(c):
    """The fp32 value of a literal, as the kernel's `...f` constants hold it."""
    return float(torch.tensor(c, dtype=torch.float32))


def horner(coef, x):
    """-> (p(x), mu, |p'(x)|): the polynomial with the fp32 values of `coef` in fp64, the running bound on the error of its fp32 Horner
    evaluation (Higham Alg. 5.1), and the magnitude of its derivative."""
    y = torch.full_like(x, f32(coef[0]))
    d = torch.zeros_like(x)
    mu = y.abs() / 2
    for c in coef[1:]:
        d = d * x + y
        y = y * x + f32(c)
        mu = mu * x.abs() + y.abs()
    return y, U32 * (2 * mu - y.abs()), d.abs()


def _odd_poly(coef, x):
    """0.5 + xc * r(xc^2), xc = clamp(x, -4, 4) -> (value, bound on its fp32 evaluation error)."""
    xc = x.clamp(-4.0, 4.0)
    u = xc * xc
    r, mu, dr = horner(coef, u)
    er = mu + dr * u * U32 * O2                       # Horner roundings + the rounding of u = xc * xc
    val = 0.5 + xc * r
    return val, xc.abs() * er + U32 * (xc * r).abs() + U32 * val.abs()


def phi_poly(x):
    return _odd_poly(PHI_C, x)


def dgelu_poly(x):
    return _odd_poly(DGELU_C, x)


def gelu_poly(x):
    p, ep = phi_poly(x)
    return x * p, x.abs() * ep + U32 * (x * p).abs()


def _erf_eval_err(ax, y):
    """Bound on |computed - formula| of 1 - poly(t) exp(-y), t = 1 / (1 + p ax), in fp32 (ax >= 0 exact, y = the exponent's magnitude)."""
    t = 1.0 / (1.0 + f32(P_AS) * ax)
    q, mu, dq = horner(AS_C, t)
    poly = t * q
    e_poly = t * (mu + dq * t * 6 * U32) + 6 * U32 * poly.abs() + U32 * poly.abs()      # q's Horner + t's 6u through q' ; t's 6u ; t * q
    e = torch.exp(-y)
    e_exp = (3 * y + 2) * U32 * e
    return (e_poly * e + poly.abs() * e_exp + U32 * poly.abs() * e + U32) * O2          # product; 1 - . (|r| <= 1)


def gelu_erf(x):
    """gelu_f of bf_common.h -> (exact gelu, bound): 0.5 x (1 + erf_fast(x c)), c = fp32(1 / sqrt 2)."""
    z = x / math.sqrt(2.0)
    erf = torch.erf(z)
    g = 0.5 * x * (1 + erf)
    # x * c: 2u relative on the argument (the product and the constant) moves erf by <= 0.97 u (conv_bounds); y = z^2 as computed
    e_erf = E_AS + _erf_eval_err(z.abs(), z * z) + 0.97 * U32
    return g, (0.5 * x.abs() * (e_erf + U32 * (1 + erf).abs()) + 2 * U32 * g.abs()) * O2


def dgelu_erf(x):
    """dgelu_f of bf_common.h -> (exact gelu', bound): cdf + x * (c0 * e), e = exp(-x^2 / 2)."""
    z = x / math.sqrt(2.0)
    y = 0.5 * x * x
    e = torch.exp(-y)
    cdf = 0.5 * (1 + torch.erf(z))
    pdf = e / math.sqrt(2 * math.pi)
    d = cdf + x * pdf
    e_cdf = 0.5 * (E_AS + _erf_eval_err(z.abs(), y) + 0.97 * U32 + U32 * 2) + U32 * cdf
    e_xp = (x * pdf).abs() * ((3 * y + 2) * U32 + 3 * U32)                                                  # exp; the constant, c0 * e, x * .
    return d, (e_cdf + e_xp + U32 * d.abs()) * O2


def gelu(t, et, bf16):
    """gelu_t<T> of a value t known to within et -> (value, bound)."""
    g, eg = gelu_poly(t) if bf16 else gelu_erf(t)
    return g, eg + L_GELU * et


def dgelu(x, bf16):
    return dgelu_poly(x) if bf16 else dgelu_erf(x)


def operand(v, pro=PRO_NONE, sc=None, sh=None, bf16=False):
    """v: the stored values as the dense [outer][K] operand (fp64); sc / sh: the fp32 tables expanded to v's shape (sh None: pure
    scale) -> (a, ea): the operand the MFMAs consume as the reference rounds it, and the bound on the kernel's deviation from it."""
    v = v.double()
    if pro == PRO_NONE:
        return v, torch.zeros_like(v)
    if pro == PRO_GELU:
        t, et = v, torch.zeros_like(v)
    elif sh is None:
        t = v * sc.double()
        et = U32 * t.abs()
    else:
        s, h = sc.double(), sh.double()
        t, et = v * s + h, 2 * U32 * ((v * s).abs() + h.abs())
    a, ea = (t, et) if pro == PRO_AFFINE else gelu(t, et, bf16)
    if not bf16:
        return a, ea
    r = rnd16(a)
    return r, torch.maximum(rnd16(a + ea) - r, r - rnd16(a - ea))


def product(a, ea, b, eb, n):
    """a (M, K), b (N, K) with their operand errors, n the length of the kernel's sum -> (S, bound on the fp32 accumulator)."""
    S = a @ b.t()
    mag = a.abs() @ b.abs().t()
    err = ea @ b.abs().t() + a.abs() @ eb.t() + ea @ eb.t()
    return S, err + gamma(n) * mag


def epilogue(S, eS, bf16, bias=None, cs=None, ch=None, rs=None, aux=None, aux_mode=AUX_NONE, out_f32=False, want_gelu=False):
    """S / eS from product(); bias / cs / ch (N,) and rs (M,) the fp32 vectors (already expanded per row), aux (M, N) exact.
    -> (ref, bnd) or, with want_gelu, (ref, bnd, gelu_ref, gelu_bnd)."""
    v, e = S, eS
    if bias is not None:
        b = bias.double()[None, :]
        e = e + U32 * (v.abs() + b.abs())
        v = v + b
    if cs is not None:
        c, h = cs.double()[None, :], ch.double()[None, :]
        e = e * c.abs() + U32 * ((v * c).abs() + h.abs())
        v = v * c + h
    if rs is not None:
        r = rs.double()[:, None]
        v, e = v * r, e * r.abs()
        e = e + U32 * v.abs()
    if aux_mode == AUX_ADD:
        e = e + U32 * (v.abs() + aux.abs())
        v = v + aux
    elif aux_mode == AUX_DGELU:
        d, ed = dgelu(aux, bf16)
        e = e * d.abs() + (v.abs() + e) * ed
        v = v * d
        e = e + U32 * v.abs()
    e = e * O2
    uo = U16 if (bf16 and not out_f32) else U32
    bnd = (1 + uo) * e + uo * v.abs()
    if not want_gelu:
        return v, bnd
    g, eg = gelu(v, e, bf16)
    return v, bnd, g, (1 + uo) * eg + uo * g.abs()


def accumulate(S, eS, n, prior=None):
    """fp32 atomics / slab sums into an fp32 output holding `prior` (None: zero or overwritten).  eS from product() with the same n (the
    slices and the prior counted in it); the prior is one more term of that sum, so its magnitude joins sum |.|: every partial total the
    slices are added to contains it."""
    if prior is not None:
        S = S + prior.double()
        eS = eS + gamma(n) * prior.double().abs()
    return S, (1 + U32) * eS + U32 * S.abs()


def colsum(x, n, prior=None):
    """Column sums of the dense operand x (tokens, C) with the kernel's sum length n -> (ref, bnd) of shape (C,)."""
    x = x.double()
    s, mag = x.sum(0), x.abs().sum(0)
    if prior is not None:
        s, mag = s + prior.double(), mag + prior.double().abs()
    return s, (1 + U32) * gamma(n) * mag + U32 * s.abs()


def splits(K, splitk, bk):
    """K-slices that gemm.hip's launch() settles on."""
    kt = -(-K // bk)
    s = max(1, min(splitk, kt))
    kper = -(-kt // s) * bk
    return -(-K // kper)


def tokred_split(Nout, Kin, M):
    """(tokens per slice, slices, ping-pong form?) of bf_gemm_tokred: tokred_impl() in gemm_tokred.hip at its default knobs."""
    pp = Nout % 192 == 0 and Kin % 192 == 0 and M % 32 == 0 and M >= 128
    if pp:
        halves = M // 32
        ns = max(1, min(max(1, 128 // ((Nout // 192) * (Kin // 192))), 16, halves // 4))
        per = -(-halves // ns)
        return per * 32, -(-halves // per), True
    steps = M // 64
    ns = max(1, min(8, 16, steps))
    per = -(-steps // ns)
    return per * 64, -(-steps // per), False


def patches(img, gh, gw):
    """k2s2 patch rows of a channels-last image (F, 2 gh, 2 gw, C) -> (F gh gw, 4 C), columns ordered (ky, kx, c) as the gather reads them."""
    Fr, C = img.shape[0], img.shape[3]
    return img.reshape(Fr, gh, 2, gw, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(Fr * gh * gw, 4 * C)
