"""Per-element error bounds for the patch-stage streaming kernels: csrc/gather_gemm.hip (gather_gemm_kernel plain / GELU / rebuilt,
scatter_gemm_kernel with its slice partials, gather_wgrad_kernel + gather_wgrad_reduce_kernel), csrc/embed_tail.hip and the last-stage
family of csrc/patch.hip (debed_last_kernel, debed_last_bwd_kernel = bf_embed_first's, debed_last_inbwd_kernel + dl_slice_sum_kernel).

Given the exact (fp64) values a kernel reads, each function returns the fp64 reference `ref` and an elementwise bound `bnd` such that a
correct kernel satisfies |got - ref| <= bnd everywhere.  `check`, `gamma`, `rnd16`, `U32`, `U16` are conv_bounds'; the GELU polynomials,
their running Horner bounds, `L_GELU`, `product` and `patches` are gemm_bounds'; `merge`, `param_grads` and `L_DGELU` are norm_bounds'.
u = 2^-24.  gamma_n = n u / (1 - n u) bounds a sum of n terms in ANY order (Higham, Accuracy and Stability of Numerical Algorithms,
Thm 3.1), so MFMA order, lane permutes, shuffle trees, slab and frame sums are covered by the term count alone.  Every constant is
derived here from the kernel source and none is fitted to GPU output.  ASSUMED, as in gemm_bounds: nothing beyond IEEE fp32 arithmetic
-- these kernels call no transcendental instruction (the bf16 GELU forms are polynomials); the one division (a / n of the last-stage
slice mean) is charged one rounding, u, which holds for a correctly rounded quotient and for v_rcp_f32 (1 ulp, the figure gemm_bounds
assumes) followed by a product only with 3u: 3u is charged.

Operand (`affine_gelu`, `round16`).  gather / scatter / wgrad kernels form bf16(gelu_fast(fmaf(v, sc, sh))): t = v sc + sh rounds once,
|dt| <= u |t|; gelu_fast is gemm_bounds.gelu_poly (the polynomial restated in fp64, so only its fp32 evaluation is bounded: the running
Horner bound) and an argument known to within et moves it by L_GELU et.  debed_last_kernel writes v * sc + sh without fmaf: two
roundings, u |v sc| + u |t| <= 2u (|v sc| + |sh|), which also covers a contracted fma.  The result is rounded to bf16 and so is the
reference: rounding is monotone, so the kernel's operand lies in [rnd(a - e), rnd(a + e)] and the operand error is the larger distance
from rnd(a) to either end (conv_bounds.operand's construction) -- one bf16 ulp where a rounding boundary lies within e of a, zero
elsewhere; no fixed allowance for flipped roundings.

Rebuilt map (`rebuilt`; REB / FREB, embed_tail's !YMAP).  y = bf16(sum_{k<16} patch[k] w0[c][k]) from one 16x16x16 MFMA in fp32:
products of bf16 are exact, the 16-term sum is within gamma_16 sum |patch||w0|, then the interval rounding above.  The rounded y (with
its interval error ey) enters the affine: et = u |t| + |sc| ey (1 + u), and the second interval rounding follows -- two nested intervals.

Sums.  gamma_n on sum |a||b| with n the length of the kernel's sum: gather 4 * 96 = 384, scatter 96, debed_last Ci, the K = 16 products
(dact, y0, the rebuilt rows) 16.  wgrad: a workgroup accumulates 32 rows per step over `steps` steps, gather_wgrad_reduce_kernel adds
the slabs (each lane every fourth, then three adds): n = 32 steps + slabs.  Operand errors enter as ea |b| + |a| eb + ea eb
(gemm_bounds.product).

Stores.  bf16 (`store16`: (1 + u16) e + u16 |ref|, u16 = 2^-8) for out, the fine map, dact, dx, y0; pred, dwprep, the wgrad output and
the parameter gradients are the fp32 values themselves: no store rounding.  Accumulated outputs carry their prior as one more term.

dpm / patches (`dpm`).  A given gradient or clip is bf16(v): bit-equal, bound 0.  Fused loss: cf = fl(coef gscale) (u |cf|; gscale
absent: exact), d = fl(pred - y) (u |d|), then cf * d rounded once, or BOTH: fmaf(cf, d, dpred) rounded once:
e = |d| e_cf + |cf| e_d + e_cf e_d + u (|cf d| + |dpred|) (the last rounding charged on the magnitudes, not on a cancelled sum), then the
interval rounding.  dact / dx / y0 are judged with the kernel's own stored dpm / patches as the exact operand.

Slice partials (`slice_partials`; scatter_gemm_kernel's 128-pixel tiles, debed_last_bwd_kernel's slices of up to 256 rows).  Of the
values as stored (exact bf16; v * v is exact in fp32): t1 = sum v within gamma_n sum |v|, t2 = sum v^2 within gamma_n sum v^2,
mu = t1 / 128 (a power of two: exact) or a / n (3u, above), then t2 - t1 mu, clamped at 0.  The reference M2 = sum v^2 - (sum v)^2 / n
is >= 0, so the clamp only moves a value towards it.  The product and the difference round once each (an fma once): charged on the
magnitudes, e_q = e_t2 + |t1| e_mu + |mu| e_t1 + e_t1 e_mu + u |t1 mu| + u (t2 + |t1 mu|) -- where |mean| >> std this is ~ 2 n u mean^2
while M2 itself may be tiny: the bound follows the magnitudes.  The merged statistics are norm_bounds.merge on the stored partials.

Loss limbs (`loss_limbs`; debed_last_kernel, loss_accum).  Per (frame, channel): num = sum (pred - y)^2 over the kernel's own fp32 pred,
den = sum y^2.  A lane forms d = fl(pred - y), d * d, adds four such terms and adds that to its running sum over its wave's 16 groups,
then four shuffle levels: a term passes 2 + 1 roundings as a square and at most 4 * 16 + 4 = 68 additions; all terms are >= 0, so a
wave's partial is within gamma_71 of its exact sum (den: gamma_69).  The partial is cut into base-2^48 digits exactly, the last one
rounded to the grid of 2^(128 - 48 BF_LOSS_LIMBS) = 2^-112 (patch.hip: "units of 2^-112"): half a unit per wave partial, ceil(groups /
16) partials per frame; integer adds are exact.

bf_debed_last_bwd_norm (`debed_last_bwd_norm`; debed_last_inbwd_kernel).  The structure of norm_bounds.in_bwd with this kernel's
rounding points, which differ from norm.hip's: a = fl(rstd w) (u), sh' = fmaf(-mean, a, b) (|mean| e_a + u |sh'|), z = fmaf(y, a, sh')
(|y| e_a + e_sh + u |z|); xh = fmaf(y, rstd, fl(-mean rstd)): u |mean rstd| + u |xh| -- not 2u |xh|: where |mean| >> std the rounding of
mean rstd dominates.  dact = sum_16 dpm wc (gamma_16), dd = fl(dact gelu'(z)): dgelu_poly's evaluation bound + L_DGELU e_z, the product's
u.  s1 = sum dd, s2 = sum fma(dd, xh, .) over S rows and ceil(S / 256) slices (dl_slice_sum_kernel): gamma_{S + slices} and
gamma_{S + slices + 1} with the carried operand errors, as in_bwd.  Pass 2: t_i = fl(s_i fl(1 / S)) (2u), I = dd - t1 - xh t2 in three
roundings (two with an fma), each charged on Mg = |dd| + |t1| + |xh t2| plus the carried error E; dx = a I: gamma_2 |a| (|I| + E_I) +
|a| E_I, then the bf16 store.  d_in_w / d_in_b: norm_bounds.param_grads on (s1, s2) (the same InReduceJob).

bf_embed_tail_bwd (`embed_tail`; the header of embed_tail.hip).  y is the given y0 or the rebuilt rows.  dact = sum_{C1} dy1 W1
(gamma_C1); z = fmaf(y, sc, sh) with the GIVEN sc / sh (u |z|, + |sc| ey rebuilt); xh = fmaf(y, rstd, fl(-mean rstd)) as above;
dd = fl(dact gelu'(z)).  s1 = sum dd, s2 = sum fma(dd, xh, .); dd is rounded to bf16 (interval rounding) as the A operand of
G = sum dd16 patch_k; M2 = sum patch_j patch_k and P1 = sum patch_k have exact terms.  Each of these sums runs over 32 tpw rows per wave
(8 tpw per lane and two swap levels for s1 / s2: fewer), two adds across the four waves, and embed_tail_frame_kernel's 4 cpf workgroup
partials: n = 32 tpw + 4 + 4 cpf (one per workgroup partial).  Frame kernel: px = rstd (sum_j w0 M2 - mean P1): gamma_16 on the
16-term fma chain plus the carried e_M2, mean P1 and the difference one rounding each, charged on |W0 M2| + |mean P1| (they cancel: PX is
a centred sum); the factor rstd once more.  slab = (rstd w) (G - t1 P1 - t2 px), t_i = fl(s_i fl(1 / S0)) (2u): the cancellation in
G - t1 P1 - t2 PX is charged on the magnitudes of the three terms, Mg = |G| + |t1 P1| + |t2 PX|, four roundings (two products, two
differences) each u (Mg + E), not on the result; then gamma_2 for rstd w and the last product.  embed_tail_sum_kernel adds the frames in
order: gamma_F on sum_f (|slab| + e) (one per frame); d_in_w / d_in_b: gamma_{F+1} with the prior as one more term.

Dispatch arithmetic restated for the GPU cases: `wave_split` / `wave_runs` (gather / scatter launchers), `wgrad_runs`,
`wgrad_ws_floats`, `tail_plan`, `tail_ws_floats`, `dl_split` (groups per wave / workgroup of the last-stage kernels).
"""
import torch

from tests.conv_bounds import U16, U32, check, gamma, rel_l2, rnd16  # noqa: F401  (re-exported to the tests)
from tests import gemm_bounds as GB
from tests import norm_bounds as NB

O2 = GB.O2
GW = 4                        # gather_gemm.hip: waves per workgroup
SLAB = 4 * 96 * 96            # floats of one weight-gradient slab
DL_GPW, DL_WAVES = 16, 4      # patch.hip: 16-row groups per wave, waves per workgroup (NT / 64)
TWAVES = 4                    # embed_tail.hip
TAIL_NPART = 16 * 6 * 16 + 256 + 16 + 2 * 16 * 6      # tail_npart<6>(): G | M2 | P1 | s1 | s2
LOSS_LIMBS = 5                # BF_LOSS_LIMBS
LIMB_UNIT = 2.0 ** (128 - 48 * LOSS_LIMBS)            # the lowest limb counts units of 2^-112
U_DIV = 3 * U32               # a / n: reciprocal (1 ulp = 2u) and product


# ---------------------------------------------------------------------------------------------------- restated host code
def wave_split(tiles, cus):
    """gather_gemm_launch / bf_scatter_gemm -> (rounds, nwaves, grid)."""
    full = 2 * cus * GW
    rounds = -(-tiles // full)
    nwaves = -(-tiles // rounds)
    return rounds, nwaves, -(-nwaves // GW)


def wave_runs(tiles, cus):
    """-> [(t_beg, t_end)] of every wave of the grid (empty runs included), as the kernels compute them."""
    nw = wave_split(tiles, cus)[2] * GW
    return [(tiles * wv // nw, tiles * (wv + 1) // nw) for wv in range(nw)]


def wgrad_runs(Fr, tpf, ws_floats=None):
    """Runs per frame of bf_gather_wgrad (0: declined).  ws_floats None: the preferred launch."""
    rpf = 0
    for r in range(1, tpf + 1):
        if tpf % r == 0 and Fr * r <= 512 and (ws_floats is None or Fr * r * SLAB <= ws_floats):
            rpf = r
    return rpf


def wgrad_ws_floats(Fr, gh, gw):
    return Fr * wgrad_runs(Fr, gh * gw // 32) * SLAB if (gh * gw) % 32 == 0 else 0


def tail_plan(S1):
    """embed_tail.hip tail_plan() -> (tiles per wave, runs per frame) or None."""
    if S1 <= 0 or S1 % (32 * TWAVES):
        return None
    wt = S1 // 32 // TWAVES
    tpw = next(t for t in range(6, 0, -1) if wt % t == 0)
    return tpw, wt // tpw


def tail_ws_floats(Fr, gh1, gw1):
    p = tail_plan(gh1 * gw1)
    return 0 if p is None else Fr * p[1] * 4 * TAIL_NPART + Fr * 96 * 16 + Fr * 2 * 96


def dl_split(h, w):
    """Last-stage kernels -> dict(groups per frame, waves that work, workgroups per frame, slices = ceil(h w / 256), rows of the last
    slice)."""
    GF = h * w // 16
    nsl = -(-GF // DL_GPW)
    return dict(groups=GF, waves=nsl, wgs=-(-GF // (DL_WAVES * DL_GPW)), slices=nsl, last_rows=16 * (GF - (nsl - 1) * DL_GPW))


# ---------------------------------------------------------------------------------------------------- layouts
def gather_rows(img, gh, gw):
    """(F, 2 gh, 2 gw, C) -> (F gh gw, 4 C), columns (q = 2 ky + kx, c)."""
    return GB.patches(img, gh, gw)


def scatter_rows(m, Fr, gh, gw):
    """(F gh gw, 4 C) with columns (q, c) -> the fine map (F, 2 gh, 2 gw, C)."""
    C = m.shape[1] // 4
    return m.reshape(Fr, gh, gw, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(Fr, 2 * gh, 2 * gw, C)


def pm_rows(t, h, w):
    """NCHW (F, Co, 2h, 2w) -> patch-major rows (F h w, 16), n = co * 4 + ky * 2 + kx, zero beyond 4 Co."""
    Fr, Co = t.shape[:2]
    out = torch.zeros(Fr * h * w, 16, dtype=t.dtype, device=t.device)
    out[:, :4 * Co] = t.reshape(Fr, Co, h, 2, w, 2).permute(0, 2, 4, 1, 3, 5).reshape(Fr * h * w, 4 * Co)
    return out


def nchw(pm, Fr, Co, h, w):
    """Patch-major rows (F h w, >= 4 Co) -> NCHW (F, Co, 2h, 2w)."""
    return pm[:, :4 * Co].reshape(Fr, h, w, Co, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(Fr, Co, 2 * h, 2 * w)


def _pf(t, v):
    """A per-(frame, channel) table (F, C) broadcast against v (F, ..., C)."""
    t = t.double()
    return t.reshape(t.shape[0], *([1] * (v.dim() - 2)), t.shape[1])


# ---------------------------------------------------------------------------------------------------- operands
def round16(a, ea):
    r = rnd16(a)
    return r, torch.maximum(rnd16(a + ea) - r, r - rnd16(a - ea))


def store16(v, e):
    return v, (1 + U16) * e + U16 * v.abs()


def affine_gelu(v, sc, sh, ev=None, fused=True):
    """gelu_fast(v sc + sh) in fp32, v (F, ..., C) exact or known to within ev, sc / sh (F, C) -> (a, ea) before the bf16 rounding."""
    v = v.double()
    s, h = _pf(sc, v), _pf(sh, v)
    t = v * s + h
    et = U32 * t.abs() if fused else 2 * U32 * ((v * s).abs() + h.abs())
    if ev is not None:
        et = et + s.abs() * ev * (1 + 2 * U32)
    return GB.gelu(t, et, True)


def pro_operand(v, sc=None, sh=None, ev=None, fused=True):
    """The MFMA operand bf16(gelu_fast(fmaf(v, sc, sh))) (sc None: v itself, exact) -> (a, ea)."""
    if sc is None:
        return v.double(), torch.zeros_like(v, dtype=torch.float64)
    return round16(*affine_gelu(v, sc, sh, ev, fused))


def rebuilt(patches, w0):
    """patches (..., 16), w0 (C0, 16) exact -> (y, ey): the map rows bf16(patch . w0) as the reference rounds them."""
    p, w = patches.double(), w0.double()
    return round16(p @ w.t(), gamma(16) * (p.abs() @ w.abs().t()))


# ---------------------------------------------------------------------------------------------------- gather / scatter GEMM
def gather(a, ea, w_nk, gh, gw):
    """a / ea (F, 2 gh, 2 gw, C0) from pro_operand, w_nk (N, 4 C0) [n][(q, c)] -> (ref, bnd) (F gh gw, N) of the bf16 output."""
    w = w_nk.double()
    S, eS = GB.product(gather_rows(a, gh, gw), gather_rows(ea, gh, gw), w, torch.zeros_like(w), w.shape[1])
    return store16(S, eS)


def scatter(a, ea, w_nk, Fr, gh, gw):
    """a / ea (F gh gw, K) from pro_operand, w_nk (4 C0, K) [(q, c)][k] -> (ref, bnd) of the fine map (F, 2 gh, 2 gw, C0)."""
    w = w_nk.double()
    S, eS = GB.product(a, ea, w, torch.zeros_like(w), w.shape[1])
    ref, bnd = store16(S, eS)
    return scatter_rows(ref, Fr, gh, gw), scatter_rows(bnd, Fr, gh, gw)


def slice_partials(x, pow2):
    """x (..., n, C): the stored rows of one slice each -> {"mean": (ref, bnd), "m2": (ref, bnd)} of shape (..., C).  pow2: the mean is
    t1 * (1 / n) with n a power of two (exact), else t1 / n."""
    x = x.double()
    n = x.shape[-2]
    t1, t2 = x.sum(-2), (x * x).sum(-2)
    e1, e2 = gamma(n) * x.abs().sum(-2), gamma(n) * t2
    mu = t1 / n
    e_mu = e1 / n + (0.0 if pow2 else U_DIV * (mu.abs() + e1 / n))
    p = (t1 * mu).abs()
    e_q = O2 * (e2 + t1.abs() * e_mu + mu.abs() * e1 + e1 * e_mu + U32 * p + U32 * (t2 + p))
    return dict(mean=(mu, e_mu), m2=((t2 - t1 * mu).clamp_min(0.0), e_q))


def sliced(x, rows, pow2):
    """x (F, S, C) -> slice_partials of every `rows`-row slice (the last one ragged), stacked to (F, slices, C)."""
    parts = [slice_partials(x[:, s0:s0 + rows], pow2) for s0 in range(0, x.shape[1], rows)]
    return {k: tuple(torch.stack([p[k][i] for p in parts], 1) for i in range(2)) for k in ("mean", "m2")}


def scatter_tiles(fmap, gh, gw):
    """The fine map (F, 2 gh, 2 gw, C) -> (F, tiles, 128, C): the 128 pixels each 32-row tile of scatter_gemm_kernel stored."""
    Fr, C = fmap.shape[0], fmap.shape[3]
    return gather_rows(fmap, gh, gw).reshape(Fr, gh * gw // 32, 32 * 4, C)


# ---------------------------------------------------------------------------------------------------- weight gradients
def wgrad(A, eA, B, eB, steps, slabs):
    """A / eA (P, 384) the fine operand rows (q, c), B / eB (P, 96) the coarse rows -> (ref, bnd) of dW (384, 96), fp32."""
    return GB.product(A.t().contiguous(), eA.t().contiguous(), B.t().contiguous(), eB.t().contiguous(), 32 * steps + slabs)


# ---------------------------------------------------------------------------------------------------- last stage
def debed_last(act, sc, sh, wc, Fr, Co, h, w):
    """act (F h w, Ci), sc / sh (F, Ci), wc (Ci, 16) -> (ref, bnd) of pred (F, Co, 2h, 2w), fp32."""
    Ci = act.shape[1]
    a, ea = pro_operand(act.reshape(Fr, h * w, Ci), sc, sh, fused=False)
    wt = wc.double().t().contiguous()
    S, eS = GB.product(a.reshape(-1, Ci), ea.reshape(-1, Ci), wt, torch.zeros_like(wt), Ci)
    return nchw(S, Fr, Co, h, w), nchw(eS, Fr, Co, h, w)


def loss_limbs(pred, y, h, w):
    """pred the kernel's own stored prediction, y the target (F, Co, 2h, 2w) -> {"num" | "den": (ref, bnd)} (F, Co)."""
    p, t = pred.double(), y.double()
    num, den = ((p - t) ** 2).sum((2, 3)), (t * t).sum((2, 3))
    q = dl_split(h, w)["waves"] * LIMB_UNIT / 2
    return dict(num=(num, gamma(2 + 1 + 4 * DL_GPW + 4) * num + q), den=(den, gamma(1 + 4 * DL_GPW + 4) * den + q))


def dpm(h, w, dpred=None, pred=None, y=None, coef=None, gscale=None):
    """The three source modes -> (ref, err) of the bf16 rows (F h w, 16); err == 0 wherever the kernel must be bit-equal."""
    if pred is None:
        v = pm_rows(dpred.double(), h, w)
        return rnd16(v), torch.zeros_like(v)
    cf = coef.double() * (1.0 if gscale is None else float(gscale.double().reshape(-1)[0]))
    e_cf = (0.0 if gscale is None else U32) * cf.abs()
    cf, e_cf = cf[:, :, None, None], e_cf[:, :, None, None]
    d = pred.double() - y.double()
    e_d = U32 * d.abs()
    g = torch.zeros_like(d) if dpred is None else dpred.double()
    v = cf * d + g
    e = O2 * (d.abs() * e_cf + cf.abs() * e_d + e_cf * e_d + U32 * ((cf * d).abs() + g.abs()))
    return round16(pm_rows(v, h, w), pm_rows(e, h, w))


def rank16(rows, wc):
    """dact / y0 = bf16(rows (P, 16) . wc (C, 16)^T), rows the kernel's own stored dpm / patches -> (ref, bnd)."""
    r, wt = rows.double(), wc.double()
    return store16(*GB.product(r, torch.zeros_like(r), wt, torch.zeros_like(wt), 16))


def _xhat(y, mean, rstd, ey=None):
    """xh = fmaf(y, rstd, fl(-mean rstd)) -> (xh, e_xh)."""
    m, r = _pf(mean, y), _pf(rstd, y)
    xh = (y - m) * r
    e = O2 * (U32 * (m * r).abs() + U32 * xh.abs())
    return xh, e if ey is None else e + r.abs() * ey * (1 + 2 * U32)


def _dd(D, e_D, z, e_z):
    """dd = fl(D gelu'(z)) -> (dd, e_dd)."""
    d, e_d = GB.dgelu_poly(z)
    e_d = e_d + NB.L_DGELU * e_z
    dd = D * d
    return dd, O2 * (D.abs() * e_d + e_D * d.abs() + e_D * e_d + U32 * dd.abs())


def _two_sums(dd, e_dd, xh, e_xh, n):
    """s1 = sum dd, s2 = sum dd xh over dim 1 with sums of length n -> ((s1, e1), (s2, e2))."""
    s1 = dd.sum(1)
    e1 = e_dd.sum(1) + gamma(n) * (dd.abs() + e_dd).sum(1)
    p = dd * xh
    e_p = e_dd * xh.abs() + dd.abs() * e_xh + e_dd * e_xh
    return (s1, e1), (p.sum(1), e_p.sum(1) + gamma(n + 1) * (p.abs() + e_p).sum(1))


def debed_last_bwd_norm(dpm_rows, wc, ymap, mean, rstd, in_w, in_b, Fr):
    """dpm_rows (P, 16) the kernel's own stored rows, wc (Ci, 16), ymap (P, Ci), mean / rstd (F, Ci), in_w / in_b (Ci,)
    -> {"dx": (ref, bnd) (P, Ci), "s1" | "s2": (ref, bnd) (F, Ci)}."""
    Ci = ymap.shape[1]
    y = ymap.double().reshape(Fr, -1, Ci)
    S = y.shape[1]
    m, r, wv, bv = mean.double(), rstd.double(), in_w.double()[None], in_b.double()[None]
    a = r * wv
    e_a = U32 * a.abs()
    shp = bv - m * a
    e_sh = O2 * (m.abs() * e_a + U32 * shp.abs())
    z = y * a[:, None] + shp[:, None]
    e_z = O2 * (y.abs() * e_a[:, None] + e_sh[:, None] + U32 * z.abs())
    wt = wc.double()
    D = (dpm_rows.double() @ wt.t()).reshape(Fr, S, Ci)
    e_D = gamma(16) * (dpm_rows.double().abs() @ wt.abs().t()).reshape(Fr, S, Ci)
    dd, e_dd = _dd(D, e_D, z, e_z)
    xh, e_xh = _xhat(y, mean, rstd)
    nsl = -(-S // (16 * DL_GPW))
    (s1, e1), (s2, e2) = _two_sums(dd, e_dd, xh, e_xh, S + nsl)
    t1, t2 = s1[:, None] / S, s2[:, None] / S
    e_t1 = O2 * (e1[:, None] / S + 2 * U32 * t1.abs())
    e_t2 = O2 * (e2[:, None] / S + 2 * U32 * t2.abs())
    I = dd - t1 - xh * t2
    Mg = dd.abs() + t1.abs() + (xh * t2).abs()
    E = e_dd + e_t1 + e_xh * t2.abs() + xh.abs() * e_t2 + e_xh * e_t2
    E_I = E + 3 * U32 * (Mg + E)
    A = a[:, None].abs()
    v = a[:, None] * I
    dx = store16(v.reshape(-1, Ci), (A * E_I + gamma(2) * A * (I.abs() + E_I)).reshape(-1, Ci))
    return dict(dx=dx, s1=(s1, e1), s2=(s2, e2))


# ---------------------------------------------------------------------------------------------------- embed tail
def embed_tail(dy1, w1, patches, w0, sc, sh, mean, rstd, in_w, Fr, gh1, gw1, y0=None, prior_w=None, prior_b=None):
    """dy1 (F gh1 gw1, C1), w1 (C1, 4 C0) columns (q, c), patches (F 4 gh1 gw1, 16) in pixel order, w0 (C0, 16), sc / sh / mean / rstd
    (F, C0) the GIVEN fp32 tables, in_w (C0,), y0 (F 4 gh1 gw1, C0) or None (rebuilt)
    -> {"dwprep": (C0, 16), "d_in_w" | "d_in_b": (C0,)}: (ref, bnd) each."""
    C0, C1 = w0.shape[0], dy1.shape[1]
    S1, S0 = gh1 * gw1, 4 * gh1 * gw1
    tpw, cpf = tail_plan(S1)
    n = 32 * tpw + 4 + 4 * cpf
    pt = patches.double().reshape(Fr, S0, 16)
    if y0 is None:
        y, ey = rebuilt(pt, w0)
    else:
        y, ey = y0.double().reshape(Fr, S0, C0), None
    a, b = dy1.double(), w1.double()
    D = scatter_rows(a @ b, Fr, gh1, gw1).reshape(Fr, S0, C0)
    e_D = gamma(C1) * scatter_rows(a.abs() @ b.abs(), Fr, gh1, gw1).reshape(Fr, S0, C0)
    z = y * _pf(sc, y) + _pf(sh, y)
    e_z = U32 * z.abs()
    if ey is not None:
        e_z = e_z + _pf(sc, y).abs() * ey * (1 + 2 * U32)
    dd, e_dd = _dd(D, e_D, z, e_z)
    xh, e_xh = _xhat(y, mean, rstd, ey)
    (s1, e1), (s2, e2) = _two_sums(dd, e_dd, xh, e_xh, n)
    d16, e16 = round16(dd, e_dd)
    pa = pt.abs()
    G = d16.transpose(1, 2) @ pt                                                       # (F, C0, 16)
    e_G = e16.transpose(1, 2) @ pa + gamma(n) * ((d16.abs() + e16).transpose(1, 2) @ pa)
    M2, aM2 = pt.transpose(1, 2) @ pt, pa.transpose(1, 2) @ pa                         # (F, 16, 16)
    e_M2 = gamma(n) * aM2
    P1, e_P1 = pt.sum(1), gamma(n) * pa.sum(1)                                         # (F, 16)
    w0d = w0.double()
    WM = w0d @ M2                                                                      # (F, C0, 16)
    e_WM = w0d.abs() @ e_M2 + gamma(16) * (w0d.abs() @ (aM2 + e_M2))
    m, r = mean.double()[:, :, None], rstd.double()[:, :, None]
    mP = m * P1[:, None]
    inner = WM - mP
    e_in = O2 * (e_WM + m.abs() * e_P1[:, None] + U32 * mP.abs() + U32 * (WM.abs() + mP.abs()))
    PX = r * inner
    e_PX = O2 * (r.abs() * e_in + U32 * PX.abs())
    t1, t2 = s1[:, :, None] / S0, s2[:, :, None] / S0
    e_t1 = O2 * (e1[:, :, None] / S0 + 2 * U32 * t1.abs())
    e_t2 = O2 * (e2[:, :, None] / S0 + 2 * U32 * t2.abs())
    T1, T2 = t1 * P1[:, None], t2 * PX
    I = G - T1 - T2
    Mg = G.abs() + T1.abs() + T2.abs()
    E = e_G + e_t1 * P1[:, None].abs() + t1.abs() * e_P1[:, None] + e_t1 * e_P1[:, None] + e_t2 * PX.abs() + t2.abs() * e_PX + e_t2 * e_PX
    E_I = E + 4 * U32 * (Mg + E)
    cf = r * in_w.double()[None, :, None]
    v = cf * I
    e_v = cf.abs() * E_I + gamma(2) * cf.abs() * (I.abs() + E_I)
    out = dict(dwprep=(v.sum(0), e_v.sum(0) + gamma(Fr) * (v.abs() + e_v).sum(0)))
    for name, (s, e), pr in (("d_in_b", (s1, e1), prior_b), ("d_in_w", (s2, e2), prior_w)):
        p = torch.zeros_like(s[0]) if pr is None else pr.double().to(s.device)
        out[name] = (s.sum(0) + p, e.sum(0) + gamma(Fr + 1) * ((s.abs() + e).sum(0) + p.abs()))
    return out
