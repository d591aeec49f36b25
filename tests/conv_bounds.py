"""Per-element error bounds for the implicit-GEMM convolutions of csrc/conv.hip.

Given the exact (fp64) values a conv reads -- its stored sources, the fp32 GroupNorm scale / shift of its prologue, its weight operand
already rounded to the compute dtype (ops._wfwd / ops._wswap) -- the functions below return the fp64 reference output `ref` and an
elementwise bound `bnd` such that a correct kernel satisfies |got - ref| <= bnd everywhere.  `check` asserts it and reports the worst
ratio |got - ref| / bnd and where it occurs.  Tensors are NCHW fp64 (frames first); the GPU tests convert the native layouts.

How the kernel rounds (conv.hip: gather(), mma_tile(), the epilogues) and what that costs -- u = 2^-24 is the fp32 unit roundoff:

Operand a (the gathered row, `gather()`).  An in-bounds tap reads v (exact: a stored bf16 / fp32 value) and applies the prologue in fp32;
padding taps are exact zeros (the reference pads the already-activated tensor).  The prologue is t = fmaf(v, sc, sh), then
gelu(t) = 0.5f * t * (1 + erff(t * c)), c = fp32(1/sqrt 2).  With T = |v*sc| + |sh| >= |t| (T = |v| for GELU alone):
  - fmaf rounds once: |dt| <= u|t|; gelu is 1.13-Lipschitz (max gelu' = 1.1289): <= 1.13 u T.
  - t * c carries 2u relative (the product and the constant); erf' * |x| = (2/sqrt pi) |x| exp(-x^2) <= 0.484, so erf moves by
    <= 0.97 u, times 0.5|t|: <= 0.49 u T.
  - erff itself is within 2 ulp (HIP's documented bound); ulp(erf) <= 2u |erf| <= 2u, times 0.5|t|: <= 2 u T.
  - 1 + erf and the final product round once each: <= 2u |a|.
  Sum 3.62 u T + 2 u |a| (+ O(u^2)), so eps_a = C_PRO * u * (T + |a|) with C_PRO = 4.  This form stays meaningful where v*sc and sh
  cancel (t ~ 0).  Without a prologue eps_a = 0.
In bf16 mode the kernel rounds its fp32 `a` to bf16 (RNE) before the MFMAs, and so does the reference: a = rnd(a_exact).  The two agree
unless a rounding boundary lies within eps_a of a_exact; rounding is monotone, so the kernel's operand lies in
[rnd(a - eps_a), rnd(a + eps_a)] and the operand error is at most the larger distance from rnd(a) to either end -- one bf16 ulp
(<= 2^-7 |a|) at such a point, zero elsewhere.  (An fp32 source read in bf16 mode, the nchw clip, is rounded the same way.)
In fp32 mode the operand error is eps_a.  The weight operand is exact: the caller rounds it before the call.

Sum (`mma_tile()`).  The kernel accumulates the n products of an output in fp32, in MFMA order.  Whatever the order, a dot product of
length n computed with unit roundoff u is within gamma_n * sum |a||w| of the exact one, gamma_n = n u / (1 - n u) (Higham, Accuracy
and Stability of Numerical Algorithms, Thm 3.1: products and additions rounded to nearest).  bf16 x bf16 products are exact in fp32,
so that case is covered a fortiori.  n is the length of the kernel's sum: kh*kw*Cin for a forward conv, the taps of the largest parity
phase times Cin for a transposed one, chunk + slabs for a weight gradient (each slab's sum, then the fixed-order slab sum), chunk +
slabs for a column sum.  The epilogue's bias and residual additions and an `accumulate` add are two / one more terms of the same sum,
with their magnitudes in sum |.|.

Store.  The result is rounded to the output dtype: |rnd(v) - ref| <= (1 + u_out) |v - ref| + u_out |ref|, u_out = 2^-24 for fp32
stores and 2^-8 for bf16 (its unit roundoff, p = 8 bits) -- one unit also covers a value at a rounding boundary going either way.

So bound = (1 + u_out) * (conv(operand error, |w|) + gamma_n * conv(|a|, |w|)) + u_out |ref|, every constant from the above and none
fitted to GPU results.
"""
import math

import torch
import torch.nn.functional as F

U32, U16 = 2.0 ** -24, 2.0 ** -8
C_PRO = 4.0
PRO_NONE, PRO_AFFINE_GELU, PRO_GELU = 0, 1, 2          # L.BF_CONV_PRO_*
CBK, CBM, CBN = 32, 64, 64                             # conv.hip tile sizes (wgrad slabs are whole multiples of CBK pixels)


def rnd16(t):
    return t.to(torch.bfloat16).double()


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def prologue(v, pro, sc=None, sh=None):
    """Exact prologue of the stored values v (F, C, H, W) -> (a, T); sc / sh (F, C) hold the kernel's fp32 values."""
    if pro == PRO_NONE:
        return v, None
    if pro == PRO_AFFINE_GELU:
        s, h = sc.double()[:, :, None, None], sh.double()[:, :, None, None]
        t, T = v * s + h, (v * s).abs() + h.abs()
    else:
        t, T = v, v.abs()
    return F.gelu(t), T


def operand(v, pro=PRO_NONE, sc=None, sh=None, bf16=False):
    """-> (a, ea): the operand the MFMAs consume, as the fp64 reference rounds it, and the elementwise bound on the kernel's deviation."""
    a, T = prologue(v.double(), pro, sc, sh)
    eps = torch.zeros_like(a) if T is None else C_PRO * U32 * (T + a.abs())
    if not bf16:
        return a, eps
    r = rnd16(a)
    return r, torch.maximum(rnd16(a + eps) - r, r - rnd16(a - eps))


def _fit(t, H, W):
    """Slice / zero-pad the spatial dims of t to H x W."""
    t = t[..., :H, :W]
    return F.pad(t, (0, W - t.shape[-1], 0, H - t.shape[-2]))


def _finish(ref, mag, err, n, u_out, extra=()):
    """ref / mag / err are the sum, its magnitude sum and its operand-error sum; `extra` more terms (bias, residual, prior value)."""
    for e in extra:
        if e is not None:
            ref, mag, n = ref + e, mag + e.abs(), n + 1
    bnd = (1 + u_out) * (err + gamma(n) * mag) + u_out * ref.abs()
    return ref, bnd


def _bc(b):
    return None if b is None else b.double()[None, :, None, None]


def conv_fwd(a, ea, w, stride, pad, Ho, Wo, bias=None, resid=None, out_bf16=False):
    """Forward gather: w (N, Cin, kh, kw) -> (ref, bound) of shape (F, N, Ho, Wo)."""
    c = lambda x, y: _fit(F.conv2d(x, y, stride=stride, padding=pad), Ho, Wo)
    w = w.double()
    n = w.shape[1] * w.shape[2] * w.shape[3]
    return _finish(c(a, w), c(a.abs(), w.abs()), c(ea, w.abs()), n, U16 if out_bf16 else U32, (_bc(bias), resid))


def transposed(x, w, stride, pad, Ho, Wo):
    """out[oy] += x[iy] w[ky] for oy = iy*s - p + ky in [0, Ho): the uncropped ConvTranspose2d shifted by p (F.conv_transpose2d's own
    padding would also drop the last p rows, which a data gradient with an odd input size needs)."""
    return _fit(F.conv_transpose2d(x, w, stride=stride)[..., pad:, pad:], Ho, Wo)


def conv_transposed(a, ea, w, stride, pad, Ho, Wo, bias=None, resid=None, out_bf16=False):
    """Transposed gather: w (Cin, N, kh, kw), out[oy] += a[iy] w[ky] where oy = iy*s - p + ky -> (ref, bound) (F, N, Ho, Wo)."""
    c = lambda x, y: transposed(x, y, stride, pad, Ho, Wo)
    w = w.double()
    n = w.shape[0] * math.ceil(w.shape[2] / stride) * math.ceil(w.shape[3] / stride)
    return _finish(c(a, w), c(a.abs(), w.abs()), c(ea, w.abs()), n, U16 if out_bf16 else U32, (_bc(bias), resid))


def wgrad_split(R, K, M):
    """(chunk, slabs) of bf_conv_wgrad: wgrad_slabs() in conv.hip, which sizes the fixed-order pixel slabs."""
    tiles = -(-R // CBM) * -(-K // CBN)
    s = min(-(-512 // tiles), -(-M // (8 * CBK)), 64)
    while s > 1 and s * R * K > 64 << 20:
        s -= 1
    s = max(s, 1)
    chunk = -(-(-(-M // s)) // CBK) * CBK
    return chunk, -(-M // chunk)


def unfold(a, k, stride, pad, Ho, Wo):
    """Forward-gather operand rows: (F, Cin, Hi, Wi) -> (F*Ho*Wo, k*k*Cin), k ordered (ky, kx, c) as the kernel orders it."""
    Fr, Cin = a.shape[:2]
    Hn = (a.shape[2] + 2 * pad - k) // stride + 1
    Wn = (a.shape[3] + 2 * pad - k) // stride + 1
    u = F.unfold(a, k, padding=pad, stride=stride).view(Fr, Cin, k * k, Hn, Wn)
    u = _fit(u, Ho, Wo)
    return u.permute(0, 3, 4, 2, 1).reshape(Fr * Ho * Wo, k * k * Cin)


def conv_wgrad(rows, a, ea, k, stride, pad, prior=None):
    """Weight gradient dW[r][(ky, kx, c)] = sum_m rows[m][r] * gather(a)[m][(ky, kx, c)]: rows (F, R, Ho, Wo) is the exact operand
    (already rounded as the kernel rounds it), a / ea from operand().  prior: the (R, K) values an accumulate = 1 call adds to.
    -> (ref, bound) of shape (R, K), the kernel's layout."""
    Fr, R, Ho, Wo = rows.shape
    rm = rows.double().permute(0, 2, 3, 1).reshape(-1, R)
    A, E = unfold(a, k, stride, pad, Ho, Wo), unfold(ea, k, stride, pad, Ho, Wo)
    chunk, slabs = wgrad_split(R, A.shape[1], rm.shape[0])
    return _finish(rm.t() @ A, rm.abs().t() @ A.abs(), rm.abs().t() @ E, chunk + slabs, U32, (prior,))


def colsum(x, prior=None):
    """Per-channel pixel sums of bf_conv_colsum: x (F, C, H, W) exact -> (ref, bound) of shape (C,)."""
    M = x.shape[0] * x.shape[2] * x.shape[3]
    chunk = -(-M // 64)
    xm = x.double().transpose(0, 1).reshape(x.shape[1], -1)
    return _finish(xm.sum(1), xm.abs().sum(1), 0.0, chunk + 64, U32, (prior,))


def check(got, ref, bnd, what, names=("frame", "channel", "y", "x")):
    """Assert |got - ref| <= bnd elementwise; -> the worst ratio |got - ref| / bnd."""
    got = got.detach().double().cpu().reshape(ref.shape)
    ref, bnd = ref.cpu(), bnd.cpu()
    assert torch.isfinite(got).all(), (what, "non-finite output")
    ratio = (got - ref).abs() / bnd.clamp_min(1e-300)
    ratio = torch.where((got - ref) == 0, torch.zeros_like(ratio), ratio)
    worst = float(ratio.max())
    if worst > 1.0:
        idx = [int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape)]
        where = ", ".join(f"{n}={i}" for n, i in zip(names, idx))
        raise AssertionError(f"{what}: |got - ref| exceeds the bound by {worst:.3g}x at ({where}): got {float(got[tuple(idx)]):.9g}, "
                             f"ref {float(ref[tuple(idx)]):.9g}, bound {float(bnd[tuple(idx)]):.3g}; "
                             f"{int((ratio > 1).sum())} of {ratio.numel()} elements out of bounds")
    return worst


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))
