"""fp64 reference and per-element error bounds for the attention kernels (csrc/attn_mfma.hip, csrc/attn.hip; 1 <= L <= 32) and for
csrc/attn_long.hip (33 <= L <= 128: the modes LONG_BF16 / LONG_FP32, "Long axes" below).

Given the stored values a kernel reads (qkv, dout, the fp32 parameters, the prior content of an accumulated output), the functions below
return for every output the fp64 value `ref` of bf_attn_fwd / bf_attn_bwd's contract and an elementwise `bnd` such that a correct kernel
satisfies |got - ref| <= bnd.  `check` asserts it and reports the worst ratio and its (sequence, head, row, channel).  Two independent
restatements live here: `reference` / `reference_axial` differentiate the forward with autograd; `plain` / `axial_pair` write every
gradient out by hand, because the bound needs the intermediates.  tests/test_attn_bounds.py holds the two to 1e-10 of each other.

A `Mode` says where a kernel rounds: u_op, the unit roundoff of the MFMA operands it forms (2^-8 for bf16: 8 significand bits, round to
nearest even, so |rnd(x) - x| <= 2^-8 |x| -- half a unit in the last place of a binade's smallest value; 0 when the operands stay fp32),
and u_st, that of its stores.  MFMA = (2^-8, 2^-8), GENERIC_BF16 = (0, 2^-8) (attn.hip on bf16 tensors: bf16 in and out, fp32 between),
FP32 = (0, 2^-24).  u = 2^-24 below is fp32's; gamma_n = n u / (1 - n u) bounds an n-term fp32 sum in ANY order by gamma_n sum |terms|
(Higham, Accuracy and Stability of Numerical Algorithms, Thm 3.1 / section 4.2), bf16 x bf16 products being exact in fp32 a fortiori.
Every rounding is charged a full unit (no boundary-flip argument as in conv_bounds.py: the softmax would make it intractable), errors
are propagated through the fp64 intermediates to first order with the second-order cross terms of every product kept, and the softmax
is enclosed exactly, not linearised.  No constant is fitted to a GPU result.

Forward, in the order the kernel computes (attn_mfma.hip: ln_quad, affine_frag, scores_softmax_pre, pack_keys, the P V loop):
  inputs     q, k, v rows are stored bf16 / fp32 values: exact.
  LayerNorm  fp32.  mu = sum / d: |d mu| <= gamma_{d+1} mean|x| =: em.  t = x - mu: et = em + u |t|.  var = mean t^2:
             evar = mean(2 |t| et) + gamma_{d+3} var.  r = rsqrtf(var + eps), within 2 ulp: relative er = evar / (2 (var + eps)) + 4 u.
             xhat = t r: exh = et r + |xhat| er + u |xhat|.  em is what keeps the bound honest for rows with a large common offset
             (|x| >> |t|), where the subtraction cancels.
  operands   Qn = (xhat qw + qb) d^-1/2, Kn = xhat kw + kb: eq = (exh |w| + 2 u (|xhat w| + |b|)) mul + 3 u |Qn| (the product by
             rsqrtf(d), itself 2 ulp), then rounded to the operand type: eq (1 + u_op) + u_op |Qn|  (affine_frag's bf16 conversion).
  scores     S = Qn Kn^T + emb[bucket]: eS = |Qn| ek + eq |Kn| + eq ek + gamma_d |Qn| |Kn|^T + 2 u (|S| + |emb|).  Buckets come from
             tests/golden/relpos_tables.npz (the reference's table), never from the device function.
  softmax    a = S - max, e = __expf(a) = exp2(a log2 e): the subtraction, the product and the constant each move the exponent by
             <= u |a|, the hardware exp2 is within 1 ulp: together a shift D = eS + u (3 |a| + 2) of the score.  For |delta_j| <= D_j the
             perturbed P_j = P_j e^dj / sum_k P_k e^dk is largest at dj = +Dj, dk = -Dk and smallest at the opposite corner; eP is the
             larger distance from P to those two values -- exact for any size of D (scores of +-30 carry D ~ 0.5, where a first-order
             softmax bound would be wrong).  The fp32 sum, reciprocal and product add gamma_{L+6} P.
  rescale    A = 1/L + (P - 1/L) hscale with 1/L = fp32(1) / fp32(L) as the kernel forms it: eA = eP |hs| + 3 u (1/L + |P - 1/L| |hs|);
             without hscale A = P.  pack_keys rounds A to the operand type: eAb = eA (1 + u_op) + u_op |A|.
  P V        O = A V, V exact, 32 k-slots in fp32: eO = eAb |V| + gamma_32 |A| |V|.
  store      val = O out_scale (+ the old stored value, exact, or the first axial pass's value with its own bound):
             e = eO |out_scale| + u |O out_scale| + e_old + u |val|;  bnd = (1 + u_st) e + u_st |val|.
Backward (attn_bwd_mfma), dO being stored values:
  dP0 = (dO V^T) out_scale: exact operands, e = gamma_d |dO| |V|^T |os| + u |dP0|.  dhscale_p = sum (P - 1/L) dP0 carries eP.
  dP = dP0 hs;  dot = sum_j P dP;  dS = P (dP - dot): eS' = eP |dP - dot| + (P + eP)(e_dP + e_dot) + 2 u |dS|.  demb_p sums dS by bucket.
  A^T and dS^T pass through bf16 LDS tiles (and pack_keys): e (1 + u_op) + u_op |.| each.  dV = A^T dO out_scale, dKn = dS^T Qn,
  dQn = d^-1/2 dS Kn with Qn, Kn the rounded operands (eq, ek above): three 32-slot fp32 products, cross terms kept.
  LayerNorm backward, fp32: g = d0 w, m1 = mean g, m2 = mean(g xhat), dx = r (g - m1 - xhat m2), every term carrying e_d0, exh and er;
  dw_p = sum_rows d0 xhat, db_p = sum_rows d0.  Stores as in the forward (accumulate 1 adds the old stored value after the LayerNorm).
  Raw modes (accumulate 2, then 5): the first pass stores bf16(dQn), bf16(dKn) -- one rounding, e (1 + u_st) + u_st |.| -- and the
  second adds them to its own in front of the one LayerNorm backward; the reference is the fp64 gradient of the sum of both passes.
Parameter gradients are sums over all problems: ref = sum_p ref_p, bnd = sum_p bnd_p + gamma_n sum_p sum |terms|, n the number of
addends of the whole sum (problems x rows, or x pairs of a bucket): valid for the registers, LDS atomics, workspace rows and global
atomics alike.  dkb is structurally zero (sum_j dS_ij = 0) and gets its absolute bound from the same formula.
The InstanceNorm bf_attn_axial_norm_fwd appends reads the bf16 values it has just stored, so `instance_norm` takes the kernel's own
`out` as exact input: fp32 two-pass statistics over the S tokens (gamma_{S+2}), one bf16 store.

Long axes (attn_long.hip; Mode.long): LONG_BF16 = (2^-8, 2^-8, long), LONG_FP32 = (0, 2^-24, long).  u_op is the rounding of pack4, which
turns every MFMA operand to bf16 as it leaves LDS; in the fp32 mode all six products are plain fp32 sums (fused or not: gamma_n covers
either) and u_op = 0.  Everything not restated here is as above.  Where the kernel rounds differently (row_stats, stage, scores,
softmax_rows, mm_block, attn_fwd_long, attn_bwd_long):
  term counts  O = A V, dV = A^T g, dqn = dS kn, dkn = dS^T qn sum over the L keys (queries): the MFMA path runs to LP = 16 ceil(L / 16) with
             exact zeros (staged rows >= L are zero, P is zero in padded rows and keys), so gamma_L, not gamma_32.  S and dA sum over d
             (columns >= d staged as zero): gamma_d.
  operands   d^-1/2 is not folded into q: qn = xhat qw + qb and kn are staged as they stand, eq = exh |w| + 2 u (|xhat w| + |b|), then
             rounded: eq (1 + u_op) + u_op |qn|.
  scores     S = acc * rsqrtf(d) + emb: rsqrtf within 2 ulp = 4 u, the product u: e = e_acc d^-1/2 (1 + 5 u) + 5 u |S|, then u |S + emb|.
             dqn and dkn are both acc * rsqrtf(d) in the same way, their operand being the unscaled kn / qn.
  softmax    one thread per row, keys in order: max, __expf(s - m) (the shift D as above), an fp32 sum of L terms, inv = 1.f / sum, e * inv:
             L - 1 additions, the division, the product <= gamma_{L+6} as above.  ASSUMED: the fp32 division 1.f / x is within 2 ulp
             (4 u; the compiler's default is the correctly rounded one).  The rescale is done in fp32 in place: eA as above.
  P V        the forward rounds A in mm_block: (1 + u_op) eA + u_op |A|.  The computed row is P~ (1 + theta), P~ = e_j / sum e exactly
             normalised and within the enclosure of P, |theta| <= gamma_{L+6}; the P~ - P sum to zero over the keys, so that part of the
             error only meets V's deviation from a constant c (the per-channel mean over the keys is used):
             eO = [encl |V - c| + gamma_{L+6} (P + encl) |V|] |hs| + 3 u (1/L + |P - 1/L| |hs|) |V|, times (1 + u_op), + u_op |A| |V| +
             gamma_L |A| |V|.  (Without this a V of 48 .. 150 would carry the whole softmax perturbation times |V|.)
  dA         stage forms g = dO out_scale in fp32, and pack4 rounds it: e_g = u |g| (1 + u_op) + u_op |g|, or 0 when out_scale = +-2^k
             (both steps exact).  dP0 = g V^T: e = e_g |V|^T + gamma_d |g| |V|^T, no product afterwards.  dV = A^T g uses the same
             staged operand and A rescaled anew from P in fp32 (the same three roundings), rounded: eAb^T (|g| + e_g) + |A|^T e_g +
             gamma_L |A|^T |g|.
  dS         dh = sum (P - 1/L) dA, dot = sum P dP and dS = P (dP - dot) are fp32, one thread per row in key order (dot: gamma_{L+1},
             dh: 2 u per term beside param_total's gamma_n); dS stays fp32 in LDS and is rounded once, as an operand of dqn / dkn.
  LayerNorm backward  m1, m2: one thread per row over d; dx, dw, db: one thread per column over the L rows; as ln_backward.
  parameter gradients  a workgroup adds its problems in order in LDS, its row goes through attn_reduce_block or float atomics:
             param_total with n = nseq heads L addends for dqw .. dkb, n = nseq L^2 for demb and dhscale, whatever the order.
  raw modes  only bf16 with d % 32 == 0.  Mode 2 stores bf16(dqn), bf16(dkn) and adds nothing to them (bit 0 is clear); mode 5 adds the
             stored values in front of the one LayerNorm backward and accumulates dV: as axial_pair, which takes a pair of modes when one
             pass is a short axis (attn_mfma.hip) and the other a long one.
"""
import math
import os
from collections import namedtuple
from types import SimpleNamespace as NS

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("dqw", "dqb", "dkw", "dkb", "demb", "dhscale")
U32, U16 = 2.0 ** -24, 2.0 ** -8
EPS = 1e-5
Mode = namedtuple("Mode", "u_op u_st long", defaults=(False,))
MFMA, GENERIC_BF16, FP32 = Mode(U16, U16), Mode(0.0, U16), Mode(0.0, U32)
LONG_BF16, LONG_FP32 = Mode(U16, U16, True), Mode(0.0, U32, True)        # csrc/attn_long.hip, 33 <= L <= 128


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def rnd16(t):
    return t.to(torch.bfloat16).to(t.dtype)


_TABLE = []


def t5_bucket(n):
    """T5 bucket of offset n = query - key from the reference's own table (tests/golden/relpos_tables.npz, L = 40): every |n| >= 27
    shares the last bucket of its side, so the 40-token table covers any length."""
    if not _TABLE:
        _TABLE.append(np.load(os.path.join(GOLDEN, "relpos_tables.npz"))["bucket_40"])
    n = max(-39, min(39, n))
    i = max(n, 0)
    return int(_TABLE[0][i][i - n])


_MATRIX = {}


def bucket_matrix(L, device="cpu"):
    """[query][key] -> bucket; built once per (L, device) and shared: callers must not write to it."""
    key = (L, str(device))
    if key not in _MATRIX:
        _MATRIX[key] = torch.tensor([[t5_bucket(i - j) for j in range(L)] for i in range(L)], device=device)
    return _MATRIX[key]


def geometry(kind, L, n_outer=3, inner=5):
    """(nseq, L, inner, outer_stride, inner_stride, tok_stride) and the token count: contiguous sequences, the temporal block's
    [B][T][S] layout, and the axial block's W and H passes over [F][h][w] frames."""
    if kind == "contig":
        return (4, L, 1, L, 0, 1), 4 * L
    if kind == "temporal":      # tokens [B][T = L][S = inner]
        return (n_outer * inner, L, inner, L * inner, 1, inner), n_outer * L * inner
    if kind == "W":             # frames [F = n_outer][h = inner][w = L]
        return (n_outer * inner, L, 1, L, 0, 1), n_outer * inner * L
    if kind == "H":             # frames [F][h = L][w = inner]
        return (n_outer * inner, L, inner, L * inner, 1, inner), n_outer * L * inner
    raise ValueError(kind)


def token_index(geo):
    nseq, L, inner, ostr, istr, tstr = geo
    s = torch.arange(nseq).view(-1, 1)
    return (s // inner) * ostr + (s % inner) * istr + torch.arange(L).view(1, -1) * tstr


def axial_geos(frames, h, w):
    """The W pass (rows of w tokens) and the H pass (columns of h tokens) over [frames][h][w] tokens."""
    return (frames * h, w, 1, w, 0, 1), (frames * w, h, w, h * w, 1, w)


# ------------------------------------------------------------------------------------------------ autograd restatement (all L in 1..128)
def _forward64(x, geo, heads, d, qw, qb, kw, kb, emb, hs, out_scale):
    """Differentiable fp64 forward on token rows x [N][3 E] -> out [N][E]; emb / hs None when the kernel gets NULL."""
    idx = token_index(geo).to(x.device)
    nseq, L = idx.shape
    t = x[idx].view(nseq, L, heads, 3, d).permute(0, 2, 1, 3, 4)           # [s][h][l][3][d]
    ln = lambda z, w, b: torch.nn.functional.layer_norm(z, (d,), eps=EPS) * w + b
    q, k, v = ln(t[..., 0, :], qw, qb), ln(t[..., 1, :], kw, kb), t[..., 2, :]
    sc = q @ k.transpose(-1, -2) / d ** 0.5
    if emb is not None:
        sc = sc + emb[bucket_matrix(L, x.device)].permute(2, 0, 1).unsqueeze(0)
    p = torch.softmax(sc, -1)
    if hs is not None:
        inv = float(np.float32(1.0) / np.float32(L))
        p = inv + (p - inv) * hs.view(1, heads, 1, 1)
    o = (p @ v).permute(0, 2, 1, 3).reshape(nseq * L, heads * d)
    return torch.zeros(x.shape[0], heads * d, dtype=torch.float64, device=x.device).index_add(0, idx.flatten(), o * out_scale)


def reference(qkv, dout, geo, heads, d, prm, out_scale, with_emb, with_hs):
    """fp64 forward and gradients of bf_attn_fwd's contract on the same input values."""
    x = qkv.double().detach().requires_grad_(True)
    qw, qb, kw, kb, emb, hs = (t.double().detach().requires_grad_(True) for t in prm)
    out = _forward64(x, geo, heads, d, qw, qb, kw, kb, emb if with_emb else None, hs if with_hs else None, out_scale)
    out.backward(dout.double())
    grads = [qw.grad, qb.grad, kw.grad, kb.grad, emb.grad if with_emb else torch.zeros_like(emb), hs.grad if with_hs else torch.zeros_like(hs)]
    return out.detach(), x.grad, grads


def reference_axial(qkv, dout, frames, h, w, heads, d, prm):
    """The axial pair: the W pass, then the H pass accumulated, each with out_scale 0.5, sharing the q / k LayerNorm.  prm =
    (qw, qb, kw, kb, emb, hscale_x, hscale_y) -> out, dqkv, [dqw, dqb, dkw, dkb, demb, dhscale_x, dhscale_y]."""
    x = qkv.double().detach().requires_grad_(True)
    ps = [t.double().detach().requires_grad_(True) for t in prm]
    gW, gH = axial_geos(frames, h, w)
    out = _forward64(x, gW, heads, d, *ps[:5], ps[5], 0.5) + _forward64(x, gH, heads, d, *ps[:5], ps[6], 0.5)
    out.backward(dout.double())
    return out.detach(), x.grad, [p.grad for p in ps]


# ------------------------------------------------------------------------------------------------ hand-written restatement with bounds
def to_problems(t, idx, heads, parts, d):
    """token rows [N][heads * parts * d] -> [s][h][l][parts][d]"""
    nseq, L = idx.shape
    return t.double()[idx.to(t.device)].view(nseq, L, heads, parts, d).permute(0, 2, 1, 3, 4)


def to_tokens(t, idx, N):
    """[s][h][l][d] -> [N][h][d]; tokens no sequence covers stay zero"""
    s, hh, L, d = t.shape
    out = torch.zeros(N, hh, d, dtype=t.dtype, device=t.device)
    out[idx.to(t.device).flatten()] = t.permute(0, 2, 1, 3).reshape(s * L, hh, d)
    return out


def _layer_norm(x):
    d = x.shape[-1]
    mu = x.mean(-1, keepdim=True)
    t = x - mu
    var = (t * t).mean(-1, keepdim=True)
    r = (var + EPS).rsqrt()
    xh = t * r
    em = gamma(d + 1) * x.abs().mean(-1, keepdim=True)
    et = em + U32 * t.abs()
    evar = (2 * t.abs() * et).mean(-1, keepdim=True) + gamma(d + 3) * var
    er = 0.5 * evar / (var + EPS) + 4 * U32
    exh = et * r + xh.abs() * er + U32 * xh.abs()
    return NS(xh=xh, exh=exh, r=r, er=er)


def _operand(n, w, b, mul, u_op, post=3):
    """post: the roundings charged after the affine (3: the product by rsqrtf(d); 0: the long kernels stage xhat w + b as it stands)"""
    lin = n.xh * w + b
    v = lin * mul
    e = (n.exh * w.abs() + 2 * U32 * ((n.xh * w).abs() + b.abs())) * mul + post * U32 * v.abs()
    return v, e * (1 + u_op) + u_op * v.abs()


def _softmax_enclosure(P, D):
    up, dn = torch.exp(D), torch.exp(-D)
    Zm, Zp = (P * dn).sum(-1, keepdim=True), (P * up).sum(-1, keepdim=True)
    hi = P * up / (Zm - P * dn + P * up)
    lo = P * dn / (Zp - P * up + P * dn)
    return torch.maximum(hi - P, P - lo)


def forward(qkv, geo, heads, d, prm, with_emb, with_hs, mode):
    """Everything the forward computes per (sequence, head) problem, with bounds: tensors [s][h][l][.]."""
    idx = token_index(geo)
    L = geo[1]
    dev = qkv.device
    qw, qb, kw, kb, emb, hs = (t.double().to(dev) for t in prm)
    x = to_problems(qkv, idx, heads, 3, d)
    nq, nk, v = _layer_norm(x[..., 0, :]), _layer_norm(x[..., 1, :]), x[..., 2, :]
    scale = d ** -0.5
    T = lambda z: z.transpose(-1, -2)
    if mode.long:             # unscaled operands; the fp32 accumulator times rsqrtf(d) (2 ulp = 4 u) and that product's rounding: 5 u
        qn, eq = _operand(nq, qw, qb, 1.0, mode.u_op, 0)
        kn, ek = _operand(nk, kw, kb, 1.0, mode.u_op, 0)
        S = (qn @ T(kn)) * scale
        eS = (qn.abs() @ T(ek) + eq @ T(kn.abs()) + eq @ T(ek) + gamma(d) * (qn.abs() @ T(kn.abs()))) * scale * (1 + 5 * U32) + 5 * U32 * S.abs()
    else:
        qn, eq = _operand(nq, qw, qb, scale, mode.u_op)
        kn, ek = _operand(nk, kw, kb, 1.0, mode.u_op)
        S = qn @ T(kn)
        eS = qn.abs() @ T(ek) + eq @ T(kn.abs()) + eq @ T(ek) + gamma(d) * (qn.abs() @ T(kn.abs()))
    bk = bucket_matrix(L, dev)
    if with_emb:
        bias = emb[bk].permute(2, 0, 1).unsqueeze(0)                        # [1][h][i][j]
        eS = eS + 2 * U32 * (S.abs() + bias.abs())
        S = S + bias
    else:
        eS = eS + 2 * U32 * S.abs()
    a = S - S.max(-1, keepdim=True).values
    P = torch.softmax(S, -1)
    encl = _softmax_enclosure(P, eS + U32 * (3 * a.abs() + 2))
    eP = encl * (1 + gamma(L + 6)) + gamma(L + 6) * P
    invL = float(np.float32(1.0) / np.float32(L))
    if with_hs:
        hv = hs.view(1, heads, 1, 1)
        A = invL + (P - invL) * hv
        eA = eP * hv.abs() + 3 * U32 * (invL + (P - invL).abs() * hv.abs())
    else:
        hv, A, eA = None, P, eP
    eAb = eA * (1 + mode.u_op) + mode.u_op * A.abs()
    O = A @ v
    if mode.long:             # the normalised row sums to one: its perturbation only sees V's deviation from a per-channel constant
        dev_v = (v - v.mean(-2, keepdim=True)).abs()
        eO = encl @ dev_v + gamma(L + 6) * ((P + encl) @ v.abs())
        if with_hs:
            eO = eO * hv.abs() + 3 * U32 * ((invL + (P - invL).abs() * hv.abs()) @ v.abs())
        eO = eO * (1 + mode.u_op) + mode.u_op * (A.abs() @ v.abs()) + gamma(L) * (A.abs() @ v.abs())
    else:
        eO = eAb @ v.abs() + gamma(32) * (A.abs() @ v.abs())
    return NS(idx=idx, L=L, heads=heads, d=d, N=qkv.shape[0], nq=nq, nk=nk, v=v, qn=qn, eq=eq, kn=kn, ek=ek, P=P, eP=eP, A=A, eAb=eAb, O=O, eO=eO,
              hv=hv, invL=invL, bk=bk, scale=scale, qw=qw, kw=kw, with_emb=with_emb, with_hs=with_hs, mode=mode)


def store(val, e, u_st, old=None, e_old=0.0):
    """A value computed with error e, optionally added to `old` (known to e_old), rounded to the output type -> (ref, bnd)."""
    if old is not None:
        val = val + old
        e = e + e_old + U32 * val.abs()
    return val, (1 + u_st) * e + u_st * val.abs()


def out_bound(F, out_scale, old=None, e_old=0.0):
    val = F.O * out_scale
    return store(val, F.eO * abs(out_scale) + U32 * val.abs(), F.mode.u_st, old, e_old)


def backward(F, dO, out_scale):
    """Gradients up to the LayerNorm outputs: dv (unstored), dqn, dkn, per-problem demb / dhscale, each with its bound."""
    if F.mode.long:
        return _backward_long(F, dO, out_scale)
    u_op, L, d, os_ = F.mode.u_op, F.L, F.d, abs(out_scale)
    T = lambda z: z.transpose(-1, -2)
    dO = dO.double()
    dP0 = (dO @ T(F.v)) * out_scale
    e_dP0 = gamma(d) * (dO.abs() @ T(F.v.abs())) * os_ + U32 * dP0.abs()
    B = NS()
    if F.with_hs:
        c = F.P - F.invL
        B.dhs = (c * dP0).sum((-1, -2))                                      # [s][h]
        B.e_dhs = (F.eP * dP0.abs() + (c.abs() + F.eP) * e_dP0).sum((-1, -2))
        B.m_dhs = (c * dP0).abs().sum((-1, -2))
        dP, e_dP = dP0 * F.hv, e_dP0 * F.hv.abs() + U32 * (dP0 * F.hv).abs()
    else:
        dP, e_dP = dP0, e_dP0
    dot = (F.P * dP).sum(-1, keepdim=True)
    e_dot = (F.eP * dP.abs() + (F.P + F.eP) * e_dP).sum(-1, keepdim=True) + gamma(L) * (F.P * dP.abs()).sum(-1, keepdim=True)
    dS = F.P * (dP - dot)
    e_dS = F.eP * (dP - dot).abs() + (F.P + F.eP) * (e_dP + e_dot) + 2 * U32 * dS.abs()
    if F.with_emb:
        flat = lambda z: torch.zeros(z.shape[0], z.shape[1], 32, dtype=z.dtype, device=z.device).index_add(2, F.bk.flatten(), z.flatten(-2))
        B.demb, B.e_demb, B.m_demb = flat(dS), flat(e_dS), flat(dS.abs())    # [s][h][32]
    e_dSb = e_dS * (1 + u_op) + u_op * dS.abs()
    B.dv = (T(F.A) @ dO) * out_scale
    B.e_dv = (T(F.eAb) @ dO.abs() + gamma(32) * (T(F.A.abs()) @ dO.abs())) * os_ + U32 * B.dv.abs()
    B.dkn = T(dS) @ F.qn
    B.e_dkn = T(e_dSb) @ (F.qn.abs() + F.eq) + T(dS.abs()) @ F.eq + gamma(32) * (T(dS.abs()) @ F.qn.abs())
    B.dqn = (dS @ F.kn) * F.scale
    B.e_dqn = (e_dSb @ (F.kn.abs() + F.ek) + dS.abs() @ F.ek + gamma(32) * (dS.abs() @ F.kn.abs())) * F.scale + 2 * U32 * B.dqn.abs()
    return B


def _backward_long(F, dO, out_scale):
    """backward() for csrc/attn_long.hip (the module docstring, "Long axes"): the same outputs."""
    u_op, L, d = F.mode.u_op, F.L, F.d
    T = lambda z: z.transpose(-1, -2)
    g = dO.double() * out_scale                                             # staged dO out_scale: fp32 product, then the operand type
    exact = out_scale == 0 or math.frexp(abs(out_scale))[0] == 0.5          # +-2^k: no rounding at either step
    e_g = 0.0 * g.abs() if exact else U32 * g.abs() * (1 + u_op) + u_op * g.abs()
    va = F.v.abs()
    dP0 = g @ T(F.v)
    e_dP0 = e_g @ T(va) + gamma(d) * (g.abs() @ T(va))
    B = NS()
    if F.with_hs:
        c = F.P - F.invL
        B.dhs = (c * dP0).sum((-1, -2))
        B.m_dhs = (c * dP0).abs().sum((-1, -2))
        B.e_dhs = (F.eP * dP0.abs() + (c.abs() + F.eP) * e_dP0).sum((-1, -2)) + 2 * U32 * B.m_dhs      # P - 1/L and the product, per term
        dP, e_dP = dP0 * F.hv, e_dP0 * F.hv.abs() + U32 * (dP0 * F.hv).abs()
    else:
        dP, e_dP = dP0, e_dP0
    dot = (F.P * dP).sum(-1, keepdim=True)
    e_dot = (F.eP * dP.abs() + (F.P + F.eP) * e_dP).sum(-1, keepdim=True) + gamma(L + 1) * (F.P * dP.abs()).sum(-1, keepdim=True)
    dS = F.P * (dP - dot)
    e_dS = F.eP * (dP - dot).abs() + (F.P + F.eP) * (e_dP + e_dot) + 2 * U32 * dS.abs()
    if F.with_emb:
        flat = lambda z: torch.zeros(z.shape[0], z.shape[1], 32, dtype=z.dtype, device=z.device).index_add(2, F.bk.flatten(), z.flatten(-2))
        B.demb, B.e_demb, B.m_demb = flat(dS), flat(e_dS), flat(dS.abs())
    e_dSb = e_dS * (1 + u_op) + u_op * dS.abs()                             # fp32 in LDS, one rounding as an operand of dqn / dkn
    B.dv = T(F.A) @ g
    B.e_dv = T(F.eAb) @ (g.abs() + e_g) + T(F.A.abs()) @ e_g + gamma(L) * (T(F.A.abs()) @ g.abs())
    post = lambda acc, e: (acc * F.scale, e * F.scale * (1 + 5 * U32) + 5 * U32 * (acc * F.scale).abs())     # acc * rsqrtf(d), as the scores
    B.dkn, B.e_dkn = post(T(dS) @ F.qn, T(e_dSb) @ (F.qn.abs() + F.eq) + T(dS.abs()) @ F.eq + gamma(L) * (T(dS.abs()) @ F.qn.abs()))
    B.dqn, B.e_dqn = post(dS @ F.kn, e_dSb @ (F.kn.abs() + F.ek) + dS.abs() @ F.ek + gamma(L) * (dS.abs() @ F.kn.abs()))
    return B


def ln_backward(n, w, d0, e_d0):
    """LayerNorm backward of rows n (from _layer_norm) for the incoming gradient d0 +- e_d0 -> dx, its bound, and per problem
    (dw, bound, sum |terms|), (db, bound, sum |terms|), summed over the rows of a problem (dim -2)."""
    xh, exh = n.xh, n.exh
    dw = ((d0 * xh).sum(-2), (e_d0 * (xh.abs() + exh) + d0.abs() * exh).sum(-2), (d0 * xh).abs().sum(-2))
    db = (d0.sum(-2), e_d0.sum(-2) if torch.is_tensor(e_d0) else e_d0, d0.abs().sum(-2))
    d = xh.shape[-1]
    g = d0 * w
    eg = e_d0 * w.abs() + U32 * g.abs()
    m1 = g.mean(-1, keepdim=True)
    em1 = eg.mean(-1, keepdim=True) + gamma(d + 1) * g.abs().mean(-1, keepdim=True)
    m2 = (g * xh).mean(-1, keepdim=True)
    em2 = (eg * (xh.abs() + exh) + g.abs() * exh).mean(-1, keepdim=True) + gamma(d + 2) * (g * xh).abs().mean(-1, keepdim=True)
    inner = g - m1 - xh * m2
    e_in = eg + em1 + exh * m2.abs() + (xh.abs() + exh) * em2 + 3 * U32 * (g.abs() + m1.abs() + (xh * m2).abs())
    dx = n.r * inner
    e_dx = n.r * (1 + n.er) * e_in + n.r * n.er * inner.abs() + U32 * dx.abs()
    return dx, e_dx, dw, db


def param_total(val, e, mag, n, reorder=None, name=None):
    """Per-problem (value, bound, sum |terms|) [s][...] -> the total over sequences and its bound for a sum of n addends in any order.
    reorder[name], if asked for, is how far two correct runs of one kernel may differ that form the same per-problem terms and only add
    them up in different orders: each sum is within gamma_n sum |terms| of the exact sum of those terms, and the kernel's terms are
    within their bounds of the reference's, so 2 gamma_n (sum |terms| + sum bounds)."""
    if reorder is not None:
        reorder[name] = 2 * gamma(n) * (mag.sum(0) + e.sum(0))
    return val.sum(0), e.sum(0) + gamma(n) * mag.sum(0)


def _param_bounds(res, F, B, dw_q, db_q, dw_k, db_k, nrows, reorder=None):
    """LayerNorm parameter sums [s][h][d] -> [d]; demb [s][h][32] -> [32][heads]; dhscale [s][h] -> [heads]."""
    if dw_q is not None:
        for name, (v, e, m) in zip(NAMES[:4], (dw_q, db_q, dw_k, db_k)):
            res[name] = param_total(v.flatten(0, 1), e.flatten(0, 1), m.flatten(0, 1), nrows, reorder, name)
    nseq = B.dhs.shape[0] if F.with_hs else (B.demb.shape[0] if F.with_emb else 0)
    if F.with_emb:
        r, b = param_total(B.demb, B.e_demb, B.m_demb, nseq * F.L * F.L, reorder, "demb")
        res["demb"] = (r.t().contiguous(), b.t().contiguous())
        if reorder is not None:
            reorder["demb"] = reorder["demb"].t().contiguous()
    if F.with_hs:
        res["dhscale"] = param_total(B.dhs, B.e_dhs, B.m_dhs, nseq * F.L * F.L, reorder, "dhscale")


def plain(qkv, dout, geo, heads, d, prm, with_emb, with_hs, out_scale, mode, old_out=None, old_dqkv=None, reorder=None):
    """bf_attn_fwd (accumulate = old_out given) and bf_attn_bwd in its plain modes (accumulate 0 / 1 = old_dqkv given).
    -> {name: (ref, bnd)}: out, dq, dk, dv as [s][h][l][d]; dqw, dqb, dkw, dkb [d]; demb [32][heads]; dhscale [heads]
    (the last two only where the kernel gets the parameter).  reorder: a dict to fill with param_total's run-to-run allowances."""
    F = forward(qkv, geo, heads, d, prm, with_emb, with_hs, mode)
    res = {"out": out_bound(F, out_scale, None if old_out is None else to_problems(old_out, F.idx, heads, 1, d)[..., 0, :])}
    if dout is None:
        return res
    B = backward(F, to_problems(dout, F.idx, heads, 1, d)[..., 0, :], out_scale)
    old = None if old_dqkv is None else to_problems(old_dqkv, F.idx, heads, 3, d)
    dxq, e_q, dw_q, db_q = ln_backward(F.nq, F.qw, B.dqn, B.e_dqn)
    dxk, e_k, dw_k, db_k = ln_backward(F.nk, F.kw, B.dkn, B.e_dkn)
    res["dq"] = store(dxq, e_q, mode.u_st, None if old is None else old[..., 0, :])
    res["dk"] = store(dxk, e_k, mode.u_st, None if old is None else old[..., 1, :])
    res["dv"] = store(B.dv, B.e_dv, mode.u_st, None if old is None else old[..., 2, :])
    _param_bounds(res, F, B, dw_q, db_q, dw_k, db_k, geo[0] * heads * geo[1], reorder)
    return res


def axial_pair(qkv, dout, frames, h, w, heads, d, prm, mode, with_emb=True, with_hs=True):
    """The W pass then the H pass accumulated (out_scale 0.5 each): forward accumulate 0 then 1 (or the one-launch kernel, which
    rounds its intermediate the same way), backward accumulate 2 then 5.  prm = (qw, qb, kw, kb, emb, hscale_x, hscale_y).
    mode: one Mode, or (the W pass's, the H pass's) when the axes run in different kernels.
    -> {name: (ref, bnd)}: out, dq, dk, dv in token layout [N][heads][d]; dqw .. dkb [d]; demb (both passes) [32][heads];
    dhscale_x, dhscale_y [heads]."""
    N = frames * h * w
    gW, gH = axial_geos(frames, h, w)
    modeW, mode = mode if isinstance(mode[0], tuple) else (mode, mode)      # (W pass's mode, H pass's mode): a short and a long axis
    assert modeW.u_st == mode.u_st
    FW = forward(qkv, gW, heads, d, list(prm[:5]) + [prm[5]], with_emb, with_hs, modeW)
    FH = forward(qkv, gH, heads, d, list(prm[:5]) + [prm[6]], with_emb, with_hs, mode)
    tokW = lambda z: to_tokens(z, FW.idx, N)
    tokH = lambda z: to_tokens(z, FH.idx, N)
    asH = lambda z: z[FH.idx.to(z.device)].permute(0, 2, 1, 3)               # token layout [N][h][d] -> the H pass's problems
    oW, bW = out_bound(FW, 0.5)                                             # the intermediate is stored (LDS tile or `out`) in the output type
    o, b = out_bound(FH, 0.5, asH(tokW(oW)), asH(tokW(bW)))
    res = {"out": (tokH(o), tokH(b))}
    if dout is None:
        return res
    BW = backward(FW, to_problems(dout, FW.idx, heads, 1, d)[..., 0, :], 0.5)
    BH = backward(FH, to_problems(dout, FH.idx, heads, 1, d)[..., 0, :], 0.5)
    u = mode.u_st
    raw = lambda v, e: (asH(tokW(v)), asH(tokW(e * (1 + u) + u * v.abs())))  # accumulate 2: one rounding of the W pass's raw gradient
    rq, e_rq = raw(BW.dqn, BW.e_dqn)
    rk, e_rk = raw(BW.dkn, BW.e_dkn)
    add = lambda a, ea, c, ec: (a + c, ea + ec + U32 * (a + c).abs())
    dxq, e_q, dw_q, db_q = ln_backward(FH.nq, FH.qw, *add(BH.dqn, BH.e_dqn, rq, e_rq))
    dxk, e_k, dw_k, db_k = ln_backward(FH.nk, FH.kw, *add(BH.dkn, BH.e_dkn, rk, e_rk))
    for name, (v, e) in (("dq", store(dxq, e_q, u)), ("dk", store(dxk, e_k, u))):
        res[name] = (tokH(v), tokH(e))
    vW, eW = store(BW.dv, BW.e_dv, u)                                        # accumulate 2 stores dV as a plain pass does; 5 adds to it
    v2, e2 = store(BH.dv, BH.e_dv, u, asH(tokW(vW)), asH(tokW(eW)))
    res["dv"] = (tokH(v2), tokH(e2))
    px, py = {}, {}
    _param_bounds(px, FW, BW, None, None, None, None, 0)
    _param_bounds(py, FH, BH, dw_q, db_q, dw_k, db_k, N * heads)
    for k in NAMES[:4]:
        res[k] = py[k]
    if with_emb:
        res["demb"] = (px["demb"][0] + py["demb"][0], px["demb"][1] + py["demb"][1] + U32 * (px["demb"][0] + py["demb"][0]).abs())
    if with_hs:
        res["dhscale_x"], res["dhscale_y"] = px["dhscale"], py["dhscale"]
    return res


def instance_norm(out, frames, S, w, b):
    """The InstanceNorm of bf_attn_axial_norm_fwd on the values the kernel stored: out [frames * S][E] (exact) ->
    {name: (ref, bnd)} for out_n [frames][S][E] (a bf16 store), mean, rstd, sc, sh [frames][E] (fp32 stores)."""
    x = out.double().view(frames, S, -1)
    w, b = w.double(), b.double()
    mu = x.mean(1)
    e_mu = gamma(S + 1) * x.abs().mean(1)
    t = x - mu[:, None]
    var = (t * t).mean(1)
    e_var = (2 * t.abs() * (e_mu[:, None] + U32 * t.abs())).mean(1) + gamma(S + 3) * var
    r = (var + EPS).rsqrt()
    er = 0.5 * e_var / (var + EPS) + 4 * U32                                # relative
    sc = r * w
    e_sc = sc.abs() * (er + U32)
    sh = b - mu * sc
    e_sh = e_mu * sc.abs() + (mu.abs() + e_mu) * e_sc + 2 * U32 * (b.abs() + (mu * sc).abs())
    on = x * sc[:, None] + sh[:, None]
    e_on = x.abs() * e_sc[:, None] + e_sh[:, None] + 2 * U32 * ((x * sc[:, None]).abs() + sh.abs()[:, None])
    f32 = lambda v, e: (v, (1 + U32) * e + U32 * v.abs())
    return {"out_n": (on, (1 + U16) * e_on + U16 * on.abs()), "mean": f32(mu, e_mu), "rstd": f32(r, r * er), "sc": f32(sc, e_sc), "sh": f32(sh, e_sh)}


def from_tokens(t, geo, heads, parts, d, part=0):
    """A kernel's token rows [N][heads * parts * d] -> the [s][h][l][d] layout of plain()'s results."""
    return to_problems(t, token_index(geo), heads, parts, d)[..., part, :]


def worst_ratio(got, ref, bnd):
    """-> (worst |got - ref| / bnd, its index, the number of elements out of bounds); inf where `got` is not finite.  Never raises."""
    got = got.detach().double().reshape(ref.shape).to(ref.device)
    diff = (got - ref).abs()
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / bnd.clamp_min(1e-300))
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    if not ratio.numel():
        return 0.0, [], 0
    idx = [int(i) for i in np.unravel_index(int(ratio.argmax()), tuple(ratio.shape))]
    return float(ratio.max()), idx, int((ratio > 1).sum())


def check(got, ref, bnd, what, names=("sequence", "head", "row", "channel")):
    """Assert |got - ref| <= bnd elementwise; -> the worst ratio |got - ref| / bnd."""
    assert torch.isfinite(bnd).all() and torch.isfinite(ref).all(), (what, "non-finite reference or bound")
    worst, idx, nbad = worst_ratio(got, ref, bnd)
    if worst > 1.0:
        got = got.detach().double().reshape(ref.shape).to(ref.device)
        where = ", ".join(f"{n}={i}" for n, i in zip(names, idx))
        raise AssertionError(f"{what}: |got - ref| exceeds the bound by {worst:.3g}x at ({where}): got {float(got[tuple(idx)]):.9g}, "
                             f"ref {float(ref[tuple(idx)]):.9g}, bound {float(bnd[tuple(idx)]):.3g}; "
                             f"{nbad} of {ref.numel()} elements out of bounds")
    return worst


def rel_l2(got, ref):
    got, ref = got.detach().double().reshape(ref.shape).to(ref.device), ref.double()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))
