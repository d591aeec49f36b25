"""Per-element error bounds for the whole-frame kernels that fuse a projection with the InstanceNorm beside it: csrc/gemm_frame.hip
(gemm_inbwd_frames_kernel, gemm_pair_kernel<0 | 2 | 3 | 4>) and csrc/frame_fwd.hip (frame_res_kernel, frame_ring_kernel).

Given the exact (fp64) values a kernel reads, each function returns the fp64 reference `ref` and an elementwise bound `bnd` such that a
correct kernel satisfies |got - ref| <= bnd everywhere.  `check`, `gamma`, `rnd16`, `U32`, `U16` are conv_bounds'; `product`, `epilogue`,
`gelu`, `O2` gemm_bounds'; `in_stats`, `affine_apply`, `in_bwd`, `param_grads` norm_bounds'.  u = 2^-24.  Every constant is derived here from
the kernels' rounding points; none is fitted to GPU output.  All operands are bf16 (the entry points refuse fp32).

Fused InstanceNorm backward (`inbwd`; gemm_inbwd_frames_kernel, pair_body<0>).
  dy is the fp32 MFMA accumulator, never rounded to bf16: |dy~ - dy| <= gamma_K sum |a||b| (gemm_bounds.product, n = K; bf16 products are
    exact in fp32).  With `fscale` the accumulator is multiplied once by fscale[frame / fdiv]: v = fl(dy~ f), e_v = |f| e_dy + u |v|.  A zero
    factor makes v = +-0 and e_v = 0: every later term of the bound vanishes, s1 = s2 = +-0 and the kernel's t is +-0 before `add`.
  xh = fl(fl(x - mu) rs): 2u |xh| (norm_bounds.in_bwd's e_xh), mean / rstd the GIVEN fp32 statistics.
  s1 += v, s2 += v * xh.  The pair kernel: 9 register adds and the 16-lane row16_sum per frame column; the one-frame kernel: 3 adds, the
    16-lane sum and 3 LDS partials added in order; the `whole` form (one 288-token frame per tile): the pair kernel's sums of the two
    halves, exchanged through LDS, and one more add.  Each is a sum of the frame's S terms in SOME order: gamma_S with S = 144 or 288 (S + 1
    for s2: the product's rounding, charged unfused), the figure norm_bounds.in_bwd takes from x's shape.  e_v is carried into both.
  t = rs * ww * (v - (s1 + xh * s2) * invS): xh s2, + s1, * invS, v - . are four roundings and invS = fl(1 / S) is a constant with one
    relative rounding of its own (1 / 144 and 1 / 288 are not fp32 numbers): 5u on the magnitude sum |v| + |s1| / S + |xh s2| / S plus the
    carried error, not on the cancelled result -- in_bwd's E_I = E + 5u (Mg + E).  rs * ww and the outer product: gamma_2 (no g).  + add:
    u (|t| + |add| + e).  The bf16 store.  So inbwd() IS norm_bounds.in_bwd on (v, e_v); nothing is added to its constants.
  ws[(f N + n) 2 ..] = {s1, s2} in fp32 as summed: in_bwd's per-(frame, column) bounds, entry by entry.
Chain (`chain`; pair_body<2>).  The kernel reads its own stored `out` rows back (bf16: exact inputs) and applies a second backward with
  statistics (cmean, crstd) of cz: k3 = fl(fl(cw cg) r3), cdz = fl(k3 fl(dd - fl(fl(c1 + fl(xh c2)) fl(1 / 144)))).  The same five roundings
  inside, three relative roundings outside (gamma_3; gamma_2 without cg): in_bwd with g = cg[frame / cgdiv] expanded per frame, dy = the stored
  rows, e_dy = 0.  cws = {c1, c2} as ws.
Forward twin (`fwd_out`, `fwd_norm`; pair_body<3 | 4>).
  out: epi_lin / epi_lin_add of gemm_common.h on the accumulator -- gemm_bounds.epilogue with rs = fscale[frame / fdiv] per row (applied in the
    scaled form only: the entry refuses fscale without colscale) and AUX_ADD for `add`.
  n1 on the kernel's own stored `out`, n2 on the stored n1.out (or `out` without n1): frame_stats() is mean = fl(sum / 144) in the
    summation order of in_stats_kernel, q = sum fmaf(d, d, .) with d = fl(x - mean), r = rsqrtf(fl(q / 144) + eps), s0 = fl(r w),
    t0 = fmaf(-m, s0, b), with g: s0 = fl(s0 g), t0 = fmaf(t0, g, 0) = fl(t0 g).  norm_bounds.in_stats charges exactly these, each fma as
    if unfused (one rounding more than performed), the division by S, and g without gb: its four tables bound mean / rstd / sc / sh.
    The normalised rows are fmaf(y, sc, sh) (+ resid) of the STORED fp32 sc / sh, which the same lanes hold: norm_bounds.affine_apply on
    the kernel's own tables (checked above) and the stored rows.
bf_frame_linear (`frame_linear`; frame_res_kernel, frame_ring_kernel, frame_epilogue).  Nothing but `out` and `out_n` is stored, so the
  statistics' bounds are carried instead of being checked on their own:
  norm in front (resident form): frame_stats<8> + fmaf(x, aa, ss) + 0 rounded to bf16 in LDS.  in_stats gives (sc, e_sc), (sh, e_sh);
    t = x sc + sh is within |x| e_sc + e_sh + u |t| (carried, times O2); the bf16 operand is conv_bounds.operand's interval rounding
    [rnd(t - e), rnd(t + e)] around rnd(t) and enters the product through gemm_bounds.product.
  epilogue without en_*: v = acc + bias; fmaf(v, cs, ch); + resid; gelu_fast; store -- gemm_bounds.epilogue (AUX_ADD, want_gelu: bf16
    kernels use the polynomial form, gemm_bounds.gelu).
  en_* (out = resid + IN(z) en_w en_g, z = bf16(acc + bias) never stored): z is the interval rounding of acc + bias within e_z; its
    statistics are in_stats with the carried input error ex = e_z (norm_bounds: the mean moves by mean(ex), sqrt(M2) by at most ||ex||_2);
    out = fmaf(z, sc, sh) + resid with every factor carried: |z| e_sc + |sc| e_z + e_z e_sc + e_sh, u |t|, u (|t| + |resid|), store.
  next_* (out_n = IN(out) next_w + next_b): in_stats of the kernel's own stored `out` (exact input), then the same carried apply with
    e_z = 0 and no residual.

Dispatch (restated host code; the GPU cases assert the profiler name each gives).  bf_gemm_inbwd_frames: S in {144, 288}, M % S = 0,
N % 128 = 0, K % 64 = 0, K >= 64, lda / ldb % 8 = 0, bf16, else refused; the pair kernel (`gemm_pair<inbwd>`) where M % 288 = 0 -- an even
number of 144-token frames or any number of 288-token ones -- else the one-frame kernel (`gemm_inbwd_frames<bf16>`, S = 144 only).  The chain
(`gemm_pair<inbwd,chain>`) needs the pair kernel with S = 144.  bf_gemm_fwd_frames: S = 144, M % 288 = 0, K >= 128; `gemm_pair<fwd[,norm][,chain]>`.
bf_frame_linear: resident at K = 384 without en_*, else the ring (which takes no norm in front); column block = the widest of 96 / 64 with
N % bn = 0 and frames * N / bn >= 180, else 32; ring slots NS = 5 / 6 / 7 for bn = 96 / 64 / 32.
"""
import torch

from tests.conv_bounds import U16, U32, check, gamma, rnd16  # noqa: F401  (re-exported to the tests)
from tests import gemm_bounds as GB
from tests import norm_bounds as NB

O2 = GB.O2
FS = 144


# ---------------------------------------------------------------------------------------------------- restated host code
def inbwd_path(M, N, K, S, bf16=True, chain=False):
    """Profiler name of the kernel bf_gemm_inbwd_frames[_chain] runs, None where the entry refuses the shape."""
    if not bf16 or S not in (144, 288) or M <= 0 or M % S or N <= 0 or N % 128 or K < 64 or K % 64:
        return None
    if M % 288 == 0:
        if chain:
            return None if S == 288 else "gemm_pair<inbwd,chain>"
        return "gemm_pair<inbwd>"
    return None if chain or S != 144 else "gemm_inbwd_frames<bf16>"


def inbwd_grid(M, N, S):
    return (M // 288 if M % 288 == 0 else M // S) * (N // 128)


def fwd_path(M, N, K, S, n1, n2, bf16=True):
    if not bf16 or S != 144 or M <= 0 or M % 288 or N <= 0 or N % 128 or K < 128 or K % 64:
        return None
    return "gemm_pair<fwd" + (",norm" if n1 else "") + (",chain" if n2 else "") + ">"


def frame_ntc(frames, N):
    for c in (3, 2):
        if N % (32 * c) == 0 and frames * (N // (32 * c)) >= 180:
            return c
    return 1


RING_NS = {3: 5, 2: 6, 1: 7}


def frame_linear_path(frames, N, K, norm=False, en=False):
    """Profiler name of bf_frame_linear's kernel, None where it refuses."""
    if N % 32 or K % 64 or K < 128 or frames < 1:
        return None
    res = K == 384 and not en
    if not res and norm:
        return None
    return "frame_linear<%s,bn%d%s>" % ("res" if res else "ring", 32 * frame_ntc(frames, N), ",norm" if norm else ",in" if en else "")


# ---------------------------------------------------------------------------------------------------- backward
def _rows(f, Fr, S):
    """Per-frame factors f (F,) -> per row (F S, 1)."""
    return f.double().repeat_interleave(S)[:, None]


def inbwd(A, B, x, mean, rstd, w, S, add=None, fscale=None):
    """A (M, K), B (K, N) exact bf16 values; x / add (M, N); mean / rstd (F, N) fp32; w (N,); fscale (F,) already expanded per frame
    (fscale[f // fdiv]) -> {"dx": (ref, bnd) (M, N), "ws": (ref, bnd) (F, N, 2)}."""
    A, B = A.double(), B.double()
    M, N = A.shape[0], B.shape[1]
    Fr = M // S
    dy, e = GB.product(A, torch.zeros_like(A), B.t(), torch.zeros_like(B.t()), A.shape[1])
    if fscale is not None:
        f = _rows(fscale, Fr, S)
        dy = dy * f
        e = e * f.abs() + U32 * dy.abs()
    v3 = lambda t: None if t is None else t.double().reshape(Fr, S, N)
    r = NB.in_bwd(v3(dy), v3(x), mean, rstd, w, torch.zeros_like(w), add=v3(add), bf16=True, e_dy=v3(e))
    ref, bnd = r["dx"]
    ws = torch.stack([r["s1"][0], r["s2"][0]], -1), torch.stack([r["s1"][1], r["s2"][1]], -1)
    return dict(dx=(ref.reshape(M, N), bnd.reshape(M, N)), ws=ws)


def summed(ws, w):
    """The (ref, bnd) pair of `ws` / `cws` summed over frames as the parameter-gradient reduction sums it (no post scale, zero priors)
    -> norm_bounds.param_grads' dict; "dw" = sum_f s2 and "db" = sum_f s1, each (ref, bnd) of shape (N,).  CPU tensors."""
    (r, e) = ws
    return NB.param_grads((r[..., 0], e[..., 0]), (r[..., 1], e[..., 1]), w, torch.zeros_like(w))


def chain(out, cz, cmean, crstd, cw, cg=None):
    """out (M, N): the kernel's own stored rows; cz (M, N); cmean / crstd (F, N); cw (N,); cg (F, N) already expanded per frame
    -> {"cdz": (ref, bnd) (M, N), "cws": (ref, bnd) (F, N, 2)}.  144-token frames."""
    M, N = out.shape
    Fr = M // FS
    v3 = lambda t: t.double().reshape(Fr, FS, N)
    r = NB.in_bwd(v3(out), v3(cz), cmean, crstd, cw, torch.zeros_like(cw), g=cg, bf16=True)
    ref, bnd = r["dx"]
    ws = torch.stack([r["s1"][0], r["s2"][0]], -1), torch.stack([r["s1"][1], r["s2"][1]], -1)
    return dict(cdz=(ref.reshape(M, N), bnd.reshape(M, N)), cws=ws)


# ---------------------------------------------------------------------------------------------------- forward twin
def fwd_out(A, Bt, bias=None, cs=None, ch=None, fscale=None, add=None):
    """A (M, K), Bt (K, N) exact bf16 values; fscale (F,) expanded per frame (only with cs / ch) -> (ref, bnd) of `out` (M, N)."""
    A, Bt = A.double(), Bt.double()
    S, eS = GB.product(A, torch.zeros_like(A), Bt.t(), torch.zeros_like(Bt.t()), A.shape[1])
    rs = None
    if fscale is not None:
        assert cs is not None
        rs = fscale.double().repeat_interleave(FS)
    return GB.epilogue(S, eS, True, bias, cs, ch, rs, None if add is None else add.double(), GB.AUX_ADD if add is not None else GB.AUX_NONE)


def fwd_norm(rows, w, b, g=None):
    """rows (M, N): the stored tensor the norm reads; g (F, N) expanded per frame -> in_stats' dict of (ref, bnd), each (F, N)."""
    return NB.in_stats(rows.double().reshape(-1, FS, rows.shape[1]), w, b, g)


def fwd_apply(rows, sc, sh, resid=None):
    """The normalised rows from the kernel's own stored fp32 sc / sh (F, N) -> (ref, bnd) (M, N)."""
    M, N = rows.shape
    v3 = lambda t: None if t is None else t.double().reshape(-1, FS, N)
    ref, bnd = NB.affine_apply(v3(rows), sc, sh, v3(resid), bf16=True)
    return ref.reshape(M, N), bnd.reshape(M, N)


# ---------------------------------------------------------------------------------------------------- bf_frame_linear
def carried_apply(z, e_z, st, resid=None, store=True):
    """fmaf(z, sc, sh) (+ resid) where z (F, S, C) is known to within e_z and sc / sh only through in_stats' bounds `st`
    -> (t, bound) before (store = False) or after the bf16 store."""
    (sc, e_sc), (sh, e_sh) = st["sc"], st["sh"]
    sc, e_sc, sh, e_sh = (t[:, None] for t in (sc, e_sc, sh, e_sh))
    t = z * sc + sh
    e = O2 * (z.abs() * e_sc + sc.abs() * e_z + e_z * e_sc + e_sh) + U32 * ((z * sc).abs() + sh.abs())
    if resid is not None:
        e = e + U32 * (t.abs() + e + resid.abs())
        t = t + resid
    if not store:
        return t, e
    return t, (1 + U16) * e + U16 * t.abs()


def _interval16(t, e):
    r = rnd16(t)
    return r, torch.maximum(rnd16(t + e) - r, r - rnd16(t - e))


def frame_linear(A, W, norm=None, bias=None, cs=None, ch=None, resid=None, gelu=False, en=None):
    """A (frames 144, K), W (N, K) exact bf16 values; norm = (w, b) (K,) in front; en = (w, b, g) (N,) behind (needs resid)
    -> (ref, bnd) of `out` (M, N)."""
    A, W = A.double(), W.double()
    M, K = A.shape
    N = W.shape[0]
    Fr = M // FS
    ea = torch.zeros_like(A)
    if norm is not None:
        a3 = A.reshape(Fr, FS, K)
        t, e = carried_apply(a3, torch.zeros_like(a3), NB.in_stats(a3, norm[0], norm[1]), store=False)
        A, ea = _interval16(t.reshape(M, K), e.reshape(M, K))
    S, eS = GB.product(A, ea, W, torch.zeros_like(W), K)
    if en is None:
        aux = None if resid is None else resid.double()
        r = GB.epilogue(S, eS, True, bias, cs, ch, None, aux, GB.AUX_ADD if aux is not None else GB.AUX_NONE, want_gelu=gelu)
        return (r[2], r[3]) if gelu else (r[0], r[1])
    z, e_z = S, eS
    if bias is not None:
        e_z = (e_z + U32 * (z.abs() + bias.double().abs()[None])) * O2
        z = z + bias.double()[None]
    z, e_z = _interval16(z, e_z)
    z3, e3 = z.reshape(Fr, FS, N), e_z.reshape(Fr, FS, N)
    g = en[2].double()[None].expand(Fr, N)
    t, b = carried_apply(z3, e3, NB.in_stats(z3, en[0], en[1], g, ex=e3), resid.double().reshape(Fr, FS, N))
    return t.reshape(M, N), b.reshape(M, N)


def frame_linear_next(out, xw, xb):
    """out (M, N): the kernel's own stored rows -> (ref, bnd) of out_n = IN(out) xw + xb."""
    M, N = out.shape
    o3 = out.double().reshape(-1, FS, N)
    t, b = carried_apply(o3, torch.zeros_like(o3), NB.in_stats(o3, xw, xb))
    return t.reshape(M, N), b.reshape(M, N)
