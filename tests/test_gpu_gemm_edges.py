"""GPU: the trunk GEMM family at its edges, every output element held to the per-element bound of tests/gemm_bounds.py.

Every default instantiation of gemm.hip's tile kernel (fp32 / bf16 x the six layout / prologue forms x 64- and 128-row tiles), column
tails (N % 8 = 4, N % 4 != 0), the epilogue and prologue modes nothing else calls at kernel level (fp32 stores, rowscale, gelu_out, the
fused column sum, the GELU-only and pure-scale prologues), the prologue table's global-memory fallback, ragged k2s2 gather / scatter
geometry, the streaming kernels (both loops, every epilogue they take, contiguous and with every leading dimension 64 elements longer
than its extent inside NaN-filled buffers) and the combinations they decline, the plain frame-pair kernel, both token-reduction kernels,
and cancelling / badly scaled inputs.  Each case asserts from the profiler's report that the intended kernel ran; the last test
of the module prints the worst |got - ref| / bound of each area."""
import ctypes
import json

import pytest
import torch

from bubbleformer_amd import _lib as L
from tests import gemm_bounds as GB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
DTS = [F32, BF16]
WORST = {}                                              # area -> (worst ratio, case)


def _note(area, ratio, case):
    if ratio >= WORST.get(area, (-1.0, ""))[0]:
        WORST[area] = (ratio, case)


def _a(area, dt):
    return f"{area}, {'bf16' if dt == BF16 else 'fp32'}"


def _K():
    from bubbleformer_amd import kernels
    return kernels


def _randn(*shape, scale=1.0, shift=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift


def _st(t, dt):
    """Exact stored values of t in dtype dt (fp64)."""
    return t.to(dt).double()


def _wide(t, dt, pad, fill=float("nan")):
    """t (R, C) as a view into a device buffer (R, C + pad) whose other columns hold `fill` -> (view, buffer)."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=dt, device=DEV)
    buf[:, :t.shape[1]] = t.to(dt).to(DEV)
    return buf[:, :t.shape[1]], buf


def _untouched(buf, ncols, what):
    torch.cuda.synchronize()
    assert torch.isnan(buf[:, ncols:].float()).all(), (what, "columns beyond the extent were written")


class _Prof:
    """Profiler names of the kernels launched inside the block."""

    def __enter__(self):
        self.h = L.lib()
        self.h.bf_prof_enable(1)
        self.names = []
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 14)
        self.h.bf_prof_report(buf, len(buf))
        self.h.bf_prof_enable(0)
        if exc[0] is None:
            self.names = list(json.loads(buf.value.decode()))
        return False

    def ran(self, want, what):
        assert any(n == want or (want.endswith("*") and n.startswith(want[:-1])) for n in self.names), (what, "expected", want, "ran", self.names)


def gk(dt, ax, bx, pro, tm):
    """gemm.hip's profiler name of one instantiation."""
    bf = dt == BF16
    return f"gemm_kernel<{'bf16' if bf else 'f32'},{'xc' if ax else 'kc'},{'xc' if bx else 'kc'},pro{pro},tm{tm},w{8 if bf else 4}>"


def run(dt, M, N, K, expect, ax=False, bx=False, pro=GB.PRO_NONE, pro_on="A", sh=True, rpf=52, nch=None, bias=False, cs=False, rs=False,
        rpg=48, aux_mode=GB.AUX_NONE, out="store", gelu_out=False, splitk=1, colsum=None, prior=False, pad=0, ldc=None, ld_aux=None,
        A=None, B=None, seed=0):
    """One bf_gemm call on dense operands A (M, K), B (N, K) against the bound -> worst ratio.  ax / bx: the operand is stored
    outer-contiguous ([K][outer]).  pad: every leading dimension is that much longer than its extent, the rest of each buffer NaN.
    out: "store" | "f32" (BF_OUT_STORE_F32) | "atomic".  colsum: None | "zero" | "prior"."""
    Kn = _K()
    bf = dt == BF16
    A = _st(_randn(M, K, scale=1.2, shift=0.2, seed=seed) if A is None else A, dt)
    B = _st(_randn(N, K, scale=K ** -0.5, seed=seed + 1) if B is None else B, dt)
    what = f"{expect} {M}x{N}x{K} pro{pro}{pro_on} epi b{int(bias)}c{int(cs)}r{int(rs)}a{aux_mode}g{int(gelu_out)} {out} sk{splitk} pad{pad}"
    # ---- prologue tables: one entry per (frame, channel), all different
    o_rows = M if pro_on == "A" else N
    sc_t = sh_t = sc = shf = None
    if pro in (GB.PRO_AFFINE, GB.PRO_AFFINE_GELU):
        xc = ax if pro_on == "A" else bx
        nch = nch or (o_rows if xc else K)
        nf = -(-(K if xc else o_rows) // rpf)
        sc = _randn(nf, nch, scale=0.3, shift=1.0, seed=seed + 2).float()
        shf = _randn(nf, nch, scale=0.5, seed=seed + 3).float() if sh else None
        if xc:
            fi, ci = (torch.arange(K) // rpf)[None, :].expand(o_rows, K), (torch.arange(o_rows) % nch)[:, None].expand(o_rows, K)
        else:
            fi, ci = (torch.arange(o_rows) // rpf)[:, None].expand(o_rows, K), (torch.arange(K) % nch)[None, :].expand(o_rows, K)
        sc_t, sh_t = sc[fi, ci], (shf[fi, ci] if sh else None)
    keep = []

    def opnd(dense, xc, with_pro):
        view, buf = _wide(dense.t() if xc else dense, dt, pad)
        keep.append(buf)
        kw = dict(layout=L.BF_LAY_XC if xc else L.BF_LAY_KC)
        if with_pro and pro != GB.PRO_NONE:
            kw.update(pro=pro)
            if sc is not None:
                scd, shd = sc.to(DEV), (shf.to(DEV) if sh else None)
                keep.extend([scd, shd])
                kw.update(sc=scd, sh=shd, rows_per_frame=rpf, nch=nch)
        return Kn.operand(view, buf.shape[1], **kw)

    Aop, Bop = opnd(A, ax, pro_on == "A"), opnd(B, bx, pro_on == "B")
    # ---- epilogue
    ldc = ldc or (N + pad)
    odt = F32 if out in ("f32", "atomic") else dt
    pri = _randn(M, N, seed=seed + 9).float() if prior else (torch.zeros(M, N) if out == "atomic" else None)
    obuf = torch.full((M, ldc), float("nan"), dtype=odt, device=DEV)
    if pri is not None:
        obuf[:, :N] = pri.to(DEV)
    vec = lambda on, sd, **kw: _randn(N, seed=seed + sd, **kw).float() if on else None
    bias_v, cs_v, ch_v = vec(bias, 4, scale=0.5), vec(cs, 5, scale=0.3, shift=1.0), vec(cs, 6, scale=0.3)
    rs_v = _randn(-(-M // rpg), scale=0.4, shift=1.0, seed=seed + 7).float() if rs else None
    ekw = dict(out_mode={"store": L.BF_OUT_STORE, "f32": L.BF_OUT_STORE_F32, "atomic": L.BF_OUT_ATOMIC_F32}[out])
    dev = lambda t: None if t is None else t.to(DEV)
    for k, v in (("bias", bias_v), ("colscale", cs_v), ("colshift", ch_v), ("rowscale", rs_v)):
        if v is not None:
            ekw[k] = dev(v)
    if rs:
        ekw["rows_per_group"] = rpg
    aux = None
    if aux_mode != GB.AUX_NONE:
        aux = _st(_randn(M, N, scale=1.5, seed=seed + 8), dt)
        av, abuf = _wide(aux, dt, (ld_aux or (N + pad)) - N)
        keep.append(abuf)
        ekw.update(aux_mode=aux_mode, aux=av, ld_aux=abuf.shape[1])
    gbuf = None
    if gelu_out:
        gbuf = torch.full((M, ldc), float("nan"), dtype=odt, device=DEV)
        ekw["gelu_out"] = gbuf
    csum = cpri = None
    if colsum:
        cpri = _randn(M, seed=seed + 10).float() if colsum == "prior" else torch.zeros(M)
        csum = cpri.clone().to(DEV)
        ekw["colsum"] = csum
    with _Prof() as prof:
        Kn.gemm(dt, M, N, K, Aop, Bop, Kn.epilogue(obuf, ldc, **ekw), splitk=splitk)
    prof.ran(expect, what)
    # ---- reference
    a, ea = GB.operand(A, pro, sc_t, sh_t, bf) if pro_on == "A" else (A, torch.zeros_like(A))
    b, eb = GB.operand(B, pro, sc_t, sh_t, bf) if pro_on == "B" else (B, torch.zeros_like(B))
    ns = GB.splits(K, splitk, 64 if bf else 32)
    n = K + (ns + 1 if out == "atomic" else 0)
    S, eS = GB.product(a, ea, b, eb, n)
    worst = 0.0
    if out == "atomic":
        ref, bnd = GB.accumulate(S, eS, n, pri)
    else:
        rows = None if rs_v is None else rs_v[torch.arange(M) // rpg]
        res = GB.epilogue(S, eS, bf, bias_v, cs_v, ch_v, rows, aux, aux_mode, out == "f32", gelu_out)
        ref, bnd = res[0], res[1]
        if gelu_out:
            worst = GB.check(gbuf[:, :N], res[2], res[3], what + " gelu_out", ("row", "col"))
            _untouched(gbuf, N, what + " gelu_out")
    worst = max(worst, GB.check(obuf[:, :N], ref, bnd, what, ("row", "col")))
    _untouched(obuf, N, what)
    if colsum:
        ref, bnd = GB.colsum(A.t(), K + ns + 1, cpri)
        worst = max(worst, GB.check(csum, ref, bnd, what + " colsum", ("row",)))
    return worst


# ---------------------------------------------------------------------------------------------------- every instantiation
FORMS = [  # (name, ax, bx, pro on)
    ("kckc", False, False, None), ("kckc+proA", False, False, "A"), ("kcxc", False, True, None), ("kcxc+proA", False, True, "A"),
    ("xcxc", True, True, None), ("xcxc+proB", True, True, "B"),
]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("tm", [2, 4])
@pytest.mark.parametrize("form,ax,bx,pro_on", FORMS)
def test_every_instantiation(dt, tm, form, ax, bx, pro_on):
    """Ragged M, N and K (a multiple of the 16-byte chunk, not of BK) on 64- and 128-row tiles.  The KC forms take 128-row tiles from
    100 tiles on (25 ragged row tiles x 4 column tiles), the token-reduction form with split-K.  An outer-contiguous bf16 operand needs
    N % 8 = 0: those cases run N = 504 / 136 in place of 500 / 132.  The 64-row cases also run with every leading dimension 8 longer
    than its extent."""
    bf = dt == BF16
    n8 = bf and bx
    if ax:
        M, N, K, splitk = (136, 72, 200, 2) if tm == 4 else (200, 136, 40, 1)
    else:
        M, N, K, splitk = (3176, 504 if n8 else 500, 72, 1) if tm == 4 else (200, 136 if n8 else 132, 40, 1)
    kw = dict(pro=GB.PRO_AFFINE_GELU, pro_on=pro_on, rpf=52) if pro_on else {}
    kw.update(dict(out="atomic", prior=True, splitk=splitk) if ax else dict(bias=True, aux_mode=GB.AUX_ADD))
    r = run(dt, M, N, K, gk(dt, ax, bx, pro_on or "0", tm), ax=ax, bx=bx, pad=8 if tm == 2 else 0, seed=len(form) + tm, **kw)
    _note(_a("instantiations", dt), r, f"{dt} {form} tm{tm}")
    if not ax:      # the same product behind an fp32 store: in bf16 mode nothing hides the accumulator behind a bf16 rounding
        kw.update(aux_mode=GB.AUX_NONE, out="f32")
        r = run(dt, M, N, K, gk(dt, ax, bx, pro_on or "0", tm), ax=ax, bx=bx, seed=len(form) + tm, **kw)
        _note(_a("instantiations (fp32 store)", dt), r, f"{dt} {form} tm{tm}")


# ---------------------------------------------------------------------------------------------------- column tails
TAIL_EPIS = [dict(bias=True), dict(bias=True, aux_mode=GB.AUX_ADD), dict(aux_mode=GB.AUX_DGELU), dict(bias=True, gelu_out=True),
             dict(bias=True, out="f32"), dict(bias=True, aux_mode=GB.AUX_ADD, out="f32"), dict(aux_mode=GB.AUX_DGELU, gelu_out=True)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N,ldc", [(13, 16), (132, 132), (132, 136)])
def test_column_tails(dt, N, ldc):
    """The per-element stores, the masked aux read and the masked gelu_out store of epilogue_rows: N % 4 != 0 and N % 8 = 4."""
    for i, e in enumerate(TAIL_EPIS):
        r = run(dt, 200, N, 40, gk(dt, False, False, "0", 2), ldc=ldc, ld_aux=ldc, seed=30 + i, **e)
        _note(_a("column tails", dt), r, f"{dt} N{N} ldc{ldc} epi{i}")


# ---------------------------------------------------------------------------------------------------- tile-kernel modes
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("epi", [dict(rs=True), dict(rs=True, bias=True, cs=True), dict(rs=True, cs=True, aux_mode=GB.AUX_ADD),
                                 dict(rs=True, aux_mode=GB.AUX_DGELU), dict(rs=True, bias=True, gelu_out=True)])
def test_rowscale_groups_cross_tile_rows(dt, epi):
    r = run(dt, 200, 132, 40, gk(dt, False, False, "0", 2), rpg=48, seed=50, **epi)
    _note(_a("rowscale", dt), r, f"{dt} {sorted(epi)}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("colsum", ["zero", "prior"])
def test_fused_column_sum(dt, splitk, colsum):
    """The bias gradient of the token-reduction form: row sums of the raw A operand beside the product."""
    tm = 2 if splitk == 1 else 4
    r = run(dt, 200, 136, 328, gk(dt, True, True, "0", tm), ax=True, bx=True, out="atomic", prior=colsum == "prior", splitk=splitk, colsum=colsum,
            seed=60 + splitk)
    _note(_a("colsum (bf_gemm)", dt), r, f"{dt} splitk{splitk} {colsum}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("pro,sh", [(GB.PRO_GELU, True), (GB.PRO_AFFINE, False), (GB.PRO_AFFINE, True), (GB.PRO_AFFINE_GELU, True),
                                    (GB.PRO_AFFINE_GELU, False)])
@pytest.mark.parametrize("on", ["A", "B"])
def test_prologue_modes(dt, pro, sh, on):
    """GELU alone, the pure scale (sh = NULL) and the affine forms on a KC A operand and on an XC B operand, frames inside the tiles."""
    if on == "A":
        r = run(dt, 200, 132, 72, gk(dt, False, False, "A", 2), pro=pro, pro_on="A", sh=sh, rpf=24, bias=True, seed=70 + pro)
    else:
        r = run(dt, 200, 136, 200, gk(dt, True, True, "B", 2), ax=True, bx=True, pro=pro, pro_on="B", sh=sh, rpf=24, out="atomic", seed=80 + pro)
    _note(_a("prologue modes", dt), r, f"{dt} pro{pro} sh{int(sh)} on {on}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rpf", [8, 64])
@pytest.mark.parametrize("pro,sh", [(GB.PRO_AFFINE_GELU, True), (GB.PRO_AFFINE, False)])
def test_prologue_table_fallback(dt, rpf, pro, sh):
    """264 channels: at 8 rows per frame a 64-row tile spans 8 frames x 264 > 2048 table slots and reads sc / sh from global memory; at
    64 rows per frame the same operand takes the LDS table."""
    r = run(dt, 200, 132, 264, gk(dt, False, False, "A", 2), pro=pro, pro_on="A", sh=sh, rpf=rpf, nch=264, bias=True, seed=90 + rpf)
    _note(_a("table fallback", dt), r, f"{dt} rpf{rpf} pro{pro}")


# ---------------------------------------------------------------------------------------------------- k2s2 geometry
@pytest.mark.parametrize("dt", DTS)
def test_k2s2_gather_scatter_and_gathered_weight_gradient(dt):
    """P = 105 patches (not a multiple of 64): the patch gather on a KC A operand (plain and behind the affine + GELU prologue), the
    scatter store, and the gathered outer-contiguous B operand with its prologue at 96 channels (384 columns, the channel wraps)."""
    Kn = _K()
    bf = dt == BF16
    Fr, gh, gw = 3, 5, 7
    P = Fr * gh * gw
    z = torch.zeros_like
    for Ci, Co, pro in ((16, 24, GB.PRO_NONE), (16, 24, GB.PRO_AFFINE_GELU), (96, 40, GB.PRO_AFFINE_GELU)):
        img = _st(_randn(Fr, 2 * gh, 2 * gw, Ci, scale=1.2, shift=0.2, seed=Ci + pro), dt)
        imgd = img.to(dt).to(DEV)
        geo = dict(gw=gw, gh=gh, gc=Ci, seglen=2 * Ci, segstride=2 * gw * Ci)
        sc = _randn(Fr, Ci, scale=0.3, shift=1.0, seed=1).float()
        sh = _randn(Fr, Ci, scale=0.5, seed=2).float()
        scd, shd = sc.to(DEV), sh.to(DEV)
        pkw = dict(pro=pro, sc=scd, sh=shd, rows_per_frame=gh * gw, nch=Ci) if pro else {}
        dense = GB.patches(img, gh, gw)                                                   # (P, 4 Ci)
        fi = (torch.arange(P) // (gh * gw))[:, None].expand(P, 4 * Ci)
        ci = (torch.arange(4 * Ci) % Ci)[None, :].expand(P, 4 * Ci)
        a, ea = GB.operand(dense, pro, sc[fi, ci], sh[fi, ci], bf)
        # forward conv: out (P, Co) = gather(img) @ w^T
        w = _st(_randn(Co, 4 * Ci, scale=(4 * Ci) ** -0.5, seed=3), dt)
        bias = _randn(Co, scale=0.5, seed=4).float()
        out = torch.full((P, Co), float("nan"), dtype=dt, device=DEV)
        wd = w.to(dt).to(DEV)
        with _Prof() as prof:
            Kn.gemm(dt, P, Co, 4 * Ci, Kn.operand(imgd, Ci, **geo, **pkw), Kn.operand(wd, 4 * Ci), Kn.epilogue(out, Co, bias=bias.to(DEV)))
        prof.ran(gk(dt, False, False, "A" if pro else "0", 2), "gather")
        S, eS = GB.product(a, ea, w, z(w), 4 * Ci)
        ref, bnd = GB.epilogue(S, eS, bf, bias)
        _note(_a("k2s2", dt), GB.check(out, ref, bnd, f"gather {dt} Ci{Ci} pro{pro}", ("patch", "col")), f"{dt} gather Ci{Ci} pro{pro}")
        # weight gradient: dW (Co, 4 Ci) += dy^T @ gather(img), both outer-contiguous
        dy = _st(_randn(P, Co, seed=5), dt)
        dyd = dy.to(dt).to(DEV)
        for splitk in (1, 3):
            dw = torch.zeros(Co, 4 * Ci, dtype=F32, device=DEV)
            with _Prof() as prof:
                Kn.gemm(dt, Co, 4 * Ci, P, Kn.operand(dyd, Co, layout=L.BF_LAY_XC), Kn.operand(imgd, Ci, layout=L.BF_LAY_XC, **geo, **pkw),
                        Kn.epilogue(dw, 4 * Ci, out_mode=L.BF_OUT_ATOMIC_F32), splitk=splitk)
            ns = GB.splits(P, splitk, 64 if bf else 32)
            prof.ran(gk(dt, True, True, "B" if pro else "0", 2 if (splitk == 1 or Co <= 64) else 4), "gathered wgrad")
            S, eS = GB.product(dy.t().contiguous(), z(dy.t()), a.t().contiguous(), ea.t().contiguous(), P + ns + 1)
            ref, bnd = GB.accumulate(S, eS, P + ns + 1)
            _note(_a("k2s2", dt), GB.check(dw, ref, bnd, f"gathered wgrad {dt} Ci{Ci} pro{pro} splitk{splitk}", ("row", "col")), f"{dt} wgrad Ci{Ci} sk{splitk}")
        # transposed conv: up (Fr, 2 gh, 2 gw, Ci) scattered from x (P, Co) @ wt (4 Ci, Co)^T
        x = _st(_randn(P, Co, seed=6), dt)
        wt = _st(_randn(4 * Ci, Co, scale=Co ** -0.5, seed=7), dt)
        xd, wtd = x.to(dt).to(DEV), wt.to(dt).to(DEV)
        up = torch.full((Fr, 2 * gh, 2 * gw, Ci), float("nan"), dtype=dt, device=DEV)
        with _Prof() as prof:
            Kn.gemm(dt, P, 4 * Ci, Co, Kn.operand(xd, Co), Kn.operand(wtd, Co), Kn.epilogue(up, Ci, **geo))
        prof.ran(gk(dt, False, False, "0", 2), "scatter")
        S, eS = GB.product(x, z(x), wt, z(wt), Co)
        ref, bnd = GB.epilogue(S, eS, bf)
        torch.cuda.synchronize()
        _note(_a("k2s2", dt), GB.check(GB.patches(up.cpu(), gh, gw), ref, bnd, f"scatter {dt} Ci{Ci}", ("patch", "col")), f"{dt} scatter Ci{Ci}")


# ---------------------------------------------------------------------------------------------------- streaming kernels
STREAM_EPIS = [
    ("plain", dict(bias=True)), ("gelu2", dict(bias=True, gelu_out=True)), ("add", dict(bias=True, aux_mode=GB.AUX_ADD)),
    ("add", dict(bias=True, cs=True, aux_mode=GB.AUX_ADD)), ("add", dict(bias=True, cs=True, rs=True, aux_mode=GB.AUX_ADD)),
    ("add", dict(bias=True, rs=True, aux_mode=GB.AUX_ADD)),
    ("dgelu", dict(bias=True, aux_mode=GB.AUX_DGELU)),
]
DECLINED = [dict(rs=True, bias=True), dict(cs=True, bias=True), dict(cs=True, bias=True, gelu_out=True), dict(rs=True, aux_mode=GB.AUX_DGELU)]


@pytest.mark.parametrize("M", [256, 512])
@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("K", [128, 192, 448, 256, 320, 384])
def test_streaming(M, N, K):
    """K = 128 / 192 / 448: the ping-pong loop; 256 / 320 / 384: the weight-stationary one.  Each epilogue contiguous and as views into
    wider NaN-filled buffers; the combinations the streaming entry declines fall through to the tile kernel and are held to the same bound."""
    name = "stream_gemm" if 256 <= K <= 384 else "stream_pp"
    for i, (tag, e) in enumerate(STREAM_EPIS):
        for pad in (0, 64):
            r = run(BF16, M, N, K, f"{name}<{tag}>", pad=pad, seed=100 + i, **e)
            _note(f"streaming ({name})", r, f"{M}x{N}x{K} {tag} {sorted(e)} pad{pad}")
    for i, e in enumerate(DECLINED):
        r = run(BF16, M, N, K, "gemm_kernel<bf16,kc,kc,pro0,*", seed=120 + i, **e)
        _note("streaming fall-through", r, f"{M}x{N}x{K} {sorted(e)}")


# ---------------------------------------------------------------------------------------------------- frame-pair kernel
@pytest.mark.parametrize("M,N,K", [(288, 128, 128), (576, 256, 192)])
@pytest.mark.parametrize("add", [False, True])
def test_pair_plain(M, N, K, add):
    """out = A @ B with B outer-contiguous on 288-row tiles; lda / ldb longer than the extents.  ldc != N is not the pair kernel's: the tile
    kernel takes it."""
    e = dict(aux_mode=GB.AUX_ADD) if add else {}
    for pad in (0, 64):
        r = run(BF16, M, N, K, "gemm_pair<add>" if add else "gemm_pair<plain>", bx=True, pad=pad, ldc=N, ld_aux=N, seed=140 + pad, **e)
        _note("pair", r, f"{M}x{N}x{K} add{int(add)} pad{pad}")
    r = run(BF16, M, N, K, "gemm_kernel<bf16,kc,xc,pro0,*", bx=True, ldc=N + 64, ld_aux=N, seed=150, **e)
    _note("pair fall-through", r, f"{M}x{N}x{K} add{int(add)}")


# ---------------------------------------------------------------------------------------------------- token reduction
@pytest.mark.parametrize("Nout,Kin,M", [(192, 192, 128), (384, 192, 32 * 7), (192, 192, 32 * 40), (128, 128, 64), (256, 128, 64 * 5)])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("with_cs", [False, True])
def test_tokred(Nout, Kin, M, accumulate, with_cs):
    """out (+)= dy^T x and colsum (+)= sum(dy): the 192 x 192 ping-pong kernel (one slice; ten slices, more than the reduce kernel's eight
    in flight) and the 128 x 128 kernel, contiguous and with ldy / ldx 64 longer than the extents inside NaN-filled buffers."""
    Kn = _K()
    per, ns, pp = GB.tokred_split(Nout, Kin, M)
    dy, x = _st(_randn(M, Nout, seed=1), BF16), _st(_randn(M, Kin, shift=0.1, seed=2), BF16)
    pri = _randn(Nout, Kin, seed=3).float()
    cpri = _randn(Nout, seed=4).float()
    z = torch.zeros_like
    S, eS = GB.product(dy.t().contiguous(), z(dy.t()), x.t().contiguous(), z(x.t()), per + ns + int(accumulate))
    ref, bnd = GB.accumulate(S, eS, per + ns + int(accumulate), pri if accumulate else None)
    cref, cbnd = GB.colsum(dy, per + ns + int(accumulate), cpri if accumulate else None)
    for pad in (0, 64):
        (dyv, b1), (xv, b2) = _wide(dy, BF16, pad), _wide(x, BF16, pad)
        out = pri.clone().to(DEV) if accumulate else torch.full((Nout, Kin), float("nan"), device=DEV)
        cs = None
        if with_cs:
            cs = cpri.clone().to(DEV) if accumulate else torch.full((Nout,), float("nan"), device=DEV)
        with _Prof() as prof:
            assert Kn.gemm_tokred(dyv, xv, out, accumulate=accumulate, colsum=cs), "declined"
        what = f"tokred {Nout}x{Kin}x{M} acc{int(accumulate)} cs{int(with_cs)} pad{pad}"
        prof.ran("tokred_pp_kernel<192x192,*" if pp else "tokred_kernel<128x128,*", what)
        area = "tokred (ping-pong)" if pp else "tokred (128 x 128)"
        _note(area, GB.check(out, ref, bnd, what, ("row", "col")), what)
        if with_cs:
            _note(area + " colsum", GB.check(cs, cref, cbnd, what + " colsum", ("row",)), what)


# ---------------------------------------------------------------------------------------------------- hard inputs
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", ["cancel_tile", "cancel_stream", "spread"])
def test_hard_inputs(dt, kind):
    """Operand rows of mean 5 against weights that sum to about zero per row: the result is far smaller than sum |a||b|, which the bound
    must follow without the slack a looser checker would have.  Weights spread over 1e4 in scale across the columns, with a column scale."""
    if kind == "spread":
        B = _randn(132, 72, scale=72 ** -0.5, seed=2) * (10.0 ** torch.linspace(-2, 2, 132, dtype=torch.float64))[:, None]
        r = run(dt, 200, 132, 72, gk(dt, False, False, "0", 2), B=B, bias=True, cs=True, aux_mode=GB.AUX_ADD, seed=160)
    else:
        M, N, K = (200, 132, 72) if kind == "cancel_tile" else (256, 128, 256)
        A = _randn(M, K, scale=0.5, shift=5.0, seed=1)
        B = _randn(N, K, scale=K ** -0.5, seed=2)
        B = B - B.mean(1, keepdim=True)
        stream = kind == "cancel_stream" and dt == BF16
        r = run(dt, M, N, K, "stream_gemm<plain>" if stream else gk(dt, False, False, "0", 2), A=A, B=B, bias=not stream, seed=170)
    _note(_a("hard inputs", dt), r, f"{dt} {kind}")


# ---------------------------------------------------------------------------------------------------- report
def test_report_worst_ratios(capsys):
    """Last in the module: prints the worst |got - ref| / bound of each area the tests above reached (all are <= 1, or they failed)."""
    assert all(r <= 1.0 for r, _ in WORST.values())
    with capsys.disabled():
        print("\nworst |got - ref| / bound per area:")
        for area, (r, case) in sorted(WORST.items()):
            print(f"  {area:34s} {r:.3e}  ({case})")
