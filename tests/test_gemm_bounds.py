"""CPU: pins tests/gemm_bounds.py.  An fp32 emulation of the GEMM kernels' arithmetic (prologue, bf16 operand rounding, accumulation in
two different orders, both epilogue forms, the stores) must fall inside the bound on every path; the same emulation with one defect each
of the kind these kernels can have -- a dropped K element, a mis-indexed table, a double rounding, a missing slab -- must be rejected;
and the restated GELU polynomials are pinned against the exact functions."""
import math

import pytest
import torch

from tests import gemm_bounds as GB

F32, BF16 = torch.float32, torch.bfloat16
DTS = [F32, BF16]


def _randn(*shape, scale=1.0, shift=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift


def _st(t, dt):
    return t.to(dt).double()


# ---------------------------------------------------------------------------------------------------- fp32 emulation
def fma32(x, y, z):
    """fmaf: the product of two fp32 values is exact in fp64."""
    return (x.double() * y.double() + z.double()).float()


def _poly32(coef, x):
    xc = x.clamp(-4.0, 4.0)
    u = xc * xc
    r = torch.full_like(x, GB.f32(coef[0]))
    for c in coef[1:]:
        r = r * u + GB.f32(c)
    return 0.5 + xc * r


def _erf_parts32(ax):
    t = 1.0 / (1.0 + GB.f32(GB.P_AS) * ax)
    q = torch.full_like(ax, GB.f32(GB.AS_C[0]))
    for c in GB.AS_C[1:]:
        q = GB.f32(c) + t * q
    return t * q


def gelu32(x, bf):
    if bf:
        return x * _poly32(GB.PHI_C, x)
    z = x * GB.f32(1 / math.sqrt(2.0))
    ax = z.abs()
    r = 1.0 - _erf_parts32(ax) * torch.exp(-ax * ax)
    return 0.5 * x * (1.0 + torch.copysign(r, z))


def dgelu32(x, bf):
    if bf:
        return _poly32(GB.DGELU_C, x)
    ax = x.abs() * GB.f32(1 / math.sqrt(2.0))
    e = torch.exp(-0.5 * x * x)
    cdf = 0.5 * (1.0 + torch.copysign(1.0 - _erf_parts32(ax) * e, x))
    return cdf + x * (GB.f32(1 / math.sqrt(2 * math.pi)) * e)


class Case:
    """One GEMM as the kernels see it.  A (M, K) and B (N, K) are the dense stored operands; `pro` sits on A with frame = row // rpf and
    channel = k % nch (the KC forms) or on B with frame = k // rpf and channel = column % nch (the token-reduction form)."""

    def __init__(self, dt, M=200, N=132, K=72, pro=GB.PRO_NONE, pro_on="A", sh=True, rpf=24, nch=None, bias=False, cs=False, rs=False,
                 rpg=48, aux_mode=GB.AUX_NONE, out_f32=False, gelu_out=False, atomic=False, prior=False, ld_aux=None, seed=0):
        self.dt, self.bf = dt, dt == BF16
        self.M, self.N, self.K = M, N, K
        self.A = _st(_randn(M, K, scale=1.2, shift=0.2, seed=seed), dt)
        self.B = _st(_randn(N, K, scale=K ** -0.5, seed=seed + 1), dt)
        self.pro, self.pro_on, self.rpf = pro, pro_on, rpf
        self.nch = nch or (K if pro_on == "A" else N)
        nf = -(-(M if pro_on == "A" else K) // rpf) + 1
        self.sc = _randn(nf, self.nch, scale=0.3, shift=1.0, seed=seed + 2).float()
        self.sh = _randn(nf, self.nch, scale=0.5, seed=seed + 3).float() if sh else None
        if pro_on == "A":
            self.fidx = (torch.arange(M) // rpf)[:, None].expand(M, K)
            self.cidx = (torch.arange(K) % self.nch)[None, :].expand(M, K)
        else:
            self.fidx = (torch.arange(K) // rpf)[None, :].expand(N, K)
            self.cidx = (torch.arange(N) % self.nch)[:, None].expand(N, K)
        self.bias = _randn(N, scale=0.5, seed=seed + 4).float() if bias else None
        self.cs = _randn(N, scale=0.3, shift=1.0, seed=seed + 5).float() if cs else None
        self.ch = _randn(N, scale=0.3, seed=seed + 6).float() if cs else None
        self.rpg = rpg
        self.rs = _randn(-(-M // rpg), scale=0.4, shift=1.0, seed=seed + 7).float() if rs else None
        self.aux_mode, self.out_f32, self.gelu_out, self.atomic = aux_mode, out_f32, gelu_out, atomic
        self.ld_aux = ld_aux or N
        self.auxbuf = _st(_randn(M, self.ld_aux, scale=1.5, seed=seed + 8), dt) if aux_mode else None
        self.prior = _randn(M, N, seed=seed + 9).float() if prior else None

    # ---- the bound
    def reference(self, nslices=1):
        tab = lambda t: None if t is None else t[self.fidx, self.cidx]
        v = self.A if self.pro_on == "A" else self.B
        o, eo = GB.operand(v, self.pro, tab(self.sc), tab(self.sh), self.bf)
        z = torch.zeros_like
        (a, ea), (b, eb) = ((o, eo), (self.B, z(self.B))) if self.pro_on == "A" else ((self.A, z(self.A)), (o, eo))
        n = self.K + (nslices if (self.atomic or nslices > 1) else 0) + (1 if self.prior is not None else 0)
        S, eS = GB.product(a, ea, b, eb, n)
        if self.atomic:
            return GB.accumulate(S, eS, n, self.prior)
        rs = None if self.rs is None else self.rs[torch.arange(self.M) // self.rpg]
        aux = None if self.auxbuf is None else self.auxbuf[:, :self.N]
        return GB.epilogue(S, eS, self.bf, self.bias, self.cs, self.ch, rs, aux, self.aux_mode, self.out_f32, self.gelu_out)

    # ---- the kernels' arithmetic in fp32, with optional defects
    def emulate(self, order="ktile", epi="tile", mutant=None, nslices=3, seed=0):
        bf, M, N, K = self.bf, self.M, self.N, self.K
        A, B = self.A.float(), self.B.float()
        fidx, cidx = self.fidx.clone(), self.cidx.clone()
        flat = None
        if mutant == "frame_off_by_one":            # the row that opens a frame inside a 64-row tile reads the frame before
            rows = torch.arange(M)
            hit = (rows % self.rpf == 0) & (rows % 64 != 0)
            fidx = fidx - hit[:, None].long()
        if mutant == "channel_not_wrapped":         # column tiles past the first index the table with the column itself
            cols = torch.arange(N)[:, None].expand(N, K)
            flat = (self.fidx * self.nch + torch.where(cols >= 128, cols, self.cidx)).clamp_max(self.sc.numel() - 1)

        def pro32(v, fi, ci):
            if self.pro == GB.PRO_NONE:
                return v
            t = v
            if self.pro != GB.PRO_GELU:
                sc = self.sc.flatten()[flat] if flat is not None else self.sc[fi, ci]
                t = v * sc
                if self.sh is not None:
                    t = t + (self.sh.flatten()[flat] if flat is not None else self.sh[fi, ci])
            return t if self.pro == GB.PRO_AFFINE else gelu32(t, bf)

        if self.pro_on == "A":
            A = pro32(A, fidx, cidx)
        else:
            B = pro32(B, fidx, cidx)
        if mutant == "ktail_gets_sh":
            # the K tail of the last tile is staged as pro(0) instead of 0 while the other operand's buffer holds data there (ld > K)
            pad = 64 - K % 64
            tail = pro32(torch.zeros(M, pad), fidx[:, :1].expand(M, pad), (torch.arange(K, K + pad) % self.nch)[None, :].expand(M, pad))
            A = torch.cat([A, tail], 1)
            B = torch.cat([B, _randn(N, pad, scale=K ** -0.5, seed=99).float()], 1)
            K = K + pad
        if bf:
            A, B = A.bfloat16().float(), B.bfloat16().float()
        if mutant == "drop_last_k":
            B = B.clone()
            B[128:, K - 1] = 0.0                    # column tile 1 stops one element short
        acc = torch.zeros(M, N) if self.prior is None else self.prior.clone()
        if order == "ktile":
            bk = 64 if bf else 32
            part = torch.zeros(M, N)
            for k0 in range(0, K, bk):
                part = part + A[:, k0:k0 + bk] @ B[:, k0:k0 + bk].t()
            acc = acc + part if self.prior is not None else part
        else:                                       # split-K: shuffled K, slices summed on their own, added in a shuffled order
            g = torch.Generator().manual_seed(seed)
            perm = torch.randperm(K, generator=g)
            sl = list(torch.chunk(perm, nslices))
            if mutant == "slab_omitted":
                sl = sl[:-1]
            for i in torch.randperm(len(sl), generator=g).tolist():
                acc = acc + A[:, sl[i]] @ B[:, sl[i]].t()
        if self.atomic:
            return acc
        one, zero = torch.ones(()), torch.zeros(())
        bias = self.bias if self.bias is not None else zero.expand(N)
        if mutant == "bias_shifted":
            bias = bias.clone()
            bias[128:] = torch.roll(self.bias, -1)[128:]
        cs, ch = (self.cs, self.ch) if self.cs is not None else (one.expand(N), zero.expand(N))
        if mutant == "colscale_shifted":
            cs = cs.clone()
            cs[128:] = torch.roll(self.cs, -1)[128:]
        rows = torch.arange(M)
        gi = rows // self.rpg
        if mutant == "rowscale_neighbour":
            gi = gi - ((rows % self.rpg == 0) & (rows % 64 != 0)).long()
        rs = self.rs[gi][:, None] if self.rs is not None else None
        aux = None
        if self.auxbuf is not None:
            ld = N if mutant == "aux_ldc" else self.ld_aux
            aux = self.auxbuf.float().flatten()[(rows[:, None] * ld + torch.arange(N)[None, :])]
        rnd_out = (lambda t: t.bfloat16().float()) if (bf and not self.out_f32) else (lambda t: t)
        v = acc + bias[None, :]
        scaled = self.cs is not None or self.rs is not None
        if epi == "tile":
            v = fma32(v, cs[None, :], ch[None, :])
            if rs is not None:
                v = v * rs
            if mutant == "double_rounding":
                v = v.bfloat16().float()
            if self.aux_mode == GB.AUX_ADD:
                v = v + aux
            elif self.aux_mode == GB.AUX_DGELU:
                v = v * dgelu32(aux, bf)
        else:                                       # epi_lin / epi_lin_add of the streaming and pair kernels
            r1 = rs if rs is not None else one
            if self.aux_mode == GB.AUX_ADD:
                v = fma32(fma32(v, cs[None, :], ch[None, :]), r1.expand(M, 1), aux) if scaled else v + aux
            else:
                v = fma32(v, cs[None, :], ch[None, :]) * r1 if scaled else v
                if self.aux_mode == GB.AUX_DGELU:
                    v = v * dgelu32(aux, bf)
        if self.gelu_out:
            return rnd_out(v), rnd_out(gelu32(v, bf))
        return rnd_out(v)

    def verdict(self, **kw):
        nsl = kw.get("nslices", 3) if kw.get("order") == "splitk" else 1
        ref = self.reference(nsl)
        got = self.emulate(**kw)
        if self.gelu_out:
            return max(GB.check(got[0], ref[0], ref[1], "c", ("row", "col")), GB.check(got[1], ref[2], ref[3], "gelu_out", ("row", "col")))
        return GB.check(got, ref[0], ref[1], "c", ("row", "col"))


EPIS = [
    dict(), dict(bias=True), dict(bias=True, cs=True), dict(rs=True), dict(bias=True, cs=True, rs=True),
    dict(bias=True, aux_mode=GB.AUX_ADD), dict(bias=True, cs=True, rs=True, aux_mode=GB.AUX_ADD), dict(rs=True, aux_mode=GB.AUX_ADD),
    dict(bias=True, aux_mode=GB.AUX_DGELU), dict(cs=True, aux_mode=GB.AUX_DGELU), dict(bias=True, gelu_out=True),
    dict(bias=True, cs=True, gelu_out=True), dict(bias=True, out_f32=True), dict(bias=True, aux_mode=GB.AUX_ADD, out_f32=True, ld_aux=140),
]
PROS = [dict(), dict(pro=GB.PRO_GELU), dict(pro=GB.PRO_AFFINE), dict(pro=GB.PRO_AFFINE, sh=False), dict(pro=GB.PRO_AFFINE_GELU)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("epi", ["tile", "stream"])
def test_emulated_epilogues_fall_inside_the_bound(dt, epi):
    """KC/KC and KC/XC differ in memory layout only (the dense operands are the same): every epilogue, both accumulation orders."""
    worst = 0.0
    for i, e in enumerate(EPIS):
        c = Case(dt, seed=10 * i, **e)
        worst = max(worst, c.verdict(order="ktile", epi=epi), c.verdict(order="splitk", epi=epi, seed=i))
    assert 1e-3 < worst <= 1.0, worst              # a bound a thousand times the emulation's error would catch nothing


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("pro", PROS)
def test_emulated_prologues_fall_inside_the_bound(dt, pro):
    worst = 0.0
    for kw in (dict(pro_on="A", bias=True, nch=24), dict(pro_on="A", aux_mode=GB.AUX_ADD, rpf=200),
               dict(pro_on="B", atomic=True, M=136, N=144, K=200, rpf=52, nch=48),
               dict(pro_on="B", atomic=True, prior=True, M=136, N=144, K=200, rpf=52, nch=48)):
        c = Case(dt, seed=7, **pro, **kw)
        worst = max(worst, c.verdict(order="ktile"), c.verdict(order="splitk", nslices=4, seed=3))
    assert 1e-3 < worst <= 1.0, worst


MUTANTS = [
    ("drop_last_k", dict(bias=True), {}),
    ("ktail_gets_sh", dict(pro=GB.PRO_AFFINE, nch=24), {}),
    ("ktail_gets_sh", dict(pro=GB.PRO_AFFINE_GELU, nch=24), {}),
    ("bias_shifted", dict(bias=True), {}),
    ("colscale_shifted", dict(bias=True, cs=True), {}),
    ("rowscale_neighbour", dict(rs=True), {}),
    ("rowscale_neighbour", dict(bias=True, cs=True, rs=True, aux_mode=GB.AUX_ADD), {}),
    ("frame_off_by_one", dict(pro=GB.PRO_AFFINE_GELU, nch=24), {}),
    ("frame_off_by_one", dict(pro=GB.PRO_AFFINE, sh=False, nch=24), {}),
    ("channel_not_wrapped", dict(pro=GB.PRO_AFFINE_GELU, pro_on="B", atomic=True, M=40, N=384, K=200, rpf=52, nch=96), {}),
    ("slab_omitted", dict(atomic=True, prior=True, M=136, N=72, K=200), dict(order="splitk", nslices=4)),
    ("aux_ldc", dict(bias=True, aux_mode=GB.AUX_ADD, ld_aux=140), {}),
    ("aux_ldc", dict(aux_mode=GB.AUX_DGELU, ld_aux=140), {}),
]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mutant,setup,how", MUTANTS)
def test_mutants_are_rejected(dt, mutant, setup, how):
    c = Case(dt, seed=21, **setup)
    assert c.verdict(**how) <= 1.0
    with pytest.raises(AssertionError, match="exceeds the bound"):
        c.verdict(mutant=mutant, **how)


def test_double_rounding_of_a_bf16_output_is_rejected():
    """fp32 -> bf16, then the residual added and rounded again: up to two bf16 roundings where the bound allows one."""
    c = Case(BF16, seed=5, bias=True, aux_mode=GB.AUX_ADD)
    assert c.verdict() <= 1.0
    with pytest.raises(AssertionError, match="exceeds the bound"):
        c.verdict(mutant="double_rounding")


@pytest.mark.parametrize("prior", [False, True])
def test_column_sums(prior):
    x = _st(_randn(200, 136, shift=0.2, seed=3), BF16)
    p = _randn(136, seed=4).float() if prior else None
    got = torch.zeros(136) if p is None else p.clone()
    for part in torch.chunk(x.float(), 3):
        got = got + part.sum(0)
    ref, bnd = GB.colsum(x, 200 + 3 + int(prior), p)
    assert GB.check(got, ref, bnd, "colsum", ("col",)) <= 1.0
    with pytest.raises(AssertionError):
        GB.check(got - x[-1].float(), ref, bnd, "colsum", ("col",))


# ---------------------------------------------------------------------------------------------------- the restated polynomials
def _grid():
    return torch.linspace(-8.0, 8.0, 1_600_001, dtype=torch.float64)


def test_restated_polynomials_against_the_exact_functions():
    """bf_common.h's phi_fast / gelu_fast / dgelu_fast as restated in gemm_bounds: a change of coefficients there without the
    restatement (or the other way round) moves these maxima."""
    x = _grid()
    Phi = 0.5 * (1 + torch.erf(x / math.sqrt(2.0)))
    dg = Phi + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    inner = x.abs() <= 4
    e_phi = (GB.phi_poly(x)[0] - Phi).abs()
    e_gelu = (GB.gelu_poly(x)[0] - x * Phi).abs()
    e_dg = (GB.dgelu_poly(x)[0] - dg).abs()
    for e, lim_in, lim_out in ((e_phi, 2.6e-5, 5e-5), (e_gelu, 7e-5, 4e-4), (e_dg, 7e-5, 5.6e-4)):
        assert float(e[inner].max()) < lim_in and float(e[~inner].max()) < lim_out
        assert float(e[inner].max()) > 0.5 * lim_in          # the figures are tight: the fit did not silently improve either


def test_gelu_forms_are_lipschitz_as_assumed():
    x = _grid()
    for f in (lambda t: GB.gelu_poly(t)[0], lambda t: 0.5 * t * (1 + torch.erf(t / math.sqrt(2.0)))):
        g = f(x)
        assert float(((g[1:] - g[:-1]) / (x[1:] - x[:-1])).abs().max()) < GB.L_GELU


@pytest.mark.parametrize("bf", [True, False])
def test_fp32_evaluation_of_the_gelu_forms_is_inside_its_bound(bf):
    x = _grid()[::4].float().double()
    for ref_fn, emu in ((lambda t: GB.gelu(t, torch.zeros_like(t), bf), gelu32), (lambda t: GB.dgelu(t, bf), dgelu32)):
        ref, bnd = ref_fn(x)
        err = (emu(x.float(), bf).double() - ref).abs()
        ratio = float((err / bnd).max())
        assert 1e-2 < ratio <= 1.0, ratio


def test_slice_counts_restate_the_host_code():
    assert GB.splits(200, 2, 64) == 2 and GB.splits(72, 3, 32) == 3 and GB.splits(72, 3, 64) == 2 and GB.splits(40, 5, 64) == 1
    assert GB.tokred_split(192, 192, 128) == (128, 1, True) and GB.tokred_split(192, 192, 32 * 40) == (128, 10, True)
    assert GB.tokred_split(384, 192, 32 * 7) == (224, 1, True)
    assert GB.tokred_split(128, 128, 64) == (64, 1, False) and GB.tokred_split(256, 128, 64 * 5) == (64, 5, False)
