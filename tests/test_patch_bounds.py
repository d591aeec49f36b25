"""CPU: pins tests/patch_bounds.py.  An fp32 emulation of each patch-stage kernel's arithmetic (bf16 operand rounding, two accumulation
orders, the slab / partial / frame sums, the stores) must fall inside the bound at small shapes; the same emulation with one defect
each of the kind these kernels can have -- a tile under the neighbouring frame's affine, two 2x2 positions exchanged, an 8-channel group
misplaced, a dropped step, a missing slab, a rebuilt row left unrounded, a missing gelu', a slice divided by the wrong count -- must be
rejected by the per-element check; where the Frobenius thresholds of tests/test_gpu_kernels.py would have let the defect through, that
is asserted too.  The restated dispatch arithmetic is tabulated against hand-computed values."""
import pytest
import torch

from tests import norm_bounds as NB
from tests import patch_bounds as PB
from tests.test_gemm_bounds import dgelu32, fma32, gelu32
from tests.test_norm_bounds import sum32

C0 = 96


def _randn(*shape, scale=1.0, shift=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift


def _b16(t):
    """Exact stored bf16 values (fp64)."""
    return t.bfloat16().double()


def bf(t):
    return t.bfloat16().float()


def mm32(a, b, order, seed=0, bk=32):
    """a (M, K) @ b (K, N) accumulated in fp32: "blocks" = K in ascending blocks of bk (the MFMA sequence), "shuffled" = K permuted, cut
    in three, the parts added in a shuffled order."""
    a, b = a.float(), b.float()
    K = a.shape[1]
    acc = torch.zeros(a.shape[0], b.shape[1])
    if order == "blocks":
        for k0 in range(0, K, bk):
            acc = acc + a[:, k0:k0 + bk] @ b[k0:k0 + bk]
        return acc
    g = torch.Generator().manual_seed(seed)
    parts = torch.chunk(torch.randperm(K, generator=g), 3)
    for i in torch.randperm(3, generator=g).tolist():
        acc = acc + a[:, parts[i]] @ b[parts[i]]
    return acc


def _frob(got, ref):
    return PB.rel_l2(got, ref)


def _tables(Fr, C, seed, spread=0.3):
    """sc / sh (F, C): a common profile, the frames `spread` apart from one another."""
    sc = (_randn(1, C, scale=0.2, shift=1.0, seed=seed) * (1 + spread * _randn(Fr, C, seed=seed + 1))).float()
    sh = (_randn(1, C, scale=0.3, seed=seed + 2) + spread * _randn(Fr, C, seed=seed + 3)).float()
    return sc, sh


def pro32(v, sc, sh, fidx, fused=True):
    """v (rows, C) fp32, fidx (rows,) the frame of each row -> bf16(gelu_fast(v sc + sh)) as fp32."""
    s, h = sc[fidx], sh[fidx]
    t = fma32(v, s, h) if fused else v * s + h
    return bf(gelu32(t, True))


# ---------------------------------------------------------------------------------------------------- gather / scatter
class Gather:
    def __init__(self, Fr=6, gh=8, gw=32, pro=True, reb=False, spread=0.3, seed=0):
        self.Fr, self.gh, self.gw, self.pro, self.reb = Fr, gh, gw, pro or reb, reb
        self.P, self.npix = Fr * gh * gw, Fr * 4 * gh * gw
        if reb:
            self.patches = _b16(_randn(self.npix, 16, shift=0.2, seed=seed))
            self.w0 = _b16(_randn(C0, 16, scale=1 / 3, seed=seed + 1))
        else:
            self.map = _b16(_randn(Fr, 2 * gh, 2 * gw, C0, scale=1.2, shift=0.1, seed=seed))
        self.W = _b16(_randn(96, 4 * C0, scale=1 / 16, seed=seed + 2))                 # [n][(q, c)]
        self.sc, self.sh = _tables(Fr, C0, seed + 3, spread)

    def reference(self):
        shape = (self.Fr, 2 * self.gh, 2 * self.gw, C0)
        if self.reb:
            y, ey = PB.rebuilt(self.patches, self.w0)
            a, ea = PB.pro_operand(y.reshape(shape), self.sc, self.sh, ev=ey.reshape(shape))
        else:
            a, ea = PB.pro_operand(self.map, *((self.sc, self.sh) if self.pro else (None, None)))
        return PB.gather(a, ea, self.W, self.gh, self.gw)

    def emulate(self, order="blocks", mutant=None):
        Fr, gh, gw = self.Fr, self.gh, self.gw
        if self.reb:
            y = mm32(self.patches, self.w0.t(), order, bk=16)
            y = (y if mutant == "rebuilt_not_rounded" else bf(y)).reshape(Fr, 2 * gh, 2 * gw, C0)
        else:
            y = self.map.float()
        rows = PB.gather_rows(y, gh, gw)                                               # (P, 384)
        fidx = torch.arange(self.P) // (gh * gw)
        tile = torch.arange(self.P) // 32
        first = (gh * gw // 32) * 2                                                    # the tile that opens frame 2
        if mutant == "neighbour_frame":                                                # ... still under frame 1's registers
            fidx = fidx - (tile == first).long()
        if self.pro:
            rows = pro32(rows.reshape(self.P * 4, C0), self.sc, self.sh, fidx.repeat_interleave(4)).reshape(self.P, 4 * C0)
        if mutant == "swap_q":                                                         # positions (0, 1) and (1, 0) of one row exchanged
            rows = rows.clone()
            r = 32 * first + 5
            rows[r, C0:3 * C0] = torch.cat([rows[r, 2 * C0:3 * C0], rows[r, C0:2 * C0]])
        out = bf(mm32(rows, self.W.t(), order))
        if mutant == "group_misplaced":                                                # one lane's 8 columns stored 8 columns off
            out = out.clone()
            out[77, 8:24] = torch.cat([out[77, 16:24], out[77, 8:16]])
        return out

    def verdict(self, **kw):
        ref, bnd = self.reference()
        got = self.emulate(**kw)
        return PB.check(got, ref, bnd, "gather", ("row", "col")), _frob(got, ref)


@pytest.mark.parametrize("pro,reb", [(False, False), (True, False), (True, True)])
def test_emulated_gather_falls_inside_the_bound(pro, reb):
    c = Gather(Fr=2, gh=4, gw=8, pro=pro, reb=reb, seed=3)
    worst = max(c.verdict(order="blocks")[0], c.verdict(order="shuffled")[0])
    assert 1e-3 < worst <= 1.0, worst


@pytest.mark.parametrize("mutant,kw,frobenius_blind", [
    ("neighbour_frame", dict(pro=True, spread=0.01, Fr=12), True),      # frames a per cent apart, as consecutive frames of a clip are
    ("neighbour_frame", dict(reb=True, spread=0.01, Fr=12), True),
    ("swap_q", dict(pro=True), False),
    ("swap_q", dict(pro=False), False),
    ("group_misplaced", dict(pro=False), False),
    ("rebuilt_not_rounded", dict(reb=True), True),
])
def test_gather_mutants_are_rejected(mutant, kw, frobenius_blind):
    c = Gather(seed=11, **kw)
    assert c.verdict()[0] <= 1.0
    with pytest.raises(AssertionError, match="exceeds the bound"):
        c.verdict(mutant=mutant)
    if frobenius_blind:                                          # test_gather_gemm_2x2_stage: _rel(out, ref) < 4e-3
        ref, _ = c.reference()
        assert _frob(c.emulate(mutant=mutant), ref) < 4e-3


class Scatter:
    def __init__(self, Fr=3, gh=4, gw=16, pro=True, seed=0):
        self.Fr, self.gh, self.gw, self.pro = Fr, gh, gw, pro
        self.P = Fr * gh * gw
        self.a = _b16(_randn(self.P, 96, seed=seed))
        self.W = _b16(_randn(4 * C0, 96, scale=1 / 8, seed=seed + 1))                  # [(q, c)][k]
        self.sc, self.sh = _tables(Fr, 96, seed + 2)

    def reference(self):
        v = self.a.reshape(self.Fr, -1, 96)
        a, ea = PB.pro_operand(v, *((self.sc, self.sh) if self.pro else (None, None)))
        return PB.scatter(a.reshape(self.P, 96), ea.reshape(self.P, 96), self.W, self.Fr, self.gh, self.gw)

    def emulate(self, order="blocks", mutant=None):
        rows = self.a.float()
        fidx = torch.arange(self.P) // (self.gh * self.gw)
        if mutant == "neighbour_frame":
            fidx = fidx - (torch.arange(self.P) // 32 == (self.gh * self.gw // 32)).long()
        if self.pro:
            rows = pro32(rows, self.sc, self.sh, fidx)
        out = bf(mm32(rows, self.W.t(), order))
        if mutant == "swap_q":
            out = out.clone()
            out[40, C0:3 * C0] = torch.cat([out[40, 2 * C0:3 * C0], out[40, C0:2 * C0]])
        return PB.scatter_rows(out, self.Fr, self.gh, self.gw)


@pytest.mark.parametrize("pro", [False, True])
def test_emulated_scatter_and_its_slice_partials_fall_inside_the_bound(pro):
    c = Scatter(pro=pro, seed=5)
    ref, bnd = c.reference()
    names = ("frame", "y", "x", "channel")
    worst = 0.0
    for order in ("blocks", "shuffled"):
        got = c.emulate(order)
        worst = max(worst, PB.check(got, ref, bnd, "scatter", names))
        # the partials are judged against the map as stored, whatever it holds
        tiles = PB.scatter_tiles(got.double(), c.gh, c.gw)
        want = PB.slice_partials(tiles, pow2=True)
        for o2 in ("tree", "seq"):
            t1 = sum32(tiles, o2, 16)
            t2 = sum32(tiles * tiles, o2, 16)
            mu = t1 * (1.0 / 128.0)
            q = (t2 - t1 * mu).clamp_min(0.0)
            assert PB.check(mu, *want["mean"], "slice mean", ("frame", "tile", "channel")) <= 1.0
            assert PB.check(q, *want["m2"], "slice m2", ("frame", "tile", "channel")) <= 1.0
    assert 1e-3 < worst <= 1.0, worst
    for mutant in ("swap_q",) + (("neighbour_frame",) if pro else ()):
        with pytest.raises(AssertionError, match="exceeds the bound"):
            PB.check(c.emulate(mutant=mutant), ref, bnd, "scatter", names)


def _emu_partials(x, n_div, order):
    """debed_last_bwd_kernel's slice partial of x (..., n, C) fp32: sums, a / n, max(b - a mu, 0)."""
    a, b = sum32(x.double(), order, 16), sum32(x.double() * x.double(), order, 16)
    mu = a / torch.tensor(float(n_div))
    return mu, (b - a * mu).clamp_min(0.0)


@pytest.mark.parametrize("shift", [0.3, 40.0])
def test_ragged_slice_partials_and_a_wrong_count(shift):
    """Slices of 256 rows, the last one of 80; a mean 40 standard deviations off zero makes t2 - t1 mu cancel."""
    x = _b16(_randn(2, 256 + 80, C0, shift=shift, seed=2))
    want = PB.sliced(x, 256, pow2=False)
    names = ("frame", "slice", "channel")
    for order in ("tree", "seq"):
        got = [_emu_partials(x[:, s0:s0 + 256].float(), min(256, 336 - s0), order) for s0 in (0, 256)]
        mu, q = (torch.stack([g[i] for g in got], 1) for i in range(2))
        assert PB.check(mu, *want["mean"], "mean", names) <= 1.0 and PB.check(q, *want["m2"], "m2", names) <= 1.0
    bad = _emu_partials(x[:, 256:].float(), 256, "tree")                               # the ragged slice divided by the full count
    mu2, q2 = mu.clone(), q.clone()
    mu2[:, 1], q2[:, 1] = bad
    with pytest.raises(AssertionError, match="exceeds the bound"):
        PB.check(mu2, *want["mean"], "mean", names)
    with pytest.raises(AssertionError, match="exceeds the bound"):
        PB.check(q2, *want["m2"], "m2", names)
    # merged through norm_bounds.merge, the stored partials being exact inputs
    w, b = _randn(C0, scale=0.1, shift=1.0, seed=3).float(), _randn(C0, scale=0.1, seed=4).float()
    st = NB.merge(mu, q, 256, 336, w, b)
    m = x.mean(1)
    assert float(((st["mean"][0] - m).abs() / (m.abs() + 1e-3)).max()) < 1e-5


# ---------------------------------------------------------------------------------------------------- weight gradients
class Wgrad:
    def __init__(self, form, Fr=2, gh=4, gw=24, rpf=1, seed=0):
        self.form, self.Fr, self.gh, self.gw, self.rpf = form, Fr, gh, gw, rpf
        self.tpf = gh * gw // 32
        self.steps = self.tpf // rpf
        self.P = Fr * gh * gw
        if form == "rebuilt":
            self.patches = _b16(_randn(self.P * 4, 16, shift=0.2, seed=seed))
            self.w0 = _b16(_randn(C0, 16, scale=1 / 3, seed=seed + 1))
        else:
            self.fine = _b16(_randn(Fr, 2 * gh, 2 * gw, C0, seed=seed))
        self.coarse = _b16(_randn(self.P, 96, seed=seed + 2))
        self.sc, self.sh = _tables(Fr, 96, seed + 3)

    def reference(self):
        shape = (self.Fr, 2 * self.gh, 2 * self.gw, C0)
        tab = (self.sc, self.sh)
        if self.form == "rebuilt":
            y, ey = PB.rebuilt(self.patches, self.w0)
            a, ea = PB.pro_operand(y.reshape(shape), *tab, ev=ey.reshape(shape))
        else:
            a, ea = PB.pro_operand(self.fine, *(tab if self.form == "fine" else (None, None)))
        b, eb = PB.pro_operand(self.coarse.reshape(self.Fr, -1, 96), *(tab if self.form == "coarse" else (None, None)))
        return PB.wgrad(PB.gather_rows(a, self.gh, self.gw), PB.gather_rows(ea, self.gh, self.gw), b.reshape(self.P, 96), eb.reshape(self.P, 96),
                        self.steps, self.Fr * self.rpf)

    def emulate(self, mutant=None):
        Fr, gh, gw = self.Fr, self.gh, self.gw
        fidx = torch.arange(self.P) // (gh * gw)
        if self.form == "rebuilt":
            y = bf(mm32(self.patches, self.w0.t(), "blocks", bk=16)).reshape(Fr, 2 * gh, 2 * gw, C0)
        else:
            y = self.fine.float()
        A = PB.gather_rows(y, gh, gw)
        if self.form in ("fine", "rebuilt"):
            A = pro32(A.reshape(self.P * 4, C0), self.sc, self.sh, fidx.repeat_interleave(4)).reshape(self.P, 4 * C0)
        B = self.coarse.float()
        if self.form == "coarse":
            B = pro32(B, self.sc, self.sh, fidx)
        slabs = []
        for wg in range(Fr * self.rpf):
            f, run = divmod(wg, self.rpf)
            acc = torch.zeros(4 * C0, 96)
            steps = self.steps - (1 if (mutant == "drop_last_step" and wg == 1) else 0)
            for st in range(steps):
                r0 = f * gh * gw + 32 * (run * self.steps + st)
                acc = acc + A[r0:r0 + 32].t() @ B[r0:r0 + 32]
            slabs.append(acc)
        if mutant == "missing_slab":
            slabs = slabs[:-1]
        lanes = [torch.zeros(4 * C0, 96) for _ in range(4)]
        for i, s in enumerate(slabs):
            lanes[i % 4] = lanes[i % 4] + s
        return (lanes[0] + lanes[1]) + (lanes[2] + lanes[3])


@pytest.mark.parametrize("form", ["plain", "fine", "coarse", "rebuilt"])
@pytest.mark.parametrize("rpf", [1, 3])
def test_emulated_wgrad_falls_inside_the_bound_and_its_mutants_do_not(form, rpf):
    c = Wgrad(form, rpf=rpf, seed=7)
    ref, bnd = c.reference()
    worst = PB.check(c.emulate(), ref, bnd, "wgrad", ("qc", "k"))
    assert 1e-3 < worst <= 1.0, worst
    for mutant in ("missing_slab",) + (("drop_last_step",) if c.steps > 1 else ()):
        with pytest.raises(AssertionError, match="exceeds the bound"):
            PB.check(c.emulate(mutant), ref, bnd, "wgrad", ("qc", "k"))


# ---------------------------------------------------------------------------------------------------- last stage
def _last_case(Ci=64, Co=3, h=5, w=16, Fr=2, seed=0):
    P = Fr * h * w
    d = dict(Ci=Ci, Co=Co, h=h, w=w, Fr=Fr, P=P)
    d["act"] = _b16(_randn(P, Ci, seed=seed))
    d["sc"], d["sh"] = _tables(Fr, Ci, seed + 1)
    wc = torch.zeros(Ci, 16, dtype=torch.float64)
    wc[:, :4 * Co] = _randn(Ci, 4 * Co, scale=Ci ** -0.5, seed=seed + 2)
    d["wc"] = _b16(wc)
    d["y"] = _randn(Fr, Co, 2 * h, 2 * w, seed=seed + 3).float()
    d["pred"] = _randn(Fr, Co, 2 * h, 2 * w, seed=seed + 4).float()
    d["dpred"] = _randn(Fr, Co, 2 * h, 2 * w, scale=0.3, seed=seed + 5).float()
    d["coef"] = (0.5 + torch.rand(Fr, Co, generator=torch.Generator().manual_seed(seed + 6))).float()
    d["gs"] = torch.tensor([0.7])
    return d


@pytest.mark.parametrize("order", ["blocks", "shuffled"])
def test_emulated_debed_last_and_its_loss_limbs(order):
    d = _last_case(seed=4)
    Fr, Co, h, w, Ci = d["Fr"], d["Co"], d["h"], d["w"], d["Ci"]
    ref, bnd = PB.debed_last(d["act"], d["sc"], d["sh"], d["wc"], Fr, Co, h, w)
    fidx = torch.arange(d["P"]) // (h * w)
    a = pro32(d["act"].float(), d["sc"], d["sh"], fidx, fused=False)
    pred = PB.nchw(mm32(a, d["wc"], order), Fr, Co, h, w)
    worst = PB.check(pred, ref, bnd, "pred")
    assert 1e-3 < worst <= 1.0, worst
    # one fp32 partial per wave of 16 groups, then exact integer limbs
    pm, ym = PB.pm_rows(pred, h, w)[:, :4 * Co].reshape(Fr, h * w, Co, 4), PB.pm_rows(d["y"], h, w)[:, :4 * Co].reshape(Fr, h * w, Co, 4)
    num = torch.zeros(Fr, Co, dtype=torch.float64)
    den = torch.zeros(Fr, Co, dtype=torch.float64)
    for r0 in range(0, h * w, 256):
        dd = pm[:, r0:r0 + 256] - ym[:, r0:r0 + 256]
        sq, y2 = (dd * dd).sum(-1), (ym[:, r0:r0 + 256] ** 2).sum(-1)                   # four terms in fp32
        for acc, t in ((num, sq), (den, y2)):
            part = sum32(t.double(), "tree", 16).double()
            acc += torch.round(part / PB.LIMB_UNIT) * PB.LIMB_UNIT
    want = PB.loss_limbs(pred, d["y"], h, w)
    assert PB.check(num, *want["num"], "num", ("frame", "channel")) <= 1.0
    assert PB.check(den, *want["den"], "den", ("frame", "channel")) <= 1.0
    with pytest.raises(AssertionError, match="exceeds the bound"):                     # one 16-row group left out of the sum
        PB.check(num - (dd[:, :16] ** 2).sum((1, 3)).double(), *want["num"], "num", ("frame", "channel"))


@pytest.mark.parametrize("mode", ["given", "fused", "both"])
def test_emulated_dpm_modes(mode):
    d = _last_case(seed=9)
    h, w = d["h"], d["w"]
    cf = (d["coef"] * d["gs"])[:, :, None, None]
    diff = d["pred"] - d["y"]
    if mode == "given":
        got, (ref, err) = bf(PB.pm_rows(d["dpred"], h, w)), PB.dpm(h, w, dpred=d["dpred"])
        assert float(err.max()) == 0.0
    elif mode == "fused":
        got, (ref, err) = bf(PB.pm_rows(cf * diff, h, w)), PB.dpm(h, w, pred=d["pred"], y=d["y"], coef=d["coef"], gscale=d["gs"])
    else:
        got = bf(PB.pm_rows(fma32(cf.expand_as(diff), diff, d["dpred"]), h, w))
        ref, err = PB.dpm(h, w, dpred=d["dpred"], pred=d["pred"], y=d["y"], coef=d["coef"], gscale=d["gs"])
    assert PB.check(got, ref, err, "dpm", ("row", "n")) <= 1.0
    # almost every element is pinned to the bit
    assert float((err == 0).double().mean()) > 0.95
    bad = got.clone()
    bad[33, 2] = bad[33, 3]                                                            # kx exchanged inside one patch
    with pytest.raises(AssertionError, match="exceeds the bound"):
        PB.check(bad, ref, err, "dpm", ("row", "n"))
    # dact from the stored rows
    ref, bnd = PB.rank16(got, d["wc"])
    for order in ("blocks", "shuffled"):
        assert PB.check(bf(mm32(got, d["wc"].t(), order, bk=16)), ref, bnd, "dact", ("row", "channel")) <= 1.0


def _emu_bwd_norm(d, dpm_rows, ymap, mean, rstd, in_w, in_b, order, mutant=None):
    Fr, Ci = d["Fr"], d["Ci"]
    S = d["h"] * d["w"]
    y = ymap.float().reshape(Fr, S, Ci)
    a = rstd * in_w[None]
    shp = fma32(-mean, a, in_b[None].expand_as(a))
    mr = -mean * rstd
    dact = mm32(dpm_rows, d["wc"].t(), order, bk=16).reshape(Fr, S, Ci)
    z = fma32(y, a[:, None].expand_as(y), shp[:, None].expand_as(y))
    dd = dact if mutant == "no_dgelu" else dact * dgelu32(z, True)
    xh = fma32(y, rstd[:, None].expand_as(y), mr[:, None].expand_as(y))
    s1 = torch.zeros(Fr, Ci)
    s2 = torch.zeros(Fr, Ci)
    for r0 in range(0, S, 256):                                                        # a slice per wave, the slices in order
        s1 = s1 + sum32(dd[:, r0:r0 + 256].double(), "tree", 16)
        s2 = s2 + sum32(dd[:, r0:r0 + 256].double() * xh[:, r0:r0 + 256].double(), "tree", 16)
    inv = torch.tensor(1.0) / torch.tensor(float(S))
    t1, t2 = (s1 * inv)[:, None], (s2 * inv)[:, None]
    dx = bf(a[:, None] * (dd - t1 - xh * t2))
    return dx.reshape(-1, Ci), s1, s2


@pytest.mark.parametrize("h,w,shift", [(5, 16, 0.2), (17, 16, 0.2), (5, 16, 30.0)])
def test_emulated_debed_last_bwd_norm(h, w, shift):
    """One slice, two slices with a ragged second, and a map whose mean is 20 standard deviations off zero (fl(-mean rstd) dominates xh)."""
    d = _last_case(h=h, w=w, seed=13)
    Fr, Ci, P = d["Fr"], d["Ci"], d["P"]
    dpm_rows = _b16(PB.pm_rows(d["dpred"].double(), h, w))
    ymap = _b16(_randn(P, Ci, scale=1.5, shift=shift, seed=14))
    yf = ymap.reshape(Fr, h * w, Ci)
    mean, rstd = yf.mean(1).float(), ((yf.var(1, unbiased=False) + 1e-5) ** -0.5).float()
    in_w, in_b = _randn(Ci, scale=0.2, shift=1.0, seed=15).float(), _randn(Ci, scale=0.3, seed=16).float()
    want = PB.debed_last_bwd_norm(dpm_rows, d["wc"], ymap, mean, rstd, in_w, in_b, Fr)
    worst = 0.0
    for order in ("blocks", "shuffled"):
        dx, s1, s2 = _emu_bwd_norm(d, dpm_rows, ymap, mean, rstd, in_w, in_b, order)
        worst = max(worst, PB.check(dx, *want["dx"], "dx", ("row", "channel")))
        assert PB.check(s1, *want["s1"], "s1", ("frame", "channel")) <= 1.0 and PB.check(s2, *want["s2"], "s2", ("frame", "channel")) <= 1.0
    assert 1e-3 < worst <= 1.0, worst
    pg = NB.param_grads(want["s1"], want["s2"], in_w, in_b, prior=dict(dw=torch.full((Ci,), 2.0), db=torch.full((Ci,), -1.0)), gelu=True)
    assert PB.check(2.0 + s2.sum(0), *pg["dw"], "dw", ("channel",)) <= 1.0 and PB.check(-1.0 + s1.sum(0), *pg["db"], "db", ("channel",)) <= 1.0
    dx, s1, s2 = _emu_bwd_norm(d, dpm_rows, ymap, mean, rstd, in_w, in_b, "blocks", mutant="no_dgelu")
    with pytest.raises(AssertionError, match="exceeds the bound"):
        PB.check(dx, *want["dx"], "dx", ("row", "channel"))
    with pytest.raises(AssertionError, match="exceeds the bound"):
        PB.check(s1, *want["s1"], "s1", ("frame", "channel"))


# ---------------------------------------------------------------------------------------------------- embed tail
def _tail_case(Fr=3, gh1=8, gw1=16, C1=96, seed=0, y_shift=0.3):
    S1, S0 = gh1 * gw1, 4 * gh1 * gw1
    d = dict(Fr=Fr, gh1=gh1, gw1=gw1, C1=C1, S0=S0)
    d["patches"] = _b16(_randn(Fr * S0, 16, shift=y_shift, seed=seed))
    d["w0"] = _b16(_randn(C0, 16, scale=1 / 3, seed=seed + 1))
    d["w1"] = _b16(_randn(C1, 4 * C0, scale=1 / 8, seed=seed + 2))
    d["dy1"] = _b16(_randn(Fr * S1, C1, seed=seed + 3))
    d["in_w"] = _randn(C0, scale=0.2, shift=1.0, seed=seed + 4).float()
    in_b = _randn(C0, scale=0.3, seed=seed + 5).float()
    d["y0"] = _b16(d["patches"] @ d["w0"].t())
    yf = d["y0"].reshape(Fr, S0, C0)
    d["mean"], d["rstd"] = yf.mean(1).float(), ((yf.var(1, unbiased=False) + 1e-5) ** -0.5).float()
    d["sc"] = d["rstd"] * d["in_w"][None]
    d["sh"] = in_b[None] - d["mean"] * d["sc"]
    return d


def _emu_tail(d, order, ymap, mutant=None):
    Fr, gh1, gw1, S0 = d["Fr"], d["gh1"], d["gw1"], d["S0"]
    pt = d["patches"].float().reshape(Fr, S0, 16)
    y = (d["y0"].float() if ymap else bf(mm32(d["patches"], d["w0"].t(), order, bk=16))).reshape(Fr, S0, C0)
    dact = PB.scatter_rows(mm32(d["dy1"], d["w1"], order), Fr, gh1, gw1).reshape(Fr, S0, C0)
    ex = lambda t: t[:, None].expand_as(y)
    z = fma32(y, ex(d["sc"]), ex(d["sh"]))
    dd = dact if mutant == "no_dgelu" else dact * dgelu32(z, True)
    xh = fma32(y, ex(d["rstd"]), ex(-d["mean"] * d["rstd"]))
    s1 = sum32(dd.double(), "tree", 16)
    s2 = sum32(dd.double() * xh.double(), "tree", 16)
    d16 = bf(dd)
    G = torch.stack([mm32(d16[f].t(), pt[f], order) for f in range(Fr)])               # (F, C0, 16)
    M2 = torch.stack([mm32(pt[f].t(), pt[f], order) for f in range(Fr)])
    P1 = sum32(pt.double(), "seq", 16)
    px = torch.zeros(Fr, C0, 16)
    w0 = d["w0"].float()
    for j in range(16):
        px = fma32(w0[None, :, j, None].expand_as(px), M2[:, None, j, :].expand_as(px), px)
    rs, mu = d["rstd"][:, :, None], d["mean"][:, :, None]
    px = rs * (px - mu * P1[:, None])
    inv = torch.tensor(1.0) / torch.tensor(float(S0))
    slab = rs * d["in_w"][None, :, None] * (G - s1[:, :, None] * inv * P1[:, None] - s2[:, :, None] * inv * px)
    dw = torch.zeros(C0, 16)
    for f in range(Fr):
        dw = dw + slab[f]
    return dw, 2.0 + s2.sum(0), -1.0 + s1.sum(0)


@pytest.mark.parametrize("ymap", [True, False])
@pytest.mark.parametrize("C1,y_shift", [(96, 0.3), (192, 0.3), (96, 6.0)])
def test_emulated_embed_tail(ymap, C1, y_shift):
    """Stored and rebuilt rows; patch rows of mean 6 make W0 M2 and mean P1 (and G, t1 P1, t2 PX) cancel."""
    d = _tail_case(C1=C1, seed=21, y_shift=y_shift)
    pri = dict(prior_w=torch.full((C0,), 2.0), prior_b=torch.full((C0,), -1.0))
    want = PB.embed_tail(d["dy1"], d["w1"], d["patches"], d["w0"], d["sc"], d["sh"], d["mean"], d["rstd"], d["in_w"], d["Fr"], d["gh1"], d["gw1"],
                         y0=d["y0"] if ymap else None, **pri)
    worst = 0.0
    for order in ("blocks", "shuffled"):
        dw, diw, dib = _emu_tail(d, order, ymap)
        worst = max(worst, PB.check(dw, *want["dwprep"], "dwprep", ("channel", "k")))
        assert PB.check(diw, *want["d_in_w"], "d_in_w", ("channel",)) <= 1.0 and PB.check(dib, *want["d_in_b"], "d_in_b", ("channel",)) <= 1.0
    assert 1e-3 < worst <= 1.0, worst
    dw, diw, dib = _emu_tail(d, "blocks", ymap, mutant="no_dgelu")
    with pytest.raises(AssertionError, match="exceeds the bound"):
        PB.check(dw, *want["dwprep"], "dwprep", ("channel", "k"))
    with pytest.raises(AssertionError, match="exceeds the bound"):
        PB.check(dib, *want["d_in_b"], "d_in_b", ("channel",))


# ---------------------------------------------------------------------------------------------------- dispatch arithmetic
def test_wave_split_restates_the_launchers():
    # 256 CUs: a full grid is 2 * 256 * 4 = 2048 waves
    assert PB.wave_split(1, 256) == (1, 1, 1) and PB.wave_split(504, 256) == (1, 504, 126) and PB.wave_split(2048, 256) == (1, 2048, 512)
    assert PB.wave_split(2049, 256) == (2, 1025, 257) and PB.wave_split(2055, 256) == (2, 1028, 257) and PB.wave_split(4105, 256) == (3, 1369, 343)
    assert PB.wave_split(10, 8) == (1, 10, 3) and PB.wave_split(65, 8) == (2, 33, 9)
    runs = PB.wave_runs(2055, 256)                       # 1028 waves: 1027 runs of two tiles and one of one
    assert len(runs) == 1028 and runs[0] == (0, 1) and runs[1] == (1, 3) and runs[-1] == (2053, 2055)
    assert sum(e - b for b, e in runs) == 2055 and all(runs[i][1] == runs[i + 1][0] for i in range(1027))
    assert sorted({e - b for b, e in runs}) == [1, 2]
    assert any(e - b == 2 and b // 5 != (e - 1) // 5 for b, e in runs)                 # five tiles per frame: runs straddle frames
    runs = PB.wave_runs(10, 8)                           # 3 workgroups = 12 waves for 10 tiles: two of them idle
    assert [e - b for b, e in runs] == [0, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1]


def test_wgrad_runs_restate_the_host_code():
    assert PB.wgrad_runs(3, 1) == 1 and PB.wgrad_runs(7, 72) == 72 and PB.wgrad_runs(8, 72) == 36 and PB.wgrad_runs(2, 12) == 12
    assert PB.wgrad_runs(2, 12, 2 * PB.SLAB * 4) == 4 and PB.wgrad_runs(2, 12, 2 * PB.SLAB * 5) == 4 and PB.wgrad_runs(2, 12, 2 * PB.SLAB) == 1
    assert PB.wgrad_runs(2, 12, 2 * PB.SLAB - 1) == 0
    assert PB.wgrad_runs(130, 5) == 1 and PB.wgrad_runs(102, 5) == 5 and PB.wgrad_runs(103, 5) == 1      # the F * r <= 512 cap
    assert PB.wgrad_ws_floats(7, 48, 48) == 7 * 72 * 36864 and PB.wgrad_ws_floats(2, 3, 5) == 0


def test_tail_plan_restates_the_host_code():
    want = {1: (1, 1), 2: (2, 1), 3: (3, 1), 4: (4, 1), 5: (5, 1), 6: (6, 1), 7: (1, 7), 8: (4, 2), 9: (3, 3), 18: (6, 3)}
    for n, plan in want.items():
        assert PB.tail_plan(128 * n) == plan
    assert PB.tail_plan(96) is None and PB.tail_plan(0) is None
    assert PB.TAIL_NPART == 2000
    assert PB.tail_ws_floats(3, 8, 16) == 3 * 1 * 4 * 2000 + 3 * 96 * 16 + 3 * 192
    assert PB.tail_ws_floats(2, 7, 128) == 2 * 7 * 4 * 2000 + 2 * 96 * 16 + 2 * 192


def test_last_stage_split_restates_the_kernels():
    s = PB.dl_split(1, 16)
    assert (s["groups"], s["waves"], s["wgs"], s["slices"], s["last_rows"]) == (1, 1, 1, 1, 16)
    for groups, waves, wgs, last in ((15, 1, 1, 240), (16, 1, 1, 256), (17, 2, 1, 16), (63, 4, 1, 240), (64, 4, 1, 256), (65, 5, 2, 16), (129, 9, 3, 16)):
        s = PB.dl_split(groups, 16)
        assert (s["groups"], s["waves"], s["wgs"], s["slices"], s["last_rows"]) == (groups, waves, wgs, waves, last)
    assert PB.LIMB_UNIT == 2.0 ** -112
