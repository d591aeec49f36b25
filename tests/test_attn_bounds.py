"""CPU: the per-element attention checker (tests/attn_bounds.py) pinned without a GPU.  A torch emulation of attn_mfma.hip's arithmetic
(fp32, with bf16 rounding exactly where the kernel rounds: the Qn d^-1/2 / Kn operands, the rescaled A, the A^T / dS^T tiles, the raw q / k
gradient between the axial passes, every store) passes it at a spread of shapes, at a peaked and at a large-offset input; ten emulated
kernel bugs fail it.  For every mutant the test also prints what the whole-tensor criteria of
test_gpu_kernels.py::test_attention_mfma_matches_generic_and_fp32 would have said (run with -s to see the table).  The second half does
the same for csrc/attn_long.hip (33 <= L <= 128) and the modes LONG_BF16 / LONG_FP32."""
import numpy as np
import pytest
import torch

from tests import attn_bounds as AB

F32 = torch.float32
OLD_LIMITS = {"out": 1.5e-2, "dq": 3e-2, "dk": 3e-2, "dv": 3e-2, "dqw": 5e-2, "dqb": 5e-2, "dkw": 5e-2, "dkb": 1e-2, "demb": 5e-2, "dhscale": 1e-1}


def bf(t):
    return t.bfloat16().float()


def make(N, heads, d, seed, wscale=0.2, embscale=0.5, qk_gain=1.0, offset=0.0, spread=1.5, axial=False):
    """Stored inputs: qkv / dout hold bf16 values (as doubles), the parameters fp32 values."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    E = heads * d
    qkv = r(N, 3 * E) * spread
    if offset:
        qkv = qkv + offset * (1 + r(N, 3 * heads, 1).abs()).expand(N, 3 * heads, d).reshape(N, 3 * E)      # a large offset common to a row
    prm = [qk_gain * (1 + wscale * r(d)), wscale * r(d), qk_gain * (1 + wscale * r(d)), wscale * r(d), embscale * r(32, heads), 1 + 0.3 * r(heads)]
    if axial:
        prm.append(1 + 0.3 * r(heads))
    return bf(qkv).double(), bf(r(N, E)).double(), [p.float() for p in prm]


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic, emulated
def emu(qkv, dout, geo, heads, d, prm, with_emb=True, with_hs=True, out_scale=0.5, acc_f=0, acc_b=0, out=None, dqkv=None, mutant=None):
    """One bf_attn_fwd + bf_attn_bwd of the MFMA kernel on padded 16 / 32-row tiles (rows >= L: clamped copies of row L - 1).
    -> out [N][E], dqkv [N][3 E] (bf16 values as doubles; tokens no sequence covers keep what they held), the six parameter gradients."""
    idx = AB.token_index(geo)
    nseq, L = idx.shape
    R = 16 if L <= 16 else 32
    E, N = heads * d, qkv.shape[0]
    rows = torch.arange(R).clamp(max=L - 1)
    idxc = idx[:, rows]
    prob = lambda t, parts: t.float()[idxc].view(nseq, R, heads, parts, d).permute(0, 2, 1, 3, 4)
    x, dO = prob(qkv, 3).clone(), prob(dout, 1)[..., 0, :].clone()
    if mutant == "stale_lookahead":                     # the last problem of a wave computed from the rows its predecessor left in `cur`
        src = (-1, -2) if heads > 1 else (-2, -1)
        x[-1, -1], dO[-1, -1] = x[src], dO[src]
    qw, qb, kw, kb, emb, hs = (p.float().clone() for p in prm[:6])
    embT = emb if with_emb else torch.zeros(32, heads)
    hsv = hs.clone() if with_hs else torch.ones(heads)
    if mutant == "head15_column":                       # column 15 of the 16-column LDS tables never staged
        embT, hsv = embT.clone(), hsv.clone()
        embT[:, 15], hsv[15] = 0.0, 1.0

    def ln(z):
        mu = z.sum(-1, keepdim=True) / d
        t = z - mu
        r = torch.rsqrt((t * t).sum(-1, keepdim=True) / d + AB.EPS)
        return t * r, r

    scale = torch.rsqrt(torch.tensor(float(d), dtype=F32))
    xq, rq = ln(x[..., 0, :])
    xk, rk = ln(x[..., 1, :])
    qf, kf, v = bf((xq * qw + qb) * scale), bf(xk * kw + kb), x[..., 2, :]
    ar = torch.arange(R)
    mkey = ar < L
    mk = (mkey[:, None] & mkey[None, :]).float()
    mneg = torch.where(mkey, 0.0, -float("inf"))
    if mutant == "dup_key_unmasked" and L < R:
        mneg[L] = 0.0
    bk = AB.bucket_matrix(R)
    if mutant == "bucket_low":                          # offsets 23..26 land one bucket low
        off = (ar[:, None] - ar[None, :]).abs()
        bk = torch.where((off >= 23) & (off <= 26), bk - 1, bk)
    S = qf @ kf.transpose(-1, -2) + embT[bk].permute(2, 0, 1).unsqueeze(0) + mneg
    e = torch.exp(S - S.max(-1, keepdim=True).values)
    P = e * (1.0 / e.sum(-1, keepdim=True))
    invL = torch.tensor(1.0 / 16 if mutant == "inv16" else float(np.float32(1.0) / np.float32(L)), dtype=F32)
    hv = hsv.view(1, heads, 1, 1)
    A = ((invL + (P - invL) * hv) if with_hs else P) * mk
    vz = v * mkey.float()[:, None]
    val = (bf(A) @ vz) * out_scale
    if acc_f:
        val = val + prob(out, 1)[..., 0, :]
    val = bf(val)
    if mutant == "row_group_from_neighbour":            # one 16-byte group of one row written from the row beside it
        s0, h0, i0 = nseq // 2, heads - 1, L // 2
        val[s0, h0, i0, 8:16] = val[s0, h0, i0 + 1 if i0 + 1 < L else i0 - 1, 8:16]
    out_t = torch.zeros(N, E, dtype=torch.float64) if out is None else out.clone()
    tok = lambda z: z[:, :, :L].permute(0, 2, 1, 3).reshape(nseq * L, -1).double()
    out_t[idx.flatten()] = tok(val)
    # ---- backward
    raw_out, raw_in, accumulate = bool(acc_b & 2), bool(acc_b & 4), bool(acc_b & 1)
    dP = (dO @ v.transpose(-1, -2)) * out_scale * mk
    dhs = torch.zeros(heads)
    if with_hs:
        dhs = ((P - invL) * dP).sum((0, 2, 3))
        dP = dP * hv
    dS = P * (dP - (P * dP).sum(-1, keepdim=True)) * mk
    demb_p = torch.zeros(nseq, heads, 32).index_add(2, bk.flatten(), dS.flatten(-2))
    if mutant == "demb_first_head":                     # a wave whose problems span several heads credits its T5 sums to its first head
        flat = demb_p.reshape(nseq * heads, 32)
        wave = torch.arange(0, nseq * heads, 4)         # problem stride 4 (one workgroup), heads not a multiple of it
        moved = flat[wave].sum(0)
        flat[wave] = 0.0
        flat[0] = moved
    demb = demb_p.sum(0).t().contiguous() if with_emb else torch.zeros(32, heads)
    T = lambda z: z.transpose(-1, -2)
    dv = (T(bf(A)) @ dO) * out_scale
    dkn = T(bf(dS)) @ qf
    dqn = (bf(dS) @ kf) * scale
    if accumulate:
        old = prob(dqkv, 3)
        if mutant != "acc_drops_v":
            dv = dv + old[..., 2, :]
    grads = [torch.zeros(d) for _ in range(4)]
    if raw_out:
        dq_s, dk_s = (dqn + old[..., 0, :], dkn + old[..., 1, :]) if accumulate else (dqn, dkn)
    else:
        res = []
        for part, (d0, xh, rs, w) in enumerate(((dqn, xq, rq, qw), (dkn, xk, rk, kw))):
            if raw_in:
                o = old[..., part, :] * (1.0 if mutant == "dup_row_in_ln_sums" else mkey.float()[:, None])
                if mutant != "raw_added_after_ln":
                    d0 = d0 + o
            grads[2 * part], grads[2 * part + 1] = (d0 * xh).sum((0, 1, 2)), d0.sum((0, 1, 2))
            g = d0 * w
            m1, m2 = g.sum(-1, keepdim=True) / d, (g * xh).sum(-1, keepdim=True) / d
            dx = rs * (g - m1 - xh * m2)
            if accumulate and (not raw_in or mutant == "raw_added_after_ln"):
                dx = dx + old[..., part, :]
            res.append(dx)
        dq_s, dk_s = res
    dq_t = torch.zeros(N, 3 * E, dtype=torch.float64) if dqkv is None else dqkv.clone()
    dq_t[idx.flatten()] = tok(bf(torch.stack([dq_s, dk_s, dv], 3)).flatten(-2))
    return out_t, dq_t, [t.double() for t in grads + [demb, dhs if with_hs else torch.zeros(heads)]]


def emu_axial(qkv, dout, frames, h, w, heads, d, prm, mutant=None, with_emb=True, with_hs=True):
    """forward accumulate 0 then 1, backward accumulate 2 then 5 -> out, dqkv, [dqw, dqb, dkw, dkb, demb, dhscale_x, dhscale_y]"""
    gW, gH = AB.axial_geos(frames, h, w)
    pW, pH = list(prm[:5]) + [prm[5]], list(prm[:5]) + [prm[6]]
    o1, d1, g1 = emu(qkv, dout, gW, heads, d, pW, with_emb, with_hs, 0.5, 0, 2)
    o2, d2, g2 = emu(qkv, dout, gH, heads, d, pH, with_emb, with_hs, 0.5, 1, 5, out=o1, dqkv=d1, mutant=mutant)
    return o2, d2, g2[:4] + [g1[4] + g2[4], g1[5], g2[5]]


# ------------------------------------------------------------------------------------------------ comparing
def ratios(res, got_out, got_dqkv, got_grads, geo, heads, d, names=AB.NAMES):
    """-> ({output: worst ratio}, [outputs out of bounds]) of an emulated / mutated result against plain()'s / axial_pair()'s bounds."""
    tokens = res["out"][0].dim() == 3
    pick = (lambda t, parts, part: t.view(t.shape[0], heads, parts, d)[:, :, part]) if tokens else (lambda t, parts, part: AB.from_tokens(t, geo, heads, parts, d, part))
    got = {"out": pick(got_out, 1, 0), "dq": pick(got_dqkv, 3, 0), "dk": pick(got_dqkv, 3, 1), "dv": pick(got_dqkv, 3, 2)}
    got.update(dict(zip(names, got_grads)))
    worst, bad = {}, []
    for k, (ref, bnd) in res.items():
        worst[k] = AB.worst_ratio(got[k], ref, bnd)[0]
        if worst[k] > 1.0:
            bad.append(k)
    return worst, bad


def old_criteria(res, got_out, got_dqkv, got_grads, geo, heads, d):
    """The whole-tensor checks of test_attention_mfma_matches_generic_and_fp32 with the fp64 reference in the fp32 kernel's place:
    {output: (figure, limit)}."""
    if geo is None:       # the axial pair: token layout, dhscale per pass
        N = got_out.shape[0]
        got = {"out": got_out.view(N, heads, d), **{n: got_dqkv.view(N, heads, 3, d)[:, :, i] for i, n in enumerate(("dq", "dk", "dv"))}}
        got.update(dict(zip(AB.NAMES[:5] + ("dhscale_x", "dhscale_y"), got_grads)))
    else:
        got = {"out": AB.from_tokens(got_out, geo, heads, 1, d), **{n: AB.from_tokens(got_dqkv, geo, heads, 3, d, i) for i, n in enumerate(("dq", "dk", "dv"))}}
        got.update(dict(zip(AB.NAMES, got_grads)))
    fig = {}
    for k, (ref, _) in res.items():
        if k == "dkb":
            fig[k] = (float((got[k] - ref).norm() / res["dqw"][0].norm()), OLD_LIMITS[k])
        else:
            fig[k] = (AB.rel_l2(got[k], ref), OLD_LIMITS[k[:7]])
    return fig


def _report(title, worst, old=None):
    line = f"{title}: worst |got - ref| / bnd " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items())
    if old is not None:
        missed = [k for k, (f, lim) in old.items() if f >= lim]
        line += " | old whole-tensor criteria: " + ("REJECT " + ", ".join(f"{k} {old[k][0]:.3g} >= {old[k][1]:g}" for k in missed) if missed else
                                                    "pass (largest " + max((f"{f / lim:.2f} of its limit ({k})" for k, (f, lim) in old.items()), key=lambda s: float(s.split()[0])) + ")")
    print(line)


# ------------------------------------------------------------------------------------------------ the two restatements agree
@pytest.mark.parametrize("L,d,heads,kind,with_emb,with_hs", [(7, 32, 2, "temporal", True, True), (24, 64, 3, "H", False, True), (16, 96, 5, "W", True, False)])
def test_handwritten_gradients_equal_autograd(L, d, heads, kind, with_emb, with_hs):
    geo, N = AB.geometry(kind, L, n_outer=2, inner=3)
    qkv, dout, prm = make(N, heads, d, L + d)
    res = AB.plain(qkv, dout, geo, heads, d, prm, with_emb, with_hs, 0.5, AB.FP32)
    o, dx, gr = AB.reference(qkv, dout, geo, heads, d, prm, 0.5, with_emb, with_hs)
    assert AB.rel_l2(res["out"][0], AB.from_tokens(o, geo, heads, 1, d)) < 1e-12
    for i, n in enumerate(("dq", "dk", "dv")):
        assert AB.rel_l2(res[n][0], AB.from_tokens(dx, geo, heads, 3, d, i)) < 1e-10, n
    for n, g in zip(AB.NAMES, gr):
        if n == "dkb":
            assert float((res[n][0] - g).abs().max()) < 1e-10 * float(gr[0].abs().max())
        elif n in res:
            assert AB.rel_l2(res[n][0], g) < 1e-10, n


def test_handwritten_axial_pair_equals_autograd():
    Fr, h, w, heads, d = 2, 5, 9, 3, 32
    qkv, dout, prm = make(Fr * h * w, heads, d, 3, axial=True)
    res = AB.axial_pair(qkv, dout, Fr, h, w, heads, d, prm, AB.MFMA)
    o, dx, gr = AB.reference_axial(qkv, dout, Fr, h, w, heads, d, prm)
    N = Fr * h * w
    assert AB.rel_l2(res["out"][0], o.view(N, heads, d)) < 1e-12
    for i, n in enumerate(("dq", "dk", "dv")):
        assert AB.rel_l2(res[n][0], dx.view(N, heads, 3, d)[:, :, i]) < 1e-10, n
    for n, g in zip(AB.NAMES[:3] + ("demb", "dhscale_x", "dhscale_y"), gr[:3] + gr[4:]):
        assert AB.rel_l2(res[n][0], g) < 1e-10, n


# ------------------------------------------------------------------------------------------------ the emulation is within the bound
SHAPES = [  # L, d, heads, geometry, emb, hscale, out_scale, accumulate
    (12, 64, 6, "contig", True, True, 0.5, False), (1, 32, 1, "contig", True, True, 1.0, False), (3, 128, 2, "temporal", False, True, 0.5, True),
    (15, 32, 16, "W", True, False, 1.0, True), (16, 96, 5, "H", True, True, 0.5, False), (17, 32, 6, "temporal", False, False, 1.0, False),
    (24, 128, 1, "H", True, True, 0.5, True), (31, 96, 3, "W", True, True, 1.0, False), (32, 64, 3, "contig", True, True, 0.5, True),
]


@pytest.mark.parametrize("L,d,heads,kind,with_emb,with_hs,out_scale,acc", SHAPES)
def test_emulation_is_within_the_bound(L, d, heads, kind, with_emb, with_hs, out_scale, acc):
    geo, N = AB.geometry(kind, L, n_outer=2, inner=3)
    qkv, dout, prm = make(N, heads, d, 11 * L + d + heads)
    g = torch.Generator().manual_seed(5)
    old_o = bf(torch.randn(N, heads * d, generator=g)).double() if acc else None
    old_d = bf(torch.randn(N, 3 * heads * d, generator=g)).double() if acc else None
    res = AB.plain(qkv, dout, geo, heads, d, prm, with_emb, with_hs, out_scale, AB.MFMA, old_o, old_d)
    o, dq, gr = emu(qkv, dout, geo, heads, d, prm, with_emb, with_hs, out_scale, int(acc), int(acc), old_o, old_d)
    worst, bad = ratios(res, o, dq, gr, geo, heads, d)
    _report(f"emulation L={L} d={d} heads={heads} {kind}", worst)
    assert not bad, (bad, worst)
    if not with_emb:
        assert float(gr[4].abs().max()) == 0.0
    if not with_hs:
        assert float(gr[5].abs().max()) == 0.0


@pytest.mark.parametrize("h,w,d,heads", [(12, 12, 64, 2), (5, 9, 32, 3), (3, 20, 128, 1), (24, 7, 96, 2)])
def test_emulated_raw_pair_is_within_the_bound(h, w, d, heads):
    Fr = 2
    qkv, dout, prm = make(Fr * h * w, heads, d, h + w, axial=True)
    res = AB.axial_pair(qkv, dout, Fr, h, w, heads, d, prm, AB.MFMA)
    o, dq, gr = emu_axial(qkv, dout, Fr, h, w, heads, d, prm)
    worst, bad = ratios(res, o, dq, gr, None, heads, d, AB.NAMES[:5] + ("dhscale_x", "dhscale_y"))
    _report(f"emulated axial pair {h}x{w} d={d}", worst)
    assert not bad, (bad, worst)


HARD = {"peaked": dict(qk_gain=5.5, embscale=8.0),      # scores q k^T d^-1/2 of order 5.5^2 = +-30, bias entries +-8: a nearly one-hot softmax
        "offset": dict(offset=48.0, spread=4.0)}        # rows 48 .. 150 +- 4: the LayerNorm subtracts a mean 10 - 40x its spread


@pytest.mark.parametrize("kind", sorted(HARD))
@pytest.mark.parametrize("L,d,heads", [(12, 64, 6), (31, 96, 2)])
def test_bound_holds_and_still_bites_at_hard_inputs(kind, L, d, heads):
    """The emulation stays within the bound; and the bound is not vacuous there: the narrowest mutant is still rejected."""
    geo, N = AB.geometry("temporal", L, n_outer=2, inner=3)
    qkv, dout, prm = make(N, heads, d, L + d, **HARD[kind])
    res = AB.plain(qkv, dout, geo, heads, d, prm, True, True, 0.5, AB.MFMA)
    worst, bad = ratios(res, *emu(qkv, dout, geo, heads, d, prm), geo, heads, d)
    _report(f"{kind} L={L} d={d}", worst)
    assert not bad, (bad, worst)
    if kind == "peaked":
        assert float(AB.forward(qkv, geo, heads, d, prm, True, True, AB.MFMA).P.max(-1).values.median()) > 0.9
    worst, bad = ratios(res, *emu(qkv, dout, geo, heads, d, prm, mutant="row_group_from_neighbour"), geo, heads, d)
    assert "out" in bad, worst
    print(f"{kind} L={L} d={d}: median bound / |out| = {float((res['out'][1] / res['out'][0].abs().clamp_min(1e-3)).median()):.3g}")


# ------------------------------------------------------------------------------------------------ emulated kernel bugs
MUTANTS = {  # name: (L or (h, w), d, heads, geometry or "axial", kwargs of emu, outputs it must break)
    "row_group_from_neighbour": (32, 64, 3, "contig14", {}, ("out",)),
    "stale_lookahead": (12, 64, 6, "temporal", {}, ("out", "dq", "dk", "dv")),
    "dup_key_unmasked": (31, 96, 2, "W", {}, ("out",)),
    "dup_row_in_ln_sums": ((3, 7), 64, 2, "axial", {}, ("dqw", "dqb", "dkw")),     # h = 3: thirteen clamped copies beside three rows.  At h = 12 (four
                                                                                   # copies) the sums move by 0.4 - 0.7 of their worst-case bound: not caught
    "bucket_low": (32, 64, 3, "contig", {}, ("out", "demb")),
    "inv16": (12, 64, 6, "H", {}, ("out",)),
    "head15_column": (8, 32, 16, "contig", {}, ("out",)),
    "acc_drops_v": (12, 64, 6, "temporal", {"acc_b": 1}, ("dv",)),
    "raw_added_after_ln": ((12, 7), 64, 2, "axial", {}, ("dq", "dk")),
    "demb_first_head": (12, 64, 6, "temporal", {}, ("demb",)),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_emulated_kernel_bug_is_rejected(name):
    L, d, heads, kind, kw, must = MUTANTS[name]
    if kind == "axial":
        Fr, (h, w) = 2, L                               # both passes have clamped duplicate rows
        qkv, dout, prm = make(Fr * h * w, heads, d, 77, axial=True)
        res = AB.axial_pair(qkv, dout, Fr, h, w, heads, d, prm, AB.MFMA)
        run = lambda m: emu_axial(qkv, dout, Fr, h, w, heads, d, prm, mutant=m)
        geo, names = None, AB.NAMES[:5] + ("dhscale_x", "dhscale_y")
    else:
        geo, N = ((14, L, 1, L, 0, 1), 14 * L) if kind == "contig14" else AB.geometry(kind, L, n_outer=2, inner=3)
        qkv, dout, prm = make(N, heads, d, 100 + L + d)
        g = torch.Generator().manual_seed(9)
        old_d = bf(torch.randn(N, 3 * heads * d, generator=g)).double() if kw.get("acc_b") else None
        res = AB.plain(qkv, dout, geo, heads, d, prm, True, True, 0.5, AB.MFMA, None, old_d)
        run = lambda m: emu(qkv, dout, geo, heads, d, prm, dqkv=old_d, mutant=m, **kw)
        names = AB.NAMES
    worst, bad = ratios(res, *run(None), geo, heads, d, names)
    assert not bad, ("the unmutated emulation must pass", bad, worst)
    got = run(name)
    worst, bad = ratios(res, *got, geo, heads, d, names)
    _report(f"mutant {name}", {k: worst[k] for k in bad}, old_criteria(res, *got, geo, heads, d))
    for k in must:
        assert k in bad, (name, k, worst)


def test_narrow_mutant_passes_the_old_whole_tensor_criteria():
    """One 8-channel group of one row of one problem taken from the neighbouring row, at a shape of the old test (L 32, d 64, 3 heads, 14
    contiguous sequences): every whole-tensor figure stays under its limit, the per-element check rejects the output."""
    L, d, heads = 32, 64, 3
    geo = (14, L, 1, L, 0, 1)
    qkv, dout, prm = make(14 * L, heads, d, 100 + L + d)
    res = AB.plain(qkv, dout, geo, heads, d, prm, True, True, 0.5, AB.MFMA)
    got = emu(qkv, dout, geo, heads, d, prm, mutant="row_group_from_neighbour")
    old = old_criteria(res, *got, geo, heads, d)
    print("old criteria on the narrow mutant:", {k: f"{f:.3g} < {lim:g}" for k, (f, lim) in old.items()})
    for k, (f, lim) in old.items():
        assert f < lim, (k, f, lim)
    worst, bad = ratios(res, *got, geo, heads, d)
    assert bad == ["out"] and worst["out"] > 1, worst


# ================================================================================================ the long-axis kernels (csrc/attn_long.hip)
# The same proof for attn_long.hip (33 <= L <= 128).  emu_long restates its arithmetic in fp32 torch on rows and keys padded to
# LP = 16 ceil(L / 16) as the kernel pads them (staged rows >= L zero, keys >= L at -inf, padded query rows zero), with bf16 rounding where
# pack4 rounds in the bf16 mode (qn, kn unscaled; the rescaled A; dO out_scale; dS) and none in the fp32 mode.
LONG_OLD_LIMITS = {"out": 1.5e-2, "dq": 3e-2, "dk": 3e-2, "dv": 3e-2, "dqw": 5e-2, "dqb": 5e-2, "dkw": 5e-2, "dkb": 1e-2, "demb": 5e-2, "dhscale": 1e-1}
LONG_FP32_LIMIT = 1e-5       # test_long_attention_fp32_matches_fp64, every output


def make_long(N, heads, d, seed, bf16, **kw):
    """make(), the stored values fp32 ones for the fp32 mode."""
    qkv, dout, prm = make(N, heads, d, seed, **kw)
    if bf16:
        return qkv, dout, prm
    g = torch.Generator().manual_seed(seed + 1)
    jit = lambda t: (t.float() * (1 + 2.0 ** -10 * torch.rand(t.shape, generator=g))).double()      # fp32 values that are not bf16 ones
    return jit(qkv), jit(dout), prm


def emu_long(qkv, dout, geo, heads, d, prm, with_emb=True, with_hs=True, out_scale=0.5, acc_f=0, acc_b=0, out=None, dqkv=None, bf16=True, mutant=None):
    """One bf_attn_fwd + bf_attn_bwd of attn_long.hip -> out [N][E], dqkv [N][3 E] (stored values as doubles), the six parameter gradients."""
    idx = AB.token_index(geo)
    nseq, L = idx.shape
    LP = 16 * ((L + 15) // 16)
    E, N = heads * d, qkv.shape[0]
    r = bf if bf16 else (lambda t: t)
    pad = lambda t: torch.nn.functional.pad(t, (0, 0, 0, LP - L))                                    # staged rows >= L are zero
    prob = lambda t, parts: t.float()[idx].view(nseq, L, heads, parts, d).permute(0, 2, 1, 3, 4)
    x, dO = prob(qkv, 3), prob(dout, 1)[..., 0, :]
    qw, qb, kw, kb, emb, hs = (p.float().clone() for p in prm[:6])
    os32 = torch.tensor(out_scale, dtype=F32)

    def ln(z, stale=False):
        mu = z.sum(-1, keepdim=True) / d
        t = z - mu
        rs = torch.rsqrt((t * t).sum(-1, keepdim=True) / d + AB.EPS)
        if stale:                                       # row L - 1 from row L - 2's statistics
            mu, rs = mu.clone(), rs.clone()
            mu[..., L - 1, :], rs[..., L - 1, :] = mu[..., L - 2, :], rs[..., L - 2, :]
        return (z - mu) * rs, rs

    scale = torch.rsqrt(torch.tensor(float(d), dtype=F32))
    xq, rq = ln(x[..., 0, :], mutant == "stale_row_stats")
    xk, rk = ln(x[..., 1, :])
    qn, kn, v = pad(xq * qw + qb), pad(xk * kw + kb), pad(x[..., 2, :])
    qs = r(qn)
    if mutant == "tail_slice_zero":                     # the columns beyond the last whole 16 never reach the score product
        qs = qs.clone()
        qs[..., 16 * (d // 16):] = 0.0
    ar = torch.arange(LP)
    live = ar < L
    mk = (live[:, None] & live[None, :]).float()
    mneg = torch.where(live, 0.0, -float("inf"))
    if mutant == "key_mask_off_by_one":
        mneg[L - 1] = -float("inf")
    bk = AB.bucket_matrix(LP)
    if mutant == "negative_far_bucket":                 # every offset <= -27 lands in the positive side's last bucket
        far = (ar[:, None] - ar[None, :]) <= -27
        bk = torch.where(far, bk.t(), bk)
    embT = (emb if with_emb else torch.zeros(32, heads)).t()[None, :, :, None].expand(nseq, heads, 32, 1)[..., 0]      # [s][h][32]
    if mutant == "stale_s_emb":                         # the second half of the problems (a workgroup's second problem) keeps the head before
        flat = embT.reshape(nseq * heads, 32).clone()
        half = (nseq * heads) // 2
        flat[half:] = embT.reshape(nseq * heads, 32)[half - 1:-1]
        embT = flat.view(nseq, heads, 32)
    S = (qs @ r(kn).transpose(-1, -2)) * scale
    if with_emb:
        S = S + embT[:, :, bk]
    S = S + mneg
    e = torch.exp(S - S.max(-1, keepdim=True).values)
    P = (e * (1.0 / e.sum(-1, keepdim=True))) * mk      # padded query rows are zero
    invL = torch.tensor(1.0 / LP if mutant == "inv_LP" else float(np.float32(1.0) / np.float32(L)), dtype=F32)
    hv = hs.view(1, heads, 1, 1)
    A = (invL + (P - invL) * hv) if with_hs else P       # padded entries meet zero rows of V / dO
    val = (r(A) @ v) * os32
    if acc_f:
        val[:, :, :L] = val[:, :, :L] + prob(out, 1)[..., 0, :]
    val = r(val) if bf16 else val
    if mutant == "row_group_from_neighbour":
        s0, h0, i0 = nseq // 2, heads - 1, L // 2
        val[s0, h0, i0, 8:16] = val[s0, h0, i0 + 1, 8:16]
    out_t = torch.zeros(N, E, dtype=torch.float64) if out is None else out.clone()
    tok = lambda z: z[:, :, :L].permute(0, 2, 1, 3).reshape(nseq * L, -1).double()
    out_t[idx.flatten()] = tok(val)
    # ---- backward
    raw_out, raw_in, accumulate = bool(acc_b & 2), bool(acc_b & 4), bool(acc_b & 1)
    T = lambda z: z.transpose(-1, -2)
    g = pad(dO * os32)
    dA = (r(pad(dO)) if mutant == "dA_without_out_scale" else r(g)) @ T(v)
    dA = dA * mk
    dhs = torch.zeros(heads)
    if with_hs:
        dhs = ((P - invL) * dA * mk).sum((0, 2, 3))
        dA = dA * hv
    dS = P * (dA - (P * dA).sum(-1, keepdim=True))
    demb = torch.zeros(nseq, heads, 32).index_add(2, bk.flatten(), dS.flatten(-2)).sum(0).t().contiguous() if with_emb else torch.zeros(32, heads)
    dv = T(r(P if mutant == "dv_from_P" else A)) @ r(g)
    dqn = (r(dS) @ r(kn)) * scale
    dkn = (T(r(dS)) @ r(qn)) * scale
    old = pad(prob(dqkv, 3).flatten(-2)).view(nseq, heads, LP, 3, d) if (accumulate or raw_in) else None
    if accumulate:
        dv = dv + old[..., 2, :]
    grads = [torch.zeros(d) for _ in range(4)]
    if raw_out:
        dq_s, dk_s = dqn, dkn                           # bit 0 is clear in mode 2: nothing is added
    else:
        res = []
        for part, (d0, xh, rs, w) in enumerate(((dqn, pad(xq), pad(rq), qw), (dkn, pad(xk), pad(rk), kw))):
            if raw_in:
                d0 = d0 + old[..., part, :]
            per = (d0 * xh).sum(2)                      # [s][h][d]
            if mutant == "a_ln_not_cleared" and part == 0:
                per[0, 0] = 2 * per[0, 0]               # one problem's dqw counted twice
            grads[2 * part], grads[2 * part + 1] = per.sum((0, 1)), d0.sum((0, 1, 2))
            gg = d0 * w
            m1, m2 = gg.sum(-1, keepdim=True) / d, (gg * xh).sum(-1, keepdim=True) / d
            dx = rs * (gg - m1 - xh * m2)
            if (accumulate and not raw_in) or (raw_in and mutant == "raw_added_again_after_ln"):
                dx = dx + old[..., part, :]
            res.append(dx)
        dq_s, dk_s = res
    dq_t = torch.zeros(N, 3 * E, dtype=torch.float64) if dqkv is None else dqkv.clone()
    st = torch.stack([dq_s, dk_s, dv], 3)
    dq_t[idx.flatten()] = tok((r(st) if bf16 else st).flatten(-2))
    return out_t, dq_t, [t.double() for t in grads + [demb, dhs if with_hs else torch.zeros(heads)]]


def emu_long_axial(qkv, dout, frames, h, w, heads, d, prm, mutant=None):
    """forward 0 then 1, backward 2 then 5; an axis of at most 32 tokens runs the short kernel's emulation"""
    gW, gH = AB.axial_geos(frames, h, w)
    pW, pH = list(prm[:5]) + [prm[5]], list(prm[:5]) + [prm[6]]
    eW, eH = (emu_long if w > 32 else emu), (emu_long if h > 32 else emu)
    o1, d1, g1 = eW(qkv, dout, gW, heads, d, pW, True, True, 0.5, 0, 2)
    o2, d2, g2 = eH(qkv, dout, gH, heads, d, pH, True, True, 0.5, 1, 5, out=o1, dqkv=d1, mutant=mutant)
    return o2, d2, g2[:4] + [g1[4] + g2[4], g1[5], g2[5]]


def long_mode(bf16):
    return AB.LONG_BF16 if bf16 else AB.LONG_FP32


def test_long_restatement_equals_autograd():
    """The short modes are the tuples they were (their callers see no long field set); the long restatement's values are the autograd ones."""
    assert AB.MFMA == (AB.U16, AB.U16, False) and AB.FP32[:2] == (0.0, AB.U32) and not AB.GENERIC_BF16.long
    L, d, heads = 49, 24, 2
    geo, N = AB.geometry("H", L, n_outer=1, inner=2)
    qkv, dout, prm = make(N, heads, d, 4)
    os_ = float(np.float32(0.37))
    res = AB.plain(qkv, dout, geo, heads, d, prm, True, True, os_, AB.LONG_BF16)
    o, dx, gr = AB.reference(qkv, dout, geo, heads, d, prm, os_, True, True)
    assert AB.rel_l2(res["out"][0], AB.from_tokens(o, geo, heads, 1, d)) < 1e-12
    for i, n in enumerate(("dq", "dk", "dv")):
        assert AB.rel_l2(res[n][0], AB.from_tokens(dx, geo, heads, 3, d, i)) < 1e-10, n
    for n, g in zip(AB.NAMES, gr):
        if n != "dkb":
            assert AB.rel_l2(res[n][0], g) < 1e-10, n
    for k, (ref, bnd) in res.items():                   # no element is left out of check(): every bound is finite (an unused T5 bucket: ref 0, bound 0, held exactly)
        assert torch.isfinite(bnd).all() and bool((bnd >= 0).all()), k


LONG_SHAPES = [  # L, d, heads, geometry, emb, hscale, out_scale, accumulate: L in {33, 48, 49, 100, 128} x d in {8, 24, 64, 128}
    (33, 8, 3, "contig", True, True, 0.5, 0), (33, 128, 1, "H", False, True, 0.37, 1), (48, 24, 2, "temporal", True, False, 0.37, 0),
    (48, 64, 2, "W", False, False, 0.5, 1), (49, 64, 2, "H", True, True, 0.37, 1), (49, 8, 16, "contig", True, True, 0.5, 0),
    (100, 24, 2, "W", True, True, 0.5, 1), (100, 128, 1, "temporal", True, True, 0.37, 0), (128, 64, 2, "contig", True, True, 0.37, 0),
    (128, 8, 2, "H", False, True, 0.5, 1), (128, 128, 1, "W", True, False, 0.5, 0), (100, 64, 3, "H", True, True, 0.5, 0),
]


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("L,d,heads,kind,with_emb,with_hs,out_scale,acc", LONG_SHAPES)
def test_long_emulation_is_within_the_bound(L, d, heads, kind, with_emb, with_hs, out_scale, acc, bf16):
    geo, N = AB.geometry(kind, L, n_outer=1, inner=2)
    qkv, dout, prm = make_long(N, heads, d, 13 * L + d + heads, bf16)
    g = torch.Generator().manual_seed(6)
    cast = bf if bf16 else (lambda t: t)
    old_o = cast(torch.randn(N, heads * d, generator=g)).double() if acc else None
    old_d = cast(torch.randn(N, 3 * heads * d, generator=g)).double() if acc else None
    os_ = float(np.float32(out_scale))                  # the value the kernel receives
    res = AB.plain(qkv, dout, geo, heads, d, prm, with_emb, with_hs, os_, long_mode(bf16), old_o, old_d)
    got = emu_long(qkv, dout, geo, heads, d, prm, with_emb, with_hs, os_, acc, acc, old_o, old_d, bf16)
    worst, bad = ratios(res, *got, geo, heads, d)
    _report(f"long emulation L={L} d={d} heads={heads} {kind} {'bf16' if bf16 else 'fp32'}", worst)
    assert not bad, (bad, worst)
    for k, (ref, bnd) in res.items():
        assert torch.isfinite(bnd).all() and bool((bnd >= 0).all()), k     # check() judges every element (an unused bucket: ref 0, bound 0, exact)


@pytest.mark.parametrize("h,w,d,heads", [(40, 12, 32, 2), (12, 64, 64, 1), (33, 48, 128, 1)])
def test_long_emulated_raw_pair_is_within_the_bound(h, w, d, heads):
    """2 then 5 with the long axis on H only, on W only and on both; the short pass is held with the short mode's bound."""
    Fr = 1
    qkv, dout, prm = make(Fr * h * w, heads, d, h + w, axial=True)
    modes = (AB.LONG_BF16 if w > 32 else AB.MFMA, AB.LONG_BF16 if h > 32 else AB.MFMA)
    res = AB.axial_pair(qkv, dout, Fr, h, w, heads, d, prm, modes)
    got = emu_long_axial(qkv, dout, Fr, h, w, heads, d, prm)
    worst, bad = ratios(res, *got, None, heads, d, AB.NAMES[:5] + ("dhscale_x", "dhscale_y"))
    _report(f"long emulated axial pair {h}x{w} d={d}", worst)
    assert not bad, (bad, worst)


def _narrowest(res, qkv, dout, geo, heads, d, prm, bf16, **kw):
    return ratios(res, *emu_long(qkv, dout, geo, heads, d, prm, bf16=bf16, mutant="row_group_from_neighbour", **kw), geo, heads, d)


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("kind", sorted(HARD))
@pytest.mark.parametrize("L,d,heads", [(33, 64, 2), (49, 24, 2), (100, 64, 2), (128, 24, 1)])
def test_long_bound_holds_and_still_bites_at_hard_inputs(kind, L, d, heads, bf16):
    """The emulation stays within the bound and the narrowest mutant (one 8-channel group of `out` from the row beside it) is rejected --
    at every case but one family: bf16, the offset input, L >= 100.  There V is 48 .. 150 and the two rows' outputs, averages over a
    hundred keys, differ by about 1 in 45, while a correct bf16 kernel may itself be off by 2^-8 |A| |V| + 2^-8 |out| ~ 0.4 plus the softmax's
    share: the swap measures 0.55 of the bound at both shapes (it is rejected at L = 33 and 49, where rows differ more, and in fp32 at
    every L).  No sound worst-case bound separates that swap from bf16 rounding; the test asserts that it is at least half the bound, so
    a bound that grew would be noticed."""
    geo, N = AB.geometry("temporal", L, n_outer=1, inner=2)
    qkv, dout, prm = make_long(N, heads, d, L + d, bf16, **HARD[kind])
    res = AB.plain(qkv, dout, geo, heads, d, prm, True, True, 0.5, long_mode(bf16))
    worst, bad = ratios(res, *emu_long(qkv, dout, geo, heads, d, prm, bf16=bf16), geo, heads, d)
    _report(f"long {kind} L={L} d={d} {'bf16' if bf16 else 'fp32'}", worst)
    assert not bad, (bad, worst)
    if kind == "peaked":
        assert float(AB.forward(qkv, geo, heads, d, prm, True, True, long_mode(bf16)).P.max(-1).values.median()) > 0.9
    worst, bad = _narrowest(res, qkv, dout, geo, heads, d, prm, bf16)
    print(f"long {kind} L={L} d={d}: the narrowest mutant measures {worst['out']:.3g} of the bound")
    if bf16 and kind == "offset" and L >= 100:
        assert worst["out"] > 0.5, worst
    else:
        assert "out" in bad, worst


LONG_MUTANTS = {  # name: (L or (h, w), d, heads, geometry or "axial", kwargs of emu_long, outputs it must break)
    "key_mask_off_by_one": (49, 64, 2, "W", {}, ("out", "dv")),
    "stale_row_stats": (48, 64, 2, "temporal", {}, ("out",)),
    "tail_slice_zero": (100, 24, 2, "H", {}, ("out",)),
    "inv_LP": (33, 64, 2, "contig", {}, ("out",)),
    "dv_from_P": (48, 64, 2, "W", {}, ("dv",)),
    "dA_without_out_scale": (49, 24, 2, "temporal", {"out_scale": 0.37}, ("dq", "dk")),
    "negative_far_bucket": (100, 64, 2, "contig", {}, ("out",)),
    "stale_s_emb": (33, 8, 3, "contig", {}, ("out",)),
    "raw_added_again_after_ln": ((40, 12), 32, 2, "axial", {}, ("dq", "dk")),
    "a_ln_not_cleared": (33, 64, 1, "W", {"bf16": False}, ("dqw",)),             # fp32 mode: in bf16 the worst-case bound of a sum over all rows
                                                                                 # (every dqn 2^-8 off, all one way) exceeds one problem's share
}


@pytest.mark.parametrize("name", list(LONG_MUTANTS))
def test_long_emulated_kernel_bug_is_rejected(name):
    L, d, heads, kind, kw, must = LONG_MUTANTS[name]
    if kind == "axial":
        Fr, (h, w) = 1, L
        qkv, dout, prm = make(Fr * h * w, heads, d, 78, axial=True)
        res = AB.axial_pair(qkv, dout, Fr, h, w, heads, d, prm, (AB.LONG_BF16 if w > 32 else AB.MFMA, AB.LONG_BF16 if h > 32 else AB.MFMA))
        run = lambda m: emu_long_axial(qkv, dout, Fr, h, w, heads, d, prm, mutant=m)
        geo, names = None, AB.NAMES[:5] + ("dhscale_x", "dhscale_y")
    else:
        geo, N = AB.geometry(kind, L, n_outer=1, inner=2)
        bf16 = kw.get("bf16", True)
        qkv, dout, prm = make_long(N, heads, d, 200 + L + d, bf16)
        os_ = float(np.float32(kw.get("out_scale", 0.5)))
        res = AB.plain(qkv, dout, geo, heads, d, prm, True, True, os_, long_mode(bf16))
        run = lambda m: emu_long(qkv, dout, geo, heads, d, prm, out_scale=os_, bf16=bf16, mutant=m)
        names = AB.NAMES
    worst, bad = ratios(res, *run(None), geo, heads, d, names)
    assert not bad, ("the unmutated emulation must pass", bad, worst)
    worst, bad = ratios(res, *run(name), geo, heads, d, names)
    _report(f"long mutant {name}", {k: worst[k] for k in bad})
    for k in must:
        assert k in bad, (name, k, worst)


def long_old_criteria(res, got_out, got_dqkv, got_grads, geo, heads, d):
    """The whole-tensor figures of tests/test_gpu_long_attention.py with the fp64 reference in the comparison kernel's place:
    {output: relative L2} (dkb: against |dqw|, as there)."""
    got = {"out": AB.from_tokens(got_out, geo, heads, 1, d), **{n: AB.from_tokens(got_dqkv, geo, heads, 3, d, i) for i, n in enumerate(("dq", "dk", "dv"))}}
    got.update(dict(zip(AB.NAMES, got_grads)))
    return {k: float((got[k] - ref).norm() / res["dqw"][0].norm()) if k == "dkb" else AB.rel_l2(got[k], ref) for k, (ref, _) in res.items()}


def test_long_narrow_mutant_passes_the_old_whole_tensor_criteria():
    """Why tests/test_gpu_long_attn_edges.py exists.  One 8-channel group of one row of one problem taken from the neighbouring row, at
    L 128, d 64, 6 heads in bf16: every whole-tensor figure of test_long_attention_bf16_matches_fp32 stays under its limit (the fp64
    reference in the fp32 kernel's place), and the per-element check rejects `out`.  The limit of test_long_attention_fp32_matches_fp64 is
    1e-5 on every output and belongs to the fp32 mode; the same mutant on the fp32 emulation leaves the backward outputs and the parameter
    sums under it (2e-7 .. 1e-6), while `out` itself measures 4e-3 there: that one limit does see a swapped group at this size (it would not see a
    group whose error is below about 0.2 % of its values -- one bf16 rounding -- which the fp32 per-element bound, about 1e-6, does)."""
    L, d, heads = 128, 64, 6
    geo, N = AB.geometry("contig", L)
    for bf16 in (True, False):
        qkv, dout, prm = make_long(N, heads, d, 300, bf16)
        res = AB.plain(qkv, dout, geo, heads, d, prm, True, True, 0.5, long_mode(bf16))
        got = emu_long(qkv, dout, geo, heads, d, prm, bf16=bf16, mutant="row_group_from_neighbour")
        old = long_old_criteria(res, *got, geo, heads, d)
        print("bf16" if bf16 else "fp32", "old criteria on the narrow mutant:", {k: f"{f:.3g}" for k, f in old.items()})
        for k, f in old.items():
            if bf16:
                assert f < LONG_OLD_LIMITS[k], (k, f)
            elif k != "out":
                assert f < LONG_FP32_LIMIT, (k, f)
        worst, bad = ratios(res, *got, geo, heads, d)
        assert bad == ["out"] and worst["out"] > 1, worst
