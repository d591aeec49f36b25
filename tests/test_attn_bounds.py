"""CPU: the per-element attention checker (tests/attn_bounds.py) pinned without a GPU.  A torch emulation of attn_mfma.hip's arithmetic
(fp32, with bf16 rounding exactly where the kernel rounds: the Qn d^-1/2 / Kn operands, the rescaled A, the A^T / dS^T tiles, the raw q / k
gradient between the axial passes, every store) passes it at a spread of shapes, at a peaked and at a large-offset input; ten emulated
kernel bugs fail it.  For every mutant the test also prints what the whole-tensor criteria of
test_gpu_kernels.py::test_attention_mfma_matches_generic_and_fp32 would have said (run with -s to see the table)."""
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
