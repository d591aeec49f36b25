"""CPU: the per-element conv checker (tests/conv_bounds.py) pinned without a GPU.  A CPU emulation of the kernel's arithmetic (prologue
in fp32, operands rounded as conv.hip rounds them, fp32 accumulation) passes it at several shapes; six emulated kernel bugs fail it.
The test also records which of them the whole-tensor rel-L2 check of the older tests (1e-2 bf16, 1e-5 fp32) lets through."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_bounds as CB

RELL2 = {False: 1e-5, True: 1e-2}


def _randn(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _stored(t, bf16):
    return CB.rnd16(t) if bf16 else t.float().double()


def _case(Fr, Hi, Wi, C0, C1, N, k, pro, bf16, seed=0):
    """Stored sources, fp32 sc / sh differing per frame, weights rounded to the compute dtype."""
    Cin = C0 + C1
    srcs = [_stored(_randn(Fr, C, Hi, Wi, seed=seed + i), bf16) for i, C in enumerate((C0, C1)) if C]
    sc = (1 + _randn(Fr, Cin, scale=0.1, seed=seed + 5)).float().double()
    sh = _randn(Fr, Cin, scale=0.1, seed=seed + 6).float().double()
    w = _stored(_randn(N, Cin, k, k, scale=(k * k * Cin) ** -0.5, seed=seed + 7), bf16)
    return srcs, sc, sh, w


# ---------------------------------------------------------------------------------------------------- CPU emulation of the kernel
def _emu_pro(v, pro, sc, sh):
    """The prologue as gather() computes it: fmaf (one rounding of the exact v*sc + sh), then fp32 exact-erf GELU."""
    if pro == CB.PRO_NONE:
        return v.float()
    t = (v * sc[:, :, None, None] + sh[:, :, None, None]).float() if pro == CB.PRO_AFFINE_GELU else v.float()
    return 0.5 * t * (1 + torch.erf(t * 0.70710678118654752440))


def _emu_rows(srcs, pro, sc, sh, k, stride, pad, Ho, Wo, bf16, mutant=None):
    """Operand rows (M, K) in fp32, K ordered (ky, kx, c)."""
    v = torch.cat(srcs, 1)
    if mutant == "c0_off_by_one":                        # the first channel of source 1 read one channel off
        v = v.clone()
        v[:, srcs[0].shape[1]] = srcs[1][:, 1]
    if mutant == "prologue_on_padding":                  # activate the zero-padded raw input: padding taps become gelu(sh)
        a = _emu_pro(F.pad(v, (pad,) * 4), pro, sc, sh)
        pad = 0
    else:
        a = _emu_pro(v, pro, sc, sh)
    rows = CB.unfold(a.double(), k, stride, pad, Ho, Wo)
    if bf16:
        r = CB.rnd16(rows)
        if mutant == "unrounded_k_run":                  # one run of 8 k-elements staged without the bf16 conversion
            r[:, 8:16] = rows[:, 8:16]
        rows = r
    return rows.float()


def emu_fwd(srcs, pro, sc, sh, w, stride, pad, Ho, Wo, bf16, bias=None, out_bf16=None, mutant=None):
    Fr, (N, Cin, k, _) = srcs[0].shape[0], w.shape
    A = _emu_rows(srcs, pro, sc, sh, k, stride, pad, Ho, Wo, bf16, mutant)
    Wg = w.permute(2, 3, 1, 0).reshape(k * k * Cin, N).float()
    out = A @ Wg
    if mutant == "tap_dropped_last_column":              # centre tap missing from the last output column
        last = (torch.arange(A.shape[0]) % Wo) == Wo - 1
        t = (k * k // 2) * Cin
        out[last] -= A[last, t:t + Cin] @ Wg[t:t + Cin]
    if bias is not None:
        out = out + bias.float()
    out = out.view(Fr, Ho, Wo, N).permute(0, 3, 1, 2)
    if mutant == "ragged_tile_last_channel_zero":
        out[:, N - 1] = 0
    return CB.rnd16(out) if (bf16 if out_bf16 is None else out_bf16) else out.double()


def emu_transposed(src, w, stride, pad, Ho, Wo, bf16):
    return CB.transposed(src.float(), w.float(), stride, pad, Ho, Wo).double()


def emu_wgrad(rows, srcs, pro, sc, sh, k, stride, pad, bf16, mutant=None):
    Fr, R, Ho, Wo = rows.shape
    A = _emu_rows(srcs, pro, sc, sh, k, stride, pad, Ho, Wo, bf16)
    rm = rows.permute(0, 2, 3, 1).reshape(-1, R)
    rm = (CB.rnd16(rm) if bf16 else rm).float()
    chunk, slabs = CB.wgrad_split(R, A.shape[1], A.shape[0])
    out = torch.zeros(R, A.shape[1], dtype=torch.float32)
    for z in range(slabs - (mutant == "last_ragged_slab_omitted")):
        out += rm[z * chunk:(z + 1) * chunk].t() @ A[z * chunk:(z + 1) * chunk]
    return out.double()


# ---------------------------------------------------------------------------------------------------- the checker accepts a correct kernel
def _fwd_ref(srcs, pro, sc, sh, w, stride, pad, Ho, Wo, bf16, bias=None, out_bf16=None):
    a, ea = CB.operand(torch.cat(srcs, 1), pro, sc, sh, bf16)
    return CB.conv_fwd(a, ea, w, stride, pad, Ho, Wo, bias=bias, out_bf16=bf16 if out_bf16 is None else out_bf16)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("Fr,Hi,Wi,C0,C1,N,k,s,p,pro", [
    (2, 5, 7, 8, 0, 8, 3, 1, 1, CB.PRO_AFFINE_GELU),
    (3, 3, 5, 12, 20, 65, 3, 1, 1, CB.PRO_AFFINE_GELU),     # two sources, ragged column tile
    (1, 7, 6, 33, 0, 16, 3, 2, 1, CB.PRO_GELU),
    (2, 4, 4, 5, 12, 24, 1, 1, 0, CB.PRO_NONE),
    (1, 2, 2, 3, 0, 8, 3, 2, 1, CB.PRO_AFFINE_GELU),        # 2x2 input at stride 2: mostly padding
])
def test_emulated_kernel_within_bound(bf16, Fr, Hi, Wi, C0, C1, N, k, s, p, pro):
    srcs, sc, sh, w = _case(Fr, Hi, Wi, C0, C1, N, k, pro, bf16, seed=Hi * 31 + N)
    Ho, Wo = (Hi + 2 * p - k) // s + 1, (Wi + 2 * p - k) // s + 1
    bias = _randn(N, scale=0.1, seed=3).float().double()
    for out_bf16 in ({bf16, False}):
        ref, bnd = _fwd_ref(srcs, pro, sc, sh, w, s, p, Ho, Wo, bf16, bias, out_bf16)
        got = emu_fwd(srcs, pro, sc, sh, w, s, p, Ho, Wo, bf16, bias, out_bf16)
        assert CB.check(got, ref, bnd, "fwd") <= 1.0
    # transposed gather (data-gradient role) and weight gradient on the same sources
    src = srcs[0]
    wt = _stored(_randn(src.shape[1], N, 4, 4, scale=(4 * src.shape[1]) ** -0.5, seed=8), bf16)
    a, ea = CB.operand(src, bf16=bf16)
    ref, bnd = CB.conv_transposed(a, ea, wt, 2, 1, 2 * Hi, 2 * Wi, out_bf16=bf16)
    got = emu_transposed(a, wt, 2, 1, 2 * Hi, 2 * Wi, bf16)
    assert CB.check(CB.rnd16(got) if bf16 else got, ref, bnd, "transposed") <= 1.0
    rows = _stored(_randn(Fr, 9, Ho, Wo, seed=9), bf16)
    a, ea = CB.operand(torch.cat(srcs, 1), pro, sc, sh, bf16)
    ref, bnd = CB.conv_wgrad(rows, a, ea, k, s, p)
    assert CB.check(emu_wgrad(rows, srcs, pro, sc, sh, k, s, p, bf16), ref, bnd, "wgrad", ("r", "k")) <= 1.0


def test_wgrad_split_matches_the_kernel_formula():
    """The slab split the wgrad bound uses: whole CBK-pixel chunks covering M, the last one partial where M is not a multiple."""
    chunk, slabs = CB.wgrad_split(8, 72, 4 * 61 * 67)
    assert (chunk, slabs) == (256, 64) and 4 * 61 * 67 - (slabs - 1) * chunk == 220
    assert CB.wgrad_split(8, 8, 15) == (32, 1)


# ---------------------------------------------------------------------------------------------------- mutants
def _m_prologue_on_padding(mutant):
    srcs, sc, sh, w = _case(1, 96, 96, 8, 0, 8, 3, CB.PRO_AFFINE_GELU, True, seed=11)
    ref, bnd = _fwd_ref(srcs, CB.PRO_AFFINE_GELU, sc, sh, w, 1, 1, 96, 96, True)
    return emu_fwd(srcs, CB.PRO_AFFINE_GELU, sc, sh, w, 1, 1, 96, 96, True, mutant=mutant), ref, bnd, True


def _m_tap_dropped_last_column(mutant):
    srcs, sc, sh, w = _case(2, 7, 6, 16, 0, 16, 3, CB.PRO_GELU, False, seed=12)
    ref, bnd = _fwd_ref(srcs, CB.PRO_GELU, sc, sh, w, 1, 1, 7, 6, False)
    return emu_fwd(srcs, CB.PRO_GELU, sc, sh, w, 1, 1, 7, 6, False, mutant=mutant), ref, bnd, False


def _m_c0_off_by_one(mutant):
    srcs, sc, sh, w = _case(2, 6, 10, 12, 20, 16, 3, CB.PRO_AFFINE_GELU, True, seed=13)
    ref, bnd = _fwd_ref(srcs, CB.PRO_AFFINE_GELU, sc, sh, w, 1, 1, 6, 10, True)
    return emu_fwd(srcs, CB.PRO_AFFINE_GELU, sc, sh, w, 1, 1, 6, 10, True, mutant=mutant), ref, bnd, True


def _m_last_ragged_slab_omitted(mutant):
    srcs, sc, sh, _ = _case(4, 61, 67, 8, 0, 8, 3, CB.PRO_NONE, False, seed=14)
    rows = _stored(_randn(4, 8, 61, 67, seed=15), False)
    a, ea = CB.operand(srcs[0])
    ref, bnd = CB.conv_wgrad(rows, a, ea, 3, 1, 1)
    return emu_wgrad(rows, srcs, CB.PRO_NONE, sc, sh, 3, 1, 1, False, mutant=mutant), ref, bnd, False


def _m_unrounded_k_run(mutant):
    srcs, sc, sh, w = _case(2, 8, 8, 16, 0, 16, 3, CB.PRO_AFFINE_GELU, True, seed=16)
    ref, bnd = _fwd_ref(srcs, CB.PRO_AFFINE_GELU, sc, sh, w, 1, 1, 8, 8, True, out_bf16=False)      # fp32 output: the dA path
    return emu_fwd(srcs, CB.PRO_AFFINE_GELU, sc, sh, w, 1, 1, 8, 8, True, out_bf16=False, mutant=mutant), ref, bnd, True


def _m_ragged_tile_last_channel_zero(mutant):
    srcs, sc, sh, w = _case(1, 5, 7, 8, 0, 100, 3, CB.PRO_GELU, True, seed=17)
    ref, bnd = _fwd_ref(srcs, CB.PRO_GELU, sc, sh, w, 1, 1, 5, 7, True)
    return emu_fwd(srcs, CB.PRO_GELU, sc, sh, w, 1, 1, 5, 7, True, mutant=mutant), ref, bnd, True


MUTANTS = {
    "prologue_on_padding": _m_prologue_on_padding,
    "tap_dropped_last_column": _m_tap_dropped_last_column,
    "c0_off_by_one": _m_c0_off_by_one,
    "last_ragged_slab_omitted": _m_last_ragged_slab_omitted,
    "unrounded_k_run": _m_unrounded_k_run,
    "ragged_tile_last_channel_zero": _m_ragged_tile_last_channel_zero,
}
# mutants the whole-tensor rel-L2 check lets through at these shapes (printed by the test; the set is part of what it pins)
RELL2_ACCEPTS = {"prologue_on_padding", "unrounded_k_run"}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_setup_passes_unmutated(name):
    got, ref, bnd, _ = MUTANTS[name](None)
    assert CB.check(got, ref, bnd, name) <= 1.0


def test_every_mutant_is_rejected(capsys):
    accepted_by_rel_l2 = set()
    rows = []
    for name, make in MUTANTS.items():
        got, ref, bnd, bf16 = make(name)
        with pytest.raises(AssertionError, match="exceeds the bound"):
            CB.check(got, ref, bnd, name)
        rel = CB.rel_l2(got, ref)
        if rel <= RELL2[bf16]:
            accepted_by_rel_l2.add(name)
        rows.append(f"  {name:32s} {'bf16' if bf16 else 'fp32'}  rel-L2 {rel:.2e} ({'accepted' if rel <= RELL2[bf16] else 'rejected'} "
                    f"by rel-L2 <= {RELL2[bf16]:g}); per-element check: rejected")
    with capsys.disabled():
        print("\nconv checker mutants:\n" + "\n".join(rows))
    assert accepted_by_rel_l2 == RELL2_ACCEPTS
