"""Short-axis attention (L <= 32: csrc/attn_mfma.hip, csrc/attn.hip) through the C ABI, every output held per element to the fp64
reference and the derived bound of tests/attn_bounds.py.  Outputs written with accumulate = 0 start as NaN; every buffer carries
sentinel tokens (and the parameter-gradient buffers and the workspace sentinel floats) that no sequence covers and that must come back
bit-unchanged; the inputs must come back bit-unchanged too.

Which case reaches which branch of attn_mfma.hip:

  test_every_instantiation          GO(NB, KS) of bf_attn_fwd_mfma and bf_attn_bwd_mfma, all eight, in bf16 (BF_MODE(0) for (1,2), BF_MODE(-1)
                                    for the others); the same shapes in fp32 (attn.hip).  Even cases pass a full workspace (`ws` branch of
                                    go_bwd_mode, attn_ws_reduce), odd ones ws = NULL (atomics).
  test_generic_kernel_in_bf16       attn.hip on bf16 tensors: d = 24, 40, 72, and d = 64 under bf_debug_force_generic_attn.
  test_accumulate_modes             forward accumulate 1, backward accumulate 1: BF_MODE(1) on (1,2); the run-time mode on (1,1) and (2,3), ragged L.
  test_raw_pair_of_passes           accumulate 2 then 5 against the fp64 axial pair: BF_MODE(2) / BF_MODE(5) on (1,2); run-time modes on (1,1), (1,3)
                                    W + (2,3) H, (2,2) H; mode 2 on NB = 2 (a W pass of 24 tokens: the raw q / k store of the second 16-row block,
                                    read back by mode 5 through old.q[1] / old.k[1]) on (2,2) W + (2,2) H and (2,3) W + (1,3) H; all with clamped rows
                                    (`raw_in && row >= L`); forward accumulate 0 then 1 on the same shapes.
  test_forward_many_problems        about 1.5 - 2 x 2048 problems on 2048 waves: half the waves (all, at 4200) take a second problem, ragged tail:
                                    `cur = nxt`, `more`, locate() of a later problem, the wsync() between problems on (1,2) and (2,2); the
                                    non-prefetch reload on (2,4).
  test_backward_few_workgroups      ws of k rows -> k workgroups loop over all problems (the truncated-ws branch): one_head true (registers) and
                                    false (LDS atomics) with 2 - 15 problems per wave on NB = 1 and NB = 2, the reload path (2,3) / (2,4), k = 1,
                                    waves without a problem; bit-identical run to run; and against a launch with one problem per wave:
                                    out / dqkv bit-identical, parameter sums within the fp32 reordering allowance (about 1e-5).
  test_backward_global_atomics_...  ws = NULL with more problems than twice the resident waves: global atomics after a multi-problem loop;
                                    against the same grid flushing through workspace rows, and against 301 workgroups (another split of the
                                    problems over the waves): out / dqkv bit-identical, parameter sums within the reordering allowance.
  test_axial_one_launch             attn_fwd_axial_mfma<KS, NORM, 12> (frames * heads <= 256), <KS, NORM, 4> with one tile per workgroup (257 .. 768)
                                    and with the tile loop (> 768), NORM false and true, KS 1 .. 4.
  test_hard_inputs                  a nearly one-hot softmax (scores +-30, bias +-8) and rows with a large common offset.
  test_zz_worst_ratios              prints the worst |got - ref| / bnd per output kind seen so far (pytest -s); the table is complete only when the
                                    whole file runs in one process, in file order.
"""
import collections

import pytest
import torch

from tests import attn_bounds as AB

pytestmark = pytest.mark.gpu

SENT = 2                                # sentinel tokens behind every token buffer
TAIL = 4                                # sentinel floats behind every parameter-gradient buffer and the workspace
WORST = collections.defaultdict(float)  # (mode, output) -> worst ratio seen
AX_NAMES = AB.NAMES[:5] + ("dhscale_x", "dhscale_y")


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def make(N, heads, d, dtype, seed, kind="plain", nhs=1):
    """qkv [N + SENT][3 E], dout [N + SENT][E] in dtype and the fp32 parameters (qw, qb, kw, kb, emb, hscale x nhs)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    E, M = heads * d, N + SENT
    gain, embs, spread = (5.5, 8.0, 1.5) if kind == "peaked" else (1.0, 0.5, 4.0 if kind == "offset" else 1.5)
    qkv = r(M, 3 * E) * spread
    if kind == "offset":
        qkv = qkv + 48.0 * (1 + r(M, 3 * heads, 1).abs()).expand(M, 3 * heads, d).reshape(M, 3 * E)
    prm = [gain * (1 + 0.2 * r(d)), 0.2 * r(d), gain * (1 + 0.2 * r(d)), 0.2 * r(d), embs * r(32, heads)] + [1 + 0.3 * r(heads) for _ in range(nhs)]
    return qkv.to(dtype), r(M, E).to(dtype), prm


def grad_buffers(prm):
    """Zeroed gradient buffers with TAIL sentinel floats each."""
    flat = [torch.cat([torch.zeros(t.numel(), device="cuda"), torch.full((TAIL,), 777.0, device="cuda")]) for t in prm]
    return flat, [f[:t.numel()].view(t.shape) for f, t in zip(flat, prm)]


def mode_of(dtype, d, forced=False):
    if dtype == torch.float32:
        return AB.FP32
    return AB.MFMA if d % 32 == 0 and not forced else AB.GENERIC_BF16


class Call:
    """One problem set: buffers, the two C calls, the sentinel / untouched-input checks."""

    def __init__(self, N, heads, d, dtype, seed, kind="plain", nhs=1):
        self.N, self.heads, self.d, self.dtype = N, heads, d, dtype
        self.qkv, self.dout, self.prm = make(N, heads, d, dtype, seed, kind, nhs)
        self.saved = [t.clone() for t in (self.qkv, self.dout, *self.prm)]
        nan = lambda cols: torch.full((N + SENT, cols), float("nan"), device="cuda", dtype=dtype)
        self.out, self.dqkv = nan(heads * d), nan(3 * heads * d)
        self.gflat, self.grads = grad_buffers(self.prm)

    def prefill(self, seed):
        """Old values for the accumulate modes; the sentinel rows stay NaN."""
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.out[:self.N] = torch.randn(self.N, self.out.shape[1], device="cuda", generator=g).to(self.dtype)
        self.dqkv[:self.N] = torch.randn(self.N, self.dqkv.shape[1], device="cuda", generator=g).to(self.dtype)
        return self.out.clone(), self.dqkv.clone()

    def _par(self, with_emb, with_hs, hs_i):
        from bubbleformer_amd.ops import _p
        p = self.prm
        return [_p(t) for t in p[:4]] + [_p(p[4]) if with_emb else None, _p(p[5 + hs_i]) if with_hs else None]

    def fwd(self, geo, with_emb=True, with_hs=True, out_scale=0.5, acc=0, hs_i=0):
        from bubbleformer_amd import _lib as L
        from bubbleformer_amd.ops import _dt, _p, _stream
        L.check(L.lib().bf_attn_fwd(_dt(self.dtype), _p(self.qkv), _p(self.out), *geo, self.heads, self.d, *self._par(with_emb, with_hs, hs_i),
                                    out_scale, acc, _stream()), "bf_attn_fwd")

    def bwd(self, geo, with_emb=True, with_hs=True, out_scale=0.5, acc=0, hs_i=0, ws_rows=None):
        """ws_rows: None = no workspace, k = a workspace of exactly k rows (NaN-filled: the kernel must write what the reduction reads)."""
        from bubbleformer_amd import _lib as L
        from bubbleformer_amd.ops import _dt, _p, _stream
        g = self.grads
        # dhscale is passed even without hscale: it must stay zero.  demb is NULL when emb is: the kernels guard the T5 sums on the demb pointer
        # alone (a non-NULL demb beside emb = NULL receives the gradient of an all-zero table, which is not zero), and no caller passes one
        # without the other, so there is nothing to hold to zero there.
        gp = [_p(t) for t in g[:4]] + [_p(g[4]) if with_emb else None, _p(g[5 + hs_i])]
        nvals = 4 * self.d + 33 * self.heads
        self.ws = None if ws_rows is None else torch.full((ws_rows * nvals + TAIL,), float("nan"), device="cuda")
        L.check(L.lib().bf_attn_bwd(_dt(self.dtype), _p(self.qkv), _p(self.dout), _p(self.dqkv), *geo, self.heads, self.d,
                                    *self._par(with_emb, with_hs, hs_i), *gp, out_scale, acc, None if self.ws is None else _p(self.ws),
                                    0 if self.ws is None else ws_rows * nvals, _stream()), "bf_attn_bwd")

    def untouched(self):
        torch.cuda.synchronize()
        for t, s in zip((self.qkv, self.dout, *self.prm), self.saved):
            assert same_bits(t, s), "an input buffer changed"
        for t in (self.out, self.dqkv):
            assert torch.isnan(t[self.N:].float()).all(), "a sentinel token was written"
        for f in self.gflat:
            assert bool((f[-TAIL:] == 777.0).all()), "a parameter-gradient sentinel was written"
        if getattr(self, "ws", None) is not None:
            assert torch.isnan(self.ws[-TAIL:]).all(), "the workspace sentinel was written"


def hold(res, got, mode, what, names=("sequence", "head", "row", "channel")):
    """Every output of `res` ({name: (ref, bnd)}) against got[name]; records the worst ratios."""
    tag = {AB.MFMA: "bf16 mfma", AB.GENERIC_BF16: "bf16 generic", AB.FP32: "fp32"}[mode]
    for k, (ref, bnd) in res.items():
        w = AB.check(got[k], ref, bnd, f"{what}: {k}", {4: names, 3: ("token", "head", "channel"), 2: ("bucket", "head"), 1: ("index",)}[ref.dim()])
        key = (tag, "dhscale" if k.startswith("dhscale") else k)
        WORST[key] = max(WORST[key], w)
        print(f"{what} [{tag}] {k}: worst ratio {w:.3g}")


def plain_outputs(c, geo, with_bwd=True):
    h, d = c.heads, c.d
    got = {"out": AB.from_tokens(c.out[:c.N], geo, h, 1, d)}
    if with_bwd:
        got.update({n: AB.from_tokens(c.dqkv[:c.N], geo, h, 3, d, i) for i, n in enumerate(("dq", "dk", "dv"))})
        got.update(dict(zip(AB.NAMES, c.grads)))
    return got


def run_plain(L, d, heads, geo, N, dtype, with_emb, with_hs, out_scale, seed, ws_rows, kind="plain", forced=False, accumulate=False):
    from bubbleformer_amd import _lib as Lb
    c = Call(N, heads, d, dtype, seed, kind)
    old_o, old_d = c.prefill(seed + 1) if accumulate else (None, None)
    if forced:
        Lb.lib().bf_debug_force_generic_attn(1)
    try:
        c.fwd(geo, with_emb, with_hs, out_scale, int(accumulate))
        c.bwd(geo, with_emb, with_hs, out_scale, int(accumulate), ws_rows=ws_rows)
        c.untouched()
    finally:
        Lb.lib().bf_debug_force_generic_attn(0)
    mode = mode_of(dtype, d, forced)
    c.reorder = {}
    res = AB.plain(c.qkv[:N], c.dout[:N], geo, heads, d, c.prm, with_emb, with_hs, out_scale, mode,
                   None if old_o is None else old_o[:N], None if old_d is None else old_d[:N], c.reorder)
    hold(res, plain_outputs(c, geo), mode, f"L={L} d={d} heads={heads}")
    if not with_hs:
        assert float(c.grads[5].abs().max()) == 0.0
    return c


EVERY = [  # L, d, heads, geometry, emb, hscale, out_scale: every L, d, heads, geometry and option value, every (NB, KS)
    (1, 32, 1, "contig", True, True, 1.0), (2, 64, 5, "temporal", True, False, 0.5), (3, 96, 6, "W", False, True, 1.0), (4, 128, 16, "H", True, True, 0.5),
    (15, 64, 6, "H", False, False, 1.0), (16, 32, 16, "temporal", True, True, 0.5), (15, 96, 1, "contig", True, True, 0.5), (16, 128, 5, "W", True, True, 1.0),
    (17, 32, 5, "H", True, True, 0.5), (24, 64, 6, "contig", True, False, 1.0), (31, 96, 16, "temporal", False, True, 0.5), (32, 128, 1, "W", True, True, 1.0),
    (17, 128, 6, "temporal", True, True, 0.5), (31, 32, 16, "W", True, True, 1.0), (24, 96, 1, "H", False, False, 0.5), (32, 64, 5, "contig", True, True, 0.5),
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", range(len(EVERY)), ids=[f"L{c[0]}-d{c[1]}-h{c[2]}-{c[3]}" for c in EVERY])
def test_every_instantiation(case, dtype):
    L, d, heads, kind, with_emb, with_hs, out_scale = EVERY[case]
    geo, N = AB.geometry(kind, L, n_outer=2 if heads == 16 else 3, inner=3)
    run_plain(L, d, heads, geo, N, dtype, with_emb, with_hs, out_scale, 500 + case, ws_rows=None if case % 2 else 1024)


@pytest.mark.parametrize("L,d,heads,kind,forced", [(12, 24, 6, "temporal", False), (20, 40, 3, "W", False), (7, 72, 2, "H", False), (16, 64, 6, "contig", True)])
def test_generic_kernel_in_bf16(L, d, heads, kind, forced):
    geo, N = AB.geometry(kind, L, n_outer=3, inner=3)
    run_plain(L, d, heads, geo, N, torch.bfloat16, True, True, 0.5, 600 + L, ws_rows=None, forced=forced)


@pytest.mark.parametrize("L,d,heads,kind", [(12, 64, 6, "temporal"), (7, 32, 3, "H"), (20, 96, 2, "W")])
def test_accumulate_modes(L, d, heads, kind):
    """accumulate = 1 in the forward and the backward: the old stored values are added (0 is every other test)."""
    geo, N = AB.geometry(kind, L, n_outer=3, inner=3)
    run_plain(L, d, heads, geo, N, torch.bfloat16, True, True, 0.5, 700 + L, ws_rows=1024, accumulate=True)


def axial_call(Fr, h, w, heads, d, seed):
    return Call(Fr * h * w, heads, d, torch.bfloat16, seed, nhs=2), AB.axial_geos(Fr, h, w)


@pytest.mark.parametrize("h,w,d,heads", [(12, 12, 64, 6), (3, 7, 32, 3), (24, 7, 96, 2), (20, 12, 64, 2), (20, 24, 64, 2), (7, 24, 96, 2)])
def test_raw_pair_of_passes(h, w, d, heads):
    """Forward accumulate 0 then 1, backward accumulate 2 then 5, against the fp64 gradient of the sum of both passes through the shared
    q / k LayerNorm -- not against the plain modes of the same kernel."""
    Fr = 3
    c, (gW, gH) = axial_call(Fr, h, w, heads, d, 800 + h + w)
    c.fwd(gW, acc=0, hs_i=0)
    c.fwd(gH, acc=1, hs_i=1)
    c.bwd(gW, acc=2, hs_i=0, ws_rows=1024)
    c.bwd(gH, acc=5, hs_i=1, ws_rows=None)
    c.untouched()
    N = c.N
    res = AB.axial_pair(c.qkv[:N], c.dout[:N], Fr, h, w, heads, d, c.prm, AB.MFMA)
    got = {"out": c.out[:N].view(N, heads, d), **{n: c.dqkv[:N].view(N, heads, 3, d)[:, :, i] for i, n in enumerate(("dq", "dk", "dv"))}}
    got.update(dict(zip(AX_NAMES, c.grads)))
    hold(res, got, AB.MFMA, f"axial pair {h}x{w} d={d}")


@pytest.mark.parametrize("L,d,heads,nseq", [(12, 64, 6, 700), (24, 64, 6, 511), (31, 128, 16, 191)])
def test_forward_many_problems(L, d, heads, nseq):
    """The forward launches at most 512 workgroups x 4 waves (go_fwd: 256 CUs x 2): with nseq * heads = 4200 / 3066 / 3056 problems, none a
    multiple of 2048, every wave takes two problems and some a third (4200), or about half the waves take a second one (3066, 3056)."""
    assert nseq * heads > 2048 and (nseq * heads) % 2048
    geo = (nseq, L, 1, L, 0, 1) if L != 24 else (nseq, L, 73, L * 73, 1, 73)      # the NB = 2 prefetch shape on the strided layout
    c = Call(nseq * L, heads, d, torch.bfloat16, 900 + L)
    c.fwd(geo)
    c.untouched()
    res = AB.plain(c.qkv[:c.N], None, geo, heads, d, c.prm, True, True, 0.5, AB.MFMA)
    hold(res, plain_outputs(c, geo, with_bwd=False), AB.MFMA, f"forward {nseq * heads} problems L={L} d={d}")


FEW = [  # L, d, heads, nseq, workspace rows k: stride = k * wpb problems, wpb = 4 (L <= 16) or 2
    (12, 64, 6, 7, 3),      # stride 12 = 2 heads' worth: one_head, 42 problems = 3 full rounds + 6
    (12, 64, 6, 7, 2),      # stride 8: a wave's problems span heads -> LDS atomics per problem; 42 = 5 rounds + 2
    (12, 64, 6, 7, 1),      # k = 1: one workgroup, 10 - 11 problems per wave
    (5, 32, 3, 1, 1),       # 3 problems, 4 waves: one wave takes none
    (17, 96, 6, 5, 6),      # NB = 2 (two waves): stride 12, one_head, 30 = 2 rounds + 6; (2,3) reloads its rows (no look-ahead registers)
    (24, 128, 5, 3, 2),     # stride 4 against 5 heads: LDS atomics; (2,4); 15 = 3 rounds + 3
    (20, 64, 1, 9, 1),      # one head, stride 2: one_head with 4 - 5 problems per wave, (2,2) look-ahead
    (3, 128, 16, 3, 5),     # stride 20 against 16 heads: atomics, (1,4), 48 = 2 rounds + 8
]


@pytest.mark.parametrize("L,d,heads,nseq,k", FEW)
def test_backward_few_workgroups(L, d, heads, nseq, k):
    """grid = ws_floats / nvals (go_bwd_mode): a workspace of k rows makes k workgroups loop over all problems."""
    wpb = 4 if L <= 16 else 2
    assert (nseq * heads) % (k * wpb) and (nseq * heads > k * wpb or k == 1)
    geo = (nseq, L, 1, L, 0, 1)
    a = run_plain(L, d, heads, geo, nseq * L, torch.bfloat16, True, True, 0.5, 1000 + L + k, ws_rows=k)
    b = run_plain(L, d, heads, geo, nseq * L, torch.bfloat16, True, True, 0.5, 1000 + L + k, ws_rows=k)
    assert same_bits(a.dqkv, b.dqkv) and same_bits(a.out, b.out)
    for x, y in zip(a.grads, b.grads):
        assert same_bits(x, y), "parameter gradients through the workspace must not depend on the run"
    one_problem_per_wave(a, L, d, heads, geo, 1000 + L + k)


def one_problem_per_wave(a, L, d, heads, geo, seed):
    """Against a launch in which no wave takes a second problem (a full workspace, few problems): which wave computes a problem must not
    change a bit of its out / dqkv rows, and the parameter gradients are the same per-problem terms added in another order -- they may
    differ by the fp32 reordering allowance of attn_bounds.param_total, about 1e-5 of the sum of their terms, which is far below the
    worst-case bound against fp64 and catches a term that a looping wave drops, doubles or credits to the wrong head."""
    full = run_plain(L, d, heads, geo, a.N, torch.bfloat16, True, True, 0.5, seed, ws_rows=1024)
    assert same_bits(a.dqkv, full.dqkv) and same_bits(a.out, full.out)
    for name, x, y in zip(AB.NAMES, a.grads, full.grads):
        AB.check(x, y.double(), a.reorder[name], f"{name} against one problem per wave", ("bucket", "head") if name == "demb" else ("index",))


def test_backward_global_atomics_beyond_the_resident_set():
    """ws = NULL with every wave looping.  (NB, KS) = (1, 2): a workgroup's LDS is 4 waves x (3 x 16 x (64 + 16) + 2 x 16 x 40) bf16 = 40960 B
    of tiles (go_bwd_mode) + 5248 B of static tables (s_demb 2048, s_dhs 64, s_par 1024, s_emb 2048, s_hsc 64) = 46208 B, so at most
    floor(160 KB / 46208 B) = 3 workgroups fit a CU: at most 256 CUs x 3 x 4 waves = 3072 resident waves.  1101 sequences x 6 heads =
    6606 problems is more than twice that and a multiple of none of the possible strides (1024, 2048, 3072)."""
    L, d, heads, nseq = 12, 64, 6, 1101
    assert nseq * heads > 2 * 3072 and all((nseq * heads) % s for s in (1024, 2048, 3072))
    geo = (nseq, L, 1, L, 0, 1)
    a = run_plain(L, d, heads, geo, nseq * L, torch.bfloat16, True, True, 0.5, 1100, ws_rows=None)
    # 4096 rows do not shrink the grid (go_bwd_mode caps it only when the workspace is too small): the same waves take the same problems and
    # only the flush differs, global atomics against workspace rows + attn_ws_reduce.  301 rows make 301 workgroups: a problem stride of
    # 1204, which is no multiple of 6 heads, so other waves take other problems and the T5 / head-scale sums go through LDS atomics.
    # (Against fp64 the parameter sums of 6606 problems carry the worst-case slack and would not notice one lost term; these two do.)
    for rows in (4096, 301):
        other = run_plain(L, d, heads, geo, nseq * L, torch.bfloat16, True, True, 0.5, 1100, ws_rows=rows)
        assert same_bits(a.dqkv, other.dqkv) and same_bits(a.out, other.out)
        for name, x, y in zip(AB.NAMES, a.grads, other.grads):
            AB.check(x, y.double(), a.reorder[name], f"{name}: atomics against {rows} workspace rows", ("bucket", "head") if name == "demb" else ("index",))


AXIAL = [  # frames, heads, h, w, d: h, w in {1, 5, 9, 12, 16}, every d, the three launch forms
    (7, 6, 12, 12, 64), (5, 3, 5, 9, 32), (3, 2, 1, 16, 96), (2, 16, 16, 16, 128),      # frames * heads <= 256: twelve waves
    (50, 6, 12, 12, 64), (20, 16, 9, 5, 128),                                           # 257 .. 768: four waves, one tile per workgroup
    (130, 6, 5, 9, 32), (49, 16, 16, 1, 96),                                            # > 768: four waves, the tile loop
]


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("Fr,heads,h,w,d", AXIAL)
def test_axial_one_launch(Fr, heads, h, w, d, norm):
    from bubbleformer_amd import _lib as L
    from bubbleformer_amd.ops import _p, _stream
    lib = L.lib()
    c, (gW, gH) = axial_call(Fr, h, w, heads, d, 1200 + Fr)
    N, E, S = c.N, heads * d, h * w
    par = [_p(t) for t in c.prm]
    if norm:
        g = torch.Generator(device="cuda").manual_seed(Fr)
        nw, nb = 1 + 0.2 * torch.randn(E, device="cuda", generator=g), 0.2 * torch.randn(E, device="cuda", generator=g)
        out_n = torch.full_like(c.out, float("nan"))
        stats = [torch.cat([torch.full((Fr * E,), float("nan"), device="cuda"), torch.full((TAIL,), 777.0, device="cuda")]) for _ in range(4)]
        rc = lib.bf_attn_axial_norm_fwd(1, _p(c.qkv), _p(c.out), _p(out_n), Fr, h, w, heads, d, *par, _p(nw), _p(nb), *[_p(s) for s in stats], _stream())
    else:
        rc = lib.bf_attn_axial_fwd(1, _p(c.qkv), _p(c.out), Fr, h, w, heads, d, *par, _stream())
    assert rc == 0
    c.untouched()
    res = AB.axial_pair(c.qkv[:N], None, Fr, h, w, heads, d, c.prm, AB.MFMA)
    hold(res, {"out": c.out[:N].view(N, heads, d)}, AB.MFMA, f"axial one launch {Fr}x{heads} tiles {h}x{w} d={d}")
    two = torch.full_like(c.out, float("nan"))                         # the two-pass path, bit for bit
    L.check(lib.bf_attn_fwd(1, _p(c.qkv), _p(two), *gW, heads, d, *par[:5], par[5], 0.5, 0, _stream()), "w")
    L.check(lib.bf_attn_fwd(1, _p(c.qkv), _p(two), *gH, heads, d, *par[:5], par[6], 0.5, 1, _stream()), "h")
    torch.cuda.synchronize()
    assert same_bits(c.out, two)
    if norm:
        assert torch.isnan(out_n[N:].float()).all() and all(bool((s[-TAIL:] == 777.0).all()) for s in stats)
        resn = AB.instance_norm(c.out[:N], Fr, S, nw, nb)
        got = {"out_n": out_n[:N].view(Fr, S, E), **{n: s[:-TAIL].view(Fr, E) for n, s in zip(("mean", "rstd", "sc", "sh"), stats)}}
        for k, (ref, bnd) in resn.items():
            wr = AB.check(got[k], ref, bnd, f"axial norm {k}", ("frame", "token", "channel"))
            WORST[("bf16 mfma", "norm " + k)] = max(WORST[("bf16 mfma", "norm " + k)], wr)


@pytest.mark.parametrize("kind", ["peaked", "offset"])
@pytest.mark.parametrize("L,d,heads", [(12, 64, 6), (31, 96, 2)])
def test_hard_inputs(kind, L, d, heads):
    """peaked: scores of order +-30 and bias entries of order +-8, a nearly one-hot softmax; offset: rows 48 .. 150 with a spread of 4,
    where the LayerNorm cancels (tests/test_attn_bounds.py shows the bound still rejects the narrowest mutant at both)."""
    geo, N = AB.geometry("temporal", L, n_outer=3, inner=3)
    run_plain(L, d, heads, geo, N, torch.bfloat16, True, True, 0.5, 1300 + L, ws_rows=1024, kind=kind)


def test_zz_worst_ratios():
    """Asserts nothing (every ratio was asserted <= 1 where it was measured): prints the summary DESIGN.md quotes.  It reads what the tests
    above left in WORST, so it is complete only when the whole file runs in one process."""
    for (tag, name), w in sorted(WORST.items()):
        print(f"worst |got - ref| / bnd  {tag:12s} {name:10s} {w:.3g}")
