"""GPU: the whole-frame kernels that fuse a projection with the InstanceNorm beside it (csrc/gemm_frame.hip: the one-frame and the
frame-pair backward, its chain, the forward twin; csrc/frame_fwd.hip: bf_frame_linear's resident and ring forms), every output element
held to the per-element bound of tests/frame_bounds.py.

Operands come from seeded CPU generators; the fp64 references are computed on the device.  Every output (the per-frame partials and the
statistics tables included) is pre-filled with NaN and carries a NaN tail that must stay NaN: every element is written, nothing beyond
it.  Each case asserts from the profiler's report which kernel ran.  The two frames of a workgroup always differ in statistics, factor
and post scale; K covers every residue of the pair kernel's 3-slot ring before and after it wraps, and KB either side of every ring
depth of bf_frame_linear.  The last test prints the worst |got - ref| / bound of each area.

Not reached from here: the scaled second copies (MODE 5, bf_gemm_inbwd_frames_scaled; out2 of bf_gemm_pair_scaled) have no C export
and stay covered through the trunk tests only."""
import ctypes
import itertools
import json
import os

import pytest
import torch

from bubbleformer_amd import _lib as L
from tests import frame_bounds as FB
from tests import norm_bounds as NB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
S = 144
TAIL = 64
WORST = {}


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A failed bound is one failed case; a device error ends the module: nothing more is launched on a device that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, nothing more is launched: {e}", returncode=3)


def _note(area, ratio, case):
    if ratio >= WORST.get(area, (-1.0, ""))[0]:
        WORST[area] = (ratio, case)


def _randn(*shape, scale=1.0, shift=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bf(t):
    """CPU fp64 -> the bf16 tensor on the device."""
    return t.to(BF16).to(DEV)


def _f(t):
    return None if t is None else t.float().to(DEV).contiguous()


def _wide(t, pad):
    """bf16 device tensor t (R, C) as a view into a NaN-filled buffer (R, C + pad)."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


class _Out:
    """An output of `shape`, NaN-filled, row stride shape[-1] + pad, followed by a NaN tail."""

    def __init__(self, shape, dt=BF16, pad=0):
        self.shape, self.pad = tuple(shape), pad
        rows = 1
        for s in shape[:-1]:
            rows *= s
        self.rows, self.ld = rows, shape[-1] + pad
        self.buf = torch.full((rows * self.ld + TAIL,), float("nan"), dtype=dt, device=DEV)

    @property
    def v(self):
        return self.buf[:self.rows * self.ld].view(self.rows, self.ld)[:, :self.shape[-1]].reshape(self.shape) if self.pad else \
            self.buf[:self.rows * self.ld].view(self.shape)

    def ptr(self):
        return self.buf.data_ptr()

    def beyond_ok(self, what):
        torch.cuda.synchronize()
        assert torch.isnan(self.buf[self.rows * self.ld:].float()).all(), (what, "written beyond the end")
        if self.pad:
            assert torch.isnan(self.buf[:self.rows * self.ld].view(self.rows, self.ld)[:, self.shape[-1]:].float()).all(), (what, "written beyond the row extent")

    def untouched(self, what):
        torch.cuda.synchronize()
        assert torch.isnan(self.buf.float()).all(), (what, "a refused call wrote")

    def bits(self):
        return self.buf.view(torch.int16 if self.buf.dtype == BF16 else torch.int32)


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
        assert self.names == [want], (what, "expected", want, "ran", self.names)


def _same_bits(a, b, what):
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x.bits(), y.bits()), (what, "a rerun on the same inputs changed bits")


def _frames_x(Fr, Sf, N, seed):
    """Activation rows whose frames differ clearly in mean and spread -> CPU fp64 (Fr * Sf, N)."""
    x = _randn(Fr, Sf, N, scale=1.5, seed=seed) * (1 + 0.5 * (torch.arange(Fr) % 5)[:, None, None]) + 0.7 * _randn(Fr, 1, N, seed=seed + 1)
    return x.reshape(Fr * Sf, N)


def _stats(x, Fr, Sf):
    """fp32 statistics tables of bf16 device rows x (the GIVEN statistics of a backward: exact inputs whatever they are)."""
    x3 = x.double().view(Fr, Sf, -1)
    return x3.mean(1).float().contiguous(), ((x3.var(1, unbiased=False) + NB.EPS) ** -0.5).float().contiguous()


FACTORS = [1.25, 0.5, 2.0, 0.75, 1.5, 1.0, 0.625]


def _factors(n, zero_at=None):
    f = torch.tensor([FACTORS[i % len(FACTORS)] for i in range(n)], dtype=F32)
    if zero_at is not None:
        f[zero_at] = 0.0
    return f.to(DEV)


# ---------------------------------------------------------------------------------------------------- backward
def run_inbwd(Fr, N, K, Sf=S, with_add=True, fdiv=0, zero_at=None, pad=0, chain=None, cgdiv=1, seed=0, A=None, B=None, x=None, w=None, rerun=False,
              area=None):
    """One bf_gemm_inbwd_frames[_chain] call against the bound -> worst ratio.  fdiv: 0 = no fscale; chain: None | "plain" | "g"."""
    lib = L.lib()
    M = Fr * Sf
    what = f"inbwd Fr{Fr} S{Sf} N{N} K{K} add{int(with_add)} fdiv{fdiv} z{zero_at} pad{pad} chain={chain}/{cgdiv}"
    A = _bf(_randn(M, K, scale=0.5, seed=seed) if A is None else A)
    B = _bf(_randn(K, N, scale=K ** -0.5, seed=seed + 1) if B is None else B)
    x = _bf(_frames_x(Fr, Sf, N, seed + 2) if x is None else x)
    add = _bf(_randn(M, N, seed=seed + 4)) if with_add else None
    w = _f(_randn(N, scale=0.3, shift=1.0, seed=seed + 5) if w is None else w)
    mean, rstd = _stats(x, Fr, Sf)
    Av, Bv = (_wide(A, pad), _wide(B, pad)) if pad else (A, B)
    fs = _factors(-(-Fr // fdiv), zero_at) if fdiv else None
    if chain:
        cz = _bf(_randn(Fr, S, N, scale=0.7, seed=seed + 6) * (1 + (torch.arange(Fr) % 3)[:, None, None]) - 0.2).view(M, N)
        cmean, crstd = _stats(cz, Fr, S)
        cw = _f(_randn(N, scale=0.3, shift=1.0, seed=seed + 7))
        cg = _f(_randn(-(-Fr // cgdiv), N, scale=0.3, shift=1.0, seed=seed + 8)) if chain == "g" else None

    def call():
        o = [_Out((M, N)), _Out((Fr, N, 2), F32)] + ([_Out((M, N)), _Out((Fr, N, 2), F32)] if chain else [])
        with _Prof() as prof:
            if chain:
                rc = lib.bf_gemm_inbwd_frames_chain(1, M, N, K, _p(Av), Av.stride(0), _p(Bv), Bv.stride(0), _p(x), _p(add), o[0].ptr(), Sf, _p(mean), _p(rstd),
                                                    _p(w), o[1].ptr(), _p(fs), max(fdiv, 1), _p(cz), o[2].ptr(), _p(cmean), _p(crstd), _p(cw), _p(cg), cgdiv,
                                                    o[3].ptr(), _stream())
            else:
                rc = lib.bf_gemm_inbwd_frames(1, M, N, K, _p(Av), Av.stride(0), _p(Bv), Bv.stride(0), _p(x), _p(add), o[0].ptr(), Sf, _p(mean), _p(rstd),
                                              _p(w), o[1].ptr(), _p(fs), max(fdiv, 1), _stream())
        assert rc == 0, (what, "rc", rc)
        prof.ran(FB.inbwd_path(M, N, K, Sf, chain=bool(chain)), what)
        return o

    o = call()
    fexp = None if fs is None else fs[torch.arange(Fr, device=DEV) // fdiv]
    r = FB.inbwd(A, B, x, mean, rstd, w, Sf, add, fexp)
    wdx, wws = FB.check(o[0].v, *r["dx"], what + " dx", ("row", "col")), FB.check(o[1].v, *r["ws"], what + " ws", ("frame", "col", "sum"))
    worst = max(wdx, wws)
    if zero_at is not None:      # the dropped frames: out is `add` to the bit (or +-0), the partials +-0
        for f in range(Fr):
            if f // fdiv == zero_at:
                rows = slice(f * Sf, (f + 1) * Sf)
                assert torch.equal(o[0].v[rows], add[rows]) if with_add else bool((o[0].v[rows] == 0).all()), (what, "dropped frame", f)
                assert bool((o[1].v[f] == 0).all()) and float(r["ws"][1][f].max()) == 0.0, (what, "partials of dropped frame", f)
    if chain:
        cgx = None if cg is None else cg[torch.arange(Fr, device=DEV) // cgdiv]
        rc_ = FB.chain(o[0].v, cz, cmean, crstd, cw, cgx)
        _note("chain: cdz", FB.check(o[2].v, *rc_["cdz"], what + " cdz", ("row", "col")), what)
        _note("chain: cws", FB.check(o[3].v, *rc_["cws"], what + " cws", ("frame", "col", "sum")), what)
    for t in o:
        t.beyond_ok(what)
    if rerun:
        _same_bits(o, call(), what)
    if area:
        _note(area + ": dx", wdx, what)
        _note(area + ": ws", wws, what)
    return worst


ONE, PAIR, WHOLE = "backward, one-frame kernel", "backward, pair kernel", "backward, 288-token frames"


@pytest.mark.parametrize("K", [64, 128, 192])
def test_backward_one_frame_kernel(K):
    """Odd frame counts: gemm_inbwd_frames_kernel, nk = 1, 2, 3; one and three column blocks; with / without add and fscale (fdiv 1 and 3)."""
    for i, (Fr, N) in enumerate(itertools.product([1, 3, 5], [128, 384])):
        run_inbwd(Fr, N, K, with_add=i % 2 == 0, fdiv=(0, 1, 3)[(i + K // 64) % 3], seed=10 * i + K, area=ONE)


@pytest.mark.parametrize("K", [64, 128, 192, 256, 320, 384])
def test_backward_pair_kernel_every_ring_residue(K):
    """Frame pairs: nk = 1 .. 6 (the x rows' slot comes out of the ring's wrap-around at each residue of nk mod 3), grids of 1 .. 9 workgroups;
    with / without add; fscale with fdiv 1 and 3 so that the two frames of a workgroup take different factors."""
    for i, (Fr, N) in enumerate(itertools.product([2, 4, 6], [128, 256, 384])):
        run_inbwd(Fr, N, K, with_add=(i + K // 64) % 2 == 0, fdiv=(1, 3, 0)[(i + K // 64) % 3], seed=10 * i + K, area=PAIR)


def test_backward_pair_kernel_on_a_grid_of_eight():
    """8 workgroups: xcd_remap deals a multiple of 8 differently from 1, 3 and 9."""
    run_inbwd(8, 256, 128, fdiv=3, seed=3, area=PAIR)
    run_inbwd(16, 128, 192, with_add=False, seed=4, area=PAIR)


@pytest.mark.parametrize("kernel", ["one", "pair"])
def test_backward_grid_larger_than_the_device(kernel):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    Fr = (cus + 1) | 1 if kernel == "one" else 2 * (cus + 1)
    assert FB.inbwd_grid(Fr * S, 128, S) > cus
    run_inbwd(Fr, 128, 64, fdiv=3, seed=5, area=ONE if kernel == "one" else PAIR)


@pytest.mark.parametrize("Fr,N,K", [(3, 128, 128), (1, 384, 64), (2, 128, 64), (4, 256, 256), (6, 384, 320)])
def test_backward_padded_leading_dimensions(Fr, N, K):
    """lda and ldb 64 longer than the extents, as views into NaN-filled buffers: a read past an extent poisons the output."""
    run_inbwd(Fr, N, K, pad=64, fdiv=1, seed=6, area=ONE if Fr % 2 else PAIR)
    run_inbwd(Fr, N, K, pad=64, with_add=False, seed=7, area=ONE if Fr % 2 else PAIR)


@pytest.mark.parametrize("Fr,fdiv,zero_at", [(3, 1, 1), (5, 3, 0), (2, 1, 1), (2, 1, 0), (6, 3, 1), (4, 3, 0)])
@pytest.mark.parametrize("with_add", [True, False])
def test_backward_zero_factor_drops_a_frame_exactly(Fr, fdiv, zero_at, with_add):
    run_inbwd(Fr, 128, 192, with_add=with_add, fdiv=fdiv, zero_at=zero_at, seed=8, area=ONE if Fr % 2 else PAIR)


@pytest.mark.parametrize("Fr", [1, 2, 3])
@pytest.mark.parametrize("fdiv", [0, 1])
def test_backward_whole_288_token_frames(Fr, fdiv):
    """One 288-token frame per workgroup: the two wave groups hold its halves and exchange their sums through the last step's slot."""
    for i, (N, K) in enumerate([(128, 64), (384, 192), (128, 256), (256, 128)]):
        run_inbwd(Fr, N, K, Sf=288, with_add=i % 2 == 0, fdiv=fdiv, zero_at=0 if (fdiv and i == 1) else None, seed=20 + i, area=WHOLE)
    run_inbwd(Fr, 128, 320, Sf=288, pad=64, fdiv=fdiv, seed=29, area=WHOLE)


@pytest.mark.parametrize("Fr", [2, 4])
@pytest.mark.parametrize("chain,cgdiv", [("plain", 1), ("g", 1), ("g", 2)])
def test_chain(Fr, chain, cgdiv):
    """MODE 2: cdz / cws judged on the kernel's own stored rows; at cgdiv = 1 the post-scale group boundary falls inside every pair."""
    for i, (N, K) in enumerate([(128, 64), (256, 128), (128, 192), (384, 256), (128, 320)]):
        run_inbwd(Fr, N, K, with_add=i % 2 == 0, fdiv=(0, 1, 3)[i % 3], chain=chain, cgdiv=cgdiv, pad=64 if i == 2 else 0, seed=30 + i, area="chain")


# ---------------------------------------------------------------------------------------------------- forward twin
def run_fwd(Fr, N, K, bias, cs, fdiv, with_add, n1, n2, seed=0, A=None, Bt=None, bias_v=None, rerun=False, area="forward twin"):
    """n1: None | (g: None | gdiv, with_resid)."""
    lib = L.lib()
    M = Fr * S
    what = f"fwd Fr{Fr} N{N} K{K} b{int(bias)} cs{int(cs)} fdiv{fdiv} add{int(with_add)} n1={n1} n2={int(n2)}"
    A = _bf(_randn(M, K, scale=0.7, seed=seed) * (1 + (torch.arange(M) // S % 3)[:, None]) if A is None else A)
    Bt = _bf(_randn(K, N, scale=K ** -0.5, seed=seed + 1) if Bt is None else Bt)
    vec = lambda sd, **kw: _f(_randn(N, seed=seed + sd, **kw))
    bias_t = (vec(2, scale=0.5) if bias_v is None else _f(bias_v)) if bias else None
    cs_t, ch_t = (vec(3, scale=0.3, shift=1.0), vec(4, scale=0.3)) if cs else (None, None)
    fs = _factors(-(-Fr // fdiv)) if fdiv else None
    add = _bf(_randn(M, N, scale=1.3, shift=0.2, seed=seed + 5)) if with_add else None
    g = resid = None
    gdiv = 1
    if n1 is not None:
        gdiv, with_resid = n1[0] or 1, n1[1]
        g = _f(_randn(-(-Fr // gdiv), N, scale=0.3, shift=1.0, seed=seed + 6)) if n1[0] else None
        resid = _bf(_randn(M, N, scale=1.3, seed=seed + 7)) if with_resid else None
        w1, b1 = vec(8, scale=0.3, shift=1.0), vec(9, scale=0.3)
    if n2:
        w2, b2 = vec(10, scale=0.3, shift=1.0), vec(11, scale=0.3)

    def call():
        o = dict(out=_Out((M, N)))
        rec1 = rec2 = None
        if n1 is not None:
            o.update({k: _Out((Fr, N), F32) for k in ("n1_mean", "n1_rstd", "n1_sc", "n1_sh")}, n1_out=_Out((M, N)))
            rec1 = L.FrameNorm(_p(w1), _p(b1), _p(g), gdiv, o["n1_mean"].ptr(), o["n1_rstd"].ptr(), o["n1_sc"].ptr(), o["n1_sh"].ptr(), _p(resid), o["n1_out"].ptr())
        if n2:
            o.update({k: _Out((Fr, N), F32) for k in ("n2_mean", "n2_rstd", "n2_sc", "n2_sh")}, n2_out=_Out((M, N)))
            rec2 = L.FrameNorm(_p(w2), _p(b2), None, 1, o["n2_mean"].ptr(), o["n2_rstd"].ptr(), o["n2_sc"].ptr(), o["n2_sh"].ptr(), None, o["n2_out"].ptr())
        with _Prof() as prof:
            rc = lib.bf_gemm_fwd_frames(1, M, N, K, _p(A), K, _p(Bt), N, _p(bias_t), _p(cs_t), _p(ch_t), _p(fs), max(fdiv, 1), _p(add), o["out"].ptr(), S,
                                        ctypes.byref(rec1) if rec1 is not None else None, ctypes.byref(rec2) if rec2 is not None else None, _stream())
        assert rc == 0, (what, "rc", rc)
        prof.ran(FB.fwd_path(M, N, K, S, n1 is not None, n2), what)
        return o

    o = call()
    fexp = None if fs is None else fs[torch.arange(Fr, device=DEV) // fdiv]
    worst = FB.check(o["out"].v, *FB.fwd_out(A, Bt, bias_t, cs_t, ch_t, fexp, add), what + " out", ("row", "col"))
    last = o["out"].v

    def norm(tag, w, b, gx, res):
        nonlocal last, worst
        st = FB.fwd_norm(last, w, b, gx)
        for k in ("mean", "rstd", "sc", "sh"):
            r = FB.check(o[f"{tag}_{k}"].v, *st[k], f"{what} {tag}.{k}", ("frame", "col"))
            _note(f"forward twin: {k}", r, what)
        r = FB.check(o[tag + "_out"].v, *FB.fwd_apply(last, o[tag + "_sc"].v, o[tag + "_sh"].v, res), f"{what} {tag}.out", ("row", "col"))
        _note("forward twin: normalised rows", r, what)
        last = o[tag + "_out"].v

    if n1 is not None:
        norm("n1", w1, b1, None if g is None else g[torch.arange(Fr, device=DEV) // gdiv], resid)
    if n2:
        norm("n2", w2, b2, None, None)
    for k, t in o.items():
        t.beyond_ok(what + " " + k)
    if rerun:
        o2 = call()
        _same_bits([o[k] for k in sorted(o)], [o2[k] for k in sorted(o2)], what)
    _note(area + ": out", worst, what)
    return worst


FWD_SHAPES = [(Fr, N, K) for Fr in (2, 4) for N in (128, 384) for K in (128, 192, 256, 320)]
N1_KINDS = [None] + [(g, r) for g in (None, 1, 2) for r in (False, True)]


@pytest.mark.parametrize("n1", N1_KINDS, ids=lambda k: "none" if k is None else f"g{k[0]}-resid{int(k[1])}")
def test_forward_twin_every_accepted_combination(n1):
    """bias x colscale / colshift x fscale (fdiv 1 and 3, only with colscale: the entry refuses it otherwise) x add x n2 for this n1 form,
    the shapes dealt round-robin; `add` together with n1->resid (the load path of stage B that no other test reaches) is among them."""
    combos = [(b, cs, fd, ad, n2) for b in (False, True) for cs in (False, True) for fd in ((0, 1, 3) if cs else (0,)) for ad in (False, True)
              for n2 in (False, True)]
    for i, (b, cs, fd, ad, n2) in enumerate(combos):
        Fr, N, K = FWD_SHAPES[(i + N1_KINDS.index(n1) * 5) % len(FWD_SHAPES)]
        run_fwd(Fr, N, K, b, cs, fd, ad, n1, n2, seed=100 + i)


@pytest.mark.parametrize("Fr,N,K", FWD_SHAPES)
def test_forward_twin_add_with_norm_residual_at_every_shape(Fr, N, K):
    run_fwd(Fr, N, K, True, True, 1, True, (1, True), True, seed=7)
    run_fwd(Fr, N, K, False, False, 0, True, (2, True), False, seed=8)


# ---------------------------------------------------------------------------------------------------- bf_frame_linear
def run_linear(frames, N, K, form, nxt=True, pad=64, seed=0, A=None, W=None, bias_v=None, rerun=False, area=None):
    """form: "norm_bias" | "norm_fold_resid" | "plain_fold_resid" | "gelu" | "bias_resid" | "en"."""
    lib = L.lib()
    M = frames * S
    what = f"frame_linear frames{frames} N{N} K{K} {form} next{int(nxt)} pad{pad}"
    A = _bf(_randn(M, K, scale=1.5, seed=seed) * (1 + 0.5 * (torch.arange(M) // S % 4)[:, None]) + 0.7 * _randn(1, K, seed=seed + 1) if A is None else A)
    W = _bf(_randn(N, K, scale=K ** -0.5, seed=seed + 2) if W is None else W)
    vec = lambda n, sd, **kw: _f(_randn(n, seed=seed + sd, **kw))
    norm = (vec(K, 3, scale=0.3, shift=1.0), vec(K, 4, scale=0.3)) if form.startswith("norm") else None
    bias = (vec(N, 5, scale=0.5) if bias_v is None else _f(bias_v)) if form in ("norm_bias", "gelu", "bias_resid", "en") else None
    cs, ch = (vec(N, 6, scale=0.3, shift=1.0), vec(N, 7, scale=0.3)) if "fold" in form else (None, None)
    resid = _bf(_randn(M, N, scale=1.2, seed=seed + 8)) if form in ("norm_fold_resid", "plain_fold_resid", "bias_resid", "en") else None
    en = (vec(N, 9, scale=0.3, shift=1.0), vec(N, 10, scale=0.3), vec(N, 11, scale=0.5)) if form == "en" else None
    nx = (vec(N, 12, scale=0.3, shift=1.0), vec(N, 13, scale=0.3)) if nxt else None
    Av, Wv = _wide(A, pad), _wide(W, pad)
    Rv = None if resid is None else _wide(resid, pad)
    nn = lambda t, i: None if t is None else _p(t[i])

    def call():
        o = [_Out((M, N), pad=pad)] + ([_Out((M, N), pad=pad)] if nxt else [])
        with _Prof() as prof:
            rc = lib.bf_frame_linear(1, frames, S, K, N, _p(Av), Av.stride(0), _p(Wv), Wv.stride(0), nn(norm, 0), nn(norm, 1), _p(bias), _p(cs), _p(ch), _p(Rv),
                                     Rv.stride(0) if Rv is not None else 0, int(form == "gelu"), nn(en, 0), nn(en, 1), nn(en, 2), o[0].ptr(), o[0].ld,
                                     nn(nx, 0), nn(nx, 1), o[1].ptr() if nxt else None, o[1].ld if nxt else 0, _stream())
        assert rc == 0, (what, "rc", rc)
        prof.ran(FB.frame_linear_path(frames, N, K, norm is not None, en is not None), what)
        return o

    o = call()
    worst = FB.check(o[0].v, *FB.frame_linear(A, W, norm, bias, cs, ch, resid, form == "gelu", en), what, ("row", "col"))
    if nxt:
        _note("frame_linear: next norm", FB.check(o[1].v, *FB.frame_linear_next(o[0].v, *nx), what + " out_n", ("row", "col")), what)
    for t in o:
        t.beyond_ok(what)
    if rerun:
        _same_bits(o, call(), what)
    _note(area or ("frame_linear: " + ("resident" if K == 384 and form != "en" else "ring") + (", norm in front" if norm else ", norm behind" if en else "")), worst, what)
    return worst


BLOCKS = [(1, 32), (2, 32), (180, 64), (180, 96)]          # (frames, N) -> bn32, bn32, bn64, bn96 through the ntc rule itself


@pytest.mark.parametrize("frames,N", BLOCKS)
def test_frame_linear_resident_form(frames, N):
    assert "BF_FRAME_NTC" not in os.environ
    for form in ("norm_bias", "norm_fold_resid", "plain_fold_resid", "gelu"):
        run_linear(frames, N, 384, form, seed=200)
    run_linear(frames, N, 384, "norm_bias", nxt=False, pad=0, seed=201)
    run_linear(frames, N, 384, "gelu", nxt=False, pad=0, seed=202)


@pytest.mark.parametrize("frames,N", BLOCKS)
@pytest.mark.parametrize("K", [128, 320, 384, 448, 512, 576])
def test_frame_linear_ring_either_side_of_its_depth(frames, N, K):
    """KB = 2, 5, 6, 7, 8, 9 against ring depths of 7 / 6 / 5 slots (column blocks of 32 / 64 / 96): fewer blocks than slots, as many,
    one more, and the ring refilled several times.  K = 384 reaches the ring only with the norm behind."""
    assert "BF_FRAME_NTC" not in os.environ
    for form in (("en",) if K == 384 else ("plain_fold_resid", "gelu", "bias_resid", "en")):
        run_linear(frames, N, K, form, seed=210 + K // 64)
    run_linear(frames, N, K, "en", nxt=False, pad=0, seed=220)
    if K != 384:
        run_linear(frames, N, K, "bias_resid", nxt=False, pad=0, seed=221)


# ---------------------------------------------------------------------------------------------------- hard inputs
def _far_mean(rows, cols, seed):
    """|mean| / std ~ 1000 in bf16-representable values: 1024 + 8 k, k Bernoulli with 8 sqrt(p (1 - p)) = 1.024."""
    g = torch.Generator().manual_seed(seed)
    return 1024.0 + 8.0 * (torch.rand(rows, cols, generator=g, dtype=torch.float64) < 0.0167).double()


def _decades(n):
    """Column scales six decades apart inside every 8-column group."""
    return 10.0 ** ((torch.arange(n) % 8).double() * (6.0 / 7.0) - 3.0)


@pytest.mark.parametrize("Fr,Sf", [(3, 144), (2, 144), (1, 288)])
@pytest.mark.parametrize("kind", ["far_mean", "constant_channel", "decades", "dy_constant", "dy_like_xhat"])
def test_backward_hard_inputs(Fr, Sf, kind):
    N, K, M = 128, 128, Fr * Sf
    kw = {}
    if kind == "far_mean":
        kw["x"] = _far_mean(M, N, 1)
    elif kind == "constant_channel":
        x = _frames_x(Fr, Sf, N, 2)
        x[:, 5] = 3.0
        x[:Sf, 17] = -0.5
        kw["x"] = x
    elif kind == "decades":
        kw["x"] = _frames_x(Fr, Sf, N, 3) * _decades(N)
        kw["B"] = _randn(K, N, scale=K ** -0.5, seed=4) * _decades(N).flip(0)
    elif kind == "dy_constant":      # every row of a frame the same: dy - s1 / S cancels, s2 ~ 0
        kw["A"] = _randn(Fr, 1, K, scale=0.5, seed=5).expand(Fr, Sf, K).reshape(M, K)
    else:                            # A = xhat, B = c I: dy = c xhat, dx cancels to the rounding of xhat
        x = _frames_x(Fr, Sf, N, 6).to(BF16).double().view(Fr, Sf, N)
        kw["x"] = x.reshape(M, N)
        kw["A"] = ((x - x.mean(1, keepdim=True)) * (x.var(1, unbiased=False, keepdim=True) + NB.EPS) ** -0.5).reshape(M, N)
        kw["B"] = 0.5 * torch.eye(N, dtype=torch.float64)
    area = "hard inputs: backward" + (" (288)" if Sf == 288 else " (pair)" if Fr % 2 == 0 else " (one-frame)")
    run_inbwd(Fr, N, K, Sf=Sf, fdiv=1, seed=40, area=area, **kw)
    run_inbwd(Fr, N, K, Sf=Sf, with_add=False, seed=41, area=area, **kw)
    if Sf == 144 and Fr == 2:
        run_inbwd(Fr, N, K, chain="g", seed=42, area=area, **kw)


@pytest.mark.parametrize("kind", ["far_mean", "constant_channel", "decades", "cancel"])
def test_forward_hard_inputs(kind):
    Fr, N, K, M = 2, 128, 128, 2 * S
    kw = {}
    if kind == "far_mean":           # the rows the folded norms see sit at 1024 with a spread of about 1
        kw["bias_v"] = torch.full((N,), 1024.0, dtype=torch.float64)
        kw["A"] = _randn(M, K, scale=1.0, seed=1)
    elif kind == "constant_channel":
        Bt = _randn(K, N, scale=K ** -0.5, seed=2)
        Bt[:, 9] = 0.0
        kw["Bt"] = Bt
    elif kind == "decades":
        kw["Bt"] = _randn(K, N, scale=K ** -0.5, seed=3) * _decades(N)
    else:                            # a [a, -a] against b [b, b]: every product has its negative in the same sum
        a, b = _randn(M, K // 2, scale=0.7, shift=3.0, seed=4), _randn(K // 2, N, scale=0.2, seed=5)
        kw["A"], kw["Bt"] = torch.cat([a, -a], 1), torch.cat([b, b], 0)
    run_fwd(Fr, N, K, True, True, 1, True, (1, True), True, seed=50, area="hard inputs: forward twin", **kw)
    run_fwd(Fr, N, K, True, False, 0, False, (None, False), True, seed=51, area="hard inputs: forward twin", **kw)


@pytest.mark.parametrize("kind", ["far_mean", "constant_channel", "decades", "cancel"])
def test_frame_linear_hard_inputs(kind):
    frames, N, M = 2, 64, 2 * S
    for K, forms in ((384, ("norm_bias", "norm_fold_resid")), (448, ("en", "gelu"))):
        kw = {}
        if kind == "far_mean":
            kw["A"] = _far_mean(M, K, 1) if K == 384 else _randn(M, K, seed=1)
            kw["bias_v"] = torch.full((N,), 1024.0, dtype=torch.float64)
        elif kind == "constant_channel":
            A = _randn(M, K, scale=1.5, seed=2)
            A[:, 11] = 2.0
            W = _randn(N, K, scale=K ** -0.5, seed=3)
            W[13] = 0.0
            kw["A"], kw["W"] = A, W
        elif kind == "decades":
            kw["A"] = _randn(M, K, scale=1.5, seed=4) * _decades(K)
            kw["W"] = _randn(N, K, scale=K ** -0.5, seed=5) * _decades(N)[:, None]
        else:
            a, b = _randn(M, K // 2, scale=0.7, shift=3.0, seed=6), _randn(N, K // 2, scale=0.2, seed=7)
            kw["A"], kw["W"] = torch.cat([a, -a], 1), torch.cat([b, b], 1)
        for form in forms:
            run_linear(frames, N, K, form, seed=60, area="hard inputs: frame_linear", **kw)


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    """Every refusal the entry points make before launching: rc = 1, no kernel in the profiler's report, every output still NaN."""
    lib = L.lib()
    Fr, N, K = 2, 128, 128
    M = Fr * S
    A, B, x = _bf(_randn(M, K, seed=1)), _bf(_randn(K, N, seed=2)), _bf(_randn(M, N, seed=3))
    mean, rstd = _stats(x, Fr, S)
    w = _f(_randn(N, seed=4))
    g = _f(_randn(Fr, N, seed=5))
    A32, B32, x32 = A.float(), B.float(), x.float()
    out, ws, dz, cws = _Out((M, N)), _Out((Fr, N, 2), F32), _Out((M, N)), _Out((Fr, N, 2), F32)
    out32 = _Out((M, N), F32)

    def bwd(dt=1, M_=M, N_=N, K_=K, S_=S, a=A, b=B, xx=x, o=out):
        return lib.bf_gemm_inbwd_frames(dt, M_, N_, K_, _p(a), K, _p(b), N, _p(xx), None, o.ptr(), S_, _p(mean), _p(rstd), _p(w), ws.ptr(), None, 1, _stream())

    def chain(M_=M, S_=S, cg=None):
        return lib.bf_gemm_inbwd_frames_chain(1, M_, N, K, _p(A), K, _p(B), N, _p(x), None, out.ptr(), S_, _p(mean), _p(rstd), _p(w), ws.ptr(), None, 1,
                                              _p(x), dz.ptr(), _p(mean), _p(rstd), _p(w), _p(cg), 1, cws.ptr(), _stream())

    st = [_Out((Fr, N), F32) for _ in range(8)]
    o1, o2 = _Out((M, N)), _Out((M, N))

    def fwd(dt=1, M_=M, N_=N, K_=K, S_=S, fs=None, n2g=None, n2r=None, with_n2=False):
        n1 = L.FrameNorm(_p(w), _p(w), None, 1, st[0].ptr(), st[1].ptr(), st[2].ptr(), st[3].ptr(), None, o1.ptr())
        n2 = L.FrameNorm(_p(w), _p(w), _p(n2g), 1, st[4].ptr(), st[5].ptr(), st[6].ptr(), st[7].ptr(), _p(n2r), o2.ptr())
        return lib.bf_gemm_fwd_frames(dt, M_, N_, K_, _p(A), K, _p(B), N, None, None, None, _p(fs), 1, None, out.ptr(), S_, ctypes.byref(n1),
                                      ctypes.byref(n2) if with_n2 else None, _stream())

    lo, ln = _Out((M, 32)), _Out((M, 32))

    def lin(dt=1, S_=S, K_=K, N_=32, norm=False, a=A):
        return lib.bf_frame_linear(dt, Fr, S_, K_, N_, _p(a), K, _p(B), K, _p(w) if norm else None, _p(w) if norm else None, None, None, None, None, 0, 0,
                                   None, None, None, lo.ptr(), 32, _p(w), _p(w), ln.ptr(), 32, _stream())

    cases = {
        "inbwd fp32": lambda: bwd(dt=0, a=A32, b=B32, xx=x32, o=out32),
        "inbwd S = 72": lambda: bwd(S_=72),
        "inbwd S = 143": lambda: bwd(M_=143 * 2, S_=143),
        "inbwd ragged M": lambda: bwd(M_=M - 8),
        "inbwd N % 128": lambda: bwd(N_=64),
        "inbwd K % 64": lambda: bwd(K_=96),
        "inbwd K = 0": lambda: bwd(K_=0),
        "chain on 288-token frames": lambda: chain(S_=288),
        "chain on an odd frame count": lambda: chain(M_=S),
        "fwd fp32": lambda: fwd(dt=0),
        "fwd S = 288": lambda: fwd(S_=288),
        "fwd odd frame count": lambda: fwd(M_=S),
        "fwd N % 128": lambda: fwd(N_=64),
        "fwd K % 64": lambda: fwd(K_=96),
        "fwd K < 128": lambda: fwd(K_=64),
        "fwd fscale without colscale": lambda: fwd(fs=w),
        "fwd chained norm with g": lambda: fwd(n2g=g, with_n2=True),
        "fwd chained norm with resid": lambda: fwd(n2r=x, with_n2=True),
        "linear fp32": lambda: lin(dt=0, a=A32),
        "linear S = 288": lambda: lin(S_=288),
        "linear N % 32": lambda: lin(N_=48),
        "linear K % 64": lambda: lin(K_=96),
        "linear K < 128": lambda: lin(K_=64),
        "linear norm in front off K = 384": lambda: lin(norm=True),
    }
    for name, fn in cases.items():
        with _Prof() as prof:
            rc = fn()
        assert rc == 1, (name, "rc", rc)
        assert prof.names == [], (name, "launched", prof.names)
    for t in [out, out32, ws, dz, cws, o1, o2, lo, ln] + st:
        t.untouched("refusals")


# ---------------------------------------------------------------------------------------------------- reruns
def test_one_rerun_per_kernel_changes_no_bit():
    run_inbwd(3, 128, 192, fdiv=1, seed=70, rerun=True)
    run_inbwd(4, 256, 320, fdiv=3, seed=71, rerun=True)
    run_inbwd(2, 128, 256, Sf=288, fdiv=1, seed=72, rerun=True)
    run_inbwd(4, 128, 256, chain="g", seed=73, rerun=True)
    run_fwd(4, 128, 256, True, True, 3, True, (1, True), True, seed=74, rerun=True)
    run_fwd(2, 128, 192, True, False, 0, False, None, True, seed=75, rerun=True)
    run_linear(2, 32, 384, "norm_fold_resid", seed=76, rerun=True)
    run_linear(2, 32, 384, "plain_fold_resid", seed=77, rerun=True)
    run_linear(2, 32, 576, "en", seed=78, rerun=True)


# ---------------------------------------------------------------------------------------------------- report
def test_report_worst_ratios(capsys):
    """Last in the module: prints the worst |got - ref| / bound of each area the tests above reached (all are <= 1, or they failed)."""
    assert all(r <= 1.0 for r, _ in WORST.values())
    with capsys.disabled():
        print("\nworst |got - ref| / bound per area:")
        for area, (r, case) in sorted(WORST.items()):
            print(f"  {area:42s} {r:.3e}  ({case})")
