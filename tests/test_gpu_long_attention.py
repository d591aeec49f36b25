"""Long-axis attention (33 <= L <= 128, csrc/attn_long.hip) through the C ABI: bf_attn_fwd / bf_attn_bwd against an fp64 torch
restatement of the same contract (layers/attention.py:80-119, 212-297: q / k LayerNorm, q k^T d^-1/2 + T5 bias, softmax, high-frequency
rescale, P V), the bf16 mode against the fp32 mode, the accumulate and raw-gradient modes, reproducibility and the T5 buckets."""
import os

import numpy as np
import pytest
import torch

from tests.attn_bounds import geometry, reference, t5_bucket, token_index  # noqa: F401  (the fp64 restatement, shared with the short axes)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("dqw", "dqb", "dkw", "dkb", "demb", "dhscale")


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def params(d, heads, g):
    return [1 + 0.2 * torch.randn(d, device="cuda", generator=g), 0.2 * torch.randn(d, device="cuda", generator=g),
            1 + 0.2 * torch.randn(d, device="cuda", generator=g), 0.2 * torch.randn(d, device="cuda", generator=g),
            0.5 * torch.randn(32, heads, device="cuda", generator=g), 1 + 0.3 * torch.randn(heads, device="cuda", generator=g)]


def run(qkv, dout, geo, heads, d, prm, with_emb=True, with_hs=True, out_scale=0.5, acc=(0, 0), out=None, dqkv=None, ws=True):
    """bf_attn_fwd + bf_attn_bwd; returns (out, dqkv, parameter gradients)."""
    from bubbleformer_amd import _lib as L
    from bubbleformer_amd.ops import _dt, _p, _stream
    h = L.lib()
    E = heads * d
    out = torch.zeros(qkv.shape[0], E, device="cuda", dtype=qkv.dtype) if out is None else out
    dqkv = torch.zeros_like(qkv) if dqkv is None else dqkv
    grads = [torch.zeros_like(t) for t in prm]
    p = [_p(t) for t in prm[:4]] + [_p(prm[4]) if with_emb else None, _p(prm[5]) if with_hs else None]
    gp = [_p(t) for t in grads[:4]] + [_p(grads[4]) if with_emb else None, _p(grads[5]) if with_hs else None]
    wsb = torch.zeros(1024 * (4 * 128 + 33 * 16), device="cuda") if ws else None
    L.check(h.bf_attn_fwd(_dt(qkv.dtype), _p(qkv), _p(out), *geo, heads, d, *p, out_scale, acc[0], _stream()), "bf_attn_fwd")
    L.check(h.bf_attn_bwd(_dt(qkv.dtype), _p(qkv), _p(dout), _p(dqkv), *geo, heads, d, *p, *gp, out_scale, acc[1],
                          _p(wsb) if ws else None, wsb.numel() if ws else 0, _stream()), "bf_attn_bwd")
    torch.cuda.synchronize()
    return out, dqkv, grads


def inputs(N, heads, d, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    E = heads * d
    qkv = (torch.randn(N, 3 * E, device="cuda", generator=g) * 1.5).to(dtype)
    dout = torch.randn(N, E, device="cuda", generator=g).to(dtype)
    return qkv, dout, params(d, heads, g)


CASES = [  # L, d, heads, geometry, emb, hscale
    (33, 32, 1, "contig", True, True), (47, 24, 6, "temporal", True, True), (64, 64, 6, "W", True, True), (64, 128, 1, "H", False, True),
    (65, 32, 16, "contig", True, False), (100, 64, 6, "H", True, True), (128, 24, 6, "W", False, False), (128, 128, 16, "temporal", True, True),
    (128, 64, 1, "contig", True, True), (100, 128, 6, "W", True, False),
]


@pytest.mark.parametrize("L,d,heads,kind,with_emb,with_hs", CASES)
def test_long_attention_fp32_matches_fp64(L, d, heads, kind, with_emb, with_hs):
    geo, N = geometry(kind, L, n_outer=2 if heads == 16 else 3, inner=3)
    qkv, dout, prm = inputs(N, heads, d, torch.float32, 1000 + L + d + heads)
    out, dqkv, grads = run(qkv, dout, geo, heads, d, prm, with_emb, with_hs)
    o_r, dq_r, g_r = reference(qkv, dout, geo, heads, d, prm, 0.5, with_emb, with_hs)
    assert _rel(out, o_r) < 1e-5
    assert _rel(dqkv, dq_r) < 1e-5
    for a, b, name in zip(grads, g_r, NAMES):
        if name == "dkb":      # structurally zero (softmax is shift invariant): absolute bound
            assert float((a.double() - b).norm()) < 1e-5 * float(g_r[0].norm()), name
        elif (name == "demb" and not with_emb) or (name == "dhscale" and not with_hs):
            assert float(a.abs().max()) == 0.0, name
        else:
            assert _rel(a, b) < 1e-5, (name, _rel(a, b))


@pytest.mark.parametrize("L,d,heads,kind,with_emb,with_hs", CASES[::2])
def test_long_attention_bf16_matches_fp32(L, d, heads, kind, with_emb, with_hs):
    """bf16 mode against the fp32 mode on the same (bf16-representable) inputs, with the bounds the short kernels are held to
    (test_gpu_kernels.py: test_attention_mfma_matches_generic_and_fp32); padded rows and keys leave no NaN anywhere."""
    geo, N = geometry(kind, L, n_outer=2, inner=3)
    qkv, dout, prm = inputs(N, heads, d, torch.bfloat16, 2000 + L + d)
    nan = lambda t: torch.full_like(t, float("nan"))
    o_b, dq_b, g_b = run(qkv, dout, geo, heads, d, prm, with_emb, with_hs)
    o_f, dq_f, g_f = run(qkv.float(), dout.float(), geo, heads, d, prm, with_emb, with_hs)
    assert torch.isfinite(o_b.float()).all() and torch.isfinite(dq_b.float()).all()
    assert _rel(o_b.float(), o_f) < 1.5e-2
    parts = lambda t: t.float().view(N, heads, 3, d)
    for pi, pn in enumerate("qkv"):
        assert _rel(parts(dq_b)[:, :, pi], parts(dq_f)[:, :, pi]) < 3e-2, pn
    for a, b, name in zip(g_b, g_f, NAMES):
        if name == "dkb":
            assert float((a - b).norm()) < 1e-2 * float(g_f[0].norm()), name
        elif float(b.norm()) > 0:
            assert float((a - b).norm()) / float(b.norm()) < (1e-1 if name == "dhscale" else 5e-2), name
    # every token the geometry covers is written, whatever the buffers held (accumulate 0)
    o2, dq2, _ = run(qkv, dout, geo, heads, d, prm, with_emb, with_hs, out=nan(o_b), dqkv=nan(dq_b))
    assert torch.equal(o2, o_b) and torch.equal(dq2, dq_b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_long_attention_accumulate_adds(dtype):
    L, d, heads = 72, 64, 6
    geo, N = geometry("H", L)
    qkv, dout, prm = inputs(N, heads, d, dtype, 31)
    o0, dq0, _ = run(qkv, dout, geo, heads, d, prm)
    base_o = torch.randn(o0.shape, device="cuda").to(dtype)
    base_d = torch.randn(dq0.shape, device="cuda").to(dtype)
    o1, dq1, _ = run(qkv, dout, geo, heads, d, prm, acc=(1, 1), out=base_o.clone(), dqkv=base_d.clone())
    tol = 1e-6 if dtype == torch.float32 else 1e-2
    assert _rel(o1.float(), base_o.float() + o0.float()) < tol
    assert _rel(dq1.float(), base_d.float() + dq0.float()) < tol


@pytest.mark.parametrize("h,w,d,heads", [(40, 12, 64, 6), (12, 64, 32, 3), (128, 20, 128, 2)])
def test_long_attention_raw_pair_of_passes(h, w, d, heads):
    """accumulate 2 then 5 (the axial block's W and H passes sharing one LayerNorm backward) against 0 then 1, with the bounds of
    test_gpu_kernels.py: test_axial_attention_backward_raw_pair_of_passes; at least one of the passes is a long axis."""
    from bubbleformer_amd import _lib as L
    from bubbleformer_amd.ops import _p, _stream
    lib = L.lib()
    Fr, E = 2, heads * d
    N = Fr * h * w
    qkv, dout, prm = inputs(N, heads, d, torch.bfloat16, 7 + h + w)
    geoW = (Fr * h, w, 1, w, 0, 1)
    geoH = (Fr * w, h, w, h * w, 1, w)
    ws = torch.zeros(1024 * (4 * 128 + 33 * 16), device="cuda")

    def go(a1, a2):
        dqkv = torch.full_like(qkv, float("nan"))
        grads = [torch.zeros_like(t) for t in prm]
        for geo, acc in ((geoW, a1), (geoH, a2)):
            L.check(lib.bf_attn_bwd(1, _p(qkv), _p(dout), _p(dqkv), *geo, heads, d, *[_p(t) for t in prm], *[_p(t) for t in grads], 0.5, acc,
                                    _p(ws), ws.numel(), _stream()), "bf_attn_bwd")
        torch.cuda.synchronize()
        return dqkv, grads

    ref, gref = go(0, 1)
    raw, graw = go(2, 5)
    assert torch.isfinite(raw.float()).all()
    parts = lambda t: t.float().view(N, heads, 3, d)
    for pi, pn in enumerate("qkv"):
        e = _rel(parts(raw)[:, :, pi], parts(ref)[:, :, pi])
        assert e < (1e-6 if pn == "v" else 8e-3), (pn, e)
    for a, b, name in zip(graw, gref, NAMES):
        if name == "dkb":
            assert float((a - b).norm()) < 1e-2 * float(gref[0].norm()), name
        else:
            assert float((a - b).norm()) / float(b.norm()) < 5e-3, (name, float((a - b).norm()) / float(b.norm()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_long_attention_bitwise_reproducible(dtype):
    """Two runs, parameter gradients through the workspace rows: every output bit for bit."""
    L, d, heads = 96, 64, 6
    geo, N = geometry("temporal", L, n_outer=4, inner=40)       # 960 problems: more than one per workgroup
    qkv, dout, prm = inputs(N, heads, d, dtype, 77)
    a = run(qkv, dout, geo, heads, d, prm)
    b = run(qkv, dout, geo, heads, d, prm)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_long_attention_rejects_129(dtype):
    from bubbleformer_amd import _lib as L
    from bubbleformer_amd.ops import _dt, _p, _stream
    h = L.lib()
    d, heads, Lq = 32, 2, 129
    qkv, dout, prm = inputs(Lq, heads, d, dtype, 5)
    out = torch.zeros(Lq, heads * d, device="cuda", dtype=dtype)
    dqkv = torch.zeros_like(qkv)
    grads = [torch.zeros_like(t) for t in prm]
    geo = (1, Lq, 1, Lq, 0, 1)
    assert h.bf_attn_fwd(_dt(dtype), _p(qkv), _p(out), *geo, heads, d, *[_p(t) for t in prm], 1.0, 0, _stream()) < 0
    assert h.bf_attn_bwd(_dt(dtype), _p(qkv), _p(dout), _p(dqkv), *geo, heads, d, *[_p(t) for t in prm], *[_p(t) for t in grads], 1.0, 0,
                         None, 0, _stream()) < 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0 and float(dqkv.abs().max()) == 0.0


def _bucket_table(L):
    z = np.load(os.path.join(GOLDEN, "relpos_tables.npz"))
    if f"bucket_{L}" in z:
        return z[f"bucket_{L}"]
    return np.load(os.path.join(GOLDEN, "relpos_tables_long.npz"))[f"bucket_{L}"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("L", [40, 64, 100, 128])
def test_long_attention_t5_buckets_bit_exact_on_device(dtype, L):
    """The one device T5 bucket function (csrc/lane_ops.h: t5_bucket) as the long kernels (csrc/attn_long.hip, the third family that calls it)
    reach it, against the reference's integer tables, read back through the forward as in
    test_gpu_kernels.py: test_attention_t5_buckets_bit_exact_on_device (q = k = 0, V = one-hot(key), emb[b] = log(1 + b): the ratio
    P[q][k] / P[q][q] is 1 + bucket(q - k))."""
    from bubbleformer_amd import _lib as Lb
    from bubbleformer_amd.ops import _dt, _p, _stream
    d, heads, nseq = 128, 1, 2
    qkv = torch.zeros(nseq * L, 3 * d, device="cuda", dtype=dtype)
    for s_ in range(nseq):
        for l_ in range(L):
            qkv[s_ * L + l_, 2 * d + l_] = 1.0
    out = torch.empty(nseq * L, d, device="cuda", dtype=dtype)
    ones, zeros = torch.ones(d, device="cuda"), torch.zeros(d, device="cuda")
    emb = torch.log1p(torch.arange(32, device="cuda", dtype=torch.float32)).view(32, 1).contiguous()
    Lb.check(Lb.lib().bf_attn_fwd(_dt(dtype), _p(qkv), _p(out), nseq, L, 1, L, 0, 1, heads, d, _p(ones), _p(zeros), _p(ones), _p(zeros),
                                  _p(emb), None, 1.0, 0, _stream()), "bf_attn_fwd")
    torch.cuda.synchronize()
    P = out.float().view(nseq, L, d)[:, :, :L]
    got = torch.round(P / torch.diagonal(P, dim1=1, dim2=2).unsqueeze(-1) - 1.0).long().cpu().numpy()
    want = _bucket_table(L)
    for s_ in range(nseq):
        assert np.array_equal(got[s_], want), (L, s_)
