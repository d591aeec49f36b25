"""GPU: the third source mode of the last debed stage's backward -- an explicit gradient w.r.t. the prediction AND the fused loss given
together, d pred = dpred + coef[f][c] * gscale * (pred - y) -- at all three entry points (bf_nchw2pm, bf_debed_last_bwd,
bf_debed_last_bwd_norm).  This is the backward of one pass of a training step unrolled through its own predictions.

Shapes: test_debed_last_stage_backward_one_pass's without its workload-sized row -- padded output channels (Co = 3, 1), a frame
shorter than one 256-row slice, and a ragged last slice.  Bounds: the patch-major rows within ONE bf16 ulp of the definition formed in
fp64 (a correctly rounded fp32 value is within half an ulp; the fp32 arithmetic in front -- coef * gscale, the difference, one fma --
has the other half) and bit-identical between the entry points; the fp32 bf_nchw2pm within 1e-6 relative L2; the data gradient, the
gradient of the map in front of the InstanceNorm and of its affine parameters within test_gpu_kernels.py's bounds for the two existing
modes (4e-3, 6e-3, 2e-3), whose arithmetic behind the rows this mode shares.  Before this mode existed the explicit gradient won and
the loss term was dropped silently: every comparison against the definition here fails on that code."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(32, 3, 6, 16), (64, 1, 5, 32), (128, 4, 3, 48)]
FRAMES = 3


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _bf16_ulp(v):
    """Spacing of bf16 (8 significant bits) at |v|, v fp64; the smallest normal's below it."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=v.device), e - 7)


def _patch_major(t, Co, h, w):
    """(F, Co, 2h, 2w) -> [F*h*w][16], n = co*4 + ky*2 + kx, zero padded."""
    P = t.shape[0] * h * w
    out = torch.zeros(P, 16, dtype=t.dtype, device=t.device)
    out[:, :4 * Co] = t.view(t.shape[0], Co, h, 2, w, 2).permute(0, 2, 4, 1, 3, 5).reshape(P, 4 * Co)
    return out


_CASES = {}


def _case(Ci, Co, h, w):
    """Inputs (drawn on the host: the same numbers wherever the test runs) and the fp64 definition, made once per shape."""
    key = (Ci, Co, h, w)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * Ci + 10 * Co + h)
        r = lambda *s: torch.randn(*s, generator=g)
        wc = torch.zeros(Ci, 16)
        wc[:, :4 * Co] = r(Ci, 4 * Co) / 4
        pred, y, dpred = r(FRAMES, Co, 2 * h, 2 * w), r(FRAMES, Co, 2 * h, 2 * w), 0.7 * r(FRAMES, Co, 2 * h, 2 * w)
        coef = 0.5 + torch.rand(FRAMES, Co, generator=g)
        gs = torch.tensor([0.7])
        ymap = (r(FRAMES * h * w, Ci) * 1.5 + 0.2).bfloat16()
        in_w, in_b = 1 + 0.2 * r(Ci), 0.3 * r(Ci)
        c = {k: v.cuda() for k, v in dict(wc=wc.bfloat16(), pred=pred, y=y, dpred=dpred, coef=coef, gs=gs, ymap=ymap, in_w=in_w, in_b=in_b).items()}
        want = c["dpred"].double() + c["coef"].double()[:, :, None, None] * c["gs"].double() * (c["pred"].double() - c["y"].double())
        c["want"] = _patch_major(want, Co, h, w)                      # fp64, [P][16]
        c["want_bf16"] = c["want"].float().bfloat16()
        _CASES[key] = c
    return _CASES[key]


def _run_nchw2pm(c, Co, h, w, dtype):
    from bubbleformer_amd import _lib as L
    from bubbleformer_amd.ops import _p, _stream
    P = FRAMES * h * w
    dpm = torch.full((P, 16), float("nan"), device="cuda", dtype=torch.bfloat16 if dtype == 1 else torch.float32)
    L.check(L.lib().bf_nchw2pm(dtype, _p(c["dpred"]), _p(c["pred"]), _p(c["y"]), _p(c["coef"]), _p(c["gs"]), _p(dpm), FRAMES, Co, h, w, 16,
                               _stream()), "bf_nchw2pm")
    return dpm


def _run_last_bwd(c, Ci, Co, h, w):
    from bubbleformer_amd import _lib as L
    from bubbleformer_amd.ops import _p, _stream
    P = FRAMES * h * w
    dpm = torch.full((P, 16), float("nan"), device="cuda", dtype=torch.bfloat16)
    dact = torch.full((P, Ci), float("nan"), device="cuda", dtype=torch.bfloat16)
    L.check(L.lib().bf_debed_last_bwd(1, _p(c["dpred"]), _p(c["pred"]), _p(c["y"]), _p(c["coef"]), _p(c["gs"]), _p(c["wc"]), _p(dpm), _p(dact),
                                      FRAMES, Ci, Co, h, w, 16, _stream()), "bf_debed_last_bwd")
    return dpm, dact


def _run_last_bwd_norm(c, Ci, Co, h, w):
    from bubbleformer_amd import _lib as L
    from bubbleformer_amd.ops import _p, _stream
    S, P = h * w, FRAMES * h * w
    yf = c["ymap"].float().view(FRAMES, S, Ci)
    mean, rstd = yf.mean(1).contiguous(), (yf.var(1, unbiased=False) + 1e-5).rsqrt().contiguous()
    dpm = torch.full((P, 16), float("nan"), device="cuda", dtype=torch.bfloat16)
    dx = torch.full((P, Ci), float("nan"), device="cuda", dtype=torch.bfloat16)
    dw, db = torch.full((Ci,), 2.0, device="cuda"), torch.full((Ci,), -1.0, device="cuda")
    nws = 2 * FRAMES * Ci * (1 + (S // 16 + 15) // 16)          # totals + one row of partials per 256-row slice
    ws = torch.full((nws,), float("nan"), device="cuda")
    L.check(L.lib().bf_debed_last_bwd_norm(1, _p(c["dpred"]), _p(c["pred"]), _p(c["y"]), _p(c["coef"]), _p(c["gs"]), _p(c["wc"]), _p(dpm),
                                           _p(c["ymap"]), _p(mean), _p(rstd), _p(c["in_w"]), _p(c["in_b"]), _p(dx), _p(dw), _p(db), FRAMES, Ci, Co,
                                           h, w, 16, _p(ws), nws, _stream()), "bf_debed_last_bwd_norm")
    return dpm, dx, dw - 2.0, db + 1.0


def _assert_within_one_bf16_ulp(dpm, c, what):
    got, want = dpm.double(), c["want"]
    assert torch.isfinite(got).all(), what
    err, ulp = (got - want).abs(), _bf16_ulp(want)
    worst = float((err / ulp).max())
    print(f"{what}: worst |dpm - definition| = {worst:.3f} bf16 ulp")
    assert worst <= 1.0, (what, worst)


@pytest.mark.parametrize("Ci,Co,h,w", SHAPES)
def test_patch_major_rows_of_both_sources(Ci, Co, h, w):
    """dpm of the three entry points, both sources given: within one bf16 ulp of the fp64 definition, bit-identical to one another, zero in
    the padded columns; bf_nchw2pm in fp32 within 1e-6; and not what either source alone gives."""
    c = _case(Ci, Co, h, w)
    a = _run_nchw2pm(c, Co, h, w, 1)
    b, _ = _run_last_bwd(c, Ci, Co, h, w)
    n, _, _, _ = _run_last_bwd_norm(c, Ci, Co, h, w)
    _assert_within_one_bf16_ulp(a, c, "bf_nchw2pm")
    _assert_within_one_bf16_ulp(b, c, "bf_debed_last_bwd")
    _assert_within_one_bf16_ulp(n, c, "bf_debed_last_bwd_norm")
    assert float(a[:, 4 * Co:].float().abs().sum()) == 0.0
    assert torch.equal(a, b) and torch.equal(b, n)
    f = _run_nchw2pm(c, Co, h, w, 0)
    e = _rel(f, c["want"])
    print(f"bf_nchw2pm fp32: relative L2 {e:.2e}")
    assert e < 1e-6
    # the loss term is there, and so is the given gradient
    only_given = _patch_major(c["dpred"].double(), Co, h, w)
    assert _rel(a, only_given) > 0.3 and _rel(a, c["want"] - only_given) > 0.3


@pytest.mark.parametrize("Ci,Co,h,w", SHAPES)
def test_data_gradient_of_both_sources(Ci, Co, h, w):
    """bf_debed_last_bwd: dact = dpm @ wc^T against a plain fp64 matmul of the definition's bf16 rows (the bound of the existing modes)."""
    c = _case(Ci, Co, h, w)
    _, dact = _run_last_bwd(c, Ci, Co, h, w)
    ref = c["want_bf16"].double() @ c["wc"].double().t()
    assert torch.isfinite(dact.float()).all()
    e = _rel(dact, ref)
    print(f"dact: relative L2 {e:.2e}")
    assert e < 4e-3                      # one bf16 rounding of the result


@pytest.mark.parametrize("Ci,Co,h,w", SHAPES)
def test_norm_in_front_gradients_of_both_sources(Ci, Co, h, w):
    """bf_debed_last_bwd_norm: dx and the InstanceNorm's affine gradients against autograd in fp64 through InstanceNorm -> GELU -> @ wc on the
    same bf16 operands, seeded with the definition's bf16 rows (the bounds of the existing modes)."""
    c = _case(Ci, Co, h, w)
    S, P = h * w, FRAMES * h * w
    _, dx, dw, db = _run_last_bwd_norm(c, Ci, Co, h, w)
    yr = c["ymap"].double().view(FRAMES, S, Ci).requires_grad_(True)
    wr, br = c["in_w"].double().requires_grad_(True), c["in_b"].double().requires_grad_(True)
    xh = (yr - yr.mean(1, keepdim=True)) / (yr.var(1, unbiased=False, keepdim=True) + 1e-5).sqrt()
    out = torch.nn.functional.gelu(xh * wr + br).view(P, Ci) @ c["wc"].double()
    (out * c["want_bf16"].double()).sum().backward()
    assert torch.isfinite(dx.float()).all()
    e = (_rel(dx, yr.grad.view(P, Ci)), _rel(dw, wr.grad), _rel(db, br.grad))
    print("dx, d_in_w, d_in_b: relative L2 %.2e %.2e %.2e" % e)
    assert e[0] < 6e-3                   # bf16 output rounding + the polynomial gelu'
    assert e[1] < 2e-3 and e[2] < 2e-3


def test_both_sources_need_the_coefficients():
    """dpred beside (pred, y) asks for the loss term: without coef the call is refused, nothing is launched."""
    from bubbleformer_amd import _lib as L
    from bubbleformer_amd.ops import _p, _stream
    Ci, Co, h, w = SHAPES[0]
    c = _case(Ci, Co, h, w)
    P = FRAMES * h * w
    dpm = torch.zeros((P, 16), device="cuda", dtype=torch.bfloat16)
    dact = torch.zeros((P, Ci), device="cuda", dtype=torch.bfloat16)
    lib = L.lib()
    assert lib.bf_nchw2pm(1, _p(c["dpred"]), _p(c["pred"]), _p(c["y"]), None, _p(c["gs"]), _p(dpm), FRAMES, Co, h, w, 16, _stream()) < 0
    assert lib.bf_debed_last_bwd(1, _p(c["dpred"]), _p(c["pred"]), _p(c["y"]), None, _p(c["gs"]), _p(c["wc"]), _p(dpm), _p(dact), FRAMES, Ci, Co, h, w, 16,
                                 _stream()) < 0
    assert b"coef" in lib.bf_last_error()
    torch.cuda.synchronize()
    assert float(dpm.float().abs().sum()) == 0.0 and float(dact.float().abs().sum()) == 0.0
    # gscale = NULL means 1, as in the single-source loss mode
    one = torch.ones(1, device="cuda")
    a = torch.empty_like(dpm)
    b = torch.empty_like(dpm)
    L.check(lib.bf_nchw2pm(1, _p(c["dpred"]), _p(c["pred"]), _p(c["y"]), _p(c["coef"]), None, _p(a), FRAMES, Co, h, w, 16, _stream()), "bf_nchw2pm")
    L.check(lib.bf_nchw2pm(1, _p(c["dpred"]), _p(c["pred"]), _p(c["y"]), _p(c["coef"]), _p(one), _p(b), FRAMES, Co, h, w, 16, _stream()), "bf_nchw2pm")
    assert torch.equal(a, b)
