"""GPU: the ClassicUnet kernels (csrc/bn.hip, with conv.hip's convs) and model against fp64 -- BatchNorm (batch and running statistics) +
GELU + 2x2 max pool forward and backward, ConvTranspose2d k2 s2 with Cin = 2 Cout, the bias-free 3x3 convs on the NCHW clip; the model
against the reference goldens and, at full width, against the fp64 restatement; bit reproducibility; TrainStep; checkpoint; graphed
rollout."""
import pytest
import torch
import torch.nn.functional as F

from tests import unet_classic_restatement as U
from tests.unet_restatement import golden_grad_errors

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2}
# fp32 model gradients (and d clip): measured worst 1.5e-5 per tensor on the goldens and 2.4e-5 at full width, on the BatchNorm parameter
# gradients whose pixel sums cancel most.  Stock PyTorch fp32 reaches 1.4e-5 on the same tensor; prediction, loss
# and buffers hold 1e-5
FP32_GRAD_TOL = 5e-5
SHIPPED = dict(time_window=16, input_fields=4, output_fields=4, hidden_channels=32)


def _rel(a, b):
    a, b = a.detach().double().flatten(), b.detach().double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _randn(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(DEV)


def _bn(C, seed, training=True):
    """(gamma, beta, bn tuple) on the device with non-trivial running statistics."""
    rm = _randn(C, scale=0.2, seed=seed).float()
    rv = (0.5 + _randn(C, seed=seed + 1).abs()).float()
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    g = (1 + _randn(C, scale=0.1, seed=seed + 2)).float()
    b = _randn(C, scale=0.1, seed=seed + 3).float()
    return g, b, (rm, rv, nbt, 1e-5, 0.1, training)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,H,W,C,ties", [
    (2, 6, 10, 1, False),       # one channel
    (3, 5, 7, 20, False),       # odd frame: a partial window row / column is activated but not pooled; 105 pixels
    (1, 18, 14, 33, True),      # 33 channels, constant 2x2 windows (exact ties) in every other channel
    (2, 6, 6, 512, False),      # 512 channels
])
def test_batchnorm_gelu_pool_vs_fp64(dt, B, H, W, C, ties):
    """bf_bn_fwd / bf_bn_act / bf_bn_bwd against fp64 F.batch_norm(training) -> F.gelu -> F.max_pool2d: forward, pool, running-statistic
    update, dgamma, dbeta and dc, with the skip gradient (an fp32 channel slice of a wider buffer) and the pooled gradient together."""
    from bubbleformer_amd import ops
    c64 = _randn(B, H, W, C, scale=2.0, seed=1) + 0.3
    if ties:
        blk = _randn(B, (H + 1) // 2, (W + 1) // 2, C, scale=2.0, seed=2).repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W]
        c64[..., ::2] = blk[..., ::2]
    c = c64.to(dt)
    g, b, bn = _bn(C, 10)
    rm0, rv0 = bn[0].clone(), bn[1].clone()
    cn = c.clone().requires_grad_(True)
    gn, bnn = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    a, port, p = ops.classic_act(cn, gn, bnn, bn, pool=True)
    wide = _randn(B, H, W, C + 7, seed=3).float()
    dA = wide[..., 5:5 + C]                               # read in place: row stride C + 7, channel offset 5
    dP = _randn(*p.shape, seed=4).to(dt)
    torch.autograd.backward([port, p], [dA, dP])
    torch.cuda.synchronize()
    # fp64 reference on the stored input
    cr = c.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    gr, br = g.double().requires_grad_(True), b.double().requires_grad_(True)
    rm, rv = rm0.double().clone(), rv0.double().clone()
    y = F.gelu(F.batch_norm(cr, rm, rv, gr, br, training=True, momentum=0.1, eps=1e-5))
    tol = TOL[dt]
    assert _rel(a.permute(0, 3, 1, 2), y) <= tol
    # the pool: max of the STORED activations, window index by F.max_pool2d's rule (first maximum)
    a_st = a.permute(0, 3, 1, 2).double().cpu()
    pw, iw = F.max_pool2d(a_st, 2, 2, return_indices=True)
    assert torch.equal(p.permute(0, 3, 1, 2).double().cpu(), pw)
    dy = dA.double().permute(0, 3, 1, 2).cpu().clone()
    flat = dy.flatten(2)
    flat.scatter_add_(2, iw.flatten(2), dP.double().permute(0, 3, 1, 2).cpu().flatten(2))
    dcr, dgr, dbr = torch.autograd.grad(y, [cr, gr, br], flat.view_as(dy).to(DEV))
    assert _rel(cn.grad.permute(0, 3, 1, 2), dcr) <= tol, _rel(cn.grad.permute(0, 3, 1, 2), dcr)
    assert _rel(gn.grad, dgr) <= tol and _rel(bnn.grad, dbr) <= tol
    assert _rel(bn[0], rm) <= 1e-5 and _rel(bn[1], rv) <= 1e-5
    assert int(bn[2]) == 1
    if ties:                                              # constant windows: every maximum is a tie, won by the window's first element
        first = iw[:, ::2]
        assert bool(((first // W) % 2 == 0).all()) and bool(((first % W) % 2 == 0).all())


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_batchnorm_eval_mode(dt):
    from bubbleformer_amd import ops
    B, H, W, C = 2, 6, 8, 33
    c = (_randn(B, H, W, C, scale=1.5, seed=5) + 0.2).to(dt)
    g, b, bn = _bn(C, 20, training=False)
    rm0, rv0 = bn[0].clone(), bn[1].clone()
    with torch.no_grad():
        a, _ = ops.classic_act(c, g, b, bn)
    torch.cuda.synchronize()
    y = F.gelu(F.batch_norm(c.double().permute(0, 3, 1, 2), rm0.double(), rv0.double(), g.double(), b.double(), training=False, eps=1e-5))
    assert _rel(a.permute(0, 3, 1, 2), y) <= TOL[dt]
    assert torch.equal(bn[0], rm0) and torch.equal(bn[1], rv0) and int(bn[2]) == 0


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,H,W,Cout,port", [(1, 3, 5, 8, False), (2, 4, 6, 20, True), (2, 3, 3, 256, True)])
def test_upconv_k2s2_vs_fp64(dt, B, H, W, Cout, port):
    """ConvTranspose2d(2*Cout, Cout, 2, stride 2): forward (four one-tap phases), data gradient (in the dtype, or fp32 through a port),
    weight gradient in the (Cin, Cout, 2, 2) layout, bias gradient."""
    from bubbleformer_amd import ops
    Cin = 2 * Cout
    w = _randn(Cin, Cout, 2, 2, scale=Cin ** -0.5, seed=6).to(dt).double()
    bias = _randn(Cout, scale=0.1, seed=7)
    x = _randn(B, Cin, H, W, seed=8).to(dt).double()
    wr, br, xr = (t.clone().requires_grad_(True) for t in (w, bias, x))
    yr = F.conv_transpose2d(xr, wr, br, stride=2)
    dy = _randn(*yr.shape, seed=9).to(dt).double()
    yr.backward(dy)
    wn, bn = w.float().requires_grad_(True), bias.float().requires_grad_(True)
    xn = x.permute(0, 2, 3, 1).to(dt).contiguous().requires_grad_(True)
    pt = ops._port(xn).requires_grad_(True) if port else None
    y = ops.unet_upconv2(xn, wn, bn, pt)
    dx = torch.autograd.grad(y, [pt if port else xn, wn, bn], dy.permute(0, 2, 3, 1).to(dt))
    torch.cuda.synchronize()
    tol = TOL[dt]
    assert _rel(y.permute(0, 3, 1, 2), yr) <= tol
    assert dx[0].dtype == (torch.float32 if port else dt)
    assert _rel(dx[0].permute(0, 3, 1, 2), xr.grad) <= tol
    assert dx[1].shape == (Cin, Cout, 2, 2) and _rel(dx[1], wr.grad) <= tol
    assert _rel(dx[2], br.grad) <= tol


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T,Cf,Cout", [(1, 1, 8), (2, 4, 20)])
def test_block_on_nchw_clip_vs_fp64(dt, T, Cf, Cout):
    """The first encoder's conv path: bias-free 3x3 conv reading the (B, T, C, H, W) fp32 clip (C = T*fields, down to 1) -> BN1 + GELU as
    conv2's prologue -> bias-free conv2.  Forward (raw conv2 output), BN1 statistics, and every gradient incl. d clip."""
    from bubbleformer_amd import ops
    B, H, W = 2, 7, 9
    Cin = T * Cf
    x = _randn(B, T, Cf, H, W, seed=11).float()
    w1 = _randn(Cout, Cin, 3, 3, scale=(9 * Cin) ** -0.5, seed=12).to(dt).float()
    w2 = _randn(Cout, Cout, 3, 3, scale=(9 * Cout) ** -0.5, seed=13).to(dt).float()
    g, b, bn = _bn(Cout, 30)
    rm0, rv0 = bn[0].clone(), bn[1].clone()
    xn = x.clone().requires_grad_(True)
    pn = [t.clone().requires_grad_(True) for t in (w1, g, b, w2)]
    c2 = ops.classic_conv(xn, None, None, pn[0], pn[1], pn[2], pn[3], bn, dt, nchw=True)
    dc2 = _randn(*c2.shape, seed=14).to(dt)
    c2.backward(dc2)
    torch.cuda.synchronize()
    xq = x.to(dt).double() if dt == torch.bfloat16 else x.double()     # the bf16 MFMAs consume the rounded clip
    xr = xq.clone().requires_grad_(True)
    pr = [t.double().clone().requires_grad_(True) for t in (w1, g, b, w2)]
    rm, rv = rm0.double().clone(), rv0.double().clone()
    h = F.conv2d(xr.reshape(B, Cin, H, W), pr[0], padding=1)
    h = F.gelu(F.batch_norm(h, rm, rv, pr[1], pr[2], training=True, momentum=0.1, eps=1e-5))
    yr = F.conv2d(h, pr[3], padding=1)
    yr.backward(dc2.double().permute(0, 3, 1, 2))
    tol = TOL[dt]
    assert _rel(c2.permute(0, 3, 1, 2), yr) <= tol
    assert _rel(xn.grad, xr.grad) <= tol
    for i, name in enumerate(("w1", "gamma1", "beta1", "w2")):
        assert _rel(pn[i].grad, pr[i].grad) <= tol, name
    stol = 1e-5 if dt == torch.float32 else 1e-2                       # bf16: statistics of the bf16-stored conv output
    assert _rel(bn[0], rm) <= stol and _rel(bn[1], rv) <= stol and int(bn[2]) == 1


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("port", [False, True])
def test_decoder_conv_skip_gradient_vs_fp64(dt, port):
    """A decoder's conv1 on cat(u, skip): the skip's gradient leaves in fp32 through a port (the U-Net's path) or, without one, as the
    skip's own gradient in its dtype -- never dropped."""
    from bubbleformer_amd import ops
    B, H, W, C0, C1, Cout = 2, 6, 10, 12, 20, 16
    u = _randn(B, C0, H, W, seed=41).to(dt)
    sk = _randn(B, C1, H, W, seed=42).to(dt)
    w1 = _randn(Cout, C0 + C1, 3, 3, scale=(9 * (C0 + C1)) ** -0.5, seed=43).to(dt).float()
    w2 = _randn(Cout, Cout, 3, 3, scale=(9 * Cout) ** -0.5, seed=44).to(dt).float()
    g, b, bn = _bn(Cout, 50)
    rm0, rv0 = bn[0].clone(), bn[1].clone()
    cl = lambda t: t.permute(0, 2, 3, 1).contiguous()
    un, skn = cl(u).requires_grad_(True), cl(sk).requires_grad_(True)
    pt = ops._port(skn).requires_grad_(True) if port else None
    pn = [t.clone().requires_grad_(True) for t in (w1, g, b, w2)]
    c2 = ops.classic_conv(un, skn, pt, pn[0], pn[1], pn[2], pn[3], bn, dt)
    dc2 = _randn(*c2.shape, seed=45).to(dt)
    c2.backward(dc2)
    torch.cuda.synchronize()
    ur, sr = u.double().requires_grad_(True), sk.double().requires_grad_(True)
    pr = [t.double().clone().requires_grad_(True) for t in (w1, g, b, w2)]
    h = F.conv2d(torch.cat((ur, sr), 1), pr[0], padding=1)
    h = F.gelu(F.batch_norm(h, rm0.double().clone(), rv0.double().clone(), pr[1], pr[2], training=True, momentum=0.1, eps=1e-5))
    yr = F.conv2d(h, pr[3], padding=1)
    yr.backward(dc2.double().permute(0, 3, 1, 2))
    tol = TOL[dt]
    assert _rel(c2.permute(0, 3, 1, 2), yr) <= tol
    assert _rel(un.grad.permute(0, 3, 1, 2), ur.grad) <= tol
    dskip = pt.grad if port else skn.grad
    assert dskip is not None and dskip.dtype == (torch.float32 if port else dt)
    assert (skn.grad is None) == port
    assert _rel(dskip.permute(0, 3, 1, 2), sr.grad) <= tol
    for i, name in enumerate(("w1", "gamma1", "beta1", "w2")):
        assert _rel(pn[i].grad, pr[i].grad) <= tol, name


def _native(cfg, p, dt=torch.float32, buf=None):
    from bubbleformer_amd.models import get_model
    m = get_model("unet_classic", compute_dtype=dt, **cfg)
    m.load_state_dict({k: v.float() for k, v in p.items()}, strict=False)
    if buf is not None:
        m.load_state_dict({k: (v if v.dtype == torch.int64 else v.float()) for k, v in buf.items()}, strict=False)
    return m.to(DEV)


def _buffers(m):
    return {k: v for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}


@pytest.mark.parametrize("name", ["h8_c1", "h16_c8", "h8_c8_b3"])
def test_model_fp32_vs_reference_goldens(name):
    spec, z, p = U.load_golden(name)
    T = spec["cfg"]["time_window"]
    m = _native(spec["cfg"], p)
    x = torch.from_numpy(z["x"]).float().to(DEV).requires_grad_(True)
    y = torch.from_numpy(z["y"]).float().to(DEV)
    loss, pred = m.forward_loss(x, y)
    loss.backward()
    torch.cuda.synchronize()
    tol, gtol = 1e-5, FP32_GRAD_TOL
    assert _rel(pred.cpu(), torch.from_numpy(z["pred"])) <= tol
    assert abs(float(loss.detach()) - float(z["loss"])) <= tol * abs(float(z["loss"]))
    assert _rel(x.grad.cpu(), torch.from_numpy(z["dx"])) <= gtol
    grads = {k: q.grad for k, q in m.named_parameters()}
    errs = golden_grad_errors(grads, z)
    print(name, "worst gradient vs golden", max(errs.items(), key=lambda kv: kv[1]))
    assert max(errs.values()) <= gtol, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    # every gradient whole against the fp64 restatement (pinned to the goldens by test_unet_classic.py)
    buf_r = U.fresh_buffers(p, device=DEV)
    _, _, dx_r, g_r = U.run(torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["y"]).to(DEV), {k: v.to(DEV) for k, v in p.items()}, buf_r, T)
    worst = {k: _rel(g, g_r[k]) for k, g in grads.items()}
    assert _rel(x.grad, dx_r) <= gtol
    assert max(worst.values()) <= gtol, sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    # BatchNorm buffers after one training forward
    want = U.golden_buffers(z, "b:")
    got = _buffers(m)
    assert set(got) == set(want)
    for k, v in want.items():
        if v.dtype == torch.int64:
            assert got[k].dtype == torch.int64 and int(got[k]) == 1, k
        else:
            assert _rel(got[k].cpu(), v) <= tol, (k, _rel(got[k].cpu(), v))
    # eval mode on seeded running statistics
    m.load_state_dict({k: (v if v.dtype == torch.int64 else v.float()) for k, v in U.golden_buffers(z, "e:").items()}, strict=False)
    m.eval()
    with torch.no_grad():
        pe = m(torch.from_numpy(z["x"]).float().to(DEV))
    torch.cuda.synchronize()
    assert _rel(pe.cpu(), torch.from_numpy(z["pred_eval"])) <= tol


def _shipped_weights():
    from tools.gen_unet_classic_golden import weights
    from bubbleformer_amd.models.unets import ClassicUnet
    return weights(ClassicUnet(**SHIPPED), 7)


def test_full_width_parity_vs_fp64_restatement():
    """Shipped width (hidden 32, T = 16, 4 fields) at 96 x 96, batch 2 (down to 6 x 6 at 512 channels).  fp32 against the fp64
    restatement of the same weights.  bf16 against the fp64 restatement of the weights and clip rounded to bf16; its gradients are held to
    3e-2 per tensor or, where more, to twice what bf16 activation storage alone does to an otherwise fp64 computation (the restatement with
    store=bf16): batch statistics make this network's gradients that sensitive to the stored activations."""
    p = _shipped_weights()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 16, 4, 96, 96, generator=g, dtype=torch.float64)
    y = torch.randn(2, 16, 4, 96, 96, generator=g, dtype=torch.float64)
    res = {}
    for dt in (torch.float32, torch.bfloat16):
        rnd = (lambda t: t) if dt == torch.float32 else (lambda t: t.bfloat16().double())
        pd = {k: rnd(v).to(DEV) for k, v in p.items()}
        buf_r = U.fresh_buffers(p, device=DEV)
        pred_r, loss_r, dx_r, g_r = U.run(rnd(x).to(DEV), y.to(DEV), pd, buf_r, 16)
        m = _native(SHIPPED, p, dt)
        xn = x.float().to(DEV).requires_grad_(True)
        loss, pred = m.forward_loss(xn, y.float().to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        bufs = _buffers(m)
        r = dict(loss=abs(float(loss.detach()) - float(loss_r)) / float(loss_r), pred=_rel(pred, pred_r), dx=_rel(xn.grad, dx_r),
                 grads={k: _rel(q.grad, g_r[k]) for k, q in m.named_parameters()},
                 bufs=max(_rel(bufs[k], v) for k, v in buf_r.items() if v.dtype != torch.int64))
        if dt == torch.bfloat16:
            pred_s, _, dx_s, g_s = U.run(rnd(x).to(DEV), y.to(DEV), pd, U.fresh_buffers(p, device=DEV), 16, store=torch.bfloat16)
            r["store"] = dict(pred=_rel(pred_s, pred_r), dx=_rel(dx_s, dx_r), grads={k: _rel(g_s[k], g_r[k]) for k in g_r})
            r["vs_store"] = dict(pred=_rel(pred, pred_s), dx=_rel(xn.grad, dx_s), grads=max(_rel(q.grad, g_s[k]) for k, q in m.named_parameters()))
            del pred_s, dx_s, g_s
        res[dt] = r
        worst = sorted(((v, k) for k, v in r["grads"].items()), reverse=True)[:4]
        print(dt, {k: v for k, v in r.items() if k not in ("grads", "store")}, "worst grads", worst)
        if "store" in r:
            print("  bf16 storage alone: pred %.3g dx %.3g worst grads %s" % (r["store"]["pred"], r["store"]["dx"],
                                                                               sorted(((v, k) for k, v in r["store"]["grads"].items()), reverse=True)[:4]))
            print("  max ratio native / storage-alone over gradients above 3e-2:",
                  max([r["grads"][k] / r["store"]["grads"][k] for k in r["grads"] if r["grads"][k] > 3e-2] or [0.0]))
        del m, pred_r, dx_r, g_r
    r = res[torch.float32]
    assert r["loss"] <= 1e-5 and r["pred"] <= 1e-5 and r["bufs"] <= 1e-5, r
    assert r["dx"] <= FP32_GRAD_TOL and max(r["grads"].values()) <= FP32_GRAD_TOL
    r = res[torch.bfloat16]
    assert r["loss"] <= 1e-3 and r["bufs"] <= 1e-2, r
    assert r["pred"] <= max(3e-2, 2 * r["store"]["pred"]) and r["dx"] <= max(3e-2, 2 * r["store"]["dx"])
    over = {k: (v, r["store"]["grads"][k]) for k, v in r["grads"].items() if v > max(3e-2, 2 * r["store"]["grads"][k])}
    assert not over, over
    # and fixed ceilings, 1.5x the measured worst cases (pred 3.7e-2, d clip 0.21, encoder1.norm2.weight 0.32), so the bound cannot
    # follow the storage-only reference upwards
    assert r["pred"] <= 0.056 and r["dx"] <= 0.32 and max(r["grads"].values()) <= 0.48, (r["pred"], r["dx"], max(r["grads"].values()))


def test_bf16_training_pass_is_bit_reproducible():
    p = _shipped_weights()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 16, 4, 192, 192, generator=g).to(DEV)
    y = torch.randn(2, 16, 4, 192, 192, generator=g).to(DEV)
    runs = []
    for _ in range(2):
        m = _native(SHIPPED, p, torch.bfloat16)
        loss, _ = m.forward_loss(x, y)
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.detach().clone(), {k: q.grad.clone() for k, q in m.named_parameters()}, {k: v.clone() for k, v in _buffers(m).items()}))
        del m
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k


@pytest.mark.parametrize("optimizer", ["adamw", "lion"])
def test_train_step(optimizer):
    from bubbleformer_amd.trainer import TrainStep
    spec, z, p = U.load_golden("h8_c8_b3")
    T = spec["cfg"]["time_window"]
    m = _native(spec["cfg"], p)
    x = torch.from_numpy(z["x"]).to(DEV)
    y = torch.from_numpy(z["y"]).to(DEV)
    step = TrainStep(m, lr=1e-3, optimizer=optimizer)
    losses, seen = [], []
    for i in range(3):
        losses.append(float(step(x.float(), None, y.float())))
        bufs = _buffers(m)
        assert int(bufs["encoder1.norm1.num_batches_tracked"]) == i + 1
        seen.append(bufs["bottleneck.norm2.running_mean"].clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    assert all(torch.isfinite(torch.tensor(losses)))
    if optimizer == "lion":
        assert losses[-1] < losses[0]
        return
    ref = {k: v.to(DEV).clone().requires_grad_(True) for k, v in p.items()}
    buf = U.fresh_buffers(p, device=DEV)
    opt = torch.optim.AdamW(list(ref.values()), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    for i in range(3):
        opt.zero_grad()
        loss = U.lp_loss(U.forward(x, ref, buf, T), y)
        loss.backward()
        opt.step()
        want = float(loss.detach())
        assert abs(losses[i] - want) <= 1e-4 * want, (i, losses[i], want)
    assert _rel(_buffers(m)["bottleneck.norm2.running_var"], buf["bottleneck.norm2.running_var"]) <= 1e-4


def test_checkpoint_round_trip_eval_forward_bitwise(tmp_path):
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    spec, z, p = U.load_golden("h16_c8")
    m = _native(spec["cfg"], p)
    x = torch.from_numpy(z["x"]).float().to(DEV)
    m.forward_loss(x, torch.from_numpy(z["y"]).float().to(DEV))          # moves the running statistics
    m.eval()
    path = str(tmp_path / "c.ckpt")
    save_checkpoint(path, m)
    fresh = get_model("unet_classic", **spec["cfg"]).to(DEV)
    load_checkpoint(path, fresh)
    fresh.eval()
    with torch.no_grad():
        a, b = m(x), fresh(x)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert int(fresh.decoder2.norm1.num_batches_tracked) == 1


def test_graphed_eval_rollout_equals_eager():
    from bubbleformer_amd.utils.rollout import autoregressive_rollout
    spec, z, p = U.load_golden("h8_c8_b3")
    m = _native(spec["cfg"], p, buf=U.golden_buffers(z, "e:"))
    m.eval()
    x0 = torch.from_numpy(z["x"][0]).float().to(DEV)
    pg, _ = autoregressive_rollout(m, x0, 3, use_graph=True)
    pe, _ = autoregressive_rollout(m, x0, 3, use_graph=False)
    torch.cuda.synchronize()
    assert torch.equal(pg, pe)
    assert int(m.encoder1.norm1.num_batches_tracked) == 7             # eval forwards leave the buffers alone
