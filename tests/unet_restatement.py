"""Plain-PyTorch restatement of ModernUnet (unet_modern) for the parity tests: stock torch.nn.functional ops on a state_dict,
in whatever dtype / device the state_dict is in.  Written from the architecture (hidden channels, ch_mults, GroupNorm(8) + GELU in front of
every conv, channel-concatenated skips), not from the model code under test."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class _Stored(torch.autograd.Function):
    """A tensor stored in a narrower dtype and read back: rounds the value, and its gradient, to `dt` (bf16 activation storage)."""

    @staticmethod
    def forward(ctx, x, dt):
        ctx.dt = dt
        return x.to(dt).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dt).to(g.dtype), None


class _Operand(torch.autograd.Function):
    """An MFMA operand rounded to `dt` on its way in: the value is rounded, the gradient passes in full precision."""

    @staticmethod
    def forward(ctx, x, dt):
        return x.to(dt).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g, None


def _stored(x, store):
    return x if store is None else _Stored.apply(x, store)


def _operand(x, store):
    return x if store is None else _Operand.apply(x, store)


def _gn_act(x, sd, name, norm=True, store=None):
    if norm:
        x = F.group_norm(x, 8, sd[name + ".weight"], sd[name + ".bias"], eps=1e-5)
    return _operand(F.gelu(x), store)


def _res(x, sd, p, store=None):
    x = _stored(x, store)
    h = _stored(F.conv2d(_gn_act(x, sd, p + ".norm1", store=store), sd[p + ".conv1.weight"], sd[p + ".conv1.bias"], padding=1), store)
    h = F.conv2d(_gn_act(h, sd, p + ".norm2", store=store), sd[p + ".conv2.weight"], sd[p + ".conv2.bias"], padding=1)
    if p + ".shortcut.weight" in sd:
        x = _stored(F.conv2d(x, sd[p + ".shortcut.weight"], sd[p + ".shortcut.bias"]), store)
    return _stored(h + x, store)


def layer_plan(ch_mults):
    """Names of the down / up modules in order: ('res', i) / ('down', i) / ('up', i)."""
    down, up = [], []
    n = len(ch_mults)
    for i in range(n):
        down += ["res", "res"] + (["down"] if i < n - 1 else [])
    for i in reversed(range(n)):
        up += ["res", "res", "res"] + (["up"] if i > 0 else [])
    return down, up


def forward(x, sd, time_window, ch_mults, norm=True, store=None):
    """x: (B, T, C, H, W) -> (B, T, C_out, H, W).

    store = torch.bfloat16 restates what bf16 storage alone does to an otherwise exact computation, at the points where the native path
    (ops.py) rounds:
      - value and gradient (_Stored): the image_proj output (_ProjFn: `out` in the compute dtype, `dout` arrives in it); in a residual
        block (_ResBlockFn) its input, whose gradient dx / ds leaves bf_gn_bwd in the compute dtype with the shortcut's gradient added,
        `h` (and its gradient dh), the 1x1 shortcut output and the block output (`dout.to(dt)`); the input and output of Downsample
        (_DownFn) and Upsample (_UpFn); the input of the final layer (_FinalFn: dx in the compute dtype).  Every input is rounded again
        where it is read, so a tensor with several consumers (the skips) has each consumer's gradient rounded before autograd sums them,
        and the sum rounded, as autograd does with bf16 gradients.
      - value only (_Operand): gelu(groupnorm(.)), the operand the prologue hands to the MFMAs of conv1 / conv2 / final; its gradient
        dA is fp32.
    Everything else -- the fp32 prediction, the conv accumulators, the fp32 data gradients -- stays in the input dtype."""
    B, T, C, H, W = x.shape
    h = _stored(F.conv2d(x.reshape(B, T * C, H, W), sd["image_proj.weight"], sd["image_proj.bias"]), store)
    skips = [h]
    down, up = layer_plan(ch_mults)
    for i, kind in enumerate(down):
        p = f"down.{i}"
        if kind == "res":
            h = _res(h, sd, p, store)
        else:
            h = _stored(F.conv2d(_stored(h, store), sd[p + ".conv.weight"], sd[p + ".conv.bias"], stride=2, padding=1), store)
        skips.append(h)
    h = _res(_res(h, sd, "middle.res1", store), sd, "middle.res2", store)
    for i, kind in enumerate(up):
        p = f"up.{i}"
        if kind == "up":
            h = _stored(F.conv_transpose2d(_stored(h, store), sd[p + ".conv.weight"], sd[p + ".conv.bias"], stride=2, padding=1), store)
        else:
            h = _res(torch.cat((h, skips.pop()), 1), sd, p, store)
    h = F.conv2d(_gn_act(_stored(h, store), sd, "norm", norm, store), sd["final.weight"], sd["final.bias"])
    return h.reshape(B, time_window, -1, H, W)


def lp_loss(pred, y):
    """Relative L2 over (H, W) per (b, t, c); mean over b, mean over t, sum over c."""
    d = (pred - y).flatten(-2).norm(dim=-1) / y.flatten(-2).norm(dim=-1)
    return d.mean(0).mean(0).sum()


def load_golden(name):
    """-> (spec, npz, fp64 state_dict) of tests/golden/unet_modern_<name>.npz."""
    from tools.gen_unet_golden import CONFIGS, weights
    from bubbleformer_amd.models.unets import ModernUnet
    spec = CONFIGS[name]
    z = np.load(os.path.join(GOLDEN, f"unet_modern_{name}.npz"))
    sd = weights(ModernUnet(**spec["cfg"]), spec["seed"])
    return spec, z, sd


def golden_grad_errors(grads, z, zero_tol=None):
    """Per parameter: relative error of `grads` against the golden gradient -- rel-L2 of the whole tensor, or, for the gradients the
    goldens keep as a sketch (tools/gen_unet_golden.py), the larger of the rel-L2 of the 16 projections and of the norm.  A golden that is
    zero up to rounding (a bias in front of a one-channel-per-group GroupNorm) is compared by the largest absolute value when
    `zero_tol` is given."""
    from tools.gen_unet_golden import sketch
    errs = {}
    for k, g in grads.items():
        g = g.detach().double().cpu()
        if "g:" + k in z.files:
            want = torch.from_numpy(z["g:" + k]).double()
            if zero_tol is not None and float(want.abs().max()) < 1e-9:
                errs[k] = float(g.abs().max()) * zero_tol
            else:
                errs[k] = float((g - want).norm() / want.norm())
        else:
            s_want = torch.from_numpy(z["s:" + k]).double()
            n_want = float(z["n:" + k])
            errs[k] = max(float((sketch(k, g) - s_want).norm() / s_want.norm()), abs(float(g.norm()) - n_want) / n_want)
    missing = {f[2:] for f in z.files if f[:2] in ("g:", "s:")} ^ set(grads)
    assert not missing, missing
    return errs


def run(x, y, sd, cfg, store=None):
    """fp64 (or the state_dict's dtype) forward + loss + backward -> (pred, loss, dx, {name: grad}); `store` as in forward()."""
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    x = x.detach().clone().requires_grad_(True)
    pred = forward(x, sd, cfg["time_window"], cfg["ch_mults"], cfg["norm"], store)
    loss = lp_loss(pred, y)
    loss.backward()
    return pred.detach(), loss.detach(), x.grad, {k: v.grad for k, v in sd.items() if v.grad is not None}
