"""GPU: gradient clipping and gradient accumulation in the training step.

csrc/gradclip.hip (bf_grad_norm, bf_adamw / bf_adam / bf_lion with coef_dev / clip_value) against fp64 torch and against torch.nn.utils.clip_grad_norm_ /
clip_grad_value_; TrainStep(gradient_clip_val, gradient_clip_algorithm, accumulate_grad_batches) and fit() with the same arguments.
Every test runs under a watchdog of its own (STEP_LIMIT_S): a test that hangs ends the process instead of starting the next one."""
import faulthandler
import math
import os
import shutil
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.helpers import load_variant, rel_l2

pytestmark = pytest.mark.gpu
STEP_LIMIT_S = 240
ULP = 2.0 ** -23

SMALL = dict(input_fields=4, output_fields=4, patch_size=16, embed_dim=384, num_heads=6, processor_blocks=12, num_fluid_params=9)


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def _small_flat_size(align=64):
    """The flat buffer TrainStep keeps for FiLMAViT-small: every parameter padded to 64 elements (trainer.FlatParams)."""
    from oracle import weights as W
    return sum((math.prod(s) + align - 1) // align * align for s in W.param_shapes(**SMALL).values())


def _spread_gradient(n, seed):
    """Magnitudes log-uniform over 1e-8 .. 1e3, random signs, and (as in FlatParams) a few runs of exact zeros."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, device="cuda", generator=g, dtype=torch.float64) * 11.0 - 8.0)
    sign = torch.where(torch.rand(n, device="cuda", generator=g) < 0.5, -1.0, 1.0)
    out = (mag * sign).float()
    if n >= 4160:
        out[4100:4160] = 0.0
    return out


# ------------------------------------------------------------------------------------------------ the norm
@pytest.mark.parametrize("n", [64, 4160, "small"])
@pytest.mark.parametrize("gscale", [1.0, 0.125])
def test_grad_norm_matches_fp64_within_one_ulp(n, gscale):
    """norm within one fp32 ulp (relative 2^-23) of gscale * sqrt(sum g^2) in fp64 -- fp64 accumulation of at most 2^25 addends leaves a
    relative 2^-28, the one rounding to fp32 2^-24; coef within one ulp of min(max_norm / (norm + 1e-6), 1) evaluated in fp32 on the
    returned norm, exactly 1.0 where max_norm is above the norm; two calls on one buffer are bit-equal."""
    from bubbleformer_amd import ops
    n = _small_flat_size() if n == "small" else n
    if n > 4160:
        assert n % 64 == 0 and n > 28906602
    grad = _spread_gradient(n, seed=n % 1000)
    want = gscale * float(grad.double().pow(2).sum().sqrt())
    for max_norm, clipped in ((4.0 * want, False), (0.37 * want, True)):
        out, again = torch.zeros(2, device="cuda"), torch.full((2,), -1.0, device="cuda")
        ops.grad_norm_(grad, out, max_norm, gscale)
        ops.grad_norm_(grad, again, max_norm, gscale, ws=ops.grad_norm_workspace(n, grad.device))
        torch.cuda.synchronize()
        norm, coef = float(out[0]), float(out[1])
        print(f"n {n} gscale {gscale} max_norm {max_norm:.6g}: norm {norm:.9g} (fp64 {want:.12g}, rel {abs(norm - want) / want:.3g}), coef {coef:.9g}")
        assert torch.equal(out, again)
        assert abs(norm - want) <= ULP * want
        ref = torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (out[0].cpu() + torch.tensor(1e-6, dtype=torch.float32)), max=1.0)
        assert abs(coef - float(ref)) <= ULP * float(ref)
        assert (coef == 1.0) == (not clipped) and (not clipped or abs(coef - 0.37) < 1e-5)


def test_grad_norm_tail_nan_and_bad_arguments():
    """n % 4 != 0 (the trailing elements join the last slab), a NaN element (NaN norm and NaN coefficient, as torch.clamp leaves it), an
    infinite one (coefficient 0), and the refusals: max_norm <= 0, a missing output."""
    from bubbleformer_amd import _lib, ops
    grad = _spread_gradient(4163, seed=5)
    out = torch.zeros(2, device="cuda")
    ops.grad_norm_(grad, out, 1.0)
    want = float(grad.double().norm())
    assert abs(float(out[0]) - want) <= ULP * want
    grad[17] = float("nan")
    ops.grad_norm_(grad, out, 1.0)
    assert torch.isnan(out).all()
    grad[17] = float("inf")
    ops.grad_norm_(grad, out, 1.0)
    assert float(out[0]) == float("inf") and float(out[1]) == 0.0
    for bad in (0.0, -1.0):
        with pytest.raises(_lib.BubbleformerHipError):
            ops.grad_norm_(grad, out, bad)
    ws = ops.grad_norm_workspace(grad.numel(), grad.device)
    assert _lib.lib().bf_grad_norm(grad.data_ptr(), grad.numel(), 1.0, 1.0, None, ws.data_ptr(), ws.numel(), None) != 0


# ------------------------------------------------------------------------------------------------ the optimizers on a device coefficient
def _opt_call(ops, name, bufs, step, **kw):
    p, g, m, v = bufs
    if name == "lion":
        ops.lion_(p, g, m, 1e-3, weight_decay=0.1, grad_scale=0.25, **kw)
    else:
        getattr(ops, name + "_")(p, g, m, v, step, 1e-3, weight_decay=0.1, grad_scale=0.25, **kw)


@pytest.mark.parametrize("name", ["adamw", "adam", "lion"])
@pytest.mark.parametrize("n", [10007, 4096])
def test_dev_optimizers_with_unit_coefficient_are_the_host_kernels_bit_for_bit(name, n):
    """coef = 1.0f and no clamp: gscale * 1.0f is gscale, the loop body is the same code, so p, m and v after three steps are
    torch.equal to the host-scale entry points' (n = 10007 runs the scalar tail)."""
    from bubbleformer_amd import ops
    g = torch.Generator(device="cuda").manual_seed(3)
    p0 = torch.randn(n, device="cuda", generator=g)
    host = [p0.clone(), None, torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    devs = {k: [p0.clone(), None, torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")] for k in ("coef", "null")}
    one = torch.ones(1, device="cuda")
    for step in range(1, 4):
        grad = _spread_gradient(n, seed=step) * 1e-2
        host[1] = grad
        _opt_call(ops, name, host, step)
        for k, bufs in devs.items():
            bufs[1] = grad
            _opt_call(ops, name, bufs, step, **({"coef": one} if k == "coef" else {"clip_value": float("inf")}))
    torch.cuda.synchronize()
    for k, bufs in devs.items():
        for a, b in zip((host[0], host[2], host[3]), (bufs[0], bufs[2], bufs[3])):
            assert torch.equal(a, b), (name, k)


def _torch_reference(name, ref, lr, wd):
    if name == "adamw":
        return torch.optim.AdamW([ref], lr=lr, weight_decay=wd)
    if name == "adam":
        return torch.optim.Adam([ref], lr=lr, weight_decay=wd)
    return None


def _lion_reference_step(p, grad, m, lr, wd, b1=0.9, b2=0.99):
    """lion_pytorch.Lion's update in fp64."""
    p.mul_(1 - lr * wd).sub_(lr * torch.sign(b1 * m + (1 - b1) * grad))
    m.mul_(b2).add_((1 - b2) * grad)


@pytest.mark.parametrize("name", ["adamw", "adam", "lion"])
@pytest.mark.parametrize("algorithm", ["norm", "value"])
def test_clipped_optimizers_match_torch_clipping(name, algorithm):
    """Five steps of the kernel with the device coefficient (or the clamp) against the torch optimizer (Lion: lion_pytorch's rule in fp64)
    fed gradients clipped by torch.nn.utils.clip_grad_norm_ / clip_grad_value_, grad_scale 0.25 applied first as the averaged gradient
    is.  Bounds: test_gpu_adam.py's -- relative L2 < 1e-6 on parameters and first moment, 2e-5 on the second."""
    from bubbleformer_amd import ops
    n, lr, wd, gscale = 10007, 2.5e-4, 0.1, 0.25
    g = torch.Generator(device="cuda").manual_seed(21)
    p0 = torch.randn(n, device="cuda", generator=g)
    ref = torch.nn.Parameter(p0.double().clone())      # fp64 reference: its clip coefficient and its moments carry no rounding of their own
    opt = _torch_reference(name, ref, lr, wd)
    m_ref = torch.zeros(n, device="cuda", dtype=torch.float64)
    p, m, v = p0.clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    out = torch.zeros(2, device="cuda")
    clipped_steps = 0
    for step in range(1, 6):
        grad = torch.randn(n, device="cuda", generator=g) * (4.0 if step % 2 else 0.02)      # above and below the threshold
        ref.grad = grad.double() * gscale
        if algorithm == "norm":
            max_norm = 20.0
            total = torch.nn.utils.clip_grad_norm_([ref], max_norm)
            clipped_steps += int(float(total) > max_norm)
            ops.grad_norm_(grad, out, max_norm, gscale)
            kw = {"coef": out[1:]}
        else:
            clipped_steps += int(float(ref.grad.abs().max()) > 0.5)
            torch.nn.utils.clip_grad_value_([ref], 0.5)
            kw = {"clip_value": 0.5}
        if opt is not None:
            opt.step()
            ops.adamw_(p, grad, m, v, step, lr, weight_decay=wd, grad_scale=gscale, **kw) if name == "adamw" else \
                ops.adam_(p, grad, m, v, step, lr, weight_decay=wd, grad_scale=gscale, **kw)
        else:
            with torch.no_grad():
                _lion_reference_step(ref.data, ref.grad, m_ref, lr, wd)
            ops.lion_(p, grad, m, lr, weight_decay=wd, grad_scale=gscale, **kw)
        assert rel_l2(p.cpu(), ref.detach().cpu()) < 1e-6, step
    assert 0 < clipped_steps < 5          # both sides of the threshold were exercised
    if opt is not None:
        st = opt.state[ref]
        assert rel_l2(m.cpu(), st["exp_avg"].cpu()) < 1e-6 and rel_l2(v.cpu(), st["exp_avg_sq"].cpu()) < 2e-5
    else:
        assert rel_l2(m.cpu(), m_ref.cpu()) < 1e-6


# ------------------------------------------------------------------------------------------------ TrainStep
def _tiny(name="filmavit", B=2):
    """(model, batches): a tiny model in fp32 parity mode without stochastic depth, and a function i -> (x, fluid, y) on the device."""
    from bubbleformer_amd.models import get_model
    from oracle import weights as W
    if name == "filmavit_bf16":
        # the smallest geometry at which the project pins a bit-reproducible bf16 training step (test_gpu_baseline_configs.py:
        # test_training_step_is_bit_reproducible_run_to_run -- 16 x 192 x 192 clips at patch 16, E 384), two blocks deep.  On smaller token
        # grids, and in the fp32 parity mode, a few small attention / norm parameter gradients are float-atomic sums and differ run to run.
        cfg = dict(SMALL, processor_blocks=2)
        model = get_model("filmavit", time_window=16, drop_path=0.0, compute_dtype=torch.bfloat16, **cfg)
        model.load_state_dict(W.generate(W.param_shapes(**cfg), seed=31))

        def data(i, B=B):
            return (W.synthetic_clip(B, 16, 4, 192, 192, 700 + i).cuda(), W.synthetic_fluid_params(B, 9, 900 + i).cuda(),
                    W.synthetic_clip(B, 16, 4, 192, 192, 800 + i).cuda())
        return model.cuda().train(), data
    if name == "filmavit":
        spec, _ = load_variant("tiny_d64")
        cfg = dict(spec["cfg"])
        model = get_model("filmavit", time_window=spec["T"], drop_path=0.0, compute_dtype=torch.float32, **cfg)
        model.load_state_dict(W.generate(W.param_shapes(**cfg), seed=spec["seed"]))

        def data(i, B=B):
            return (W.synthetic_clip(B, spec["T"], cfg["input_fields"], spec["H"], spec["W"], 700 + i).cuda(),
                    W.synthetic_fluid_params(B, cfg["num_fluid_params"], 900 + i).cuda(),
                    W.synthetic_clip(B, spec["T"], cfg["output_fields"], spec["H"], spec["W"], 800 + i).cuda())
        return model.cuda().train(), data
    from tests import unet_classic_restatement as U
    spec, _, p = U.load_golden("h8_c8_b3")
    cfg = spec["cfg"]
    model = get_model("unet_classic", compute_dtype=torch.float32, **cfg)
    model.load_state_dict({k: v.float() for k, v in p.items()}, strict=False)

    def data(i, B=B):
        g = torch.Generator().manual_seed(40 + i)
        return (torch.randn(B, cfg["time_window"], cfg["input_fields"], spec["H"], spec["W"], generator=g).cuda(), None,
                torch.randn(B, cfg["time_window"], cfg["output_fields"], spec["H"], spec["W"], generator=g).cuda())
    return model.cuda().train(), data


@pytest.mark.parametrize("optimizer", ["adamw", "adam", "lion"])
def test_clipping_that_never_bites_changes_no_bit(optimizer):
    """Three steps with gradient_clip_val = 1e30 (norm and coefficient computed, coefficient exactly 1) against three steps without:
    parameters, moments and losses are torch.equal.  Run where the step itself is bit-reproducible (_tiny("filmavit_bf16")): two runs
    WITHOUT clipping differ in the last bits anywhere else."""
    from bubbleformer_amd.trainer import TrainStep
    runs = []
    for clip in (None, 1e30):
        model, data = _tiny("filmavit_bf16")
        step = TrainStep(model, lr=1e-3, weight_decay=1e-2, optimizer=optimizer, gradient_clip_val=clip)
        losses = [step(*data(i)) for i in range(3)]
        torch.cuda.synchronize()
        runs.append((step.flat.flat.clone(), step.m.clone(), None if step.v is None else step.v.clone(), torch.stack(losses), step))
    a, b = runs
    assert a[4].grad_norm is None and float(b[4].grad_norm[1]) == 1.0 and float(b[4].grad_norm[0]) > 0
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    assert (a[2] is None and b[2] is None) or torch.equal(a[2], b[2])
    assert a[4].step_no == b[4].step_no == 3


def test_lion_step_clipped_to_half_the_norm_keeps_its_sign_pattern():
    """Lion's first step moves every parameter by lr * sign(gradient): clipping to half the measured norm halves the gradient and leaves
    every sign, so the parameters after the step are the unclipped run's bit for bit; the coefficient is 1/2 (up to the 1e-6 in its
    denominator) and the momentum is that fraction of the unclipped one."""
    from bubbleformer_amd.trainer import TrainStep
    model, data = _tiny("filmavit_bf16")            # a bit-reproducible step: both runs see the same gradient
    free = TrainStep(model, lr=1e-3, weight_decay=0.0, optimizer="lion", gradient_clip_val=1e30)
    free(*data(0))
    norm = float(free.grad_norm[0])
    model2, _ = _tiny("filmavit_bf16")
    half = TrainStep(model2, lr=1e-3, weight_decay=0.0, optimizer="lion", gradient_clip_val=0.5 * norm)
    half(*data(0))
    torch.cuda.synchronize()
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    coef = float(half.grad_norm[1])
    want = float(f32(0.5 * norm) / (f32(norm) + f32(1e-6)))          # 1/2 up to the 1e-6 in the denominator
    assert float(half.grad_norm[0]) == norm and abs(coef - want) <= ULP * want and 0.49 < coef <= 0.5
    assert torch.equal(half.flat.flat, free.flat.flat)
    assert (free.m != 0).any() and torch.equal(torch.sign(half.m), torch.sign(free.m))
    assert rel_l2(half.m.cpu(), coef * free.m.cpu()) < 1e-6


def test_value_clipping_in_the_step_clamps_the_averaged_gradient():
    """gradient_clip_algorithm="value": one Adam step equals torch.optim.Adam fed the step's own flat gradient clamped by clip_grad_value_."""
    from bubbleformer_amd.trainer import TrainStep
    model, data = _tiny()
    step = TrainStep(model, lr=1e-3, weight_decay=0.0, optimizer="adam", gradient_clip_val=1e-4, gradient_clip_algorithm="value")
    ref = torch.nn.Parameter(step.flat.flat.detach().double().clone())
    opt = torch.optim.Adam([ref], lr=1e-3)
    step(*data(0))
    torch.cuda.synchronize()
    assert step.grad_norm is None
    ref.grad = step.flat.grad.detach().double().clone()
    assert float(ref.grad.abs().max()) > 1e-4          # the clamp bites
    torch.nn.utils.clip_grad_value_([ref], 1e-4)
    opt.step()
    assert rel_l2(step.flat.flat.cpu(), ref.detach().cpu()) < 1e-6


PARITY = 1e-4      # the project's fp32 parity bound (README): relative L2 per tensor


def _per_tensor(flat, buf):
    return [buf[o:o + p.numel()] for p, o in zip(flat.params, flat.offsets)]


@pytest.mark.parametrize("name", ["filmavit", "unet_classic"])
def test_two_micro_batches_of_four_equal_one_batch_of_eight(name):
    """accumulate_grad_batches=2 over two micro-batches of 4 against one step on the batch of 8: every gradient tensor and every parameter
    after the step within the fp32 parity bound.  The losses are means over the batch, so the sum of the two micro-gradients times 1/2 is the
    gradient of the batch of 8.  A writer that overwrote instead of adding would leave the second micro-batch's gradient alone (times
    1/2): the one-micro-batch control below shows that this is O(1) away.  step_no and the schedule advance once per group.

    The optimizer step under comparison is AdamW's first at lr = 1, eps = 1: p -= g / (|g| + 1) per element, a map with Lipschitz constant 1,
    so the parameters inherit the gradients' bound.  (At the default eps = 1e-8 the first step is lr * sign(g): an element whose gradient is
    small beside its tensor's norm may flip, which says nothing about accumulation.)

    unet_classic normalises with BatchNorm over the batch a call sees (as the reference does under accumulation), so two different halves
    are not the function the batch of 8 is: its second micro-batch is the first in reverse order -- equal batch statistics, the same
    sum of gradients -- and the control is the first micro-batch alone."""
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.lr_schedulers import CosineWarmupLR
    _, data = _tiny(name, B=4)
    x0, c0, y0 = data(0)
    if name == "unet_classic":
        x1, c1, y1 = x0.flip(0), None, y0.flip(0)
    else:
        x1, c1, y1 = data(1)
    cat = lambda a, b: None if a is None else torch.cat([a, b])

    def run(k, calls):
        model, _ = _tiny(name, B=4)
        sched = CosineWarmupLR(2.0, 2, 10, 1e-6)
        sched.step()                                   # one step into the warm-up (the schedule's first learning rate is 0): lr = 1
        step = TrainStep(model, lr=2.0, weight_decay=1e-2, eps=1.0, optimizer="adamw", scheduler=sched, accumulate_grad_batches=k)
        p0 = step.flat.flat.clone()
        seen = []
        for args in calls:
            step(*args)
            seen.append((step.step_no, step.scheduler.get_last_lr()[0], step.micro))
        torch.cuda.synchronize()
        return step, p0, seen

    whole, p0, _ = run(1, [(cat(x0, x1), cat(c0, c1), cat(y0, y1))])
    acc, _, seen = run(2, [(x0, c0, y0), (x1, c1, y1)])
    assert seen == [(0, 1.0, 1), (1, 2.0, 0)], seen            # step_no and the schedule advance once per group
    assert rel_l2(acc.flat.flat.cpu(), p0.cpu()) > 100 * PARITY      # the step moved the parameters far more than the bound below
    worst = 0.0
    for (k, _), gw, ga, pw, pa in zip(whole.model.named_parameters(), _per_tensor(whole.flat, whole.flat.grad),
                                      _per_tensor(acc.flat, acc.flat.grad * 0.5), _per_tensor(whole.flat, whole.flat.flat),
                                      _per_tensor(acc.flat, acc.flat.flat)):
        if float(gw.abs().max()) == 0.0 or k.endswith(("knorm.bias", "mlp.fc2.bias")):      # structurally zero gradients: rounding noise on both sides
            assert float(ga.abs().max()) <= 1e-5 * float(whole.flat.grad.abs().max()), k
        else:
            e = rel_l2(ga.cpu(), gw.cpu())
            worst = max(worst, e)
            assert e <= PARITY, (k, e)
        assert rel_l2(pa.cpu(), pw.cpu()) <= PARITY, k
    print(f"{name}: worst gradient rel-L2, accumulated against whole batch: {worst:.3e}")
    # control: one micro-batch alone, scaled as the accumulated run scales, is O(1) away from the batch of 8
    single, _, _ = run(1, [(x0, c0, y0)])
    assert rel_l2((single.flat.grad * 0.5).cpu(), whole.flat.grad.cpu()) > 0.3


def _accumulated_twice(name, B):
    from bubbleformer_amd.trainer import TrainStep
    runs = []
    for _ in range(2):
        model, data = _tiny(name, B=B)
        step = TrainStep(model, lr=1e-3, weight_decay=1e-2, optimizer="adamw", accumulate_grad_batches=2, gradient_clip_val=1e-3)
        for i in range(2):
            step(*data(i))
        torch.cuda.synchronize()
        assert step.step_no == 1
        runs.append(step)
    return runs


@pytest.mark.parametrize("name", ["filmavit", "unet_classic"])
def test_accumulated_step_repeats_bit_for_bit(name):
    """The accumulated step (two micro-batches of 4, k = 2, fp32 parity mode) run twice from the same state: gradients, norm, parameters
    and moments are torch.equal.  What that rests on beside the step's slab sums: the generic attention backward (csrc/attn.hip
    attn_bwd_kernel) leaves its small parameter gradients as one workspace row per workgroup, summed in row order; the stage-0 patch
    weight gradient is a slab sum where the 16-wide stream declines; and the W and the H pass of a spatial stage, which share their
    LayerNorms and bias table, add into those slots one after the other from the same threads (launch_reduce_jobs) -- as concurrent
    workgroups their two addends were order free only on a zeroed slot, which the second micro-batch does not find."""
    a, b = _accumulated_twice(name, 4)
    differing = [k for (k, _), ga, gb in zip(a.model.named_parameters(), _per_tensor(a.flat, a.flat.grad), _per_tensor(b.flat, b.flat.grad))
                 if not torch.equal(ga, gb)]
    print(f"{name}: {len(differing)} gradient tensors differ between two accumulated runs: {differing[:8]}")
    assert not differing, differing
    assert torch.equal(a.grad_norm, b.grad_norm) and torch.equal(a.flat.flat, b.flat.flat) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)


def test_accumulated_bf16_step_repeats_on_the_single_writer_families():
    """The same in bf16 at the geometry where the plain step is bit-reproducible (test_training_step_is_bit_reproducible_run_to_run).
    The families test_gpu_ddp.py pins as produced by one writer in a fixed order (EXACT: the trunk's conv / Linear weights and biases)
    are torch.equal; every tensor agrees to that file's bound for the others (relative L2 1e-4).  The others are not pinned bit for bit
    here: a slot that takes one addend from each of the library's two queues (norm2's bias: outproj_finalize_kernel on the side stream,
    the stage's InstanceNorm job on the caller's) is order free on a zeroed slot only, and under accumulation nothing orders the two."""
    from tests.test_gpu_ddp import EXACT
    a, b = _accumulated_twice("filmavit_bf16", 2)
    n_exact, differing = 0, []
    for (k, _), ga, gb in zip(a.model.named_parameters(), _per_tensor(a.flat, a.flat.grad), _per_tensor(b.flat, b.flat.grad)):
        if k.startswith("blocks.") and k.endswith(EXACT):
            assert torch.equal(ga, gb), k
            n_exact += 1
        elif not torch.equal(ga, gb):
            differing.append(k)
            assert float((ga - gb).norm()) <= 1e-4 * float(gb.norm()) + 1e-12, k
    print(f"filmavit_bf16: {len(differing)} of {len(a.flat.params)} gradient tensors differ between two accumulated runs: {differing}")
    assert n_exact == 2 * (2 * 2 + 4)
    assert abs(float(a.grad_norm[0]) - float(b.grad_norm[0])) <= ULP * float(b.grad_norm[0])


def test_finish_accumulation_steps_on_a_partial_group_with_the_full_factor():
    """One micro-batch pending of k = 2, then finish_accumulation(): one optimizer step on gscale = 1/2 (Lightning on an epoch's last
    batch), i.e. torch.optim.Adam on half the micro-batch's gradient; a second call does nothing."""
    from bubbleformer_amd.trainer import TrainStep
    model, data = _tiny()
    step = TrainStep(model, lr=1e-3, weight_decay=0.0, optimizer="adam", accumulate_grad_batches=2)
    ref = torch.nn.Parameter(step.flat.flat.detach().double().clone())
    opt = torch.optim.Adam([ref], lr=1e-3)
    step(*data(0))
    assert step.step_no == 0 and step.micro == 1 and torch.equal(step.flat.flat.double(), ref.detach())
    assert step.finish_accumulation() and step.step_no == 1 and step.micro == 0
    assert not step.finish_accumulation() and step.step_no == 1
    torch.cuda.synchronize()
    ref.grad = step.flat.grad.detach().double() * 0.5
    opt.step()
    assert rel_l2(step.flat.flat.cpu(), ref.detach().cpu()) < 1e-6


# ------------------------------------------------------------------------------------------------ fit()
def test_fit_with_accumulation_and_clipping_steps_six_times_and_resumes(tmp_path):
    """5 batches per epoch, k = 2, 2 epochs: optimizer steps after batches 1, 3 and 4 of each epoch -- 6 in all, one gradient norm each;
    the learning rate of a batch is that of the 6-step schedule at the optimizer step it belongs to; a run resumed from the epoch-0
    checkpoint repeats epoch 1."""
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.fit import fit
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils.lr_schedulers import CosineWarmupLR
    samples = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samples")

    def make():
        torch.manual_seed(0)
        return get_model("avit", input_fields=4, output_fields=4, time_window=4, patch_size=8, embed_dim=64, num_heads=2, processor_blocks=2,
                         drop_path=0.0, compute_dtype=torch.float32).cuda()
    tr = BubbleForecast([os.path.join(samples, "sample_1.hdf5")], norm="std", time_window=4, start_time=5)
    tr.normalize()
    kw = dict(batch_size=4, max_epochs=2, optimizer="adamw", lr=2e-3, weight_decay=1e-2, warmup_iters=2, eta_min=1e-6, limit_train_batches=5,
              seed=42, accumulate_grad_batches=2, gradient_clip_val=0.05)
    ck, ck0 = str(tmp_path / "last.ckpt"), str(tmp_path / "after_epoch0.ckpt")
    events = []

    def log(e):
        events.append(e)
        if e.get("epoch") == 1 and e.get("batch_idx") == 0:
            shutil.copy(ck, ck0)
    h = fit(make(), tr, None, checkpoint_path=ck, log=log, **kw)
    assert len(h["train_loss"]) == 10 and len(h["lr"]) == 10 and len(h["grad_norm"]) == 6
    assert np.isfinite(h["train_loss"]).all() and np.isfinite(h["grad_norm"]).all() and min(h["grad_norm"]) > 0
    ref = CosineWarmupLR(2e-3, 2, 6, 1e-6)
    want = []
    for _ in range(6):
        want.append(ref.get_last_lr()[0]); ref.step()
    per_batch = [want[s] for s in (0, 0, 1, 1, 2, 3, 3, 4, 4, 5)]
    assert np.allclose(h["lr"], per_batch, rtol=1e-12)
    assert [e["global_step"] for e in events] == [0, 1, 1, 2, 3, 3, 4, 4, 5, 6]
    stepped = [e for e in events if "grad_norm" in e]
    assert [(e["epoch"], e["batch_idx"]) for e in stepped] == [(0, 1), (0, 3), (0, 4), (1, 1), (1, 3), (1, 4)]
    assert all(e["grad_norm"].is_cuda and e["grad_norm"].dim() == 0 for e in stepped)
    assert [float(e["grad_norm"]) for e in stepped] == h["grad_norm"]
    saved = torch.load(ck, weights_only=False)
    assert saved["epoch"] == 1 and saved["global_step"] == 6 and saved["optimizer_states"][0]["step"] == 6
    h2 = fit(make(), tr, None, resume_from=ck0, **kw)
    assert len(h2["train_loss"]) == 5 and np.allclose(h2["lr"], per_batch[5:], rtol=1e-12)
    assert np.allclose(h2["train_loss"], h["train_loss"][5:], rtol=1e-4) and np.allclose(h2["grad_norm"], h["grad_norm"][3:], rtol=1e-4)


# ------------------------------------------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, out, backend):
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True, file=sys.stderr)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    torch.cuda.set_device(rank if backend == "nccl" else 0)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from bubbleformer_amd.trainer import TrainStep
    model, data = _tiny()
    step = TrainStep(model, lr=1e-3, weight_decay=1e-2, optimizer="adamw", gradient_clip_val=1e-3, accumulate_grad_batches=2)
    nb = max(step.reducer.bucket_of_ptr.values()) + 1
    logs = []
    for i in range(2):
        step(*data(10 * rank + i))          # every rank trains on clips of its own
        logs.append(list(step.reducer.launch_log))
        if i == 0:
            assert step.reducer.pending == [0] * nb and not step.reducer.handles and step.reducer.held is None
    torch.cuda.synchronize()
    torch.save({"logs": logs, "nb": nb, "pair": step.grad_norm.cpu(), "flat": step.flat.flat.cpu(), "step_no": step.step_no}, out + str(rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("backend", ["gloo", "nccl"])
def test_two_ranks_agree_on_the_clip_coefficient_and_hold_their_collectives(tmp_path, backend):
    """World size 2, each rank on clips of its own, k = 2, clipping by norm: the first micro-step launches no collective, the second one
    per bucket; norm and coefficient (computed after the exchange, on the averaged gradient) are bit-equal on the two ranks, and so are
    the parameters after the step.  "nccl" = RCCL, one GPU per rank; "gloo" runs both ranks on one GPU as test_gpu_ddp.py does."""
    if backend == "nccl" and torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (RCCL over xGMI); the one-GPU box runs the gloo variant")
    out = str(tmp_path / "rank")
    mp.spawn(_rank_worker, args=(2, _free_port(), out, backend), nprocs=2, join=True)
    a, b = torch.load(out + "0"), torch.load(out + "1")
    for r in (a, b):
        assert r["logs"][0] == [] and sorted(r["logs"][1]) == list(range(r["nb"])) and r["step_no"] == 1
    assert a["logs"][1] == b["logs"][1]
    assert torch.equal(a["pair"], b["pair"]) and 0 < float(a["pair"][1]) < 1 and float(a["pair"][0]) > 1e-3
    assert torch.equal(a["flat"], b["flat"])
