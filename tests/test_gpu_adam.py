"""GPU: the fused Adam kernel (csrc/gradclip.hip: bf_adam, torch.optim.Adam semantics) against torch.optim.Adam, and TrainStep(optimizer="adam")
(config/optim_cfg/adam.yaml) on FiLMAViT against the oracle and on the classic U-Net."""
import numpy as np
import pytest
import torch

from tests.helpers import load_variant, rel_l2, structurally_zero

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [10007, 3, 4096])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-5, 0.1])
@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
def test_fused_adam_matches_torch(n, weight_decay, grad_scale):
    """Five steps, each applied by the kernel to two copies of the same state: unpadded buffers of exactly n elements (n = 10007 and 3 run
    the scalar tail on their last 3 elements, n = 3 nothing else; 4096 has no tail) and a buffer padded to a multiple of 64 plus 64
    zeros in p and g, as FlatParams lays it out.  Both follow torch.optim.Adam to the relative L2 bound of test_fused_adamw_matches_torch,
    and the padding stays exactly zero.  weight_decay 0.1 makes the L2 term (it passes through the moments) visible against AdamW's
    decoupled decay."""
    from bubbleformer_amd import ops
    g = torch.Generator(device="cuda").manual_seed(9)
    padded = (n + 63) // 64 * 64 + 64
    p0 = torch.randn(n, device="cuda", generator=g)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=2.5e-4, weight_decay=weight_decay)
    bufs = []
    for size in (n, padded):                         # [p, grad, m, v]; the unpadded ones are allocations of their own, 16-byte aligned
        t = [torch.zeros(size, device="cuda") for _ in range(4)]
        t[0][:n] = p0
        bufs.append(t)
    assert bufs[0][0].numel() == n and bufs[1][0].numel() % 4 == 0
    for step in range(1, 6):
        grad = torch.randn(n, device="cuda", generator=g)
        ref.grad = grad * grad_scale
        opt.step()
        for p, gb, m, v in bufs:
            gb[:n] = grad
            ops.adam_(p, gb, m, v, step, 2.5e-4, weight_decay=weight_decay, grad_scale=grad_scale)
            assert rel_l2(p[:n].cpu(), ref.detach().cpu()) < 1e-6, (step, p.numel())
    if n % 4:                                        # the tail elements on their own
        tail = slice(n - n % 4, n)
        assert rel_l2(bufs[0][0][tail].cpu(), ref.detach()[tail].cpu()) < 1e-6
    # the kernel takes beta2 as fp32, so its 1 - beta2 is 1 - 0.999f = 0.99998713e-3 where torch uses the double 1e-3: v carries that
    # 1.3e-5 relative offset (measured 1.29e-5, as bf_adamw's does), which reaches p only through sqrt(v) and the ratio m / sqrt(v)
    st = opt.state[ref]
    for p, gb, m, v in bufs:
        assert rel_l2(m[:n].cpu(), st["exp_avg"].cpu()) < 1e-6 and rel_l2(v[:n].cpu(), st["exp_avg_sq"].cpu()) < 2e-5
    p, _, m, v = bufs[1]
    for t in (p, m, v):
        assert not t[n:].any()


def test_fused_adam_is_not_adamw():
    """With weight decay the two rules differ: Adam's L2 term is normalised by the moments, AdamW's decay is not."""
    from bubbleformer_amd import ops
    g = torch.Generator(device="cuda").manual_seed(4)
    p0 = torch.randn(4096, device="cuda", generator=g)
    grad = torch.randn(4096, device="cuda", generator=g)
    out = []
    for fn in (ops.adam_, ops.adamw_):
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        fn(p, grad, m, v, 1, 1e-2, weight_decay=0.5)
        out.append(p)
    assert rel_l2((out[0] - p0).cpu(), (out[1] - p0).cpu()) > 0.1


def _tiny_d64():
    from bubbleformer_amd.models import get_model
    from oracle import weights as W
    spec, _ = load_variant("tiny_d64")
    cfg = dict(spec["cfg"])
    model = get_model(spec["model"], time_window=spec["T"], drop_path=0.0, compute_dtype=torch.float32, **cfg)
    model.load_state_dict(W.generate(W.param_shapes(**cfg), seed=spec["seed"]))
    return spec, model.cuda()


def test_adam_training_trajectory_matches_the_oracle_trained_with_torch():
    """Eight TrainStep(optimizer="adam") steps -- forward, fused loss, backward, fused Adam, per-batch cosine warm-up -- in fp32 against the
    oracle restatement in fp64 driven by torch.optim.Adam and the reference's scheduler formula, fresh input every step; the bounds and
    the skipped structurally zero families are those of test_training_trajectory_matches_the_oracle_trained_with_torch, and so is the
    weight decay 1e-2.  At these bounds this test does not tell Adam from AdamW; test_train_step_applies_adam_not_adamw does."""
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.lr_schedulers import CosineWarmupLR
    from oracle import filmavit_ref as R, weights as W
    spec, model = _tiny_d64()
    cfg = spec["cfg"]
    steps, base_lr, wd = 8, 2e-3, 1e-2
    sched = CosineWarmupLR(base_lr, 3, steps, 1e-6)
    step = TrainStep(model, lr=base_lr, weight_decay=wd, optimizer="adam", scheduler=sched)
    sd = {k: v.double().requires_grad_(True) for k, v in W.generate(W.param_shapes(**cfg), seed=spec["seed"]).items()}
    opt = torch.optim.Adam(list(sd.values()), lr=base_lr, weight_decay=wd)
    kw = dict(patch_size=cfg["patch_size"], num_heads=cfg["num_heads"])
    got, want = [], []
    for i in range(steps):
        x = W.synthetic_clip(spec["B"], spec["T"], cfg["input_fields"], spec["H"], spec["W"], 400 + i)
        y = W.synthetic_clip(spec["B"], spec["T"], cfg["output_fields"], spec["H"], spec["W"], 500 + i)
        c = W.synthetic_fluid_params(spec["B"], cfg["num_fluid_params"], 600 + i)
        got.append(float(step(x.cuda(), c.cuda(), y.cuda())))
        for v in sd.values():
            v.grad = None
        loss = R.lp_loss(R.filmavit_forward(sd, x.double(), c.double(), **kw), y.double())
        loss.backward()
        want.append(float(loss.detach()))
        with torch.no_grad():
            for gp in opt.param_groups:
                gp["lr"] = R.cosine_warmup_lr(i, base_lr, 3, steps, 1e-6)
            opt.step()
    assert np.allclose(got, want, rtol=2e-4), (got, want)
    torch.cuda.synchronize()
    for k, p_ in model.named_parameters():
        if not structurally_zero(k):
            assert rel_l2(p_.detach().cpu(), sd[k].detach()) < 5e-3, k


# TrainStep(optimizer="adam") against torch.optim.Adam (fp64) fed the gradients the native step left in the flat buffer: the kernel test's
# bound.  The same gradients fed to torch.optim.AdamW must land more than 100x further away.  Measured on one MI355X: 2.7e-8 and 4.4e-8
# against Adam, 1.2e-2 and 2.2e-2 against AdamW.
ADAM_STEP_TOL = 1e-6


def test_train_step_applies_adam_not_adamw():
    """Two TrainStep(optimizer="adam") steps on tiny_d64 in fp32 at weight decay 0.5.  After each step, the whole flat parameter buffer
    (padding included) equals torch.optim.Adam applied to the step's own flat gradient within ADAM_STEP_TOL.  torch.optim.AdamW fed the
    same gradients misses by more than 100x that bound, so a TrainStep that applied AdamW's rule would fail."""
    from bubbleformer_amd.trainer import TrainStep
    from oracle import weights as W
    spec, model = _tiny_d64()
    cfg = spec["cfg"]
    lr, wd = 1e-3, 0.5
    step = TrainStep(model, lr=lr, weight_decay=wd, optimizer="adam")
    refs = {}
    for name, cls in (("adam", torch.optim.Adam), ("adamw", torch.optim.AdamW)):
        p = torch.nn.Parameter(step.flat.flat.detach().double().clone())
        refs[name] = (p, cls([p], lr=lr, weight_decay=wd))
    errs = {"adam": [], "adamw": []}
    for i in range(2):
        x = W.synthetic_clip(spec["B"], spec["T"], cfg["input_fields"], spec["H"], spec["W"], 410 + i)
        y = W.synthetic_clip(spec["B"], spec["T"], cfg["output_fields"], spec["H"], spec["W"], 510 + i)
        c = W.synthetic_fluid_params(spec["B"], cfg["num_fluid_params"], 610 + i)
        step(x.cuda(), c.cuda(), y.cuda())
        torch.cuda.synchronize()
        grad = step.flat.grad.detach().double()
        for name, (p, opt) in refs.items():
            p.grad = grad.clone()
            opt.step()
            errs[name].append(rel_l2(step.flat.flat.cpu(), p.detach().cpu()))
    print("TrainStep(adam) vs torch Adam %s, vs torch AdamW %s" % (errs["adam"], errs["adamw"]))
    assert max(errs["adam"]) < ADAM_STEP_TOL, errs
    assert min(errs["adamw"]) > 100 * ADAM_STEP_TOL, errs


def test_unet_classic_adam_step_lowers_the_loss():
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.trainer import TrainStep
    from tests import unet_classic_restatement as U
    spec, z, p = U.load_golden("h8_c8_b3")
    m = get_model("unet_classic", compute_dtype=torch.float32, **spec["cfg"])
    m.load_state_dict({k: v.float() for k, v in p.items()}, strict=False)
    m = m.cuda()
    x = torch.from_numpy(z["x"]).float().cuda()
    y = torch.from_numpy(z["y"]).float().cuda()
    step = TrainStep(m, lr=1e-3, weight_decay=1e-5, optimizer="adam")
    losses = [float(step(x, None, y)) for _ in range(2)]
    assert all(np.isfinite(losses)) and losses[1] < losses[0], losses
    assert step.step_no == 2 and step.v.abs().sum() > 0


def test_fit_with_adam_trains_and_resumes(tmp_path):
    """fit(optimizer="adam") with adam.yaml's hyperparameters (lr 2.5e-4 scaled up for a 6-step run, wd 1e-5): the loss falls over two
    epochs, the checkpoint records the optimizer, and a run resumed from the end of epoch 0 repeats epoch 1."""
    import os
    import shutil
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.fit import fit
    from bubbleformer_amd.models import get_model
    samples = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samples")

    def make():
        torch.manual_seed(0)
        return get_model("avit", input_fields=4, output_fields=4, time_window=4, patch_size=8, embed_dim=64, num_heads=2, processor_blocks=2,
                         drop_path=0.0, compute_dtype=torch.float32).cuda()
    tr = BubbleForecast([os.path.join(samples, "sample_1.hdf5")], norm="std", time_window=4, start_time=5)
    tr.normalize()
    kw = dict(batch_size=4, max_epochs=2, optimizer="adam", lr=2e-3, weight_decay=1e-5, warmup_iters=2, eta_min=1e-6, limit_train_batches=3,
              seed=42)
    ck, ck0 = str(tmp_path / "last.ckpt"), str(tmp_path / "after_epoch0.ckpt")

    def log(e):
        if e.get("epoch") == 1 and e.get("batch_idx") == 0:
            shutil.copy(ck, ck0)
    h = fit(make(), tr, None, checkpoint_path=ck, log=log, **kw)
    assert np.isfinite(h["train_loss"]).all() and h["epoch_train_loss"][1] < h["epoch_train_loss"][0]
    saved = torch.load(ck, weights_only=False)["optimizer_states"][0]
    assert saved["name"] == "adam" and saved["step"] == 6 and saved["v"].abs().sum() > 0
    h2 = fit(make(), tr, None, resume_from=ck0, **kw)
    assert np.allclose(h2["lr"], h["lr"][3:], rtol=1e-12) and np.allclose(h2["train_loss"], h["train_loss"][3:], rtol=1e-4)


def test_fit_without_schedule_records_the_reference_checkpoint_lr(tmp_path):
    """fit(warmup_iters=None, resume_from=<reference checkpoint>): with no schedule the optimizer runs at the checkpoint's param_groups[0]
    lr, as Optimizer.load_state_dict leaves it, and hist["lr"] reports that lr, not fit's own argument."""
    import os
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.fit import fit
    from bubbleformer_amd.models import get_model
    samples = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samples")

    def make():
        torch.manual_seed(0)
        return get_model("avit", input_fields=4, output_fields=4, time_window=4, patch_size=8, embed_dim=64, num_heads=2, processor_blocks=2,
                         drop_path=0.0, compute_dtype=torch.float32)
    model = make()
    params = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    opt = torch.optim.Adam(params, lr=3e-4, weight_decay=1e-5)           # a reference run's optimizer after one step
    g = torch.Generator().manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g) * 1e-2
    opt.step()
    path = str(tmp_path / "hpc_ckpt_1.ckpt")
    torch.save({"epoch": 0, "global_step": 1, "state_dict": {"model." + k: v for k, v in model.state_dict().items()},
                "optimizer_states": [opt.state_dict()], "lr_schedulers": [], "hyper_parameters": {"optim_cfg": {"name": "adam"}}}, path)
    tr = BubbleForecast([os.path.join(samples, "sample_1.hdf5")], norm="std", time_window=4, start_time=5)
    tr.normalize()
    h = fit(make().cuda(), tr, None, batch_size=4, max_epochs=2, optimizer="adam", lr=2e-3, weight_decay=1e-5, warmup_iters=None,
            limit_train_batches=3, resume_from=path)
    assert h["lr"] == [3e-4] * 3 and np.isfinite(h["train_loss"]).all()
