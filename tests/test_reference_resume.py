"""Resuming the reference's Lightning training runs: the CPU conversion of a torch.optim state dict into the flat optimizer buffers
(utils/checkpoint.py: flat_state_from_torch_optim) and its refusals, the import of a real reference checkpoint
(tests/golden/reference_resume_*.pt, written by tools/gen_reference_resume_golden.py) into a TrainStep, and, on the GPU, the
continued run against the reference's own continuation."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import structurally_zero

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fixture(name):
    return torch.load(os.path.join(GOLDEN, f"reference_resume_{name}.pt"), weights_only=True)


def _native_model(spec, device="cpu"):
    from bubbleformer_amd.models import get_model
    return get_model("filmavit", time_window=spec["T"], drop_path=0.0, compute_dtype=torch.float32, **spec["cfg"]).to(device)


def _flat(model):
    from bubbleformer_amd.trainer import FlatParams
    return FlatParams(model)


def _stepped_torch_optimizer(params, cls, steps=3, **kw):
    ps = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt = cls(ps, **kw)
    g = torch.Generator().manual_seed(3)
    for _ in range(steps):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt


def _padding_mask(flat):
    mask = torch.ones(flat.numel, dtype=torch.bool)
    for p, o in zip(flat.params, flat.offsets):
        mask[o:o + p.numel()] = False
    return mask


def _convert(osd, flat, optimizer):
    from bubbleformer_amd.utils.checkpoint import flat_state_from_torch_optim
    return flat_state_from_torch_optim(osd, [p.shape for p in flat.params], flat.offsets, flat.numel, optimizer)


@pytest.mark.parametrize("name", ["adamw", "adam"])
def test_torch_optim_state_round_trips_bit_exact(name):
    spec = _fixture(name)["spec"]
    flat = _flat(_native_model(spec))
    cls = torch.optim.AdamW if name == "adamw" else torch.optim.Adam
    opt = _stepped_torch_optimizer(flat.params, cls, lr=1e-3, betas=(0.8, 0.95), eps=1e-7, weight_decay=3e-3)
    got = _convert(opt.state_dict(), flat, name)
    pad = _padding_mask(flat)
    assert pad.any()
    for t in (got["m"], got["v"]):
        assert t.shape == (flat.numel,) and t.dtype == torch.float32
        assert torch.equal(t[pad], torch.zeros(int(pad.sum())))
    for i, (p, o) in enumerate(zip(flat.params, flat.offsets)):
        st = opt.state[opt.param_groups[0]["params"][i]]
        assert torch.equal(got["m"][o:o + p.numel()].view(p.shape), st["exp_avg"]), i
        assert torch.equal(got["v"][o:o + p.numel()].view(p.shape), st["exp_avg_sq"]), i
    assert got["step"] == 3
    assert got["betas"] == (0.8, 0.95) and got["eps"] == pytest.approx(1e-7, rel=0) and got["weight_decay"] == pytest.approx(3e-3, rel=0)
    assert got["lr"] == pytest.approx(1e-3, rel=0)


def _lion_state(flat, seed=5):
    g = torch.Generator().manual_seed(seed)
    return {"state": {i: {"exp_avg": torch.randn(p.shape, generator=g)} for i, p in enumerate(flat.params)},
            "param_groups": [{"lr": 5e-5, "betas": (0.9, 0.99), "weight_decay": 0.1, "use_triton": False,
                              "params": list(range(len(flat.params)))}]}


def test_lion_state_converts_to_m_only():
    spec = _fixture("adamw")["spec"]
    flat = _flat(_native_model(spec))
    osd = _lion_state(flat)
    got = _convert(osd, flat, "lion")
    assert got["v"] is None and got["step"] is None and got["eps"] is None
    assert got["betas"] == (0.9, 0.99) and got["weight_decay"] == pytest.approx(0.1, rel=0)
    assert torch.equal(got["m"][_padding_mask(flat)], torch.zeros(int(_padding_mask(flat).sum())))
    for i, (p, o) in enumerate(zip(flat.params, flat.offsets)):
        assert torch.equal(got["m"][o:o + p.numel()].view(p.shape), osd["state"][i]["exp_avg"]), i


def _adamw_state(flat):
    return _stepped_torch_optimizer(flat.params, torch.optim.AdamW, steps=2, lr=1e-3).state_dict()


def test_conversion_refusals():
    spec = _fixture("adamw")["spec"]
    flat = _flat(_native_model(spec))
    n = len(flat.params)
    shapes, offs = [p.shape for p in flat.params], flat.offsets
    from bubbleformer_amd.utils.checkpoint import flat_state_from_torch_optim as conv

    osd = _adamw_state(flat)                                     # count mismatch
    with pytest.raises(ValueError, match=f"holds {n} parameters, the model has {n - 1}"):
        conv(osd, shapes[:-1], offs[:-1], flat.numel, "adamw")

    bad = 5                                                      # shape mismatch names the first bad index
    assert shapes[bad] != shapes[bad + 1]
    with pytest.raises(ValueError, match=f"state {bad} has shape"):
        conv(osd, shapes[:bad] + [shapes[bad + 1]] + shapes[bad + 1:], offs, flat.numel, "adamw")

    osd = _adamw_state(flat)                                     # a parameter without state
    del osd["state"][7]
    with pytest.raises(ValueError, match="no state for parameter 7"):
        conv(osd, shapes, offs, flat.numel, "adamw")

    osd = _adamw_state(flat)                                     # unequal steps
    osd["state"][4]["step"] = torch.tensor(1.0)
    with pytest.raises(ValueError, match="state 4 has step 1"):
        conv(osd, shapes, offs, flat.numel, "adamw")

    p = [torch.nn.Parameter(q.detach().clone()) for q in flat.params]   # amsgrad
    opt = torch.optim.Adam(p, amsgrad=True)
    for q in p:
        q.grad = torch.ones_like(q)
    opt.step()
    with pytest.raises(ValueError, match="amsgrad"):
        conv(opt.state_dict(), shapes, offs, flat.numel, "adam")

    with pytest.raises(ValueError, match="Lion optimizer state, the training step uses 'adamw'"):
        conv(_lion_state(flat), shapes, offs, flat.numel, "adamw")
    with pytest.raises(ValueError, match="Adam / AdamW optimizer state, the training step uses 'lion'"):
        conv(_adamw_state(flat), shapes, offs, flat.numel, "lion")
    with pytest.raises(ValueError, match="torch.optim.AdamW state, the training step uses 'adam'"):
        conv(_adamw_state(flat), shapes, offs, flat.numel, "adam")

    osd = _adamw_state(flat)                                     # two parameter groups
    g0 = dict(osd["param_groups"][0])
    osd["param_groups"] = [dict(g0, params=list(range(3))), dict(g0, params=list(range(3, n)))]
    with pytest.raises(ValueError, match="2 parameter groups"):
        conv(osd, shapes, offs, flat.numel, "adamw")


def test_adam_optimizer_is_accepted():
    """TrainStep(optimizer="adam") (config/optim_cfg/adam.yaml) builds its moment buffers and Adam's default betas."""
    from bubbleformer_amd.trainer import TrainStep
    step = TrainStep(_native_model(_fixture("adam")["spec"]), lr=2.5e-4, weight_decay=1e-5, optimizer="adam")
    assert step.optimizer == "adam" and step.betas == (0.9, 0.999)
    assert step.v is not None and step.v.shape == step.m.shape == step.flat.flat.shape


def _trainstep(spec, name, device="cpu"):
    """A TrainStep whose hyperparameters and schedule all differ from the fixture's, so the import must set every one of them."""
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.lr_schedulers import CosineWarmupLR
    model = _native_model(spec, device)
    sched = CosineWarmupLR(7.0, 100, 1000, 0.5)
    return model, TrainStep(model, lr=7.0, weight_decay=0.5, betas=(0.5, 0.5), eps=0.25, optimizer=name, scheduler=sched)


@pytest.mark.parametrize("name", ["adamw", "adam"])
def test_reference_checkpoint_loads_into_train_step(name, tmp_path):
    """The real reference checkpoint: parameter order, weights, moments, step, hyperparameters and the schedule position."""
    from bubbleformer_amd.utils.checkpoint import load_checkpoint
    fx = _fixture(name)
    ck, spec = fx["checkpoint"], fx["spec"]
    path = str(tmp_path / "hpc_ckpt_1.ckpt")
    torch.save(ck, path)
    model, step = _trainstep(spec, name)
    assert [k for k, _ in model.named_parameters()] == fx["param_names"]      # native registration order = the reference optimizer's
    load_checkpoint(path, model, step)
    for k, p in model.named_parameters():
        assert torch.equal(p.detach(), ck["state_dict"]["model." + k]), k
    osd = ck["optimizer_states"][0]
    for i, (p, o) in enumerate(zip(step.flat.params, step.flat.offsets)):
        assert torch.equal(step.m[o:o + p.numel()].view(p.shape), osd["state"][i]["exp_avg"]), i
        assert torch.equal(step.v[o:o + p.numel()].view(p.shape), osd["state"][i]["exp_avg_sq"]), i
    pad = _padding_mask(step.flat)
    assert not step.m[pad].any() and not step.v[pad].any()
    pg = osd["param_groups"][0]
    assert step.step_no == 3 and step.betas == tuple(pg["betas"]) and step.eps == pg["eps"] and step.wd == pg["weight_decay"]
    s = step.scheduler
    assert (s.base_lr, s.warmup_iters, s.max_iters, s.eta_min, s.last_epoch) == (
        spec["optim"]["lr"], spec["warmup_iters"], spec["max_iters"], spec["eta_min"], 3)
    got = []
    for _ in fx["lrs"]:
        got.append(s.get_last_lr()[0])
        s.step()
    # the native schedule is closed-form, the reference's CosineAnnealingLR recursive: equal up to double rounding
    np.testing.assert_allclose(got, fx["lrs"], rtol=1e-12, atol=0)
    assert got[0] == pytest.approx(float(pg["lr"]), rel=1e-12)


def test_reference_checkpoint_refusals(tmp_path):
    from bubbleformer_amd.utils.checkpoint import load_checkpoint
    fx = _fixture("adamw")
    ck, spec = fx["checkpoint"], fx["spec"]

    def load(c, name):
        path = str(tmp_path / "c.ckpt")
        torch.save(c, path)
        model, step = _trainstep(spec, name)
        before = {k: v.clone() for k, v in model.state_dict().items()}
        with pytest.raises(ValueError) as e:
            load_checkpoint(path, model, step)
        assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())     # refused before any weight is written
        assert step.step_no == 0 and not step.m.any()
        return str(e.value)

    assert "optim_cfg 'adamw', the training step uses 'adam'" in load(dict(ck, hyper_parameters={"optim_cfg": {"name": "adamw"}}), "adam")
    assert "AdamW state, the training step uses 'adam'" in load(dict(ck, hyper_parameters={}), "adam")
    assert "Adam / AdamW optimizer state, the training step uses 'lion'" in load(dict(ck, hyper_parameters={}), "lion")
    bad = dict(ck, lr_schedulers=[{"last_epoch": 3}])
    assert "not the state of the reference's CosineWarmupLR" in load(bad, "adamw")


def test_native_checkpoint_loads_as_before(tmp_path):
    """A file in the native flat layout (save_checkpoint) still loads through the native path, Adam included."""
    from bubbleformer_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    spec = _fixture("adam")["spec"]
    model, step = _trainstep(spec, "adam")
    step.m.normal_()
    step.v.uniform_()
    step.step_no = 11
    step.scheduler.step()
    path = str(tmp_path / "native.ckpt")
    save_checkpoint(path, model, train_step=step, epoch=2)
    model2, step2 = _trainstep(spec, "adam")
    ck = load_checkpoint(path, model2, step2)
    assert ck["optimizer_states"][0]["name"] == "adam"
    assert step2.step_no == 11 and torch.equal(step2.m, step.m) and torch.equal(step2.v, step.v)
    assert step2.scheduler.last_epoch == step.scheduler.last_epoch and step2.betas == (0.5, 0.5)


def _flat_params(model):
    return {k: p.detach().double().cpu() for k, p in model.named_parameters()}


def _displacement_error(got, ref, start):
    """||(got - start) - (ref - start)|| / ||ref - start|| over the parameters whose gradient is not structurally zero."""
    keys = [k for k in ref if not structurally_zero(k)]
    d_ref = torch.cat([(ref[k].double() - start[k].double()).flatten() for k in keys])
    d_got = torch.cat([(got[k] - start[k].double()).flatten() for k in keys])
    return float((d_got - d_ref).norm() / d_ref.norm())


# The continued native run in fp32 against the reference's own continuation (fp32 on the CPU), measured as the relative L2 error of the
# two steps' parameter displacement over the parameters whose gradient is not structurally zero.  Measured on one MI355X: 3.2e-4 (AdamW)
# and 4.0e-5 (Adam); the weights-only control misses by 0.84 for both, more than 400x the bound.
RESUME_TOL = 2e-3


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["adamw", "adam"])
def test_resumed_reference_run_matches_the_reference_continuation(name, tmp_path):
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.checkpoint import load_checkpoint
    from bubbleformer_amd.utils.lr_schedulers import CosineWarmupLR
    fx = _fixture(name)
    ck, spec = fx["checkpoint"], fx["spec"]
    path = str(tmp_path / "hpc_ckpt_1.ckpt")
    torch.save(ck, path)
    start = {k[len("model."):]: v for k, v in ck["state_dict"].items()}

    def run(model, step):
        lrs = []
        for b in fx["batches"]:
            lrs.append(step.scheduler.get_last_lr()[0])
            step(b["x"].cuda(), b["cond"].cuda(), b["y"].cuda())
        lrs.append(step.scheduler.get_last_lr()[0])
        torch.cuda.synchronize()
        return lrs, _flat_params(model)

    model, step = _trainstep(spec, name, "cuda")
    load_checkpoint(path, model, step)
    lrs, got = run(model, step)
    np.testing.assert_allclose(lrs, fx["lrs"], rtol=1e-12, atol=0)
    err = _displacement_error(got, fx["params_after"], start)

    # control: the same weights with fresh moments and a fresh warm-up (what a weights-only resume gives)
    model_c = _native_model(spec, "cuda")
    load_checkpoint(path, model_c)
    sched = CosineWarmupLR(spec["optim"]["lr"], spec["warmup_iters"], spec["max_iters"], spec["eta_min"])
    _, got_c = run(model_c, TrainStep(model_c, lr=spec["optim"]["lr"], weight_decay=spec["optim"]["weight_decay"], optimizer=name,
                                      scheduler=sched))
    err_c = _displacement_error(got_c, fx["params_after"], start)
    print(f"{name}: resumed displacement error {err:.3e}, weights-only control {err_c:.3e}")
    assert err < RESUME_TOL, err
    assert err_c > 10 * RESUME_TOL, err_c
