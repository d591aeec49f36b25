"""GPU: parameter groups in the fused optimizers (csrc/optim_kernels.h GRP = true: bf_adamw / bf_adam / bf_lion with chunk_group;
csrc/gradclip.hip: bf_group_sumsq, bf_group_clip_coef) against torch optimizers built with one torch param group per live group, and
TrainStep(param_groups=...) / fit(param_groups=...) on the tiny FiLMAViT in fp32."""
import os
import shutil

import numpy as np
import pytest
import torch

from tests.helpers import load_variant, rel_l2

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
CHUNK = 64
# 64*5 + 3: the scalar tail sits in a partial last chunk; 64*7: no tail; 4096*256*4 + 64*3: one grid-stride wrap past opt_grid_for's cap
SIZES = [64 * 5 + 3, 64 * 7, 4096 * 256 * 4 + 64 * 3]
MODES = ["host", "dev", "clamp"]
# G = 4, chunk c belongs to group c % 4, so neighbouring chunks always differ: (lr_scale, weight_decay, frozen)
TABLE = [(1.0, 0.1, False), (0.25, 0.0, False), (0.5, 0.3, True), (0.0, 0.05, False)]      # group 2 frozen; group 3 is torch's lr = 0
FROZEN_K = 2
LR, GSCALE, COEF, CLIP = 1e-3, 0.25, 0.5, 0.03125


def _groups(n, table=TABLE, device="cuda"):
    from bubbleformer_amd import ops
    chunks = (n + CHUNK - 1) // CHUNK
    cmap = (torch.arange(chunks) % len(table)).to(torch.uint8)
    return ops.param_group_tables(cmap, [t[0] for t in table], [t[1] for t in table], [t[2] for t in table], n, device), cmap


def _element_group(cmap, n):
    return cmap.repeat_interleave(CHUNK)[:n].cuda()


def _mode_kw(mode):
    """(keyword arguments of the ops call, gradient -> the gradient the optimizer rule sees)"""
    if mode == "host":
        return {}, lambda g: g * GSCALE
    coef = torch.tensor([COEF], device="cuda")
    if mode == "dev":
        return {"coef": coef}, lambda g: g * (GSCALE * COEF)
    return {"coef": coef, "clip_value": CLIP}, lambda g: (g * (GSCALE * COEF)).clamp(-CLIP, CLIP)


def _call(name, bufs, step, lr, wd, betas, **kw):
    from bubbleformer_amd import ops
    p, g, m, v = bufs
    if name == "lion":
        ops.lion_(p, g, m, lr, betas, wd, GSCALE, **kw)
    else:
        getattr(ops, name + "_")(p, g, m, v, step, lr, betas, 1e-8, wd, GSCALE, **kw)


def _unpadded(n, src=None):
    """An allocation of its own of exactly n floats (16-byte aligned by the allocator), not a view into a larger one."""
    t = torch.zeros(n, device="cuda")
    if src is not None:
        t.copy_(src)
    assert t.numel() == n and t.data_ptr() % 16 == 0 and t.untyped_storage().nbytes() == 4 * n
    return t


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("with_avg", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["adamw", "adam", "lion"])
def test_grouped_optimizers_match_torch_param_groups(name, mode, with_avg, n):
    """Five steps.  AdamW / Adam: torch.optim.AdamW / Adam (fp64 parameters) with one torch param group per live group -- lr * scale, the
    group's decay -- and the frozen elements not handed to torch at all.  Lion: the rule of optim_kernels.h's comment,
    p *= 1 - lr*wd; p -= lr * sign(b1*m + (1-b1)*g); m = b2*m + (1-b2)*g, restated in fp64 per group; its gradients lie on a dyadic lattice
    and its betas are (0.5, 0.75), so that the argument of sign() is exact in fp32 and in fp64 alike (no element's sign is decided by a
    rounding: over 4 M elements and 5 steps some would be with random inputs, and one flipped sign is 2 lr on that element).
    Bounds: test_gpu_adam.py's, per group -- relative L2 < 1e-6 on p and m, 2e-5 on v.  The frozen group's p, m, v and avg are torch.equal
    to their initial values, also with NaN in its gradient (last step), and every live group stays finite."""
    from bubbleformer_amd import ops  # noqa: F401
    gen = torch.Generator(device="cuda").manual_seed(n % 997 + len(name))
    groups, cmap = _groups(n)
    eg = _element_group(cmap, n)
    idx = [torch.nonzero(eg == k).flatten() for k in range(len(TABLE))]
    betas = (0.5, 0.75) if name == "lion" else (0.9, 0.999)
    p0 = torch.randn(n, device="cuda", generator=gen)
    m0 = torch.zeros(n, device="cuda")
    v0 = torch.zeros(n, device="cuda")
    m0[idx[FROZEN_K]] = 0.125            # a frozen group's state is whatever it was: it must keep these bits
    v0[idx[FROZEN_K]] = 0.25
    a0 = p0 * 0.5
    p, m, v, a, gb = (_unpadded(n, t) for t in (p0, m0, v0, a0, None))
    w = 0.25
    kw, seen = _mode_kw(mode)
    if with_avg:
        kw = dict(kw, avg=a, avg_weight=w)
    live = [k for k, t in enumerate(TABLE) if not t[2]]
    ref = {k: torch.nn.Parameter(p0[idx[k]].double()) for k in live}
    m_ref = {k: torch.zeros(idx[k].numel(), device="cuda", dtype=torch.float64) for k in live}
    a_ref = {k: a0[idx[k]].double() for k in live}
    opt = None
    if name != "lion":
        cls = torch.optim.AdamW if name == "adamw" else torch.optim.Adam
        opt = cls([{"params": [ref[k]], "lr": LR * TABLE[k][0], "weight_decay": TABLE[k][1]} for k in live], lr=LR, betas=betas, eps=1e-8)
    for step in range(1, 6):
        if name == "lion":
            grad = torch.randint(-512, 513, (n,), device="cuda", generator=gen).float() / 1024.0
        else:
            grad = torch.randn(n, device="cuda", generator=gen)
        if step == 5:
            grad[idx[FROZEN_K]] = float("nan")
        gb.copy_(grad)
        for k in live:
            ref[k].grad = seen(grad[idx[k]].double())
        if opt is not None:
            opt.step()
        else:
            with torch.no_grad():
                for k in live:
                    lr_k, wd_k = LR * TABLE[k][0], TABLE[k][1]
                    ref[k].mul_(1 - lr_k * wd_k).sub_(lr_k * torch.sign(betas[0] * m_ref[k] + (1 - betas[0]) * ref[k].grad))
                    m_ref[k].mul_(betas[1]).add_((1 - betas[1]) * ref[k].grad)
        for k in live:
            a_ref[k] = a_ref[k] + w * (ref[k].detach() - a_ref[k])
        _call(name, (p, gb, m, v), step, LR, 123.0, betas, groups=groups, **kw)      # the call's own weight decay is ignored
        for k in live:
            err = rel_l2(p[idx[k]].cpu(), ref[k].detach().cpu())
            assert err < 1e-6, (step, k, err)
    for k in live:
        want_m = m_ref[k] if opt is None else opt.state[ref[k]]["exp_avg"]
        errs = {"m": rel_l2(m[idx[k]].cpu(), want_m.cpu())}
        if opt is not None:
            errs["v"] = rel_l2(v[idx[k]].cpu(), opt.state[ref[k]]["exp_avg_sq"].cpu())
        if with_avg:
            errs["avg"] = rel_l2(a[idx[k]].cpu(), a_ref[k].cpu())
        print(f"{name} {mode} avg={with_avg} n={n} group {k}: {errs}")
        assert errs["m"] < 1e-6 and errs.get("v", 0.0) < 2e-5 and errs.get("avg", 0.0) < 1e-6, (k, errs)
        assert all(torch.isfinite(t[idx[k]]).all() for t in (p, m, v, a))
    zero_lr = idx[3]
    assert torch.equal(p[zero_lr], p0[zero_lr]) and m[zero_lr].abs().sum() > 0      # lr_scale 0, not frozen: the moments move, p does not
    fz = idx[FROZEN_K]
    for got, init in ((p, p0), (m, m0), (v, v0), (a, a0)):
        assert torch.equal(got[fz], init[fz])
    if not with_avg:
        assert torch.equal(a, a0)
    if name == "lion":
        assert torch.equal(v, v0)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["adamw", "adam", "lion"])
def test_one_default_group_is_the_ungrouped_entry_point_bit_for_bit(name, mode, n):
    """One group (scale 1, the call's weight decay, not frozen): every buffer comes out torch.equal to the ungrouped entry point's over
    three steps; and with avg, p and the moments are the bits of the grouped call without it."""
    gen = torch.Generator(device="cuda").manual_seed(7 + n % 13)
    wd = 0.1
    groups, _ = _groups(n, [(1.0, wd, False)])
    betas = (0.9, 0.99) if name == "lion" else (0.9, 0.999)
    p0 = torch.randn(n, device="cuda", generator=gen)
    kw, _ = _mode_kw(mode)
    runs = {}
    for tag in ("plain", "grouped", "grouped_avg", "plain_avg"):
        runs[tag] = [_unpadded(n, p0), _unpadded(n), _unpadded(n), _unpadded(n), _unpadded(n, p0)]      # p, g, m, v, avg
    for step in range(1, 4):
        grad = torch.randn(n, device="cuda", generator=gen)
        for tag, (p, g, m, v, a) in runs.items():
            g.copy_(grad)
            extra = dict(kw)
            if tag.startswith("grouped"):
                extra["groups"] = groups
            if tag.endswith("avg"):
                extra.update(avg=a, avg_weight=0.1)
            _call(name, (p, g, m, v), step, LR, wd if not tag.startswith("grouped") else 0.0, betas, **extra)
    for i, what in enumerate(("p", "g", "m", "v")):
        assert torch.equal(runs["grouped"][i], runs["plain"][i]), what
        assert torch.equal(runs["grouped_avg"][i], runs["grouped"][i]), what
    assert torch.equal(runs["grouped_avg"][4], runs["plain_avg"][4]) and not torch.equal(runs["grouped_avg"][4], p0)
    assert torch.equal(runs["grouped"][4], p0)


def _spread(n, seed):
    """Magnitudes log-uniform over 1e-8 .. 1e3, random signs (test_gpu_grad_clip.py's gradient)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, device="cuda", generator=g, dtype=torch.float64) * 11.0 - 8.0)
    sign = torch.where(torch.rand(n, device="cuda", generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign).float()


@pytest.mark.parametrize("n", SIZES)
def test_group_sumsq_and_clip_coefficient(n):
    """Four groups.  sums[k] against numpy's fp64 sum of the squares of group k's elements: both add at most n_k fp64 terms, each sum is
    within n_k * 2^-53 relative of the exact one, so they agree within 2 * n_k * 2^-53.  Norm (over the three live groups; the frozen one is
    left out) and coefficient from group_clip_coef_ within one fp32 ulp, the bound of test_grad_norm_matches_fp64_within_one_ulp; the
    per-group norms likewise; two calls give equal bits; an infinite element in a live group gives coefficient 0, a NaN in the frozen
    group nothing."""
    from bubbleformer_amd import ops
    groups, cmap = _groups(n)
    x = _unpadded(n, _spread(n, seed=n % 1000))
    eg = cmap.repeat_interleave(CHUNK)[:n].numpy()
    xs = x.cpu().numpy().astype(np.float64)
    want = np.array([np.sum(xs[eg == k] ** 2) for k in range(4)])
    sums = ops.group_sumsq(x, groups)
    again = ops.group_sumsq(x, groups, ws=ops.group_sumsq_workspace(n, x.device))
    torch.cuda.synchronize()
    got = sums.cpu().numpy()
    assert sums.dtype == torch.float64 and sums.shape == (4,) and torch.equal(sums, again)
    for k in range(4):
        bound = 2.0 * max(int((eg == k).sum()), 1) * 2.0 ** -53
        print(f"n {n} group {k}: {got[k]:.17g} (numpy {want[k]:.17g}, rel {abs(got[k] - want[k]) / want[k]:.3g}, bound {bound:.3g})")
        assert abs(got[k] - want[k]) <= bound * want[k]
    gscale = 0.125
    live = [k for k in range(4) if not TABLE[k][2]]
    norm64 = gscale * float(np.sqrt(want[live].sum()))
    assert norm64 < gscale * float(np.sqrt(want.sum()))           # the frozen group is left out
    for max_norm, clipped in ((4.0 * norm64, False), (0.37 * norm64, True)):
        out, out2, gn = torch.zeros(2, device="cuda"), torch.full((2,), -1.0, device="cuda"), torch.zeros(4, device="cuda")
        ops.group_clip_coef_(sums, groups, out, max_norm, gscale, gn)
        ops.group_clip_coef_(again, groups, out2, max_norm, gscale)
        norm, coef = float(out[0]), float(out[1])
        assert torch.equal(out, out2)
        assert abs(norm - norm64) <= ULP * norm64
        ref = torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (out[0].cpu() + torch.tensor(1e-6, dtype=torch.float32)), max=1.0)
        assert abs(coef - float(ref)) <= ULP * float(ref)
        assert (coef == 1.0) == (not clipped) and (not clipped or abs(coef - 0.37) < 1e-5)
        for k in range(4):
            assert abs(float(gn[k]) - gscale * np.sqrt(want[k])) <= ULP * gscale * np.sqrt(want[k])
    out = torch.zeros(2, device="cuda")
    fz = int(np.nonzero(eg == FROZEN_K)[0][0])
    x[fz] = float("nan")
    ops.group_clip_coef_(ops.group_sumsq(x, groups), groups, out, 1.0, gscale)
    assert abs(float(out[0]) - norm64) <= ULP * norm64           # a NaN in the frozen group reaches nothing
    x[int(np.nonzero(eg == 1)[0][-1])] = float("inf")
    ops.group_clip_coef_(ops.group_sumsq(x, groups), groups, out, 1.0, gscale)
    assert float(out[0]) == float("inf") and float(out[1]) == 0.0


def test_refusals():
    """At the ops level: null tables, n_groups 0 and 65, a chunk map of the wrong length (for the tables' constructor and for a call on a
    buffer of another length), an id past the tables."""
    from bubbleformer_amd import _lib, ops
    E = _lib.BubbleformerHipError
    n = 64 * 7
    cmap = torch.zeros(7, dtype=torch.uint8)
    ok = ops.param_group_tables(cmap, [1.0], [0.0], [False], n, "cuda")
    bufs = [torch.zeros(n, device="cuda") for _ in range(4)]
    for bad in (dict(lr_scale=None), dict(weight_decay=None), dict(frozen=None)):
        with pytest.raises(E):
            ops.param_group_tables(cmap, **{**dict(lr_scale=[1.0], weight_decay=[0.0], frozen=[False]), **bad}, numel=n, device="cuda")
    with pytest.raises(E):
        ops.param_group_tables(None, [1.0], [0.0], [False], n, "cuda")
    for G in (0, 65):
        with pytest.raises(E):
            ops.param_group_tables(cmap, [1.0] * G, [0.0] * G, [False] * G, n, "cuda")
    for wrong in (torch.zeros(6, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8), torch.zeros(7, dtype=torch.int32)):
        with pytest.raises(E):
            ops.param_group_tables(wrong, [1.0], [0.0], [False], n, "cuda")
    with pytest.raises(E):
        ops.param_group_tables(torch.ones(7, dtype=torch.uint8), [1.0], [0.0], [False], n, "cuda")      # names group 1 of 1
    with pytest.raises(E):
        ops.param_group_tables(cmap, [-1.0], [0.0], [False], n, "cuda")
    # the entry points' own checks, through ops: a record whose tables are missing or whose count is out of range
    for field, value in (("lr_scale", None), ("weight_decay", None), ("frozen", None), ("n_groups", 0), ("n_groups", 65)):
        forged = ops.ParamGroupTables(ok.chunk, ok.lr_scale, ok.weight_decay, ok.frozen, ok.n_groups, ok.numel)
        setattr(forged, field, value)
        before = [b.clone() for b in bufs]
        with pytest.raises(E):
            ops.lion_(bufs[0], bufs[1], bufs[2], 1e-3, groups=forged)
        with pytest.raises(E):
            ops.adamw_(*bufs, 1, 1e-3, groups=forged)
        with pytest.raises(E):
            ops.adam_(*bufs, 1, 1e-3, groups=forged)
        assert all(torch.equal(a, b) for a, b in zip(bufs, before))
    short = [torch.zeros(n - 64, device="cuda") for _ in range(4)]
    with pytest.raises(E):
        ops.adamw_(*short, 1, 1e-3, groups=ok)                   # the map is 7 chunks long, the buffer 6
    with pytest.raises(E):
        ops.group_sumsq(short[0], ok)
    with pytest.raises(E):
        ops.lion_(bufs[0], bufs[1], bufs[2], 1e-3, groups="no_weight_decay")
    sums = ops.group_sumsq(bufs[0], ok)
    for bad in (0.0, -1.0):
        with pytest.raises(E):
            ops.group_clip_coef_(sums, ok, torch.zeros(2, device="cuda"), bad)
    forged = ops.ParamGroupTables(ok.chunk, ok.lr_scale, ok.weight_decay, None, 1, n)
    with pytest.raises(E):
        ops.group_clip_coef_(sums, forged, torch.zeros(2, device="cuda"), 1.0)


# ------------------------------------------------------------------------------------------------ TrainStep on the tiny FiLMAViT, fp32
def _tiny(B=2):
    from bubbleformer_amd.models import get_model
    from oracle import weights as W
    spec, _ = load_variant("tiny_d64")
    cfg = dict(spec["cfg"])
    model = get_model("filmavit", time_window=spec["T"], drop_path=0.0, compute_dtype=torch.float32, **cfg)
    model.load_state_dict(W.generate(W.param_shapes(**cfg), seed=spec["seed"]))

    def data(i):
        return (W.synthetic_clip(B, spec["T"], cfg["input_fields"], spec["H"], spec["W"], 700 + i).cuda(),
                W.synthetic_fluid_params(B, cfg["num_fluid_params"], 900 + i).cuda(),
                W.synthetic_clip(B, spec["T"], cfg["output_fields"], spec["H"], spec["W"], 800 + i).cuda())
    return model.cuda().train(), data


TRUNK = r"^blocks\."


def test_lion_step_moves_every_group_by_its_own_learning_rate():
    """Lion, lr 1e-3, no weight decay, fresh state, one step: p moves by exactly lr * scale wherever the gradient is not zero.  Scales
    {1, 0.25, frozen}: every element of a group of scale s with a non-zero gradient has |p1 - p0| = fp32(lr) * s within one ulp of the
    parameter (the one rounding of the subtraction), every frozen parameter keeps its bits -- an ungrouped step moves them all by lr."""
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.param_groups import GroupSpec, freeze
    model, data = _tiny()
    lr = 1e-3
    step = TrainStep(model, lr=lr, weight_decay=0.0, optimizer="lion", param_groups=[GroupSpec(TRUNK, lr_scale=0.25)] + freeze(r"^(embed|debed)\."))
    res = step.resolved_groups
    assert sorted(res.table) == sorted([(1.0, 0.0, False), (0.25, 0.0, False), (0.0, 0.0, True)])
    p0 = step.flat.flat.clone()
    step(*data(0))
    torch.cuda.synchronize()
    checked = {1.0: 0, 0.25: 0}
    lr32 = float(torch.tensor(lr, dtype=torch.float32))
    for name, p in model.named_parameters():
        o = step.flat.offsets[[id(q) for q in step.flat.params].index(id(p))]
        before, grad = p0[o:o + p.numel()].view(p.shape), p.grad
        scale, _, frozen = res.params[name]
        if frozen:
            assert torch.equal(p.detach(), before), name
            assert name.startswith(("embed.", "debed.")) and grad.abs().sum() > 0      # its gradient was computed all the same
            continue
        moved = grad != 0
        delta = (p.detach().double() - before.double()).abs()
        big = torch.maximum(p.detach().abs(), before.abs())
        ulp = (torch.nextafter(big, torch.full_like(big, float("inf"))) - big).double()
        assert ((delta - lr32 * scale).abs() <= ulp)[moved].all(), name
        assert torch.equal(p.detach()[~moved], before[~moved]), name
        checked[scale] += int(moved.sum())
    assert checked[1.0] > 1000 and checked[0.25] > 100000, checked


def _run_adamw(param_groups, weight_decay, steps, shadow_decays=()):
    """`steps` TrainStep(adamw, lr 1e-3) steps -> (initial flat buffer, final flat buffer, step, {wd: flat buffer}).  Every shadow is a copy
    of the initial state stepped by the plain, ungrouped ops.adamw_ at its own weight decay on the gradient the step has just used."""
    from bubbleformer_amd import ops
    from bubbleformer_amd.trainer import TrainStep
    model, data = _tiny()
    step = TrainStep(model, lr=1e-3, weight_decay=weight_decay, optimizer="adamw", param_groups=param_groups)
    p0 = step.flat.flat.clone()
    shadows = {wd: [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)] for wd in shadow_decays}
    for i in range(steps):
        step(*data(i))
        for wd, (p, m, v) in shadows.items():
            ops.adamw_(p, step.flat.grad, m, v, step.step_no, 1e-3, step.betas, step.eps, wd, 1.0)
    torch.cuda.synchronize()
    return p0, step.flat.flat.clone(), step, {wd: t[0] for wd, t in shadows.items()}


def test_adamw_without_decay_on_the_vectors():
    """AdamW, weight_decay 0.5, param_groups=no_weight_decay(), four steps, against plain weight_decay 0.5 and plain weight_decay 0: the
    matrices and convolution kernels follow the decayed run (1e-6 relative L2), the vectors and bias tables the undecayed one (1e-6), and
    the vectors' displacement differs from the decayed run's by more than 1e-3 relative L2.
    Over four steps the plain runs are the ungrouped kernel stepping copies of the initial state on the grouped step's own gradients, not
    separate TrainSteps: from the second step on, three separate runs no longer see the same gradients, because the loss couples every
    matrix to the vectors that are decayed in one run and not in the other (measured on one MI355X with three separate runs of four steps:
    matrices 8.6e-5 from the decayed run, vectors 1.9e-3 from the undecayed one -- the runs, not the kernel).  Three separate TrainSteps
    are compared after ONE step, where all three have seen the same gradient, at the same bounds."""
    from bubbleformer_amd.utils.param_groups import no_weight_decay
    for steps, separate in ((4, False), (1, True)):
        p0, grouped, step, shadow = _run_adamw(no_weight_decay(), 0.5, steps, () if separate else (0.5, 0.0))
        if separate:
            decayed, free = _run_adamw(None, 0.5, steps)[1], _run_adamw(None, 0.0, steps)[1]
        else:
            decayed, free = shadow[0.5], shadow[0.0]
        res = step.resolved_groups
        assert res.table == [(1.0, 0.5, False), (1.0, 0.0, False)]
        name_of = {id(p): n for n, p in step.model.named_parameters()}
        n_vec, worst, vec = 0, {"matrix": 0.0, "vector": 0.0}, []
        for p, o in zip(step.flat.params, step.flat.offsets):
            name, sl = name_of[id(p)], slice(o, o + p.numel())
            if res.params[name][1] == 0.5:
                assert p.dim() >= 2, name
                worst["matrix"] = max(worst["matrix"], rel_l2(grouped[sl].cpu(), decayed[sl].cpu()))
            else:
                n_vec += 1
                worst["vector"] = max(worst["vector"], rel_l2(grouped[sl].cpu(), free[sl].cpu()))
                vec.append(torch.arange(o, o + p.numel(), device="cuda"))
        vec = torch.cat(vec)                   # the vectors' displacement as one vector: a bias that starts at zero has nothing to decay yet
        worst["apart"] = rel_l2((grouped[vec] - p0[vec]).cpu(), (decayed[vec] - p0[vec]).cpu())
        print("no_weight_decay, %d step(s), %s: worst relative L2 -- matrices vs decayed %.3g, vectors vs undecayed %.3g; the vectors' displacement "
              "against the decayed run's %.3g" % (steps, "separate runs" if separate else "shared gradients", worst["matrix"], worst["vector"],
                                                  worst["apart"]))
        assert n_vec > 50 and worst["matrix"] < 1e-6 and worst["vector"] < 1e-6 and worst["apart"] > 1e-3, (steps, worst)


def test_norm_clipping_with_the_trunk_frozen_takes_the_live_norm():
    """grad_norm[0] is the fp64 norm of the live parameters' .grad within one fp32 ulp, and smaller than the whole buffer's; group_grad_norm
    holds both groups' norms; the coefficient clips by the live norm."""
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.param_groups import freeze, group_norms
    model, data = _tiny()
    step = TrainStep(model, lr=1e-3, weight_decay=0.0, optimizer="adamw", gradient_clip_val=1e-3, param_groups=freeze(TRUNK))
    step(*data(0))
    torch.cuda.synchronize()
    live = sum(float(p.grad.double().pow(2).sum()) for n, p in model.named_parameters() if not n.startswith("blocks."))
    trunk = sum(float(p.grad.double().pow(2).sum()) for n, p in model.named_parameters() if n.startswith("blocks."))
    norm, coef = float(step.grad_norm[0]), float(step.grad_norm[1])
    print(f"live norm {live ** 0.5:.9g}, whole buffer {(live + trunk) ** 0.5:.9g}, grad_norm {norm:.9g}, coef {coef:.6g}")
    assert abs(norm - live ** 0.5) <= ULP * live ** 0.5
    assert norm < (live + trunk) ** 0.5 and trunk > 0
    assert abs(coef - 1e-3 / (norm + 1e-6)) <= 2 * ULP * coef
    names = step.resolved_groups.names
    assert names == ["default", "frozen"] and step.group_grad_norm.shape == (2,)
    assert abs(float(step.group_grad_norm[0]) - live ** 0.5) <= ULP * live ** 0.5
    assert abs(float(step.group_grad_norm[1]) - trunk ** 0.5) <= ULP * trunk ** 0.5
    norms = group_norms(step)
    assert set(norms) == set(names) and abs(norms["frozen"][1] - trunk ** 0.5) <= 1e-6 * trunk ** 0.5
    want_p = sum(float(p.detach().double().pow(2).sum()) for n, p in model.named_parameters() if n.startswith("blocks.")) ** 0.5
    assert abs(norms["frozen"][0] - want_p) <= 1e-6 * want_p


def test_average_of_a_frozen_group_stays_the_parameter():
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.averaging import AverageSpec
    from bubbleformer_amd.utils.param_groups import freeze
    model, data = _tiny()
    step = TrainStep(model, lr=1e-3, weight_decay=0.1, optimizer="adamw", weight_average=AverageSpec("ema", decay=0.9),
                     param_groups=freeze(TRUNK))
    p0 = step.flat.flat.clone()
    for i in range(3):
        step(*data(i))
    torch.cuda.synchronize()
    assert step.n_averaged == 3
    at = {id(p): o for p, o in zip(step.flat.params, step.flat.offsets)}
    for name, p in model.named_parameters():
        o = at[id(p)]
        avg = step.avg[o:o + p.numel()].view(p.shape)
        if name.startswith("blocks."):
            assert torch.equal(avg, p.detach()) and torch.equal(p.detach(), p0[o:o + p.numel()].view(p.shape)), name
        elif p.grad.abs().sum() > 0:
            assert not torch.equal(avg, p.detach()), name
    assert not step.m[step.groups.chunk.repeat_interleave(CHUNK) == 1].any()      # the frozen trunk's moments were never written


def test_param_groups_none_is_the_step_without_the_argument():
    from bubbleformer_amd.trainer import TrainStep
    out = []
    for kw in ({}, {"param_groups": None}):
        model, data = _tiny()
        step = TrainStep(model, lr=1e-3, weight_decay=0.1, optimizer="adamw", gradient_clip_val=0.05, **kw)
        assert step.groups is None and step.resolved_groups is None and step.group_grad_norm is None
        for i in range(3):
            step(*data(i))
        torch.cuda.synchronize()
        out.append(step.flat.flat.clone())
    assert torch.equal(out[0], out[1])


def test_fit_with_param_groups_records_group_norms_and_resumes(tmp_path):
    """fit on the two golden samples, time_window 4, batch 2, 3 batches x 2 epochs, param_groups + clipping by norm + a checkpoint:
    hist["group_grad_norm"] has one row per optimizer step and G columns, the file holds "param_groups", a run resumed from the epoch-0
    file repeats epoch 1 (rtol 1e-4, as test_fit_with_accumulation_and_clipping_steps_six_times_and_resumes), and resuming into another
    partition is a ValueError that leaves the model's weights untouched."""
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.fit import fit
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils.param_groups import freeze, layer_decay, no_weight_decay
    samples = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samples")

    def make():
        torch.manual_seed(0)
        return get_model("avit", input_fields=4, output_fields=4, time_window=4, patch_size=8, embed_dim=64, num_heads=2, processor_blocks=2,
                         drop_path=0.0, compute_dtype=torch.float32).cuda()
    tr = BubbleForecast([os.path.join(samples, "sample_1.hdf5"), os.path.join(samples, "sample_2.hdf5")], norm="std", time_window=4, start_time=5)
    tr.normalize()
    specs = no_weight_decay() + layer_decay(make(), 0.75) + freeze(r"^blocks\.0\.")
    kw = dict(batch_size=2, max_epochs=2, optimizer="adamw", lr=2e-3, weight_decay=1e-2, warmup_iters=2, eta_min=1e-6, limit_train_batches=3,
              seed=42, gradient_clip_val=0.05)
    ck, ck0 = str(tmp_path / "last.ckpt"), str(tmp_path / "after_epoch0.ckpt")
    events = []

    def log(e):
        events.append(e)
        if e.get("epoch") == 1 and e.get("batch_idx") == 0:
            shutil.copy(ck, ck0)
    model = make()
    frozen0 = {k: v.detach().clone() for k, v in model.named_parameters() if k.startswith("blocks.0.")}
    h = fit(model, tr, None, checkpoint_path=ck, log=log, param_groups=specs, **kw)
    saved = torch.load(ck, weights_only=False)
    G = len(saved["param_groups"])
    rows = np.array(h["group_grad_norm"])
    assert rows.shape == (6, G) and G >= 5 and len(h["grad_norm"]) == 6 and np.isfinite(rows).all() and np.isfinite(h["train_loss"]).all()
    part = saved["param_groups"]
    assert all(set(g) == {"name", "lr_scale", "weight_decay", "frozen", "params"} for g in part) and part[0]["name"] == "default"
    fz = [g for g in part if g["frozen"]]
    assert len(fz) == 1 and fz[0]["params"] and all(n.startswith("blocks.0.") for n in fz[0]["params"])
    live = [k for k, g in enumerate(part) if not g["frozen"]]
    assert np.allclose(np.sqrt((rows[:, live] ** 2).sum(1)), h["grad_norm"], rtol=1e-6)      # the clipped norm is the live groups'
    stepped = [e for e in events if "group_grad_norm" in e]
    assert len(stepped) == 6 and all(e["group_grad_norm"].is_cuda and e["group_grad_norm"].shape == (G,) for e in stepped)
    assert all(torch.equal(v, frozen0[k]) for k, v in model.named_parameters() if k in frozen0)
    h2 = fit(make(), tr, None, resume_from=ck0, param_groups=specs, **kw)
    assert len(h2["train_loss"]) == 3 and np.allclose(h2["train_loss"], h["train_loss"][3:], rtol=1e-4)
    assert np.allclose(h2["group_grad_norm"], rows[3:], rtol=1e-4, atol=1e-12)
    other = make()
    before = {k: v.detach().clone() for k, v in other.state_dict().items()}
    with pytest.raises(ValueError, match="parameter groups"):
        fit(other, tr, None, resume_from=ck0, param_groups=no_weight_decay() + freeze(r"^blocks\.1\."), **kw)
    assert all(torch.equal(v, before[k]) for k, v in other.state_dict().items())
    h3 = fit(make(), tr, None, resume_from=ck0, **kw)      # a step without groups ignores the key, as one without an average ignores that
    assert len(h3["train_loss"]) == 3
