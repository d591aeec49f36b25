"""GPU: seeded Gaussian input noise -- bf_clip_noise against its host restatement element by element, its purity, its moments, and the
training step, the unrolled step and fit() with ``input_noise``.

The per-element bound: |got - (x + sigma z64)| <= sigma K 2^-23 max(r, 1) + 2^-24 |x + sigma z64|, z64 and the Box-Muller radius r from
tests/noise_restatement.py in fp64.  The second term is the rounding of the fused multiply-add; the first allows K fp32 ulps on the chain
logf -> sqrtf -> cospif / sinpif -> product of a normal of radius r.  K_MEASURED is the largest K the cases below needed on an MI355X
(a K above 8 would mean the approximate functions ran: a defect, not a tolerance to widen); the tests hold K = twice that, rounded up."""
import ctypes
import json

import numpy as np
import pytest
import torch

from tests import noise_restatement as NR
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu

K_MEASURED = 1.082        # (2, 2, 4, 16, 16), draw 2^32 - 1, pass 3, seed 2^63 + 42; the other cases 0.02 .. 0.92
K = 3.0
SIGMA = (0.5, 0.0, 2.0, 1.0)
IDS = (7, 2 ** 31 + 3, 0)
PARAMS = [(0, 0, 0), (2 ** 32 - 1, 3, 2 ** 63 + 42)]            # (draw, pass, seed)


def _noise(x, sigma, ids, draw, pas, seed, out=None):
    from bubbleformer_amd.utils import add_gaussian_noise
    return add_gaussian_noise(x, sigma, None if ids is None else torch.tensor(ids, dtype=torch.int64, device="cuda"), draw, pas, seed, out=out)


def _clip(shape, seed, offset=0):
    """A random fp32 clip on the device; offset > 0: a contiguous view that begins `offset` floats into its buffer (misaligned)."""
    n = int(np.prod(shape))
    buf = torch.randn(n + offset, generator=torch.Generator().manual_seed(seed)).cuda()
    return buf[offset:].view(shape)


def _hold(got, x, sigma, ids, draw, pas, seed, what):
    want, r, sig = NR.noisy_clip(x.cpu().numpy(), sigma, ids, draw, pas, seed)
    g = got.cpu().numpy().astype(np.float64)
    need = NR.needed_K(g, want, r, sig)
    print(f"{what}: K needed {need:.3f} (held: {K})")
    assert np.all(np.abs(g - want) <= NR.element_bound(want, r, sig, K)), (what, need)
    return need


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("draw,pas,seed", PARAMS)
@pytest.mark.parametrize("shape,offset", [((3, 2, 3, 5, 7), 0), ((2, 2, 4, 16, 16), 0), ((1, 1, 1, 1, 1), 0), ((2, 1, 3, 4, 4), 1)])
def test_kernel_matches_the_restatement_element_by_element(shape, offset, draw, pas, seed):
    """(3, 2, 3, 5, 7): 210 elements per sample -- a ragged last group, rows that are no multiple of 4; (2, 2, 4, 16, 16): the 16-byte path;
    one element; and an aligned-size clip on a view one float into its buffer, which takes the scalar path."""
    x = _clip(shape, 5, offset)
    assert (x.data_ptr() % 16 != 0) == (offset != 0)
    sigma, ids = SIGMA[:shape[2]], IDS[:shape[0]]
    keep = x.clone()
    got = _noise(x, sigma, ids, draw, pas, seed)
    assert got.data_ptr() != x.data_ptr() and torch.equal(x, keep)
    _hold(got, x, sigma, ids, draw, pas, seed, f"{shape} +{offset} draw {draw} pass {pas} seed {seed}")
    if shape[2] > 1:
        assert torch.equal(got[:, :, 1], x[:, :, 1])                    # sigma = 0: bit for bit
        assert not torch.equal(got[:, :, 0], x[:, :, 0]) and not torch.equal(got[:, :, 2], x[:, :, 2])
    if offset:
        into = _clip(shape, 6, offset)                                  # a misaligned destination as well
        assert torch.equal(_noise(x, sigma, ids, draw, pas, seed, out=into), got) and into.data_ptr() % 16 != 0


@pytest.mark.parametrize("shape", [(3, 2, 3, 5, 7), (3, 2, 4, 16, 16)])
def test_noise_is_a_pure_function_of_its_counter(shape):
    x = _clip(shape, 8)
    sigma = SIGMA[:shape[2]]
    draw, pas, seed = 12, 1, 99
    got = _noise(x, sigma, IDS, draw, pas, seed)
    for b in range(3):                                                   # a row is the one-sample call with that row's id
        assert torch.equal(got[b:b + 1], _noise(x[b:b + 1].contiguous(), sigma, IDS[b:b + 1], draw, pas, seed)), b
    assert torch.equal(_noise(x, sigma, IDS, draw, pas, seed), got)      # two calls: the same bits
    inplace = x.clone()
    assert _noise(inplace, sigma, IDS, draw, pas, seed, out=inplace) is inplace and torch.equal(inplace, got)
    for what, args in {"seed": (IDS, draw, pas, seed + 1), "draw": (IDS, draw + 1, pas, seed), "pass": (IDS, draw, pas + 1, seed),
                       "sample id": ((7, 2 ** 31 + 3, 1), draw, pas, seed), "seed high word": (IDS, draw, pas, seed + 2 ** 32)}.items():
        other = _noise(x, sigma, *args)
        assert not torch.equal(other, got), what
        if what == "sample id":
            assert torch.equal(other[:2], got[:2]) and not torch.equal(other[2], got[2])
    assert torch.equal(_noise(x, sigma, None, draw, pas, seed), _noise(x, sigma, (0, 1, 2), draw, pas, seed))
    assert torch.equal(_noise(x, sigma, (2 ** 32 + 7, 2 ** 31 + 3, 0), draw, pas, seed), got)        # ids count modulo 2^32
    from bubbleformer_amd.utils import add_gaussian_noise
    assert torch.equal(add_gaussian_noise(x, sigma, list(IDS), draw, pas, seed), got)                # host ids are staged
    assert torch.equal(add_gaussian_noise(x, torch.tensor(sigma, device="cuda"), torch.tensor(IDS, device="cuda"), draw, pas, seed), got)


def test_arguments_are_checked():
    from bubbleformer_amd import _lib as L
    from bubbleformer_amd.utils import add_gaussian_noise
    x = _clip((2, 1, 3, 4, 4), 1)
    with pytest.raises(ValueError):
        add_gaussian_noise(x, (0.1, 0.2))
    with pytest.raises(ValueError):
        add_gaussian_noise(x, -0.1)
    with pytest.raises(ValueError):
        add_gaussian_noise(x, 0.1, sample_ids=[1, 2, 3])
    with pytest.raises(ValueError):
        add_gaussian_noise(x[0], 0.1)
    with pytest.raises(L.BubbleformerHipError):
        add_gaussian_noise(x.double(), 0.1)
    with pytest.raises(L.BubbleformerHipError):
        add_gaussian_noise(x.transpose(3, 4), 0.1)
    with pytest.raises(L.BubbleformerHipError):
        add_gaussian_noise(x, 0.1, out=torch.empty(2, 1, 3, 4, 5, device="cuda"))


def test_moments_on_the_device():
    """One (1, 4, 4, 256, 256) clip of zeros with sigma = 1 is 2^20 normals: the five statistics of tests/test_noise.py within +-5 standard
    errors, |z| <= 5.77, and the first 4096 values within the per-element bound of the restatement."""
    x = torch.zeros(1, 4, 4, 256, 256, device="cuda")
    z = _noise(x, 1.0, (5,), 1, 0, 42)
    st = NR.moment_statistics(z.cpu().numpy())
    print({k: round(float(v), 3) for k, v in st.items()}, "max |z| %.4f" % float(z.abs().max()))
    assert all(abs(v) <= 5.0 for v in st.values()), st
    assert float(z.abs().max()) <= NR.Z_MAX
    want, r = NR.normals(42, 5, 1, 0, 4096)
    got = z.flatten()[:4096].cpu().numpy().astype(np.float64)
    one = np.ones(4096)
    print("first 4096: K needed %.3f" % NR.needed_K(got, want, r, one))
    assert np.all(np.abs(got - want) <= NR.element_bound(want, r, one, K))


# ------------------------------------------------------------------------------------------------ the step
def _tiny_model(name):
    from bubbleformer_amd.models import get_model
    torch.manual_seed(0)
    kw = dict(num_fluid_params=9) if name == "filmavit" else {}
    return get_model(name, input_fields=4, output_fields=4, time_window=2, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=1,
                     drop_path=0.0, compute_dtype=torch.float32, **kw).cuda().train()


def _tiny_data(name, i=0):
    g = torch.Generator().manual_seed(40 + i)
    x, y = torch.randn(2, 2, 4, 16, 16, generator=g).cuda(), torch.randn(2, 2, 4, 16, 16, generator=g).cuda()
    return x, (torch.randn(2, 9, generator=g).cuda() if name == "filmavit" else None), y


@pytest.mark.parametrize("name", ["avit", "filmavit"])
def test_step_with_noise_is_the_plain_step_on_the_hand_perturbed_clip(name):
    """Bit for bit: the loss and the flat gradient buffer, over two optimizer steps (draw = 0, then 1); the caller's x is not written."""
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils import NoiseSpec, add_gaussian_noise
    spec = NoiseSpec(SIGMA, seed=2 ** 63 + 42)
    ids = torch.tensor([7, 2 ** 31 + 3], device="cuda")
    noisy, plain = TrainStep(_tiny_model(name), lr=1e-3, input_noise=spec), TrainStep(_tiny_model(name), lr=1e-3)
    for i in range(2):
        x, c, y = _tiny_data(name, i)
        keep = x.clone()
        la = noisy(x, c, y, sample_ids=ids)
        assert torch.equal(x, keep)
        fed = add_gaussian_noise(x, SIGMA, ids, draw=i, pass_index=0, seed=spec.seed)
        assert not torch.equal(fed, x)
        lb = plain(fed, c, y)
        assert torch.equal(la, lb) and torch.equal(noisy.flat.grad, plain.flat.grad), i
        assert noisy.step_no == plain.step_no == i + 1
    assert torch.equal(noisy.flat.flat, plain.flat.flat)
    # ... and it is not the step on the clean clip, nor the step under another draw
    clean = TrainStep(_tiny_model(name), lr=1e-3)
    x, c, y = _tiny_data(name, 0)
    assert not torch.equal(clean(x, c, y), TrainStep(_tiny_model(name), lr=1e-3, input_noise=spec)(x, c, y, sample_ids=ids))


def _unrolled_case():
    from tests.test_gpu_unroll_model import _clips
    from tests.test_gpu_parity import build_product_model
    spec, _, model = build_product_model("avit_plain", torch.float32)
    x, ys, _ = _clips(spec, 2, torch.float32)
    return model.train(), x.cuda(), torch.stack(ys).cuda()


def _sigma_for(model_inputs):
    return SIGMA[:model_inputs] if model_inputs <= len(SIGMA) else tuple(SIGMA[i % len(SIGMA)] for i in range(model_inputs))


@pytest.mark.parametrize("passes", ["all", "input", "fed_back"])
@pytest.mark.parametrize("backprop", [False, True])
def test_unrolled_step_feeds_back_the_perturbed_prediction(passes, backprop):
    """k = 2: step.unroll_losses are, bit for bit, the losses of a hand-run two-pass computation that applies add_gaussian_noise where the
    spec says -- pass 0 sees x itself under "fed_back", pass 1 sees pred_0 itself under "input"."""
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils import NoiseSpec, add_gaussian_noise
    model, x, ys = _unrolled_case()
    sigma = _sigma_for(x.shape[2])
    spec = NoiseSpec(sigma, seed=17, passes=passes)
    ids = torch.tensor([2 ** 31 + 3], device="cuda")
    step = TrainStep(model, lr=1e-3, unroll_steps=2, unroll_backprop=backprop, input_noise=spec)
    keep = x.clone()
    step(x, None, ys, sample_ids=ids)
    got = step.unroll_losses.clone()
    assert torch.equal(x, keep)
    hand, _, _ = _unrolled_case()                                       # the same forwards as the step runs them, no backward
    x0 = add_gaussian_noise(x, sigma, ids, 0, 0, 17) if passes != "fed_back" else x
    l0, p0 = hand.forward_loss(x0, ys[0], pred_grad=backprop)
    p0 = p0.detach()
    x1 = add_gaussian_noise(p0, sigma, ids, 0, 1, 17) if passes != "input" else p0
    l1, _ = hand.forward_loss(x1.clone().requires_grad_() if backprop else x1, ys[1])
    clean = hand.forward_loss(hand.forward_loss(x, ys[0])[1].detach(), ys[1])[0]
    assert torch.equal(got, torch.stack([l0, l1]).detach().float()), (got, l0, l1)
    assert (passes == "fed_back") == torch.equal(x0, x) and (passes == "input") == torch.equal(x1, p0)
    assert not torch.equal(l1, clean)


def test_unrolled_backprop_gradient_is_that_of_the_graph_with_the_noise_held_constant():
    """k = 2 with gradients through the fed-back prediction: every gradient tensor against ONE autograd graph whose second input is
    pred_0 + n, n = the noise as a constant -- per tensor within the bound tests/test_gpu_unroll_model.py holds fused against composed
    (max(1e-4, 4 x the oracle's own fp32-against-fp64 error of the unrolled computation))."""
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils import NoiseSpec, add_gaussian_noise
    from tests.test_gpu_unroll_model import _bounds, _close_per_tensor, oracle_unrolled
    model, x, ys = _unrolled_case()
    sigma = tuple(0.05 * s for s in _sigma_for(x.shape[2]))
    ids = torch.tensor([3], device="cuda")
    step = TrainStep(model, lr=1e-3, unroll_steps=2, unroll_backprop=True, input_noise=NoiseSpec(sigma, seed=17))
    step(x, None, ys, sample_ids=ids)
    got = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}
    hand, _, _ = _unrolled_case()
    l0, p0 = hand.forward_loss(add_gaussian_noise(x, sigma, ids, 0, 0, 17), ys[0], pred_grad=True)
    n = add_gaussian_noise(p0.detach(), sigma, ids, 0, 1, 17) - p0.detach()
    l1, _ = hand.forward_loss(p0 + n, ys[1])
    (0.5 * l0 + 0.5 * l1).backward()
    want = {n: p.grad.detach().cpu().clone() for n, p in hand.named_parameters()}
    bounds = _bounds(oracle_unrolled("avit_plain", 2, None, True, torch.float64), oracle_unrolled("avit_plain", 2, None, True, torch.float32))
    _close_per_tensor(got, want, bounds, "noisy unrolled step against the hand-built graph")
    # control: the noise reached the gradient -- the clean unrolled step's is further away than the bound
    clean, _, _ = _unrolled_case()
    TrainStep(clean, lr=1e-3, unroll_steps=2, unroll_backprop=True)(x, None, ys)
    name = next(k for k in want if k.startswith("embed.") and k.endswith("0.weight"))
    assert rel_l2(dict(clean.named_parameters())[name].grad.cpu(), want[name]) > 2 * bounds[name]


def test_off_is_off():
    """input_noise=None and NoiseSpec(std=0.0) give torch.equal losses and flat gradients over two steps, and the launch profile of the
    step holds no clip_noise entry (one with noise on holds one per perturbed pass)."""
    from bubbleformer_amd import _lib as L
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils import NoiseSpec
    h = L.lib()

    def run(spec, profile=False):
        step = TrainStep(_tiny_model("avit"), lr=1e-3, input_noise=spec)
        out = []
        if profile:
            h.bf_prof_enable(1)
        for i in range(2):
            x, c, y = _tiny_data("avit", i)
            out.append((step(x, c, y, sample_ids=[4, 5]).clone(), step.flat.grad.clone()))
        torch.cuda.synchronize()
        names = None
        if profile:
            buf = ctypes.create_string_buffer(1 << 15)
            h.bf_prof_report(buf, len(buf))
            h.bf_prof_enable(0)
            names = json.loads(buf.value.decode())
        return out, names
    a, names_off = run(None, profile=True)
    b, names_zero = run(NoiseSpec(std=0.0), profile=True)
    for (la, ga), (lb, gb) in zip(a, b):
        assert torch.equal(la, lb) and torch.equal(ga, gb)
    assert names_off and "clip_noise" not in names_off and "clip_noise" not in names_zero and sorted(names_off) == sorted(names_zero)
    _, names_on = run(NoiseSpec(0.1), profile=True)
    assert names_on["clip_noise"]["calls"] == 2 and sorted(set(names_on) - {"clip_noise"}) == sorted(names_off)


# ------------------------------------------------------------------------------------------------ the loop
def _train_set():
    import os
    from bubbleformer_amd.data import BubbleForecast
    samples = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samples")
    tr = BubbleForecast([os.path.join(samples, f"sample_{i}.hdf5") for i in (1, 2)], norm="std", time_window=2, start_time=5)
    tr.normalize()
    return tr


def _fit(max_epochs=2, seed=3, resume_from=None, checkpoint=None):
    """Two epochs of three batches of four clips of the two sample files at a constant learning rate (so that a run of one epoch is the
    first epoch of a run of two); seed = the noise's, None = no noise.  -> the history"""
    from bubbleformer_amd.fit import fit
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils import NoiseSpec
    tr = _train_set()
    torch.manual_seed(0)
    model = get_model("avit", input_fields=4, output_fields=4, time_window=2, patch_size=8, embed_dim=64, num_heads=2, processor_blocks=1,
                      drop_path=0.0, compute_dtype=torch.float32).cuda()
    noise = NoiseSpec(0.01, relative=True, seed=seed) if seed is not None else None
    hist = fit(model, tr, None, batch_size=4, max_epochs=max_epochs, optimizer="adamw", lr=1e-3, weight_decay=1e-2, warmup_iters=None,
               limit_train_batches=3, seed=42, input_noise=noise, resume_from=resume_from, checkpoint_path=checkpoint)
    torch.cuda.synchronize()
    return hist


def test_fit_with_noise_repeats_resumes_and_depends_on_the_seed(tmp_path):
    a, b = _fit(), _fit()
    assert a == b and len(a["train_loss"]) == 6 and np.isfinite(a["train_loss"]).all()
    ck = str(tmp_path / "epoch0.ckpt")
    first = _fit(max_epochs=1, checkpoint=ck)
    second = _fit(resume_from=ck)
    resumed = torch.tensor(first["train_loss"] + second["train_loss"])
    assert torch.equal(resumed, torch.tensor(a["train_loss"])), (resumed, a["train_loss"])
    other = _fit(seed=4)
    assert other["train_loss"] != a["train_loss"]
    plain = _fit(seed=None)
    assert plain["train_loss"] != a["train_loss"] and plain["train_loss"][0] != a["train_loss"][0]


def test_field_std_of_the_device_store_agrees_with_the_cpu_store():
    tr = _train_set()
    gpu, cpu = tr.device_store("cuda").field_std(), tr.device_store("cpu").field_std()
    assert sorted(gpu) == sorted(cpu) == sorted(tr.fields)
    for name in cpu:
        assert abs(gpu[name] - cpu[name]) <= 1e-6 * abs(cpu[name]), (name, gpu[name], cpu[name])
