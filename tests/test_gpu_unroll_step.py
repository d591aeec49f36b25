"""GPU: the unrolled training step at step level, its clip supply and the epoch loop.

* the default is the step it was: TrainStep(unroll_steps=1) and TrainStep() from the same state give torch.equal losses and parameters,
  in bf16 and in fp32 (at the geometries where the project pins the plain step as bit-reproducible, tests/test_gpu_grad_clip.py: _tiny);
* two runs of two optimizer steps with k = 3 in bf16 (direct-gradient mode) give torch.equal losses and flat gradient buffers;
* DeviceClipStore.gather(idx, unroll=3): targets[j] is bit for bit the target clip of sample idx + j * T, with and without
  downsampling, with fluid rows, for host and device indices; a host index outside unrollable(3) raises;
* fit(..., unroll_steps=2): finite losses, k per-pass losses per batch; with the defaults the history and the parameters are those of a
  run without the new arguments."""
import numpy as np
import pytest
import torch

from tests.test_gpu_grad_clip import _tiny

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the step
@pytest.mark.parametrize("name", ["filmavit_bf16", "filmavit"])
def test_unroll_steps_one_is_the_step_it_was(name):
    from bubbleformer_amd.trainer import TrainStep
    runs = []
    for kw in ({}, dict(unroll_steps=1, unroll_weights=None, unroll_backprop=True)):
        model, data = _tiny(name)
        step = TrainStep(model, lr=1e-3, weight_decay=1e-2, **kw)
        losses = torch.stack([step(*data(i)) for i in range(2)])
        torch.cuda.synchronize()
        assert step.unroll_losses is None and step.step_no == 2
        runs.append((losses.clone(), step.flat.flat.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def _unrolled_twice(k, backprop):
    from bubbleformer_amd.trainer import TrainStep
    from oracle import weights as W
    model, data = _tiny("filmavit_bf16", B=1)
    step = TrainStep(model, lr=1e-3, weight_decay=1e-2, unroll_steps=k, unroll_backprop=backprop)
    losses, grads = [], []
    for i in range(2):
        x, c, _ = data(i)
        ys = torch.stack([W.synthetic_clip(1, 16, 4, 192, 192, 800 + 10 * i + j) for j in range(k)]).cuda()
        losses.append(step(x, c, ys))
        losses.append(step.unroll_losses.sum())
        grads.append(step.flat.grad.clone())
    torch.cuda.synchronize()
    assert step.step_no == 2
    return torch.stack(losses), grads, step


def test_unrolled_bf16_step_repeats_bit_for_bit():
    """k = 3, bf16, gradients through the fed-back predictions, at the geometry where the plain bf16 step is pinned bit-reproducible: the
    losses and the flat gradient buffer after each of two optimizer steps are torch.equal between two runs."""
    a, b = _unrolled_twice(3, True), _unrolled_twice(3, True)
    assert torch.isfinite(a[0]).all()
    differing = []
    for i in range(2):
        per = [[r[1][i][o:o + p.numel()] for p, o in zip(r[2].flat.params, r[2].flat.offsets)] for r in (a, b)]
        for (n, _), ga, gb in zip(a[2].model.named_parameters(), *per):
            if not torch.equal(ga, gb):
                differing.append((i, n, float((ga - gb).norm() / gb.norm().clamp_min(1e-30))))
    print(f"k = 3 bf16: {len(differing)} gradient tensors differ between two runs: {differing[:8]}")
    assert torch.equal(a[0], b[0]), (a[0], b[0])
    assert not differing, differing


def _transient_bytes(k, backprop):
    """Peak allocation of one optimizer step above what is allocated before it (model, optimizer state, inputs, the library's cached
    scratch), measured on the second step."""
    from bubbleformer_amd.trainer import TrainStep
    from oracle import weights as W
    model, data = _tiny("filmavit_bf16", B=1)
    step = TrainStep(model, lr=1e-3, weight_decay=1e-2, unroll_steps=k, unroll_backprop=backprop)
    x, c, y = data(0)
    ys = y if k == 1 else torch.stack([W.synthetic_clip(1, 16, 4, 192, 192, 800 + j) for j in range(k)]).cuda()
    step(x, c, ys)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step(x, c, ys)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_pushforward_keeps_one_pass_alive():
    """unroll_backprop=False: a finished pass's saved activations are released before the next pass runs, also those the deferred
    weight-gradient work keeps referenced.  Beyond the plain step a pushforward pass holds the detached prediction it is fed (one fp32
    clip) while it produces its own: the step's transient allocation is the plain step's plus at most two clips, whatever k; with
    gradients through the predictions it grows by a pass's activations per pass."""
    clip = 16 * 4 * 192 * 192 * 4
    plain = _transient_bytes(1, True)
    push = {k: _transient_bytes(k, False) for k in (2, 3)}
    back = _transient_bytes(3, True)
    print(f"transient MB: k1 {plain / 2**20:.1f}, k2 pushforward {push[2] / 2**20:.1f}, k3 pushforward {push[3] / 2**20:.1f}, k3 backprop {back / 2**20:.1f}")
    assert push[2] <= plain + 2 * clip and push[3] <= plain + 2 * clip, (plain, push)
    assert back > 2 * plain


# ------------------------------------------------------------------------------------------------ the supply
T_WIN, START = 3, 2
LENS = (26, 19)


def _store(downsample=1, fluid=True):
    from bubbleformer_amd.data.dataset import BubbleForecast, FLUID_PARAM_KEYS
    g = np.random.default_rng(5)
    names = ["dfun", "temperature", "velx"]
    trajs = [{n: g.standard_normal((L, 12, 20)).astype(np.float32) for n in names} for L in LENS]
    fp = None
    if fluid:
        fp = [dict({k: float(g.standard_normal()) for k in FLUID_PARAM_KEYS}, heater={"nucWaitTime": 0.1 * (i + 1), "wallTemp": 90.0 + i}) for i in range(len(LENS))]
    ds = BubbleForecast.from_arrays(trajs, fluid_params=fp, input_fields=names, output_fields=["temperature", "dfun"], norm="std", time_window=T_WIN,
                                    start_time=START, downsample_factor=downsample)
    ds.normalize()
    return ds, ds.device_store("cuda")


@pytest.mark.parametrize("downsample,fluid", [(1, True), (2, True), (1, False)])
def test_unrolled_gather_is_the_single_clip_gather_of_the_later_samples(downsample, fluid):
    ds, store = _store(downsample, fluid)
    k = 3
    ok = ds.unrollable(k)
    assert 0 < len(ok) < len(ds) and {ds.locate(i)[0] for i in ok} == {0, 1}
    per0 = ds._per_traj()[0]
    idx = [ok[0], ok[5], [i for i in ok if i < per0][-1], [i for i in ok if i >= per0][0], ok[-1]]      # first / last unrollable sample of each file
    got = store.gather(idx, unroll=k)
    plain = store.gather(idx)
    assert len(got) == len(plain) == (3 if fluid else 2)
    H, Wd = 12 // downsample, 20 // downsample
    assert got[1].shape == (k, len(idx), T_WIN, 2, H, Wd) and got[1].is_contiguous() and got[1][1].is_contiguous()
    assert torch.equal(got[0], plain[0])
    if fluid:
        assert torch.equal(got[2], plain[2])
    for j in range(k):
        later = store.gather([i + j * T_WIN for i in idx])      # sample i + j T starts j T frames later in the same file
        assert torch.equal(got[1][j], later[1]), j
    # the same from device indices, and unroll = 1 is the plain target with a leading axis
    dev = store.gather(torch.tensor(idx, device="cuda"), unroll=k)
    assert all(torch.equal(a, b) for a, b in zip(dev, got))
    one = store.gather(idx, unroll=1)
    assert one[1].shape[0] == 1 and torch.equal(one[1][0], plain[1])
    # against the dataset's own host path
    want = torch.stack([ds[idx[1] + T_WIN][1], ds[idx[1] + 2 * T_WIN][1]])
    assert torch.allclose(got[1][1:, 1].cpu(), want, rtol=1e-6, atol=1e-6)


def test_unrolled_gather_refuses_host_indices_whose_clips_leave_their_file():
    ds, store = _store()
    ok = set(ds.unrollable(3))
    outside = [i for i in range(len(ds)) if i not in ok]
    assert outside
    with pytest.raises(IndexError, match="unrollable"):
        store.gather([min(ok), outside[0]], unroll=3)
    with pytest.raises(IndexError):
        store.gather(torch.tensor([outside[-1]]), unroll=3)          # a host tensor is checked too
    with pytest.raises(IndexError):
        store.gather([len(ds)], unroll=3)
    with pytest.raises(ValueError):
        store.gather([0], unroll=0)
    store.gather([outside[0]])                                        # ... and is a valid sample without unroll
    # a device index is clamped, not checked: the call returns finite frames of the store, whatever they are
    got = store.gather(torch.tensor([len(ds) - 1, 10 ** 6, -4], device="cuda"), unroll=3)
    torch.cuda.synchronize()
    assert torch.isfinite(got[1]).all() and torch.isfinite(got[0]).all()
    assert torch.equal(got[0][1], got[0][0]) and torch.equal(got[0][2], store.gather([0])[0][0])


# ------------------------------------------------------------------------------------------------ the loop
def _fit_run(**extra):
    from bubbleformer_amd.data.dataset import BubbleForecast
    from bubbleformer_amd.fit import fit
    from bubbleformer_amd.models import get_model
    g = np.random.default_rng(9)
    names = ["dfun", "temperature", "velx", "vely"]
    trajs = [{n: g.standard_normal((L, 16, 32)).astype(np.float32) for n in names} for L in (30, 21)]
    ds = BubbleForecast.from_arrays(trajs, input_fields=names, output_fields=names, norm="std", time_window=2, start_time=1)
    ds.normalize()
    torch.manual_seed(0)
    model = get_model("avit", input_fields=4, output_fields=4, time_window=2, patch_size=4, embed_dim=64, num_heads=2, processor_blocks=1,
                      drop_path=0.0, compute_dtype=torch.float32).cuda()
    events = []
    hist = fit(model, ds, None, batch_size=4, max_epochs=2, optimizer="adamw", lr=1e-3, weight_decay=1e-2, warmup_iters=2, limit_train_batches=3,
               seed=42, log=events.append, **extra)
    torch.cuda.synchronize()
    return ds, hist, torch.cat([p.detach().flatten() for p in model.parameters()]).clone(), events


def test_fit_unrolls_and_its_defaults_change_nothing(monkeypatch):
    from bubbleformer_amd.data.dataset import DeviceClipStore
    from bubbleformer_amd.fit import batches, epoch_indices
    k = 2
    calls, real = [], DeviceClipStore.gather

    def recording(self, indices, unroll=None):
        calls.append((list(indices), unroll))
        return real(self, indices, unroll=unroll)
    monkeypatch.setattr(DeviceClipStore, "gather", recording)
    ds, hist, _, events = _fit_run(unroll_steps=k, unroll_weights=(0.25, 0.75))
    monkeypatch.setattr(DeviceClipStore, "gather", real)
    # an epoch shuffles unrollable(k) under the plain loop's seeding and gathers with unroll = k
    pool = ds.unrollable(k)
    want = [b for e in range(2) for b in batches([pool[i] for i in epoch_indices(len(pool), e, 42, True, 0, 1)], 4, 3)]
    assert calls == [(b, k) for b in want] and len(pool) < len(ds)
    assert len(hist["train_loss"]) == 6 and np.isfinite(hist["train_loss"]).all()
    assert len(hist["unroll_loss"]) == 6 and all(len(row) == k for row in hist["unroll_loss"]) and np.isfinite(hist["unroll_loss"]).all()
    for total, row in zip(hist["train_loss"], hist["unroll_loss"]):
        assert abs(total - (0.25 * row[0] + 0.75 * row[1])) <= 1e-5 * abs(total)
    assert [e["global_step"] for e in events if "train_loss" in e] == [1, 2, 3, 4, 5, 6]
    # the defaults: the history and the parameters of a run without the new arguments
    _, h0, p0, _ = _fit_run()
    _, h1, p1, _ = _fit_run(unroll_steps=1, unroll_weights=None, unroll_backprop=True)
    assert "unroll_loss" not in h0 and h0.keys() == h1.keys()
    assert h0 == h1 and torch.equal(p0, p1)
    assert h0["train_loss"] != hist["train_loss"]
