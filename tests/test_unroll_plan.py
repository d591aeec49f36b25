"""CPU: the parts of the unrolled training step that need no GPU.

* ``trainer.unroll_plan``: which passes of a step unrolled through k of the model's own predictions take gradients, in which order their
  backwards run and which of them synchronises -- held to its rule over k = 1..4, both ``unroll_backprop`` values, weights with zeros,
  and a completing / non-completing micro-batch of ``accumulate_grad_batches`` (1 and 3);
* ``BubbleForecast.unrollable(k)`` against a brute-force check of ``locate()`` and the file lengths;
* BucketReducer in the direct-gradient mode (``stage_ready``) under K passes through the same parameters (gloo, world 2, as
  test_ddp_gloo.py runs it): with all but the last pass inside ``no_sync()`` every bucket is exchanged once, after the last pass began,
  and the result is the mean over ranks of the summed gradients."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_ddp_gloo import Toy, _free_port

WEIGHTS = {1: [None, (2.0,)], 2: [None, (0.25, 0.75), (0.0, 1.0), (1.0, 0.0)], 3: [None, (0.0, 1.0, 0.0), (0.5, 0.0, 0.5), (1.0, 0.0, 0.0)],
           4: [None, (0.0, 0.0, 0.0, 1.0), (0.0, 1.0, 0.0, 2.0), (0.1, 0.2, 0.3, 0.4)]}
CASES = [(k, w) for k in (1, 2, 3, 4) for w in WEIGHTS[k]]


@pytest.mark.parametrize("accumulate_grad_batches", [1, 3])
@pytest.mark.parametrize("backprop", [True, False])
@pytest.mark.parametrize("k,weights", CASES)
def test_unroll_plan_rule(k, weights, backprop, accumulate_grad_batches):
    from bubbleformer_amd.trainer import unroll_plan
    for micro in range(accumulate_grad_batches):
        final = micro + 1 >= accumulate_grad_batches          # TrainStep.__call__'s rule
        w, plan = unroll_plan(k, weights, backprop, final)
        assert len(w) == k and (w == [1.0 / k] * k if weights is None else w == [float(v) for v in weights])
        fwd = [(j, g) for op, j, g in plan if op == "forward"]
        bwd = [(j, s) for op, j, s in plan if op == "backward"]
        assert [j for j, _ in fwd] == list(range(k))                        # every pass runs forward once, in order
        pos = {(op, j): i for i, (op, j, _) in enumerate(plan)}
        assert len(pos) == len(plan)
        grad = dict(fwd)
        if backprop:
            # pass j is on the gradient path of every later loss: it takes gradients iff some w_i > 0 with i >= j
            want = [any(v > 0 for v in w[j:]) for j in range(k)]
            assert [grad[j] for j in range(k)] == want
            assert [j for j, _ in bwd] == [j for j in reversed(range(k)) if want[j]]      # from the last such pass down to the first
            assert all(pos[("forward", k - 1)] < pos[("backward", j)] for j, _ in bwd)   # all forwards first
        else:
            want = [v > 0 for v in w]                                       # detached feedback: only its own loss reaches a pass
            assert [grad[j] for j in range(k)] == want
            assert [j for j, _ in bwd] == [j for j in range(k) if want[j]]
            assert all(pos[("backward", j)] == pos[("forward", j)] + 1 for j, _ in bwd)   # right behind its forward: one pass alive
        assert bwd, "some pass has a positive weight"
        assert all(grad[j] for j, _ in bwd)
        # a bucket is exchanged once per optimizer step, during the backward that runs last -- of a completing micro-batch only
        assert [s for _, s in bwd] == [False] * (len(bwd) - 1) + [final]


def test_unroll_plan_known_cases():
    from bubbleformer_amd.trainer import unroll_plan
    assert unroll_plan(1) == ([1.0], [("forward", 0, True), ("backward", 0, True)])
    assert unroll_plan(2, None, True)[1] == [("forward", 0, True), ("forward", 1, True), ("backward", 1, False), ("backward", 0, True)]
    assert unroll_plan(2, None, False)[1] == [("forward", 0, True), ("backward", 0, False), ("forward", 1, True), ("backward", 1, True)]
    assert unroll_plan(3, (0.5, 0.0, 0.5), False, False)[1] == [("forward", 0, True), ("backward", 0, False), ("forward", 1, False),
                                                                ("forward", 2, True), ("backward", 2, False)]
    assert unroll_plan(3, (0.0, 1.0, 0.0), True)[1] == [("forward", 0, True), ("forward", 1, True), ("forward", 2, False),
                                                        ("backward", 1, False), ("backward", 0, True)]


@pytest.mark.parametrize("k,weights", [(0, None), (-1, None), (1.5, None), (2, (1.0,)), (2, (1.0, 1.0, 1.0)), (2, (0.0, 0.0)), (2, (1.0, -0.5)),
                                       (2, (float("nan"), 1.0)), (2, (float("inf"), 1.0))])
def test_unroll_plan_refuses_invalid_arguments(k, weights):
    from bubbleformer_amd.trainer import TrainStep, unroll_plan
    with pytest.raises(ValueError):
        unroll_plan(k, weights)
    with pytest.raises(ValueError):
        TrainStep(Toy(), criterion=lambda p, y: ((p - y) ** 2).mean(), unroll_steps=k, unroll_weights=weights)


def test_train_step_unroll_defaults_and_refusals():
    from bubbleformer_amd.trainer import TrainStep
    step = TrainStep(Toy())
    assert step.unroll_steps == 1 and step.unroll_weights == [1.0] and step.unroll_backprop and step.unroll_losses is None
    step = TrainStep(Toy(), criterion=lambda p, y: ((p - y) ** 2).mean(), unroll_steps=3, unroll_backprop=False)
    assert step.unroll_steps == 3 and step.unroll_weights == [1 / 3] * 3 and not step.unroll_backprop
    # a model whose forward_loss cannot keep its prediction in the graph (the U-Nets; the toy has none at all) is not unrolled through it
    with pytest.raises(NotImplementedError, match="forward_loss"):
        TrainStep(Toy(), unroll_steps=2)

    class NoFeedback(Toy):
        def forward_loss(self, x, target):
            return ((self(x) - target) ** 2).mean(), None
    with pytest.raises(NotImplementedError, match="pred_grad"):
        TrainStep(NoFeedback(), unroll_steps=2)
    TrainStep(NoFeedback(), unroll_steps=1)


@pytest.mark.parametrize("name", ["unet_modern", "unet_classic"])
def test_unet_forward_loss_is_not_unrolled(name):
    """The U-Nets' fused loss is out of the unrolled step's scope: asked for it, TrainStep says so; with a criterion it builds."""
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.trainer import TrainStep
    model = get_model(name, time_window=2, input_fields=2, output_fields=2, hidden_channels=8)
    with pytest.raises(NotImplementedError, match="U-Nets"):
        TrainStep(model, unroll_steps=2)
    assert TrainStep(model, unroll_steps=2, criterion=lambda p, y: ((p - y) ** 2).mean()).unroll_steps == 2


def test_fit_refuses_to_unroll_over_unequal_field_lists():
    """Equal counts are not enough: predictions would be fed back into the wrong channels.  fit compares the lists, as plan_rollouts does."""
    from bubbleformer_amd.data.dataset import BubbleForecast
    from bubbleformer_amd.fit import fit
    trajs = [{n: np.zeros((12, 4, 4), np.float32) for n in ("dfun", "temperature")}]
    ds = BubbleForecast.from_arrays(trajs, input_fields=["dfun", "temperature"], output_fields=["temperature", "dfun"], time_window=2, start_time=0)
    with pytest.raises(ValueError, match="feeds predictions back as inputs"):
        fit(Toy(), ds, None, batch_size=2, max_epochs=1, unroll_steps=2)


# ------------------------------------------------------------------------------------------------ unrollable(k)
def _dataset(lens, T, start):
    from bubbleformer_amd.data.dataset import BubbleForecast
    trajs = [{"dfun": np.zeros((n, 4, 4), np.float32), "temperature": np.zeros((n, 4, 4), np.float32)} for n in lens]
    return BubbleForecast.from_arrays(trajs, input_fields=["dfun", "temperature"], output_fields=["dfun", "temperature"], time_window=T,
                                      start_time=start)


@pytest.mark.parametrize("lens,T,start", [((23, 14, 31), 3, 2), ((40, 17), 4, 5), ((12,), 2, 0)])
def test_unrollable_equals_a_brute_force_check(lens, T, start):
    ds = _dataset(lens, T, start)
    assert len(ds) == sum(n - start - 2 * T + 1 for n in lens)
    assert ds.unrollable(1) == list(range(len(ds)))                         # one target clip: every sample has it
    for k in (1, 2, 3, 4):
        want = []
        for i in range(len(ds)):
            fi, first = ds.locate(i)
            if first + (k + 1) * T <= ds.traj_lens[fi]:                     # the last frame of target clip k is frame first + (k + 1) T - 1
                want.append(i)
        assert ds.unrollable(k) == want, k
        per_file = [max(0, n - start - (k + 1) * T + 1) for n in lens]
        assert len(want) == sum(per_file)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            ds.unrollable(bad)


def test_unrollable_skips_a_file_that_is_too_short():
    ds = _dataset((23, 14, 31), 3, 2)               # file 1: 14 - 2 - 4 * 3 + 1 = 1 sample for k = 3 ... and none for k = 4; file 0: 23 - 2 - 12 + 1 = 10
    assert [ds.locate(i)[0] for i in ds.unrollable(3)].count(1) == 1
    assert 1 not in {ds.locate(i)[0] for i in ds.unrollable(4)}
    short = _dataset((23, 11, 31), 3, 2)            # 11 - 2 - 12 + 1 < 0: the file has samples (4) but none that unrolls three times
    assert short._per_traj()[1] == 4
    files = [short.locate(i)[0] for i in short.unrollable(3)]
    assert files.count(1) == 0 and files.count(0) == 10 and files.count(2) == 18
    assert _dataset((12,), 2, 0).unrollable(6) == []


# ------------------------------------------------------------------------------------------------ reducer under K passes
PASSES = 3


def _passes_worker(rank, world, port, out, guarded):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from bubbleformer_amd.trainer import BucketReducer, FlatParams, stage_buckets
    torch.manual_seed(0)
    model = Toy()
    flat = FlatParams(model)
    buckets = stage_buckets(model, blocks_per_bucket=1)
    red = BucketReducer(flat, buckets, use_hooks=False)                 # TrainStep's direct-gradient mode: stage_ready() completes buckets
    stages = [[p.data_ptr() for p in m.parameters()] for m in [model.debed, *reversed(model.blocks), model.embed]]      # gradient-ready order
    g = torch.Generator().manual_seed(77)
    grads = torch.randn(PASSES, world, flat.numel, generator=g)          # what pass i's kernels add to the flat buffer on this rank
    flat.zero_grad()
    red.begin_step()
    began_last_at = None
    for i in range(PASSES):
        last = i == PASSES - 1
        if last:
            began_last_at = len(red.launch_log)
        with red.no_sync() if (guarded and not last) else _null():
            for ptrs in stages:
                lo = min(flat.offsets[j] for j, p in enumerate(flat.params) if p.data_ptr() in ptrs)
                hi = max(flat.offsets[j] + p.numel() for j, p in enumerate(flat.params) if p.data_ptr() in ptrs)
                flat.grad[lo:hi] += grads[i, rank, lo:hi]
                red.stage_ready(ptrs)
    red.flush()
    log = list(red.launch_log)
    scale = red.wait()
    torch.save({"grad": flat.grad * scale, "log": log, "began_last_at": began_last_at, "grads": grads, "offsets": flat.offsets,
                "numels": [p.numel() for p in flat.params]}, out + str(rank))
    dist.barrier()
    dist.destroy_process_group()


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def test_bucket_reducer_under_unrolled_passes(tmp_path):
    out = str(tmp_path / "unr")
    mp.spawn(_passes_worker, args=(2, _free_port(), out, True), nprocs=2, join=True)
    a, b = torch.load(out + "0"), torch.load(out + "1")
    assert a["log"] == b["log"] == [4, 3, 2, 1, 0]              # each bucket once, in gradient-ready order
    assert a["began_last_at"] == 0                               # ... and none of them before the last pass began
    assert torch.equal(a["grad"], b["grad"])
    want = a["grads"].sum(0).mean(0)                             # the mean over ranks of the gradients summed over the passes
    live = torch.zeros(want.numel(), dtype=torch.bool)
    for o, n in zip(a["offsets"], a["numels"]):
        live[o:o + n] = True
    assert torch.allclose(a["grad"][live], want[live], rtol=1e-6, atol=1e-7)


def test_bucket_reducer_without_the_guard_exchanges_too_early(tmp_path):
    """What the schedule is there to prevent: K passes of stage_ready() outside no_sync() complete every bucket in the first pass, while
    later passes still add to it -- the buckets are launched before the last pass begins, and more than once."""
    out = str(tmp_path / "raw")
    mp.spawn(_passes_worker, args=(2, _free_port(), out, False), nprocs=2, join=True)
    a = torch.load(out + "0")
    assert a["began_last_at"] > 0 and len(a["log"]) > 5
