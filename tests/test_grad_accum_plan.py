"""CPU: gradient accumulation and clipping, the parts that need no GPU.

* the stepping arithmetic of ``accumulate_grad_batches`` (trainer.accumulation_plan): which batches of an epoch step the optimizer, and how
  many steps that makes -- Lightning steps on every k-th batch and on the epoch's last one, ``estimated_stepping_batches`` counts
  ceil(batches / k) per epoch;
* BucketReducer under accumulation (gloo, world 2, as test_ddp_gloo.py runs it): micro-steps inside no_sync() launch nothing, the final one
  launches one collective per bucket in gradient-ready order, and the result is the mean over ranks of the summed micro-gradients;
* TrainStep refuses an unknown ``gradient_clip_algorithm``; the C ABI declares the new entry points on both sides."""
import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_ddp_gloo import Toy, _free_port

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("per_epoch", [1, 5, 6, 1000])
@pytest.mark.parametrize("k", [1, 2, 4])
def test_accumulation_plan(per_epoch, k):
    from bubbleformer_amd.trainer import accumulation_plan
    steps, n = accumulation_plan(per_epoch, k)
    assert n == len(steps) == math.ceil(per_epoch / k)
    # every full group ends on its k-th batch; the last batch always steps; nothing else does
    assert steps == sorted(set(steps)) and steps[-1] == per_epoch - 1
    full = [i for i in range(per_epoch) if i % k == k - 1]
    assert steps[:len(full)] == full and len(steps) - len(full) == (1 if per_epoch % k else 0)
    # replaying the plan as TrainStep counts it: a group never holds more than k batches, and all of them but the epoch's last hold exactly k
    sizes, pending = [], 0
    for i in range(per_epoch):
        pending += 1
        if i in steps:
            sizes.append(pending)
            pending = 0
    assert pending == 0 and sum(sizes) == per_epoch and all(s == k for s in sizes[:-1]) and 1 <= sizes[-1] <= k
    if k == 1:
        assert steps == list(range(per_epoch))


def test_accumulation_plan_known_cases():
    from bubbleformer_amd.trainer import accumulation_plan
    assert accumulation_plan(5, 2) == ([1, 3, 4], 3)
    assert accumulation_plan(6, 4) == ([3, 5], 2)
    assert accumulation_plan(1, 4) == ([0], 1)
    assert accumulation_plan(0, 2) == ([], 0)
    with pytest.raises(ValueError):
        accumulation_plan(5, 0)


MICRO = 3      # micro-batches per group in the reducer test


def _accum_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from bubbleformer_amd.trainer import BucketReducer, FlatParams, stage_buckets
    torch.manual_seed(0)
    model = Toy()
    flat = FlatParams(model)
    red = BucketReducer(flat, stage_buckets(model, blocks_per_bucket=1))
    g = torch.Generator().manual_seed(321)
    xs = torch.randn(MICRO, world, 4, 6, generator=g)
    ys = torch.randn(MICRO, world, 4, 2, generator=g)
    flat.zero_grad()
    logs = []
    for i in range(MICRO):
        red.begin_step()
        loss = ((model(xs[i, rank]) - ys[i, rank]) ** 2).mean()
        if i < MICRO - 1:
            with red.no_sync():
                loss.backward()
            assert red.sync and not red.handles and red.held is None and not red.done and red.pending == [0] * len(red.pending)
        else:
            loss.backward()
        logs.append(list(red.launch_log))
    scale = red.wait() / MICRO
    assert logs[:-1] == [[]] * (MICRO - 1), logs
    assert logs[-1] == [4, 3, 2, 1, 0], logs          # one collective per bucket, gradient-ready order, as without accumulation
    assert red.pending == [0] * len(red.pending) and not red.handles
    torch.save({"grad": flat.grad * scale, "xs": xs, "ys": ys}, out + str(rank))
    dist.barrier()
    dist.destroy_process_group()


def test_bucket_reducer_under_accumulation(tmp_path):
    out = str(tmp_path / "acc")
    mp.spawn(_accum_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    a, b = torch.load(out + "0"), torch.load(out + "1")
    assert torch.equal(a["grad"], b["grad"])          # the same averaged gradient on both ranks
    from bubbleformer_amd.trainer import FlatParams
    # the mean over ranks of the summed micro-gradients, over MICRO: each rank's micro-gradients summed on their own first
    per_rank = []
    for rank in range(2):
        torch.manual_seed(0)
        model = Toy()
        flat = FlatParams(model)
        for i in range(MICRO):
            ((model(a["xs"][i, rank]) - a["ys"][i, rank]) ** 2).mean().backward()
        per_rank.append(flat.grad.clone())
    want = (per_rank[0] + per_rank[1]) / 2 / MICRO
    assert want.abs().max() > 0
    assert torch.allclose(a["grad"], want, rtol=1e-5, atol=1e-7)
    # and it is not what the last micro-batch alone would give
    torch.manual_seed(0)
    model = Toy()
    flat = FlatParams(model)
    ((model(a["xs"][MICRO - 1].reshape(8, 6)) - a["ys"][MICRO - 1].reshape(8, 2)) ** 2).mean().backward()
    assert not torch.allclose(a["grad"], flat.grad / MICRO, rtol=1e-2, atol=1e-7)


def test_train_step_refuses_an_unknown_clip_algorithm():
    from bubbleformer_amd.trainer import TrainStep
    with pytest.raises(ValueError):
        TrainStep(Toy(), gradient_clip_val=1.0, gradient_clip_algorithm="nope")
    with pytest.raises(ValueError):
        TrainStep(Toy(), accumulate_grad_batches=0)
    with pytest.raises(ValueError):
        TrainStep(Toy(), gradient_clip_val=-1.0)


def test_train_step_defaults_are_off():
    from bubbleformer_amd.trainer import TrainStep
    step = TrainStep(Toy())
    assert step.clip_val is None and step.grad_norm is None and step.accumulate_grad_batches == 1 and step.micro == 0
    assert TrainStep(Toy(), gradient_clip_val=0.0).clip_val is None          # Lightning: 0 means no clipping
    assert not step.finish_accumulation() and step.step_no == 0             # nothing pending: nothing happens


def test_abi_declares_the_clip_entry_points():
    """test_abi_exports.py compares the header, the library and _lib.SIGNATURES as sets; this names the new members of all three."""
    import re
    from bubbleformer_amd import _lib
    txt = open(os.path.join(REPO, "include", "bubbleformer_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(bf_[a-z0-9_]+)\s*\(", txt))
    new = {"bf_grad_norm", "bf_grad_norm_ws_doubles", "bf_adamw", "bf_adam", "bf_lion"}
    assert new <= declared and new <= set(_lib.SIGNATURES)
    # the device coefficient and the clamp are fields of the optimizers' bf_opt_step record: the _dev entries are gone, one entry of two parameters each
    gone = {"bf_adamw_dev", "bf_adam_dev", "bf_lion_dev"}
    assert not any(n in txt for n in gone) and not gone & set(_lib.SIGNATURES)
    assert all(len(_lib.SIGNATURES[n][1]) == 2 and len(re.search(r"\b%s\s*\(([^)]*)\)" % n, txt).group(1).split(",")) == 2 for n in ("bf_adamw", "bf_adam", "bf_lion"))
    assert {"coef_dev", "clip_value"} <= {n for n, _ in _lib.OptStep._fields_}
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    h = _lib.lib()
    assert all(hasattr(h, n) for n in new) and h.bf_abi_version() == 3
    # the slab rule depends on n alone: at most 1024 partials, one for a short buffer
    assert h.bf_grad_norm_ws_doubles(64) == 1 and h.bf_grad_norm_ws_doubles(4160) == 2 and 1 <= h.bf_grad_norm_ws_doubles(1 << 34) <= 1024
