"""Checkpoints in the layout the reference's Lightning runs write and its inference script reads
(bubbleformer/modules.py:57 `save_hyperparameters()`, scripts/inference.py:205-226): a dict with

  "state_dict"        parameter tensors keyed "model.<name>" (the LightningModule holds the network as `self.model`)
  "hyper_parameters"  the module's constructor arguments, incl. "normalization_constants" = (diff_terms, div_terms)
  "global_step"       optimizer steps taken
plus, for resuming the native training step, "optimizer_states" / "lr_schedulers" entries holding the flat AdamW / Adam / Lion
moments and the scheduler position (Lightning stores its torch.optim state dicts under those keys; ours are flat buffers, so a
checkpoint written here resumes here, while its "state_dict" loads anywhere the reference's does).  A training step that keeps an
averaged copy of the weights (TrainStep(weight_average=...)) adds "weight_average": its spec, the update count and the flat average;
a step with parameter groups (TrainStep(param_groups=...)) adds "param_groups": its partition, a list of {name, lr_scale, weight_decay,
frozen, params: [names]} (utils.param_groups.ResolvedGroups.partition), which a grouped step checks on loading;
a step with a guard (TrainStep(step_guard=...)) adds "step_guard": {"skipped": the optimizer steps skipped so far};
`save_checkpoint(averaged=True)` instead writes the averaged weights AS the "state_dict", with no training state: the file to release.

`load_checkpoint` also resumes from a file the reference's Lightning run wrote (e.g. the pre-emption `hpc_ckpt_*.ckpt` files of
scripts/train.py): its `optimizer_states[0]` is a torch.optim state dict, which `flat_state_from_torch_optim` puts into the flat
buffers, and its `lr_schedulers[0]` is the state of the reference's `CosineWarmupLR(SequentialLR)`.  Such a file keeps the run's
`hyper_parameters` as OmegaConf objects, so unpickling it needs the `omegaconf` package, which this project does not ship; a file
whose hyper_parameters are plain dicts loads without it."""
import math
import os
from collections import OrderedDict
from typing import Optional, Sequence

import torch

PREFIX = "model."


def to_reference_state_dict(model: torch.nn.Module) -> "OrderedDict[str, torch.Tensor]":
    return OrderedDict((PREFIX + k, v.detach().to("cpu", copy=True)) for k, v in model.state_dict().items())


def from_reference_state_dict(sd) -> "OrderedDict[str, torch.Tensor]":
    """Strip Lightning's "model." prefix exactly as scripts/inference.py:222-225 does (`key[6:]`)."""
    out = OrderedDict()
    for k, v in sd.items():
        if not k.startswith(PREFIX):
            raise KeyError(f"checkpoint key {k!r} does not start with {PREFIX!r}")
        out[k[len(PREFIX):]] = v
    return out


def save_checkpoint(path: str, model: torch.nn.Module, hyper_parameters: Optional[dict] = None, normalization_constants=None,
                    train_step=None, global_step: Optional[int] = None, epoch: Optional[int] = None, averaged: bool = False) -> None:
    """One torch.save into `path + ".tmp"`, then os.replace: a kill between two writes (the reference's use case is SLURM pre-emption,
    scripts/train.py:36-67) can never leave a half-written or epoch-less file behind.  A `train_step` that averages its weights adds
    "weight_average" = {kind, decay, warmup, start_step, every, n_averaged, avg (the flat buffer, on the CPU)}.  averaged=True: the
    "state_dict" is `train_step.averaged_state_dict()` and no optimizer, scheduler or average state is written -- what the reference's
    `load_state_dict` (scripts/inference.py:205-226) should be handed."""
    hp = dict(hyper_parameters or {})
    if normalization_constants is not None:
        hp["normalization_constants"] = normalization_constants
    if averaged and (train_step is None or getattr(train_step, "avg", None) is None):
        raise ValueError("save_checkpoint(averaged=True) needs a train_step that keeps an average (TrainStep(weight_average=...))")
    ckpt = {"state_dict": train_step.averaged_state_dict() if averaged else to_reference_state_dict(model), "hyper_parameters": hp,
            "global_step": int(global_step if global_step is not None else (train_step.step_no if train_step is not None else 0))}
    if train_step is not None and not averaged:
        ckpt["optimizer_states"] = [{"name": train_step.optimizer, "step": train_step.step_no, "m": train_step.m.detach().cpu(),
                                     "v": None if train_step.v is None else train_step.v.detach().cpu()}]
        ckpt["lr_schedulers"] = [train_step.scheduler.state_dict()] if train_step.scheduler is not None else []
        if getattr(train_step, "avg", None) is not None:
            spec = train_step.weight_average
            ckpt["weight_average"] = {"kind": spec.kind, "decay": spec.decay, "warmup": spec.warmup, "start_step": spec.start_step,
                                      "every": spec.every, "n_averaged": int(train_step.n_averaged), "avg": train_step.avg.detach().cpu()}
        if getattr(train_step, "resolved_groups", None) is not None:
            ckpt["param_groups"] = train_step.resolved_groups.partition()
        if getattr(train_step, "guard", None) is not None:
            ckpt["step_guard"] = {"skipped": int(train_step.guard[2])}
    if epoch is not None:
        ckpt["epoch"] = int(epoch)
    tmp = path + ".tmp"
    torch.save(ckpt, tmp)
    os.replace(tmp, path)


def is_torch_optim_state(st) -> bool:
    """True for a torch.optim `state_dict()` (what Lightning writes into optimizer_states), False for the native flat layout."""
    return isinstance(st, dict) and "state" in st and "param_groups" in st and "name" not in st


def _scalar(x) -> float:
    return float(x.item()) if torch.is_tensor(x) else float(x)


def flat_state_from_torch_optim(osd: dict, shapes: Sequence, offsets: Sequence[int], numel: int, optimizer: str) -> dict:
    """Pure conversion of a torch.optim state dict into the flat layout of `trainer.FlatParams` (CPU tensors, nothing is modified).

    State index i belongs to the i-th parameter (`shapes[i]`, flat offset `offsets[i]`): the reference builds its optimizer from
    `self.model.parameters()` (modules.py:132-140) and the native modules register their parameters in the reference's order.
    Adam / AdamW (`exp_avg`, `exp_avg_sq`, `step`) fill m and v and give the single step count; Lion (lion_pytorch: `exp_avg` only)
    fills m.  The alignment padding between parameters stays zero.  Returns {"m", "v" (None for Lion), "step" (None for Lion), "lr",
    "betas", "eps" (None for Lion), "weight_decay"} from the state and `param_groups[0]`.  Raises ValueError for what one flat step
    count and one hyperparameter set cannot represent: a parameter count or shape mismatch (naming the first bad index), a
    parameter without state, unequal steps, amsgrad, more than one parameter group, or a state of another kind than `optimizer`."""
    if optimizer not in ("adamw", "adam", "lion"):
        raise ValueError(f"Optimizer {optimizer} not supported")
    groups = osd["param_groups"]
    if len(groups) != 1:
        raise ValueError(f"checkpoint optimizer has {len(groups)} parameter groups; the flat optimizer holds exactly one")
    pg = groups[0]
    ids = list(pg["params"])
    if len(ids) != len(shapes):
        raise ValueError(f"checkpoint optimizer holds {len(ids)} parameters, the model has {len(shapes)}")
    if ids != list(range(len(ids))):
        raise ValueError("checkpoint optimizer does not list its parameters as 0 .. n-1 in order")
    if pg.get("amsgrad", False):
        raise ValueError("checkpoint optimizer uses amsgrad=True, which the fused Adam / AdamW kernels do not implement")
    if pg.get("maximize", False):
        raise ValueError("checkpoint optimizer uses maximize=True, which the fused kernels do not implement")
    state = osd["state"]
    adam_like = any("exp_avg_sq" in state[i] for i in ids if i in state)
    kind = "adam" if adam_like else "lion"
    if (kind == "adam") != (optimizer in ("adamw", "adam")):
        raise ValueError(f"checkpoint holds a{'n Adam / AdamW' if adam_like else ' Lion'} optimizer state, the training step uses {optimizer!r}")
    decoupled = pg.get("decoupled_weight_decay")          # written by torch >= 2.6: True for AdamW, False for Adam
    if kind == "adam" and decoupled is not None and bool(decoupled) != (optimizer == "adamw"):
        raise ValueError(f"checkpoint holds a torch.optim.{'AdamW' if decoupled else 'Adam'} state, the training step uses {optimizer!r}")
    m = torch.zeros(numel, dtype=torch.float32)
    v = torch.zeros(numel, dtype=torch.float32) if kind == "adam" else None
    step = None
    for i, (shape, off) in enumerate(zip(shapes, offsets)):
        st = state.get(i)
        if st is None or "exp_avg" not in st:
            raise ValueError(f"checkpoint optimizer has no state for parameter {i}: one flat step count cannot represent it")
        if v is not None and ("exp_avg_sq" not in st or "step" not in st):
            raise ValueError(f"checkpoint optimizer state {i} lacks exp_avg_sq / step")
        n = math.prod(shape)
        if tuple(st["exp_avg"].shape) != tuple(shape) or (v is not None and tuple(st["exp_avg_sq"].shape) != tuple(shape)):
            raise ValueError(f"checkpoint optimizer state {i} has shape {tuple(st['exp_avg'].shape)}, parameter {i} is {tuple(shape)}")
        m[off:off + n] = st["exp_avg"].detach().reshape(-1).to(torch.float32)
        if v is not None:
            v[off:off + n] = st["exp_avg_sq"].detach().reshape(-1).to(torch.float32)
            s_i = _scalar(st["step"])
            if s_i != int(s_i) or s_i < 1:
                raise ValueError(f"checkpoint optimizer state {i} has step {s_i}")
            if step is None:
                step = int(s_i)
            elif int(s_i) != step:
                raise ValueError(f"checkpoint optimizer state {i} has step {int(s_i)}, state 0 has {step}: the flat optimizer keeps one step count")
    return {"m": m, "v": v, "step": step, "lr": float(pg["lr"]), "betas": tuple(float(b) for b in pg["betas"]),
            "eps": float(pg["eps"]) if "eps" in pg else None, "weight_decay": float(pg.get("weight_decay", 0.0))}


def _cfg_name(hp):
    """`hyper_parameters["optim_cfg"]["name"]` when present (a plain dict or an OmegaConf DictConfig), else None."""
    try:
        cfg = hp.get("optim_cfg") if hp is not None else None
        return None if cfg is None else cfg.get("name")
    except AttributeError:
        return None


def _load_reference_scheduler(sched, sd: dict) -> None:
    """Sets a native CosineWarmupLR from the state_dict() of the reference's CosineWarmupLR(SequentialLR) (utils/lr_schedulers.py:4-31):
    base lr, warm-up length (the milestone), max_iters and eta_min (the CosineAnnealingLR child) and the position (last_epoch)."""
    from .lr_schedulers import CosineWarmupLR
    if not isinstance(sched, CosineWarmupLR):
        raise ValueError(f"a reference CosineWarmupLR state can only be loaded into utils.lr_schedulers.CosineWarmupLR, not {type(sched).__name__}")
    kids = sd.get("_schedulers") or []
    if len(sd.get("_milestones", [])) != 1 or len(kids) != 2 or "T_max" not in kids[1]:
        raise ValueError("lr_schedulers[0] is not the state of the reference's CosineWarmupLR (LambdaLR warm-up, then CosineAnnealingLR)")
    sched.base_lrs = [float(b) for b in kids[1]["base_lrs"]]
    sched.base_lr = sched.base_lrs[0]
    sched.warmup_iters = int(sd["_milestones"][0])
    sched.max_iters = int(kids[1]["T_max"])
    sched.eta_min = float(kids[1]["eta_min"])
    sched.load_state_dict({"last_epoch": int(sd["last_epoch"])})


def _load_reference_optimizer(ckpt: dict, model: torch.nn.Module, train_step) -> None:
    name = _cfg_name(ckpt.get("hyper_parameters"))
    if name is not None and name != train_step.optimizer:
        raise ValueError(f"checkpoint was trained with optim_cfg {name!r}, the training step uses {train_step.optimizer!r}")
    flat = train_step.flat
    if len(flat.params) != len(list(model.parameters())):
        raise ValueError("the reference's optimizer holds every model parameter; this training step's flat buffer does not")
    got = flat_state_from_torch_optim(ckpt["optimizer_states"][0], [p.shape for p in flat.params], flat.offsets, flat.numel,
                                      train_step.optimizer)
    if getattr(train_step, "resolved_groups", None) is not None and got["weight_decay"] != train_step.wd:
        raise ValueError(f"the checkpoint's weight_decay {got['weight_decay']} would replace the training step's {train_step.wd}, from which its "
                         f"parameter-group tables were built: construct the TrainStep with weight_decay={got['weight_decay']}")
    if train_step.scheduler is None:
        train_step.lr = got["lr"]             # what Optimizer.load_state_dict leaves in the group when nothing schedules it
    elif ckpt.get("lr_schedulers"):
        _load_reference_scheduler(train_step.scheduler, ckpt["lr_schedulers"][0])
    train_step.m.copy_(got["m"])
    if train_step.v is not None:
        train_step.v.copy_(got["v"])
    train_step.step_no = got["step"] if got["step"] is not None else int(ckpt.get("global_step", 0))
    train_step.betas, train_step.wd = got["betas"], got["weight_decay"]
    if got["eps"] is not None:
        train_step.eps = got["eps"]


def load_checkpoint(path: str, model: torch.nn.Module, train_step=None, map_location="cpu") -> dict:
    """Loads the weights (into `model`, in place, so a FlatParams re-homing stays valid) and, if given, the training-step state.

    The training-step state is either the native flat layout (save_checkpoint) or the reference's Lightning layout: a torch.optim
    state dict in optimizer_states[0] (flat_state_from_torch_optim) and a CosineWarmupLR(SequentialLR) state in lr_schedulers[0].
    A reference state brings its hyperparameters along, as Optimizer.load_state_dict does under a Lightning resume: betas, eps and
    weight_decay of param_groups[0] become the training step's, and a native CosineWarmupLR takes the reference schedule's base lr,
    warm-up, max_iters, eta_min and position.  Lightning's loop state ("loops") is not restored.  A training step that averages its weights
    takes "weight_average" (the flat average and its update count; a numel mismatch is a ValueError) or, from a file without it, starts
    its average from the loaded parameters with a count of 0; a step that does not average ignores the key.  A training step with parameter
    groups refuses (ValueError, before any weight is written) a file whose "param_groups" partition differs from its own -- the moments of a
    parameter that was frozen there are not the moments of one that trained; a file without the key loads as always, and a step without
    groups ignores it.  A training step with a guard takes "step_guard" -- its device record restarts live, out of any streak, with the file's
    count of skipped steps (0 from a file without the key); a step without a guard ignores the key.  The reference's multi-group torch.optim state stays refused (flat_state_from_torch_optim), and a grouped step refuses a
    reference state whose weight_decay is not its own (its default group's row was built from that).  Unpickling a real Lightning file
    whose hyper_parameters hold OmegaConf objects needs the `omegaconf` package (not a dependency of this project)."""
    ckpt = torch.load(path, map_location=map_location, weights_only=False)
    sd = from_reference_state_dict(ckpt["state_dict"])
    own = model.state_dict()
    missing = [k for k in own if k not in sd]
    unexpected = [k for k in sd if k not in own]
    if missing or unexpected:
        raise KeyError(f"checkpoint / model mismatch: missing {missing[:3]}..., unexpected {unexpected[:3]}...")
    reference = train_step is not None and bool(ckpt.get("optimizer_states")) and is_torch_optim_state(ckpt["optimizer_states"][0])
    averages = train_step is not None and getattr(train_step, "avg", None) is not None
    wa = ckpt.get("weight_average") if averages else None
    if wa is not None and wa["avg"].numel() != train_step.avg.numel():
        raise ValueError(f"checkpoint average holds {wa['avg'].numel()} elements, the training step's flat buffer {train_step.avg.numel()}")
    own_groups = getattr(train_step, "resolved_groups", None) if train_step is not None else None
    if own_groups is not None and ckpt.get("param_groups") is not None:
        from .param_groups import same_partition
        if not same_partition(ckpt["param_groups"], own_groups.partition()):
            raise ValueError("checkpoint was written with other parameter groups than the training step's: its (lr_scale, weight_decay, frozen) "
                             f"partition {[(g['name'], len(g['params'])) for g in ckpt['param_groups']]} differs from "
                             f"{[(n, len(m)) for n, m in zip(own_groups.names, own_groups.members)]}")
    if reference:
        _load_reference_optimizer(ckpt, model, train_step)          # refuses before any weight is written
    with torch.no_grad():
        for k, t in own.items():
            t.copy_(sd[k])
    if train_step is not None and ckpt.get("optimizer_states") and not reference:
        st = ckpt["optimizer_states"][0]
        if st["name"] != train_step.optimizer:
            raise ValueError(f"checkpoint optimizer {st['name']!r} != {train_step.optimizer!r}")
        train_step.step_no = int(st["step"])
        train_step.m.copy_(st["m"])
        if train_step.v is not None:
            train_step.v.copy_(st["v"])
        if train_step.scheduler is not None and ckpt.get("lr_schedulers"):
            train_step.scheduler.load_state_dict(ckpt["lr_schedulers"][0])
    if averages:
        if wa is not None:
            train_step.avg.copy_(wa["avg"])
            train_step.n_averaged = int(wa["n_averaged"])
        else:                                 # an older file, or the reference's: the average starts from the loaded weights
            train_step.avg.copy_(train_step.flat.flat)
            train_step.n_averaged = 0
    if train_step is not None and getattr(train_step, "guard", None) is not None:      # a file without the key: nothing skipped so far
        skipped = int((ckpt.get("step_guard") or {}).get("skipped", 0))
        train_step.guard.copy_(torch.tensor([1, 0, skipped, -1], dtype=torch.int32))
    from .. import ops
    ops._weights_changed()                    # prepared inference weights (ops.trunk_eval) are re-made from the loaded parameters
    if train_step is not None and hasattr(train_step, "sync_from_rank0"):
        train_step.sync_from_rank0()          # data parallel: every replica continues from rank 0's weights, moments and step count
    return ckpt
