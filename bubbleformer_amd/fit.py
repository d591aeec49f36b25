"""The epoch loop the reference's `Trainer.fit(ForecastModule, ...)` runs (scripts/train.py:157-171, bubbleformer/modules.py:76-171),
driving the native training step from device-resident clips.

What is kept from the reference's run configuration:
  * one optimizer step per batch, `CosineWarmupLR` stepped per batch (``interval="step"``, modules.py:153-171) with
    ``max_iters = trainer.estimated_stepping_batches`` = max_epochs x batches per epoch (modules.py:63-68);
  * `Trainer`'s ``gradient_clip_val`` / ``gradient_clip_algorithm`` / ``accumulate_grad_batches`` (off by default, as there): with
    accumulation the optimizer and the schedule step once per group of k batches and on an epoch's last batch, so
    ``estimated_stepping_batches`` = max_epochs x ceil(batches per epoch / k);
  * ``limit_train_batches`` / ``limit_val_batches`` (train.py:167-168: 1000 / 25): an epoch is at most that many batches of a
    freshly shuffled pass over the dataset; validation runs after every epoch, unshuffled, no sanity pass (train.py:169);
  * the last, partial batch is kept (DataLoader's ``drop_last=False``);
  * a checkpoint in the Lightning layout after every epoch (utils/checkpoint.py), from which a run resumes at the next epoch;
  * seeding: the shuffle of epoch e on every rank is ``randperm`` under ``seed + e`` and rank r takes ``[r::world]`` of it after
    padding to a multiple of the world size -- `torch.utils.data.DistributedSampler`, which Lightning injects under DDP
    (SURVEY.md section 8e); default seed 42 (config/default.yaml:2).
Logging back-ends (CSV / wandb), SLURM pre-emption and the model summary are the reference's control plane and are not rebuilt;
`log` receives one dict per step / validation instead.
"""
import math
from typing import Callable, Dict, List, Optional

import torch

from .trainer import TrainStep, accumulation_plan
from .utils.checkpoint import load_checkpoint, save_checkpoint
from .utils.lr_schedulers import CosineWarmupLR


def epoch_indices(n: int, epoch: int, seed: int = 42, shuffle: bool = True, rank: int = 0, world: int = 1) -> List[int]:
    """Sample order of one rank for one epoch (DistributedSampler semantics, drop_last=False)."""
    if shuffle:
        g = torch.Generator()
        g.manual_seed(seed + epoch)
        order = torch.randperm(n, generator=g).tolist()
    else:
        order = list(range(n))
    if world > 1:
        total = math.ceil(n / world) * world
        order = (order + order[:total - n])[:total] if n > 0 else order
        order = order[rank:total:world]
    return order


def batches(order: List[int], batch_size: int, limit: Optional[int]) -> List[List[int]]:
    out = [order[i:i + batch_size] for i in range(0, len(order), batch_size)]
    return out if limit is None else out[:int(limit)]


def fit(model: torch.nn.Module, train_set, val_set=None, *, batch_size: int, max_epochs: int, optimizer: str = "lion", lr: float = 5e-5,
        weight_decay: float = 0.1, warmup_iters: Optional[int] = 1000, eta_min: float = 1e-6, limit_train_batches: Optional[int] = 1000,
        limit_val_batches: Optional[int] = 25, seed: int = 42, rank: int = 0, world: int = 1, checkpoint_path: Optional[str] = None,
        resume_from: Optional[str] = None, hyper_parameters: Optional[dict] = None, log: Optional[Callable[[Dict], None]] = None,
        criterion: Optional[Callable] = None, gradient_clip_val: Optional[float] = None, gradient_clip_algorithm: str = "norm",
        accumulate_grad_batches: int = 1, panel_dir: Optional[str] = None, unroll_steps: int = 1, unroll_weights=None,
        unroll_backprop: bool = True, input_noise=None, weight_average=None, param_groups=None, augment=None, train_storage: str = "fp32",
        step_guard=None) -> Dict:
    """Trains `model` (a bubbleformer_amd model on the GPU) on `train_set` (data.BubbleForecast, already normalised).  Defaults are the
    reference's: Lion lr 5e-5 wd 0.1 (config/optim_cfg/lion.yaml), cosine schedule with 1000 warm-up steps to 1e-6
    (config/scheduler_cfg/cosine_warmup.yaml).  ``optimizer="adamw"`` / ``"adam"`` are the reference's other choices
    (config/optim_cfg/adamw.yaml: lr 2.5e-4 wd 1e-2; adam.yaml: lr 2.5e-4 wd 1e-5).  ``resume_from`` takes a file written here or by
    the reference's Lightning run (utils/checkpoint.py: load_checkpoint).  ``warmup_iters=None`` runs at a constant learning rate.  ``criterion``: None = the
    model's fused relative-L2 loss; or a callable (prediction, target) -> scalar tensor that training and validation both use (TrainStep).
    ``gradient_clip_val`` / ``gradient_clip_algorithm`` / ``accumulate_grad_batches``: see TrainStep.  The history and `log` keep one
    loss and one learning rate per batch; with clipping by norm, ``hist["grad_norm"]`` holds the (unclipped) gradient norm of every
    optimizer step, read from the device at the end of the epoch like the losses, and the `log` dict of a batch that stepped carries
    it as a device scalar.  ``panel_dir``: after every validation, the picture strips ForecastModule.on_validation_epoch_end logs
    (modules.py:191-250) of sample 0 of validation batch 0 as ``epoch_<e>_{sdf,temp,vel}_{target,pred}.png`` (utils/plot_utils.py; a field the
    dataset does not output is skipped); None renders and writes nothing.
    ``unroll_steps = k > 1`` / ``unroll_weights`` / ``unroll_backprop``: every training batch is a step unrolled through k of the model's
    own predictions (TrainStep): an epoch then shuffles ``train_set.unrollable(k)`` -- the samples whose k target clips lie in their own
    file -- under the same seeding and rank split, the clips come from ``gather(idx, unroll=k)``, ``train_loss`` is the weighted sum and
    ``hist["unroll_loss"]`` keeps the k per-pass losses of every batch.  Validation stays the single-step criterion; checkpoints and
    resume are unchanged.  The training set's input and output fields must be the same list (ValueError, as plan_rollouts refuses it).
    ``input_noise``: a utils.noise.NoiseSpec -- seeded Gaussian noise on the clips the model is fed while training (TrainStep): every batch's
    dataset indices are its sample ids (staged as ``gather`` stages them: a device tensor costs no synchronisation), the draw is the
    optimizer-step count, so a resumed run continues the sequence and the checkpoint needs no new key; ``relative=True`` is resolved once
    from the training store (``DeviceClipStore.field_std()`` of the input fields).  Every rank uses the same seed and ranks differ by
    their sample ids; a sample that occurs twice inside one optimizer step (DistributedSampler padding, accumulation over a tiny set)
    gets the same noise both times.  Validation is never perturbed.  None: history and parameters are bit for bit those without it.
    ``weight_average``: a utils.averaging.AverageSpec -- the training step keeps an EMA / SWA copy of the weights inside its optimizer kernel
    (TrainStep).  With a validation set every epoch then validates twice: ``hist["val_loss"]`` (and the panels) stay the live weights,
    ``hist["val_loss_avg"]`` is the same validation inside ``step.averaged_weights()``, and `log` gets ``val_loss_avg`` beside ``val_loss``.
    Checkpoints carry the average and a resumed run continues it (utils/checkpoint.py).  None: nothing of this runs.
    ``param_groups``: a list of utils.param_groups.GroupSpec -- frozen parameters, per-group learning-rate scale and weight decay inside the
    one optimizer launch (TrainStep; the scale multiplies the scheduled learning rate).  With clipping by norm ``hist["group_grad_norm"]``
    holds one row per optimizer step with the scaled gradient norm of every group, recorded as ``grad_norm`` is, and the `log` dict of a
    batch that stepped carries the row as a device tensor.  Checkpoints record the partition, and resuming into another one is refused.
    ``augment``: a utils.augment.AugmentSpec -- every training batch is gathered with a seeded mirror in x and / or a seeded window per sample,
    inside the gather's one launch (``DeviceClipStore.gather(idx, augment=..., draw=step.step_no)``): the decision of a sample is a pure
    function of (seed, dataset index, optimizer-step count), so a resumed run continues the sequence and the checkpoint needs no new key;
    every rank uses the same seed and ranks differ by their sample ids.  With a crop the model trains on ``Hc x Wc`` windows and validation
    sees ``augment.eval_view()`` -- never mirrored, the window centred in x on the heater row -- so its clips have the training shape;
    without a crop validation is gathered plainly.  Panels show what validation saw.  Composes with ``unroll_steps``, ``input_noise``,
    accumulation and conditioning; None or an inactive spec: every call, history and parameter bit for bit as without it.
    ``train_storage``: the form the TRAINING set is held in on the device, handed to ``train_set.device_store(dev, storage=...)``: "fp32", or
    "q16" -- 16-bit codes decoded inside the gather's launch, half the resident bytes, every clip within the store's bound of the original
    (data.Q16ClipStore); the training losses are bit for bit those of training on the decoded frames.  The validation store stays fp32:
    validation losses are against exact targets.  ``hist["train_storage"]`` and the checkpoint's hyper-parameters record the value.
    ``step_guard``: a utils.guard.GuardSpec -- an optimizer step whose gradient is not finite is skipped on the device (TrainStep).
    ``hist["skipped"]`` holds one 0 / 1 per optimizer step, kept as ``grad_norm`` is (a device scalar cloned per step, read at the end of the
    epoch), ``hist["guard_norm"]`` the guard's own gradient norm of every optimizer step where there is no clipping by norm, and the `log`
    dict of a batch that stepped carries ``live`` (1 = taken) as a device scalar.  ``epoch_train_loss`` is then the mean over the batches
    whose loss is finite.  Where the epoch synchronises anyway fit reads the counters, and raises FloatingPointError carrying
    ``step.diagnose()`` when the run ends the epoch in a streak of ``max_consecutive`` or more skipped steps -- before validation and before
    the checkpoint is written, so no file is written during such a streak.  Checkpoints carry the count of skipped steps and a resumed
    run continues it.  None: every call, history key and parameter bit for bit as without it.
    A criterion with a ``field_terms()`` method (utils.losses.InterfaceLpLoss): ``hist["field_loss"]`` keeps the C per-field terms of every
    training batch (of its last pass where the step is unrolled), kept as ``grad_norm`` is -- device clones, read at the end of the epoch -- and
    the `log` dict of a batch carries them as a device tensor.
    Returns the history."""
    dev = next(model.parameters()).device
    conditioned = getattr(train_set, "return_fluid_params", False)
    k = int(unroll_steps)
    if k > 1 and list(train_set.input_fields) != list(train_set.output_fields):
        raise ValueError(f"an unrolled step feeds predictions back as inputs: input fields {list(train_set.input_fields)} and output fields "
                         f"{list(train_set.output_fields)} must be the same")
    pool = train_set.unrollable(k) if k > 1 else None      # the samples an epoch draws from; None = all of them, as range(len)
    if pool is not None and not pool:
        raise ValueError(f"unroll_steps = {k}: no sample of the training set has {k} target clips inside its own file")
    n_pool = len(train_set) if pool is None else len(pool)
    per_epoch = len(batches(epoch_indices(n_pool, 0, seed, True, rank, world), batch_size, limit_train_batches))
    store = train_set.device_store(dev, storage=train_storage)
    vstore = val_set.device_store(dev) if val_set is not None else None
    steps_per_epoch = accumulation_plan(per_epoch, accumulate_grad_batches)[1]
    sched = CosineWarmupLR(lr, warmup_iters, max_epochs * steps_per_epoch, eta_min) if warmup_iters is not None else None
    noisy = input_noise is not None and input_noise.active
    if augment is not None:
        from .utils.augment import AugmentSpec
        if not isinstance(augment, AugmentSpec):
            raise ValueError(f"augment {augment!r} must be None or a utils.augment.AugmentSpec")
        if not augment.active:
            augment = None
    val_view = augment.eval_view() if augment is not None and augment.crop is not None else None
    field_std = None
    if noisy and input_noise.relative:
        fs = store.field_std()
        field_std = [fs[n] for n in train_set.input_fields]
    step = TrainStep(model, lr=lr, weight_decay=weight_decay, optimizer=optimizer, scheduler=sched, criterion=criterion,
                     gradient_clip_val=gradient_clip_val, gradient_clip_algorithm=gradient_clip_algorithm,
                     accumulate_grad_batches=accumulate_grad_batches, unroll_steps=unroll_steps, unroll_weights=unroll_weights,
                     unroll_backprop=unroll_backprop, input_noise=input_noise, field_std=field_std, weight_average=weight_average,
                     param_groups=param_groups, step_guard=step_guard)
    norm = (train_set.diff_terms, train_set.div_terms)
    hist: Dict[str, list] = {"train_loss": [], "lr": [], "val_loss": [], "epoch_train_loss": [], "train_storage": store.storage}
    if step.grad_norm is not None:
        hist["grad_norm"] = []
    if step.group_grad_norm is not None:
        hist["group_grad_norm"] = []
    if k > 1:
        hist["unroll_loss"] = []
    if step.guard is not None:
        hist["skipped"] = []
        if step.guard_norm is not None:
            hist["guard_norm"] = []
    if step.avg is not None and vstore is not None:
        hist["val_loss_avg"] = []
    field_terms = getattr(criterion, "field_terms", None)
    if field_terms is not None:
        hist["field_loss"] = []
    first_epoch = 0
    if resume_from is not None:
        ck = load_checkpoint(resume_from, model, step)
        # an epoch-less file (written by an older version, or by save_checkpoint outside fit) resumes at the epoch its step count implies
        first_epoch = int(ck["epoch"]) + 1 if "epoch" in ck else int(ck.get("global_step", 0)) // max(steps_per_epoch, 1)
    for epoch in range(first_epoch, max_epochs):
        model.train()
        losses, norms, gnorms, per_pass, lives, wnorms, fterms = [], [], [], [], [], [], []
        order = epoch_indices(n_pool, epoch, seed, True, rank, world)
        todo = batches(order if pool is None else [pool[i] for i in order], batch_size, limit_train_batches)
        for bi, idx in enumerate(todo):
            if augment is None:
                got = store.gather(idx) if k == 1 else store.gather(idx, unroll=k)
            else:
                got = store.gather(idx, unroll=k if k > 1 else None, augment=augment, draw=step.step_no)
            x, y, c = (got[0], got[1], got[2]) if conditioned else (got[0], got[1], None)
            cur_lr = sched.get_last_lr()[0] if sched is not None else step.lr      # step.lr: a reference checkpoint brings its own
            before = step.step_no
            loss = step(x, c, y, sample_ids=idx) if noisy else step(x, c, y)
            if bi == len(todo) - 1:
                step.finish_accumulation()      # an epoch's last batch completes its group, whatever the group holds
            losses.append(loss)
            if k > 1:
                per_pass.append(step.unroll_losses)
            hist["lr"].append(cur_lr)
            entry = {"epoch": epoch, "batch_idx": bi, "global_step": step.step_no, "train_loss": loss, "learning_rate": cur_lr}
            if field_terms is not None:
                fterms.append(field_terms())                 # a clone of what the batch's (last) forward left on the device
                entry["field_loss"] = fterms[-1]
            if step.grad_norm is not None and step.step_no != before:
                norms.append(step.grad_norm[0].clone())      # the next step overwrites the pair
                entry["grad_norm"] = norms[-1]
                if step.group_grad_norm is not None:
                    gnorms.append(step.group_grad_norm.clone())
                    entry["group_grad_norm"] = gnorms[-1]
            if step.guard is not None and step.step_no != before:
                lives.append(step.guard[0].clone())          # the next step overwrites the record
                entry["live"] = lives[-1]
                if step.guard_norm is not None:
                    wnorms.append(step.guard_norm[0].clone())
            if log is not None:
                log(entry)
        ep = torch.stack(losses).float()
        hist["train_loss"].extend(ep.tolist())
        if norms:
            hist["grad_norm"].extend(torch.stack(norms).tolist())
        if gnorms:
            hist["group_grad_norm"].extend(torch.stack(gnorms).tolist())
        if fterms:
            hist["field_loss"].extend(torch.stack(fterms).tolist())
        if per_pass:
            hist["unroll_loss"].extend(torch.stack(per_pass).tolist())
        if lives:
            hist["skipped"].extend((1 - torch.stack(lives)).tolist())
        if wnorms:
            hist["guard_norm"].extend(torch.stack(wnorms).tolist())
        hist["epoch_train_loss"].append(float(ep.mean() if step.guard is None else ep[torch.isfinite(ep)].mean()))
        if step.guard is not None:
            counts = step.guard_counts()
            if step_guard.tripped(counts["consecutive"]):
                raise FloatingPointError(f"epoch {epoch} ends in a streak of {counts['consecutive']} skipped optimizer steps ({counts['skipped']} "
                                         f"skipped in all, the last at step {counts['last_skipped_step']}): {step.diagnose()}")
        if vstore is not None:
            sample = [] if panel_dir is not None and rank == 0 else None
            hist["val_loss"].append(validate(model, val_set, vstore, batch_size, limit_val_batches, rank, world, criterion, sample, val_view))
            if sample:
                write_validation_strips(panel_dir, epoch, list(val_set.output_fields), *sample)
            entry = {"epoch": epoch, "val_loss": hist["val_loss"][-1]}
            if step.avg is not None:
                with step.averaged_weights():
                    hist["val_loss_avg"].append(validate(model, val_set, vstore, batch_size, limit_val_batches, rank, world, criterion, augment=val_view))
                entry["val_loss_avg"] = hist["val_loss_avg"][-1]
            if log is not None:
                log(entry)
        if checkpoint_path is not None and rank == 0:
            save_checkpoint(checkpoint_path, model, dict(hyper_parameters or {}, train_storage=store.storage), norm, step, epoch=epoch)       # one atomic write
    return hist


@torch.no_grad()
def validate(model, val_set, vstore, batch_size: int, limit_val_batches: Optional[int], rank: int = 0, world: int = 1, criterion=None,
             sample: Optional[list] = None, augment=None) -> float:
    """Mean over the (limited) validation batches of the training criterion, as `validation_step` logs it on epoch end.  A list passed as
    ``sample`` receives (target, prediction) of sample 0 of batch 0, (T, C, H, W) each (`validation_sample` of modules.py:185-189).
    ``augment``: the view the clips are gathered in (fit passes ``AugmentSpec.eval_view()`` of a spec with a crop); None gathers plainly."""
    was_training = model.training
    model.eval()
    conditioned = getattr(val_set, "return_fluid_params", False)
    tot, n = 0.0, 0
    for idx in batches(epoch_indices(len(val_set), 0, 0, False, rank, world), batch_size, limit_val_batches):
        got = vstore.gather(idx) if augment is None else vstore.gather(idx, augment=augment)
        if criterion is None:
            loss, pred = model.forward_loss(got[0], got[2], got[1]) if conditioned else model.forward_loss(got[0], got[1])
        else:
            pred = model(got[0], got[2]) if conditioned else model(got[0])
            loss = criterion(pred, got[1])
        if sample is not None and n == 0:
            sample.extend((got[1][0].detach().float().clone(), pred[0].detach().float().clone()))
        tot += float(loss)
        n += 1
    model.train(was_training)
    return tot / max(n, 1)


def write_validation_strips(panel_dir: str, epoch: int, fields: List[str], target: torch.Tensor, pred: torch.Tensor) -> List[str]:
    """The six strips of one validation sample (T, C, H, W): each field that is among ``fields`` as target and as prediction, every strip
    scaled to its own data as the reference's plotters are.  Returns the files written."""
    import os
    from .utils import plot_utils as P
    os.makedirs(panel_dir, exist_ok=True)
    spec = P.RenderSpec()
    T, _, H, W = target.shape
    layout = spec.layout(H, W, 1, T)
    written = []
    for name, title, needs, strip in (("sdf", "SDF", ("dfun",), P.sdf_strip), ("temp", "TEMP", ("temperature",), P.temp_strip),
                                      ("vel", "VEL", ("velx", "vely"), P.vel_strip)):
        if any(n not in fields for n in needs):
            continue                                  # the reference's `except ValueError: pass`
        idx = [fields.index(n) for n in needs]
        for side, clip in (("target", target), ("pred", pred)):
            frames = clip[:, idx] if len(idx) == 2 else clip[:, idx[0]]
            written.append(os.path.join(panel_dir, f"epoch_{epoch}_{name}_{side}.png"))
            P.write_strip(written[-1], strip(frames, spec=spec), title, layout)
    return written
