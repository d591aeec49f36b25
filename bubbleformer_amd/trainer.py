"""Data-parallel training step for the native FiLMAViT path.

* ``FlatParams``   -- re-homes every parameter (and its gradient) of a module into ONE fp32 buffer each, in
                      registration order, so the optimizer is a single fused kernel (csrc/optim_kernels.h: adamw_kernel)
                      and gradient buckets are contiguous slices.
* ``BucketReducer``-- the data-parallel exchange (reference: Lightning's ``strategy="ddp"``, scripts/train.py:158-172):
                      mean all-reduce of gradient buckets over ``torch.distributed`` (backend "nccl" = RCCL over xGMI),
                      issued per bucket as soon as backward has produced every gradient in it (debed first, then
                      blocks N-1 .. 0, then embed), overlapped with the rest of backward.  One process per GPU.
* ``TrainStep``    -- forward (+ fused relative-L2 loss, or a caller's criterion on the prediction) -> backward -> bucket wait ->
                      [gradient norm and clip coefficient, on the device] -> fused AdamW / Adam / Lion; with
                      ``accumulate_grad_batches=k`` the exchange and the optimizer run on every k-th call only; with
                      ``unroll_steps=k`` the model is run through k of its own predictions with a loss on each (``unroll_plan``);
                      with ``weight_average=`` the optimizer kernel also keeps an averaged copy of the weights (EMA / SWA);
                      with ``param_groups=`` it freezes parameters and gives groups their own learning-rate scale and weight decay;
                      with ``step_guard=`` a step whose gradient is not finite is skipped, by a flag the optimizer launch reads on the device.
Device agnostic where it can be (the reducer and the flat views are tested on CPU with gloo); the model itself
only runs on the GPU.
"""
from typing import List, Optional, Sequence, Tuple

import contextlib
import inspect
import math
import os

import torch
import torch.distributed as dist
import torch.nn as nn

from ._lib import BF_OPT_CHUNK


class FlatParams:
    def __init__(self, module: nn.Module, align: int = BF_OPT_CHUNK):
        """align: every parameter starts on a multiple of it.  The default is the optimizers' chunk (one parameter-group id per chunk,
        utils/param_groups.py); a step with param_groups needs a multiple of it."""
        params = [p for p in module.parameters() if p.requires_grad]
        self.params = params
        offs, n = [], 0
        for p in params:
            offs.append(n)
            n += (p.numel() + align - 1) // align * align
        dev = params[0].device
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.offsets, self.numel = offs, n
        for p, o in zip(params, offs):
            v = self.flat[o:o + p.numel()].view(p.shape)
            v.copy_(p.data)
            p.data = v
            p.grad = self.grad[o:o + p.numel()].view(p.shape)

    def zero_grad(self):
        self.grad.zero_()


class BucketReducer:
    """Mean all-reduce of contiguous slices of a flat gradient buffer, launched from post-accumulate hooks."""

    def __init__(self, flat: FlatParams, bucket_of: Sequence[int], group=None, use_hooks: bool = True, bucket_dtype=None):
        """use_hooks=False: buckets are completed by stage_ready() only (TrainStep's direct-gradient mode -- autograd runs the
        post-accumulate hooks even for the ``None`` gradients that mode returns, which would count every bucket twice).
        bucket_dtype=torch.bfloat16 (or BF_GRAD_BUCKET_DTYPE=bf16): a bucket travels as a bf16 copy -- half the bytes per xGMI link
        (57.8 MB instead of 115.6 MB per step for FiLMAViT-small) for one cast each way; the sum of `world`
        bf16-rounded addends carries a relative error of ~2^-9 per element, the master gradients and the optimizer stay fp32."""
        self.flat, self.group = flat, group
        if bucket_dtype is None and os.environ.get("BF_GRAD_BUCKET_DTYPE", "").lower() in ("bf16", "bfloat16"):
            bucket_dtype = torch.bfloat16
        self.bucket_dtype = bucket_dtype
        self.launch_log = []      # bucket ids in launch order (this step); tests assert the reverse-forward order and one collective per bucket
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        nb = max(bucket_of) + 1
        self.lo = [None] * nb
        self.hi = [None] * nb
        self.count = [0] * nb
        for p, o, b in zip(flat.params, flat.offsets, bucket_of):
            self.lo[b] = o if self.lo[b] is None else min(self.lo[b], o)
            self.hi[b] = o + p.numel() if self.hi[b] is None else max(self.hi[b], o + p.numel())
            self.count[b] += 1
        self.pending = [0] * nb
        self.handles = []
        self.held = None          # direct-gradient mode: a complete bucket waits until the NEXT one is complete (see stage_ready)
        self.enabled = self.world > 1
        self.sync = True          # False inside no_sync(): gradients accumulate locally, nothing is counted, launched or held
        self.done = set()         # buckets reduced in this step
        if self.enabled and use_hooks:
            for p, b in zip(flat.params, bucket_of):
                p.register_post_accumulate_grad_hook(self._make_hook(b))

        self.bucket_of_ptr = {p.data_ptr(): b for p, b in zip(flat.params, bucket_of)}

    def _launch(self, b):
        self.done.add(b)
        self.launch_log.append(b)
        g = self.flat.grad[self.lo[b]:self.hi[b]]
        if self.bucket_dtype is not None and self.bucket_dtype != g.dtype:
            buf = g.to(self.bucket_dtype)
            self.handles.append((dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group, async_op=True), g, buf))
        else:
            self.handles.append((dist.all_reduce(g, op=dist.ReduceOp.SUM, group=self.group, async_op=True), None, None))

    @contextlib.contextmanager
    def no_sync(self):
        """A backward under this context launches no collective (DistributedDataParallel.no_sync, which Lightning enters on the
        micro-batches of ``accumulate_grad_batches`` that do not step): its gradients stay in the flat buffer, and the next backward
        outside the context reduces the sum."""
        was, self.sync = self.sync, False
        try:
            yield
        finally:
            self.sync = was

    def _arrived(self, b, hold=False):
        if not self.sync:
            return
        self.pending[b] += 1
        if self.pending[b] == self.count[b]:
            self.pending[b] = 0
            if self.enabled:
                if self.held is not None:
                    self._launch(self.held)
                    self.held = None
                if hold:
                    self.held = b
                else:
                    self._launch(b)

    def _make_hook(self, b):
        def hook(_p):
            self._arrived(b)
        return hook

    def stage_ready(self, ptrs):
        """Direct-gradient mode: the stage's kernels (accumulating into the flat buffer) are enqueued on the current stream --
        except possibly its last weight-gradient GEMM, which the library joins inside the next stage call (bf_side_defer).  A
        complete bucket is therefore reduced when the next bucket completes, the last one in flush() after bf_side_join()."""
        for ptr in ptrs:
            self._arrived(self.bucket_of_ptr[ptr], hold=True)

    def flush(self):
        if self.held is not None:
            self._launch(self.held)
            self.held = None

    def wait(self) -> float:
        """Block the current stream on the outstanding buckets; returns the factor the optimizer must apply (1/world)."""
        self.flush()
        if self.enabled:          # buckets nobody completed (a stage that fell back to autograd accumulation, unused parameters):
            for b in range(len(self.count)):      # the backward is over, so they are final; same order on every rank
                if b not in self.done and self.lo[b] is not None:
                    self._launch(b)
        for h, g, buf in self.handles:
            h.wait()
            if buf is not None:
                g.copy_(buf)
        self.handles.clear()
        self.done.clear()
        self.pending = [0] * len(self.pending)
        return 1.0 / self.world

    def begin_step(self):
        self.launch_log = []


def stage_buckets(model: nn.Module, blocks_per_bucket: Optional[int] = None) -> List[int]:
    """Bucket index per parameter: one bucket per top-level stage and per group of `blocks_per_bucket` consecutive processor blocks
    (gradient-ready order is the reverse of this list).  Each bucket is one collective: fewer, larger ones cost less host time
    and fewer stream synchronisations, more of them start the exchange earlier: a bucket is launched one bucket late (see
    BucketReducer.stage_ready), so at the end of the backward two buckets are still travelling.  BF_BLOCKS_PER_BUCKET, default 2
    (19 MB of fp32 gradients per collective for FiLMAViT-small)."""
    if blocks_per_bucket is None:
        blocks_per_bucket = int(os.environ.get("BF_BLOCKS_PER_BUCKET", "2"))
    ids, names = [], {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        parts = name.split(".")
        key = "blocks.%d" % (int(parts[1]) // max(1, blocks_per_bucket)) if parts[0] == "blocks" else parts[0]
        ids.append(names.setdefault(key, len(names)))
    return ids


def accumulation_plan(per_epoch: int, k: int) -> Tuple[List[int], int]:
    """(batch indices of an epoch of `per_epoch` batches after which the optimizer steps under ``accumulate_grad_batches=k``, their number):
    every k-th batch, and the epoch's last batch whatever the group holds -- ceil(per_epoch / k) steps per epoch, which is what
    Lightning's ``estimated_stepping_batches`` counts."""
    if per_epoch < 0 or k < 1:
        raise ValueError(f"accumulation_plan: per_epoch {per_epoch} must be >= 0 and accumulate_grad_batches {k} >= 1")
    steps = [i for i in range(per_epoch) if (i + 1) % k == 0 or i == per_epoch - 1]
    assert len(steps) == -(-per_epoch // k)
    return steps, len(steps)


def unroll_weights_checked(k: int, weights=None) -> List[float]:
    """The per-pass loss weights of a step unrolled through k passes: 1/k each by default; given ones must be k finite numbers >= 0, not all 0."""
    if int(k) != k or k < 1:
        raise ValueError(f"unroll_steps {k!r} must be an integer >= 1")
    k = int(k)
    if weights is None:
        return [1.0 / k] * k
    w = [float(v) for v in weights]
    if len(w) != k:
        raise ValueError(f"unroll_weights: {len(w)} weights for unroll_steps = {k}")
    if not all(math.isfinite(v) and v >= 0.0 for v in w) or not any(v > 0.0 for v in w):
        raise ValueError(f"unroll_weights {w} must be finite and >= 0, and not all 0")
    return w


def unroll_plan(k: int, weights=None, backprop: bool = True, final: bool = True) -> Tuple[List[float], List[Tuple[str, int, bool]]]:
    """The schedule of one training step unrolled through k passes, x_1 = x, x_{j+1} = pred_j, loss = sum_j w_j loss_j (passes are numbered
    from 0 here): -> (weights, [(op, pass, flag), ...] in execution order) with
      ("forward", j, grad)  -- pass j's forward; grad False = under no_grad, no backward follows;
      ("backward", j, sync) -- pass j's backward; sync False = inside BucketReducer.no_sync().
    Every pass runs forward once, in order (its loss is reported whatever its weight).
      * backprop=True: gradients flow through the fed-back predictions.  Pass j takes gradients when some pass i >= j has w_i > 0 (it is
        then on the path of that loss); all forwards run first, then the backwards from the last such pass down to pass 0 -- pass j's gets
        w_j for its loss (when > 0) and the gradient its prediction collected as the input of pass j + 1.
      * backprop=False (the pushforward form): the fed-back prediction is detached; pass j takes gradients when w_j > 0 and its backward
        runs right after its forward, so one pass's activations are alive at a time.
    Only the backward that runs LAST synchronises, and only when ``final`` (the micro-batch completes its accumulate_grad_batches group):
    every bucket is then exchanged once per optimizer step, after all k passes have added to it."""
    w = unroll_weights_checked(k, weights)
    k = len(w)
    if backprop:
        last = max(j for j in range(k) if w[j] > 0.0)
        grad = [j <= last for j in range(k)]
        plan = [("forward", j, grad[j]) for j in range(k)] + [("backward", j, False) for j in range(last, -1, -1)]
    else:
        plan = []
        for j in range(k):
            plan.append(("forward", j, w[j] > 0.0))
            if w[j] > 0.0:
                plan.append(("backward", j, False))
    if final:
        i = max(i for i, (op, _, _) in enumerate(plan) if op == "backward")
        plan[i] = ("backward", plan[i][1], True)
    return w, plan


class TrainStep:
    """optimizer: "adamw" (config/optim_cfg/adamw.yaml; modules.py:135-136), "adam" (config/optim_cfg/adam.yaml, torch.optim.Adam
    with its L2 weight decay; modules.py:137-138) or "lion" (config/optim_cfg/lion.yaml, the reference default; modules.py:139-140).
    The constructor's weight_decay default is AdamW's; pass adam.yaml's 1e-5 / lion.yaml's 0.1 explicitly.  scheduler: optional
    object with get_last_lr() / step() (utils.lr_schedulers.CosineWarmupLR), stepped once per optimizer step like the reference's
    ``interval="step"`` (modules.py:166-171).  criterion: None = the model's fused forward_loss (relative L2 as configured at
    modules.py:50); or a callable (prediction, target) -> scalar tensor, e.g. utils.losses.LpLoss(...) plus a physics penalty: the step
    then runs model(x[, fluid]), the criterion and loss.backward() through the same gradient slots and bucket reducer.
    gradient_clip_val / gradient_clip_algorithm / accumulate_grad_batches: Lightning's `Trainer` arguments of those names.
      * "norm": the averaged gradient (after the bucket exchange, so identical on every rank) is scaled by
        min(gradient_clip_val / (its 2-norm + 1e-6), 1) -- torch.nn.utils.clip_grad_norm_.  Norm and coefficient are computed on the
        device into ``self.grad_norm`` (two fp32: {norm, coef} of the last optimizer step) and the optimizer kernel reads the coefficient
        from there: no host synchronisation.  "value": every element is clamped to +-gradient_clip_val (clip_grad_value_).
        None (or 0) = off: the step launches what it launched without these arguments.
      * accumulate_grad_batches = k: a call that does not complete a group of k only adds its gradient to the flat buffer (no
        zero_grad, no collective -- BucketReducer.no_sync -- no optimizer, no scheduler step); the completing call exchanges the
        buckets, applies 1/(world*k) and steps once.  ``step_no`` counts optimizer steps.  finish_accumulation() steps on a partial
        group with the same factor, as Lightning does on an epoch's last batch.
    unroll_steps = k > 1: the step runs the model through k of its own predictions, x_1 = x, x_{j+1} = pred_j, with a loss on each against
    ``target[j]`` -- ``target`` is (k, B, T, C, H, W) (DeviceClipStore.gather(idx, unroll=k)) or a sequence of k clips -- and optimises
    sum_j w_j loss_j (``unroll_weights``, default 1/k each), which is also what the call returns; ``unroll_losses`` keeps the k losses of
    the last call on the device.  ``unroll_backprop=True`` sends gradients through the fed-back predictions: every pass has its own graph
    (x_{j+1} = pred_j.detach().requires_grad_()), the backwards run from pass k down to pass 1, and pass j's gets its loss weight and the
    gradient x_{j+1} collected TOGETHER -- with the fused loss that is the third source mode of the debed backward (dpred + w_j * dloss
    formed in registers), so all k passes' activations are alive at the turn.  ``False`` is the pushforward form: predictions are fed
    back detached and each pass's backward follows its forward (one pass's activations alive; a pass with w_j = 0 runs under no_grad).
    Stochastic depth is drawn per pass.  Every backward but the last runs inside BucketReducer.no_sync() (unroll_plan).  The input and
    output fields must be the same (ValueError); a model whose forward_loss cannot keep its prediction in the graph (the U-Nets) is
    refused with NotImplementedError unless a criterion is given.  unroll_steps = 1 is the step it always was.
    input_noise = utils.noise.NoiseSpec: seeded Gaussian noise on what the model is fed (one bf_clip_noise launch per perturbed pass).  The
    gathered clip is pass 0; with unroll_steps = k the input of pass j + 1 is pred_j + noise(pass = j + 1), built from pred_j.detach() and, with
    unroll_backprop, marked requires_grad: the gradient it collects is handed to pred_j unchanged (the addition's Jacobian is the identity).
    The noisy clip is always a new tensor: the caller's x and the prediction a fused-loss backward has saved are never written; targets are
    never perturbed.  The noise of element e of sample s is a pure function of (spec.seed, s, step_no at the time of the call, pass, e);
    s comes from ``sample_ids`` of the call (the batch's dataset indices; None numbers the rows 0 .. B - 1), step_no counts optimizer steps
    and is in every checkpoint, so a resumed run continues the sequence.  Every micro-batch of an accumulate_grad_batches group draws
    under the same step_no: two occurrences of one sample inside one optimizer step get the same noise (NoiseSpec).  ``relative=True``
    needs ``field_std`` (one deviation per input field, DeviceClipStore.field_std(); fit resolves it).  None, or a spec whose std is all
    zero, is off: the step launches exactly what it launches without the argument.
    weight_average = utils.averaging.AverageSpec: an averaged copy of the flat parameter buffer, ``self.avg`` (fp32, 4 bytes per parameter),
    kept by the optimizer kernel itself -- ``spec.weight(step_no, n_averaged)`` is handed to the fused optimizer as ``avg_weight``, so an
    update costs one more read and write of one buffer and no launch; a step the schedule skips runs the plain kernel, and micro-batches
    that do not step never touch the average.  ``n_averaged`` counts the updates past ``start_step``.  The copy starts as the (rank 0)
    parameters; every rank then computes the same average from the same parameters, so the feature launches no collective.
    ``averaged_state_dict()`` exports it, ``averaged_weights()`` puts it behind the model's parameters for a ``with`` block (validation,
    evaluate_rollouts), checkpoints carry it (utils/checkpoint.py).  Module buffers (BatchNorm running statistics) are not averaged.
    None: no buffer, and the optimizer calls are the ones made without the argument.
    param_groups = a list of utils.param_groups.GroupSpec (its helpers no_weight_decay / layer_decay / freeze return such lists and compose by
    ``+``): the parameters are sorted into at most 64 groups of one (lr_scale, weight_decay, frozen) each (``resolved_groups``; group 0 is the
    default: scale 1, this step's weight_decay), and a one-byte group id per 64-element chunk of the flat buffer (``groups``: the map and the
    tables on the device, built once) selects them inside the same single optimizer launch.  The SCHEDULED learning rate is multiplied by the
    group's scale -- timm's ``lr_scale`` convention.  That is not torch's per-group CosineAnnealingLR, whose ``eta_min`` is absolute: here the
    floor of a group is eta_min * lr_scale.  A frozen parameter, its moments and its average are never read or written by the optimizer (the
    average stays bit-equal to the parameter); its gradient is still computed and, data parallel, exchanged.  Clipping by norm takes the norm
    over the parameters that are not frozen -- what clip_grad_norm_ sees of a torch optimizer's parameters -- from ops.group_sumsq +
    ops.group_clip_coef_ in place of ops.grad_norm_; ``grad_norm`` keeps its meaning ({norm, coef} of the last optimizer step), and
    ``group_grad_norm`` (fp32 [groups], on the device; clipping by norm only, None otherwise) holds the scaled gradient norm of every group,
    frozen ones included, of the last optimizer step.  Clipping by value, the averaged weights, accumulation, unrolling and input noise work
    as without groups; every rank builds the same tables from the same specs.  ``requires_grad=False`` is not a way to freeze here: such a
    parameter has no home in the flat buffers.  None: nothing is built and the optimizer calls are the ones made without the argument.
    utils.param_groups.group_norms(step) gives every group's parameter and gradient norm on demand.
    step_guard = utils.guard.GuardSpec: an optimizer step whose gradient holds an inf or a NaN is not taken -- parameters, moments and the
    averaged copy keep their bits -- and training goes on, as under AMP's GradScaler.  The decision is made on the device and read by the
    optimizer launch itself, so the step still never synchronises with the host.  After the bucket exchange (data parallel: every rank then
    holds the same gradient, so every rank decides alike with no further collective) the 2-norm of the gradient is the witness: its fp64 sum
    of squares is non-finite exactly when some element is (include/bubbleformer_hip.h: bf_step_guard; a finite gradient whose scaled norm
    exceeds fp32's 3.4e38 is skipped too).  With clipping by norm it is the norm the step computes anyway; otherwise (no clipping, or
    clipping by value) the step computes one for the guard alone, with max_norm = +inf, into ``guard_norm`` ({norm, coef} on the device,
    None with clipping by norm) -- the optimizer is not handed that coefficient and keeps the scale mode it has without the guard.  With
    param_groups the norm is the one over the groups that are not frozen: a NaN in a frozen parameter's gradient reaches nothing and does not
    skip the step.  One bf_step_guard launch then updates ``guard``, four int32 on the device {live, consecutive, skipped,
    last_skipped_step}, and the optimizer reads ``guard[0]``.  ``guard_counts()`` reads the counters (it synchronises); ``diagnose()`` finds
    the first non-finite element of the parameters or the gradient and names its parameter.  The host-side counters cannot know the
    device's decision without the synchronisation this exists to avoid, so they advance on a skipped step as on any other: ``step_no`` (hence
    Adam's bias correction and the noise / augmentation draw), the scheduler (the learning-rate schedule counts the skipped step) and
    ``n_averaged`` (an SWA mean stays a convex combination of the snapshots taken, but is no longer exactly uniform; the average starts as a
    copy of the parameters, so a skipped "copy" step leaves it finite).  Not protected: state a forward pass writes outside the flat buffers
    -- the one case is ClassicUnet's BatchNorm running statistics, which a non-finite activation reaches before any gradient exists.
    None: no buffer, no launch, and the optimizer calls are the ones made without the argument."""

    def __init__(self, model: nn.Module, lr: float = 2.5e-4, weight_decay: float = 1e-2, betas=None, eps: float = 1e-8,
                 optimizer: str = "adamw", scheduler=None, criterion=None, gradient_clip_val: Optional[float] = None,
                 gradient_clip_algorithm: str = "norm", accumulate_grad_batches: int = 1, unroll_steps: int = 1, unroll_weights=None,
                 unroll_backprop: bool = True, input_noise=None, field_std=None, weight_average=None, param_groups=None, step_guard=None):
        from . import ops
        from .utils.averaging import AverageSpec
        from .utils.guard import GuardSpec
        from .utils.noise import NoiseSpec
        if weight_average is not None and not isinstance(weight_average, AverageSpec):
            raise ValueError(f"weight_average {weight_average!r} must be None or a utils.averaging.AverageSpec")
        if input_noise is not None and not isinstance(input_noise, NoiseSpec):
            raise ValueError(f"input_noise {input_noise!r} must be None or a utils.noise.NoiseSpec")
        if step_guard is not None and not isinstance(step_guard, GuardSpec):
            raise ValueError(f"step_guard {step_guard!r} must be None or a utils.guard.GuardSpec")
        if input_noise is not None and input_noise.active and input_noise.relative and field_std is None:
            raise ValueError("input_noise: NoiseSpec(relative=True) needs the input fields' standard deviations -- train through fit(), which "
                             "takes them from the training store, or pass field_std= (DeviceClipStore.field_std())")
        self.input_noise = input_noise if input_noise is not None and input_noise.active else None
        self._noise_field_std = None if field_std is None else [float(v) for v in field_std]
        self._noise_sigma = None      # the per-channel deviations on the device, built at the first perturbed call
        if optimizer not in ("adamw", "adam", "lion"):
            raise ValueError(f"Optimizer {optimizer} not supported")
        if gradient_clip_algorithm not in ("norm", "value"):
            raise ValueError(f"gradient_clip_algorithm {gradient_clip_algorithm!r} not supported: 'norm' or 'value'")
        if gradient_clip_val is not None and not gradient_clip_val >= 0:
            raise ValueError(f"gradient_clip_val {gradient_clip_val!r} must be None or >= 0")
        if int(accumulate_grad_batches) != accumulate_grad_batches or accumulate_grad_batches < 1:
            raise ValueError(f"accumulate_grad_batches {accumulate_grad_batches!r} must be an integer >= 1")
        self.unroll_weights = unroll_weights_checked(unroll_steps, unroll_weights)
        self.unroll_steps = len(self.unroll_weights)
        self.unroll_backprop = bool(unroll_backprop)
        self.unroll_losses = None      # (k,) device tensor: the per-pass losses of the last call
        if self.unroll_steps > 1:
            fl = getattr(model, "forward_loss", None)
            if criterion is None and (fl is None or "pred_grad" not in inspect.signature(fl).parameters):
                raise NotImplementedError(f"unroll_steps = {self.unroll_steps}: {type(model).__name__}.forward_loss cannot feed its prediction back "
                                          "(no pred_grad: the U-Nets' fused loss is not unrolled); pass a criterion to unroll through model(x)")
        self.ops = ops
        self.model = model
        self.flat = FlatParams(model)
        self.reducer = BucketReducer(self.flat, stage_buckets(model), use_hooks=False)
        self.slots = {p.data_ptr(): p.grad for p in self.flat.params}
        self.optimizer = optimizer
        self.m = torch.zeros_like(self.flat.flat)
        self.v = torch.zeros_like(self.flat.flat) if optimizer in ("adamw", "adam") else None
        if betas is None:
            betas = (0.9, 0.999) if optimizer in ("adamw", "adam") else (0.9, 0.99)
        self.lr, self.wd, self.betas, self.eps = lr, weight_decay, betas, eps
        self.scheduler = scheduler
        self.criterion = criterion
        self.step_no = 0
        self.clip_val = float(gradient_clip_val) if gradient_clip_val else None      # Lightning: None and 0 both mean no clipping
        self.clip_algorithm = gradient_clip_algorithm
        self.accumulate_grad_batches = int(accumulate_grad_batches)
        self.micro = 0            # micro-batches whose gradient is pending in the flat buffer
        self.grad_norm = None     # "norm" clipping: device {norm, coef} of the last optimizer step
        if self.clip_val is not None and gradient_clip_algorithm == "norm":
            self.grad_norm = torch.zeros(2, dtype=torch.float32, device=self.flat.flat.device)
            self._coef = self.grad_norm[1:]
            self._norm_ws = None
        self.step_guard = step_guard
        self.guard = None         # step_guard: the device record {live, consecutive, skipped, last_skipped_step}
        self.guard_norm = None    # step_guard without "norm" clipping: device {norm, coef} of the last optimizer step, for the guard alone
        if step_guard is not None:
            self.guard = torch.tensor([1, 0, 0, -1], dtype=torch.int32, device=self.flat.flat.device)
            self._live = self.guard[:1]
            if self.grad_norm is None:
                self.guard_norm = torch.zeros(2, dtype=torch.float32, device=self.flat.flat.device)
                self._norm_ws = None
        self._unroll_w = None
        if self.unroll_steps > 1:
            self._unroll_w = torch.tensor(self.unroll_weights, dtype=torch.float32, device=self.flat.flat.device)
        self.resolved_groups = None    # utils.param_groups.ResolvedGroups of param_groups
        self.groups = None             # ops.ParamGroupTables: the chunk map and the group tables on the device
        self.group_grad_norm = None    # param_groups and "norm" clipping: the scaled gradient norm of every group, last optimizer step
        if param_groups is not None:
            self._build_groups(param_groups)
        self.weight_average = weight_average
        self.avg = None           # the averaged copy of flat.flat; taken below, from the parameters every rank starts with
        self.n_averaged = 0       # updates of the average past spec.start_step
        self._swapped = False     # inside averaged_weights(): flat.flat holds the average and avg the live weights
        self.sync_from_rank0()
        if weight_average is not None:
            self.avg = self.flat.flat.clone()

    def _build_groups(self, specs) -> None:
        from .utils.param_groups import CHUNK, resolve
        flat = self.flat
        if any(o % CHUNK for o in flat.offsets) or flat.numel % CHUNK:
            raise ValueError(f"param_groups: the flat buffer must start every parameter on a multiple of {CHUNK} elements")
        self.resolved_groups = res = resolve(self.model, list(specs), self.wd)
        name_of = {id(p): n for n, p in self.model.named_parameters()}
        cmap = res.chunk_map([name_of[id(p)] for p in flat.params], flat.offsets, flat.numel)
        self.groups = self.ops.param_group_tables(cmap, [t[0] for t in res.table], [t[1] for t in res.table], [t[2] for t in res.table],
                                                  flat.numel, flat.flat.device)
        if self.grad_norm is not None:
            self.group_grad_norm = torch.zeros(len(res), dtype=torch.float32, device=flat.flat.device)
        if self.grad_norm is not None or self.guard is not None:
            self._group_sums = torch.zeros(len(res), dtype=torch.float64, device=flat.flat.device)

    @staticmethod
    def _check_unroll_fields(cin: int, cout: int) -> None:
        if int(cin) != int(cout):
            raise ValueError(f"an unrolled step feeds predictions back as inputs: input fields ({int(cin)}) and output fields ({int(cout)}) "
                             "must be the same")

    def sync_from_rank0(self) -> None:
        """Data parallel: every replica starts (and resumes) from rank 0's parameters, optimizer moments and step count -- what
        `DistributedDataParallel` does at construction under Lightning's strategy="ddp" (scripts/train.py:158-172).  Only gradients are
        averaged afterwards, so a rank built from another seed would otherwise diverge silently."""
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        avg = getattr(self, "avg", None)      # the averaged weights and their update count travel too, once the step holds them
        for t in (self.flat.flat, self.m, self.v, avg, getattr(self, "guard", None)):      # ... and the guard's counters
            if t is not None:
                dist.broadcast(t, src=0)
        n = torch.tensor([self.step_no] + ([self.n_averaged] if avg is not None else []), dtype=torch.int64, device=self.flat.flat.device)
        dist.broadcast(n, src=0)
        self.step_no = int(n[0])
        if avg is not None:
            self.n_averaged = int(n[1])
        from . import ops
        ops._weights_changed()           # the broadcast wrote the flat buffer behind the parameters' version counters: prepared inference weights are stale

    def _noise_ids(self, x, sample_ids):
        """The sample ids of a call as the noise kernel reads them (staged once per call, no synchronisation); None when noise is off."""
        if self.input_noise is None:
            return None
        from .utils.noise import stage_sample_ids
        return stage_sample_ids(sample_ids, x.shape[0], x.device)

    def _noisy(self, clip, pass_index: int, ids):
        """``clip`` as pass ``pass_index`` is fed it: the clip itself where the spec leaves that pass alone, otherwise a NEW tensor
        clip + sigma * z(seed, sample, step_no, pass) -- ``clip`` is never written."""
        spec = self.input_noise
        if spec is None or not spec.perturbs(pass_index):
            return clip
        if self._noise_sigma is None or self._noise_sigma.device != clip.device or self._noise_sigma.numel() != clip.shape[2]:
            self._noise_sigma = torch.tensor(spec.sigma(clip.shape[2], self._noise_field_std), dtype=torch.float32, device=clip.device)
        return self.ops.clip_noise(clip.detach().contiguous(), self._noise_sigma, ids, self.step_no, pass_index, spec.seed)

    def __call__(self, x, fluid, target, sample_ids=None) -> torch.Tensor:
        self._refuse_while_swapped("a training step")
        final = self.micro + 1 >= self.accumulate_grad_batches
        ids = self._noise_ids(x, sample_ids)
        if self.micro == 0:
            self.flat.zero_grad()
        self.reducer.begin_step()
        self.ops.set_direct_grad_slots(self.slots, self.reducer.stage_ready, self.reducer.flush)
        self.ops.set_side_defer(True)       # a stage's weight-gradient GEMMs may run into the next stage; joined below
        try:
            with contextlib.nullcontext() if final else self.reducer.no_sync():
                if self.unroll_steps == 1:
                    loss = self._fwd_bwd(self._noisy(x, 0, ids), fluid, target)
                else:
                    loss = self._fwd_bwd_unrolled(x, fluid, target, final, ids)
        finally:
            self.ops.set_side_defer(False)
            self.ops.set_direct_grad_slots(None)
        self.micro += 1
        if final:
            self._optimizer_step()
        return loss.detach()

    def finish_accumulation(self) -> bool:
        """Step on the gradient of a partial group (an epoch's last batches), with the full group's 1/(world*k); nothing to do when no
        gradient is pending.  The pending micro-batches ran without collectives, so every bucket is exchanged here.  -> stepped or not"""
        self._refuse_while_swapped("finish_accumulation()")
        if self.micro == 0:
            return False
        self.reducer.begin_step()
        self._optimizer_step()
        return True

    def _optimizer_step(self) -> None:
        gscale = self.reducer.wait() / self.accumulate_grad_batches
        self.micro = 0
        self.step_no += 1
        lr = self.scheduler.get_last_lr()[0] if self.scheduler is not None else self.lr
        clip = {}
        if self.grad_norm is not None and self.groups is not None:      # the norm over the groups that are not frozen
            if self._norm_ws is None:
                self._norm_ws = self.ops.group_sumsq_workspace(self.flat.numel, self.flat.grad.device)
            self.ops.group_sumsq(self.flat.grad, self.groups, self._group_sums, self._norm_ws)
            self.ops.group_clip_coef_(self._group_sums, self.groups, self.grad_norm, self.clip_val, gscale, self.group_grad_norm)
            clip = {"coef": self._coef}
        elif self.grad_norm is not None:
            if self._norm_ws is None:
                self._norm_ws = self.ops.grad_norm_workspace(self.flat.numel, self.flat.grad.device)
            self.ops.grad_norm_(self.flat.grad, self.grad_norm, self.clip_val, gscale, self._norm_ws)
            clip = {"coef": self._coef}
        elif self.clip_val is not None:
            clip = {"clip_value": self.clip_val}
        if self.guard is not None:
            witness = self.grad_norm
            if witness is None:                  # no norm clipping: a norm for the guard alone; its coefficient is not handed on
                witness = self._guard_witness(gscale)
            self.ops.step_guard_(witness[:1], self.guard, self.step_no)
            clip["live"] = self._live
        if self.weight_average is not None:
            w = self.weight_average.weight(self.step_no, self.n_averaged)
            if w is not None:
                clip.update(avg=self.avg, avg_weight=w)
                if self.weight_average.counts(self.step_no):
                    self.n_averaged += 1
        if self.groups is not None:
            clip["groups"] = self.groups
        if self.optimizer == "adamw":
            self.ops.adamw_(self.flat.flat, self.flat.grad, self.m, self.v, self.step_no, lr, self.betas, self.eps, self.wd, gscale, **clip)
        elif self.optimizer == "adam":
            self.ops.adam_(self.flat.flat, self.flat.grad, self.m, self.v, self.step_no, lr, self.betas, self.eps, self.wd, gscale, **clip)
        else:
            self.ops.lion_(self.flat.flat, self.flat.grad, self.m, lr, self.betas, self.wd, gscale, **clip)
        if self.scheduler is not None:
            self.scheduler.step()

    # ---------------------------------------------------------------------------------------- the step guard
    def _guard_witness(self, gscale: float) -> torch.Tensor:
        """{norm, coef} of the exchanged gradient into ``guard_norm``, as clipping by norm with max_norm = +inf would form them (over the
        groups that are not frozen, with param_groups)."""
        inf = float("inf")
        if self.groups is not None:
            if self._norm_ws is None:
                self._norm_ws = self.ops.group_sumsq_workspace(self.flat.numel, self.flat.grad.device)
            self.ops.group_sumsq(self.flat.grad, self.groups, self._group_sums, self._norm_ws)
            return self.ops.group_clip_coef_(self._group_sums, self.groups, self.guard_norm, inf, gscale)
        if self._norm_ws is None:
            self._norm_ws = self.ops.grad_norm_workspace(self.flat.numel, self.flat.grad.device)
        return self.ops.grad_norm_(self.flat.grad, self.guard_norm, inf, gscale, self._norm_ws)

    def guard_counts(self) -> dict:
        """{"skipped", "consecutive", "last_skipped_step"} of the device record: optimizer steps skipped so far, the length of the streak
        the run is in (0 after a step that was taken) and the ``step_no`` of the last skipped step (-1: none).  This copies the record to
        the host and so SYNCHRONISES with the device: call it where the run waits anyway (fit does at the end of an epoch)."""
        if self.guard is None:
            raise RuntimeError("guard_counts(): this TrainStep has no guard (step_guard=None)")
        live, consecutive, skipped, last = self.guard.tolist()
        return {"skipped": skipped, "consecutive": consecutive, "last_skipped_step": last}

    def diagnose(self) -> dict:
        """Where the first non-finite value is: ops.nonfinite_scan over the parameters first, then over the gradient buffer (which holds
        the last call's gradient until the next call clears it).  -> {"buffer": "parameters" | "gradient" | None, "parameter": the name
        of the parameter the element belongs to, or "padding after <name>" (None when nothing was found), "index": its place in the flat
        buffer (-1), "count": how many non-finite elements that buffer holds (0)}.  A diagnostic for after something has gone wrong: two
        launches per buffer and a synchronisation, never part of a step; it needs no guard."""
        from .utils.guard import locate
        name_of = {id(p): n for n, p in self.model.named_parameters()}
        for what, buf in (("parameters", self.flat.flat), ("gradient", self.flat.grad)):
            first, count = self.ops.nonfinite_scan(buf).tolist()
            if count:
                where = locate(first, [name_of[id(p)] for p in self.flat.params], self.flat.offsets, [p.numel() for p in self.flat.params])
                return {"buffer": what, "parameter": where, "index": first, "count": count}
        return {"buffer": None, "parameter": None, "index": -1, "count": 0}

    # ---------------------------------------------------------------------------------------- the averaged weights
    def _refuse_while_swapped(self, what: str) -> None:
        if self._swapped:
            raise RuntimeError(f"{what} inside averaged_weights(): the model's parameters are the averaged weights until the block ends")

    def _require_average(self, what: str) -> None:
        if self.avg is None:
            raise RuntimeError(f"{what}: this TrainStep keeps no average (weight_average=None)")

    def averaged_state_dict(self):
        """The averaged weights in the reference's ``state_dict`` layout ("model.<name>" keys, CPU clones; utils.checkpoint.
        to_reference_state_dict): every trained parameter is read from ``avg`` at its flat offset, everything else -- frozen parameters,
        module buffers such as BatchNorm running statistics -- is the live value."""
        from .utils.checkpoint import PREFIX, to_reference_state_dict
        self._require_average("averaged_state_dict()")
        sd = to_reference_state_dict(self.model)
        avg = self.flat.flat if self._swapped else self.avg
        at = {p.data_ptr(): o for p, o in zip(self.flat.params, self.flat.offsets)}
        for name, p in self.model.named_parameters():
            o = at.get(p.data_ptr())
            if o is not None and PREFIX + name in sd:
                sd[PREFIX + name] = avg[o:o + p.numel()].view(p.shape).detach().to("cpu", copy=True)
        return sd

    @contextlib.contextmanager
    def averaged_weights(self):
        """``with step.averaged_weights():`` -- inside, the model's parameters (views of the flat buffer) ARE the averaged weights: one
        exchange of ``flat`` and ``avg`` on entry (ops.swap_buffers_, which also marks the prepared inference weights stale) and one on
        exit, also when the block raises.  For validation, evaluate_rollouts and anything else that runs the model.  A training step,
        finish_accumulation() or a second averaged_weights() inside the block raises RuntimeError.  Module buffers are left alone: SWA of
        a model with BatchNorm normally recomputes the running statistics for the averaged weights afterwards, which is not done here."""
        self._require_average("averaged_weights()")
        self._refuse_while_swapped("averaged_weights()")
        self.ops.swap_buffers_(self.flat.flat, self.avg, parameters=True)
        self._swapped = True
        try:
            yield self.model
        finally:
            self.ops.swap_buffers_(self.flat.flat, self.avg, parameters=True)
            self._swapped = False

    def _fwd_bwd(self, x, fluid, target):
        if self.criterion is None:
            loss, _ = self.model.forward_loss(x, fluid, target) if fluid is not None else self.model.forward_loss(x, target)
        else:
            loss = self.criterion(self.model(x, fluid) if fluid is not None else self.model(x), target)
        loss.backward()
        return loss

    def _fwd_bwd_unrolled(self, x, fluid, target, final: bool, ids=None):
        """The schedule of unroll_plan: k forward passes through the model's own predictions, their backwards in the plan's order, all but
        the last inside no_sync().  Returns sum_j w_j loss_j; the k losses stay in ``unroll_losses``.  With input noise, pass j is fed
        _noisy(., j, ids): the gradient a noisy fed-back clip collects belongs to the prediction it was built from, unchanged."""
        k, w, backprop = self.unroll_steps, self.unroll_weights, self.unroll_backprop
        if isinstance(target, torch.Tensor):
            if target.dim() != x.dim() + 1 or target.shape[0] != k:
                raise ValueError(f"unroll_steps = {k}: target must be (k, B, T, C, H, W) or a sequence of k clips, got {tuple(target.shape)}")
        elif len(target) != k:
            raise ValueError(f"unroll_steps = {k}: {len(target)} target clips")
        self._check_unroll_fields(x.shape[2], target[0].shape[2])
        plan = unroll_plan(k, w, backprop, final)[1]
        takes_grad = {j: g for op, j, g in plan if op == "forward"}
        inputs, preds, losses = [self._noisy(x, 0, ids)] + [None] * (k - 1), [None] * k, [None] * k
        for op, j, flag in plan:
            if op == "forward":
                feeds = backprop and j + 1 < k and takes_grad[j + 1]        # the prediction carries a gradient back from pass j + 1
                with torch.enable_grad() if flag else torch.no_grad():
                    if self.criterion is None:
                        args = (inputs[j], fluid, target[j]) if fluid is not None else (inputs[j], target[j])
                        losses[j], pred = self.model.forward_loss(*args, pred_grad=feeds)
                    else:
                        pred = self.model(inputs[j], fluid) if fluid is not None else self.model(inputs[j])
                        losses[j] = self.criterion(pred, target[j])
                preds[j] = pred if feeds else None
                if not backprop:
                    inputs[j] = None                                        # pushforward: a fed-back clip is done with after its pass's forward
                if j + 1 < k:
                    fed = self._noisy(pred.detach(), j + 1, ids)
                    inputs[j + 1] = fed.requires_grad_() if feeds else fed
            else:
                outs, grads = [], []
                if w[j] > 0.0:
                    outs.append(losses[j])
                    grads.append(self._unroll_w[j])
                if preds[j] is not None and inputs[j + 1].grad is not None:
                    outs.append(preds[j])
                    grads.append(inputs[j + 1].grad)
                with contextlib.nullcontext() if flag else self.reducer.no_sync():
                    torch.autograd.backward(outs, grads)
                self.ops.release_deferred()                                 # the pass's saved activations are not held to the end of the step
                preds[j] = None                                             # this pass's graph and what it fed are done with
                if backprop and j + 1 < k:
                    inputs[j + 1] = None
                losses[j] = losses[j].detach()
        self.unroll_losses = torch.stack([l.detach().float() for l in losses])
        return (self.unroll_losses * self._unroll_w).sum()
