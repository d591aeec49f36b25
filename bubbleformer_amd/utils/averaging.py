"""An averaged copy of the weights for the training step: an exponential moving average (EMA) or a uniform stochastic weight average (SWA).

The averaged weights are what one validates, evaluates rollouts on and releases: they are smoother than the weights the optimizer last
wrote.  The copy lives in ``TrainStep`` as one flat fp32 buffer beside the parameters and is updated inside the fused optimizer kernel
(csrc/optim_kernels.h: the AVG bodies), where the new parameter value is already in registers.  This module is the schedule alone -- pure
Python, no device: which optimizer steps update the average, and with what weight.

* ``AverageSpec`` -- what ``TrainStep(weight_average=...)`` and ``fit(weight_average=...)`` take.
"""
import dataclasses
from typing import Optional

KINDS = ("ema", "swa")


@dataclasses.dataclass(frozen=True)
class AverageSpec:
    """The update after optimizer step ``step_no`` is ``a <- a + w * (p - a)`` with ``w = weight(step_no, n_averaged)``.

    kind        "ema": w = 1 - decay.  "swa": w = 1 / (n_averaged + 1), the running mean of the weights averaged so far.
    decay       the EMA's decay, in [0, 1); unused by "swa".
    warmup      EMA only: the decay of update n is min(decay, (1 + n) / (10 + n)), so a young average is not held at its start.
    start_step  up to and including this optimizer step the average follows the weights (w = 1) and counts nothing.
    every       after start_step only every ``every``-th optimizer step updates the average; the others run the plain optimizer kernel.

    With ``start_step=1`` the EMA is ``torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay))`` updated after every
    step (its first update copies, the later ones lerp) and "swa" is ``AveragedModel``'s default running mean."""
    kind: str = "ema"
    decay: float = 0.999
    warmup: bool = False
    start_step: int = 0
    every: int = 1

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"AverageSpec: kind {self.kind!r} must be one of {KINDS}")
        if isinstance(self.decay, bool) or not isinstance(self.decay, (int, float)) or not 0.0 <= self.decay < 1.0:
            raise ValueError(f"AverageSpec: decay {self.decay!r} must be a number in [0, 1)")
        if isinstance(self.start_step, bool) or not isinstance(self.start_step, int) or self.start_step < 0:
            raise ValueError(f"AverageSpec: start_step {self.start_step!r} must be an integer >= 0")
        if isinstance(self.every, bool) or not isinstance(self.every, int) or self.every < 1:
            raise ValueError(f"AverageSpec: every {self.every!r} must be an integer >= 1")
        object.__setattr__(self, "decay", float(self.decay))
        object.__setattr__(self, "warmup", bool(self.warmup))

    def weight(self, step_no: int, n_averaged: int) -> Optional[float]:
        """The weight of the update applied after optimizer step ``step_no`` (1-based) when ``n_averaged`` updates have been counted:
        1.0 while the average follows the weights (n_averaged stays 0), None on a step that leaves the average alone, otherwise the
        EMA's 1 - decay or the running mean's 1 / (n_averaged + 1) -- after which the caller counts one more."""
        if step_no <= self.start_step:
            return 1.0
        if (step_no - self.start_step) % self.every != 0:
            return None
        if self.kind == "swa":
            return 1.0 / (n_averaged + 1)
        d = min(self.decay, (1.0 + n_averaged) / (10.0 + n_averaged)) if self.warmup else self.decay
        return 1.0 - d

    def counts(self, step_no: int) -> bool:
        """Whether an update after optimizer step ``step_no`` is counted in n_averaged (it is past start_step)."""
        return step_no > self.start_step
