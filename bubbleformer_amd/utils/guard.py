"""Skipping optimizer steps whose gradient is not finite, decided on the device.

One overflowing bf16 activation or one corrupt frame gives a gradient with an inf or a NaN in it, and a fused optimizer launch that is handed
such a gradient turns the master weights, the moments and the averaged copy to NaN at once.  With a guard the training step does what AMP's
``GradScaler`` does for a bf16 trainer: the step is not taken, training goes on, and the run says how often that happened and where.  The
decision is one int32 in device memory that the optimizer launch itself reads (csrc/optim_kernels.h: the GUARD bodies), written by
``bf_step_guard`` from the gradient norm the step computes anyway: the step keeps its property of never synchronising with the host.

* ``GuardSpec``  -- what ``TrainStep(step_guard=...)`` and ``fit(step_guard=...)`` take.
* ``GUARD_FIELDS`` / ``locate`` -- the layout of the device record, and the parameter a flat-buffer index belongs to (``TrainStep.diagnose``).
"""
import dataclasses
from typing import Optional, Sequence

# the device record of bf_step_guard: four int32
GUARD_FIELDS = ("live", "consecutive", "skipped", "last_skipped_step")


@dataclasses.dataclass(frozen=True)
class GuardSpec:
    """max_consecutive  ``fit`` reads the counters where it synchronises anyway, at the end of an epoch, and raises FloatingPointError (with
                     ``TrainStep.diagnose()``'s finding, before the epoch's checkpoint is written) when the run is then in a streak of at
                     least this many skipped steps: a single bad batch is skipped and forgotten, a run that has diverged stops.  None never
                     raises.  ``TrainStep`` itself only counts."""
    max_consecutive: Optional[int] = 16

    def __post_init__(self):
        m = self.max_consecutive
        if m is not None and (isinstance(m, bool) or not isinstance(m, int) or m < 1):
            raise ValueError(f"GuardSpec: max_consecutive {m!r} must be None or an integer >= 1")

    def tripped(self, consecutive: int) -> bool:
        """Whether a streak of ``consecutive`` skipped steps ends the run."""
        return self.max_consecutive is not None and int(consecutive) >= self.max_consecutive


def locate(index: int, names: Sequence[str], offsets: Sequence[int], numels: Sequence[int]) -> str:
    """The parameter that element ``index`` of a flat buffer belongs to: parameter i occupies [offsets[i], offsets[i] + numels[i]) and the
    alignment padding up to offsets[i + 1] follows it (trainer.FlatParams) -- its name, or "padding after <name>"."""
    if not names or index < offsets[0]:
        raise ValueError(f"locate: index {index} lies before the first parameter")
    i = max(j for j, o in enumerate(offsets) if o <= index)
    return names[i] if index < offsets[i] + numels[i] else f"padding after {names[i]}"
