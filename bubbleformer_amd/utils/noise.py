"""Seeded Gaussian input noise for the training step (csrc/noise.hip: bf_clip_noise).

The other standard trick against rollout drift besides unrolling: the model is trained on perturbed inputs -- the gathered clip, and the
predictions an unrolled step feeds back -- so that their imperfection at evaluation time is something training has seen.  The noise comes
from a counter-based generator: what is added to element e of sample s at optimizer step n in pass p is a pure function of
(seed, s, n, p, e).  No generator state, no dependence on the launch geometry or on the batch a sample travels in: a resumed run, a run at
another world size and a batch with one sample swapped all train on the same noise for the samples they share.

* ``add_gaussian_noise`` -- one launch on a batch of clips.
* ``NoiseSpec``          -- what ``TrainStep(input_noise=...)`` and ``fit(input_noise=...)`` take.
"""
import dataclasses
import math
from typing import List, Optional, Sequence, Tuple, Union

import torch

PASSES = ("all", "input", "fed_back")


def _sigma_tensor(sigma, channels: int, device) -> torch.Tensor:
    if isinstance(sigma, torch.Tensor):
        if sigma.device != device or sigma.dtype != torch.float32 or tuple(sigma.shape) != (channels,):
            raise ValueError(f"add_gaussian_noise: a sigma tensor must be fp32 of shape ({channels},) on {device}")
        return sigma.contiguous()
    vals = [float(sigma)] * channels if isinstance(sigma, (int, float)) else [float(v) for v in sigma]
    if len(vals) != channels:
        raise ValueError(f"add_gaussian_noise: {len(vals)} sigmas for {channels} channels")
    if not all(math.isfinite(v) and v >= 0.0 for v in vals):
        raise ValueError(f"add_gaussian_noise: sigma {vals} must be finite and >= 0")
    return torch.tensor(vals, dtype=torch.float32, device=device)


def stage_sample_ids(sample_ids, batch: int, device) -> Optional[torch.Tensor]:
    """Sample ids as the kernel reads them: an int64 device tensor of ``batch`` entries (None stays None: the kernel then uses the row
    number).  A device tensor is used where it lies; host ids travel through pinned memory without a synchronisation, as
    ``DeviceClipStore.gather`` stages its indices."""
    if sample_ids is None:
        return None
    if isinstance(sample_ids, torch.Tensor) and sample_ids.device == device:
        ids = sample_ids.to(torch.int64).contiguous()
    else:
        host = sample_ids.to(torch.int64).cpu() if isinstance(sample_ids, torch.Tensor) else torch.tensor([int(i) for i in sample_ids], dtype=torch.int64)
        ids = host.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else host
    if ids.numel() != batch:
        raise ValueError(f"sample_ids: {ids.numel()} ids for a batch of {batch}")
    return ids.view(batch)


def add_gaussian_noise(clip: torch.Tensor, sigma, sample_ids=None, draw: int = 0, pass_index: int = 0, seed: int = 0,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``clip + sigma[c] * z`` on a contiguous fp32 device clip (B, T, C, H, W), in one launch.  ``sigma``: a float, one float per channel,
    or an fp32 device tensor of C entries; a channel with sigma 0 is returned bit for bit.  z is standard normal (Box-Muller on
    Philox4x32-10 words, |z| <= 5.77) and a pure function of ``(seed, sample_ids[b], draw, pass_index, element index inside the sample)``:
    row b of a batch is the one-sample call with that sample's id, two calls give the same bits.  ``sample_ids``: None (row b has id b), a
    sequence of ints or an integer tensor (a device tensor costs no host work); ids count modulo 2^32, ``draw`` / ``pass_index`` modulo
    2^32, ``seed`` modulo 2^64.  ``out=clip`` works in place; ``out=None`` returns a new tensor.  There is no CPU path."""
    from .. import _lib as L
    from .. import ops
    if not isinstance(clip, torch.Tensor) or not clip.is_cuda:
        where = f"a tensor on {clip.device}" if isinstance(clip, torch.Tensor) else type(clip).__name__
        raise L.BubbleformerHipError(f"add_gaussian_noise runs only on a ROCm GPU (gfx950): got {where}; there is no CPU fallback")
    if clip.dim() != 5:
        raise ValueError(f"add_gaussian_noise: the clip must be (B, T, C, H, W), got {tuple(clip.shape)}")
    return ops.clip_noise(clip, _sigma_tensor(sigma, clip.shape[2], clip.device), stage_sample_ids(sample_ids, clip.shape[0], clip.device),
                          draw, pass_index, seed, out)


@dataclasses.dataclass(frozen=True)
class NoiseSpec:
    """Gaussian noise on what the model is fed during training (``TrainStep(input_noise=...)``, ``fit(input_noise=...)``).

    std       a float >= 0, or one per input field, in the units the model sees (after normalisation).  All zero means off: the step
              then launches what it launches without the argument.
    relative  multiply ``std`` by each input field's standard deviation over the training store, in those same units
              (``DeviceClipStore.field_std()``): ``fit`` resolves it; a ``TrainStep`` built by hand takes ``field_std=``.
    seed      the generator's key.  Under data parallelism every rank uses the same seed; ranks differ because their sample ids differ.
    passes    which passes of a step are perturbed: "input" -- the gathered clip only (pass 0); "fed_back" -- the predictions an unrolled
              step feeds back (passes >= 1) only; "all" -- both.  Targets are never perturbed.

    The noise of element e of sample s at optimizer step n in pass p is a pure function of (seed, s, n, p, e) (``add_gaussian_noise``),
    n being the optimizer steps completed so far: a resumed run continues the sequence.  A known limit: two occurrences of one sample
    inside one optimizer step (``DistributedSampler`` padding, or gradient accumulation over a tiny set) get the same noise."""
    std: Union[float, Tuple[float, ...]]
    relative: bool = False
    seed: int = 0
    passes: str = "all"

    def __post_init__(self):
        std = self.std
        if isinstance(std, bool) or not isinstance(std, (int, float, list, tuple)):
            raise ValueError(f"NoiseSpec: std {std!r} must be a number >= 0 or a sequence of them, one per input field")
        vals = [std] if isinstance(std, (int, float)) else list(std)
        if not vals or any(isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0 for v in vals):
            raise ValueError(f"NoiseSpec: std {std!r} must be finite and >= 0 (one number, or one per input field)")
        if not isinstance(self.relative, bool):
            raise ValueError(f"NoiseSpec: relative {self.relative!r} must be a bool")
        if isinstance(self.seed, bool) or not isinstance(self.seed, int):
            raise ValueError(f"NoiseSpec: seed {self.seed!r} must be an integer")
        if self.passes not in PASSES:
            raise ValueError(f"NoiseSpec: passes {self.passes!r} must be one of {PASSES}")
        object.__setattr__(self, "std", float(std) if isinstance(std, (int, float)) else tuple(float(v) for v in std))

    @property
    def active(self) -> bool:
        return any(v > 0.0 for v in ([self.std] if isinstance(self.std, float) else self.std))

    def perturbs(self, pass_index: int) -> bool:
        """Whether pass ``pass_index`` of a step (0 = the gathered clip) is fed a perturbed input."""
        if not self.active:
            return False
        return self.passes == "all" or (self.passes == "input") == (pass_index == 0)

    def sigma(self, channels: int, field_std: Optional[Sequence[float]] = None) -> List[float]:
        """The per-channel standard deviations for a clip of ``channels`` input fields; ``relative`` needs ``field_std`` (one per field)."""
        vals = [self.std] * channels if isinstance(self.std, float) else list(self.std)
        if len(vals) != channels:
            raise ValueError(f"NoiseSpec: {len(vals)} standard deviations for {channels} input fields")
        if self.relative:
            if field_std is None:
                raise ValueError("NoiseSpec(relative=True) needs the fields' standard deviations: train through fit(), or pass field_std= to TrainStep")
            fs = [float(v) for v in field_std]
            if len(fs) != channels or not all(math.isfinite(v) and v >= 0.0 for v in fs):
                raise ValueError(f"NoiseSpec: field_std {fs} must be {channels} finite numbers >= 0")
            vals = [v * f for v, f in zip(vals, fs)]
        return vals
