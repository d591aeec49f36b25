"""Seeded mirror and crop augmentation of the device clip gather (csrc/clip_store.hip: bf_clip_gather_augment).

Pool boiling is mirror-symmetric in x if ``velx`` changes sign, and a model trained at 192 x 192 can be trained on full-resolution windows of
a 512 x 512 simulation.  Both are an index map and a sign inside the gather's one launch.  The decision of a sample is a pure function of
(seed, sample id, draw), computed on the device: the same in any batch, at any world size and after a resume.

The definition, on the gather's OUTPUT grid ``Ho x Wo`` (after ``downsample_factor``), for a ``Hc x Wc`` window (the whole grid without a crop):

    (w0, w1, w2, w3) = Philox4x32-10(counter = {0xFFFFFFFF, sample id mod 2^32, draw mod 2^32, 0}, key = {low, high word of seed})
    mirrored  iff  w0 < thr,  thr = min(round(flip_p * 2^32), 2^32)         (0 never mirrors, 2^32 always does)
    x0 = (w1 * (Wo - Wc + 1)) >> 32
    y0 = (w2 * (Ho - Hc + 1)) >> 32  with crop_y = "random",  0 with crop_y = "bottom"  (the window keeps row 0, the heater row)
    out[c][t][y][x] = (s_c * raw(c, t, y0 + y, xs) - diff_c) / div_c,   xs = x0 + x, or x0 + Wc - 1 - x when mirrored
    s_c = -1 iff the sample is mirrored and the channel's field is in odd_fields

``bf_clip_noise`` draws from the same generator with counter word 0 = a group number < 2^29: under one seed the two never share a block.

* ``AugmentSpec``  -- what ``DeviceClipStore.gather(augment=...)`` and ``fit(augment=...)`` take.
* ``augment_plan`` -- the same draw on the host (numpy), for users who must undo an augmentation.
"""
import dataclasses
from typing import Optional, Tuple

import numpy as np

CROP_Y = ("bottom", "random")
_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def _philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """Philox4x32-10 (Random123's constants) on uint64 arrays that hold 32-bit words -> four such arrays."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(_MASK) for v in np.broadcast_arrays(c0, c1, c2, c3)]
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]                # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(_MASK), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(_MASK)]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c


def flip_threshold(flip_p: float) -> int:
    """min(round(flip_p * 2^32), 2^32): a sample is mirrored iff its word 0 lies below it."""
    return min(int(round(float(flip_p) * 2.0 ** 32)), 2 ** 32)


@dataclasses.dataclass(frozen=True)
class AugmentSpec:
    """Mirror and crop augmentation of gathered clips (``DeviceClipStore.gather(augment=...)``, ``fit(augment=...)``).

    flip_p      probability in [0, 1] that a sample is mirrored in x; the fields in ``odd_fields`` then change sign (on the stored value,
                before normalisation: the mirrored physical field).
    crop        None, or (Hc, Wc): a window of the gather's output grid, its origin drawn per sample.
    crop_y      "bottom": every window starts at output row 0, the heater row the heat-flux code reads; "random": y0 is drawn as x0 is.
    odd_fields  the fields that are odd under x -> -x; names the dataset does not have are ignored.
    seed        the generator's key, any int, taken modulo 2^64.  Every rank uses the same seed; ranks differ by their sample ids.

    Off (``active`` false: flip_p = 0 and no crop) the gather makes exactly the calls it makes without the argument."""
    flip_p: float = 0.0
    crop: Optional[Tuple[int, int]] = None
    crop_y: str = "bottom"
    odd_fields: Tuple[str, ...] = ("velx",)
    seed: int = 0
    eval: bool = dataclasses.field(default=False, repr=False)      # set by eval_view(): the deterministic companion

    def __post_init__(self):
        p = self.flip_p
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:      # a NaN fails the comparison
            raise ValueError(f"AugmentSpec: flip_p {p!r} must be a number in [0, 1]")
        crop = self.crop
        if crop is not None:
            if not isinstance(crop, (tuple, list)) or len(crop) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 for v in crop):
                raise ValueError(f"AugmentSpec: crop {crop!r} must be None or a pair of positive ints (Hc, Wc)")
            object.__setattr__(self, "crop", (int(crop[0]), int(crop[1])))
        if self.crop_y not in CROP_Y:
            raise ValueError(f"AugmentSpec: crop_y {self.crop_y!r} must be one of {CROP_Y}")
        odd = self.odd_fields
        if isinstance(odd, str) or not isinstance(odd, (tuple, list)) or not all(isinstance(n, str) for n in odd):
            raise ValueError(f"AugmentSpec: odd_fields {odd!r} must be a sequence of field names")
        if isinstance(self.seed, bool) or not isinstance(self.seed, int):
            raise ValueError(f"AugmentSpec: seed {self.seed!r} must be an integer")
        if not isinstance(self.eval, bool):
            raise ValueError(f"AugmentSpec: eval {self.eval!r} must be a bool")
        object.__setattr__(self, "flip_p", float(p))
        object.__setattr__(self, "odd_fields", tuple(odd))
        object.__setattr__(self, "seed", self.seed % 2 ** 64)

    @property
    def active(self) -> bool:
        return self.flip_p > 0.0 or self.crop is not None

    def eval_view(self) -> "AugmentSpec":
        """The deterministic companion for validation: never mirrored, the window centred in x (``x0 = (Wo - Wc) // 2``) at ``y0 = 0``."""
        return dataclasses.replace(self, flip_p=0.0, eval=True)

    def window(self, Ho: int, Wo: int) -> Tuple[int, int]:
        """(Hc, Wc) on a ``Ho x Wo`` output grid; a crop larger than the grid raises ValueError."""
        hc, wc = self.crop if self.crop is not None else (int(Ho), int(Wo))
        if hc > Ho or wc > Wo:
            raise ValueError(f"AugmentSpec: crop {(hc, wc)} is larger than the gather's output grid {(int(Ho), int(Wo))}")
        return hc, wc


def augment_plan(spec: AugmentSpec, sample_ids, draw: int, Ho: int, Wo: int):
    """The decisions ``gather(sample_ids, augment=spec, draw=draw)`` makes on a ``Ho x Wo`` output grid, on the host:
    ``(flip [B] bool, x0 [B] int64, y0 [B] int64)``.  Sample ids count modulo 2^32, as does ``draw``.  What a user needs to undo an
    augmentation: ``out[..., y, x]`` is output-grid pixel ``(y0 + y, x0 + x)``, or ``(y0 + y, x0 + Wc - 1 - x)`` with the odd fields
    negated where ``flip`` is set."""
    if not isinstance(spec, AugmentSpec):
        raise ValueError(f"augment_plan: spec {spec!r} must be an AugmentSpec")
    hc, wc = spec.window(Ho, Wo)
    ids = np.asarray(sample_ids, dtype=np.int64).reshape(-1).astype(np.uint64) & np.uint64(_MASK)
    if spec.eval:
        return np.zeros(ids.size, dtype=bool), np.full(ids.size, (int(Wo) - wc) // 2, dtype=np.int64), np.zeros(ids.size, dtype=np.int64)
    w = _philox4x32_10(np.uint64(_MASK), ids, np.uint64(int(draw) & _MASK), np.uint64(0), spec.seed & _MASK, spec.seed >> 32)
    flip = w[0] < np.uint64(flip_threshold(spec.flip_p))
    x0 = ((w[1] * np.uint64(int(Wo) - wc + 1)) >> np.uint64(32)).astype(np.int64)
    y0 = ((w[2] * np.uint64(int(Ho) - hc + 1)) >> np.uint64(32)).astype(np.int64) if spec.crop_y == "random" else np.zeros(ids.size, dtype=np.int64)
    return flip, x0, y0
