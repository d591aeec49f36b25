"""The definition of the clip gather's mirror / window draw, restated from the counter layout of include/bubbleformer_hip.h:
bf_clip_gather_augment -- one Philox4x32-10 block per sample, Python integers behind it.  Nothing of the package's or the device's code."""
import numpy as np

from tests import noise_restatement as NR

C0 = 0xFFFFFFFF            # word 0 of every augmentation counter; bf_clip_noise's is a group number < 2^29


def counters(sample_ids, draw):
    """The counter blocks {0xFFFFFFFF, sample id (low 32 bits), draw, 0} of a list of samples, as tuples of ints."""
    return [(C0, int(i) & NR.MASK, int(draw) & NR.MASK, 0) for i in sample_ids]


def decisions(seed, sample_ids, draw, flip_p, Ho, Wo, Hc, Wc, crop_y="bottom"):
    """-> (flip, x0, y0): lists of bool / int, one entry per sample id."""
    seed = int(seed) % 2 ** 64
    blocks = counters(sample_ids, draw)
    w = NR.philox4x32_10(tuple(np.array([b[k] for b in blocks], dtype=np.uint64) for k in range(4)), (seed & NR.MASK, seed >> 32))
    thr = min(round(flip_p * 2 ** 32), 2 ** 32)
    flip = [int(v) < thr for v in w[0]]
    x0 = [(int(v) * (Wo - Wc + 1)) >> 32 for v in w[1]]
    y0 = [(int(v) * (Ho - Hc + 1)) >> 32 if crop_y == "random" else 0 for v in w[2]]
    return flip, x0, y0
