"""NumPy restatement of the step guard's device record and of the non-finite scan (csrc/gradclip.hip: bf_step_guard, bf_nonfinite_scan),
written from include/bubbleformer_hip.h alone; the GPU tests compare the kernels against it exactly (everything here is an integer)."""
import numpy as np

FIELDS = ("live", "consecutive", "skipped", "last_skipped_step")
FRESH = (1, 0, 0, -1)            # the record a training step starts with

GN_NT, GN_MAX_SLABS, GN_MIN_SLAB_GROUPS = 256, 1024, 1024


def guard_update(record, norm, step):
    """The record after bf_step_guard(norm, step): live = isfinite(fp32(norm)); not live: consecutive and skipped grow by one and the step
    is recorded; live: the streak ends."""
    live, consecutive, skipped, last = (int(v) for v in record)
    with np.errstate(over="ignore"):
        live = int(np.isfinite(np.float32(norm)))
    if live:
        return (1, 0, skipped, last)
    return (0, consecutive + 1, skipped + 1, int(step))


def guard_run(norms, first_step=1, record=FRESH):
    """The records after each of a sequence of steps."""
    out = []
    for i, x in enumerate(norms):
        record = guard_update(record, x, first_step + i)
        out.append(record)
    return out


def slab_groups(n):
    """16-byte groups per slab of a buffer of n elements: bf_grad_norm's rule, which bf_nonfinite_scan shares."""
    G = n // 4
    per = max(GN_MIN_SLAB_GROUPS, -(-G // GN_MAX_SLABS))
    return -(-per // GN_NT) * GN_NT


def slabs(n):
    return max(1, -(-(n // 4) // slab_groups(n)))


def scan(x):
    """(index of the first inf / NaN or -1, how many there are)."""
    bad = np.flatnonzero(~np.isfinite(np.asarray(x, dtype=np.float32)))
    return (int(bad[0]) if bad.size else -1, int(bad.size))
