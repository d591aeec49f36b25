"""The averaged-weights update and its schedule, restated in fp64 numpy / plain Python (no device, no bubbleformer_amd import): what
tests/test_weight_average.py and tests/test_gpu_weight_average.py hold the kernels, TrainStep and fit to.

The kernels compute, per element and in fp32, ``a' = p if w == 1 else fma(w, p - a, a)``: a subtraction rounded once and one fused
multiply-add rounded once.  ``lerp`` is that expression in fp64 on the fp32 inputs (w as the fp32 the kernel receives); ``lerp_bound`` is
the per-element bound two correctly rounded fp32 operations can miss it by."""
import numpy as np

EPS = 2.0 ** -24          # half an fp32 ulp, relative


def lerp(a_prev, p_new, w):
    """fp64 ``a + w * (p - a)`` on fp32 inputs; w == 1 gives p itself (the kernel copies)."""
    a = np.asarray(a_prev, dtype=np.float64)
    p = np.asarray(p_new, dtype=np.float64)
    w32 = float(np.float32(w))
    if w32 == 1.0:
        return p.copy()
    return a + w32 * (p - a)


def lerp_bound(a_prev, p_new, units: float = 4.0):
    """``units * 2^-24 * (|a_prev| + |p_new|)`` per element.  The rounded difference d = fl(p - a) is off by at most 2^-24 |p - a| <=
    2^-24 (|a| + |p|), which the product scales by w <= 1; the fma's one rounding adds at most 2^-24 |a'| with |a'| <= max(|a|, |p|) (a
    convex combination) plus what the first error moved it by -- under 3 units in all, and 4 leaves one to spare."""
    return units * EPS * (np.abs(np.asarray(a_prev, dtype=np.float64)) + np.abs(np.asarray(p_new, dtype=np.float64)))


def schedule_weight(kind, decay, warmup, start_step, every, step_no, n_averaged):
    """AverageSpec.weight restated: 1.0 up to start_step, None on a skipped step, else 1 - d (EMA) or 1 / (n + 1) (SWA)."""
    if step_no <= start_step:
        return 1.0
    if (step_no - start_step) % every != 0:
        return None
    if kind == "swa":
        return 1.0 / (n_averaged + 1)
    d = min(decay, (1.0 + n_averaged) / (10.0 + n_averaged)) if warmup else decay
    return 1.0 - d


def replay(snapshots, kind="ema", decay=0.999, warmup=False, start_step=0, every=1, first=None):
    """The average after each optimizer step, from the parameter snapshots taken after steps 1, 2, ...: -> (list of fp64 averages, one
    per step, each carried forward in fp64 from the PREVIOUS fp64 average, n_averaged at the end).  ``first``: the average before
    step 1 (the initial parameters); only read when step 1 is skipped by ``every``."""
    a = None if first is None else np.asarray(first, dtype=np.float64)
    n, out = 0, []
    for i, p in enumerate(snapshots):
        step_no = i + 1
        w = schedule_weight(kind, decay, warmup, start_step, every, step_no, n)
        if w is not None:
            a = lerp(np.asarray(p, dtype=np.float64) if a is None else a, p, w)
            if step_no > start_step:
                n += 1
        out.append(None if a is None else a.copy())
    return out, n
