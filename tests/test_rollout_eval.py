"""Batched rollout evaluation, the parts that need no GPU: host planning of `evaluate_rollouts`, the per-frame relative L2 against
tests/golden/rollout_eval.npz (tools/gen_rollout_eval_golden.py: the REFERENCE model rolled out from both sample trajectories as
scripts/inference.py:239-252 does, scored by utils/plot_utils.py:30-34), and the declaration of the scoring entry point."""
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
FILES = [os.path.join(GOLDEN, "samples", f"sample_{i}.hdf5") for i in (1, 2)]


def golden_dataset(z, **kw):
    """The two-file dataset with the fixture's constants (shared with tests/test_gpu_rollout_eval.py)."""
    from bubbleformer_amd.data import BubbleForecast
    ds = BubbleForecast(FILES, norm="std", time_window=int(z["T"]), start_time=int(z["start_time"]), **kw)
    names = [str(n) for n in z["fields"]]
    ds.normalize({n: float(v) for n, v in zip(names, z["diff"])}, {n: float(v) for n, v in zip(names, z["div"])})
    return ds


def test_plan_rollouts_checks_and_timesteps():
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.utils.rollout import plan_rollouts
    ds = BubbleForecast(FILES, time_window=2, start_time=5)
    assert len(ds) == 84                                                     # 42 samples per 50-frame file
    plan = plan_rollouts(ds, [0, 42, 47], 18)
    assert plan.files == [0, 1, 1] and plan.first == [5, 50 + 5, 50 + 10]
    T = 2
    for b, local in enumerate([0, 0, 5]):                                    # start_time + local index + (s + 1) * T + t, file-relative
        want = [5 + local + (s + 1) * T + t for s in range(18) for t in range(T)]
        assert plan.timesteps.dtype == torch.int64 and plan.timesteps[b].tolist() == want
    assert int(plan.timesteps[2, -1]) == 47                                  # frame 47 of 50: the last target frame of sample 47 - 42 + 17 * 2 = 39
    plan_rollouts(ds, [0, 42], 21)                                           # sample 40 of each file is its last but one: 21 steps fit
    with pytest.raises(IndexError, match=r"trajectory 1 .*step 20 is the last that fits"):
        plan_rollouts(ds, [0, 44], 21)
    with pytest.raises(IndexError, match=r"trajectory 0 .*step 1 is the last that fits"):
        plan_rollouts(ds, [41, 42], 2)                                       # sample 41 + 2 is file 1's: the rollout would cross files
    with pytest.raises(IndexError):
        plan_rollouts(ds, [84], 1)
    with pytest.raises(ValueError):
        plan_rollouts(ds, [0], 0)
    with pytest.raises(ValueError, match="time_window"):
        plan_rollouts(ds, [0], 1, model_time_window=3)
    with pytest.raises(ValueError, match="fields"):
        plan_rollouts(BubbleForecast(FILES, input_fields=["dfun", "velx"], output_fields=["dfun"], time_window=2, start_time=5), [0], 1)


def test_relative_l2_per_frame_matches_the_reference_curves():
    """The oracle's fp64 rollout (oracle.filmavit_ref.avit_forward, as test_oracle_rollout_matches_the_reference_rollout drives it) of both
    trajectories, scored by relative_l2_per_frame, against the reference's fp64 matrices: rtol 1e-9 up to step 5 and 1e-6 after it.  Both
    come from that test's pins of the oracle against the reference (the step-5 field to 1e-11, the last field to 1e-7; an entry is a ratio
    of norms of size one, so it moves by about the field's relative error), with a factor ten over the later pin."""
    from bubbleformer_amd.utils.rollout import relative_l2_per_frame
    from oracle import filmavit_ref as R, weights as W
    from oracle.gen_golden import ROLLOUT
    z = np.load(os.path.join(GOLDEN, "rollout_eval.npz"))
    ds = golden_dataset(z)
    T, steps, cfg = ROLLOUT["T"], ROLLOUT["steps"], ROLLOUT["cfg"]
    assert (int(z["T"]), int(z["steps"]), int(z["start_time"])) == (T, steps, ROLLOUT["start_time"])
    sd = {k: v.double() for k, v in W.generate(W.param_shapes(**cfg), seed=ROLLOUT["seed"]).items()}
    for b, start in enumerate(z["starts"]):
        want = z[f"rel_l2_f64/{b}"]
        assert want.shape == (steps * T, 4)
        x = ds[int(start)][0].double()
        with torch.no_grad():
            for s in range(steps):
                x = R.avit_forward(sd, x.unsqueeze(0), patch_size=cfg["patch_size"], num_heads=cfg["num_heads"]).squeeze(0)
                got = relative_l2_per_frame(x, ds[int(start) + s * T][1].double()).numpy()
                assert got.shape == (T, 4)
                err = np.abs(got - want[s * T:(s + 1) * T]) / want[s * T:(s + 1) * T]
                assert err.max() <= (1e-9 if s < 5 else 1e-6), (b, s, err.max())
    p, t = torch.randn(3, 2, 5, 7), torch.randn(3, 2, 5, 7)                  # the definition itself (utils/plot_utils.py:30-33), fp32 in, fp32 out
    assert torch.equal(relative_l2_per_frame(p, t), torch.norm(p - t, p=2, dim=(2, 3)) / torch.norm(t, p=2, dim=(2, 3)))


def test_scoring_entry_point_is_declared_and_bound():
    from bubbleformer_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "bubbleformer_hip.h")).read(), flags=re.S)
    for name in ("bf_rollout_score", "bf_rollout_score_ws_doubles"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.SIGNATURES, name
    res, args = _lib.SIGNATURES["bf_rollout_score"]
    m = re.search(r"\bint\s+bf_rollout_score\s*\((.*?)\)\s*;", txt, flags=re.S)
    assert m and len(m.group(1).split(",")) == len(args)                     # one ctypes entry per declared parameter
