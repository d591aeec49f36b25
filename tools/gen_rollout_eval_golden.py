"""Golden values for the batched rollout evaluation, generated on the CPU from the reference implementation.

    python tools/gen_rollout_eval_golden.py [--reference /path/to/Bubbleformer]

writes tests/golden/rollout_eval.npz: the reference AViT of oracle/gen_golden.py's ROLLOUT (same configuration, weights, T = 2,
start_time = 5) rolled out 20 steps as scripts/inference.py:239-252 does, from the first sample of BOTH sample trajectories (dataset
indices 0 and 42 of the two-file dataset).  The clips are `BubbleForecast([sample_1, sample_2], ...)[i]` itself, normalised with the
constants `oracle.gen_golden.rollout_clips` uses (fp64 mean / standard deviation of each field of sample_1, no epsilon) handed in through
`normalize(diff, div)`, so the fixture is generated from the very clips `DeviceClipStore.gather` returns and its first trajectory is the
one tests/golden/rollout.npz pins.  Per trajectory, from the reference's fp64 run and from its fp32 run: the (40, 4) relative-L2 matrix of
utils/plot_utils.py:30-34 (those lines are executed as they stand) and the rollout notebook's `get_eikonal_loss` (that cell is executed as
it stands) of the de-normalised predicted and target dfun; plus the fp32 run's field drift per step, as rollout.npz has it."""
import argparse
import json
import os
import sys
import textwrap

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
if REPO not in sys.path:
    sys.path.insert(0, REPO)

STARTS = (0, 42)


def constants():
    """{field: fp64 mean}, {field: fp64 std} of sample_1, as oracle.gen_golden.rollout_clips takes them."""
    from bubbleformer_amd.data import hdf5_lite
    f = hdf5_lite.File(os.path.join(GOLDEN, "samples", "sample_1.hdf5"))
    data = {k: np.array(f[k][...], dtype=np.float64) for k in sorted(f.keys())}
    return {k: float(v.mean()) for k, v in data.items()}, {k: float(v.std()) for k, v in data.items()}


def dataset(diff, div, T, start_time):
    from bubbleformer_amd.data import BubbleForecast
    ds = BubbleForecast([os.path.join(GOLDEN, "samples", f"sample_{i}.hdf5") for i in (1, 2)], norm="std", time_window=T, start_time=start_time)
    ds.normalize(dict(diff), dict(div))
    return ds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="checkout of the reference implementation (default: oracle/gen_golden.py's)")
    args = ap.parse_args()
    from oracle import gen_golden, weights as W
    if args.reference:
        gen_golden.REF = args.reference
    ref_models, _, LpLoss = gen_golden._import_reference()
    nb = json.load(open(os.path.join(gen_golden.REF, "scripts", "inference_autoregressive.ipynb")))
    ns = {"torch": torch}
    exec(next("".join(c["source"]) for c in nb["cells"] if c["cell_type"] == "code" and "def get_eikonal_loss" in "".join(c["source"])), ns)
    eikonal = ns["get_eikonal_loss"]
    plot_lines = open(os.path.join(gen_golden.REF, "bubbleformer", "utils", "plot_utils.py")).read().splitlines()[29:34]
    rel_src = textwrap.dedent("\n".join(plot_lines))
    assert "relative_l2_error = diff_norm / bnorm" in rel_src, rel_src

    def rel_l2(preds, targets):
        scope = {"torch": torch, "preds": preds, "targets": targets}
        exec(rel_src, scope)
        return scope["relative_l2_error"]

    R = gen_golden.ROLLOUT
    T, steps = R["T"], R["steps"]
    diff, div = constants()
    ds = dataset(diff, div, T, R["start_time"])
    assert len(ds) == 84 and ds.locate(STARTS[1]) == (1, R["start_time"]), (len(ds), ds.locate(STARTS[1]))
    names = list(ds.output_fields)
    sdf = names.index("dfun")
    out = {"fields": np.array(names), "diff": np.array([diff[n] for n in names]), "div": np.array([div[n] for n in names]),
           "starts": np.array(STARTS), "T": np.array(T), "steps": np.array(steps), "start_time": np.array(R["start_time"])}
    criterion = LpLoss(d=2, p=2, reduce_dims=[0, 1], reductions=["mean", "mean"])
    for b, start in enumerate(STARTS):
        runs = {}
        for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            model = ref_models.get_model(R["model"], time_window=T, drop_path=0.0, **R["cfg"]).to(dtype)
            model.load_state_dict({k: v.to(dtype) for k, v in W.generate(W.param_shapes(**R["cfg"]), seed=R["seed"]).items()})
            model.eval()
            preds, tgts, crit = [], [], []
            with torch.no_grad():
                for itr in range(0, steps * T, T):                                   # scripts/inference.py:239-252
                    inp, tgt = ds[start + itr]
                    if preds:
                        inp = preds[-1]
                    pred = model(inp.to(dtype).unsqueeze(0)).squeeze(0)
                    preds.append(pred)
                    tgts.append(tgt.to(dtype))
                    crit.append(float(criterion(pred, tgts[-1])))
            p, t = torch.cat(preds), torch.cat(tgts)
            # de-normalised dfun (the notebook's `preds = model_preds * div_term + diff_term`), constants as the dataset applied them (fp32)
            dv, df = torch.tensor(np.float32(div["dfun"]), dtype=dtype), torch.tensor(np.float32(diff["dfun"]), dtype=dtype)
            out[f"rel_l2_{tag}/{b}"] = rel_l2(p, t).numpy()
            out[f"criterion_{tag}/{b}"] = np.array(crit)
            out[f"eikonal_pred_{tag}/{b}"] = eikonal(p[:, sdf] * dv + df).numpy()
            out[f"eikonal_target_{tag}/{b}"] = eikonal(t[:, sdf] * dv + df).numpy()
            runs[tag] = torch.stack(preds).double()
        p64, p32 = runs["f64"], runs["f32"]
        out[f"field_drift_f32/{b}"] = ((p32 - p64).flatten(1).norm(dim=1) / p64.flatten(1).norm(dim=1)).numpy()
        drift = out[f"field_drift_f32/{b}"]
        tol = np.maximum(2e-5, 4 * drift)
        for key, per_step in (("rel_l2", np.repeat(tol, T)[:, None]), ("eikonal_pred", np.repeat(tol, T)), ("eikonal_target", np.repeat(tol, T))):
            a64, a32 = out[f"{key}_f64/{b}"], out[f"{key}_f32/{b}"]
            print(f"trajectory {b}: the reference's fp32 {key} uses {np.max(np.abs(a32 - a64) / np.abs(a64) / per_step):.3f} of the drift rule's allowance")
        print(f"trajectory {b}: smallest rms of a normalised target field frame {float(torch.cat(tgts).pow(2).mean(dim=(2, 3)).sqrt().min()):.3f}")
    # trajectory 0 is the rollout tests/golden/rollout.npz pins: its criterion must agree within that file's drift rule
    z = np.load(os.path.join(GOLDEN, "rollout.npz"))
    err = np.abs(out["criterion_f64/0"] - z["criterion_f64"]) / np.abs(z["criterion_f64"])
    allow = np.maximum(2e-5, 4 * z["field_drift_f32"])
    print("trajectory 0 criterion against rollout.npz: relative", " ".join(f"{e:.1e}" for e in err[[0, 4, steps - 1]]),
          f"(steps 1, 5, {steps}); worst share of the drift rule {np.max(err / allow):.1e}")
    assert np.all(err <= allow), (err, allow)
    np.savez_compressed(os.path.join(GOLDEN, "rollout_eval.npz"), **out)
    print("wrote rollout_eval.npz", os.path.getsize(os.path.join(GOLDEN, "rollout_eval.npz")), "bytes")


if __name__ == "__main__":
    main()
