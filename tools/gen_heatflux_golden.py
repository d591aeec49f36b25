"""Golden values for the heat-flux evaluation, generated on the CPU from the reference implementation.

    python tools/gen_heatflux_golden.py [--reference /path/to/Bubbleformer]

writes tests/golden/heatflux_eval.npz (arrays only):
  * per-frame heat fluxes: the reference's `heatflux` (utils/heatflux.py, loaded by path) called as it stands on every single-frame slice
    of the seeded (3, 512, 512) fields of tests/golden/physics.npz, for two heater temperatures (the mean over one frame is that frame's row),
    and on every frame of the synthetic two-file 512 x 512 study of tests/heatflux_restatement.py with one heater temperature per file;
  * KL cases: cell 4 of examples/data_visualization.ipynb executed as it stands (scipy's gaussian_kde and simpson) on the seeded sets of
    tests/heatflux_restatement.py: the divergence, the grid, both densities, and A = the integral of |integrand| by the same rule.
The tool asserts what a test must not hide behind: the reference's simulated density is positive on every stored grid (the 0 log 0
convention is never what is compared), and in the exact-zero case every grid point is either robustly zero (largest exponent argument over
the model's samples below -800) or robustly normal (above -600); the seed of that case is searched and recorded."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def notebook_cell(ref):
    nb = json.load(open(os.path.join(ref, "examples", "data_visualization.ipynb")))
    code = ["".join(c["source"]) for c in nb["cells"] if c["cell_type"] == "code"]
    imports = next(c for c in code if "gaussian_kde" in c and "import" in c)
    cell = next(c for c in code if "kl_div_continuous" in c and "gaussian_kde(" in c)
    return imports, cell


def run_cell(imports, cell, sim, model, points):
    """Cell 4 as it stands; only the grid size, a literal 1000 in the cell, is replaced for the 401-point case."""
    if points != 1000:
        assert cell.count("1000)") == 1
        cell = cell.replace("1000)", f"{points})")
    ns = {"np": np, "heat_flux_sim": sim, "heat_flux_model": model}
    exec(imports, ns)
    with np.errstate(all="ignore"):
        exec(cell, ns)
    return float(ns["kl_div_continuous"]), ns["x_vals"], ns["pdf_sim"], ns["pdf_model"], ns["integrand"], ns["simpson"]


def zero_case_is_robust(sim, model, points, H):
    """Every grid point robustly zero or robustly normal in the model's density, and the simulated density nowhere near underflow."""
    x = np.linspace(min(sim.min(), model.min()), max(sim.max(), model.max()), points)
    nearest = lambda s: np.abs(x[:, None] - s[None, :]).min(axis=1)
    arg_q = -0.5 * (nearest(model) / H.kde_bandwidth(model)) ** 2
    arg_p = -0.5 * (nearest(sim) / H.kde_bandwidth(sim)) ** 2
    return bool(np.all((arg_q < -800) | (arg_q > -600)) and np.all(arg_p > -600)), int((arg_q < -800).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="checkout of the reference implementation (default: oracle/gen_golden.py's)")
    args = ap.parse_args()
    import scipy
    from oracle import gen_golden
    from tests import heatflux_restatement as H
    ref = args.reference or gen_golden.REF
    spec = importlib.util.spec_from_file_location("ref_heatflux", os.path.join(ref, "bubbleformer", "utils", "heatflux.py"))
    hf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(hf)
    out = {"scipy_version": np.array(scipy.__version__), "heater_temps": np.array(H.HEATER_TEMPS), "study_heater_temps": np.array(H.STUDY_HEATER_TEMPS)}

    def rows(dfun, temp, ht):
        r = [hf.heatflux(dfun[t:t + 1], temp[t:t + 1], ht) for t in range(dfun.shape[0])]
        assert all(a == b for a, b in r)                                            # one frame: its mean is its max is its row
        return np.array([a for a, _ in r], dtype=np.float64)

    dfun, temp = H.flux_fields()
    z = np.load(os.path.join(GOLDEN, "physics.npz"))
    for k, ht in enumerate(H.HEATER_TEMPS):
        out[f"flux/{k}"] = rows(dfun, temp, ht)
        mean, mx = hf.heatflux(dfun, temp, ht)
        assert mean == np.mean(out[f"flux/{k}"]) and mx == np.max(out[f"flux/{k}"])      # the rows' mean and max are the three-frame call's outputs
        mine = H.heatflux_rows(dfun[:, 0], temp[:, 0], ht)
        print(f"heater {ht}: rows {out[f'flux/{k}']}, restatement off by {np.max(np.abs(mine - out[f'flux/{k}']) / np.abs(out[f'flux/{k}'])):.1e} relative")
    assert float(z["heater_temp"]) == H.HEATER_TEMPS[0] and np.mean(out["flux/0"]) == float(z["heatflux_mean"]) and np.max(out["flux/0"]) == float(z["heatflux_max"])
    for i, (traj, ht) in enumerate(zip(H.synthetic_study(), H.STUDY_HEATER_TEMPS)):
        out[f"study_flux/{i}"] = rows(traj["dfun"], traj["temperature"], ht)
        liquid, vapour = H.heater_cells(traj["dfun"][:, 0], -8.0, 1 / 32)
        assert liquid > 0 and vapour > 0
        print(f"study file {i} (heater {ht}): rows {out[f'study_flux/{i}'][:3]} ..., {liquid} liquid / {vapour} vapour heater cells")

    imports, cell = notebook_cell(ref)
    for case in H.KL_CASES:
        seed = case["seed"]
        if case["kind"] == "zero":
            for seed in range(400):
                ok, zeros = zero_case_is_robust(*H.kl_sets(case, seed), case["points"], H)
                if ok and zeros > 0:
                    break
            else:
                raise SystemExit("no seed in 0 .. 399 gives a robust exact-zero case")
        sim, model = H.kl_sets(case, seed)
        kl, x, p, q, integrand, simpson = run_cell(imports, cell, sim, model, case["points"])
        assert np.isfinite(kl) and np.all(p > 0), case["name"]                      # the 0 log 0 convention is never what is compared
        A = float(simpson(np.abs(integrand), x))
        mine_kl, mine_x, mine_p, mine_q, mine_A = H.kde_kl(sim, model, case["points"])
        big = p > 1e-250
        dev_p = np.max(np.abs(mine_p - p)[big] / p[big])
        raw_q = np.where(q == 1e-10, 0.0, q) if case["kind"] == "zero" else q        # the cell overwrites exact zeros with its epsilon
        bigq = raw_q > 1e-250
        dev_q = np.max(np.abs(mine_q - raw_q)[bigq] / raw_q[bigq])
        assert np.array_equal(mine_q == 0, raw_q == 0) and np.array_equal(mine_x, x)
        n = case["name"]
        out[f"kl/{n}"], out[f"A/{n}"], out[f"x/{n}"], out[f"pdf_sim/{n}"], out[f"pdf_model/{n}"] = np.array(kl), np.array(A), x, p, raw_q
        out[f"seed/{n}"], out[f"restatement_kl_dev/{n}"], out[f"restatement_pdf_dev/{n}"] = np.array(seed), np.array(abs(mine_kl - kl)), np.array(max(dev_p, dev_q))
        print(f"{n}: seed {seed}, KL {kl:.6f}, A {A:.6f}, smallest density {min(p.min(), raw_q[raw_q > 0].min()):.1e}, zeros in q {int((raw_q == 0).sum())}; "
              f"restatement: KL off by {abs(mine_kl - kl):.1e} (allowance {1e-13 * (A + 2):.1e}), worst density {max(dev_p, dev_q):.1e} relative, A off by {abs(mine_A - A):.1e}")
        if case["kind"] == "zero":
            assert int((raw_q == 0).sum()) > 0
    path = os.path.join(GOLDEN, "heatflux_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote heatflux_eval.npz", os.path.getsize(path), "bytes; scipy", scipy.__version__)


if __name__ == "__main__":
    main()
