"""Heat-flux evaluation, the parts that need no GPU: the numpy restatements of tests/heatflux_restatement.py against
tests/golden/heatflux_eval.npz (tools/gen_heatflux_golden.py: the reference's `heatflux` per frame, and cell 4 of
examples/data_visualization.ipynb executed as it stands), the `HeaterSpec` checks, and the declaration of the new entry points."""
import os
import re

import numpy as np
import pytest

from tests import heatflux_restatement as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


def test_restatements_reproduce_the_reference():
    """Per-frame fluxes to 1e-12 relative; at 512 columns their mean / max are physics.npz's heatflux_mean / heatflux_max.  Each KL within
    1e-13 * (A + 2) of the notebook's value and each density within 1e-12 relative: scipy and numpy are both fp64 on the CPU (the generator
    saw 9e-17 ... 1.4e-14 absolute on the divergences and at most 1.3e-13 relative on a density, stored as restatement_*_dev)."""
    z = np.load(os.path.join(GOLDEN, "heatflux_eval.npz"))
    phys = np.load(os.path.join(GOLDEN, "physics.npz"))
    dfun, temp = H.flux_fields()
    assert tuple(z["heater_temps"]) == H.HEATER_TEMPS and tuple(z["study_heater_temps"]) == H.STUDY_HEATER_TEMPS
    for k, ht in enumerate(H.HEATER_TEMPS):
        got = H.heatflux_rows(dfun[:, 0], temp[:, 0], ht)
        assert got.shape == (3,) and np.allclose(got, z[f"flux/{k}"], rtol=1e-12, atol=0)
    rows = H.heatflux_rows(dfun[:, 0], temp[:, 0], float(phys["heater_temp"]))
    assert rows.mean() == pytest.approx(float(phys["heatflux_mean"]), rel=1e-12) and rows.max() == pytest.approx(float(phys["heatflux_max"]), rel=1e-12)
    for i, (traj, ht) in enumerate(zip(H.synthetic_study(), H.STUDY_HEATER_TEMPS)):
        got = H.heatflux_rows(traj["dfun"][:, 0], traj["temperature"][:, 0], ht)
        assert got.shape == (H.STUDY_FRAMES,) and np.allclose(got, z[f"study_flux/{i}"], rtol=1e-12, atol=0)
    for case in H.KL_CASES:
        n = case["name"]
        sim, model = H.kl_sets(case, int(z[f"seed/{n}"]))
        kl, x, p, q, A = H.kde_kl(sim, model, case["points"])
        want, wA = float(z[f"kl/{n}"]), float(z[f"A/{n}"])
        print(f"{n}: KL {kl:.6f} (reference {want:.6f}), off by {abs(kl - want):.1e} of {1e-13 * (wA + 2):.1e}")
        assert abs(kl - want) <= 1e-13 * (wA + 2) and abs(A - wA) <= 1e-13 * (wA + 2)
        assert np.array_equal(x, z[f"x/{n}"])
        assert np.all(z[f"pdf_sim/{n}"] > 0)                                        # the 0 log 0 convention is not what is compared
        for got, ref in ((p, z[f"pdf_sim/{n}"]), (q, z[f"pdf_model/{n}"])):
            assert np.array_equal(got == 0, ref == 0)
            big = ref > 1e-250
            assert np.max(np.abs(got - ref)[big] / ref[big]) <= 1e-12
    assert int((z["pdf_model/exact_zero"] == 0).sum()) > 100                         # that case takes the eps branch


def test_kl_restatement_conventions():
    """Simpson's two rules against closed forms, and the 0 log 0 = 0 rule where numpy alone has NaN (two sets 60 apart)."""
    for N in (401, 400, 7, 4, 3):
        x = np.linspace(0.0, 2.0, N)
        step = 2.0 / (N - 1)
        assert H.simpson_uniform(x ** 2, step) == pytest.approx(8.0 / 3, rel=1e-13)          # both rules are exact for a parabola
        if N > 4:
            assert H.simpson_uniform(np.exp(x), step) == pytest.approx(np.exp(2.0) - 1, rel=3e-3 if N < 10 else 1e-6)
    rs = np.random.RandomState(5)
    a, b = rs.standard_normal(300), rs.standard_normal(200) + 60.0
    kl, x, p, q, A = H.kde_kl(a, b, 500)
    assert np.isfinite(kl) and (p == 0).any() and (q == 0).any()
    with np.errstate(all="ignore"):
        assert np.isnan(p * np.log(p / np.where(q == 0, 1e-10, q))).any()             # the notebook's expression as it stands


def test_heater_spec_checks():
    from bubbleformer_amd.utils import HeaterSpec
    from bubbleformer_amd.utils.physics import HeaterSpec as SamePlace
    assert HeaterSpec is SamePlace
    spec = HeaterSpec(heater_temp=1.0)
    assert (spec.temperature_field, spec.sdf_field, spec.x_min, spec.dx, spec.lc, spec.conductivity) == ("temperature", "dfun", -8.0, 1 / 32, 0.0007, 0.054)
    with pytest.raises(Exception):
        spec.dx = 1.0                                                                # frozen
    spec.check_width(512)
    HeaterSpec(1.0, dx=16 / 192).check_width(192)                                    # no binary fraction: accepted within 1e-9 relative
    HeaterSpec(1.0, dx=1 / 4).check_width(64)
    with pytest.raises(ValueError, match=r"256 columns.*0\.03125.*8\.0"):
        spec.check_width(256)
    with pytest.raises(ValueError):
        HeaterSpec(1.0, dx=16 / 192 * (1 + 1e-6)).check_width(192)
    assert spec.temperatures([0, 1, 0], 2) == [1.0, 1.0, 1.0]
    assert HeaterSpec((1.0, 1.2)).temperatures([0, 1, 0], 2) == [1.0, 1.2, 1.0]
    with pytest.raises(ValueError, match="3 entries.*2 files"):
        HeaterSpec((1.0, 1.2, 1.3)).temperatures([0, 1], 2)
    assert spec.channels(["velx", "temperature", "dfun"]) == (2, 1)
    with pytest.raises(ValueError, match="temperature"):
        spec.channels(["dfun", "velx"])
    with pytest.raises(ValueError, match="sdf"):
        HeaterSpec(1.0, sdf_field="sdf").channels(["dfun", "temperature"])


def test_report_without_heatflux_rows_says_so():
    import torch
    from bubbleformer_amd.utils.rollout import RolloutReport
    r = RolloutReport(torch.zeros(1, 2, 1), torch.zeros(1, 1), None, None, torch.zeros(1, 2, dtype=torch.int64), ["dfun"])
    assert r.heatflux_pred is None and r.heatflux_target is None
    with pytest.raises(ValueError, match="HeaterSpec"):
        r.heatflux_kl()
    with pytest.raises(ValueError, match="HeaterSpec"):
        r.save_heatfluxes("unused.pt")


def test_entry_points_are_declared_and_bound():
    from bubbleformer_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "bubbleformer_hip.h")).read(), flags=re.S)
    for name in ("bf_rollout_heatflux", "bf_kde_kl", "bf_kde_kl_ws_doubles"):
        assert name in _lib.SIGNATURES, name
        m = re.search(r"\b(?:int|int64_t)\s+%s\s*\((.*?)\)\s*;" % name, txt, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name     # one ctypes entry per declared parameter
    src = open(os.path.join(REPO, "bubbleformer_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bphysics\.hip\b", src, flags=re.M)
