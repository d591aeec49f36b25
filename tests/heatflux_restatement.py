"""Seeded inputs and fp64 numpy restatements for the heat-flux evaluation (tests/golden/heatflux_eval.npz, tools/gen_heatflux_golden.py):
the per-frame heater heat flux of utils/heatflux.py for any accepted frame width, and the KDE / KL comparison of
examples/data_visualization.ipynb cell 4 without scipy.  Imported by the generator and by tests/test_heatflux_eval.py /
tests/test_gpu_heatflux_eval.py; nothing here touches a GPU."""
import numpy as np

HEATER_TEMPS = (1.0, 1.35)             # the seeded (T, 512, 512) fields are evaluated at both
STUDY_HEATER_TEMPS = (1.0, 1.2)        # one per file of the synthetic 512 x 512 study
STUDY_FRAMES = 8
FIELDS = ("dfun", "temperature", "velx", "vely")


def flux_fields():
    """The seeded (3, 512, 512) dfun / temperature fields tests/golden/physics.npz was made from."""
    from oracle.gen_golden import physics_inputs
    _, dfun, temp = physics_inputs()
    return dfun, temp


def synthetic_study(seed=77):
    """Two in-memory 512 x 512 trajectories of STUDY_FRAMES frames: one dict {field: (frames, 512, 512) fp32} per file.  The heater row has
    liquid and vapour cells in every frame, and the temperature stays below the heater's."""
    rs = np.random.RandomState(seed)
    trajs = []
    for i in range(2):
        shape = (STUDY_FRAMES, 512, 512)
        trajs.append({"dfun": (rs.standard_normal(shape) - 0.2 + 0.1 * i).astype(np.float32),
                      "temperature": np.abs(rs.standard_normal(shape) * (0.25 + 0.05 * i)).astype(np.float32),
                      "velx": rs.standard_normal(shape).astype(np.float32), "vely": rs.standard_normal(shape).astype(np.float32)})
    return trajs


def heatflux_rows(dfun_row, temp_row, heater_temp, x_min=-8.0, dx=1.0 / 32, lc=0.0007, conductivity=0.054):
    """utils/heatflux.py:25-36 on the heater rows alone: dfun_row, temp_row (..., W) fp32 = row 0 of every frame -> (...) fp64 fluxes.  As in
    the reference, the difference heater_temp - temp is formed in fp32 (a Python float against an fp32 array) and everything after it in fp64."""
    dfun_row, temp_row = np.asarray(dfun_row, dtype=np.float32), np.asarray(temp_row, dtype=np.float32)
    W = dfun_row.shape[-1]
    xc = x_min + (np.arange(W) + 0.5) * dx
    mask = (xc >= -5.0) & (xc <= 5.0)
    rows = (mask & (dfun_row < 0)).astype(np.float64) * (np.float32(heater_temp) - temp_row).astype(np.float64)
    return (conductivity * (rows / (dx * lc))).mean(axis=-1)


def heater_cells(dfun_row, x_min, dx):
    """(liquid, vapour) cell counts over the heater |x_c| <= 5 of rows (..., W)."""
    W = dfun_row.shape[-1]
    xc = x_min + (np.arange(W) + 0.5) * dx
    mask = (xc >= -5.0) & (xc <= 5.0)
    d = np.asarray(dfun_row)[..., mask]
    return int((d < 0).sum()), int((d >= 0).sum())


# ------------------------------------------------------------------------------------------------ KDE / KL
KL_CASES = (
    dict(name="gamma_800", kind="gamma", seed=101, n=800, m=800, points=1000),
    dict(name="gamma_5000_3200", kind="gamma", seed=102, n=5000, m=3200, points=1000),
    dict(name="gamma_20000", kind="gamma", seed=103, n=20000, m=20000, points=1000),
    dict(name="exact_zero", kind="zero", seed=None, n=500, m=400, points=401),      # the seed is searched by the generator and stored
)


def kl_sets(case, seed=None):
    """(sim, model) fp64 sample sets of a case, regenerated from its seed: gamma-shaped like a flux histogram, or the pair whose model
    density is exactly zero over most of the grid (the eps branch)."""
    rs = np.random.RandomState(case["seed"] if seed is None else int(seed))
    n, m = case["n"], case["m"]
    if case["kind"] == "gamma":
        return rs.gamma(6.0, 2.0, n) + 3.0, rs.gamma(5.0, 2.4, m) + 2.5 + 0.4 * rs.standard_normal(m)
    return 3.0 * rs.standard_normal(n), 0.02 * rs.standard_normal(m) + 0.5


def simpson_uniform(f, step):
    """scipy.integrate.simpson (1.15) on a uniform grid: composite Simpson for an odd number of nodes; for an even number composite Simpson
    over the first N - 1 nodes plus step * (5 f[N-1] + 8 f[N-2] - f[N-3]) / 12 for the last interval."""
    f = np.asarray(f, dtype=np.float64)
    N = f.shape[0]
    M = N if N % 2 else N - 1
    total = step / 3.0 * (f[0] + f[M - 1] + 4.0 * f[1:M - 1:2].sum() + 2.0 * f[2:M - 2:2].sum())
    if M != N:
        total += step * (5.0 * f[N - 1] + 8.0 * f[N - 2] - f[N - 3]) / 12.0
    return float(total)


def kde_bandwidth(samples):
    """Scott's factor for one dimension times the unbiased standard deviation (scipy.stats.gaussian_kde's default)."""
    s = np.asarray(samples, dtype=np.float64)
    return float(s.shape[0] ** (-1.0 / 5) * np.sqrt(((s - s.mean()) ** 2).sum() / (s.shape[0] - 1)))


def kde_pdf(samples, x, chunk=2048):
    """sum_j exp(-((x_i - s_j) / h)^2 / 2) / (n h sqrt(2 pi)), in slabs of samples (no points x n matrix)."""
    s = np.asarray(samples, dtype=np.float64)
    h = kde_bandwidth(s)
    acc = np.zeros_like(x)
    with np.errstate(under="ignore"):
        for j in range(0, s.shape[0], chunk):
            d = (x[:, None] - s[None, j:j + chunk]) / h
            acc += np.exp(-0.5 * d * d).sum(axis=1)
    return acc / (s.shape[0] * h * np.sqrt(2.0 * np.pi))


def kl_integrand(pdf_p, pdf_q, eps=1e-10):
    """p log(p / q) with q == 0 -> eps, and 0 where p == 0 (the limit; numpy alone gives NaN there)."""
    q = np.where(pdf_q == 0, eps, pdf_q)
    safe = np.where(pdf_p == 0, 1.0, pdf_p)
    with np.errstate(over="ignore", invalid="ignore"):                               # entries the mask discards
        return np.where(pdf_p == 0, 0.0, pdf_p * np.log(safe / q))


def kde_kl(sim, model, points=1000, eps=1e-10):
    """The notebook's cell 4 restated: returns (kl, x, pdf_sim, pdf_model, A) with A = the same rule applied to |integrand|."""
    sim, model = np.asarray(sim, dtype=np.float64), np.asarray(model, dtype=np.float64)
    x = np.linspace(min(sim.min(), model.min()), max(sim.max(), model.max()), points)
    p, q = kde_pdf(sim, x), kde_pdf(model, x)
    f = kl_integrand(p, q, eps)
    step = (x[-1] - x[0]) / (points - 1)
    return simpson_uniform(f, step), x, p, q, simpson_uniform(np.abs(f), step)
