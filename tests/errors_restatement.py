"""numpy fp64 restatement of the error rows of DESIGN.md section 18 (csrc/spectra.hip): the oracle of tests/test_field_errors.py and
tests/test_gpu_field_errors.py.  The transform is np.fft.fft2 over the full plane, the shell of a mode comes from Python integers, the
interface window from an edge-padded mask (a clipped window and an edge-padded one hold the same values)."""
import math

import numpy as np


def shell_count(H, W):
    S = min(H, W)
    return math.isqrt(S * S // 2) + 1


def shell_table(H, W):
    """(H, W) int64: the shell of mode (ky, kx), the largest q with q^2 H^2 W^2 <= S^2 (fy^2 W^2 + fx^2 H^2), all in Python integers."""
    S = min(H, W)
    out = np.zeros((H, W), np.int64)
    for ky in range(H):
        fy = ky if ky <= H // 2 else ky - H
        for kx in range(W):
            fx = kx if kx <= W // 2 else kx - W
            out[ky, kx] = math.isqrt(S * S * (fy * fy * W * W + fx * fx * H * H) // (H * H * W * W))
    return out


def shell_power(x, table=None):
    """(K,) fp64: sum of |X|^2 / (H W)^2 over the modes of every shell of one (H, W) field."""
    H, W = x.shape
    table = shell_table(H, W) if table is None else table
    with np.errstate(invalid="ignore"):
        power = np.abs(np.fft.fft2(x.astype(np.float64))) ** 2 / float(H * W) ** 2
    return np.bincount(table.reshape(-1), weights=power.reshape(-1), minlength=shell_count(H, W))


def interface_mask(sdf, r=1):
    """Cells whose (2r+1)^2 window, clipped to the frame, holds both vapour (sdf > 0) and liquid (anything else, zero and NaN included)."""
    with np.errstate(invalid="ignore"):
        vap = np.pad(sdf > 0, r, mode="edge")
    H, W = sdf.shape
    any_v, any_l = np.zeros((H, W), bool), np.zeros((H, W), bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            win = vap[dy:dy + H, dx:dx + W]
            any_v |= win
            any_l |= ~win
    return any_v & any_l


def ring_mask(H, W):
    m = np.zeros((H, W), bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


def bands_of(power, lo, hi):
    K = power.shape[-1]
    lo, hi = min(lo, K), min(hi, K)
    return np.sqrt(np.array([power[:lo].sum(), power[lo:hi].sum(), power[hi:].sum()]))


def field_errors(pred, target, sdf=None, r=1, lo=4, hi=12):
    """Every row of one frame: pred, target (H, W) float32 (the bits the kernel reads), sdf (H, W) float32 or None -> dict of fp64 values."""
    H, W = pred.shape
    p, y = pred.astype(np.float64), target.astype(np.float64)
    e = p - y
    table = shell_table(H, W)
    with np.errstate(invalid="ignore"):
        out = {"rmse": np.sqrt(np.mean(e * e)), "max_error": np.max(np.abs(e)) if not np.isnan(e).any() else np.nan,
               "boundary_rmse": np.sqrt(np.mean(e[ring_mask(H, W)] ** 2))}
        if sdf is not None:
            m = interface_mask(sdf, r)
            out["interface_cells"] = int(m.sum())
            out["interface_rmse"] = np.sqrt(np.mean(e[m] ** 2)) if m.any() else np.nan
        out["spectrum_error"], out["spectrum_pred"], out["spectrum_target"] = shell_power(e, table), shell_power(p, table), shell_power(y, table)
        out["spectral_error"] = bands_of(out["spectrum_error"], lo, hi)
        out["total"] = {"spectrum_error": np.mean(e * e), "spectrum_pred": np.mean(p * p), "spectrum_target": np.mean(y * y)}
    return out


def smooth(H, W, rng):
    """A few low modes with random phases, O(1): what a surrogate produces."""
    y, x = np.mgrid[0:H, 0:W]
    f = np.zeros((H, W))
    for _ in range(4):
        ky, kx = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        f += np.cos(2 * np.pi * (ky * y / H + kx * x / W) + rng.random() * 2 * np.pi)
    return f / 2


CASES = ("smooth", "noise", "smooth + 1e-3 noise", "pred == target", "NaN", "no vapour")


def case_frames(H, W, seed):
    """The six frames of a shape: (pred, target, sdf) float32 arrays of shape (6, H, W), in the order of CASES.  The signed distance is a
    smooth field with islands of vapour; frame 0 holds an exact zero and frame 1 a NaN in it (both liquid), frame 5 no vapour at all."""
    rng = np.random.default_rng(seed)
    pred, target, sdf = (np.zeros((6, H, W), np.float32) for _ in range(3))
    for k in range(6):
        kind = k if k < 3 else 0
        for out in (pred, target):
            f = smooth(H, W, rng) if kind != 1 else rng.standard_normal((H, W))
            if kind == 2:
                f = f + 1e-3 * rng.standard_normal((H, W))
            out[k] = f
        sdf[k] = smooth(H, W, rng) - 0.2
    pred[3] = target[3]
    pred[4, H // 2, W // 2] = np.nan
    sdf[0, 0, 0] = 0.0
    sdf[1, H - 1, W - 1] = np.nan
    sdf[5] = -np.abs(sdf[5]) - 1.0
    return pred, target, sdf


def shell_bound(want, total, H, W):
    """One fp32 rounding plus the normwise FFT error bound carried through |X|^2: eta = 64 max(1, log2(H W)) 2^-53."""
    eta = 64.0 * max(1.0, math.log2(H * W)) * 2.0 ** -53
    return 2.0 ** -23 * want + 2.0 * eta * np.sqrt(want * total) + eta * eta * total


def band_bound(want, total, H, W):
    """The same carried through the square root: an amplitude error of eta sqrt(total), and one fp32 rounding."""
    eta = 64.0 * max(1.0, math.log2(H * W)) * 2.0 ** -53
    return 2.0 ** -23 * want + eta * math.sqrt(total)
