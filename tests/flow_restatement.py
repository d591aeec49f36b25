"""numpy fp64 restatement of the flow-consistency rows of DESIGN.md section 32 (csrc/flow.hip), straight from their definitions, cell by cell.

Frames are [H][W], x runs along W (index j) and y along H (index i), the spacing is dx on both axes; vapour is phi > 0, anything else is liquid
(zero and NaN included); interior cells are 1 <= i <= H - 2, 1 <= j <= W - 2.  Inputs are widened to fp64 before any arithmetic."""
import numpy as np

FRAME_ROWS = ("divergence_rms", "kinetic_energy", "enstrophy", "bulk_cells")
PAIR_ROWS = ("transport_rms", "interface_speed_rms", "transport_cells")


def denormalise(x, div, diff):
    """pred * div + diff as the kernels form it: an fp32 product, rounded, then an fp32 sum."""
    prod = np.asarray(x, dtype=np.float32) * np.float32(div)
    return prod + np.float32(diff)


def _rms(total, n):
    return np.sqrt(total / n) if n > 0 else np.float64("nan")


def frame_rows(phi, u, v, dx, r):
    """The four rows of one frame."""
    phi, u, v = (np.asarray(a, dtype=np.float64) for a in (phi, u, v))
    H, W = phi.shape
    vapour = phi > 0
    div2, bulk, ens = 0.0, 0, 0.0
    for i in range(1, H - 1):
        for j in range(1, W - 1):
            w = ((v[i, j + 1] - v[i, j - 1]) - (u[i + 1, j] - u[i - 1, j])) / (2 * dx)
            ens += 0.5 * w * w
            if not vapour[max(i - r, 0):i + r + 1, max(j - r, 0):j + r + 1].any():
                d = ((u[i, j + 1] - u[i, j - 1]) + (v[i + 1, j] - v[i - 1, j])) / (2 * dx)
                div2 += d * d
                bulk += 1
    ke = float(np.sum(0.5 * (u * u + v * v)))
    with np.errstate(invalid="ignore"):
        return {"divergence_rms": _rms(div2, bulk), "bulk_cells": bulk, "kinetic_energy": ke / (H * W), "enstrophy": ens / ((H - 2) * (W - 2))}


def pair_rows(f0, f1, dx, dt, band):
    """The three rows of the pair (f0 the earlier, f1 the later frame, each (phi, u, v)), and ``scale``: the root mean square over the band cells of
    |s| + |um dpm/dx| + |vm dpm/dy|, the size of the terms that cancel in the residual."""
    p0, u0, v0 = (np.asarray(a, dtype=np.float64) for a in f0)
    p1, u1, v1 = (np.asarray(a, dtype=np.float64) for a in f1)
    H, W = p0.shape
    pm, um, vm = 0.5 * (p0 + p1), 0.5 * (u0 + u1), 0.5 * (v0 + v1)
    res2, s2, scale2, n = 0.0, 0.0, 0.0, 0
    for i in range(1, H - 1):
        for j in range(1, W - 1):
            if not abs(pm[i, j]) < band:
                continue
            s = (p1[i, j] - p0[i, j]) / dt
            ax = um[i, j] * ((pm[i, j + 1] - pm[i, j - 1]) / (2 * dx))
            ay = vm[i, j] * ((pm[i + 1, j] - pm[i - 1, j]) / (2 * dx))
            res = s + ax + ay
            res2 += res * res
            s2 += s * s
            scale2 += (abs(s) + abs(ax) + abs(ay)) ** 2
            n += 1
    with np.errstate(invalid="ignore"):
        return {"transport_rms": _rms(res2, n), "interface_speed_rms": _rms(s2, n), "transport_cells": n, "scale": _rms(scale2, n)}


def sequence_rows(phi, u, v, dx, dt, band, r):
    """The rows of one sequence (T, H, W): the frame rows as (T,) arrays, the pair rows and ``scale`` as (T - 1,), row t - 1 the pair that ends in
    frame t."""
    T = phi.shape[0]
    frames = [frame_rows(phi[t], u[t], v[t], dx, r) for t in range(T)]
    pairs = [pair_rows((phi[t - 1], u[t - 1], v[t - 1]), (phi[t], u[t], v[t]), dx, dt, band) for t in range(1, T)]
    out = {k: np.array([f[k] for f in frames]) for k in FRAME_ROWS}
    out.update({k: np.array([p[k] for p in pairs]) for k in PAIR_ROWS + ("scale",)})
    return out


def smooth(H, W, rng, modes=3):
    """A smooth field of order one: a few low Fourier modes with random phases."""
    y, x = np.meshgrid(np.arange(H) / max(H, 2), np.arange(W) / max(W, 2), indexing="ij")
    out = np.zeros((H, W))
    for _ in range(modes):
        ky, kx = rng.integers(0, 3, size=2)
        out += rng.uniform(0.3, 1.0) * np.cos(2 * np.pi * (ky * y + kx * x) + rng.uniform(0, 2 * np.pi))
    return out


def fields(S, T, H, W, rng, dx=1.0 / 32, noise=1e-3):
    """S sequences of T frames (sdf, velx, vely) as fp32: a tilted plane through the middle of every frame that drifts with t (an interface through
    every frame) plus a smooth part, smooth velocities, and a little noise on all three."""
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = np.empty((3, S, T, H, W), dtype=np.float32)
    for s in range(S):
        a, b = rng.uniform(-1, 1, size=2)
        for t in range(T):
            plane = (a * (j - (W - 1) / 2) + b * (i - (H - 1) / 2)) * dx + 0.3 * dx * (t - (T - 1) / 2)
            out[0, s, t] = plane + 0.5 * dx * smooth(H, W, rng) + noise * dx * rng.standard_normal((H, W))
            out[1, s, t] = 0.2 * smooth(H, W, rng) + noise * rng.standard_normal((H, W))
            out[2, s, t] = 0.2 * smooth(H, W, rng) + noise * rng.standard_normal((H, W))
    return out
