"""The bubble census restated in numpy and plain Python, for machines without scipy: a flood fill in raster order whose label images equal
`scipy.ndimage.label`'s (tools/gen_bubble_census_golden.py asserts that on every mask below and on every frame of the two sample files, for
both connectivities, before it writes tests/golden/bubble_census.npz), the per-frame figures derived from a label image, and the synthetic
masks of the tests as formulas."""
import numpy as np

MASK_SHAPE = (40, 72)          # no multiple of 4, of a wave or of the workgroup in either direction; 2880 cells: three cells per thread, then none
CONNECTIVITIES = (4, 8)
# name -> components under (4, 8)-connectivity at MASK_SHAPE
MASK_COUNTS = {"empty": (0, 0), "full": (1, 1), "checkerboard": (1440, 1), "alternate_rows": (20, 20), "comb": (1, 1), "serpentine": (1, 1),
               "u_around_blob": (2, 2), "diagonal": (40, 1), "corners_and_three": (7, 5), "random_0.5": (219, 23), "random_0.593": (91, 6)}


def masks(shape=MASK_SHAPE):
    """name -> bool (H, W), in the order of MASK_COUNTS."""
    H, W = shape
    y, x = np.mgrid[0:H, 0:W]
    out = {"empty": np.zeros(shape, bool), "full": np.ones(shape, bool), "checkerboard": (y + x) % 2 == 0, "alternate_rows": y % 2 == 0}
    out["comb"] = (x % 2 == 0) | (y == H - 1)                                        # teeth that join only in the last row: late merges
    out["serpentine"] = (y % 2 == 0) | ((y % 4 == 1) & (x == W - 1)) | ((y % 4 == 3) & (x == 0))      # one path through every row
    u = (((x == 10) | (x == 30)) & (y >= 5) & (y <= 25)) | ((y == 25) & (x >= 10) & (x <= 30))
    out["u_around_blob"] = u | ((y >= 10) & (y <= 12) & (x >= 18) & (x <= 20))       # the U's arms meet after the blob began: numbering by first cell
    out["diagonal"] = y == x * H // W
    m = np.zeros(shape, bool)
    for cy, cx in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (31, 31), (32, 32), (31, 33)):
        m[cy, cx] = True
    out["corners_and_three"] = m
    rng = np.random.default_rng(7)
    out["random_0.5"] = rng.random(shape) < 0.5
    out["random_0.593"] = rng.random(shape) < 0.593                                   # the second draw of the same generator
    assert list(out) == list(MASK_COUNTS)
    return out


def phi_of(mask, seed=0):
    """A float32 field whose vapour mask (phi > 0) is `mask`: magnitudes in [0.5, 1.5), and among the liquid cells an exact zero, a negative
    zero and a NaN where there is room (all three count as liquid)."""
    rng = np.random.default_rng(seed)
    phi = (rng.random(mask.shape) + 0.5).astype(np.float32) * np.where(mask, 1.0, -1.0).astype(np.float32)
    liquid = np.flatnonzero(~mask.ravel())
    for k, v in zip(liquid[:3], (0.0, -0.0, np.nan)):
        phi.ravel()[k] = v
    return phi


def label(mask, connectivity=4):
    """int32 (H, W): components of `mask` numbered 1, 2, ... in raster order of their first cell, 0 elsewhere; the number of components."""
    assert connectivity in CONNECTIVITIES
    H, W = mask.shape
    near = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    lab = np.zeros((H, W), np.int32)
    m = np.asarray(mask, bool)
    n = 0
    for y0, x0 in zip(*np.nonzero(m)):                                               # np.nonzero walks in raster order
        if lab[y0, x0]:
            continue
        n += 1
        lab[y0, x0] = n
        stack = [(int(y0), int(x0))]
        while stack:
            cy, cx = stack.pop()
            for dy, dx in near:
                yy, xx = cy + dy, cx + dx
                if 0 <= yy < H and 0 <= xx < W and m[yy, xx] and not lab[yy, xx]:
                    lab[yy, xx] = n
                    stack.append((yy, xx))
    return lab, n


def census(mask, connectivity=4, max_bubbles=256):
    """The figures bf_bubble_census leaves for one frame, from the flood fill: a dict of count, vapour_cells, attached, labels, and area /
    centroid / on_heater of the first max_bubbles components (zero-padded).  A centroid is np.float32(integer sum / area): one fp64 division,
    one rounding."""
    lab, n = label(mask, connectivity)
    H, W = lab.shape
    area_all = np.bincount(lab.ravel(), minlength=n + 1)[1:].astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    sy = np.bincount(lab.ravel(), weights=yy.ravel(), minlength=n + 1)[1:]            # exact: integers far below 2^53
    sx = np.bincount(lab.ravel(), weights=xx.ravel(), minlength=n + 1)[1:]
    heater = np.zeros(n, bool)
    heater[np.unique(lab[0][lab[0] > 0]) - 1] = True
    k = min(n, max_bubbles)
    area = np.zeros(max_bubbles, np.int32)
    centroid = np.zeros((max_bubbles, 2), np.float32)
    on_heater = np.zeros(max_bubbles, bool)
    area[:k] = area_all[:k]
    centroid[:k, 0] = (sy[:k] / area_all[:k]).astype(np.float32)
    centroid[:k, 1] = (sx[:k] / area_all[:k]).astype(np.float32)
    on_heater[:k] = heater[:k]
    return {"count": n, "vapour_cells": int(np.count_nonzero(mask)), "attached": int(heater.sum()), "labels": lab, "area": area,
            "centroid": centroid, "on_heater": on_heater, "area_all": area_all}


def blobs(shape, seed, count=40):
    """A mask of at most `count` discs of radius 2 .. 9 at seeded places (they may touch or overlap), some of them on row 0."""
    H, W = shape
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    m = np.zeros(shape, bool)
    for k in range(count):
        cy, cx, r = (0 if k % 5 == 0 else rng.integers(0, H)), rng.integers(0, W), rng.integers(2, 10)
        m |= (y - cy) ** 2 + (x - cx) ** 2 <= r * r
    return m


def smooth_field(shape, seed, threshold=0.35):
    """A few sinusoids minus a threshold, float32 of `shape` (..., H, W): a smooth random field with a handful of positive islands per frame."""
    rng = np.random.default_rng(seed)
    H, W = shape[-2:]
    y, x = np.mgrid[0:H, 0:W]
    out = np.zeros(shape, np.float64)
    for idx in np.ndindex(*shape[:-2]):
        f = np.zeros((H, W))
        for _ in range(4):
            ky, kx = rng.integers(1, 5, size=2)
            py, px = rng.random(2) * 2 * np.pi
            f += np.sin(2 * np.pi * ky * y / H + py) * np.sin(2 * np.pi * kx * x / W + px)
        out[idx] = f / 2 - threshold
    return out.astype(np.float32)
