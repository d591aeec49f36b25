"""Predicted bubbles matched to simulated ones, restated in numpy straight from the definitions on top of the flood fill of
tests/bubbles_restatement.py, and the synthetic frame pairs of the tests as formulas."""
import numpy as np

from tests import bubbles_restatement as R

INT_ROWS = ("match_pred", "match_target", "overlap", "counts", "mask")
ROWS = INT_ROWS + ("displacement",)
COUNTS = ("hits", "misses", "false_alarms", "heater_hits", "heater_misses", "heater_false_alarms")


def _centroid_sums(lab, k):
    """Exact integer sums of y and of x over the cells of labels 1 .. k: two int64 arrays of k."""
    yy, xx = np.mgrid[0:lab.shape[0], 0:lab.shape[1]]
    keep = (lab >= 1) & (lab <= k)
    sy, sx = np.zeros(k, np.int64), np.zeros(k, np.int64)
    np.add.at(sy, lab[keep] - 1, yy[keep])
    np.add.at(sx, lab[keep] - 1, xx[keep])
    return sy, sx


def match(p, s, max_bubbles, min_iou=0.0):
    """One frame pair -> a dict of match_pred, match_target, overlap (max_bubbles int32), displacement (max_bubbles float32), counts (6 int32),
    mask (2 int32), and the kp x ks overlap table.  p, s: the dicts `bubbles_restatement.census` leaves for the prediction and the simulation
    (labels, count, attached, area); a count of -1 marks a census that gave up."""
    mb = max_bubbles
    if p["count"] < 0 or s["count"] < 0:
        out = {k: np.full(mb, -1, np.int32) for k in INT_ROWS[:3]}
        out.update(displacement=np.full(mb, np.nan, np.float32), counts=np.full(6, -1, np.int32), mask=np.full(2, -1, np.int32), table=np.zeros((0, 0), np.int64))
        return out
    lp, ls = p["labels"], s["labels"]
    kp, ks = min(p["count"], mb), min(s["count"], mb)
    table = np.zeros((kp, ks), np.int64)
    keep = (lp >= 1) & (lp <= kp) & (ls >= 1) & (ls <= ks)                            # labels above kp / ks are liquid for the table
    np.add.at(table, (lp[keep] - 1, ls[keep] - 1), 1)
    best_s = [int(np.argmax(table[i])) + 1 if table[i].max(initial=0) > 0 else 0 for i in range(kp)]         # argmax: the first of equals
    best_p = [int(np.argmax(table[:, j])) + 1 if table[:, j].max(initial=0) > 0 else 0 for j in range(ks)]
    (syp, sxp), (sys_, sxs) = _centroid_sums(lp, kp), _centroid_sums(ls, ks)
    out = {k: np.zeros(mb, np.int32) for k in INT_ROWS[:3]}
    out["displacement"] = np.zeros(mb, np.float32)
    hits = heater_hits = 0
    bound = float(np.float32(min_iou))
    for i in range(1, kp + 1):
        j = best_s[i - 1]
        if j == 0 or best_p[j - 1] != i:
            continue
        o, ap, as_ = int(table[i - 1, j - 1]), int(p["area"][i - 1]), int(s["area"][j - 1])
        if not float(o) >= bound * float(ap + as_ - o):
            continue
        out["match_pred"][i - 1], out["match_target"][j - 1], out["overlap"][i - 1] = j, i, o
        dy = np.float64(syp[i - 1]) / np.float64(ap) - np.float64(sys_[j - 1]) / np.float64(as_)
        dx = np.float64(sxp[i - 1]) / np.float64(ap) - np.float64(sxs[j - 1]) / np.float64(as_)
        out["displacement"][i - 1] = np.float32(np.sqrt(dy * dy + dx * dx))            # fp64 throughout, one rounding
        hits += 1
        heater_hits += i <= p["attached"] and j <= s["attached"]
    out["counts"] = np.array([hits, ks - hits, kp - hits, heater_hits, min(s["attached"], ks) - heater_hits, min(p["attached"], kp) - heater_hits], np.int32)
    out["mask"] = np.array([np.count_nonzero((lp > 0) & (ls > 0)), np.count_nonzero((lp > 0) | (ls > 0))], np.int32)
    out["table"] = table
    return out


def match_masks(mask_p, mask_s, connectivity=4, max_bubbles=256, min_iou=0.0):
    """`match` of two boolean masks, with the two censuses it was made from under "pred" and "target"."""
    p, s = R.census(mask_p, connectivity, max_bubbles), R.census(mask_s, connectivity, max_bubbles)
    out = match(p, s, max_bubbles, min_iou)
    out["pred"], out["target"] = p, s
    return out


def match_fields(phi_p, phi_s, connectivity=4, max_bubbles=256, min_iou=0.0):
    """phi_p, phi_s (F, H, W) -> the rows of every frame pair stacked (F, ...), and the censuses' count / attached / area under *_pred / *_target:
    what `bubble_match` leaves."""
    per = [match_masks(a > 0, b > 0, connectivity, max_bubbles, min_iou) for a, b in zip(phi_p, phi_s)]
    out = {k: np.stack([f[k] for f in per]) for k in ROWS}
    for side in ("pred", "target"):
        for k in ("count", "attached", "area"):
            out[f"{k}_{side}"] = np.stack([np.asarray(f[side][k], np.int32) for f in per])
    out["tables"] = [f["table"] for f in per]
    return out


def iou(rows):
    """(..., max_bubbles) float32 per predicted slot from stacked rows: overlap / union in fp64, rounded once; NaN where unmatched."""
    mp, ov = rows["match_pred"].astype(np.int64), rows["overlap"].astype(np.float64)
    partner = np.take_along_axis(rows["area_target"].astype(np.int64), np.clip(mp - 1, 0, None), -1)
    union = np.where(mp > 0, rows["area_pred"] + partner - rows["overlap"], 0).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(union > 0, ov / union, np.nan).astype(np.float32)


def scores(counts, attached=False):
    """precision, recall, csi (float32, NaN where the denominator is 0) from counts (..., 6)."""
    c = np.asarray(counts, np.float64)[..., 3:] if attached else np.asarray(counts, np.float64)[..., :3]
    h, m, f = c[..., 0], c[..., 1], c[..., 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        q = lambda num, den: np.where(den > 0, num / den, np.nan).astype(np.float32)
        return q(h, h + f), q(h, h + m), q(h, h + m + f)


def _box(shape, y0, y1, x0, x1):
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    return (y >= y0) & (y <= y1) & (x >= x0) & (x <= x1)


def _disc(shape, cy, cx, r2):
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    return (y - cy) ** 2 + (x - cx) ** 2 <= r2


def mixed_pair(shape=(24, 31)):
    """(prediction, simulation) masks of about ten bubbles a side: heater bubbles on both sides (heater hits), one in row 0 of the prediction
    only that overlaps a detached simulated one, one in row 0 of the simulation only (a heater miss), a predicted blob over two simulated
    bubbles (a merge: one hit, one miss), two predicted bubbles inside one simulated (a split: one hit, one false alarm), a predicted bubble
    that shares four cells with each of two simulated ones (a tie), a bubble only predicted, one only simulated, and two shifted discs."""
    b, d = (lambda *a: _box(shape, *a)), (lambda *a: _disc(shape, *a))
    pred = (b(0, 2, 1, 3) | b(0, 1, 7, 8) | b(0, 0, 20, 25) | b(5, 7, 1, 9) | b(10, 12, 1, 4) | b(10, 12, 6, 8) | b(15, 16, 1, 5) | b(19, 20, 12, 13)
            | d(8, 20, 9) | d(16, 24, 5))
    sim = (b(0, 2, 2, 4) | b(1, 2, 7, 8) | b(0, 1, 22, 27) | b(0, 1, 12, 14) | b(5, 7, 1, 3) | b(5, 7, 5, 9) | b(10, 12, 1, 8) | b(15, 16, 1, 2)
           | b(15, 16, 4, 5) | b(19, 21, 20, 22) | d(9, 22, 9) | d(17, 25, 5))
    return pred, sim


def single_cells(shape=(34, 34)):
    """(prediction, simulation): isolated single cells on the even lattice, 17 x 17 = 289 a side; the simulation's are one cell to the right
    on the lower half of the frame, where no predicted cell meets a simulated one."""
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    pred = (y % 2 == 0) & (x % 2 == 0)
    sim = (y % 2 == 0) & np.where(y < shape[0] // 2, x % 2 == 0, x % 2 == 1)
    return pred, sim


def half_iou_pair(shape=(5, 7)):
    """(prediction, simulation): three cells each in a row, two of them shared: overlap 2, union 4, an IoU of exactly 1/2."""
    return _box(shape, 2, 2, 1, 3), _box(shape, 2, 2, 2, 4)


def large_pair(shape=(208, 200)):
    """(prediction, simulation) of more cells than the census labels in LDS, with a handful of discs: four shifted pairs (one of them on the
    heater), one disc only predicted and one only simulated."""
    d = lambda *a: _disc(shape, *a)
    pred = d(3, 20, 64) | d(60, 50, 400) | d(100, 150, 225) | d(180, 30, 100) | d(150, 100, 49)
    sim = d(4, 23, 64) | d(66, 58, 380) | d(97, 149, 260) | d(183, 26, 90) | d(30, 170, 81)
    return pred, sim


def phi_pair(masks, seed=0):
    """Two masks -> two float32 fields (`bubbles_restatement.phi_of`) with those vapour masks."""
    return R.phi_of(masks[0], seed=seed), R.phi_of(masks[1], seed=seed + 1)
