"""Bubble links, events and track ids restated in numpy straight from their definitions, on top of the flood fill of
tests/bubbles_restatement.py, and the synthetic sequences of the tests as formulas."""
import numpy as np

from tests import bubbles_restatement as R

EVENTS = ("births", "deaths", "merges", "splits", "departures")
LINK_KEYS = ("successor", "n_successors", "predecessor", "n_predecessors", "departure_area")


def links(la, ka, lb, kb, attached_a, attached_b, area_a, max_bubbles=None):
    """One pair of label images -> a dict of successor, n_successors, predecessor, n_predecessors, departure_area (each max_bubbles int32, 0
    behind ka / kb), events (5 int32) and the ka x kb overlap table.  ka / kb = min(count, max_bubbles); labels above them are liquid."""
    mb = max(ka, kb) if max_bubbles is None else max_bubbles
    overlap = np.zeros((ka, kb), np.int64)
    keep = (la >= 1) & (la <= ka) & (lb >= 1) & (lb <= kb)
    np.add.at(overlap, (la[keep] - 1, lb[keep] - 1), 1)
    out = {k: np.zeros(mb, np.int32) for k in LINK_KEYS}
    for i in range(ka):
        row = overlap[i]
        out["n_successors"][i] = np.count_nonzero(row)
        out["successor"][i] = int(np.argmax(row)) + 1 if row.max(initial=0) > 0 else 0          # argmax: the first of equals
    for j in range(kb):
        col = overlap[:, j]
        out["n_predecessors"][j] = np.count_nonzero(col)
        out["predecessor"][j] = int(np.argmax(col)) + 1 if col.max(initial=0) > 0 else 0
    departures = 0
    for i in range(1, ka + 1):
        j = int(out["successor"][i - 1])
        if i <= attached_a and j >= 1 and j > attached_b and out["predecessor"][j - 1] == i:
            out["departure_area"][i - 1] = area_a[i - 1]
            departures += 1
    out["events"] = np.array([np.count_nonzero(out["predecessor"][:kb] == 0), np.count_nonzero(out["successor"][:ka] == 0),
                              np.count_nonzero(out["n_predecessors"] >= 2), np.count_nonzero(out["n_successors"] >= 2), departures], np.int32)
    out["overlap"] = overlap
    return out


def track_ids(counts, successor, predecessor, max_bubbles):
    """counts (T,), successor / predecessor (T - 1, max_bubbles) -> track_id (T, max_bubbles) int32 and the number of tracks.  Bubble j of frame
    t + 1 continues bubble i of frame t iff each names the other; a pair of -1 ends all tracks."""
    T = len(counts)
    ids = np.zeros((T, max_bubbles), np.int32)
    n = 0
    for t in range(T):
        for k in range(max(0, min(int(counts[t]), max_bubbles))):
            p = int(predecessor[t - 1][k]) if t > 0 else 0
            if p > 0 and successor[t - 1][p - 1] == k + 1:
                ids[t, k] = ids[t - 1, p - 1]
            else:
                n += 1
                ids[t, k] = n
    return ids, n


def tracks(phi, connectivity=4, max_bubbles=256):
    """phi (T, H, W) -> a dict: count / attached (T,), area (T, mb), labels (T, H, W), the link rows (T - 1, mb), events (T - 1, 5), track_id
    (T, mb), n_tracks: what `bubble_tracks` leaves for one sequence."""
    mb = max_bubbles
    frames = [R.census(f > 0, connectivity, mb) for f in phi]
    T = len(frames)
    out = {"count": np.array([f["count"] for f in frames], np.int32), "attached": np.array([f["attached"] for f in frames], np.int32),
           "area": np.stack([f["area"] for f in frames]), "labels": np.stack([f["labels"] for f in frames])}
    rows = {k: np.zeros((T - 1, mb), np.int32) for k in LINK_KEYS}
    rows["events"] = np.zeros((T - 1, 5), np.int32)
    for t in range(T - 1):
        a, b = frames[t], frames[t + 1]
        got = links(a["labels"], min(a["count"], mb), b["labels"], min(b["count"], mb), a["attached"], b["attached"], a["area"], mb)
        for k in rows:
            rows[k][t] = got[k]
    out.update(rows)
    out["track_id"], out["n_tracks"] = track_ids(out["count"], rows["successor"], rows["predecessor"], mb)
    return out


def _disc(shape, cy, cx, r2):
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    return (y - cy) ** 2 + (x - cx) ** 2 <= r2


def rising_discs(frames=12, shape=R.MASK_SHAPE):
    """bool (frames, H, W): a disc that rises off the heater row and leaves it (a departure), two discs that drift together and merge, one
    that grows on the heater from frame 6 (a birth) and one that shrinks away before frame 5 (a death)."""
    out = np.zeros((frames,) + tuple(shape), bool)
    for t in range(frames):
        m = _disc(shape, 2 * t - 4, 12, 25) | _disc(shape, 20, 30 + t, 9) | _disc(shape, 20, 52 - t, 9)
        if t >= 6:
            m |= _disc(shape, 0, 60, (t - 5) ** 2)
        if t < 5:
            m |= _disc(shape, 35, 5, (5 - t) ** 2 - 1)
        out[t] = m
    return out


def dense_dots(shape=R.MASK_SHAPE):
    """bool (2, H, W): 360 two-cell dots per frame, every dot of the second frame one column to the right of its dot of the first: each
    overlaps exactly that one, in one cell."""
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    return np.stack([(y % 2 == 0) & (x % 4 < 2), (y % 2 == 0) & ((x + 3) % 4 < 2)])


def phi_of_sequence(masks, seed=0):
    return np.stack([R.phi_of(m, seed=seed + i) for i, m in enumerate(masks)])
