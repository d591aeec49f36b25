"""The renderer of csrc/render.hip restated in numpy, fp64, independent of the product code: layout, colour rule, interface outline, velocity
arrows with their distances, colour bars, and the composition of a 2 x 3 panel and of a strip.

Everything returns plain arrays.  The arrow functions also return each pixel's distance to the nearest stroke it is tested against, so a
test can set aside the pixels whose distance lies within a hair of the stroke's half-width (the only place where two correct fp64
evaluations may disagree)."""
import numpy as np

SDF, TEMP, SPEED = 0, 1, 2
WHITE = np.array([255, 255, 255], dtype=np.uint8)
BAND = 1e-6        # pixels


def layout(H, W, scale=2, rows=2, cols=3, stride=8, gutter=6, bar_gap=4, bar_width=8, label_width=38, title_height=10, stroke=None):
    """Slot (r, c): tile at rows oy + r * pitch_y .., columns ox + c * pitch_x ..; bar bar_dx right of the tile's left edge."""
    s = scale
    bar_dx = W * s + bar_gap
    pitch_x = bar_dx + bar_width + label_width + gutter
    pitch_y = H * s + gutter + title_height
    img_w = gutter + cols * pitch_x
    img_w += (-img_w) % 4
    return dict(H=H, W=W, scale=s, rows=rows, cols=cols, ox=gutter, oy=gutter + title_height, pitch_x=pitch_x, pitch_y=pitch_y, bar_dx=bar_dx,
                bar_w=bar_width, img_h=gutter + rows * pitch_y, img_w=img_w, stride=stride, stroke=max(0.6, 0.2 * s) if stroke is None else stroke,
                title_h=title_height, label_w=label_width)


def colour_index(x, vmin, vmax):
    """matplotlib's Normalize + Colormap.__call__ in fp64 -> (index 0 .. 255, is-NaN).  vmax == vmin: index 0 everywhere, never NaN."""
    x = np.asarray(x).astype(np.float64)
    if vmax == vmin:
        return np.zeros(x.shape, dtype=np.int64), np.zeros(x.shape, dtype=bool)
    with np.errstate(all="ignore"):
        t = (x - np.float64(vmin)) / (np.float64(vmax) - np.float64(vmin))
        bad = np.isnan(t)
        k = np.floor(np.where(bad, 0.0, t) * 256.0)
    return np.clip(k, 0, 255).astype(np.int64), bad


def colour_tile(x, vmin, vmax, lut):
    idx, bad = colour_index(x, vmin, vmax)
    out = lut[idx]
    out[bad] = WHITE
    return out


def speed(u, v):
    u, v = np.asarray(u).astype(np.float64), np.asarray(v).astype(np.float64)
    return np.sqrt(u * u + v * v)


def edge_cells(sdf):
    """Liquid cells (sdf < 0) with at least one in-range 4-neighbour that is not liquid."""
    liq = np.asarray(sdf) < 0
    H, W = liq.shape
    touch = np.zeros_like(liq)
    touch[1:, :] |= ~liq[:-1, :]
    touch[:-1, :] |= ~liq[1:, :]
    touch[:, 1:] |= ~liq[:, :-1]
    touch[:, :-1] |= ~liq[:, 1:]
    return liq & touch


def outline(sdf):
    """The 3 x 3 dilation of the edge cells."""
    e = edge_cells(sdf)
    H, W = e.shape
    pad = np.zeros((H + 2, W + 2), dtype=bool)
    pad[1:-1, 1:-1] = e
    out = np.zeros_like(e)
    for di in range(3):
        for dj in range(3):
            out |= pad[di:di + H, dj:dj + W]
    return out


def upscale(cells, s):
    """Cell image (H, W, ...) with row 0 at the bottom -> pixel image (H s, W s, ...) with row 0 on top."""
    return np.repeat(np.repeat(cells[::-1], s, axis=0), s, axis=1)


def _segment_distance(px, py, ax, ay, bx, by):
    ex, ey = bx - ax, by - ay
    l2 = ex * ex + ey * ey
    wx, wy = px - ax, py - ay
    t = np.clip((wx * ex + wy * ey) / l2, 0.0, 1.0) if l2 > 0 else np.zeros_like(wx)
    return np.sqrt((wx - t * ex) ** 2 + (wy - t * ey) ** 2)


def arrow_strokes(u, v, vmax, cx, cy, full):
    """The three strokes [(ax, ay, bx, by)] of the arrow of velocity (u, v) about the pixel centre (cx, cy), screen y downwards; [] for none."""
    u, v = float(u), float(v)
    q = float(np.sqrt(np.float64(u) * u + np.float64(v) * v))
    if not (q > 0 and np.isfinite(q) and vmax > 0):
        return []
    ln = full * min(q / vmax, 1.0)
    dx, dy = u / q, -v / q
    tx, ty = cx + 0.5 * ln * dx, cy + 0.5 * ln * dy
    c, s_, k = -np.sqrt(3.0) / 2.0, 0.5, 0.35 * ln
    return [(cx - 0.5 * ln * dx, cy - 0.5 * ln * dy, tx, ty),
            (tx, ty, tx + k * (c * dx - s_ * dy), ty + k * (s_ * dx + c * dy)),
            (tx, ty, tx + k * (c * dx + s_ * dy), ty + k * (-s_ * dx + c * dy))]


def arrow_distance(u, v, mask, s, stride, vmax):
    """(H s, W s) fp64: every pixel centre's distance to the nearest stroke of the arrows of its own block of stride x stride cells and of the
    8 blocks around it (inf where there is none).  Anchors: cells i % stride == j % stride == stride // 2; their velocity is zeroed where
    mask > 0."""
    u, v = np.asarray(u), np.asarray(v)
    H, W = u.shape
    dist = np.full((H * s, W * s), np.inf)
    py, px = np.meshgrid(np.arange(H * s) + 0.5, np.arange(W * s) + 0.5, indexing="ij")
    cell_i = H - 1 - np.arange(H * s) // s          # field row of every pixel row
    cell_j = np.arange(W * s) // s
    for ai in range(stride // 2, H, stride):
        for aj in range(stride // 2, W, stride):
            uu, vv = (0.0, 0.0) if (mask is not None and mask[ai, aj] > 0) else (u[ai, aj], v[ai, aj])
            strokes = arrow_strokes(uu, vv, vmax, (aj + 0.5) * s, (H - 1 - ai + 0.5) * s, 0.9 * stride * s)
            if not strokes:
                continue
            rows = np.abs(cell_i // stride - ai // stride) <= 1
            cols = np.abs(cell_j // stride - aj // stride) <= 1
            win = np.ix_(rows, cols)
            for a in strokes:
                dist[win] = np.minimum(dist[win], _segment_distance(px[win], py[win], *a))
    return dist


def bar(hs, bar_w, lut):
    """The colour bar beside a tile of hs pixel rows: vmax on top, vmin at the bottom."""
    idx = ((hs - 1 - np.arange(hs)) * 256) // hs
    return np.repeat(lut[idx][:, None, :], bar_w, axis=1)


def tile(kind, a, b, mask, vmin, vmax, lay, luts):
    """-> ((H s, W s, 3) uint8, (H s, W s) bool: pixels inside the arrow band).  luts = (Blues, turbo)."""
    s = lay["scale"]
    if kind == SPEED:
        img = upscale(colour_tile(speed(a, b), vmin, vmax, luts[1]), s)
        d = arrow_distance(a, b, mask, s, lay["stride"], vmax)
        img[d <= lay["stroke"]] = WHITE
        return img, np.abs(d - lay["stroke"]) <= BAND
    img = upscale(colour_tile(a, vmin, vmax, luts[0 if kind == SDF else 1]), s)
    if kind == SDF:
        img[upscale(outline(a), s)] = 0
    return img, np.zeros(img.shape[:2], dtype=bool)


def compose(slots, lay, luts):
    """slots: per slot in row-major order (kind, a, b, mask, vmin, vmax) -> (image (img_h, img_w, 3) uint8, band (img_h, img_w) bool)."""
    img = np.full((lay["img_h"], lay["img_w"], 3), 255, dtype=np.uint8)
    band = np.zeros(img.shape[:2], dtype=bool)
    hs, ws = lay["H"] * lay["scale"], lay["W"] * lay["scale"]
    for k, (kind, a, b, mask, vmin, vmax) in enumerate(slots):
        y0 = lay["oy"] + (k // lay["cols"]) * lay["pitch_y"]
        x0 = lay["ox"] + (k % lay["cols"]) * lay["pitch_x"]
        img[y0:y0 + hs, x0:x0 + ws], band[y0:y0 + hs, x0:x0 + ws] = tile(kind, a, b, mask, vmin, vmax, lay, luts)
        img[y0:y0 + hs, x0 + lay["bar_dx"]:x0 + lay["bar_dx"] + lay["bar_w"]] = bar(hs, lay["bar_w"], luts[0 if kind == SDF else 1])
    return img, band


def panel(pred, target, ranges, lay, luts, channels=(0, 1, 2, 3)):
    """One frame (C, H, W) each: the simulation on top, the prediction below; the arrows of both rows hidden where the SIMULATION's signed
    distance is positive."""
    sdf, temp, vx, vy = channels
    slots = []
    for x in (target, pred):
        if sdf >= 0:
            slots.append((SDF, x[sdf], None, None, *ranges[0]))
        if temp >= 0:
            slots.append((TEMP, x[temp], None, None, *ranges[1]))
        if vx >= 0 and vy >= 0:
            slots.append((SPEED, x[vx], x[vy], target[sdf] if sdf >= 0 else None, *ranges[2]))
    return compose(slots, lay, luts)


def strip(frames, kind, vrange, lay, luts):
    """T frames of one quantity side by side ((T, H, W), or (T, 2, H, W) for the speed); vrange None = the frames' own minimum and maximum,
    NaN left out."""
    frames = np.asarray(frames)
    if vrange is None:
        x = speed(frames[:, 0], frames[:, 1]) if kind == SPEED else frames.astype(np.float64)
        vrange = (np.nanmin(x), np.nanmax(x))
    slots = [(kind, f[0], f[1], None, *vrange) if kind == SPEED else (kind, f, None, None, *vrange) for f in frames]
    return compose(slots, lay, luts)


def ranges(frames, channels):
    """bf_render_ranges: (3, 5) fp64 rows {n, sum, sum of squares, min, max} of the signed distance, the temperature and the speed of
    (F, C, H, W) frames; min and max leave NaN out; a quantity with a channel of -1 has n = 0."""
    frames = np.asarray(frames)
    sdf, temp, vx, vy = channels
    out = np.zeros((3, 5))
    out[:, 3], out[:, 4] = np.inf, -np.inf
    for q, x in enumerate((frames[:, sdf].astype(np.float64) if sdf >= 0 else None, frames[:, temp].astype(np.float64) if temp >= 0 else None,
                           speed(frames[:, vx], frames[:, vy]) if vx >= 0 and vy >= 0 else None)):
        if x is None:
            continue
        with np.errstate(all="ignore"):
            finite = x[~np.isnan(x)]
            out[q] = (x.size, x.sum(), (x * x).sum(), finite.min() if finite.size else np.inf, finite.max() if finite.size else -np.inf)
    return out
