"""Pictures of predictions, rendered on the device (reference: bubbleformer/utils/plot_utils.py; csrc/render.hip).

``plot_bubbleml`` writes the reference's 2 x 3 panel per predicted frame (signed distance, temperature and speed; simulation on top,
prediction below) and ``sdf_strip`` / ``temp_strip`` / ``vel_strip`` are its three ``wandb_*_plotter`` strips -- without matplotlib or cv2:
one kernel launch turns all frames of a call into uint8 RGB images, one copy brings them to the host, and the standard library writes the
PNG files (utils/png.py).  The colours are matplotlib's to the byte.  Two things are drawn differently, by definition rather than by
approximation: the interface outline is the 3 x 3 dilation of the liquid cells that touch a cell which is not liquid (the reference runs
cv2.Canny + dilate on the same mask), and the velocity is shown as one arrow per block of cells (the reference integrates streamlines).
The titles and the colour-bar end values are stamped on the host from a 5 x 7 glyph table kept here."""
import dataclasses
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import png

QUANTITIES = ("sdf", "temperature", "velocity")


@dataclasses.dataclass(frozen=True)
class RenderLayout:
    """Where everything of an image of rows x cols slots lies, in pixels (``RenderSpec.layout``)."""
    H: int
    W: int
    scale: int
    rows: int
    cols: int
    ox: int                 # left edge of the tile of slot (0, 0)
    oy: int                 # its top edge
    pitch_x: int            # from one tile's left edge to the next one's
    pitch_y: int
    bar_dx: int             # from a tile's left edge to its colour bar's
    bar_w: int
    img_h: int
    img_w: int              # a multiple of 4
    stride: int             # cells between two arrows
    stroke: float           # half-width of an arrow stroke
    title_h: int            # rows above a tile that the host stamps its title into
    label_w: int            # columns right of a bar that the host stamps its end values into

    def tile_origin(self, r: int, c: int):
        return self.oy + r * self.pitch_y, self.ox + c * self.pitch_x


@dataclasses.dataclass(frozen=True)
class RenderSpec:
    """The constants of a picture.  ``scale``: pixels per cell (nearest-neighbour); ``stride``: one arrow per stride x stride cells;
    ``stroke``: half-width of an arrow stroke in pixels, None = max(0.6, 0.2 * scale)."""
    scale: int = 2
    stride: int = 8
    gutter: int = 6
    bar_gap: int = 4
    bar_width: int = 8
    label_width: int = 38        # six glyphs of 5 + 1 pixels and a gap
    title_height: int = 10       # a glyph row of 7 pixels, 1 above and 2 below
    stroke: Optional[float] = None

    def layout(self, H: int, W: int, rows: int = 2, cols: int = 3) -> RenderLayout:
        s = int(self.scale)
        if min(H, W, s, rows, cols, self.stride) < 1 or min(self.gutter, self.bar_gap, self.bar_width, self.label_width, self.title_height) < 0:
            raise ValueError("sizes, scale and stride must be positive, the margins not negative")
        bar_dx = W * s + self.bar_gap
        pitch_x = bar_dx + self.bar_width + self.label_width + self.gutter
        pitch_y = H * s + self.gutter + self.title_height
        stroke = max(0.6, 0.2 * s) if self.stroke is None else float(self.stroke)
        return RenderLayout(H, W, s, rows, cols, self.gutter, self.gutter + self.title_height, pitch_x, pitch_y, bar_dx, self.bar_width,
                            self.gutter + rows * pitch_y, (self.gutter + cols * pitch_x + 3) // 4 * 4, int(self.stride), stroke,
                            self.title_height, self.label_width)


# ---------------------------------------------------------------------------------------------------------------- glyphs
_GLYPH_ROWS = {      # 5 x 7, '#' = ink; only what the titles and the end values need
    "0": ".###. #...# #..## #.#.# ##..# #...# .###.", "1": "..#.. .##.. ..#.. ..#.. ..#.. ..#.. .###.",
    "2": ".###. #...# ....# ...#. ..#.. .#... #####", "3": ".###. #...# ....# ..##. ....# #...# .###.",
    "4": "...#. ..##. .#.#. #..#. ##### ...#. ...#.", "5": "##### #.... ####. ....# ....# #...# .###.",
    "6": ".###. #.... #.... ####. #...# #...# .###.", "7": "##### ....# ...#. ..#.. ..#.. ..#.. ..#..",
    "8": ".###. #...# #...# .###. #...# #...# .###.", "9": ".###. #...# #...# .#### ....# ....# .###.",
    "-": "..... ..... ..... ##### ..... ..... .....", "+": "..... ..#.. ..#.. ##### ..#.. ..#.. .....",
    ".": "..... ..... ..... ..... ..... .##.. .##..", " ": "..... ..... ..... ..... ..... ..... .....",
    "S": ".#### #.... #.... .###. ....# ....# ####.", "D": "####. #...# #...# #...# #...# #...# ####.",
    "F": "##### #.... #.... ####. #.... #.... #....", "T": "##### ..#.. ..#.. ..#.. ..#.. ..#.. ..#..",
    "E": "##### #.... #.... ####. #.... #.... #####", "M": "#...# ##.## #.#.# #.#.# #...# #...# #...#",
    "P": "####. #...# #...# ####. #.... #.... #....", "V": "#...# #...# #...# #...# #...# .#.#. ..#..",
    "L": "#.... #.... #.... #.... #.... #.... #####", "A": ".###. #...# #...# ##### #...# #...# #...#",
    "B": "####. #...# #...# ####. #...# #...# ####.", "R": "####. #...# #...# ####. #.#.. #..#. #...#",
}
GLYPHS = {ch: np.array([[c == "#" for c in row] for row in rows.split()], dtype=bool) for ch, rows in _GLYPH_ROWS.items()}
GLYPH_W, GLYPH_H = 5, 7


def stamp_text(image: np.ndarray, y: int, x: int, text: str, x_end: Optional[int] = None) -> None:
    """Black 5 x 7 glyphs, one pixel apart, with the top-left corner at (y, x) of a (h, w, 3) uint8 image; what falls outside the image or
    right of ``x_end`` is dropped.  A character without a glyph raises KeyError."""
    h, w = image.shape[:2]
    x_end = w if x_end is None else min(w, x_end)
    for k, ch in enumerate(text):
        g = GLYPHS[ch]
        x0 = x + k * (GLYPH_W + 1)
        for gy, gx in zip(*np.nonzero(g)):
            yy, xx = y + int(gy), x0 + int(gx)
            if 0 <= yy < h and 0 <= xx < x_end:
                image[yy, xx] = 0


def end_value(v: float) -> str:
    """A colour-bar end value in the glyphs the table has."""
    return f"{float(v):.2f}" if np.isfinite(v) else "-"


def stamp_labels(image: np.ndarray, layout: RenderLayout, titles: Sequence[str], ranges: Sequence) -> None:
    """The host's share of an image: the title above every tile and vmax / vmin beside the ends of its colour bar.  titles and ranges
    (pairs (vmin, vmax)) are per slot, in row-major order."""
    g = layout
    for k, (title, (vmin, vmax)) in enumerate(zip(titles, ranges)):
        y0, x0 = g.tile_origin(k // g.cols, k % g.cols)
        stamp_text(image, y0 - g.title_h + 1, x0, title, x0 + g.bar_dx + g.bar_w)
        lx, lend = x0 + g.bar_dx + g.bar_w + 2, x0 + g.bar_dx + g.bar_w + g.label_w
        stamp_text(image, y0, lx, end_value(vmax), lend)
        if g.H * g.scale >= 2 * GLYPH_H + 1:
            stamp_text(image, y0 + g.H * g.scale - GLYPH_H, lx, end_value(vmin), lend)


# ---------------------------------------------------------------------------------------------------------------- device images
def _range_tensor(ranges, device) -> torch.Tensor:
    """(3, 2) fp64 on the device from a (3, 2) tensor or nested sequence of {vmin, vmax} per quantity (None for an absent one)."""
    if isinstance(ranges, torch.Tensor):
        if ranges.shape != (3, 2):
            raise ValueError("ranges must have shape (3, 2): {vmin, vmax} of the signed distance, the temperature and the speed")
        return ranges.to(device=device, dtype=torch.float64).contiguous()
    host = torch.tensor([[0.0, 0.0] if r is None else [float(r[0]), float(r[1])] for r in ranges], dtype=torch.float64)
    if host.shape != (3, 2):
        raise ValueError("ranges must be three pairs {vmin, vmax}: the signed distance, the temperature and the speed")
    return host.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else host.to(device)


def _columns(channels) -> list:
    sdf, temp, velx, vely = (-1 if c is None else int(c) for c in channels)
    return [q for q, present in enumerate((sdf >= 0, temp >= 0, velx >= 0 and vely >= 0)) if present]


def _clip(x: torch.Tensor, who: str) -> torch.Tensor:
    if x.dim() != 4:
        raise ValueError(f"{who} must be (frames, channels, H, W), got {tuple(x.shape)}")
    return x.float().contiguous()


def render_panels(pred: torch.Tensor, target: torch.Tensor, ranges, spec: RenderSpec = RenderSpec(), channels=(0, 1, 2, 3)) -> torch.Tensor:
    """pred, target (F, C, H, W) on the device -> (F, img_h, img_w, 3) uint8 on the device: per frame the simulation on top and the prediction
    below, one column per quantity whose channels are present (``channels`` = (sdf, temperature, velx, vely), None or -1 for an absent field).
    ranges: {vmin, vmax} per quantity, a (3, 2) tensor or sequence.  The arrows of BOTH rows vanish where the simulation's signed distance is
    positive (plot_utils.py:103-106).  One launch, no synchronisation."""
    from .. import _lib as L, ops
    pred, target = _clip(pred, "pred"), _clip(target, "target")
    if pred.shape != target.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} differ")
    cols = _columns(channels)
    if not cols:
        raise ValueError("none of the three quantities has its channels")
    sdf, temp, velx, vely = (-1 if c is None else int(c) for c in channels)
    rng = _range_tensor(ranges, pred.device)
    F, _, H, W = pred.shape
    layout = spec.layout(H, W, 2, len(cols))
    view = lambda x, c: x[:, c].unsqueeze(1)
    tiles = []
    for x in (target, pred):
        for q in cols:
            if q == 0:
                tiles.append({"kind": L.BF_RENDER_SDF, "a": view(x, sdf), "range": rng[0]})
            elif q == 1:
                tiles.append({"kind": L.BF_RENDER_TEMP, "a": view(x, temp), "range": rng[1]})
            else:
                tiles.append({"kind": L.BF_RENDER_SPEED, "a": view(x, velx), "b": view(x, vely), "mask": view(target, sdf) if sdf >= 0 else None,
                              "range": rng[2]})
    return ops.render_tiles(tiles, layout, F)


def render_strip(frames: torch.Tensor, quantity: str, vrange=None, spec: RenderSpec = RenderSpec()) -> torch.Tensor:
    """T frames of one quantity side by side -> (img_h, img_w, 3) uint8 on the device.  frames: (T, H, W) for "sdf" and "temperature",
    (T, 2, H, W) for "velocity".  vrange: (vmin, vmax); None scales to the frames' own minimum and maximum, as imshow does (taken on the
    device: nothing synchronises)."""
    from .. import _lib as L, ops
    if quantity not in QUANTITIES:
        raise ValueError(f"quantity must be one of {QUANTITIES}")
    q = QUANTITIES.index(quantity)
    want = 4 if q == 2 else 3
    if frames.dim() != want or (q == 2 and frames.shape[1] != 2):
        raise ValueError(f"a {quantity} strip takes {'(T, 2, H, W)' if q == 2 else '(T, H, W)'} frames, got {tuple(frames.shape)}")
    x = frames.float().contiguous()
    x = x if q == 2 else x.unsqueeze(1)                  # (T, C, H, W)
    T, _, H, W = x.shape
    if vrange is None:
        stats = ops.render_ranges(x, [(0, -1, -1, -1), (-1, 0, -1, -1), (-1, -1, 0, 1)][q])
        rng = stats[q, 3:5]                              # {min, max} lie side by side
    else:
        rng = _range_tensor([vrange if k == q else None for k in range(3)], x.device)[q]
    slot = lambda c: x[:, c].unsqueeze(0)                # (1, T, H, W): one image, T rounds through one description
    tile = {"kind": (L.BF_RENDER_SDF, L.BF_RENDER_TEMP, L.BF_RENDER_SPEED)[q], "a": slot(0), "range": rng}
    if q == 2:
        tile["b"] = slot(1)
    return ops.render_tiles([tile], spec.layout(H, W, 1, T), 1)[0]


def sdf_strip(sdf: torch.Tensor, vrange=None, spec: RenderSpec = RenderSpec()) -> torch.Tensor:
    """wandb_sdf_plotter: a (T, H, W) signed distance as one picture strip with the interface outlined."""
    return render_strip(sdf, "sdf", vrange, spec)


def temp_strip(temp: torch.Tensor, vrange=None, spec: RenderSpec = RenderSpec()) -> torch.Tensor:
    """wandb_temp_plotter: a (T, H, W) temperature."""
    return render_strip(temp, "temperature", vrange, spec)


def vel_strip(vel: torch.Tensor, vrange=None, spec: RenderSpec = RenderSpec()) -> torch.Tensor:
    """wandb_vel_plotter: a (T, 2, H, W) velocity as its speed with arrows (the strips have no interface to hide arrows behind)."""
    return render_strip(vel, "velocity", vrange, spec)


def write_strip(path, image: torch.Tensor, name: str, layout: RenderLayout, vrange=None) -> None:
    """A strip from ``*_strip`` to a PNG file with its titles ("SDF 0", "TEMP 1", ...); ``layout`` = spec.layout(H, W, 1, T).  The end
    values are stamped when ``vrange`` is given (a strip scaled to its own data keeps them on the device)."""
    host = png.to_host(image).copy()
    if host.shape[:2] != (layout.img_h, layout.img_w):
        raise ValueError(f"the image is {host.shape[:2]}, the layout {(layout.img_h, layout.img_w)}")
    for t in range(layout.cols):
        y0, x0 = layout.tile_origin(0, t)
        stamp_text(host, y0 - layout.title_h + 1, x0, f"{name} {t}", x0 + layout.bar_dx + layout.bar_w)
    if vrange is not None:
        stamp_labels(host, layout, [""] * layout.cols, [vrange] * layout.cols)
    png.write_png(path, host)


# ---------------------------------------------------------------------------------------------------------------- the reference's entry point
def reference_ranges(stats: np.ndarray) -> list:
    """plot_utils.py:49-57 from bf_render_ranges' rows {n, sum, sum of squares, min, max}: (round(mean - 3 std, 2), round(mean + 3 std, 2))
    with the unbiased standard deviation, per quantity; None for a quantity that was skipped."""
    out = []
    for n, s1, s2, _, _ in np.asarray(stats, dtype=np.float64):
        if n == 0:
            out.append(None)
            continue
        mean = s1 / n
        std = np.sqrt(max(s2 - s1 * s1 / n, 0.0) / (n - 1)) if n > 1 else float("nan")
        out.append((round(float(mean - 3 * std), 2), round(float(mean + 3 * std), 2)))
    return out


PANEL_NAMES = ("SDF", "TEMP", "VEL")


def panel_titles(cols: Sequence[int], i: int) -> list:
    return [f"{PANEL_NAMES[q]} {row} {i}" for row in ("LABEL", "PRED") for q in cols]


def plot_bubbleml(preds: torch.Tensor, targets: torch.Tensor, timesteps, save_dir, *, spec: RenderSpec = RenderSpec(), channels=(0, 1, 2, 3),
                  apng: bool = False, vmin=None, vmax=None, fps: float = 10.0, workers: int = 8, chunk: int = 256) -> dict:
    """The reference's ``plot_bubbleml(preds, targets, timesteps, save_dir)`` for (T, C, H, W) clips on the device.

    Writes ``save_dir/plots/0000.png ...`` (one 2 x 3 panel per frame), with ``apng`` also ``plots/rollout.png``, and
    ``relative_l2_error.csv`` (a row per frame: the time step and the relative L2 error of every channel, plot_utils.py:30-34; the line chart
    itself is not drawn).  The colour ranges are the reference's, from the TARGETS: round(mean -+ 3 std, 2); ``vmin`` / ``vmax`` (three values:
    signed distance, temperature, speed) replace them.  A range that is not finite raises ValueError.  Frames go through the device ``chunk`` at a
    time.  Returns {"ranges", "files", "seconds": {"kernel", "copy", "compress"}} (kernel: host time until the device has finished rendering)."""
    import time
    from .. import ops
    from .rollout import relative_l2_per_frame
    preds, targets = _clip(preds, "preds"), _clip(targets, "targets")
    if preds.shape != targets.shape:
        raise ValueError(f"preds {tuple(preds.shape)} and targets {tuple(targets.shape)} differ")
    F, _, H, W = preds.shape
    steps = [int(t) for t in (timesteps.tolist() if isinstance(timesteps, torch.Tensor) else timesteps)]
    if len(steps) != F:
        raise ValueError(f"{len(steps)} time steps for {F} frames")
    cols = _columns(channels)
    ch = [-1 if c is None else int(c) for c in channels]
    if vmin is None or vmax is None:
        ranges = reference_ranges(ops.render_ranges(targets, ch).cpu().numpy())
    else:
        ranges = [(float(a), float(b)) if q in cols else None for q, (a, b) in enumerate(zip(vmin, vmax))]
    for q in cols:
        if not all(np.isfinite(v) for v in ranges[q]):
            raise ValueError(f"the colour range of the {QUANTITIES[q]} is not finite: {ranges[q]} (pass vmin / vmax)")
    plot_dir = os.path.join(str(save_dir), "plots")
    os.makedirs(plot_dir, exist_ok=True)
    err = relative_l2_per_frame(preds, targets).cpu().numpy()
    with open(os.path.join(str(save_dir), "relative_l2_error.csv"), "w") as f:
        f.write("timestep," + ",".join(f"channel_{c}" for c in range(err.shape[1])) + "\n")
        for t, row in zip(steps, err):
            f.write(f"{t}," + ",".join(f"{float(v):.9g}" for v in row) + "\n")
    layout = spec.layout(H, W, 2, len(cols))
    slot_ranges = [ranges[q] for _ in range(2) for q in cols]
    rng = _range_tensor(ranges, preds.device)
    files, kept, seconds = [], [], {"kernel": 0.0, "copy": 0.0, "compress": 0.0}
    for lo in range(0, F, max(1, int(chunk))):
        hi = min(F, lo + max(1, int(chunk)))
        t0 = time.perf_counter()
        dev = render_panels(preds[lo:hi], targets[lo:hi], rng, spec, channels)
        torch.cuda.current_stream(dev.device).synchronize()
        t1 = time.perf_counter()
        host = png.to_host(dev)
        t2 = time.perf_counter()
        for k in range(hi - lo):
            stamp_labels(host[k], layout, panel_titles(cols, lo + k), slot_ranges)
        paths = [os.path.join(plot_dir, f"{i:04d}.png") for i in range(lo, hi)]
        png.write_pngs(paths, host, workers=workers)
        if apng:
            kept.extend(host[k].copy() for k in range(hi - lo))
        files.extend(paths)
        seconds["kernel"] += t1 - t0
        seconds["copy"] += t2 - t1
        seconds["compress"] += time.perf_counter() - t2
    if apng:
        files.append(os.path.join(plot_dir, "rollout.png"))
        png.write_apng(files[-1], kept, fps, workers=workers)
    return {"ranges": ranges, "files": files, "seconds": seconds}
