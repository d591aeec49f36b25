"""The renderer's host side, without a GPU: colour tables, the colour rule against matplotlib, PNG / APNG files, layout, and the numpy
restatement (tests/render_restatement.py) on hand-made fields."""
import os
import struct
import zlib

import numpy as np
import pytest

from tests import render_restatement as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")

SHAPES = [(1, 1), (1, 8), (2, 3), (5, 8), (7, 22), (16, 16), (31, 64), (64, 64)]
SCALES = [1, 2, 3, 5]


def _luts():
    z = np.load(os.path.join(GOLDEN, "colormaps.npz"))
    return z["Blues"], z["turbo"]


def test_colour_tables_equal_the_recorded_ones():
    from bubbleformer_amd.utils import colormaps
    blues, turbo = _luts()
    assert colormaps.BLUES.dtype == np.uint8 and colormaps.BLUES.shape == (256, 3) and colormaps.TURBO.shape == (256, 3)
    assert np.array_equal(colormaps.BLUES, blues) and np.array_equal(colormaps.TURBO, turbo)
    assert not colormaps.BLUES.flags.writeable


def test_colour_tables_equal_matplotlibs():
    mpl = pytest.importorskip("matplotlib")
    from bubbleformer_amd.utils import colormaps
    for name, table in (("Blues", colormaps.BLUES), ("turbo", colormaps.TURBO)):
        assert np.array_equal(mpl.colormaps[name](np.arange(256), bytes=True)[:, :3], table), name


def test_colour_rule_equals_matplotlibs_on_fp32_values():
    """20,000 seeded fp32 values, a tenth of them beyond the range ends and both ends themselves among them: the restatement's fp64 index
    gives the bytes of cmap(Normalize(vmin, vmax)(x), bytes=True) with no mismatch."""
    mpl = pytest.importorskip("matplotlib")
    from matplotlib.colors import Normalize
    rng = np.random.default_rng(20)
    vmin, vmax = -0.37, 1.21
    x = rng.uniform(vmin - 0.08, vmax + 0.08, 20000).astype(np.float32)
    x[:4] = np.float32(vmin), np.float32(vmax), np.nextafter(np.float32(vmax), np.float32(2)), np.nextafter(np.float32(vmin), np.float32(-2))
    for name, lut in zip(("Blues", "turbo"), _luts()):
        want = mpl.colormaps[name](Normalize(vmin, vmax)(x), bytes=True)[:, :3]
        got = R.colour_tile(x, vmin, vmax, lut)
        print(name, "mismatches:", int((got != want).any(axis=1).sum()))
        assert np.array_equal(got, want), name
    assert np.array_equal(R.colour_tile(np.float32([0.3, np.nan, 9.0]), 2.0, 2.0, _luts()[1]), np.repeat(_luts()[1][:1], 3, axis=0))     # vmax == vmin: index 0
    ends = R.colour_tile(np.float32([np.nan, np.inf, -np.inf]), 0.0, 1.0, _luts()[1])
    assert np.array_equal(ends, np.stack([R.WHITE, _luts()[1][255], _luts()[1][0]]))


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (186, 600)])
def test_png_round_trip(tmp_path, shape):
    from bubbleformer_amd.utils.png import read_chunks, read_png, write_png
    img = np.random.default_rng(shape[0]).integers(0, 256, shape + (3,), dtype=np.uint8)
    path = tmp_path / "a.png"
    write_png(path, img)
    assert np.array_equal(read_png(path), img)
    kinds = [k for k, _ in read_chunks(path)]                     # read_chunks verifies every CRC
    assert kinds == [b"IHDR", b"IDAT", b"IEND"]
    raw = bytearray(path.read_bytes())
    raw[40] ^= 1                                                  # a flipped bit inside IDAT: its CRC no longer matches
    (tmp_path / "b.png").write_bytes(bytes(raw))
    with pytest.raises(ValueError, match="CRC"):
        read_png(tmp_path / "b.png")
    with pytest.raises(ValueError):
        write_png(path, img.astype(np.float32))


def test_png_is_read_by_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from bubbleformer_amd.utils.png import write_apng, write_png
    img = np.random.default_rng(3).integers(0, 256, (37, 52, 3), dtype=np.uint8)
    write_png(tmp_path / "a.png", img)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "a.png").convert("RGB")), img)
    frames = [np.roll(img, k, axis=0) for k in range(3)]
    write_apng(tmp_path / "b.png", frames, fps=5)
    with Image.open(tmp_path / "b.png") as im:
        assert getattr(im, "n_frames", 1) == 3
        for k in range(3):
            im.seek(k)
            assert np.array_equal(np.asarray(im.convert("RGB")), frames[k]), k


def test_apng_chunks_and_worker_counts(tmp_path):
    from bubbleformer_amd.utils.png import read_chunks, read_png, write_apng, write_pngs
    rng = np.random.default_rng(4)
    frames = [rng.integers(0, 256, (20, 24, 3), dtype=np.uint8) for _ in range(5)]
    for workers in (1, 16, 99):                                   # 99 is capped at 16
        write_apng(tmp_path / f"w{workers}.png", frames, fps=12.5, workers=workers)
        d = tmp_path / f"d{workers}"
        d.mkdir()
        write_pngs([d / f"{k}.png" for k in range(5)], frames, workers=workers)
    one = (tmp_path / "w1.png").read_bytes()
    assert one == (tmp_path / "w16.png").read_bytes() == (tmp_path / "w99.png").read_bytes()
    for k in range(5):
        assert (tmp_path / "d1" / f"{k}.png").read_bytes() == (tmp_path / "d16" / f"{k}.png").read_bytes()
        assert np.array_equal(read_png(tmp_path / "d16" / f"{k}.png"), frames[k])
    chunks = read_chunks(tmp_path / "w1.png")
    kinds = [k for k, _ in chunks]
    assert kinds == [b"IHDR", b"acTL", b"fcTL", b"IDAT"] + [b"fcTL", b"fdAT"] * 4 + [b"IEND"]
    assert struct.unpack(">II", chunks[1][1]) == (5, 0)
    seq = [struct.unpack(">I", d[:4])[0] for k, d in chunks if k in (b"fcTL", b"fdAT")]
    assert seq == list(range(9))
    assert struct.unpack(">IIIIIHHBB", chunks[2][1])[1:7] == (24, 20, 0, 0, 80, 1000)          # 12.5 frames per second
    got = read_png(tmp_path / "w1.png", all_frames=True)
    assert len(got) == 5 and all(np.array_equal(a, b) for a, b in zip(got, frames))
    assert zlib.crc32(b"IEND") & 0xFFFFFFFF == struct.unpack(">I", one[-4:])[0]


@pytest.mark.parametrize("rows,cols", [(2, 3), (2, 1), (1, 1), (1, 4)])
def test_layout_matches_the_restatement_and_tiles_do_not_overlap(rows, cols):
    from bubbleformer_amd.utils.plot_utils import RenderSpec
    for H, W in SHAPES:
        for s in SCALES:
            for stride in (1, 8):
                g = RenderSpec(scale=s, stride=stride).layout(H, W, rows, cols)
                want = R.layout(H, W, s, rows, cols, stride)
                assert {k: getattr(g, k) for k in want} == want
                assert g.img_w % 4 == 0
                taken = np.zeros((g.img_h, g.img_w), dtype=np.int32)
                for r in range(rows):
                    for c in range(cols):
                        y0, x0 = g.tile_origin(r, c)
                        assert y0 - g.title_h >= 0 and x0 >= 0 and y0 + H * s <= g.img_h and x0 + g.bar_dx + g.bar_w + g.label_w <= g.img_w
                        taken[y0 - g.title_h:y0 + H * s, x0:x0 + W * s] += 1                              # the tile and its title
                        taken[y0:y0 + H * s, x0 + g.bar_dx:x0 + g.bar_dx + g.bar_w + g.label_w] += 1      # the bar and its end values
                assert taken.max() == 1
    with pytest.raises(ValueError):
        RenderSpec(scale=0).layout(4, 4)


def test_outline_on_a_hand_made_field():
    sdf = np.ones((5, 5), dtype=np.float32)
    sdf[0:2, 0:2] = -1.0                       # a liquid corner block: every one of its cells touches vapour or is next to one that does
    edge = R.edge_cells(sdf)
    want_edge = np.zeros((5, 5), dtype=bool)
    want_edge[0, 1] = want_edge[1, 0] = want_edge[1, 1] = True        # (0, 0) has only liquid neighbours in range
    assert np.array_equal(edge, want_edge)
    want = np.zeros((5, 5), dtype=bool)
    want[0:3, 0:3] = True
    assert np.array_equal(R.outline(sdf), want)
    assert not R.outline(-np.ones((5, 5), dtype=np.float32)).any()    # all liquid: the border of the field is no interface
    assert not R.outline(np.ones((5, 5), dtype=np.float32)).any()
    nan = -np.ones((5, 5), dtype=np.float32)
    nan[4, 4] = np.nan                         # a NaN is not liquid
    assert R.edge_cells(nan).sum() == 2 and R.outline(nan)[3:, 3:].all() and R.outline(nan).sum() == 8
    # row 0 of the field is the bottom row of the picture
    img, _ = R.tile(R.SDF, sdf, None, None, -2.0, 2.0, R.layout(5, 5, 2), _luts())
    assert (img[-6:, :6] == 0).all() and (img[:4] != 0).any(axis=2).all()


def test_arrow_on_a_hand_made_field():
    """One anchor at cell (2, 2) of a 5 x 5 field (stride 5), u = vmax to the right: the shaft lies on the anchor's pixel row from
    c - l/2 to c + l/2 with l = 0.9 * 5 * s."""
    s, stride = 4, 5
    u, v = np.zeros((5, 5), dtype=np.float32), np.zeros((5, 5), dtype=np.float32)
    u[2, 2] = 2.0
    lay = R.layout(5, 5, s, stride=stride)
    d = R.arrow_distance(u, v, None, s, stride, 2.0)
    cx = cy = 2.5 * s
    ln = 0.9 * stride * s
    assert d[int(cy), int(cx)] == pytest.approx(0.5) and d[int(cy), 5] == pytest.approx(0.5)       # pixel centres half a pixel off the axis
    assert d[int(cy), int(cx + ln / 2)] == pytest.approx(np.hypot(0.5, 0.5)) and d[int(cy), 0] == pytest.approx(np.hypot(0.5, 0.5))
    strokes = R.arrow_strokes(2.0, 0.0, 2.0, cx, cy, ln)
    assert strokes[0] == (cx - ln / 2, cy, cx + ln / 2, cy)
    for (_, _, bx, by), sign in zip(strokes[1:], (1, -1)):                                  # the head: 0.35 l long, back from the tip, either side
        assert np.hypot(bx - strokes[0][2], by - cy) == pytest.approx(0.35 * ln) and bx < strokes[0][2] and np.sign(by - cy) == sign
    img, band = R.tile(R.SPEED, u, v, None, 0.0, 2.0, lay, _luts())
    assert (img[int(cy), int(cx - ln / 2) + 1:int(cx + ln / 2)] == 255).all() and not band.any()
    # v upwards in the field is upwards on the screen (smaller row)
    up = R.arrow_strokes(0.0, 1.0, 2.0, cx, cy, ln)[0]
    assert up[3] < up[1] and up[0] == up[2]
    # a positive mask at the anchor, a zero velocity and vmax <= 0 give no arrow; half the speed half the length
    mask = np.where(u > 0, 1.0, -1.0).astype(np.float32)
    assert np.isinf(R.arrow_distance(u, v, mask, s, stride, 2.0)).all() and np.isinf(R.arrow_distance(v, v, None, s, stride, 2.0)).all()
    assert np.isinf(R.arrow_distance(u, v, None, s, stride, 0.0)).all()
    assert R.arrow_strokes(1.0, 0.0, 2.0, cx, cy, ln)[0] == (cx - ln / 4, cy, cx + ln / 4, cy)
    assert np.isinf(R.arrow_distance(u, v, None, s, 12, 2.0)).all()                         # stride / 2 = 6 lies outside the field: no anchor


def test_glyphs_cover_the_titles_and_values():
    from bubbleformer_amd.utils import plot_utils as P
    assert set("0123456789-.+ ") | set("SDFTEMPVELLABELPRED") == set(P.GLYPHS)
    assert all(g.shape == (7, 5) and (g.any() or ch == " ") for ch, g in P.GLYPHS.items())
    assert len({g.tobytes() for g in P.GLYPHS.values()}) == len(P.GLYPHS)
    img = np.full((12, 40, 3), 255, dtype=np.uint8)
    P.stamp_text(img, 2, 1, "VEL 7", x_end=20)
    ink = (img == 0).all(axis=2)
    assert ink[2:9, 1:6].sum() == P.GLYPHS["V"].sum() and not ink[:, 20:].any() and not ink[:2].any() and not ink[9:].any()
    P.stamp_text(img, 8, 36, "8")                                  # runs off two edges: clipped, no error
    assert P.end_value(-1.005) == "-1.00" and P.end_value(float("nan")) == "-"
    assert P.reference_ranges(np.array([[4.0, 10.0, 30.0, 1.0, 4.0], [0.0, 0.0, 0.0, np.inf, -np.inf]])) == [
        (round(2.5 - 3 * np.sqrt(5.0 / 3.0), 2), round(2.5 + 3 * np.sqrt(5.0 / 3.0), 2)), None]
