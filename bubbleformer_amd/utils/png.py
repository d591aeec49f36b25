"""PNG and APNG files from uint8 RGB images, with the standard library alone (``zlib`` and ``struct``).

A rendered batch leaves the device in one copy through pinned memory (``to_host``) and is compressed by a small thread pool
(``write_pngs``: ``zlib`` releases the GIL while it works).  Every scanline is written with filter 0, so ``read_png`` -- the reader the tests
use -- only has to strip one byte per row."""
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor
from typing import List, Sequence

import numpy as np

_SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_WORKERS = 16


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def _check(image) -> np.ndarray:
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"an image is a (height, width, 3) uint8 array, got {a.dtype} {a.shape}")
    return a


def _ihdr(a: np.ndarray) -> bytes:
    return _chunk(b"IHDR", struct.pack(">IIBBBBB", a.shape[1], a.shape[0], 8, 2, 0, 0, 0))        # 8 bits, colour type 2 (RGB), no interlace


def _deflate(a: np.ndarray, level: int) -> bytes:
    """The zlib stream of the image's scanlines, each behind a filter byte of 0."""
    rows = np.zeros((a.shape[0], 1 + a.shape[1] * 3), dtype=np.uint8)
    rows[:, 1:] = a.reshape(a.shape[0], -1)
    return zlib.compress(rows.tobytes(), level)


def encode_png(image, level: int = 1) -> bytes:
    a = _check(image)
    return _SIGNATURE + _ihdr(a) + _chunk(b"IDAT", _deflate(a, level)) + _chunk(b"IEND", b"")


def write_png(path, image, level: int = 1) -> None:
    with open(path, "wb") as f:
        f.write(encode_png(image, level))


def _workers(workers: int) -> int:
    return max(1, min(int(workers), MAX_WORKERS))


def write_pngs(paths: Sequence, images: Sequence, level: int = 1, workers: int = 8) -> None:
    """One file per image; compression in ``workers`` threads (at most 16).  The bytes do not depend on the number of workers."""
    if len(paths) != len(images):
        raise ValueError(f"{len(paths)} paths for {len(images)} images")
    with ThreadPoolExecutor(_workers(workers)) as pool:
        list(pool.map(lambda job: write_png(job[0], job[1], level), zip(paths, images)))


def write_apng(path, frames: Sequence, fps: float, level: int = 1, workers: int = 8) -> None:
    """An animated PNG that loops for ever: the first frame is also the still image a plain PNG reader shows."""
    frames = [_check(f) for f in frames]
    if not frames or any(f.shape != frames[0].shape for f in frames):
        raise ValueError("an animation needs at least one frame, all of one size")
    if not fps > 0:
        raise ValueError("fps must be positive")
    den = 1000
    num = max(1, min(65535, int(round(den / float(fps)))))
    with ThreadPoolExecutor(_workers(workers)) as pool:
        streams = list(pool.map(lambda f: _deflate(f, level), frames))
    h, w = frames[0].shape[:2]
    out = [_SIGNATURE, _ihdr(frames[0]), _chunk(b"acTL", struct.pack(">II", len(frames), 0))]
    seq = 0
    for k, data in enumerate(streams):
        out.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, 0, 0, num, den, 0, 0)))
        seq += 1
        if k == 0:
            out.append(_chunk(b"IDAT", data))
        else:
            out.append(_chunk(b"fdAT", struct.pack(">I", seq) + data))
            seq += 1
    out.append(_chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(b"".join(out))


def read_chunks(path) -> List[tuple]:
    """[(type, data)] of a PNG file; raises on a bad signature, a truncated chunk or a CRC that does not match."""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:8] != _SIGNATURE:
        raise ValueError(f"{path}: not a PNG file")
    at, chunks = 8, []
    while at < len(raw):
        if at + 12 > len(raw):
            raise ValueError(f"{path}: truncated chunk")
        (n,) = struct.unpack(">I", raw[at:at + 4])
        kind, data = raw[at + 4:at + 8], raw[at + 8:at + 8 + n]
        if len(data) != n or at + 12 + n > len(raw):
            raise ValueError(f"{path}: truncated chunk")
        (crc,) = struct.unpack(">I", raw[at + 8 + n:at + 12 + n])
        if crc != zlib.crc32(kind + data) & 0xFFFFFFFF:
            raise ValueError(f"{path}: bad CRC in a {kind!r} chunk")
        chunks.append((kind, data))
        at += 12 + n
    return chunks


def _unfilter(data: bytes, h: int, w: int, where) -> np.ndarray:
    rows = np.frombuffer(zlib.decompress(data), dtype=np.uint8)
    if rows.size != h * (1 + 3 * w):
        raise ValueError(f"{where}: {rows.size} bytes of image data for {w} x {h} RGB")
    rows = rows.reshape(h, 1 + 3 * w)
    if rows[:, 0].any():
        raise ValueError(f"{where}: only filter 0 is read")
    return rows[:, 1:].reshape(h, w, 3).copy()


def read_png(path, all_frames: bool = False):
    """The (height, width, 3) uint8 image of an 8-bit RGB file whose scanlines all use filter 0 -- what this module writes.  With
    ``all_frames`` the list of frames of an animation (full-size frames only)."""
    chunks = read_chunks(path)
    if not chunks or chunks[0][0] != b"IHDR" or chunks[-1][0] != b"IEND":
        raise ValueError(f"{path}: IHDR must come first and IEND last")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    if (depth, colour, comp, filt, lace) != (8, 2, 0, 0, 0):
        raise ValueError(f"{path}: only 8-bit RGB without interlace is read")
    first = _unfilter(b"".join(d for k, d in chunks if k == b"IDAT"), h, w, path)
    if not all_frames:
        return first
    frames, later = [first], []
    for k, d in chunks:
        if k == b"fcTL" and later:
            frames.append(_unfilter(b"".join(later), h, w, path))
            later = []
        elif k == b"fdAT":
            later.append(d[4:])
    if later:
        frames.append(_unfilter(b"".join(later), h, w, path))
    return frames


def to_host(images) -> np.ndarray:
    """A device tensor as a numpy array in ONE device-to-host copy through pinned memory (a host tensor is passed through)."""
    import torch
    if not isinstance(images, torch.Tensor):
        return np.asarray(images)
    if images.device.type == "cpu":
        return images.numpy()
    host = torch.empty(images.shape, dtype=images.dtype, pin_memory=True)
    host.copy_(images.contiguous(), non_blocking=True)
    torch.cuda.current_stream(images.device).synchronize()
    return host.numpy()
