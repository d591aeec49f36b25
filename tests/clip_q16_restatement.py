"""The 16-bit clip store's format, restated in numpy from its description (csrc/clip_store_q16.hip's header comment):
segment scales, encode, decode, the error bound, a whole store's codes, and a plain gather composed from them.  Every operation is one
np.float32 operation (numpy never fuses), so the device kernels are held to these bits."""
import numpy as np

F32 = np.float32


def scales(x):
    """(lo, hi, step, inv) of one segment: the exact fp32 extremes; the two quotients in fp64, rounded to fp32 once; all-zero scales when constant."""
    x = np.asarray(x, dtype=F32)
    lo, hi = F32(x.min()), F32(x.max())
    span = float(hi) - float(lo)
    if span == 0.0:
        return lo, hi, F32(0.0), F32(0.0)
    return lo, hi, F32(span / 65535.0), F32(65535.0 / span)


def encode(x, lo, inv):
    """code = clamp(rint((x - lo) * inv), 0, 65535): an fp32 difference, an fp32 product, round half to even."""
    x = np.asarray(x, dtype=F32)
    diff = x - F32(lo)
    q = diff * F32(inv)
    assert diff.dtype == F32 and q.dtype == F32
    return np.clip(np.rint(q), F32(0.0), F32(65535.0)).astype(np.uint16)


def decode(code, lo, step):
    """x^ = fp32(fp32(code * step) + lo): a rounded product, then a rounded sum."""
    prod = np.asarray(code).astype(F32) * F32(step)
    out = prod + F32(lo)
    assert prod.dtype == F32 and out.dtype == F32
    return out


def bound(lo, hi, step):
    """|x^ - x| <= 0.53 step + 2^-24 max(|lo|, |hi|), in fp64: half a step, six fp32 roundings of at most 0.004 step each, the final sum's rounding."""
    return 0.53 * float(step) + 2.0 ** -24 * max(abs(float(lo)), abs(float(hi)))


def store(trajectories, fields):
    """The whole store of a list of {field: [frames][H][W]} trajectories: codes [fields][total frames][H][W] uint16 (files concatenated on
    the frame axis), lo / hi / step [fields][files] fp32, and frame_seg [total frames] = the file of every frame."""
    nfile = len(trajectories)
    lo, hi, step = (np.zeros((len(fields), nfile), dtype=F32) for _ in range(3))
    codes = []
    for ci, name in enumerate(fields):
        parts = []
        for fi, t in enumerate(trajectories):
            x = np.asarray(t[name], dtype=F32)
            lo[ci, fi], hi[ci, fi], step[ci, fi], inv = scales(x)
            parts.append(encode(x, lo[ci, fi], inv))
        codes.append(np.concatenate(parts))
    frame_seg = np.repeat(np.arange(nfile, dtype=np.int32), [len(t[fields[0]]) for t in trajectories])
    return np.stack(codes), lo, hi, step, frame_seg


def decode_store(codes, lo, step, frame_seg):
    """The fp32 frames a store decodes to: every frame under the scale of its own file."""
    out = np.empty(codes.shape, dtype=F32)
    for ci in range(codes.shape[0]):
        for fr in range(codes.shape[1]):
            out[ci, fr] = decode(codes[ci, fr], lo[ci, frame_seg[fr]], step[ci, frame_seg[fr]])
    return out


def nearest(n_out, n_in):
    """Source indices of F.interpolate(mode="nearest"): floor(dst * fp32(in / out)) held to in - 1; the identity at full resolution."""
    if n_out == n_in:
        return np.arange(n_in)
    scale = F32(n_in) / F32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=F32) * scale).astype(np.int64), n_in - 1)


def gather(codes, lo, step, frame_seg, first, t0, T, field_ids, diff, div, Ho, Wo):
    """(B, T, C, Ho, Wo): out[b][t][c] = (x^[field_ids[c]][min(first[b] + t0 + t, last frame)][ys][xs] - diff[c]) / div[c] in fp32, the scale
    that of the frame read."""
    nframes, H, W = codes.shape[1:]
    ys, xs = nearest(Ho, H), nearest(Wo, W)
    out = np.empty((len(first), T, len(field_ids), Ho, Wo), dtype=F32)
    for b, f0 in enumerate(first):
        for t in range(T):
            fr = min(int(f0) + t0 + t, nframes - 1)
            for c, fid in enumerate(field_ids):
                x = decode(codes[fid, fr][np.ix_(ys, xs)], lo[fid, frame_seg[fr]], step[fid, frame_seg[fr]])
                out[b, t, c] = (x - F32(diff[c])) / F32(div[c])
    return out
