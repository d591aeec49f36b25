"""The definition of the training step's input noise, restated on the host in numpy with fp64 functions: Philox4x32-10 (Random123's
constants), the counter layout and the Box-Muller map of include/bubbleformer_hip.h: bf_clip_noise.  Nothing of the device code."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
Z_MAX = 5.77            # sqrt(-2 ln 2^-24) = sqrt(48 ln 2) = 5.768


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: (k0, k1) ints -> four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(MASK), p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [v.astype(np.uint32) for v in c]


def box_muller(a, b):
    """A word pair -> (z0, z1, r) in fp64."""
    u1 = ((a >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24          # (0, 1]
    two_u2 = (b >> np.uint32(8)).astype(np.float64) * 2.0 ** -23               # 2 u2 in [0, 2), exact
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(np.pi * two_u2), r * np.sin(np.pi * two_u2), r


def normals(seed, sample_id, draw, pass_index, n):
    """The n normals of one sample's flattened clip, and the Box-Muller radius behind each: (z [n], r [n]) in fp64."""
    groups = (n + 3) // 4
    seed = int(seed) & (2 ** 64 - 1)
    w = philox4x32_10((np.arange(groups, dtype=np.uint64), int(sample_id) & MASK, int(draw) & MASK, int(pass_index) & MASK), (seed & MASK, seed >> 32))
    z0, z1, ra = box_muller(w[0], w[1])
    z2, z3, rb = box_muller(w[2], w[3])
    z = np.stack([z0, z1, z2, z3], axis=1).reshape(-1)[:n]
    r = np.stack([ra, ra, rb, rb], axis=1).reshape(-1)[:n]
    return z, r


def noisy_clip(x, sigma, sample_ids, draw, pass_index, seed):
    """x (B, T, C, H, W) -> (x + sigma[c] z in fp64, r, sigma per element), all of x's shape; sample_ids None numbers the rows."""
    x = np.asarray(x, dtype=np.float64)
    B, T, C, H, W = x.shape
    ids = range(B) if sample_ids is None else sample_ids
    sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64).reshape(1, 1, C, 1, 1), x.shape)
    z, r = zip(*[normals(seed, ids[b], draw, pass_index, T * C * H * W) for b in range(B)])
    z, r = np.stack(z).reshape(x.shape), np.stack(r).reshape(x.shape)
    return x + sig * z, r, sig


def element_bound(want, r, sig, K):
    """|got - want| <= sigma K 2^-23 max(r, 1) + 2^-24 |want|: K ulps of the fp32 Box-Muller chain on a normal of radius r, and the final
    rounding of the fused multiply-add."""
    return sig * K * 2.0 ** -23 * np.maximum(r, 1.0) + 2.0 ** -24 * np.abs(want)


def needed_K(got, want, r, sig):
    """The smallest K with which element_bound holds everywhere (0 where sigma is 0)."""
    slack = np.abs(np.asarray(got, dtype=np.float64) - want) - 2.0 ** -24 * np.abs(want)
    den = sig * 2.0 ** -23 * np.maximum(r, 1.0)
    ok = den > 0
    return float(np.max(np.where(ok, slack / np.where(ok, den, 1.0), 0.0), initial=0.0))


def moment_statistics(z):
    """mean sqrt N, (var - 1) sqrt(N / 2), skew sqrt(N / 6), (kurtosis - 3) sqrt(N / 24), lag-1 product mean sqrt N: each a standard
    normal variable for independent standard normals."""
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    N = z.size
    m, v = z.mean(), z.var()
    s = (z - m) / np.sqrt(v)
    return {"mean": m * np.sqrt(N), "var": (v - 1.0) * np.sqrt(N / 2.0), "skew": (s ** 3).mean() * np.sqrt(N / 6.0),
            "kurtosis": ((s ** 4).mean() - 3.0) * np.sqrt(N / 24.0), "lag1": (z[:-1] * z[1:]).mean() * np.sqrt(N - 1)}
