"""A plain numpy restatement of redistancing as DESIGN.md section 25 defines it (the reference has no program for it), twice: Gauss-Seidel fast
sweeping in the four diagonal orders, cell by cell, and vectorised red-black (checkerboard) passes, cells with even x + y first -- the order
csrc/redistance.hip visits them in, so its pass count is comparable.  Both take the monotone scheme to its fixed point, which does not depend on
the visiting order apart from rounding.  fp64 by default; ``dtype=np.float32`` runs the red-black copy in the kernel's own unfused fp32
operations.  Also the test fields."""
import numpy as np


def vapour(phi):
    """The sign convention: vapour iff phi > 0, an exact zero is liquid."""
    return np.asarray(phi) > 0


def interface_cells(phi):
    """Cells with a 4-neighbour inside the frame of the other sign."""
    s = vapour(phi)
    m = np.zeros(s.shape, bool)
    m[:, 1:] |= s[:, 1:] != s[:, :-1]
    m[:, :-1] |= s[:, :-1] != s[:, 1:]
    m[1:, :] |= s[1:, :] != s[:-1, :]
    m[:-1, :] |= s[:-1, :] != s[1:, :]
    return m


def _initial(phi, h, dtype):
    """(d, frozen): the interface cells' distances, +inf elsewhere."""
    f = dtype
    a = np.abs(np.asarray(phi, dtype=f))
    s = vapour(phi)
    H, W = a.shape
    h = f(h)
    inf = f(np.inf)

    def axis_t(lo_self, lo_other):
        """The smaller crossing distance over the two neighbours along one axis; slices select the neighbour pairs."""
        t = np.full((H, W), inf, dtype=f)
        for me, nb in ((lo_self, lo_other), (lo_other, lo_self)):
            opp = s[me] != s[nb]
            with np.errstate(divide="ignore", invalid="ignore"):
                cand = (h * a[me]) / (a[me] + a[nb])
            t[me] = np.where(opp, np.minimum(t[me], cand), t[me])
        return t

    tx = axis_t((slice(None), slice(1, None)), (slice(None), slice(None, -1)))
    ty = axis_t((slice(1, None), slice(None)), (slice(None, -1), slice(None)))
    hasx, hasy = np.isfinite(tx), np.isfinite(ty)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        both = f(1) / np.sqrt(f(1) / (tx * tx) + f(1) / (ty * ty))
    both = np.where((tx == 0) | (ty == 0), f(0), both)
    d = np.where(hasx & hasy, both, np.where(hasx, tx, np.where(hasy, ty, inf))).astype(f)
    return d, hasx | hasy


def _update(a, b, h, band, f):
    """The Godunov upwind value from the per-axis minima a, b (arrays or scalars; +inf = absent)."""
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    with np.errstate(invalid="ignore"):
        df = hi - lo
        far = ~np.isfinite(hi) | (df >= h)
        root = np.sqrt(np.maximum(f(2) * h * h - df * df, f(0)))
        u = np.where(far, lo + h, (lo + hi + root) * f(0.5))
    if band is not None:
        u = np.minimum(u, f(band))
    return u.astype(f) if isinstance(u, np.ndarray) else f(u)


def _finish(phi, d, status, H, W, h, band, f):
    if status > 0 or status == -2:
        d = np.where(np.isfinite(d), d, f(band if band is not None else (H + W) * h))
        return np.where(vapour(phi), d, -d).astype(f), status
    return np.asarray(phi, dtype=f).copy(), status


def _prepare(phi, h, dtype):
    phi = np.asarray(phi)
    assert phi.ndim == 2
    if not np.isfinite(phi).all():
        return None, None, -1
    d, frozen = _initial(phi, h, dtype)
    if not frozen.any():
        return None, None, 0
    return d, frozen, 1


def redistance_rb(phi, h, band=None, max_rounds=None, dtype=np.float64):
    """(field, rounds) by red-black passes.  rounds as bf_redistance reports it: >= 1 passes with the quiet one, 0 one sign, -1 non-finite,
    -2 max_rounds (default H + W) ran out."""
    f = dtype
    H, W = np.asarray(phi).shape
    d, frozen, status = _prepare(phi, h, f)
    if status <= 0:
        return _finish(phi, d, status, H, W, h, band, f)
    hh = f(h)
    yy, xx = np.mgrid[0:H, 0:W]
    colour = (yy + xx) & 1
    limit = H + W if max_rounds is None else int(max_rounds)
    status = -2
    for r in range(1, limit + 1):
        changed = False
        for c in (0, 1):
            p = np.pad(d, 1, constant_values=f(np.inf))
            a = np.minimum(p[1:-1, :-2], p[1:-1, 2:])
            b = np.minimum(p[:-2, 1:-1], p[2:, 1:-1])
            u = _update(a, b, hh, band, f)
            take = (colour == c) & ~frozen & (u < d)
            if take.any():
                d = np.where(take, u, d)
                changed = True
        if not changed:
            status = r
            break
    return _finish(phi, d, status, H, W, h, band, f)


def redistance_sweep(phi, h, band=None, max_rounds=None):
    """(field, rounds) by Gauss-Seidel fast sweeping, fp64: a pass is the four diagonal sweeps, cell by cell in place."""
    f = np.float64
    H, W = np.asarray(phi).shape
    d, frozen, status = _prepare(phi, h, f)
    if status <= 0:
        return _finish(phi, d, status, H, W, h, band, f)
    inf = np.inf
    limit = H + W if max_rounds is None else int(max_rounds)
    status = -2
    for r in range(1, limit + 1):
        changed = False
        for ys, xs in ((range(H), range(W)), (range(H), range(W - 1, -1, -1)), (range(H - 1, -1, -1), range(W)), (range(H - 1, -1, -1), range(W - 1, -1, -1))):
            for y in ys:
                for x in xs:
                    if frozen[y, x]:
                        continue
                    a = min(d[y, x - 1] if x > 0 else inf, d[y, x + 1] if x < W - 1 else inf)
                    b = min(d[y - 1, x] if y > 0 else inf, d[y + 1, x] if y < H - 1 else inf)
                    u = float(_update(f(a), f(b), f(h), band, f))
                    if u < d[y, x]:
                        d[y, x] = u
                        changed = True
        if not changed:
            status = r
            break
    return _finish(phi, d, status, H, W, h, band, f)


def change_rms(new, old):
    e = np.asarray(new, np.float64) - np.asarray(old, np.float64)
    return float(np.sqrt(np.mean(e * e)))


def eikonal_l1(phi, h):
    """mean | |grad phi| - 1 | with np.gradient's differences (central inside, one-sided at the border)."""
    phi = np.asarray(phi, np.float64)
    gy, gx = np.gradient(phi, h)
    return float(np.mean(np.abs(np.sqrt(gx * gx + gy * gy) - 1.0)))


def crossings(phi):
    """The linearly interpolated zero crossings: for every pair of 4-neighbours of opposite sign, |phi_a| / (|phi_a| + |phi_b|), the position
    along the edge from its left / upper cell a, in cells; horizontal pairs first, each in raster order."""
    phi = np.asarray(phi, np.float64)
    s = vapour(phi)
    out = []
    for a, b, sa, sb in ((phi[:, :-1], phi[:, 1:], s[:, :-1], s[:, 1:]), (phi[:-1, :], phi[1:, :], s[:-1, :], s[1:, :])):
        m = sa != sb
        out.append(np.abs(a[m]) / (np.abs(a[m]) + np.abs(b[m])))
    return np.concatenate(out)


# ---------------------------------------------------------------------------- the test fields (fp32, physical units)
def _centres(H, W, h):
    y, x = np.mgrid[0:H, 0:W]
    return (y + 0.5) * h, (x + 0.5) * h


def circles(H, W, h, discs):
    """The signed distance to the union of the discs (cx, cy, r) in physical units, positive inside: exact for discs that do not overlap."""
    yc, xc = _centres(H, W, h)
    best = np.full((H, W), -np.inf)
    for cx, cy, r in discs:
        best = np.maximum(best, r - np.sqrt((xc - cx) ** 2 + (yc - cy) ** 2))
    return best


def distort(true):
    """A field with the zero level set and the signs of `true` that is no signed distance: true * (1 + 0.8 sin(7 true))."""
    return true * (1.0 + 0.8 * np.sin(7.0 * true))


def single_disc(H, W, h):
    """One disc off the centre of the frame, radius 0.3 of the shorter side (at least 0.6 cell)."""
    r = max(0.3 * min(H, W) * h, 0.6 * h)
    return [(0.47 * W * h, 0.55 * H * h, r)]


def two_discs(H, W, h):
    r = max(0.17 * min(H, W) * h, 0.6 * h)
    return [(0.27 * W * h, 0.3 * H * h, r), (0.7 * W * h, 0.68 * H * h, 0.8 * r)]


def corner(H, W, h):
    """One vapour cell in the corner: the longest dependency chain a frame can have."""
    phi = np.full((H, W), -h)
    phi[0, 0] = h
    return phi


def walls(H, W, h):
    """Two vapour walls one cell thick (columns W // 3 and 2 W // 3) in liquid."""
    phi = np.full((H, W), -h)
    phi[:, W // 3] = 0.25 * h
    phi[:, (2 * W) // 3] = 0.25 * h
    return phi


def noise(H, W, h, seed=0):
    return np.random.default_rng(1000 * H + W + seed).standard_normal((H, W)) * h


def fields(H, W, h):
    """name -> fp32 field: every test field at one shape."""
    out = {"disc": distort(circles(H, W, h, single_disc(H, W, h))), "two_discs": distort(circles(H, W, h, two_discs(H, W, h))),
           "corner": corner(H, W, h), "walls": walls(H, W, h), "noise": noise(H, W, h)}
    return {k: v.astype(np.float32) for k, v in out.items()}
