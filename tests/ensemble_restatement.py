"""numpy fp64 restatement of the ensemble rows of DESIGN.md section 23 (csrc/ensemble.hip), straight from their definitions, and a bound per row
on what a correct kernel may differ by: the oracle of tests/test_ensemble.py and tests/test_gpu_ensemble.py.

For M members x_m and the truth y at the n pixels p of a frame:
  mean_rmse = sqrt(1/n sum_p (xbar_p - y_p)^2)                      xbar_p = 1/M sum_m x_m
  spread    = sqrt(1/n sum_p 1/(M-1) sum_m (x_m - xbar_p)^2)
  crps      = 1/n sum_p [1/M sum_m |x_m - y| - w sum_m sum_n |x_m - x_n|],  w = 1/(2 M^2), fair: 1/(2 M (M-1))
  rank_hist[r] = #{p : exactly r members are strictly below y_p}
  mean      = xbar_p

The bounds.  u = 2^-53 is the unit roundoff of the fp64 arithmetic both sides use, U32 = 2^-24 that of the one fp32 rounding at the store, and
gamma(k) = k u / (1 - k u) bounds a sum of k terms added in ANY order (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1 / section 4.2).
The fp32 inputs are exact in fp64, and an fp64 difference of two fp64 numbers is rounded once, RELATIVE TO THE DIFFERENCE: so |x_m - y| and |x_m - x_n|
carry u of themselves, however large the offset the two share.  Only the member mean feels the offset: a sum of M terms and a quotient,
|d xbar_p| <= gamma(M + 1) a_p with a_p = 1/M sum_m |x_m|.
  e_p = xbar_p - y_p:        |d e_p| <= D_p = gamma(M + 1) a_p + u |e_p|
  S = sum_p e_p^2:           |dS| <= sum_p (2 |e_p| D_p + D_p^2) + gamma(n + 1) sum_p e_p^2          (squares rounded once, n terms in any order)
  c_m = x_m - xbar_p:        |d c_m| <= D_pm = gamma(M + 1) a_p + u |c_m|
  V = sum_p sum_m c_m^2:     |dV| <= sum (2 |c_m| D_pm + D_pm^2) + gamma(n M + 1) V
  r = sqrt(S / n), sqrt(V / (M - 1) / n):   |sqrt(a) - sqrt(b)| <= min(|a - b| / sqrt(b), sqrt|a - b|), plus 4 u r for the quotients and the root
  crps:                      both sums are of non-negative terms, P = 1/M sum sum |x_m - y| and Q = w sum sum sum |x_m - x_n|: each is within
                             gamma(n M^2 + 4) of ITSELF, and their difference cancels, so |d crps| <= gamma(n M^2 + 8) (P + Q) / n
  mean:                      |d xbar_p| as above.
The restatement is computed in the same arithmetic, so every term above is taken twice; then the store: |fl32(v') - v| <= |v' - v| + U32 |v'|.
No constant is fitted to what the GPU gives."""
import numpy as np

U64, U32 = 2.0 ** -53, 2.0 ** -24


def gamma(k):
    return k * U64 / (1.0 - k * U64)


def pair_weight(M, fair):
    return 1.0 / (2.0 * M * (M - 1)) if fair else 1.0 / (2.0 * M * M)


def _stored(ref, err):
    """The bound on an fp32 value stored from a computation within err of ref (the restatement's own error included in err)."""
    return err + U32 * (np.abs(ref) + err)


def _root(b, db, scale):
    """sqrt(b * scale) for b within db of the exact sum: (value, bound on the root's error)."""
    r = np.sqrt(b * scale)
    with np.errstate(divide="ignore", invalid="ignore"):
        lin = np.where(b > 0, db * scale / r, np.inf)
    return r, np.minimum(lin, np.sqrt(db * scale)) + 4 * U64 * r


def frame_rows(x, y, fair=False):
    """x (M, H, W), y (H, W) fp32 -> (rows, bounds): dicts of the five outputs in fp64 (rank_hist int64, its bound 0) and of their bounds; rows also
    holds "pair", the CRPS' pair term w sum_m sum_n |x_m - x_n| averaged over the pixels."""
    assert x.dtype == np.float32 and y.dtype == np.float32
    M, n = x.shape[0], y.size
    xd, yd = x.reshape(M, n).astype(np.float64), y.reshape(n).astype(np.float64)
    mean = xd.sum(0) / M
    a = np.abs(xd).sum(0) / M
    dmean = gamma(M + 1) * a
    e = mean - yd
    D = dmean + U64 * np.abs(e)
    S = (e * e).sum()
    dS = 2 * ((2 * np.abs(e) * D + D * D).sum() + gamma(n + 1) * S)
    c = xd - mean
    Dm = dmean + U64 * np.abs(c)
    V = (c * c).sum()
    dV = 2 * ((2 * np.abs(c) * Dm + Dm * Dm).sum() + gamma(n * M + 1) * V)
    w = pair_weight(M, fair)
    P = np.abs(xd - yd).sum() / M
    pairs = 0.0
    for m in range(M):                                  # sum_m sum_n |x_m - x_n| = 2 sum_{m < n}: the matrix is symmetric with a zero diagonal
        pairs += 2.0 * np.abs(xd[m + 1:] - xd[m]).sum()
    Q = w * pairs
    rows, bounds = {}, {}
    r, dr = _root(S, dS, 1.0 / n)
    rows["mean_rmse"], bounds["mean_rmse"] = r, _stored(r, dr)
    r, dr = _root(V, dV, 1.0 / (M - 1) / n)
    rows["spread"], bounds["spread"] = r, _stored(r, dr)
    rows["crps"] = (P - Q) / n
    bounds["crps"] = _stored(rows["crps"], 2 * gamma(n * M * M + 8) * (P + Q) / n)
    rows["pair"] = Q / n
    below = (xd < yd).sum(0)
    rows["rank_hist"], bounds["rank_hist"] = np.bincount(below, minlength=M + 1).astype(np.int64), 0
    rows["mean"], bounds["mean"] = mean.reshape(y.shape), _stored(mean, 2 * dmean).reshape(y.shape)
    return rows, bounds


def ensemble_rows(members, target, fair=False):
    """members (M, F, H, W), target (F, H, W) fp32 -> (rows, bounds) with the frames stacked along axis 0."""
    per = [frame_rows(members[:, f], target[f], fair) for f in range(target.shape[0])]
    return ({k: np.stack([np.asarray(r[k]) for r, _ in per]) for k in per[0][0]},
            {k: np.stack([np.asarray(b[k], dtype=np.float64) for _, b in per]) for k in per[0][1]})


def crps_sorted(x, y, fair=False):
    """The CRPS of one frame in the sorted weighted-sum form, in fp64: 1/n sum_p [1/M sum_m |x_m - y| - 2 w sum_i (2 i - M + 1) x_(i)].  Equal to the
    pairwise form in exact arithmetic; in fp32 it cancels when the members share a large offset, which is why the kernel does not use it."""
    M, n = x.shape[0], y.size
    xs = np.sort(x.reshape(M, n).astype(np.float64), axis=0)
    weights = (2.0 * np.arange(M) - M + 1)[:, None]
    pair = 2.0 * pair_weight(M, fair) * (weights * xs).sum(0)
    return float((np.abs(xs - y.reshape(n).astype(np.float64)).sum(0) / M - pair).sum() / n)


KINDS = ("normal", "offset", "equal", "ties")


def case(kind, M, F, H, W, seed):
    """The inputs of one test case, fp32: members (M, F, H, W), target (F, H, W).  normal: standard normal; offset: members and truth 1e4 + 1e-2 z, the
    cancellation case (a sorted fp32 form loses every digit of the pair term there); equal: every member the same field; ties: the truth equals
    one member bit for bit on half the pixels (a member equal to the truth is not below it)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, F, H, W))
    y = rng.standard_normal((F, H, W))
    if kind == "offset":
        x, y = 1e4 + 1e-2 * x, 1e4 + 1e-2 * y
    elif kind == "equal":
        x = np.broadcast_to(x[:1], x.shape)
    x, y = np.ascontiguousarray(x, dtype=np.float32), y.astype(np.float32)
    if kind == "ties":
        which = rng.integers(0, M, size=(F, H, W))
        tied = np.take_along_axis(x, which[None], axis=0)[0]
        y = np.where(rng.random((F, H, W)) < 0.5, tied, y).astype(np.float32)
    return x, y
