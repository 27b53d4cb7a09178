"""Brute-force k nearest neighbours, the reference of include/gs_knn.h: every pair, the squared distance
((dx*dx + dy*dy) + dz*dz) evaluated in the dtype asked for (numpy rounds every operation once and fuses nothing), the k
smallest (d2, row) pairs per row, the row itself excluded by index, rows that are masked or hold a non-finite coordinate
neither asking nor answering (+inf / -1).  float32 is the library's own arithmetic -- its output must equal this bit for
bit -- and float64 the yardstick for the mean distance.  Also the five point clouds the k-NN tests share."""
import numpy as np


def takes_part(xyz, invalid_mask=None):
    ok = np.isfinite(np.asarray(xyz)).all(axis=1)
    return ok if invalid_mask is None else ok & (np.asarray(invalid_mask) == 0)


def knn(xyz, k, invalid_mask=None, dtype=np.float32, chunk=512):
    """-> d2 (N,k) dtype ascending, idx (N,k) int32"""
    x = np.asarray(xyz)
    n = x.shape[0]
    d2_out = np.full((n, k), np.inf, dtype)
    idx_out = np.full((n, k), -1, np.int32)
    cols = np.flatnonzero(takes_part(x, invalid_mask))
    if cols.size == 0:
        return d2_out, idx_out
    p = x[cols].astype(dtype)
    have = min(k, cols.size - 1)
    for a in range(0, cols.size, chunk):
        q = p[a:a + chunk]
        dx, dy, dz = (q[:, None, c] - p[None, :, c] for c in range(3))
        with np.errstate(over="ignore"):
            d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == dtype
        rows = np.arange(q.shape[0])
        d2[rows, a + rows] = np.nan                          # the row itself: out of the running, unlike a pair at +inf
        for j in range(have):
            first = np.nanargmin(d2, axis=1)                 # the first of equal distances: the smaller row
            d2_out[cols[a:a + chunk], j] = d2[rows, first]
            idx_out[cols[a:a + chunk], j] = cols[first]
            d2[rows, first] = np.nan
    return d2_out, idx_out


def mean_distance(xyz, k=3, invalid_mask=None, dtype=np.float64):
    d2, _ = knn(xyz, k, invalid_mask, dtype)
    return np.sqrt(d2).mean(axis=1)


def uniform(n, seed=0):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)


def clouds():
    """name -> (N,3) f32, each from seed 0"""
    out = {"uniform": uniform(4096)}
    rng = np.random.default_rng(0)
    far = rng.normal(0.0, 1.0, (8, 3)) * np.array([1e4, 1e5, 1e6])
    out["outliers"] = np.concatenate([rng.normal(0.0, 0.05, (4000, 3)), far]).astype(np.float32)
    out["duplicates"] = (1000.0 + 1e-3 * np.random.default_rng(0).uniform(0.0, 1.0, (3000, 3))).astype(np.float32)
    flat = np.random.default_rng(0).uniform(-1.0, 1.0, (2000, 3))
    flat[:, 2] = 0.25
    out["coplanar"] = flat.astype(np.float32)
    rng = np.random.default_rng(0)
    out["clusters"] = np.concatenate([c + rng.normal(0.0, s, (700, 3)) for c, s in
                                      (((0.0, 0.0, 0.0), 1e-3), ((3.0, 1.0, -2.0), 1e-1), ((-20.0, 5.0, 9.0), 2.0))]).astype(np.float32)
    return out


def logit_bar(c, logit, c0=0.28209479177387814):
    """Per-element bar for logit(c) / c0 evaluated in f32 against float64, c in [0, 0.99], u = 2^-24: c carries a relative u
    (the division by 255, or 0.99 itself as f32), which 1 - c sees as u c / (1 - c); the quotient c / (1 - c) and its two
    roundings make (c / (1 - c) + 3) u relative, which is the absolute error of the log; the log's own rounding and the division
    by c0 add 2 u of the result.  At c = 0.99 that is 102 u / c0 + 2 u 16.3 = 2.4e-5; at c = 0.5, 1.4e-6."""
    u = 2.0 ** -24
    with np.errstate(divide="ignore", invalid="ignore"):
        return (c / (1.0 - c) + 3.0) * u / c0 + 2.0 * u * np.abs(logit)
