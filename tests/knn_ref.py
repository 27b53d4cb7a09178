"""Brute-force k nearest neighbours, the reference of include/gs_knn.h: every pair, the squared distance
((dx*dx + dy*dy) + dz*dz) evaluated in the dtype asked for (numpy rounds every operation once and fuses nothing), the k
smallest (d2, row) pairs per row, the row itself excluded by index, rows that are masked or hold a non-finite coordinate
neither asking nor answering (+inf / -1).  float32 is the library's own arithmetic -- its output must equal this bit for
bit -- and float64 the yardstick for the mean distance.  torch_knn() is the same brute force in torch, for clouds too large
for numpy on every row.  Also the point clouds and masks the k-NN tests share."""
import numpy as np


def takes_part(xyz, invalid_mask=None):
    ok = np.isfinite(np.asarray(xyz)).all(axis=1)
    return ok if invalid_mask is None else ok & (np.asarray(invalid_mask) == 0)


def knn(xyz, k, invalid_mask=None, dtype=np.float32, chunk=512, rows=None):
    """-> d2 (R,k) dtype ascending, idx (R,k) int32 for the R query rows `rows` (default: every row, in order) against the
    whole cloud.  Per query the k smallest (d2, row) pairs in lexicographic order over the rows that take part, the query
    itself struck out by its index: a pair at +inf is a pair like any other and comes with its row, behind every finite one;
    only where fewer than k other rows take part is the tail +inf / -1.  No NaN: the difference of two finite numbers is
    finite or infinite, and so are its square and the sums."""
    x = np.asarray(xyz)
    ask = np.arange(x.shape[0]) if rows is None else np.asarray(rows, np.int64)
    d2_out = np.full((ask.size, k), np.inf, dtype)
    idx_out = np.full((ask.size, k), -1, np.int32)
    part = takes_part(x, invalid_mask)
    cols = np.flatnonzero(part)
    if cols.size == 0:
        return d2_out, idx_out
    p = x[cols].astype(dtype)
    have = min(k, cols.size - 1)
    slots = np.flatnonzero(part[ask])                        # places in the output whose row asks
    for a in range(0, slots.size, chunk):
        out = slots[a:a + chunk]
        q = x[ask[out]].astype(dtype)
        with np.errstate(over="ignore"):
            dx, dy, dz = (q[:, None, c] - p[None, :, c] for c in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == dtype
        taken = cols[None, :] == ask[out][:, None]           # the row itself: out of the running by its index
        at = np.arange(out.size)
        for j in range(have):
            least = np.where(taken, np.inf, d2).min(axis=1)
            first = np.argmax(~taken & (d2 == least[:, None]), axis=1)      # the first of equal distances: the smaller row
            d2_out[out, j] = d2[at, first]
            idx_out[out, j] = cols[first]
            taken[at, first] = True
    return d2_out, idx_out


def torch_knn(xyz, k, invalid_mask=None, chunk=2048):
    """The same brute force in torch, on the device of `xyz` ((N,3) f32 tensor; invalid_mask (N,) tensor or None)
    -> d2 (N,k) f32, idx (N,k) int32 tensors there.  Three eager subtractions, three eager products, two eager sums: each an
    elementwise kernel of its own, so each rounded once and nothing fused.  Selection is topk over the int64 keys
    (bits of d2 << 32) | row: d2 is never negative, so its bits order like its value and a pair at +inf keeps its row; the
    query's own column holds the largest int64.  Peak memory: about 30 bytes per (query, row) pair of a chunk."""
    import torch
    n = xyz.shape[0]
    d2_out = torch.full((n, k), float("inf"), dtype=torch.float32, device=xyz.device)
    idx_out = torch.full((n, k), -1, dtype=torch.int32, device=xyz.device)
    part = torch.isfinite(xyz).all(dim=1)
    if invalid_mask is not None:
        part &= invalid_mask == 0
    cols = torch.nonzero(part)[:, 0]
    have = min(k, cols.numel() - 1)
    if have <= 0:
        return d2_out, idx_out
    p = xyz[cols].to(torch.float32)
    for a in range(0, cols.numel(), chunk):
        q = p[a:a + chunk]
        sq = []
        for c in range(3):
            d = q[:, None, c] - p[None, :, c]
            sq.append(d * d)
            del d
        d2 = sq[0] + sq[1]
        d2 = d2 + sq[2]
        del sq
        assert d2.dtype == torch.float32
        key = (d2.view(torch.int32).to(torch.int64) << 32) | cols[None, :]
        at = torch.arange(q.shape[0], device=xyz.device)
        key[at, a + at] = torch.iinfo(torch.int64).max
        best = torch.topk(key, have, dim=1, largest=False, sorted=True).values
        d2_out[cols[a:a + chunk], :have] = (best >> 32).to(torch.int32).view(torch.float32)
        idx_out[cols[a:a + chunk], :have] = (best & 0xffffffff).to(torch.int32)
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


def lattice():
    g = np.arange(16, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def copies():
    x = np.tile(np.array([[0.3, -1.7, 2.9]], np.float32), (302, 1))
    x[100] = (0.3, -1.7, 3.0)
    x[301] = (5.0, 5.0, 5.0)
    return x


def overflow():
    """300 rows: every seventh scaled by 3e38 (its squared distance to anything overflows to +inf) and the rows behind them by
    2e19 (squared distances around 1e38, finite, +inf among themselves only where they add up past the largest f32)"""
    x = uniform(300)
    x[::7] *= np.float32(3e38)
    x[1::7] *= np.float32(2e19)
    return x


def subnormal():
    """4097 rows in units of 3e-21: no coordinate is subnormal, every squared distance to a near neighbour is"""
    return (uniform(4097).astype(np.float64) * 3e-21).astype(np.float32)


def identical():
    """5000 copies of one point: every distance 0, every sort key the same"""
    return np.tile(np.array([[0.3, -1.7, 2.9]], np.float32), (5000, 1))


def big_clusters():
    """65 537 rows (1025 leaves of 64): the three clusters of clouds() at 21 840 rows each and one more, and 16 outliers at
    1e4 times their extent, shuffled so that masks by stride meet all of them"""
    rng = np.random.default_rng(0)
    sizes = (21840, 21840, 21841)
    x = np.concatenate([c + rng.normal(0.0, s, (m, 3)) for m, (c, s) in
                        zip(sizes, (((0.0, 0.0, 0.0), 1e-3), ((3.0, 1.0, -2.0), 1e-1), ((-20.0, 5.0, 9.0), 2.0)))])
    extent = float((x.max(axis=0) - x.min(axis=0)).max())
    d = rng.normal(0.0, 1.0, (16, 3))
    far = x.mean(axis=0) + d / np.linalg.norm(d, axis=1, keepdims=True) * extent * 1e4
    x = np.concatenate([x, far]).astype(np.float32)
    return x[rng.permutation(len(x))]


EXTRA = {"lattice": lattice, "copies": copies, "overflow": overflow, "subnormal": subnormal, "identical": identical,
         "big_clusters": big_clusters}


def masked(x, mask_name):
    """-> a copy of x and its int8 mask (None for mask_name None), by the names the k-NN tests use"""
    x = x.copy()
    if mask_name is None:
        return x, None
    mask = np.zeros(len(x), np.int8)
    if mask_name == "third":
        mask[::3] = 1
    elif mask_name == "fifth":
        mask[::5] = 1
    elif mask_name == "all":
        mask[:] = 1
    elif mask_name == "garbage":                 # invalid rows hold NaN and 1e30: they must not move anything
        mask[::3] = 1
        x[::6] = np.nan
        x[3::6] = 1e30
    elif mask_name == "half_garbage":            # ... and half of the invalid rows hold clean coordinates
        mask[::3] = 1
        x[::12] = np.nan
        x[3::12] = 1e30
    elif mask_name == "nan_row":                 # a VALID row with one NaN coordinate (and one with an infinite one)
        x[17, 1] = np.nan
        x[40, 2] = np.inf
    else:
        raise KeyError(mask_name)
    return x, mask


def logit_bar(c, logit, c0=0.28209479177387814):
    """Per-element bar for logit(c) / c0 evaluated in f32 against float64, c in [0, 0.99], u = 2^-24: c carries a relative u
    (the division by 255, or 0.99 itself as f32), which 1 - c sees as u c / (1 - c); the quotient c / (1 - c) and its two
    roundings make (c / (1 - c) + 3) u relative, which is the absolute error of the log; the log's own rounding and the division
    by c0 add 2 u of the result.  At c = 0.99 that is 102 u / c0 + 2 u 16.3 = 2.4e-5; at c = 0.5, 1.4e-6."""
    u = 2.0 ** -24
    with np.errstate(divide="ignore", invalid="ignore"):
        return (c / (1.0 - c) + 3.0) * u / c0 + 2.0 * u * np.abs(logit)
