"""include/gs_mcmc.h restated in numpy and Python integers: the checker of tests/test_gpu_mcmc.py and of the host tests.

Philox is tests/density_ref.py's, the library's f32 exp is oracle.expf (bit for bit), integers are Python ints, and everything the
header computes in float64 is computed here in Python floats in the header's order.  Where the header works in f32 the
restatement is float64 from the same inputs, except for the values that decide something or feed a cancellation: gs_sigmoid
and the angle two_pi * U of the Box-Muller step are restated in f32, operation for operation."""
import bisect
import math

import numpy as np

from density_ref import philox4x32_10_numpy, seed_key

BLOCK = 256
N_MAX = 51
WEIGHT_ONE = 2 ** 24
STREAM_NOISE, STREAM_RELOCATE = 2, 3
P_MIN, P_MAX = 0.005, 1.0 - 2.0 ** -24
TWO_PI_F32 = np.float32(2.0 * 3.141592653589)
COUNTS = ("valid_before", "dead", "alive", "free", "new", "destinations", "sources", "valid_after")


def _expf(x):
    from oracle import oracle
    return oracle.expf(np.asarray(x, np.float32))


def sigmoid_f32(x):
    """gs_sigmoid: 1.0f / (1.0f + gs_expf(-x)), every operation in f32"""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        return (np.float32(1.0) / (np.float32(1.0) + _expf(-x))).astype(np.float32)


def min_opacity_logit(min_opacity=0.005):
    return np.float32(math.log(min_opacity / (1.0 - min_opacity)))


def _draws(rows, second, stream, seed):
    rows = np.asarray(rows, np.uint64)
    ctr = np.stack([rows, np.full_like(rows, second), np.full_like(rows, stream), np.zeros_like(rows)], -1)
    return philox4x32_10_numpy(ctr, seed_key(seed)).astype(np.uint64)


def rotation(q):
    x, y, z, w = (q[..., i] for i in range(4))
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


# ---- gs_mcmc_noise -----------------------------------------------------------------------------------------------------
def noise(features, mask, noise_scale, seed, step_index, gate_k=100.0, gate_x0=0.995, with_smallest_term=False):
    """-> (delta (N,3) float64, magnitude (N,3) float64 = sum_j |Sigma_ij v_j|, moves (N) bool: valid with a finite delta).
    delta and magnitude are 0 where the row does not move.  with_smallest_term: and the smallest non-zero |Sigma_ij v_j| of each row."""
    ft = np.asarray(features, np.float32)
    n = ft.shape[0]
    valid = np.asarray(mask) == 0
    o = sigmoid_f32(ft[:, 7]).astype(np.float64)
    k, x0, scale = float(np.float32(gate_k)), float(np.float32(gate_x0)), float(np.float32(noise_scale))
    with np.errstate(all="ignore"):
        g = 1.0 / (1.0 + np.exp(np.clip(-(k * ((1.0 - o) - x0)), -86.0, 88.0)))
        s = g * scale
        u = _draws(np.arange(n), step_index, STREAM_NOISE, seed)
        U = (((u >> np.uint64(8)) + np.uint64(1)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
        a1 = (TWO_PI_F32 * U[:, 1]).astype(np.float32).astype(np.float64)          # one f32 multiply, as on the device
        a3 = (TWO_PI_F32 * U[:, 3]).astype(np.float32).astype(np.float64)
        r1, r3 = np.sqrt(-2.0 * np.log(U[:, 0].astype(np.float64))), np.sqrt(-2.0 * np.log(U[:, 2].astype(np.float64)))
        z = np.stack([r1 * np.cos(a1), r1 * np.sin(a1), r3 * np.cos(a3)], -1)
        R = rotation(ft[:, 0:4].astype(np.float64))
        e = _expf(ft[:, 4:7]).astype(np.float64)
        RS = R * e[:, None, :]
        Sigma = (RS * e[:, None, :]) @ np.swapaxes(R, -1, -2)
        v = z * s[:, None]
        terms = Sigma * v[:, None, :]
        delta, magnitude = terms.sum(-1), np.abs(terms).sum(-1)
    moves = valid & np.isfinite(delta).all(-1)
    delta[~moves] = 0.0
    magnitude[~moves] = 0.0
    if with_smallest_term:
        size = np.where(terms == 0.0, np.inf, np.abs(terms))         # (a product that is exactly zero has no rounding)
        return delta, magnitude, moves, np.where(moves, size.min((-1, -2)), 0.0)
    return delta, magnitude, moves


# ---- gs_mcmc_regulariser -----------------------------------------------------------------------------------------------
def regulariser(features, mask, lambda_opacity, lambda_scale, upstream=1.0):
    """-> (value_and_count (3,) float64, added (N,56) float64: the term the call adds to the gradient)"""
    ft = np.asarray(features, np.float32)
    valid = np.asarray(mask) == 0
    V = int(valid.sum())
    added = np.zeros(ft.shape, np.float64)
    if V == 0:
        return np.zeros(3), added
    lo, ls, up = float(np.float32(lambda_opacity)), float(np.float32(lambda_scale)), float(np.float32(upstream))
    o = sigmoid_f32(ft[:, 7]).astype(np.float64)
    e = _expf(ft[:, 4:7]).astype(np.float64)
    value = np.array([lo * o[valid].sum() / V, ls * e[valid].sum() / (3 * V), V], np.float64)
    added[valid, 7] = ((up * lo) / V) * (o[valid] * (1.0 - o[valid]))
    added[valid, 4:7] = ((up * ls) / (3.0 * V)) * e[valid]
    return value, added


# ---- gs_mcmc_relocate --------------------------------------------------------------------------------------------------
def weights(features, mask, min_logit):
    """-> (cls (N) of 'a' alive / 'd' dead / 'f' free / 'o' other, w: list of Python ints)"""
    ft = np.asarray(features, np.float32)
    mask = np.asarray(mask)
    logit = ft[:, 7]
    with np.errstate(invalid="ignore"):
        above = logit > np.float32(min_logit)
    o = sigmoid_f32(logit)
    scaled = np.floor(o * np.float32(WEIGHT_ONE))                   # exact: a power of two
    cls, w = [], []
    for n in range(ft.shape[0]):
        if mask[n] == 1:
            cls.append("f"); w.append(0)
        elif mask[n] != 0:
            cls.append("o"); w.append(0)
        elif above[n]:
            cls.append("a"); w.append(min(max(int(scaled[n]), 1), WEIGHT_ONE - 1))
        else:
            cls.append("d"); w.append(0)
    return cls, w


def budget(valid, dead, alive, free, grow_permille, cap_max):
    """-> (n_new, D), Python ints"""
    target = min(cap_max, valid + valid * grow_permille // 1000)
    n_new = min(free, max(0, target - valid))
    if alive == 0:
        return 0, 0
    return n_new, dead + n_new


def draw_sources(w, D, seed, call_index):
    """-> (source_of: list of D rows, t: the D integers drawn, W)"""
    incl, run = [], 0
    for x in w:
        run += x
        incl.append(run)
    W = run
    if D == 0:
        return [], [], W
    u = _draws(np.arange(D), call_index, STREAM_RELOCATE, seed)
    ts = [((int(u[j, 0]) + (int(u[j, 1]) << 32)) * W) >> 64 for j in range(D)]
    return [bisect.bisect_right(incl, t) for t in ts], ts, W


def clamp_p(p):
    return P_MIN if p < P_MIN else (P_MAX if p > P_MAX else p)


def double_sum(p, M):
    """d of step 5, in Python floats in the header's order"""
    d = 0.0
    for i in range(1, M + 1):
        c, pk = 1.0, p
        for k in range(i):
            term = (c * pk) / math.sqrt(float(k + 1))
            d = d - term if k & 1 else d + term
            c = (c * float(i - 1 - k)) / float(k + 1)
            pk = pk * p
    return d


def relocated(logit, log_scales, m, n_max):
    """-> (new logit, new log-scales (3,)) as float64 values BEFORE the rounding to f32, and (o, p, d)"""
    M = min(m + 1, n_max)
    o = float(sigmoid_f32(np.float32(logit)))
    p = clamp_p(1.0 - math.pow(1.0 - o, 1.0 / M))
    d = double_sum(p, M)
    shift = math.log(o / d)
    return math.log(p / (1.0 - p)), np.asarray(log_scales, np.float64) + shift, (o, p, d)


def relocate(point_cloud, features, mask, object_id, seed, call_index, min_logit=None, n_max=N_MAX, grow_permille=50, cap_max=None):
    """The whole call on copies.  -> dict: counts (8 ints), dest_row, source_of (D), multiplicity (N, or None when D = 0),
    point_cloud / features64 (float64: the new logit and log-scales unrounded) / mask / object_id after the call, touched (N)
    bool: the rows whose moments are zeroed."""
    pc, ft = np.array(point_cloud, np.float32), np.array(features, np.float32)
    mask, obj = np.array(mask, np.int8), np.array(object_id, np.int32)
    n = ft.shape[0]
    min_logit = min_opacity_logit() if min_logit is None else min_logit
    cap_max = n if cap_max is None else cap_max
    cls, w = weights(ft, mask, min_logit)
    dead_rows = [i for i in range(n) if cls[i] == "d"]
    free_rows = [i for i in range(n) if cls[i] == "f"]
    alive = cls.count("a")
    valid = alive + len(dead_rows)
    n_new, D = budget(valid, len(dead_rows), alive, len(free_rows), grow_permille, cap_max)
    dest = (dead_rows + free_rows[:n_new]) if D else []
    source_of, _, W = draw_sources(w, D, seed, call_index)
    ft64 = ft.astype(np.float64)
    touched = np.zeros(n, bool)
    multiplicity = None
    if D:
        multiplicity = np.zeros(n, np.int64)
        for s in source_of:
            multiplicity[s] += 1
        for s in np.nonzero(multiplicity)[0]:
            logit, ls, _ = relocated(ft[s, 7], ft[s, 4:7], int(multiplicity[s]), n_max)
            group = [s] + [dest[j] for j in range(D) if source_of[j] == s]
            for r in group:
                pc[r], obj[r], mask[r] = pc[s], obj[s], 0
                ft64[r] = ft[s].astype(np.float64)
                ft64[r, 7], ft64[r, 4:7] = logit, ls
                touched[r] = True
    sources = 0 if multiplicity is None else int((multiplicity > 0).sum())
    counts = [valid, len(dead_rows), alive, len(free_rows), n_new, D, sources, valid + n_new]
    return dict(counts=counts, dest_row=dest, source_of=source_of, multiplicity=multiplicity, point_cloud=pc, features64=ft64, mask=mask,
                object_id=obj, touched=touched, W=W, weights=w)


def ulp_distance_f32(got, want64):
    """|got - want| in units of the f32 ulp at want, for f32 `got` against the unrounded float64 `want64`"""
    want64 = np.asarray(want64, np.float64)
    ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - want64) / ulp
