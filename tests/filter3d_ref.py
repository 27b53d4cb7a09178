"""include/gs_filter3d.h restated in numpy: the sampling rate in float32, operation for operation; the transform of a row and
its gradient in float64, rounded once.  What the GPU tests compare the kernels against, and what test_filter3d_ref_host.py
checks against closed forms."""
import numpy as np

VIEW_FLOATS = 16
FEATURES = 56
ROWS_PER_BLOCK = 256
MAX_POINTS = 2 ** 30
MAX_VIEWS = 2 ** 20
F = np.float32


def filter_k(variance, factor):
    """sqrtf(variance) * factor in float32"""
    return float(np.sqrt(F(variance)) * F(factor))


def window(W, H, margin):
    margin = F(margin)
    return (-margin) * F(W), (F(1.0) + margin) * F(W), (-margin) * F(H), (F(1.0) + margin) * F(H)


def rate(point_cloud, point_invalid_mask, views, W, H, near, margin):
    """-> (N,) float32: gs_filter3d_rate"""
    pc = np.asarray(point_cloud, dtype=F).reshape(-1, 3)
    valid = np.asarray(point_invalid_mask).reshape(-1) == 0
    views = np.asarray(views, dtype=F).reshape(-1, VIEW_FLOATS)
    lo_x, hi_x, lo_y, hi_y = window(W, H, margin)
    near = F(near)
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    best = np.zeros(pc.shape[0], dtype=F)
    with np.errstate(all="ignore"):
        for w in views:
            p0 = ((w[0] * x + w[1] * y) + w[2] * z) + w[9]
            p1 = ((w[3] * x + w[4] * y) + w[5] * z) + w[10]
            p2 = ((w[6] * x + w[7] * y) + w[8] * z) + w[11]
            fx, fy, cx, cy = w[12], w[13], w[14], w[15]
            u = (fx * p0) / p2 + cx
            v = (fy * p1) / p2 + cy
            fm = fx if fx > fy else fy
            c = fm / p2
            assert p0.dtype == u.dtype == c.dtype == F
            sees = (p2 > near) & (lo_x <= u) & (u <= hi_x) & (lo_y <= v) & (v <= hi_y) & (c > F(0.0))
            best = np.where(sees & (c > best), c, best)
    seen = valid & (best > 0)
    smallest = best[seen].min() if seen.any() else F(np.inf)
    return np.where(valid, np.where(seen, best, smallest), F(np.inf)).astype(F)


def normalised_quaternions(q):
    """k_project's normalisation of (N,4) float32 rows, in float32"""
    q = np.asarray(q, dtype=F)
    with np.errstate(all="ignore"):
        n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        return (q / n[:, None]).astype(F)


def _row_terms(ls, f):
    """t (N,3), r (N,3), c (N,) in float64"""
    v = f.astype(np.float64) * f.astype(np.float64)
    e = np.exp(ls.astype(np.float64))
    s = e * e
    t = s + v[:, None]
    r = s / t
    c = np.sqrt((r[:, 0] * r[:, 1]) * r[:, 2])
    return t, r, c


def filter_width(rate_, k):
    with np.errstate(all="ignore"):
        return (F(k) / np.asarray(rate_, dtype=F)).astype(F)


def apply(features, rate_, k):
    """-> (features_out, features after the call): gs_filter3d_apply"""
    feat = np.array(features, dtype=F).reshape(-1, FEATURES)
    out = feat.copy()
    f = filter_width(rate_, k)
    on = f > 0
    if on.any():
        with np.errstate(all="ignore"):
            q = normalised_quaternions(feat[on, 0:4])
            t, r, c = _row_terms(feat[on, 4:7], f[on])
            a = feat[on, 7].astype(np.float64)
            ls = (0.5 * np.log(t)).astype(F)
            logit = (np.log(c) - np.log((1.0 - c) + np.exp(-a))).astype(F)
        feat[on, 0:4] = q
        out[on, 0:4] = q
        out[on, 4:7] = ls
        out[on, 7] = logit
    return out, feat


def apply_backward_f64(grad_out, features, rate_, k):
    """-> (grad_in in float64 before its one rounding, the summed magnitude of the terms of every element)"""
    g = np.asarray(grad_out, dtype=F).reshape(-1, FEATURES)
    feat = np.asarray(features, dtype=F).reshape(-1, FEATURES)
    out = g.astype(np.float64)
    mag = np.abs(out)
    f = filter_width(rate_, k)
    on = f > 0
    if on.any():
        with np.errstate(all="ignore"):
            _, r, c = _row_terms(feat[on, 4:7], f[on])
            E = np.exp(-feat[on, 7].astype(np.float64))
            D = (1.0 - c) + E
            ga = g[on, 7].astype(np.float64)
            gls = g[on, 4:7].astype(np.float64)
            through = ga * (1.0 + c / D)
            A = np.where(gls == 0, 0.0, gls * r)
            B = np.where(ga[:, None] == 0, 0.0, through[:, None] * (1.0 - r))
            out_a = np.where(ga == 0, 0.0, (ga * E) / D)
        out[on, 4:7] = A + B
        mag[on, 4:7] = np.abs(A) + np.abs(B)
        out[on, 7] = out_a
        mag[on, 7] = np.abs(out_a)
    return out, mag


def apply_backward(grad_out, features, rate_, k):
    """-> grad_in (N,56) float32: gs_filter3d_apply_backward"""
    with np.errstate(all="ignore"):
        return apply_backward_f64(grad_out, features, rate_, k)[0].astype(F)


def ulp_distance(a, b):
    """elementwise distance of two float32 arrays in units in the last place (equal bits or both NaN: 0)"""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)

    def ordered(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    d = np.abs(ordered(a) - ordered(b))
    return np.where(np.isnan(a) & np.isnan(b), 0, d)


def ulp_of(x):
    """the spacing of float32 at |x| (float64 in, float64 out)"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    return np.spacing(np.maximum(x, np.finfo(F).tiny).astype(F)).astype(np.float64)
