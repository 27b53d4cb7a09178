"""A numpy float64 restatement of include/gs_pose_table.h: compose, its backward, the series threshold and the selection rule,
operation by operation in the header's order.  float32 inputs are widened exactly, every result is rounded to float32 once."""
import numpy as np

# the per-element bar of a gradient: |got - want| <= BAR_ABS + BAR_REL * magnitude, magnitude = the sum of the absolute values of
# the terms (the bar of tests/test_gpu_appearance.py's backward test)
from appearance_ref import BAR_ABS, BAR_REL, within_bar          # noqa: F401

DELTA_FLOATS = 6
THREADS = 256
SERIES_S = 1e-8
MAX_VIEWS = 2 ** 24
MAX_OBJECTS = 64


def coefficients(s, series=None):
    """-> (A, C, B) of s = |w|^2: sin(th/2)/th, cos(th/2), (C/2 - A)/s; series: force a branch (None: the header's threshold)"""
    s = float(s)
    if series is None:
        series = s < SERIES_S
    if not series:
        th = np.sqrt(s)
        A = np.sin(th / 2.0) / th
        C = np.cos(th / 2.0)
        return A, C, (C / 2.0 - A) / s
    return 1.0 / 2.0 + s * (-1.0 / 48.0 + s / 3840.0), 1.0 + s * (-1.0 / 8.0 + s / 384.0), -1.0 / 24.0 + s / 960.0


def rotation(q):
    x, y, z, w = (float(v) for v in q)
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    return np.array([[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
                     [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
                     [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]], dtype=np.float64)


def compose64(delta, q_base, t_base):
    """-> (q', t') in float64, not rounded, without selection: the formulas alone.  delta (V,6), q_base (V,K,4), t_base (V,K,3)"""
    delta, q_base, t_base = (np.asarray(a, dtype=np.float64) for a in (delta, q_base, t_base))
    V, K = q_base.shape[:2]
    q_out, t_out = np.empty((V, K, 4)), np.empty((V, K, 3))
    with np.errstate(all="ignore"):
        for v in range(V):
            w0, w1, w2, u0, u1, u2 = delta[v]
            s = (w0 * w0 + w1 * w1) + w2 * w2
            A, C, _ = coefficients(s)
            x1, y1, z1, ww1 = A * w0, A * w1, A * w2, C
            for k in range(K):
                x, y, z, w = q_base[v, k]
                R = rotation(q_base[v, k])
                q_out[v, k] = [((w * x1 + x * ww1) + y * z1) - z * y1, ((w * y1 - x * z1) + y * ww1) + z * x1,
                               ((w * z1 + x * y1) - y * x1) + z * ww1, ((w * ww1 - x * x1) - y * y1) - z * z1]
                t_out[v, k] = [t_base[v, k, i] + ((R[i, 0] * u0 + R[i, 1] * u1) + R[i, 2] * u2) for i in range(3)]
    return q_out, t_out


def compose(delta, q_base, t_base):
    """gs_pose_compose: -> (q', t') float32.  A view of six exact zeros gets its base rows bit for bit; a view with a
    non-finite float gets NaN."""
    delta, q_base, t_base = (np.asarray(a, dtype=np.float32) for a in (delta, q_base, t_base))
    q64, t64 = compose64(delta, q_base, t_base)
    with np.errstate(all="ignore"):
        q_out, t_out = q64.astype(np.float32), t64.astype(np.float32)
    for v in range(delta.shape[0]):
        if np.all(delta[v] == 0.0):
            q_out[v], t_out[v] = q_base[v], t_base[v]
        elif not np.all(np.isfinite(delta[v])):
            q_out[v], t_out[v] = np.nan, np.nan
    return q_out, t_out


def backward64(delta, q_base, grad_q, grad_t, reg=0.0):
    """gs_pose_compose_backward in float64, not rounded: -> (grad_delta (V,6), magnitude (V,6)); magnitude: the sum of the
    absolute values of the terms of every element, what the bar is relative to"""
    delta, q_base, grad_q, grad_t = (np.asarray(a, dtype=np.float64) for a in (delta, q_base, grad_q, grad_t))
    reg = float(np.float32(reg))
    V, K = q_base.shape[:2]
    out, mag = np.zeros((V, 6)), np.zeros((V, 6))
    with np.errstate(all="ignore"):
        for v in range(V):
            d = delta[v]
            Gu, Gdq, Mu, Mdq = np.zeros(3), np.zeros(4), np.zeros(3), np.zeros(4)
            for k in range(K):
                x, y, z, w = q_base[v, k]
                g0, g1, g2, g3 = grad_q[v, k]
                h0, h1, h2 = grad_t[v, k]
                R = rotation(q_base[v, k])
                for j in range(3):
                    Gu[j] += (R[0, j] * h0 + R[1, j] * h1) + R[2, j] * h2
                    Mu[j] += abs(R[0, j] * h0) + abs(R[1, j] * h1) + abs(R[2, j] * h2)
                Gdq[0] += ((w * g0 + z * g1) - y * g2) - x * g3
                Gdq[1] += ((-(z * g0) + w * g1) + x * g2) - y * g3
                Gdq[2] += ((y * g0 - x * g1) + w * g2) - z * g3
                Gdq[3] += ((x * g0 + y * g1) + z * g2) + w * g3
                Mdq += [abs(w * g0) + abs(z * g1) + abs(y * g2) + abs(x * g3), abs(z * g0) + abs(w * g1) + abs(x * g2) + abs(y * g3),
                        abs(y * g0) + abs(x * g1) + abs(w * g2) + abs(z * g3), abs(x * g0) + abs(y * g1) + abs(z * g2) + abs(w * g3)]
            s = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            A, C, B = coefficients(s)
            dot = (d[0] * Gdq[0] + d[1] * Gdq[1]) + d[2] * Gdq[2]
            mdot = abs(d[0]) * Mdq[0] + abs(d[1]) * Mdq[1] + abs(d[2]) * Mdq[2]
            for j in range(3):
                Gw = (A * Gdq[j] + (B * d[j]) * dot) - ((A * d[j]) / 2.0) * Gdq[3]
                out[v, j] = Gw + reg * d[j]
                out[v, 3 + j] = Gu[j] + reg * d[3 + j]
                mag[v, j] = abs(A) * Mdq[j] + abs(B * d[j]) * mdot + abs(A * d[j] / 2.0) * Mdq[3] + abs(reg * d[j])
                mag[v, 3 + j] = Mu[j] + abs(reg * d[3 + j])
    return out, mag


def backward(delta, q_base, grad_q, grad_t, reg=0.0):
    """-> (grad_delta float32 (V,6), magnitude float64 (V,6))"""
    out, mag = backward64(np.asarray(delta, np.float32), np.asarray(q_base, np.float32), np.asarray(grad_q, np.float32),
                          np.asarray(grad_t, np.float32), reg)
    with np.errstate(all="ignore"):
        return out.astype(np.float32), mag


def ulps_apart(got, want):
    """-> for every element, how many float32 values lie between got and want (0: the same bits or both NaN; -0 and +0 are 1
    apart); a NaN on one side only is 2^32"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    a, b = got.view(np.int32).astype(np.int64), want.view(np.int32).astype(np.int64)
    a, b = np.where(a < 0, -(a & 0x7fffffff) - 1, a), np.where(b < 0, -(b & 0x7fffffff) - 1, b)
    d = np.abs(a - b)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    return np.where(nan_g & nan_w, 0, np.where(nan_g | nan_w, 2 ** 32, d))


def lr_at(iteration, lr=1e-3, lr_final=1e-4, num_iterations=None, start_iteration=0):
    if num_iterations is None:
        return lr
    t = min(max((iteration - start_iteration) / max(num_iterations - start_iteration, 1), 0.0), 1.0)
    return float(np.exp((1 - t) * np.log(lr) + t * np.log(lr_final)))
