"""The float64 reference of include/gs_normals.h, restated in numpy: the normal of a Gaussian with its gradient to the quaternion,
and the consistency of the rendered normals with the depth normal (the depth normal itself is geometry_ref's).  No package import.

As in geometry_ref: whole arrays, but a row's or a pixel's operations are the header's, in the header's order; a selection is a
mask; only the sums over the picture are numpy's.  The backward functions also return, per element, the summed magnitude of what
was added into it: what the bars of the GPU tests are relative to."""
import numpy as np

import geometry_ref as G

FEATURES, BLOCK, MAX_PIXELS, LOSS_TERMS = 56, 256, 715827200, 8
FORWARD_LAUNCHES, BACKWARD_LAUNCHES = 2, 1
DBL_MAX = G.DBL_MAX


def rotation(q):
    """R(q) (..., 3, 3) of float64 quaternions (..., 4) xyzw, as stored: rotation_from_quaternion in float64"""
    x, y, z, w = (q[..., k] for k in range(4))
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    rows = [[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
            [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
            [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]]
    return np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)


def column_partials(k, q):
    """J (N, 4, 3): J[i, e, j] = d c_j / d q_e of column k[i] of R(q[i])"""
    x, y, z, w = (q[:, e] for e in range(4))
    o = np.zeros_like(x)
    tables = [
        [[o, 2 * y, 2 * z], [-4 * y, 2 * x, -2 * w], [-4 * z, 2 * w, 2 * x], [o, 2 * z, -2 * y]],
        [[2 * y, -4 * x, 2 * w], [2 * x, o, 2 * z], [-2 * w, -4 * z, 2 * y], [-2 * z, o, 2 * x]],
        [[2 * z, -2 * w, -4 * x], [2 * w, 2 * z, -4 * y], [2 * x, 2 * y, o], [2 * y, -2 * x, o]],
    ]
    J = np.stack([np.stack([np.stack(row, axis=-1) for row in t], axis=-2) for t in tables])          # (3, N, 4, 3)
    return J[k, np.arange(len(k))]


def _rows(point_cloud, features, q_pc, t_pc, point_object_id):
    """what forward and backward share: dict(ok, k, q, u, l, P, m, flip, a, p); rows that are zeroed compute with harmless values"""
    pc = np.asarray(point_cloud, dtype=np.float32)
    f = np.asarray(features, dtype=np.float32)
    N, K = len(pc), len(q_pc)
    oid = np.zeros(N, dtype=np.int64) if point_object_id is None else np.asarray(point_object_id).astype(np.int64)
    ok = (oid >= 0) & (oid < K)
    ok &= np.isfinite(f[:, :7]).all(axis=1) & np.isfinite(pc).all(axis=1)
    oid = np.where(ok, oid, 0)
    s = f[:, 4:7]
    k = np.zeros(N, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        k = np.where(s[:, 1] < s[np.arange(N), k], 1, k)
        k = np.where(s[:, 2] < s[np.arange(N), k], 2, k)
    q = np.where(ok[:, None], f[:, :4], 0).astype(np.float64)
    ok &= ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3] > 0
    R = rotation(q)
    c = R[np.arange(N), :, k]                                                   # column k
    l2 = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
    ok &= (l2 > 0) & (l2 <= DBL_MAX)
    l = np.sqrt(np.where(ok, l2, 1.0))
    u = c / l[:, None]
    P = rotation(np.asarray(q_pc, dtype=np.float32).astype(np.float64))[oid]      # (N,3,3)
    t = np.asarray(t_pc, dtype=np.float32).astype(np.float64)[oid]
    d = np.where(ok[:, None], pc, 0).astype(np.float64) - t
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.stack([(P[:, 0, j] * u[:, 0] + P[:, 1, j] * u[:, 1]) + P[:, 2, j] * u[:, 2] for j in range(3)], axis=1)
        p = np.stack([(P[:, 0, j] * d[:, 0] + P[:, 1, j] * d[:, 1]) + P[:, 2, j] * d[:, 2] for j in range(3)], axis=1)
        a = (m[:, 0] * p[:, 0] + m[:, 1] * p[:, 1]) + m[:, 2] * p[:, 2]
        flip = ~(a <= 0)
    return dict(ok=ok, k=k, q=q, u=u, l=l, P=P, m=m, flip=flip, a=a, p=p)


def gaussian_normals_forward(point_cloud, features, q_pc, t_pc, point_object_id=None):
    """-> (normals (N,3) float64, 0 for a zeroed row; magnitude (N,3): the summed magnitude of the three products of m_j)"""
    r = _rows(point_cloud, features, q_pc, t_pc, point_object_id)
    n = np.where(r["flip"][:, None], -r["m"], r["m"])
    P, u = r["P"], r["u"]
    mag = np.stack([(np.abs(P[:, 0, j] * u[:, 0]) + np.abs(P[:, 1, j] * u[:, 1])) + np.abs(P[:, 2, j] * u[:, 2]) for j in range(3)], axis=1)
    ok = r["ok"][:, None]
    return np.where(ok, n, 0.0), np.where(ok, mag, 0.0)


def gaussian_normals_backward(point_cloud, features, q_pc, t_pc, point_object_id, grad_normals):
    """-> (grad_features (N,56) float64, magnitude (N,56)): columns 0..3 by the header, the rest 0"""
    r = _rows(point_cloud, features, q_pc, t_pc, point_object_id)
    g = np.asarray(grad_normals, dtype=np.float32).astype(np.float64)
    N = len(g)
    gm = np.where(r["flip"][:, None], -g, g)
    P, u, l = r["P"], r["u"], r["l"]
    gu = np.stack([(P[:, j, 0] * gm[:, 0] + P[:, j, 1] * gm[:, 1]) + P[:, j, 2] * gm[:, 2] for j in range(3)], axis=1)
    gu_mag = np.stack([(np.abs(P[:, j, 0] * gm[:, 0]) + np.abs(P[:, j, 1] * gm[:, 1])) + np.abs(P[:, j, 2] * gm[:, 2]) for j in range(3)], axis=1)
    b = (gu[:, 0] * u[:, 0] + gu[:, 1] * u[:, 1]) + gu[:, 2] * u[:, 2]
    b_mag = (gu_mag[:, 0] * np.abs(u[:, 0]) + gu_mag[:, 1] * np.abs(u[:, 1])) + gu_mag[:, 2] * np.abs(u[:, 2])
    gc = (gu - b[:, None] * u) / l[:, None]
    gc_mag = (gu_mag + b_mag[:, None] * np.abs(u)) / l[:, None]
    J = column_partials(r["k"], r["q"])
    out, mag = np.zeros((N, FEATURES)), np.zeros((N, FEATURES))
    for e in range(4):
        out[:, e] = (J[:, e, 0] * gc[:, 0] + J[:, e, 1] * gc[:, 1]) + J[:, e, 2] * gc[:, 2]
        mag[:, e] = (np.abs(J[:, e, 0]) * gc_mag[:, 0] + np.abs(J[:, e, 1]) * gc_mag[:, 1]) + np.abs(J[:, e, 2]) * gc_mag[:, 2]
    ok = r["ok"][:, None]
    return np.where(ok, out, 0.0), np.where(ok, mag, 0.0)


# ---- the consistency loss -------------------------------------------------------------------------------------------------------
def _consistency_terms(D, K, R, w_p, max_rel_jump, min_length):
    f = G.normal_fields(D, K, max_rel_jump)
    m = np.moveaxis(np.asarray(R, dtype=np.float32).astype(np.float64), 2, 0)              # (3,H,W)
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        usable = (k >= np.float64(np.float32(min_length))) & (k <= DBL_MAX)
    w = np.ones(f["exists"].shape, dtype=np.float32) if w_p is None else G.clamp_weight(w_p)
    selected = f["exists"] & usable & (w > 0)
    k = np.where(selected, k, 1.0)
    w = np.where(selected, w, np.float32(0)).astype(np.float64)
    h = np.where(selected, np.where(selected, m, 0.0) / k, 0.0)
    n = np.where(selected, f["c"] / f["len"], 0.0)
    cos = (n[0] * h[0] + n[1] * h[1]) + n[2] * h[2]
    return f, selected, w, n, h, cos, k


def normal_consistency_forward(D, K, R, w_p=None, max_rel_jump=0.1, min_length=0.5):
    """-> (terms (8,) float32, float64 values dict(L, S_w, count, mean_cos), selected (H,W))"""
    _, selected, w, n, h, cos, _ = _consistency_terms(D, K, R, w_p, max_rel_jump, min_length)
    S_l, S_w, count = float(np.sum(w[selected] * (1.0 - cos[selected]))), float(np.sum(w[selected])), int(selected.sum())
    mean_cos = float(np.sum(cos[selected])) / count if count else 0.0
    values = dict(L=S_l / S_w if S_w > 0 else 0.0, S_w=S_w, count=count, mean_cos=mean_cos)
    return G._terms(S_l, S_w, count, mean_cos), values, selected


def normal_consistency_backward(D, K, R, w_p, max_rel_jump, min_length, terms, upstream=1.0):
    """-> (grad_D (H,W), its magnitude, touched (H,W) bool, grad_R (H,W,3), its magnitude, selected (H,W)), all float64"""
    D = G._depth_plane(D)
    H, W = D.shape
    f, selected, w, n, h, cos, k = _consistency_terms(D, K, R, w_p, max_rel_jump, min_length)
    S_w = np.float32(terms[1])
    zero = np.zeros((H, W))
    if not S_w > 0:
        return zero, zero, np.zeros((H, W), dtype=bool), np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W), dtype=bool)
    s = np.float64(np.float32(upstream)) / np.float64(S_w)
    coef = -(s * w)
    g = (coef * (h - cos * n)) / f["len"]
    px, py = f["px"], f["py"]
    gx = np.stack([g[1] * py[2] - g[2] * py[1], g[2] * py[0] - g[0] * py[2], g[0] * py[1] - g[1] * py[0]])
    gy = np.stack([px[1] * g[2] - px[2] * g[1], px[2] * g[0] - px[0] * g[2], px[0] * g[1] - px[1] * g[0]])
    a, b = G._ab(H, W, K)
    owes_right = (gx[0] * a(1) + gx[1] * b(0)) + gx[2]
    owes_left = -((gx[0] * a(-1) + gx[1] * b(0)) + gx[2])
    owes_down = (gy[0] * a(0) + gy[1] * b(1)) + gy[2]
    owes_up = -((gy[0] * a(0) + gy[1] * b(-1)) + gy[2])
    grad, magnitude, touched = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W), dtype=bool)
    for owes, (dy, dx) in ((owes_right, (0, -1)), (owes_left, (0, 1)), (owes_down, (-1, 0)), (owes_up, (1, 0))):
        term = np.where(G.shift(selected, dy, dx, False), G.shift(owes, dy, dx, 0.0), 0.0)
        grad = grad + term
        magnitude = magnitude + np.abs(term)
        touched |= G.shift(selected, dy, dx, False)
    grad_R = np.where(selected, (coef * (n - cos * h)) / k, 0.0)
    mag_R = np.where(selected, (np.abs(coef) * (np.abs(n) + np.abs(cos * h))) / k, 0.0)
    return grad, magnitude, touched, np.moveaxis(grad_R, 0, 2), np.moveaxis(mag_R, 0, 2), selected
