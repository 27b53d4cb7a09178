"""The float64 reference of the geometry regularisers (include/gs_geometry.h), restated in numpy: the depth-derived normal, the
normal loss and the depth smoothness, each with its analytic backward.  No package import.

Every function works on whole planes, but a pixel's operations are the header's, in the header's order: a neighbour is a
shifted view of the plane (what lies outside the picture is an invalid depth and a zero weight), a selection is a mask, and a
gather adds its contributions one after the other in the header's order (an unselected one adds 0.0, which changes nothing).
Only the sums over the picture are numpy's (pairwise), not the device's block order: the difference is of the order of 1e-16.

The backward functions also return, per element, the summed magnitude of the contributions gathered into it: what the bars of
the GPU tests are relative to."""
import numpy as np

PRIOR_UNIT_RANGE, PRIOR_FLIP_YZ, NORMAL_FLAGS_ALL = 1, 2, 3
INVERSE, SECOND_ORDER, SMOOTH_FLAGS_ALL = 4, 8, 12
TILE_W, TILE_H, HALO = 64, 16, 2
FINISH_THREADS = 256
LOSS_TERMS = 8
FLT_MAX = np.float32(np.finfo(np.float32).max)
DBL_MAX = np.finfo(np.float64).max


def shift(plane, dy, dx, fill=0):
    """-> B with B[y, x] = plane[y + dy, x + dx], `fill` outside the picture"""
    H, W = plane.shape
    out = np.full_like(plane, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    if abs(dy) < H and abs(dx) < W:
        out[yd, xd] = plane[ys, xs]
    return out


def _depth_plane(D):
    """the depth as the float32 plane the device sees; a float64 array is kept as it is, so that a test can look at the
    formulas without the rounding of their input"""
    D = np.asarray(D)
    return D if D.dtype == np.float64 else D.astype(np.float32)


def valid_depth(D):
    with np.errstate(invalid="ignore"):
        return (D > 0) & (D <= FLT_MAX)


def clamp_weight(w):
    """a = w > 0 ? w : 0 of a float32 plane"""
    w = np.asarray(w, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(w > 0, w, np.float32(0))


def _camera(K):
    """(fx, fy, cx, cy) as the float64 values of the float32 arguments"""
    return tuple(np.float64(np.float32(v)) for v in K)


def _ab(H, W, K):
    """a_x (1,W) and b_y (H,1), and accessors for a_{x+k}, b_{y+k}"""
    fx, fy, cx, cy = _camera(K)
    a = lambda k: ((np.arange(W, dtype=np.float64)[None, :] + np.float64(k)) + 0.5 - cx) / fx     # noqa: E731  (x + k is exact)
    b = lambda k: ((np.arange(H, dtype=np.float64)[:, None] + np.float64(k)) + 0.5 - cy) / fy     # noqa: E731
    return a, b


# ---- the normal ---------------------------------------------------------------------------------------------------------------
def normal_fields(D, K, max_rel_jump=0.0):
    """-> dict(exists (H,W) bool, px, py, c (3,H,W), len (H,W)) of a float32 depth plane; the values are 0 where the normal does
    not exist"""
    D = _depth_plane(D)
    H, W = D.shape
    jump = np.float32(max_rel_jump)
    l, r, u, d = shift(D, 0, -1), shift(D, 0, 1), shift(D, -1, 0), shift(D, 1, 0)
    yy, xx = np.mgrid[0:H, 0:W]
    exists = (xx >= 1) & (xx <= W - 2) & (yy >= 1) & (yy <= H - 2)
    for v in (l, r, u, d, D):
        exists &= valid_depth(v)
    z = lambda v: np.where(exists, v, 0).astype(np.float64)      # noqa: E731  (nothing unselected is computed with)
    l, r, u, d, m = z(l), z(r), z(u), z(d), z(D)
    dx, dy = r - l, d - u
    if jump > 0:
        lim = np.float64(jump) * m
        exists = exists & (np.abs(dx) <= lim) & (np.abs(dy) <= lim)
    a, b = _ab(H, W, K)
    px = np.stack([a(1) * r - a(-1) * l, b(0) * dx, dx])
    py = np.stack([a(0) * dy, b(1) * d - b(-1) * u, dy])
    t = np.stack([[py[1] * px[2], py[2] * px[1]], [py[2] * px[0], py[0] * px[2]], [py[0] * px[1], py[1] * px[0]]])   # (3,2,H,W)
    c = t[:, 0] - t[:, 1]
    q = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
    exists = exists & (q > 0) & (q <= DBL_MAX)
    length = np.sqrt(np.where(exists, q, 1.0))
    keep = lambda v: np.where(exists, v, 0.0)                                  # noqa: E731
    return dict(exists=exists, px=keep(px), py=keep(py), c=keep(c), len=np.where(exists, length, 1.0),
                c_magnitude=keep(np.abs(t[:, 0]) + np.abs(t[:, 1])))


def depth_normals(D, K, max_rel_jump=0.0):
    """-> (normals (3,H,W) float64, 0 where there is none; magnitude (3,H,W): (|t1| + |t2|) / len of the two products an
    element of c is the difference of)"""
    f = normal_fields(D, K, max_rel_jump)
    return np.where(f["exists"], f["c"] / f["len"], 0.0), np.where(f["exists"], f["c_magnitude"] / f["len"], 0.0)


def decode_prior(N, flags):
    """-> (usable (H,W) bool, h (3,H,W) float64 unit prior, 0 where not usable)"""
    v = np.asarray(N, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = 2.0 * v - 1.0 if flags & PRIOR_UNIT_RANGE else v.copy()
        if flags & PRIOR_FLIP_YZ:
            m[1], m[2] = -m[1], -m[2]
        k = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        usable = (k >= 0.5) & (k <= DBL_MAX)
        h = np.where(usable, m / np.where(usable, k, 1.0), 0.0)
    return usable, h


def _normal_terms(D, K, N, w_n, w_p, max_rel_jump, flags):
    f = normal_fields(D, K, max_rel_jump)
    usable, h = decode_prior(N, flags)
    w = clamp_weight(w_n)
    if w_p is not None:
        with np.errstate(invalid="ignore"):
            w = w * clamp_weight(w_p)                       # one f32 multiply
    with np.errstate(invalid="ignore"):
        selected = f["exists"] & usable & (w > 0)
    w = np.where(selected, w, np.float32(0)).astype(np.float64)
    n = np.where(selected, f["c"] / f["len"], 0.0)
    h = np.where(selected, h, 0.0)
    cos = (n[0] * h[0] + n[1] * h[1]) + n[2] * h[2]
    return f, selected, w, n, h, cos


def _terms(loss_sum, weight_sum, count, fourth=0.0):
    """the eight terms as the device rounds them: float64 values rounded once to float32"""
    out = np.zeros(LOSS_TERMS, dtype=np.float32)
    if weight_sum > 0:
        out[0], out[1], out[2], out[3] = np.float32(loss_sum / weight_sum), np.float32(weight_sum), np.float32(count), np.float32(fourth)
    return out


def normal_loss_forward(D, K, N, w_n, w_p=None, max_rel_jump=0.1, flags=0):
    """-> (terms (8,) float32, float64 values dict(L, S_w, count, mean_cos), selected (H,W))"""
    _, selected, w, n, h, cos = _normal_terms(D, K, N, w_n, w_p, max_rel_jump, flags)
    S_l, S_w, count = float(np.sum(w[selected] * (1.0 - cos[selected]))), float(np.sum(w[selected])), int(selected.sum())
    mean_cos = float(np.sum(cos[selected])) / count if count else 0.0
    values = dict(L=S_l / S_w if S_w > 0 else 0.0, S_w=S_w, count=count, mean_cos=mean_cos)
    return _terms(S_l, S_w, count, mean_cos), values, selected


def normal_loss_backward(D, K, N, w_n, w_p, max_rel_jump, flags, terms, upstream=1.0):
    """-> (grad_D (H,W) float64, magnitude (H,W), touched (H,W) bool: a selected normal reads the pixel): the gather of the header,
    S_w read from terms[1] as the float32 it is"""
    D = _depth_plane(D)
    H, W = D.shape
    f, selected, w, n, h, cos = _normal_terms(D, K, N, w_n, w_p, max_rel_jump, flags)
    S_w = np.float32(terms[1])
    if not S_w > 0:
        return np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W), dtype=bool)
    s = np.float64(np.float32(upstream)) / np.float64(S_w)
    coef = -(s * w)
    g = (coef * (h - cos * n)) / f["len"]
    px, py = f["px"], f["py"]
    gx = np.stack([g[1] * py[2] - g[2] * py[1], g[2] * py[0] - g[0] * py[2], g[0] * py[1] - g[1] * py[0]])
    gy = np.stack([px[1] * g[2] - px[2] * g[1], px[2] * g[0] - px[0] * g[2], px[0] * g[1] - px[1] * g[0]])
    a, b = _ab(H, W, K)
    owes_right = (gx[0] * a(1) + gx[1] * b(0)) + gx[2]
    owes_left = -((gx[0] * a(-1) + gx[1] * b(0)) + gx[2])
    owes_down = (gy[0] * a(0) + gy[1] * b(1)) + gy[2]
    owes_up = -((gy[0] * a(0) + gy[1] * b(-1)) + gy[2])
    grad, magnitude, touched = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W), dtype=bool)
    # left neighbour's right, right neighbour's left, upper neighbour's down, lower neighbour's up
    for owes, (dy, dx) in ((owes_right, (0, -1)), (owes_left, (0, 1)), (owes_down, (-1, 0)), (owes_up, (1, 0))):
        term = np.where(shift(selected, dy, dx, False), shift(owes, dy, dx, 0.0), 0.0)
        grad = grad + term
        magnitude = magnitude + np.abs(term)
        touched |= shift(selected, dy, dx, False)
    return grad, magnitude, touched


# ---- the smoothness -----------------------------------------------------------------------------------------------------------
def _space(D, valid, flags):
    d = np.where(valid, D, 1).astype(np.float64)
    return np.where(valid, 1.0 / d if flags & INVERSE else d, 0.0)


def _edge(I, shift_i, shift_j, edge_lambda, shape):
    """-> (allowed bool, e float64) of the guide between the pixels at the two shifts"""
    if I is None:
        return np.ones(shape, dtype=bool), np.ones(shape)
    I = np.asarray(I, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = [np.abs(shift(I[k], *shift_j) - shift(I[k], *shift_i)) for k in range(3)]
        t = ((d[0] + d[1]) + d[2]) / 3.0
        allowed = t <= DBL_MAX
        e = np.exp(-(np.float64(np.float32(edge_lambda)) * np.where(allowed, t, 0.0)))
    return allowed, e


def smooth_term_fields(D, I, w_p, edge_lambda, flags):
    """-> [horizontal, vertical], each dict(selected, w (f64 of the f32 product), we, r, members): the term OWNED by every
    pixel -- the pair that begins there, or the triple centred there -- 0 where not selected.  members: ((dy, dx), coefficient)
    of the term's pixels relative to its owner."""
    D = _depth_plane(D)
    valid = valid_depth(D)
    x = _space(D, valid, flags)
    a = np.ones(D.shape, dtype=np.float32) if w_p is None else clamp_weight(w_p)
    out = []
    for sy, sx in ((0, 1), (1, 0)):
        if flags & SECOND_ORDER:
            members = (((-sy, -sx), 1.0), ((0, 0), -2.0), ((sy, sx), 1.0))
            sel = shift(valid, -sy, -sx, False) & valid & shift(valid, sy, sx, False)
            with np.errstate(invalid="ignore"):
                w = (shift(a, -sy, -sx) * a) * shift(a, sy, sx)
            allowed, e = _edge(I, (-sy, -sx), (sy, sx), edge_lambda, D.shape)
            r = (shift(x, -sy, -sx) - 2.0 * x) + shift(x, sy, sx)
        else:
            members = (((0, 0), -1.0), ((sy, sx), 1.0))
            sel = valid & shift(valid, sy, sx, False)
            with np.errstate(invalid="ignore"):
                w = a * shift(a, sy, sx)
            allowed, e = _edge(I, (0, 0), (sy, sx), edge_lambda, D.shape)
            r = shift(x, sy, sx) - x
        with np.errstate(invalid="ignore"):
            sel = sel & (w > 0) & allowed
        w = np.where(sel, w, np.float32(0)).astype(np.float64)
        out.append(dict(selected=sel, w=w, we=np.where(sel, w * np.where(sel, e, 0.0), 0.0), r=np.where(sel, r, 0.0), members=members))
    return out


def depth_smooth_forward(D, I=None, w_p=None, edge_lambda=10.0, flags=0):
    """-> (terms (8,) float32, dict(L, S_w, count))"""
    S_l = S_w = 0.0
    count = 0
    for t in smooth_term_fields(D, I, w_p, edge_lambda, flags):
        sel = t["selected"]
        S_l += float(np.sum(t["we"][sel] * np.abs(t["r"][sel])))
        S_w += float(np.sum(t["w"][sel]))
        count += int(sel.sum())
    return _terms(S_l, S_w, count), dict(L=S_l / S_w if S_w > 0 else 0.0, S_w=S_w, count=count)


def depth_smooth_backward(D, I, w_p, edge_lambda, flags, terms, upstream=1.0):
    """-> (grad_D (H,W) float64, magnitude (H,W), touched (H,W) bool): the gather of the header in its order -- horizontal terms first, and of a
    direction the term owned by the pixel before, (second order: by the pixel itself,) by the pixel (after)"""
    D = _depth_plane(D)
    S_w = np.float32(terms[1])
    if not S_w > 0:
        return np.zeros(D.shape), np.zeros(D.shape), np.zeros(D.shape, dtype=bool)
    s = np.float64(np.float32(upstream)) / np.float64(S_w)
    acc, magnitude, touched = np.zeros(D.shape), np.zeros(D.shape), np.zeros(D.shape, dtype=bool)
    for t in smooth_term_fields(D, I, w_p, edge_lambda, flags):
        k = t["we"] * (np.where(t["r"] > 0, 1.0, 0.0) - np.where(t["r"] < 0, 1.0, 0.0))
        # pixel p is the member at offset o of the term owned by p - o: the members in reverse visit the owners in ascending order
        for (dy, dx), coefficient in reversed(t["members"]):
            term = coefficient * shift(k, -dy, -dx, 0.0)
            acc = acc + term
            magnitude = magnitude + np.abs(term)
            touched |= shift(t["selected"], -dy, -dx, False)
    grad, magnitude = acc * s, magnitude * abs(s)
    if flags & INVERSE:
        x = _space(D, valid_depth(D), flags)
        grad, magnitude = grad * -(x * x), magnitude * (x * x)
    return np.where(touched, grad, 0.0), magnitude, touched
