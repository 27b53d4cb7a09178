"""include/gs_background.h restated in numpy: the yardstick of the background tests.

Images are (3,H,W) float32 arrays, alpha an (H,W) one, a background 48 float32 values coef[16 i + k].  Everything with
dtype=np.float32 follows the header's f32 operation order, operation for operation -- the block and finishing sums of the
backward included, derived from the header's constants -- so the library is compared with it bit for bit.  The same functions
with dtype=np.float64 are the closed form: the formulas in double, with plain sums.  basis() and colour() are written with
arithmetic operators alone, so torch tensors go through them too (the autograd reference of the host tests).
"""
import numpy as np

PIXELS_PER_BLOCK = 1024
FINISH_THREADS = 256
FINISH_BLOCKS = 48
COEF_FLOATS = 48
MAX_BANDS = 3
STRAIGHT, COLOURS_ONLY = 1, 2
WAVE = 64
THREADS = PIXELS_PER_BLOCK // 4
WHITE = np.array(([1.0] + [0.0] * 15) * 3, dtype=np.float32)


def _f32(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a


def rotation(q, c=np.float32):
    """rotation_from_quaternion: q = xyzw, not normalised -> the nine entries, row-major"""
    x, y, z, w = q[0], q[1], q[2], q[3]
    xx, yy, zz = x * x, y * y, z * z
    xy, xz, yz = x * y, x * z, y * z
    wx, wy, wz = w * x, w * y, w * z
    one, two = c(1.0), c(2.0)
    return [one - two * (yy + zz), two * (xy - wz), two * (xz + wy),
            two * (xy + wz), one - two * (xx + zz), two * (yz - wx),
            two * (xz - wy), two * (yz + wx), one - two * (xx + yy)]


def sh16(x, y, z, c=np.float32):
    """the rasteriser's 16 basis values of a direction, in its operation order; entry 0 is the basis' own constant"""
    return [c(0.28209479177387814),
            c(-0.48860251190291987) * y,
            c(0.48860251190291987) * z,
            c(-0.48860251190291987) * x,
            c(1.0925484305920792) * x * y,
            c(-1.0925484305920792) * y * z,
            c(0.94617469575755997) * z * z - c(0.31539156525251999),
            c(-1.0925484305920792) * x * z,
            c(0.54627421529603959) * x * x - c(0.54627421529603959) * y * y,
            c(0.59004358992664352) * y * (c(-3.0) * x * x + y * y),
            c(2.8906114426405538) * x * y * z,
            c(0.45704579946446572) * y * (c(1.0) - c(5.0) * z * z),
            c(0.3731763325901154) * z * (c(5.0) * z * z - c(3.0)),
            c(0.45704579946446572) * x * (c(1.0) - c(5.0) * z * z),
            c(1.4453057213202769) * z * (x * x - y * y),
            c(0.59004358992664352) * x * (-x * x + c(3.0) * y * y)]


def basis(px, py, q, K9, c=np.float32, sqrt=np.sqrt):
    """Y_1 .. Y_15 of the pixels (px, py) (already in the working precision) -> a list of 16, entry 0 the number 1"""
    fx, cx, fy, cy = K9[0], K9[2], K9[4], K9[5]
    a = ((px + c(0.5)) - cx) / fx
    b = ((py + c(0.5)) - cy) / fy
    n = sqrt((a * a + b * b) + c(1.0))
    d0, d1, d2 = a / n, b / n, c(1.0) / n
    R = rotation(q, c)
    d = [(R[3 * j] * d0 + R[3 * j + 1] * d1) + R[3 * j + 2] * d2 for j in range(3)]
    Y = sh16(d[0], d[1], d[2], c)
    Y[0] = c(1.0)
    return Y


def colour(coef, Y, bands):
    """c_i = (..(coef[16i] + coef[16i+1] Y_1) ..) + coef[16i+K-1] Y_{K-1} -> a list of three"""
    out = []
    for i in range(3):
        v = coef[16 * i]
        for k in range(1, (bands + 1) ** 2):
            v = v + coef[16 * i + k] * Y[k]
        out.append(v)
    return out


def _grid(H, W, dtype):
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return px.astype(dtype), py.astype(dtype)


def _basis_np(bands, q, K9, H, W, dtype):
    """(16,H,W) of dtype; only the first K rows mean anything"""
    Y = np.zeros((16, H, W), dtype=dtype)
    Y[0] = 1
    if bands > 0:
        px, py = _grid(H, W, dtype)
        q = np.asarray(q, dtype=dtype).reshape(4)
        K9 = np.asarray(K9, dtype=dtype).reshape(9)
        with np.errstate(all="ignore"):
            full = basis(px, py, q, K9, dtype)
        for k in range(1, (bands + 1) ** 2):
            Y[k] = full[k]
    return Y


def colours(coef, bands, q, K9, H, W, dtype=np.float32):
    """(3,H,W): the background's colour at every pixel"""
    coef = np.asarray(coef).astype(dtype).reshape(COEF_FLOATS)
    Y = _basis_np(bands, q, K9, H, W, dtype)
    with np.errstate(all="ignore"):
        c = colour(coef, Y, bands)
    return np.stack([np.broadcast_to(np.asarray(ci, dtype=dtype), (H, W)) for ci in c]).astype(dtype)


def composite(image, alpha, coef, bands, q=None, K9=None, flags=0, dtype=np.float32):
    """out_i = x_i + t c_i, x_i A + t c_i (STRAIGHT) or c_i (COLOURS_ONLY; image = (H, W) then), t = 1 - A"""
    if flags & COLOURS_ONLY:
        H, W = image
        return colours(coef, bands, q, K9, H, W, dtype)
    x, A = np.asarray(image).astype(dtype), np.asarray(alpha).astype(dtype)
    c = colours(coef, bands, q, K9, x.shape[1], x.shape[2], dtype)
    with np.errstate(all="ignore"):
        t = dtype(1.0) - A
        fg = x * A if flags & STRAIGHT else x
        return (fg + t * c).astype(dtype)


def selected(grad_out):
    """(H,W) bool: at least one of the three upstream values is not exactly 0 (a NaN is not 0)"""
    g = np.asarray(grad_out)
    return ~((g[0] == 0) & (g[1] == 0) & (g[2] == 0))


def grad_alpha(grad_out, coef, bands, q=None, K9=None, dtype=np.float32):
    """-((g_0 c_0 + g_1 c_1) + g_2 c_2) where the pixel is selected, exactly +0 elsewhere"""
    g = np.asarray(grad_out).astype(dtype)
    c = colours(coef, bands, q, K9, g.shape[1], g.shape[2], dtype)
    with np.errstate(all="ignore"):
        out = (-((g[0] * c[0] + g[1] * c[1]) + g[2] * c[2])).astype(dtype)
    out[~selected(grad_out)] = 0.0
    return out


def _butterfly(v):
    """v[..., 64] -> v[..., 0] after v_l <- v_l + v_{l ^ o}, o = 32, 16, 8, 4, 2, 1"""
    lanes = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def block_sums(terms, sel):
    """terms (n,) f32 per pixel, sel (n,) bool -> (blocks,) f32: the header's per-block sums"""
    n = terms.shape[0]
    nb = (n + PIXELS_PER_BLOCK - 1) // PIXELS_PER_BLOCK
    t = np.zeros(nb * PIXELS_PER_BLOCK, dtype=np.float32)
    t[:n] = np.where(sel, terms, np.float32(0.0))
    t = t.reshape(nb, THREADS // WAVE, WAVE, 4)
    with np.errstate(all="ignore"):
        acc = np.zeros(t.shape[:3], dtype=np.float32)
        for k in range(4):                                  # the thread's four pixels in ascending order
            acc = acc + t[..., k]
        waves = _butterfly(acc)                             # (nb, 4)
        total = waves[:, 0]
        for w in range(1, THREADS // WAVE):
            total = total + waves[:, w]
    assert total.dtype == np.float32
    return total


def finish(partial):
    """(blocks,) f32 -> one f32: the finishing block's float64 sum, rounded once"""
    nb = partial.shape[0]
    rounds = (nb + FINISH_THREADS - 1) // FINISH_THREADS
    p = np.zeros(rounds * FINISH_THREADS, dtype=np.float64)
    p[:nb] = partial.astype(np.float64)
    p = p.reshape(rounds, FINISH_THREADS)
    with np.errstate(all="ignore"):
        a = np.zeros(FINISH_THREADS, dtype=np.float64)
        for r in range(rounds):                             # thread u: the blocks u, u + threads, ...
            a = a + p[r]
        waves = _butterfly(a.reshape(FINISH_THREADS // WAVE, WAVE))
        total = waves[0]
        for w in range(1, FINISH_THREADS // WAVE):
            total = total + waves[w]
        return np.float32(total)


def grad_coef(grad_out, alpha, bands, q=None, K9=None, dtype=np.float32):
    """(48,): sum over the selected pixels of (g_i t) Y_k, Y_0 := 1; +0 for k >= K.  float32: the header's sums, bit for bit;
    float64: plain sums of the same terms in double"""
    g, A = np.asarray(grad_out).astype(dtype), np.asarray(alpha).astype(dtype)
    H, W = A.shape
    K = (bands + 1) ** 2
    sel = selected(grad_out).reshape(-1)
    Y = _basis_np(bands, q, K9, H, W, dtype)
    out = np.zeros(COEF_FLOATS, dtype=dtype)
    with np.errstate(all="ignore"):
        t = dtype(1.0) - A
        for i in range(3):
            gt = (g[i] * t).reshape(-1)
            for k in range(K):
                terms = gt if k == 0 else gt * Y[k].reshape(-1)
                if dtype == np.float32:
                    out[16 * i + k] = finish(block_sums(terms, sel))
                else:
                    out[16 * i + k] = terms[sel].sum()
    return out


def grad_coef_magnitude(grad_out, alpha, bands, q=None, K9=None):
    """(48,) float64: the sums of the absolute values of grad_coef's terms"""
    g, A = np.asarray(grad_out).astype(np.float64), np.asarray(alpha).astype(np.float64)
    sel = selected(grad_out)
    Y = _basis_np(bands, q, K9, A.shape[0], A.shape[1], np.float64)
    out = np.zeros(COEF_FLOATS)
    for i in range(3):
        for k in range((bands + 1) ** 2):
            out[16 * i + k] = np.abs((g[i] * (1.0 - A) * Y[k])[sel]).sum()
    return out


def camera(H, W, fx=None, fy=None, cx=None, cy=None):
    """a row-major (3,3) float32 camera matrix; the defaults are a centred pinhole with a 90 degree horizontal field"""
    fx = W / 2.0 if fx is None else fx
    return np.array([fx, 0, W / 2.0 if cx is None else cx, 0, fx if fy is None else fy, H / 2.0 if cy is None else cy, 0, 0, 1],
                    dtype=np.float32).reshape(3, 3)
