"""include/gs_appearance.h restated in numpy: the yardstick of the exposure-compensation tests.

Images are (3,H,W) float32 arrays, a transform is 12 float32 values, row-major [A | b].  apply() and grad_image() follow the
header's f32 operation order, so the library is compared with them bit for bit; the sums (grad_transform, moments) are float64
sums of float64 products of the f32 inputs -- exact to a few ulp of float64 -- and come with the sum of the magnitudes of
their terms, which the tolerance of a comparison is stated in.
"""
import numpy as np

PIXELS_PER_BLOCK = 1024
FINISH_THREADS = 256
FINISH_BLOCKS_BACKWARD, FINISH_BLOCKS_MOMENTS = 12, 23
TRANSFORM_FLOATS = 12
MOMENTS = 23
UPPER_TRIANGLE = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64)
# the project's per-element gradient bar (README, parity row): |got - want| <= ABS + REL * sum |terms|
BAR_ABS, BAR_REL = 2e-5, 5e-6


def _f32(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a


def apply(image, transform):
    """c_i = ((A_i0 x_0 + A_i1 x_1) + A_i2 x_2) + b_i, every operation rounded to f32"""
    x, M = _f32(image), _f32(transform).reshape(3, 4)
    with np.errstate(all="ignore"):
        return np.stack([((M[i, 0] * x[0] + M[i, 1] * x[1]) + M[i, 2] * x[2]) + M[i, 3] for i in range(3)]).astype(np.float32)


def selected(grad_corrected):
    """(H,W) bool: at least one of the three upstream values is not exactly 0 (a NaN is not 0)"""
    g = _f32(grad_corrected)
    return ~((g[0] == 0) & (g[1] == 0) & (g[2] == 0))


def grad_image(grad_corrected, transform):
    """grad_image_j = (A_0j g_0 + A_1j g_1) + A_2j g_2 in f32 where the pixel is selected, exactly +0 elsewhere"""
    g, M = _f32(grad_corrected), _f32(transform).reshape(3, 4)
    sel = selected(g)
    with np.errstate(all="ignore"):
        out = np.stack([(M[0, j] * g[0] + M[1, j] * g[1]) + M[2, j] * g[2] for j in range(3)]).astype(np.float32)
    out[:, ~sel] = 0.0
    return out


def grad_transform(image, grad_corrected):
    """-> (value (12,) float64, magnitude (12,) float64): sum over the selected pixels of g_i x_j (j < 3) and of g_i (j = 3), and
    the same sums of the terms' absolute values"""
    x, g = _f32(image).astype(np.float64), _f32(grad_corrected).astype(np.float64)
    sel = selected(grad_corrected)
    value, magnitude = np.zeros((3, 4)), np.zeros((3, 4))
    for i in range(3):
        gi = g[i][sel]
        for j in range(4):
            terms = gi * x[j][sel] if j < 3 else gi
            value[i, j], magnitude[i, j] = terms.sum(), np.abs(terms).sum()
    return value.reshape(12), magnitude.reshape(12)


def effective_weight(pixel_weight, shape):
    """w as the library has it: the weight where it is > 0, else 0 (negative and NaN included); None: ones"""
    if pixel_weight is None:
        return np.ones(shape, dtype=np.float64)
    w = _f32(pixel_weight)
    with np.errstate(invalid="ignore"):
        return np.where(w > 0, w, np.float32(0)).astype(np.float64)


def moments(image, target, pixel_weight=None):
    """-> (value (23,) float64, magnitude (23,) float64).  A pixel with w == 0 is left out, whatever it holds."""
    x, y = _f32(image).astype(np.float64), _f32(target).astype(np.float64)
    w = effective_weight(pixel_weight, x.shape[1:])
    sel = w > 0
    w = w[sel]
    u = [x[0][sel], x[1][sel], x[2][sel], np.ones_like(w)]
    terms = [(w * u[i]) * u[j] for i, j in UPPER_TRIANGLE]
    terms += [y[i][sel] * (w * u[j]) for i in range(3) for j in range(4)]
    terms.append(w)
    return np.array([t.sum() for t in terms]), np.array([np.abs(t).sum() for t in terms])


def solve_affine(m):
    """The fit of the package (appearance.solve_affine) restated: the solution of (sum w u u^T) M_i^T = sum w y_i u in float64;
    identity when sum w == 0, a moment is not finite, or the system scaled to a unit diagonal has a condition number >= 1e12"""
    m = np.asarray(m, dtype=np.float64).reshape(MOMENTS)
    if not np.all(np.isfinite(m)) or not m[22] > 0:
        return IDENTITY.copy()
    G = np.zeros((4, 4))
    for value, (i, j) in zip(m[:10], UPPER_TRIANGLE):
        G[i, j] = G[j, i] = value
    B = m[10:22].reshape(3, 4)
    d = np.sqrt(np.diag(G))
    if not np.all(d > 0):
        return IDENTITY.copy()
    Gn = G / np.outer(d, d)
    if not np.linalg.cond(Gn) < 1e12:
        return IDENTITY.copy()
    M = np.linalg.solve(Gn, (B / d).T).T / d
    return M.reshape(12) if np.all(np.isfinite(M)) else IDENTITY.copy()


def within_bar(got, want, magnitude):
    """-> (ok, worst): every |got - want| <= BAR_ABS + BAR_REL * magnitude; worst = the largest |got - want| / that bound"""
    got, want, magnitude = (np.asarray(a, dtype=np.float64) for a in (got, want, magnitude))
    ratio = np.abs(got - want) / (BAR_ABS + BAR_REL * magnitude)
    return bool(np.all(ratio <= 1.0)), float(np.max(ratio))


def lr_at(iteration, lr=0.01, lr_final=0.001, num_iterations=None):
    if num_iterations is None:
        return lr
    t = min(max(iteration / num_iterations, 0.0), 1.0)
    return float(np.exp((1 - t) * np.log(lr) + t * np.log(lr_final)))
