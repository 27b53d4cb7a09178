"""include/gs_bilateral.h restated in numpy: the yardstick of the bilateral-grid tests.

Images are (3,H,W) arrays, a grid is (Gy,Gx,L,12), vertex (iy,ix,l) a row-major [A | b].  Every function takes the number
format `f`: with f = np.float32 it follows the header's f32 operation order -- and, for the grid's gradient and the total
variation, the header's summation order (thread, butterfly, waves, blocks in float64) -- so the library is compared with it
bit for bit.  With f = np.float64 the same expressions are the closed form of the mathematics; grad_grid64() and tv64() state
the two sums without any order (one float64 scatter).
"""
import numpy as np

VERTEX_FLOATS = 12
MIN_GRID, MAX_XY, MAX_L = 2, 64, 8
THREADS, GATHER_THREADS, TV_THREADS = 256, 256, 1024
TARGET_BLOCKS = 1024
MAX_PIXELS = 2 ** 31 - 2048
LUMINANCE = (0.299, 0.587, 0.114)
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64)


def identity_grid(Gx, Gy, L, dtype=np.float32):
    return np.tile(IDENTITY.astype(dtype), (Gy, Gx, L, 1))


def dims(grid):
    Gy, Gx, L, k = grid.shape
    assert k == VERTEX_FLOATS
    return Gx, Gy, L


def scale(G, n, f=np.float32):
    return f(G - 1) / f(n - 1) if n > 1 else f(0)


def cell(n, G, f=np.float32):
    """-> (i0 (n,) int, t (n,) f): the lower vertex and the fraction of the coordinates 0..n-1 along an image-plane axis"""
    g = np.arange(n).astype(f) * scale(G, n, f)
    i0 = np.minimum(g.astype(np.int64), G - 2)
    return i0, g - i0.astype(f)


def luminance(x, f=np.float32):
    c = [f(v) for v in LUMINANCE]
    with np.errstate(all="ignore"):
        return (c[0] * x[0] + c[1] * x[1]) + c[2] * x[2]


def level(x, L, f=np.float32):
    """-> (i0, t, inside) of the luminance guide of the (3,H,W) image x (already of format f)"""
    lum = luminance(x, f)
    with np.errstate(all="ignore"):
        lc = np.where(lum > 0, np.where(lum < 1, lum, f(1)), f(0)).astype(f)
        inside = (lum > 0) & (lum < 1)
    g = lc * f(L - 1)
    i0 = np.minimum(g.astype(np.int64), L - 2)
    return i0, g - i0.astype(f), inside


def _lerp(a, b, t):
    return a + t * (b - a)


def transform(image, grid, f=np.float32):
    """-> (M (12,H,W), dM (12,H,W), inside (H,W)): x, then y, then z, as the header has it"""
    x, v = np.asarray(image).astype(f), np.asarray(grid).astype(f)
    _, H, W = x.shape
    Gx, Gy, L = dims(v)
    ix0, tx = cell(W, Gx, f)
    iy0, ty = cell(H, Gy, f)
    iz0, tz, inside = level(x, L, f)
    IY, IX, TX, TY = iy0[:, None], ix0[None, :], tx[None, :, None], ty[:, None, None]
    with np.errstate(all="ignore"):
        P = []
        for l in (iz0, iz0 + 1):
            top = _lerp(v[IY, IX, l], v[IY, IX + 1, l], TX)
            bottom = _lerp(v[IY + 1, IX, l], v[IY + 1, IX + 1, l], TX)
            P.append(_lerp(top, bottom, TY))
        dM = P[1] - P[0]
        M = P[0] + tz[:, :, None] * dM
    return np.moveaxis(M, 2, 0).astype(f), np.moveaxis(dM, 2, 0).astype(f), inside


def slice(image, grid, f=np.float32):
    """c_i = ((M_i0 x_0 + M_i1 x_1) + M_i2 x_2) + M_i3"""
    x = np.asarray(image).astype(f)
    M, _, _ = transform(x, grid, f)
    with np.errstate(all="ignore"):
        return np.stack([((M[4 * i] * x[0] + M[4 * i + 1] * x[1]) + M[4 * i + 2] * x[2]) + M[4 * i + 3] for i in range(3)]).astype(f)


def selected(grad_corrected):
    g = np.asarray(grad_corrected)
    return ~((g[0] == 0) & (g[1] == 0) & (g[2] == 0))


def grad_image(image, grad_corrected, grid, f=np.float32):
    """a_j + ((L-1) c_j) S where the luminance is strictly inside (0,1), a_j where it is clamped, +0 where not selected"""
    x, g = np.asarray(image).astype(f), np.asarray(grad_corrected).astype(f)
    M, dM, inside = transform(x, grid, f)
    L = dims(grid)[2]
    sel = selected(grad_corrected)
    with np.errstate(all="ignore"):
        D = [((dM[4 * i] * x[0] + dM[4 * i + 1] * x[1]) + dM[4 * i + 2] * x[2]) + dM[4 * i + 3] for i in range(3)]
        S = (g[0] * D[0] + g[1] * D[1]) + g[2] * D[2]
        out = []
        for j in range(3):
            a = (M[j] * g[0] + M[4 + j] * g[1]) + M[8 + j] * g[2]
            out.append(np.where(inside, a + (f(L - 1) * f(LUMINANCE[j])) * S, a))
    out = np.stack(out).astype(f)
    out[:, ~sel] = 0.0
    return out


def split(Gx, Gy):
    return max(1, TARGET_BLOCKS // (Gx * Gy))


def cells(n, G):
    """first[c], c = 0..G-1: the first coordinate whose cell is >= c (first[G-1] = n)"""
    i0, _ = cell(n, G)
    first = np.searchsorted(i0, np.arange(G), side="left")
    first[0] = 0
    assert first[G - 1] == n
    return first


def _butterfly(a):
    """a: (waves, 64, ...) -> the same with every lane holding its wave's sum, added as v += v[lane ^ o], o = 32 .. 1"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[:, lanes ^ o]
    return a


def _block_sum(terms, threads):
    """terms (n, K): thread t adds the rows t, t + threads, ... in order from +0, butterfly, waves in order -> (K,)"""
    n, K = terms.shape
    iters = max(1, -(-n // threads))
    padded = np.zeros((iters * threads, K), dtype=terms.dtype)
    padded[:n] = terms
    padded = padded.reshape(iters, threads, K)
    with np.errstate(all="ignore"):
        acc = np.zeros((threads, K), dtype=terms.dtype)
        for it in range(iters):
            acc = acc + padded[it]
        acc = _butterfly(acc.reshape(threads // 64, 64, K))
        out = acc[0, 0]
        for w in range(1, threads // 64):
            out = out + acc[w, 0]
    return out


def _pixel_terms(image, grad_corrected, L):
    """what every selected pixel adds: -> dict of per-pixel arrays in f32 (the header's products, before the weights)"""
    x, g = np.asarray(image), np.asarray(grad_corrected)
    assert x.dtype == np.float32 and g.dtype == np.float32
    iz0, tz, _ = level(x, L)
    return dict(x=x, g=g, iz0=iz0, tz=tz, sel=selected(g))


def grad_grid(image, grad_corrected, Gx, Gy, L):
    """The grid's gradient in the header's summation order, f32 (the float64 step where blocks meet included): (Gy,Gx,L,12)"""
    p = _pixel_terms(image, grad_corrected, L)
    _, H, W = p["x"].shape
    ix0, tx = cell(W, Gx)
    iy0, ty = cell(H, Gy)
    xs, ys = cells(W, Gx), cells(H, Gy)
    S = split(Gx, Gy)
    one = np.float32(1)
    out = np.zeros((Gy, Gx, L, 12), dtype=np.float32)
    levels = np.arange(L)[None, :, None]
    for iy in range(Gy):
        y0, y1 = ys[max(iy - 1, 0)], ys[min(iy + 1, Gy - 1)]
        R = -(-(y1 - y0) // S)
        wy_all = np.where(iy0 == iy, one - ty, ty).astype(np.float32)
        for ix in range(Gx):
            xa, xb = xs[max(ix - 1, 0)], xs[min(ix + 1, Gx - 1)]
            wx = np.where(ix0[xa:xb] == ix, one - tx[xa:xb], tx[xa:xb]).astype(np.float32)
            blocks = np.zeros((S, L * 12), dtype=np.float32)
            for s in range(S):
                ya = y0 + s * R
                yb = min(ya + R, y1)
                if yb <= ya or xb <= xa:
                    continue
                g = p["g"][:, ya:yb, xa:xb].reshape(3, -1)
                u = p["x"][:, ya:yb, xa:xb].reshape(3, -1)
                sel, iz0, tz = (p[k][ya:yb, xa:xb].reshape(-1) for k in ("sel", "iz0", "tz"))
                with np.errstate(all="ignore"):
                    wxy = (wx[None, :] * wy_all[ya:yb, None]).reshape(-1)
                    w0, w1 = wxy * (one - tz), wxy * tz
                    t0, t1 = np.empty((g.shape[1], 12), dtype=np.float32), np.empty((g.shape[1], 12), dtype=np.float32)
                    for i in range(3):
                        a0, a1 = w0 * g[i], w1 * g[i]
                        for j in range(3):
                            t0[:, 4 * i + j], t1[:, 4 * i + j] = a0 * u[j], a1 * u[j]
                        t0[:, 4 * i + 3], t1[:, 4 * i + 3] = a0, a1
                lo = (levels == iz0[:, None, None]) & sel[:, None, None]
                hi = (levels == iz0[:, None, None] + 1) & sel[:, None, None]
                terms = np.where(lo, t0[:, None, :], np.where(hi, t1[:, None, :], np.float32(0))).astype(np.float32)
                blocks[s] = _block_sum(terms.reshape(-1, L * 12), GATHER_THREADS)
            if S == 1:
                total = blocks[0]
            else:
                total = np.zeros(L * 12, dtype=np.float64)
                with np.errstate(all="ignore"):
                    for s in range(S):
                        total = total + blocks[s].astype(np.float64)
                    total = total.astype(np.float32)
            out[iy, ix] = total.reshape(L, 12)
    return out


def grad_grid64(image, grad_corrected, Gx, Gy, L, f=np.float64, reach=False):
    """-> (value, magnitude), both (Gy,Gx,L,12) float64: the sum over the selected pixels of wx wy wz g_i u_j as one scatter, and
    the same sum of the terms' absolute values.  reach=True: a third array, the sum of |g_i u_j| over the pixels that reach
    the vertex, without the weights -- what an error of the coordinates themselves is stated in."""
    x, g = np.asarray(image).astype(f), np.asarray(grad_corrected).astype(f)
    _, H, W = x.shape
    ix0, tx = cell(W, Gx, f)
    iy0, ty = cell(H, Gy, f)
    iz0, tz, _ = level(x, L, f)
    sel = selected(grad_corrected)
    u = np.concatenate([x, np.ones((1, H, W), dtype=f)])
    gu = (g[:, None] * u[None, :]).reshape(12, H, W)
    gu = np.where(sel[None], gu, 0.0)
    value, magnitude, reached = (np.zeros((Gy, Gx, L, 12), dtype=f) for _ in range(3))
    IY, IX = np.broadcast_to(iy0[:, None], (H, W)), np.broadcast_to(ix0[None, :], (H, W))
    TY, TX = np.broadcast_to(ty[:, None], (H, W)), np.broadcast_to(tx[None, :], (H, W))
    for dy in (0, 1):
        for dx in (0, 1):
            for dz in (0, 1):
                w = (TY if dy else 1 - TY) * (TX if dx else 1 - TX) * (tz if dz else 1 - tz)
                w = np.where(sel, w, 0.0)
                terms = np.moveaxis(w[None] * gu, 0, 2)
                np.add.at(value, (IY + dy, IX + dx, iz0 + dz), terms)
                np.add.at(magnitude, (IY + dy, IX + dx, iz0 + dz), np.abs(terms))
                if reach:
                    np.add.at(reached, (IY + dy, IX + dx, iz0 + dz), np.abs(np.moveaxis(gu, 0, 2)))
    return (value, magnitude, reached) if reach else (value, magnitude)


def _tv_layout(Gx, Gy, L):
    n = 12 * Gx * Gy * L
    e = np.arange(n)
    vtx = e // 12
    r, l = vtx // L, vtx % L
    iy, ix = r // Gx, r % Gx
    strides = dict(x=12 * L, y=12 * L * Gx, z=12)
    has_next = dict(x=ix + 1 < Gx, y=iy + 1 < Gy, z=l + 1 < L)
    has_prev = dict(x=ix > 0, y=iy > 0, z=l > 0)
    counts = dict(x=12 * Gy * (Gx - 1) * L, y=12 * (Gy - 1) * Gx * L, z=12 * Gy * Gx * (L - 1))
    return n, e, strides, has_next, has_prev, counts


def _tv_diffs(grid):
    """next[a], prev[a]: v(next) - v and v - v(previous) in f32 along the axes, 0 where there is none; flat over the values"""
    v = np.asarray(grid)
    assert v.dtype == np.float32
    Gx, Gy, L = dims(v)
    n, e, strides, has_next, has_prev, counts = _tv_layout(Gx, Gy, L)
    flat = v.reshape(-1)
    nxt, prv = {}, {}
    with np.errstate(all="ignore"):
        for a in "xyz":
            nxt[a] = np.where(has_next[a], flat[np.minimum(e + strides[a], n - 1)] - flat, np.float32(0)).astype(np.float32)
            prv[a] = np.where(has_prev[a], flat - flat[np.maximum(e - strides[a], 0)], np.float32(0)).astype(np.float32)
    return nxt, prv, counts


def tv(grid):
    """The total variation in the header's order: float64 sums per thread, butterfly, waves -> one f32"""
    nxt, _, counts = _tv_diffs(grid)
    sq = np.stack([nxt[a].astype(np.float64) * nxt[a].astype(np.float64) for a in "xyz"], axis=1)
    T = _block_sum(sq, TV_THREADS)
    return np.float32((T[0] / float(counts["x"]) + T[1] / float(counts["y"])) + T[2] / float(counts["z"]))


def tv_add_grad(grid, weight, grad):
    """-> grad + weight * ((r_x q_x + r_y q_y) + r_z q_z) in f32, r_a = 2 / count_a, q_a = (v - previous) - (next - v)"""
    nxt, prv, counts = _tv_diffs(grid)
    r = {a: np.float32(2.0) / np.float32(counts[a]) for a in "xyz"}
    q = {a: prv[a] - nxt[a] for a in "xyz"}
    with np.errstate(all="ignore"):
        t = (r["x"] * q["x"] + r["y"] * q["y"]) + r["z"] * q["z"]
        out = np.asarray(grad, dtype=np.float32).reshape(-1) + np.float32(weight) * t
    return out.astype(np.float32).reshape(np.asarray(grid).shape)


def tv64(grid):
    """-> (tv, d tv / d grid) in float64, without any order"""
    v = np.asarray(grid).astype(np.float64)
    value, grad = 0.0, np.zeros_like(v)
    for axis in (1, 0, 2):
        d = np.diff(v, axis=axis)
        value += float((d * d).sum()) / d.size
        pad = [(0, 0)] * 4
        pad[axis] = (1, 0)
        before = np.pad(d, pad)
        pad[axis] = (0, 1)
        after = np.pad(d, pad)
        grad += 2.0 * (before - after) / d.size
    return value, grad


def torch_slice(image, grid):
    """The same mathematics in torch operations, through grid_sample (bilinear, align_corners, border) on the (1,12,L,Gy,Gx)
    volume: image (3,H,W) and grid (Gy,Gx,L,12) tensors of one dtype and device -> (3,H,W), differentiable in both.  In float64
    on the CPU it is what the float64 form is checked against; in float32 on the GPU it shows what f32 costs these formulas."""
    import torch
    import torch.nn.functional as F
    _, H, W = image.shape
    kw = dict(dtype=image.dtype, device=image.device)
    xn = torch.linspace(-1, 1, W, **kw) if W > 1 else torch.full((1,), -1.0, **kw)
    yn = torch.linspace(-1, 1, H, **kw) if H > 1 else torch.full((1,), -1.0, **kw)
    lum = LUMINANCE[0] * image[0] + LUMINANCE[1] * image[1] + LUMINANCE[2] * image[2]
    zn = 2.0 * lum.clamp(0.0, 1.0) - 1.0
    coords = torch.stack([xn[None, :].expand(H, W), yn[:, None].expand(H, W), zn], dim=-1)[None, None]      # (1,1,H,W,3)
    volume = grid.permute(3, 2, 0, 1)[None]                                                                   # (1,12,L,Gy,Gx)
    M = F.grid_sample(volume, coords, mode="bilinear", align_corners=True, padding_mode="border")[0, :, 0]   # (12,H,W)
    M = M.reshape(3, 4, H, W)
    return (M[:, :3] * image[None]).sum(1) + M[:, 3]
