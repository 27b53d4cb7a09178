"""Float64 reference of the feature-channel operator (render_channels): a numpy restatement over the CPU oracle's frame.

Per tile it takes the oracle's sorted list and tile range, the per-point uv, conic, rescale and opacity (which the parity tests
prove bit-identical to the GPU's) and pixel_offset_of_last_effective_point, forms alpha in float64 for all 256 pixels x entries,
masks by alpha >= 1/255, by index < last and by inside-image, clamps at 0.99, takes T as the exclusive cumulative product and
w = alpha T.  Both directions are linear in their input, so neither needs autograd:

    forward   out[pixel]        = w @ values[ids]
    backward  grad_values[ids] += w^T @ grad_out[pixel]

Beside them come the magnitudes the per-element bars are relative to: sum w |v| per output element, S = sum w |G| per
gradient element, and the contributor count of every pixel (a pixel where it differs from the forward's own
pixel_valid_point_count is MARGINAL: the reference decided alpha >= 1/255 in float64, the forward in f32).
Nothing here touches the GPU."""
import numpy as np

ALPHA_EPS = 1.0 / 255.0
ALPHA_MAX = 0.99


def tile_weights(f):
    """Yields, per non-empty tile of the oracle frame f, (o, p, w): flat pixel indices (P,), in-camera point indices of the
    list entries (n,), weights (P, n) float64 (zero where the pixel takes nothing from the entry)."""
    H, W = f.H, f.W
    tiles_x = (W + 15) // 16
    uv = f.point_uv.astype(np.float64)
    conic = f.point_uv_conic_and_rescale.astype(np.float64)
    opacity = f.point_alpha_after_activation.astype(np.float64)
    last_img = f.pixel_offset_of_last_effective_point
    tu, tv = np.meshgrid(np.arange(16), np.arange(16))
    for tile in range(len(f.tile_points_start)):
        start, end = int(f.tile_points_start[tile]), int(f.tile_points_end[tile])
        if end <= start:
            continue
        pu = (tile % tiles_x) * 16 + tu.ravel()
        pv = (tile // tiles_x) * 16 + tv.ravel()
        inside = (pu < W) & (pv < H)
        pu, pv = pu[inside], pv[inside]
        o = pv * W + pu
        last = last_img.ravel()[o].astype(np.int64)
        stop = min(end, int(last.max()))
        if stop <= start:
            continue
        p = f.point_offset_with_sort_key[start:stop].astype(np.int64)
        dx = (pu + 0.5)[:, None] - uv[p, 0][None, :]
        dy = (pv + 0.5)[:, None] - uv[p, 1][None, :]
        e = -0.5 * (dx * dx * conic[p, 0] + dy * dy * conic[p, 2]) - dx * dy * conic[p, 1]
        alpha = np.exp(e) * conic[p, 3] * opacity[p]
        use = (alpha >= ALPHA_EPS) & ((start + np.arange(stop - start))[None, :] < last[:, None])
        alpha = np.where(use, np.minimum(alpha, ALPHA_MAX), 0.0)
        T = np.cumprod(1.0 - alpha, axis=1)
        T = np.concatenate([np.ones((T.shape[0], 1)), T[:, :-1]], axis=1)          # exclusive
        yield o, p, alpha * T


def run(f, values=None, grad_out=None):
    """values (N,C) and/or grad_out (H,W,C) -> dict with
         out (H,W,C), out_abs (H,W,C) = sum w |v|                      when values is given
         grad (N,C), grad_abs (N,C) = S = sum w |G|                    when grad_out is given
         count (H,W) contributors per pixel, weight (H,W) = sum w      always"""
    H, W = f.H, f.W
    ids = f.point_id_in_camera_list.astype(np.int64)
    r = {"count": np.zeros(H * W, np.int64), "weight": np.zeros(H * W)}
    if values is not None:
        V = np.asarray(values, np.float64)
        r["out"] = np.zeros((H * W, V.shape[1]))
        r["out_abs"] = np.zeros((H * W, V.shape[1]))
    if grad_out is not None:
        G = np.asarray(grad_out, np.float64).reshape(H * W, -1)
        gm = np.zeros((len(ids), G.shape[1]))          # per in-camera point
        gm_abs = np.zeros_like(gm)
    for o, p, w in tile_weights(f):
        r["count"][o] = (w > 0).sum(axis=1)
        r["weight"][o] = w.sum(axis=1)
        if values is not None:
            rows = V[ids[p]]
            r["out"][o] = w @ rows
            r["out_abs"][o] = w @ np.abs(rows)
        if grad_out is not None:
            # a point appears once per tile list: plain indexed addition within a tile, tiles one after the other
            gm[p] += w.T @ G[o]
            gm_abs[p] += w.T @ np.abs(G[o])
    r["count"] = r["count"].reshape(H, W)
    r["weight"] = r["weight"].reshape(H, W)
    if values is not None:
        r["out"] = r["out"].reshape(H, W, -1)
        r["out_abs"] = r["out_abs"].reshape(H, W, -1)
    if grad_out is not None:
        N = f.N
        r["grad"] = np.zeros((N, G.shape[1]))
        r["grad_abs"] = np.zeros((N, G.shape[1]))
        r["grad"][ids] = gm
        r["grad_abs"][ids] = gm_abs
    return r


def marginal_pixels(ref_count, forward_count):
    """(H,W) bool: pixels whose float64 contributor count differs from the forward's own; at most 1e-4 of a scene's pixels
    may be (asserted here)."""
    m = np.asarray(ref_count) != np.asarray(forward_count)
    assert m.mean() <= 1e-4, f"{int(m.sum())} of {m.size} pixels are marginal"
    return m
