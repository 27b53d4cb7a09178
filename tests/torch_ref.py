"""Float64 torch.autograd restatement of the rasteriser for TINY scenes (tests only): image, depth and accumulated alpha,
and their gradients with respect to the points or to the pose.

Purpose: pin the oracle's hand-written backward (oracle/gs_oracle.c, restating GaussianPointCloudRasterisation.py:488-772)
and the HIP backward (pose, depth and alpha gradients included) against automatic differentiation, because the reference ships
no test for loop-1 accumulation, the SH gradient, the grad factors or loop 2 as a whole (SURVEY 8c "parity unpinned" list).

The integer structure (visible ids, sorted per-tile lists, tile ranges) is taken from the oracle; every floating-point quantity
is recomputed here in float64 with autograd.  Per pixel: image = sum(w colour), depth D = sum(w d) / clamp(sum(w), 1e-6) with
w = alpha T the blend weight and d the splat's camera-space z (NOT detached: the depth gradient reaches the position through
p_cam = W x + t), accumulated alpha A = 1 - T_final.

The reference's analytic backward deliberately differs from the true derivative in a few places; the same stops are placed here.
In both modes (they live in the upstream loop 1 hands over):
  * rescale is a constant                                                          (UTIL:347 "known caveat")
  * no gradient through the 0.99 clamp test: the clamped value is used in the formulas but d alpha / d (g * opacity) = 1, and
    the use / saturation masks, sort, cull and radius are discrete                 (RAST:634-662)
  * q of a splat is the already-normalised quaternion                              (RAST:264-266)
  * the count output carries no gradient                                           (RAST:1026)
With respect to the points (wrt="points": leaves point_cloud and features) only:
  * Sigma' does not feed xyz: J is built from a detached p_cam                     (RAST:757-761, GP3D:237-331)
  * the SH view direction does not feed xyz                                        (RAST:749-756)
With respect to the pose (wrt="pose") J(p) and the view direction d = x - o are live -- the pose gradient is the derivative of
the forward as it is computed -- and the pose is expanded to per-point leaves (q[obj[ids]] (M,4), t[obj[ids]] (M,3)), so that
autograd yields each point's contribution: their index_add by object is the gradient, the index_add of their absolute values
the summed magnitude of the per-element bar (parity_util.elem_margins style).

Every stop is recorded (aux["stops"]) and can be replayed (`stops=`): the replayed function's plain derivative is the gradient
with stops, which is what the finite differences of test_pose_ref_host.py and test_depth_alpha_ref_host.py check.
"""
import numpy as np
import torch

ALPHA_EPS = 1.0 / 255.0
F64 = torch.float64


def quat_to_R(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    R = torch.stack([
        torch.stack([1 - 2 * (yy + zz), 2 * (xy - wz), 2 * (xz + wy)], -1),
        torch.stack([2 * (xy + wz), 1 - 2 * (xx + zz), 2 * (yz - wx)], -1),
        torch.stack([2 * (xz - wy), 2 * (yz + wx), 1 - 2 * (xx + yy)], -1)], -2)
    return R


def sh16(d):
    d = d / d.norm(dim=-1, keepdim=True)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return torch.stack([
        torch.full_like(x, 0.28209479177387814),
        -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
        1.0925484305920792 * x * y, -1.0925484305920792 * y * z,
        0.94617469575755997 * z * z - 0.31539156525251999,
        -1.0925484305920792 * x * z, 0.54627421529603959 * x * x - 0.54627421529603959 * y * y,
        0.59004358992664352 * y * (-3.0 * x * x + y * y), 2.8906114426405538 * x * y * z,
        0.45704579946446572 * y * (1.0 - 5.0 * z * z), 0.3731763325901154 * z * (5.0 * z * z - 3.0),
        0.45704579946446572 * x * (1.0 - 5.0 * z * z), 1.4453057213202769 * z * (x * x - y * y),
        0.59004358992664352 * x * (-x * x + 3.0 * y * y)], -1)


def blend(uv, conic_a, conic_b, conic_c, rescale, opacity, color, z, H, W, fwd, decisions=None):
    """-> image (H,W,3), depth (H,W), alpha (H,W), decisions: per blend step (use mask, saturation mask, clamp offset), the
    discrete part of the blend.  decisions=None: made here; otherwise those of an earlier call, taken instead of made."""
    image = torch.zeros(H, W, 3, dtype=F64)
    depth = torch.zeros(H, W, dtype=F64)
    alpha = torch.zeros(H, W, dtype=F64)
    tiles_x = (W + 15) // 16                       # = W // 16 at the reference's sizes; partial edge tiles are an extension
    lst = fwd.point_offset_with_sort_key
    yy, xx = torch.meshgrid(torch.arange(16, dtype=F64), torch.arange(16, dtype=F64), indexing="ij")
    replay = decisions is not None
    taken, made = iter(decisions or ()), []
    for tile in range(tiles_x * ((H + 15) // 16)):
        s, e = int(fwd.tile_points_start[tile]), int(fwd.tile_points_end[tile])
        if e <= s:
            continue
        tu, tv = tile % tiles_x, tile // tiles_x
        px = (xx + tu * 16 + 0.5).reshape(-1)
        py = (yy + tv * 16 + 0.5).reshape(-1)
        T = torch.ones(256, dtype=F64)
        C = torch.zeros(256, 3, dtype=F64)
        S = torch.zeros(256, dtype=F64)
        Wsum = torch.zeros(256, dtype=F64)
        alive = torch.ones(256, dtype=torch.bool)
        for idx in range(s, e):
            p = int(lst[idx])
            dx, dy = px - uv[p, 0], py - uv[p, 1]
            g = torch.exp(-0.5 * (dx * dx * conic_a[p] + dy * dy * conic_c[p]) - dx * dy * conic_b[p]) * rescale[p]
            a = g * opacity[p]
            if replay:
                use0, sat, off = next(taken)
            else:
                use0 = alive & (a.detach() >= ALPHA_EPS)
                off = (torch.clamp(a, max=0.99) - a).detach()
            a_c = a + off                                         # clamp value, straight-through gradient
            nT = T * (1 - a_c)
            if not replay:
                sat = use0 & (nT.detach() < 1e-4)
                made.append((use0, sat, off))
            alive = alive & ~sat
            use = use0 & ~sat
            w = torch.where(use, a_c * T, torch.zeros_like(T))
            C = C + w[:, None] * color[p][None, :]
            S = S + w * z[p]
            Wsum = Wsum + w
            T = torch.where(use, nT, T)
        D = S / torch.clamp(Wsum, min=1e-6)
        A = 1 - T
        hh, ww = min(16, H - tv * 16), min(16, W - tu * 16)
        rows, cols = slice(tv * 16, tv * 16 + hh), slice(tu * 16, tu * 16 + ww)
        image[rows, cols, :] = C.reshape(16, 16, 3)[:hh, :ww]
        depth[rows, cols] = D.reshape(16, 16)[:hh, :ww]
        alpha[rows, cols] = A.reshape(16, 16)[:hh, :ww]
    return image, depth, alpha, decisions if replay else made


def per_point(xyz, f, q_pts, t_pts, Kmat, live, stops):
    """Everything the blend needs of each visible point (M rows): -> uv, (conic_a, conic_b, conic_c), opacity, colour, z,
    the stops {"pc", "dir", "rescale"} and Sigma' = J W Sigma W^T J^T (M,2,2), the covariance before + 0.3 I.  live: J(p) and the SH view direction are differentiated (the pose mode); otherwise
    they are constants, recorded in the stops.  stops: None (record), or those of an earlier call (replay)."""
    # pose: inverse of (q_pc, t_pc), UTIL:426-432 (the conjugate is NOT renormalised for W, the rotation the kernels use)
    q_cp = torch.cat([-q_pts[:, :3], q_pts[:, 3:]], -1)
    R_unit = quat_to_R(q_cp / q_cp.norm(dim=-1, keepdim=True))
    t_cp = -(R_unit @ t_pts[..., None])[..., 0]
    Wm = quat_to_R(q_cp)
    pcam = (Wm @ xyz[..., None])[..., 0] + t_cp
    uv = ((Kmat @ pcam[..., None])[..., 0])[:, :2] / pcam[:, 2:3]
    rec = {} if stops is None else dict(stops)
    # covariance
    p = pcam if live else rec.setdefault("pc", pcam.detach())
    fx, fy = Kmat[0, 0], Kmat[1, 1]
    zero = torch.zeros_like(p[:, 0])
    J = torch.stack([torch.stack([fx / p[:, 2], zero, -fx * p[:, 0] / p[:, 2] ** 2], -1),
                     torch.stack([zero, fy / p[:, 2], -fy * p[:, 1] / p[:, 2] ** 2], -1)], -2)
    R = quat_to_R(f[:, 0:4])
    S = torch.diag_embed(torch.exp(f[:, 4:7]))
    Sigma = R @ S @ S.transpose(-1, -2) @ R.transpose(-1, -2)
    U = J @ Wm
    cov = U @ Sigma @ U.transpose(-1, -2)
    cov_b = cov + 0.3 * torch.eye(2, dtype=F64)
    det_pre = cov[:, 0, 0] * cov[:, 1, 1] - cov[:, 0, 1] * cov[:, 1, 0]
    det = cov_b[:, 0, 0] * cov_b[:, 1, 1] - cov_b[:, 0, 1] * cov_b[:, 1, 0]
    if stops is None:
        rec["rescale"] = torch.sqrt(torch.clamp(det_pre / det, min=0.0)).detach()
    conics = (cov_b[:, 1, 1] / det, -cov_b[:, 0, 1] / det, cov_b[:, 0, 0] / det)
    # colour: ray origin = camera centre in the point-cloud frame as the forward computes it, o = -W^T t_cp
    origin = -(Wm.transpose(-1, -2) @ t_cp[..., None])[..., 0]
    Y = sh16(xyz - origin if live else rec.setdefault("dir", (xyz - origin).detach()))
    color = torch.sigmoid(torch.stack([(f[:, 8:24] * Y).sum(-1), (f[:, 24:40] * Y).sum(-1), (f[:, 40:56] * Y).sum(-1)], -1))
    return uv, conics, torch.sigmoid(f[:, 7]), color, pcam[:, 2], rec, cov


def _t(x):
    return x if x is None or torch.is_tensor(x) else torch.as_tensor(np.asarray(x, np.float64))


def render(point_cloud, features, q_pc, t_pc, Kmat, H, W, fwd, object_id=None, stops=None, wrt="points"):
    """-> image (H,W,3), depth (H,W), alpha (H,W), aux.  `fwd` is an oracle.Forward (ints only are used).  point_cloud (N,3),
    features (N,56) (features[:, :4] normalised: the oracle's features_after), q_pc (K,4), t_pc (K,3).
    wrt="points": point_cloud and features are the float64 leaves (tensors); aux["uv"] (M,2) keeps its gradient.
    wrt="pose": aux["q_pts"] (M,4), aux["t_pts"] (M,3) are the per-point pose leaves, aux["obj"] (M) their object ids.
    aux["stops"]: the values the gradient stops froze; passed as `stops` to a later call they are replayed, not recomputed."""
    ids = torch.as_tensor(fwd.point_id_in_camera_list.astype(np.int64))
    point_cloud, features = _t(point_cloud), _t(features)
    obj = torch.zeros(point_cloud.shape[0], dtype=torch.long) if object_id is None else torch.as_tensor(np.asarray(object_id)).long()
    oid = obj[ids]
    pose = wrt == "pose"
    q_pts = _t(np.asarray(q_pc, np.float64).reshape(-1, 4))[oid].clone().requires_grad_(pose)
    t_pts = _t(np.asarray(t_pc, np.float64).reshape(-1, 3))[oid].clone().requires_grad_(pose)
    uv, conics, opacity, color, z, rec, _ = per_point(point_cloud[ids], features[ids], q_pts, t_pts, _t(Kmat), pose, stops)
    if uv.requires_grad:
        uv.retain_grad()
    image, depth, alpha, rec["blend"] = blend(uv, *conics, rec["rescale"], opacity, color, z, H, W, fwd, rec.get("blend"))
    return image, depth, alpha, {"uv": uv, "q_pts": q_pts, "t_pts": t_pts, "obj": oid, "stops": rec}


def _backward(scene, q, t, fwd, feat_after, upstreams, pc=None, wrt="points"):
    """backward of sum(g_image image) + sum(g_depth depth) + sum(g_alpha alpha) over the upstreams that are not None -> aux"""
    *outs, aux = render(scene.point_cloud if pc is None else pc, feat_after, q, t, scene.camera_intrinsics, scene.height,
                        scene.width, fwd, scene.point_object_id, wrt=wrt)
    sum((out * _t(g)).sum() for out, g in zip(outs, upstreams) if g is not None).backward()
    return aux


def point_gradients(scene, q, t, fwd, feat_after, g_image=None, g_depth=None, g_alpha=None):
    """(grad_pointcloud (N,3), grad_features (N,56)) of the loss of _backward, float64 numpy; all grad factors 1, every SH band."""
    pc = torch.tensor(np.asarray(scene.point_cloud, np.float64), requires_grad=True)
    ft = torch.tensor(np.asarray(feat_after, np.float64), requires_grad=True)
    _backward(scene, q, t, fwd, ft, (g_image, g_depth, g_alpha), pc)
    grad = lambda x: x.grad.numpy() if x.grad is not None else np.zeros(x.shape)
    return grad(pc), grad(ft)


def _by_object(K, oid, leaves):
    """per-point leaf gradients (q (M,4), t (M,3)) -> (grad_q, grad_t, summed_q, summed_t): their index_add by object and that of
    their absolute values"""
    res = []
    for leaf, w in zip(leaves, (4, 3)):
        g = leaf.grad if leaf.grad is not None else torch.zeros(oid.shape[0], w, dtype=F64)
        res.append(torch.zeros(K, w, dtype=F64).index_add_(0, oid, g).numpy())
        res.append(torch.zeros(K, w, dtype=F64).index_add_(0, oid, g.abs()).numpy())
    return res[0], res[2], res[1], res[3]


def pose_gradients(scene, q, t, fwd, feat_after, g_image=None, g_depth=None, g_alpha=None):
    """(grad_q (K,4), grad_t (K,3), summed_q (K,4), summed_t (K,3)) of the same loss, float64 numpy"""
    aux = _backward(scene, q, t, fwd, feat_after, (g_image, g_depth, g_alpha), wrt="pose")
    return _by_object(np.asarray(q).reshape(-1, 4).shape[0], aux["obj"], (aux["q_pts"], aux["t_pts"]))


def pose_gradients_from_sums(scene, q, t, ids, feat_after, sums):
    """The same four arrays from loop 1's per-splat sums instead of a blend: the float64 restatement of what k_pose.hip computes
    from them, vectorised over the M in-camera points `ids` (no pixel loop, so any M).  sums (M,12) in the reference's scaling
    (oracle.backward_sums): columns 0-1 dL/duv, 2-4 dL/dSigma' xx, xy, yy, 5-7 dL/dcolour, 11 dL/d depth (zero without a depth
    upstream); they are constants of the surrogate
        sum_m [ s0 u + s1 v + s2 Sigma'00 + 2 s3 Sigma'01 + s4 Sigma'11 + s5..7 . colour + s11 p_z ]
    whose derivative with respect to the per-point pose leaves is each point's contribution.  A point whose sums are all zero
    contributes exact zeros."""
    ids = torch.as_tensor(np.asarray(ids).astype(np.int64))
    s = _t(np.asarray(sums, np.float64).reshape(-1, 12))
    assert s.shape[0] == ids.shape[0]
    oid = torch.as_tensor(np.asarray(scene.point_object_id)).long()[ids]
    q = np.asarray(q, np.float64).reshape(-1, 4)
    q_pts = _t(q)[oid].clone().requires_grad_(True)
    t_pts = _t(np.asarray(t, np.float64).reshape(-1, 3))[oid].clone().requires_grad_(True)
    uv, _, _, color, z, _, cov = per_point(_t(scene.point_cloud)[ids], _t(feat_after)[ids], q_pts, t_pts,
                                           _t(scene.camera_intrinsics), True, None)
    surrogate = (s[:, 0:2] * uv).sum() + (s[:, 2] * cov[:, 0, 0] + 2.0 * s[:, 3] * cov[:, 0, 1] + s[:, 4] * cov[:, 1, 1]).sum() \
        + (s[:, 5:8] * color).sum() + (s[:, 11] * z).sum()
    surrogate.backward()
    return _by_object(q.shape[0], oid, (q_pts, t_pts))
