"""Float64 torch.autograd reference of the DEPTH and ACCUMULATED-ALPHA outputs and their gradients (tests only).

torch_ref.render's blend on the oracle's integer structure (visible ids, sorted per-tile lists, tile ranges), with two more
outputs per pixel:
  * D = sum(w d) / clamp(sum(w), 1e-6), w = alpha T the blend weight and d the splat's camera-space z, NOT detached (the
    depth gradient reaches the position through p_cam = W x + t);
  * A = 1 - T_final.
Same stops as torch_ref: rescale is a constant, the 0.99 clamp is straight-through, J and the SH view direction are constants
with respect to xyz, q is the already-normalised quaternion, the count carries no gradient.  For pose gradients, `render_pose`
rebuilds the per-point quantities as tests/pose_ref.py does (live J(p) and view direction, per-point pose leaves).

Every stop can be recorded (`stops` out) and replayed (`stops` in): the replayed function's plain derivative is the gradient
with stops, which is what the finite differences of test_depth_alpha_ref_host.py check.
"""
import numpy as np
import torch

from torch_ref import ALPHA_EPS, F64, quat_to_R, sh16


def blend(uv, conic_a, conic_b, conic_c, rescale, opacity, color, z, H, W, fwd, steps=None):
    """-> image (H,W,3), depth (H,W), alpha (H,W).  steps: None (compute the discrete decisions), or a list to append
    (use, sat, clamp offset) of every step to (record), or an iterator to take them from (replay)."""
    image = torch.zeros(H, W, 3, dtype=F64)
    depth = torch.zeros(H, W, dtype=F64)
    alpha = torch.zeros(H, W, dtype=F64)
    tiles_x = (W + 15) // 16
    lst = fwd.point_offset_with_sort_key
    yy, xx = torch.meshgrid(torch.arange(16, dtype=F64), torch.arange(16, dtype=F64), indexing="ij")
    replay = steps is not None and not isinstance(steps, list)
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
                use0, sat, off = next(steps)
            else:
                use0 = alive & (a.detach() >= ALPHA_EPS)
                off = (torch.clamp(a, max=0.99) - a).detach()
                sat = use0 & ((T * (1 - (a + off))).detach() < 1e-4)
                if steps is not None:
                    steps.append((use0, sat, off))
            a_c = a + off                                         # clamp value, straight-through gradient
            nT = T * (1 - a_c)
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
    return image, depth, alpha


def _pose_inverse(q_pc, t_pc):
    """W (unnormalised conjugate, as the kernels) and t_cp = -R(q_cp / |q_cp|) t_pc, UTIL:426-432"""
    q_cp = torch.cat([-q_pc[:, :3], q_pc[:, 3:]], -1)
    R_unit = quat_to_R(q_cp / q_cp.norm(dim=-1, keepdim=True))
    return quat_to_R(q_cp), -(R_unit @ t_pc[..., None])[..., 0]


def _conics(J, Wm, f):
    R = quat_to_R(f[:, 0:4])
    S = torch.diag_embed(torch.exp(f[:, 4:7]))
    Sigma = R @ S @ S.transpose(-1, -2) @ R.transpose(-1, -2)
    U = J @ Wm
    cov = U @ Sigma @ U.transpose(-1, -2)
    cov_b = cov + 0.3 * torch.eye(2, dtype=F64)
    det_pre = cov[:, 0, 0] * cov[:, 1, 1] - cov[:, 0, 1] * cov[:, 1, 0]
    det = cov_b[:, 0, 0] * cov_b[:, 1, 1] - cov_b[:, 0, 1] * cov_b[:, 1, 0]
    rescale = torch.sqrt(torch.clamp(det_pre / det, min=0.0)).detach()
    return cov_b[:, 1, 1] / det, -cov_b[:, 0, 1] / det, cov_b[:, 0, 0] / det, rescale


def _J(Kmat, p):
    fx, fy = Kmat[0, 0], Kmat[1, 1]
    zero = torch.zeros_like(p[:, 0])
    return torch.stack([torch.stack([fx / p[:, 2], zero, -fx * p[:, 0] / p[:, 2] ** 2], -1),
                        torch.stack([zero, fy / p[:, 2], -fy * p[:, 1] / p[:, 2] ** 2], -1)], -2)


def _colour(f, Y):
    return torch.sigmoid(torch.stack([(f[:, 8:24] * Y).sum(-1), (f[:, 24:40] * Y).sum(-1), (f[:, 40:56] * Y).sum(-1)], -1))


def render(point_cloud, features, q_pc, t_pc, Kmat, H, W, fwd, object_id=None, stops=None):
    """torch_ref.render plus depth and alpha -> (image, depth, alpha, stops).  point_cloud (N,3), features (N,56) float64 leaves
    (features[:, :4] normalised: the oracle's features_after).  stops: None = compute and return them; a dict = replay it."""
    ids = torch.as_tensor(fwd.point_id_in_camera_list.astype(np.int64))
    obj = torch.zeros(point_cloud.shape[0], dtype=torch.long) if object_id is None else torch.as_tensor(np.asarray(object_id)).long()
    q_all = torch.as_tensor(np.asarray(q_pc, np.float64).reshape(-1, 4))
    t_all = torch.as_tensor(np.asarray(t_pc, np.float64).reshape(-1, 3))
    Kmat = torch.as_tensor(np.asarray(Kmat, np.float64))
    Wall, t_cp = _pose_inverse(q_all, t_all)
    Wm, tt = Wall[obj[ids]], t_cp[obj[ids]]
    xyz, f = point_cloud[ids], features[ids]
    pcam = (Wm @ xyz[..., None])[..., 0] + tt
    uv = ((Kmat @ pcam[..., None])[..., 0])[:, :2] / pcam[:, 2:3]
    rec = stops is None
    if rec:
        stops = {"pc": pcam.detach(), "dir": None, "blend": []}
    conic_a, conic_b, conic_c, rescale = _conics(_J(Kmat, stops["pc"]), Wm, f)
    if rec:
        stops["rescale"] = rescale
        origin = -(Wall.transpose(-1, -2) @ t_cp[..., None])[..., 0]
        stops["dir"] = (xyz - origin[obj[ids]]).detach()
    color = _colour(f, sh16(stops["dir"]))
    steps = stops["blend"] if rec else iter(stops["blend"])
    image, depth, alpha = blend(uv, conic_a, conic_b, conic_c, stops["rescale"], torch.sigmoid(f[:, 7]), color, pcam[:, 2],
                                H, W, fwd, steps)
    return image, depth, alpha, stops


def render_pose(point_cloud, features, q_pc, t_pc, Kmat, H, W, fwd, object_id=None):
    """pose_ref.render plus depth and alpha -> (image, depth, alpha, aux) with the per-point pose leaves aux["q_pts"] (M,4),
    aux["t_pts"] (M,3) and their object ids aux["obj"]."""
    ids = torch.as_tensor(fwd.point_id_in_camera_list.astype(np.int64))
    N = point_cloud.shape[0]
    obj = torch.zeros(N, dtype=torch.long) if object_id is None else torch.as_tensor(np.asarray(object_id)).long()
    oid = obj[ids]
    q_pts = torch.as_tensor(np.asarray(q_pc, np.float64).reshape(-1, 4))[oid].clone().requires_grad_(True)
    t_pts = torch.as_tensor(np.asarray(t_pc, np.float64).reshape(-1, 3))[oid].clone().requires_grad_(True)
    Kmat = torch.as_tensor(np.asarray(Kmat, np.float64))
    xyz = torch.as_tensor(np.asarray(point_cloud, np.float64))[ids]
    f = torch.as_tensor(np.asarray(features, np.float64))[ids]
    Wm, t_cp = _pose_inverse(q_pts, t_pts)
    pcam = (Wm @ xyz[..., None])[..., 0] + t_cp
    uv = ((Kmat @ pcam[..., None])[..., 0])[:, :2] / pcam[:, 2:3]
    conic_a, conic_b, conic_c, rescale = _conics(_J(Kmat, pcam), Wm, f)
    origin = -(Wm.transpose(-1, -2) @ t_cp[..., None])[..., 0]
    color = _colour(f, sh16(xyz - origin))
    image, depth, alpha = blend(uv, conic_a, conic_b, conic_c, rescale, torch.sigmoid(f[:, 7]), color, pcam[:, 2], H, W, fwd)
    return image, depth, alpha, {"q_pts": q_pts, "t_pts": t_pts, "obj": oid}


def _t(x):
    return None if x is None else torch.as_tensor(np.asarray(x, np.float64))


def point_gradients(scene, q, t, fwd, feat_after, g_image=None, g_depth=None, g_alpha=None):
    """(grad_pointcloud (N,3), grad_features (N,56)) of sum(g_image image) + sum(g_depth depth) + sum(g_alpha alpha), float64
    numpy, all grad factors 1 and every SH band."""
    pc = torch.tensor(np.asarray(scene.point_cloud, np.float64), requires_grad=True)
    ft = torch.tensor(np.asarray(feat_after, np.float64), requires_grad=True)
    img, dep, alp, _ = render(pc, ft, q, t, scene.camera_intrinsics, scene.height, scene.width, fwd, scene.point_object_id)
    loss = sum((out * _t(g)).sum() for out, g in ((img, g_image), (dep, g_depth), (alp, g_alpha)) if g is not None)
    loss.backward()
    grad = lambda x: x.grad.numpy() if x.grad is not None else np.zeros(x.shape)
    return grad(pc), grad(ft)


def pose_gradients(scene, q, t, fwd, feat_after, g_image=None, g_depth=None, g_alpha=None):
    """(grad_q (K,4), grad_t (K,3), summed_q, summed_t) of the same loss, as pose_ref.pose_gradients"""
    K = np.asarray(q).reshape(-1, 4).shape[0]
    img, dep, alp, aux = render_pose(scene.point_cloud, feat_after, q, t, scene.camera_intrinsics, scene.height, scene.width, fwd,
                                     scene.point_object_id)
    loss = 0.0
    for out, g in ((img, g_image), (dep, g_depth), (alp, g_alpha)):
        if g is not None:
            loss = loss + (out * _t(g)).sum()
    loss.backward()
    oid = aux["obj"]
    res = []
    for leaf, w in ((aux["q_pts"], 4), (aux["t_pts"], 3)):
        g = leaf.grad if leaf.grad is not None else torch.zeros(oid.shape[0], w, dtype=F64)
        res.append(torch.zeros(K, w, dtype=F64).index_add_(0, oid, g).numpy())
        res.append(torch.zeros(K, w, dtype=F64).index_add_(0, oid, g.abs()).numpy())
    return res[0], res[2], res[1], res[3]
