"""Float64 torch.autograd reference of the POSE gradient (tests only).

Built from tests/torch_ref.py's pieces (quat_to_R, sh16) and the same integer structure taken from the CPU
oracle (visible ids, sorted per-tile lists, tile ranges).  Two differences from torch_ref.render:
  * J is built from the live camera-space position p, and the SH view direction d = x - o is live: the pose
    gradient is the derivative of the forward as it is computed, J(p) and view-direction paths included;
  * the pose is expanded to per-point leaves (q[obj[ids]] (M,4), t[obj[ids]] (M,3)), so that autograd yields each
    point's contribution; their index_add by object is the gradient, the index_add of their absolute values the
    summed magnitude of the per-element bar (parity_util.elem_margins style).
The blend-level stops of torch_ref stay (they live in the upstream loop 1 hands over): rescale is a constant, the
0.99 clamp is straight-through, depth and count carry no gradient, sort / cull / radius are discrete.
"""
import numpy as np
import torch

from torch_ref import ALPHA_EPS, F64, quat_to_R, sh16


def render(point_cloud, features, q_pc, t_pc, Kmat, H, W, fwd, object_id=None, stops=None):
    """-> image (H,W,3) f64, aux with the per-point pose leaves "q_pts" (M,4), "t_pts" (M,3), "obj" (M) object ids and
    "stops", the values the gradient stops froze (rescale, and per blend step the masks and the clamp offset).
    point_cloud (N,3), features (N,56) (normalised quaternions: the oracle's features_after), q_pc (K,4), t_pc (K,3).
    stops: the "stops" of an earlier call, replayed instead of recomputed -- a function whose plain derivative is the
    gradient with stops (finite differences of it check the autograd gradient)."""
    ids = torch.as_tensor(fwd.point_id_in_camera_list.astype(np.int64))
    N = point_cloud.shape[0]
    obj = torch.zeros(N, dtype=torch.long) if object_id is None else torch.as_tensor(np.asarray(object_id)).long()
    oid = obj[ids]
    q_all = torch.as_tensor(np.asarray(q_pc, np.float64).reshape(-1, 4))
    t_all = torch.as_tensor(np.asarray(t_pc, np.float64).reshape(-1, 3))
    q_pts = q_all[oid].clone().requires_grad_(True)
    t_pts = t_all[oid].clone().requires_grad_(True)
    Kmat = torch.as_tensor(np.asarray(Kmat, np.float64))
    xyz = torch.as_tensor(np.asarray(point_cloud, np.float64))[ids]
    f = torch.as_tensor(np.asarray(features, np.float64))[ids]
    # pose: inverse of (q_pc, t_pc), UTIL:426-432 (the conjugate is NOT renormalised for W)
    q_cp = torch.cat([-q_pts[:, :3], q_pts[:, 3:]], -1)
    R_unit = quat_to_R(q_cp / q_cp.norm(dim=-1, keepdim=True))
    t_cp = -(R_unit @ t_pts[..., None])[..., 0]
    Wm = quat_to_R(q_cp)
    pcam = (Wm @ xyz[..., None])[..., 0] + t_cp
    uv1 = (Kmat @ pcam[..., None])[..., 0]
    uv = uv1[:, :2] / pcam[:, 2:3]
    fx, fy = Kmat[0, 0], Kmat[1, 1]
    zero = torch.zeros_like(pcam[:, 0])
    J = torch.stack([torch.stack([fx / pcam[:, 2], zero, -fx * pcam[:, 0] / pcam[:, 2] ** 2], -1),
                     torch.stack([zero, fy / pcam[:, 2], -fy * pcam[:, 1] / pcam[:, 2] ** 2], -1)], -2)
    R = quat_to_R(f[:, 0:4])
    S = torch.diag_embed(torch.exp(f[:, 4:7]))
    Sigma = R @ S @ S.transpose(-1, -2) @ R.transpose(-1, -2)
    U = J @ Wm
    cov = U @ Sigma @ U.transpose(-1, -2)
    cov_b = cov + 0.3 * torch.eye(2, dtype=F64)
    det_pre = cov[:, 0, 0] * cov[:, 1, 1] - cov[:, 0, 1] * cov[:, 1, 0]
    det = cov_b[:, 0, 0] * cov_b[:, 1, 1] - cov_b[:, 0, 1] * cov_b[:, 1, 0]
    rescale = torch.sqrt(torch.clamp(det_pre / det, min=0.0)).detach() if stops is None else stops["rescale"]
    conic_a, conic_b, conic_c = cov_b[:, 1, 1] / det, -cov_b[:, 0, 1] / det, cov_b[:, 0, 0] / det
    opacity = torch.sigmoid(f[:, 7])
    # colour: camera centre as the forward computes it, o = -W^T t_cp (origin_fwd)
    origin = -(Wm.transpose(-1, -2) @ t_cp[..., None])[..., 0]
    Y = sh16(xyz - origin)
    color = torch.sigmoid(torch.stack([(f[:, 8:24] * Y).sum(-1), (f[:, 24:40] * Y).sum(-1), (f[:, 40:56] * Y).sum(-1)], -1))
    steps = [] if stops is None else list(reversed(stops["blend"]))
    image = blend(uv, conic_a, conic_b, conic_c, rescale, opacity, color, H, W, fwd, steps, replay=stops is not None)
    return image, {"q_pts": q_pts, "t_pts": t_pts, "obj": oid, "stops": {"rescale": rescale, "blend": steps}}


def blend(uv, conic_a, conic_b, conic_c, rescale, opacity, color, H, W, fwd, steps, replay):
    """torch_ref.render's blend, on the oracle's tile lists.  replay: pop (use, sat, clamp offset) of every step from `steps`
    instead of computing them; otherwise append them."""
    image = torch.zeros(H, W, 3, dtype=F64)
    tiles_x = (W + 15) // 16
    lst = fwd.point_offset_with_sort_key
    yy, xx = torch.meshgrid(torch.arange(16, dtype=F64), torch.arange(16, dtype=F64), indexing="ij")
    for tile in range(tiles_x * ((H + 15) // 16)):
        s, e = int(fwd.tile_points_start[tile]), int(fwd.tile_points_end[tile])
        if e <= s:
            continue
        tu, tv = tile % tiles_x, tile // tiles_x
        px = (xx + tu * 16 + 0.5).reshape(-1)
        py = (yy + tv * 16 + 0.5).reshape(-1)
        T = torch.ones(256, dtype=F64)
        C = torch.zeros(256, 3, dtype=F64)
        alive = torch.ones(256, dtype=torch.bool)
        for idx in range(s, e):
            p = int(lst[idx])
            dx, dy = px - uv[p, 0], py - uv[p, 1]
            g = torch.exp(-0.5 * (dx * dx * conic_a[p] + dy * dy * conic_c[p]) - dx * dy * conic_b[p]) * rescale[p]
            a = g * opacity[p]
            if replay:
                use0, sat, off = steps.pop()
                a_c = a + off
                nT = T * (1 - a_c)
            else:
                use0 = alive & (a.detach() >= ALPHA_EPS)
                off = (torch.clamp(a, max=0.99) - a).detach()
                a_c = a + off                                         # clamp value, straight-through gradient
                nT = T * (1 - a_c)
                sat = use0 & (nT.detach() < 1e-4)
                steps.append((use0, sat, off))
            alive = alive & ~sat
            use = use0 & ~sat
            w = torch.where(use, a_c * T, torch.zeros_like(T))
            C = C + w[:, None] * color[p][None, :]
            T = torch.where(use, nT, T)
        hh, ww = min(16, H - tv * 16), min(16, W - tu * 16)
        image[tv * 16:tv * 16 + hh, tu * 16:tu * 16 + ww, :] = C.reshape(16, 16, 3)[:hh, :ww]
    return image


def pose_gradients(scene, q, t, fwd, feat_after, g_image):
    """(grad_q (K,4), grad_t (K,3), summed_q (K,4), summed_t (K,3)) of sum(g_image * image), float64 numpy."""
    K = np.asarray(q).reshape(-1, 4).shape[0]
    img, aux = render(scene.point_cloud, feat_after, q, t, scene.camera_intrinsics, scene.height, scene.width, fwd,
                      scene.point_object_id)
    img.backward(torch.as_tensor(np.asarray(g_image, np.float64)))
    oid = aux["obj"]
    out = []
    for leaf, w in ((aux["q_pts"], 4), (aux["t_pts"], 3)):
        g = leaf.grad if leaf.grad is not None else torch.zeros(0, w, dtype=F64)
        out.append(torch.zeros(K, w, dtype=F64).index_add_(0, oid, g).numpy())
        out.append(torch.zeros(K, w, dtype=F64).index_add_(0, oid, g.abs()).numpy())
    return out[0], out[2], out[1], out[3]
