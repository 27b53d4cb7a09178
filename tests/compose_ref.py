"""Baking a placed scene, restated in numpy / torch on the CPU: the reference the compose tests judge compose.py and
k_compose.hip by.  Nothing here imports the package's own statement of the same things.

  sh16(d)             the rasteriser's 16 colour basis functions (its signs, not the textbook ones), float64
  sh_matrices(R)      M_l with Y_l(R d) = M_l Y_l(d), l = 0..3, by least squares over random directions
  bake(...)           one similarity (q_A, t_A, s) applied to rows, in a dtype: float64 is the reference proper; float32 is the
                      error an f32 evaluation of the same formulas has, which sets the kernel's bar
  covariance(...)     R diag(exp(log s))^2 R^T of feature rows
  compose / inverse   similarities as (q, t, s) triples
"""
import numpy as np
import torch

BANDS = ((0, 1), (1, 4), (4, 9), (9, 16))


def sh16(d):
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    c1, c4, c6a, c6b, c8 = 0.48860251190291987, 1.0925484305920792, 0.94617469575755997, 0.31539156525251999, 0.54627421529603959
    c9, c10, c11, c12, c14 = 0.59004358992664352, 2.8906114426405538, 0.45704579946446572, 0.3731763325901154, 1.4453057213202769
    return np.stack([0.28209479177387814 + 0 * x, -c1 * y, c1 * z, -c1 * x,
                     c4 * x * y, -c4 * y * z, c6a * z * z - c6b, -c4 * x * z, c8 * (x * x - y * y),
                     c9 * y * (y * y - 3 * x * x), c10 * x * y * z, c11 * y * (1 - 5 * z * z), c12 * z * (5 * z * z - 3),
                     c11 * x * (1 - 5 * z * z), c14 * z * (x * x - y * y), c9 * x * (3 * y * y - x * x)], axis=-1)


def unit_directions(n, seed):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def rotation(q):
    """xyzw -> (3,3) float64 of q / |q|"""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def sh_matrices(R, seed=11, n=400):
    """-> [M_0 (1,1), M_1 (3,3), M_2 (5,5), M_3 (7,7)] float64 and the largest least-squares residual"""
    D = unit_directions(n, seed)
    Y, Yr = sh16(D), sh16(D @ np.asarray(R, np.float64).T)
    mats, worst = [], 0.0
    for lo, hi in BANDS:
        Mt = np.linalg.lstsq(Y[:, lo:hi], Yr[:, lo:hi], rcond=None)[0]
        worst = max(worst, float(np.abs(Y[:, lo:hi] @ Mt - Yr[:, lo:hi]).max()))
        mats.append(Mt.T)
    return mats, worst


def qmul(a, b):
    """Hamilton product a (x) b, xyzw, torch"""
    av, aw, bv, bw = a[..., :3], a[..., 3:4], b[..., :3], b[..., 3:4]
    return torch.cat([aw * bv + bw * av + torch.cross(av.expand_as(bv), bv, dim=-1), aw * bw - (av * bv).sum(-1, keepdim=True)], dim=-1)


def bake(xyz, features, q_A, t_A, scale, dtype=torch.float64):
    """rows under p -> scale R(q_A) p + t_A -> (xyz', features') in `dtype`.  The transform's constants (R, log scale, M_l) are
    made in float64 and rounded once to `dtype`, as the library makes them; the per-row arithmetic runs in `dtype`."""
    xyz, ft = torch.as_tensor(xyz).to(dtype), torch.as_tensor(features).to(dtype).clone()
    qa = np.asarray(q_A, np.float64) / np.linalg.norm(np.asarray(q_A, np.float64))
    R = rotation(qa)
    mats, _ = sh_matrices(R)
    sR = torch.tensor(float(scale) * R).to(dtype)
    out_xyz = xyz @ sR.T + torch.tensor(np.asarray(t_A, np.float64)).to(dtype)
    q = ft[:, 0:4]
    norm = q.norm(dim=1, keepdim=True)
    ok = (torch.isfinite(norm) & (norm > 0)).squeeze(1)
    rotated = qmul(torch.tensor(qa).to(dtype).expand(int(ok.sum()), 4), q[ok] / norm[ok])
    ft[ok, 0:4] = rotated
    ft[:, 4:7] = ft[:, 4:7] + torch.tensor(np.log(float(scale))).to(dtype)
    for c in range(3):
        for (lo, hi), M in zip(BANDS, mats):
            a, b = 8 + 16 * c + lo, 8 + 16 * c + hi
            ft[:, a:b] = torch.as_tensor(features).to(dtype)[:, a:b] @ torch.tensor(M).to(dtype).T
    return out_xyz, ft


def covariance(features):
    """(n,56) -> (n,3,3) float64: R(q / |q|) diag(exp(2 log s)) R^T"""
    ft = np.asarray(features, np.float64)
    out = np.empty((ft.shape[0], 3, 3))
    for i, row in enumerate(ft):
        R = rotation(row[0:4])
        out[i] = R @ np.diag(np.exp(2.0 * row[4:7])) @ R.T
    return out


def compose(A, B):
    """A o B as (q, t, s): p -> A(B(p))"""
    (qa, ta, sa), (qb, tb, sb) = A, B
    q = qmul(torch.tensor(np.asarray(qa, np.float64) / np.linalg.norm(qa)), torch.tensor(np.asarray(qb, np.float64) / np.linalg.norm(qb))).numpy()
    return q, sa * rotation(qa) @ np.asarray(tb, np.float64) + np.asarray(ta, np.float64), sa * sb


def inverse(A):
    q, t, s = A
    qi = np.asarray(q, np.float64) / np.linalg.norm(q) * [-1.0, -1.0, -1.0, 1.0]
    return qi, -(rotation(qi) @ np.asarray(t, np.float64)) / s, 1.0 / s


def random_scene(n, seed):
    """(xyz (n,3), features (n,56)) f32 numpy: non-unit quaternions, log-scales around -2, every SH band filled"""
    rng = np.random.default_rng(seed)
    xyz = rng.normal(0, 2.0, (n, 3)).astype(np.float32)
    ft = rng.normal(0, 0.5, (n, 56)).astype(np.float32)
    ft[:, 0:4] = rng.normal(0, 1.0, (n, 4)).astype(np.float32) * rng.uniform(0.2, 3.0, (n, 1)).astype(np.float32)
    ft[:, 4:7] -= 2.0
    return xyz, ft


def random_placement(seed, scale=1.0):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    return q / np.linalg.norm(q), rng.normal(0, 1.5, 3), float(scale)


# ---- the equivalence on rendered frames -----------------------------------------------------------------------------------
# (seed, points, sigma0, width = height) of parity_util.multi_object_case with three objects
EQUIVALENCE_CASES = ((1, 64, 0.5, 32), (2, 256, 0.5, 48), (3, 700, 0.15, 48), (4, 1200, 0.15, 64))


def equivalence_case(seed, n, sigma0, width):
    """-> (scene, q (3,4) unit, t (3,3), placements): the three-pose frame with its pose quaternions normalised, and the
    similarity A_k = T_0 o T_k^-1 that carries object k's rows into object 0's frame (the identity for object 0)"""
    import parity_util as U
    scene, q, t, _ = U.multi_object_case(seed, 3, n, sigma0, width, width)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    placements = [compose((q[0], t[0], 1.0), inverse((q[k], t[k], 1.0))) for k in range(3)]
    placements[0] = (np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3), 1.0)
    return scene, q, t, placements


def baked_into_first_frame(scene, placements):
    """a copy of the scene with the rows of objects 1.. baked by the float64 reference, rounded to f32, all of object 0"""
    import copy
    out = copy.copy(scene)
    out.point_cloud, out.point_cloud_features = scene.point_cloud.copy(), scene.point_cloud_features.copy()
    out.point_object_id = np.zeros_like(scene.point_object_id)
    for k, (qa, ta, sa) in enumerate(placements):
        rows = np.nonzero(scene.point_object_id == k)[0]
        if k == 0 or rows.size == 0:
            continue
        xyz, ft = bake(scene.point_cloud[rows], scene.point_cloud_features[rows], qa, ta, sa)
        out.point_cloud[rows], out.point_cloud_features[rows] = xyz.numpy().astype(np.float32), ft.numpy().astype(np.float32)
    return out


def assert_same_picture(image_a, count_a, image_b, count_b, report=None):
    """the bar of the equivalence: equal contributor counts at >= 99.5 % of the pixels, images within 1e-5 where the counts
    agree and within 2/255 elsewhere (a contributor on the 1/255 alpha threshold may flip; nothing else may)"""
    image_a, image_b = np.asarray(image_a, np.float64), np.asarray(image_b, np.float64)
    same = np.asarray(count_a) == np.asarray(count_b)
    diff = np.abs(image_a - image_b).max(axis=-1)
    figures = dict(same_count=float(same.mean()), max_diff_same=float(diff[same].max()) if same.any() else 0.0,
                   max_diff_other=float(diff[~same].max()) if (~same).any() else 0.0)
    if report is not None:
        print(report, figures)
    assert figures["same_count"] >= 0.995, figures
    assert figures["max_diff_same"] <= 1e-5, figures
    assert figures["max_diff_other"] <= 2.0 / 255.0, figures
    return figures
