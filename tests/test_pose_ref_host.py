"""CPU: the float64 pose-gradient reference (tests/pose_ref.py) that the GPU pose tests compare against is the derivative of
its own render: central finite differences for the oracle's fixed integer structure, with the gradient stops replayed."""
import numpy as np
import pytest
import torch

import pose_ref
from oracle import oracle
from taichi_3d_gaussian_splatting_amd.synthetic import synth


def _scene(seed, n, sigma0, width, height, n_objects):
    s = synth(n, width, height, sigma0, sh_deg=3, seed=seed)
    rng = np.random.default_rng(seed + 100)
    ang = 0.05
    q = np.array([[0.02, np.sin(ang / 2), -0.01, np.cos(ang / 2)]], np.float32) * np.float32(1.3)   # not unit
    t = np.array([[0.03, -0.02, 0.1]], np.float32)
    if n_objects > 1:
        s.point_object_id[:] = (np.arange(n) % n_objects).astype(np.int32)
        q = np.repeat(q, n_objects, 0) + rng.normal(0, 0.01, (n_objects, 4)).astype(np.float32)
        t = np.repeat(t, n_objects, 0) + rng.normal(0, 0.01, (n_objects, 3)).astype(np.float32)
    target = rng.uniform(0, 1, (height, width, 3))
    return s, q, t, target


@pytest.mark.parametrize("seed,n,sigma0,width,height,n_objects", [(0, 40, 0.4, 32, 32, 1), (3, 48, 0.5, 41, 27, 2)])
def test_pose_gradient_matches_finite_differences(seed, n, sigma0, width, height, n_objects):
    s, q, t, target = _scene(seed, n, sigma0, width, height, n_objects)
    cfg = oracle.default_config(allow_partial_tiles=int(width % 16 != 0 or height % 16 != 0))
    f, feat_after = oracle.forward(s.point_cloud, s.point_cloud_features, s.point_invalid_mask, s.point_object_id,
                                   q, t, s.camera_intrinsics, s.height, s.width, cfg)
    assert f.K > 0 and f.pixel_valid_point_count.max() >= 3
    img, _ = pose_ref.render(s.point_cloud, feat_after, q, t, s.camera_intrinsics, s.height, s.width, f, s.point_object_id)
    assert np.allclose(img.detach().numpy(), f.rasterized_image, atol=2e-5)      # the same frame as the f32 oracle
    g_img = 2.0 * (f.rasterized_image.astype(np.float64) - target)
    gq, gt, sq, st = pose_ref.pose_gradients(s, q, t, f, feat_after, g_img)
    assert np.all(np.abs(gq) <= sq * (1 + 1e-12)) and np.all(np.abs(gt) <= st * (1 + 1e-12))
    assert np.abs(gq).max() > 0 and np.abs(gt).max() > 0

    _, aux = pose_ref.render(s.point_cloud, feat_after, q, t, s.camera_intrinsics, s.height, s.width, f, s.point_object_id)
    stops = aux["stops"]
    G = torch.as_tensor(g_img)

    def loss(qq, tt):
        with torch.no_grad():
            im, _ = pose_ref.render(s.point_cloud, feat_after, qq, tt, s.camera_intrinsics, s.height, s.width, f,
                                    s.point_object_id, stops=stops)
            return float((im * G).sum())

    h = 1e-6
    q64, t64 = q.astype(np.float64), t.astype(np.float64)
    for which, base, grad in (("q", q64, gq), ("t", t64, gt)):
        fd = np.zeros_like(base)
        for idx in np.ndindex(base.shape):
            lo, hi = base.copy(), base.copy()
            lo[idx] -= h
            hi[idx] += h
            a = loss(lo, t64) if which == "q" else loss(q64, lo)
            b = loss(hi, t64) if which == "q" else loss(q64, hi)
            fd[idx] = (b - a) / (2 * h)
        err = np.abs(fd - grad).max() / np.abs(grad).max()
        assert err < 1e-6, (which, err, fd, grad)
