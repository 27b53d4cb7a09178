"""CPU: tests/depth_alpha_ref.py, the float64 reference of the depth / accumulated-alpha gradients, against torch_ref (zero
depth and alpha upstream), float64 central finite differences of its replayed-stops function, and the oracle's forward."""
import numpy as np
import pytest
import torch

import depth_alpha_ref
import pose_ref
import torch_ref
from oracle import oracle
from taichi_3d_gaussian_splatting_amd.synthetic import synth

CASES = [(0, 48, 0.25, 32, 32), (1, 64, 0.6, 32, 32), (3, 56, 0.5, 41, 27)]


def _tiny(seed, n, sigma0, width, height):
    s = synth(n, width, height, sigma0, sh_deg=3, seed=seed)
    ang = 0.05
    q = np.array([[0.02, np.sin(ang / 2), -0.01, np.cos(ang / 2)]], np.float32)     # deliberately not unit
    t = np.array([[0.03, -0.02, 0.1]], np.float32)
    partial = int(width % 16 != 0 or height % 16 != 0)
    f, feat_after = oracle.forward(s.point_cloud, s.point_cloud_features, s.point_invalid_mask, s.point_object_id, q, t,
                                   s.camera_intrinsics, s.height, s.width, oracle.default_config(allow_partial_tiles=partial))
    assert f.K > 0 and f.pixel_valid_point_count.max() >= 3
    return s, q, t, f, feat_after


def _upstream(s, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, (s.height, s.width, 3)), rng.normal(0, 1, (s.height, s.width)), rng.normal(0, 1, (s.height, s.width)))


@pytest.mark.parametrize("case", CASES)
def test_zero_depth_and_alpha_upstream_is_torch_ref(case):
    s, q, t, f, feat_after = _tiny(*case)
    gi, _, _ = _upstream(s, 1)
    pc = torch.tensor(s.point_cloud, dtype=torch.float64, requires_grad=True)
    ft = torch.tensor(feat_after, dtype=torch.float64, requires_grad=True)
    img, _ = torch_ref.render(pc, ft, q, t, s.camera_intrinsics, s.height, s.width, f)
    img.backward(torch.as_tensor(gi))
    zeros = np.zeros((s.height, s.width))
    gp, gf = depth_alpha_ref.point_gradients(s, q, t, f, feat_after, gi, zeros, zeros)
    np.testing.assert_array_equal(gp, pc.grad.numpy())
    np.testing.assert_array_equal(gf, ft.grad.numpy())
    # pose: the same against pose_ref
    rq, rt, _, _ = pose_ref.pose_gradients(s, q, t, f, feat_after, gi)
    aq, at, _, _ = depth_alpha_ref.pose_gradients(s, q, t, f, feat_after, gi, zeros, zeros)
    np.testing.assert_array_equal(aq, rq)
    np.testing.assert_array_equal(at, rt)


@pytest.mark.parametrize("case", CASES)
def test_depth_and_alpha_match_the_oracle_forward(case):
    s, q, t, f, feat_after = _tiny(*case)
    pc = torch.tensor(s.point_cloud, dtype=torch.float64)
    ft = torch.tensor(feat_after, dtype=torch.float64)
    img, dep, alp, _ = depth_alpha_ref.render(pc, ft, q, t, s.camera_intrinsics, s.height, s.width, f)
    for name, a, ref in (("depth", dep, f.rasterized_depth), ("alpha", alp, f.pixel_accumulated_alpha)):
        a = a.numpy()
        assert np.abs(a - ref).max() <= 1e-5 * np.abs(ref).max(), name
    assert np.abs(img.numpy() - f.rasterized_image).max() <= 2e-5


@pytest.mark.parametrize("case", CASES)
def test_gradients_match_central_differences(case):
    """The gradient with stops is the plain derivative of the function with the stops replayed: central differences of that
    function (float64, h = 1e-6) at random elements of the positions and features, for depth, alpha and the image together."""
    s, q, t, f, feat_after = _tiny(*case)
    gi, gd, ga = _upstream(s, 2)
    gp, gf = depth_alpha_ref.point_gradients(s, q, t, f, feat_after, gi, gd, ga)
    pc0 = torch.tensor(s.point_cloud, dtype=torch.float64)
    ft0 = torch.tensor(feat_after, dtype=torch.float64)
    _, _, _, stops = depth_alpha_ref.render(pc0, ft0, q, t, s.camera_intrinsics, s.height, s.width, f)
    G = [torch.as_tensor(x) for x in (gi, gd, ga)]

    def L(pc, ft):
        img, dep, alp, _ = depth_alpha_ref.render(pc, ft, q, t, s.camera_intrinsics, s.height, s.width, f, stops=stops)
        return float((img * G[0]).sum() + (dep * G[1]).sum() + (alp * G[2]).sum())

    rng = np.random.default_rng(case[0])
    ids = f.point_id_in_camera_list
    h = 1e-6
    checked = 0
    for which, grad, base in (("pc", gp, pc0), ("ft", gf, ft0)):
        cols = [0, 1, 2] if which == "pc" else [0, 4, 7, 8, 30]
        for _ in range(8):
            i, j = int(rng.choice(ids)), int(rng.choice(cols))
            up, dn = base.clone(), base.clone()
            up[i, j] += h
            dn[i, j] -= h
            args_up = (up, ft0) if which == "pc" else (pc0, up)
            args_dn = (dn, ft0) if which == "pc" else (pc0, dn)
            fd = (L(*args_up) - L(*args_dn)) / (2 * h)
            scale = max(np.abs(grad).max(), 1e-12)
            assert abs(fd - grad[i, j]) <= 1e-5 * scale + 1e-6 * abs(grad[i, j]), (which, i, j, fd, grad[i, j])
            checked += 1
    assert checked == 16
    # the depth term does reach the positions: without it the xyz gradient changes
    gp_no_depth, _ = depth_alpha_ref.point_gradients(s, q, t, f, feat_after, gi, None, ga)
    assert np.abs(gp_no_depth - gp).max() > 1e-6 * np.abs(gp).max()

