"""CPU: the depth / accumulated-alpha outputs of tests/torch_ref.py and their gradients, against the oracle's forward, float64
central finite differences of its replayed-stops function, and itself (an all-zero depth and alpha upstream is no upstream)."""
import numpy as np
import pytest
import torch

import parity_util as P
import torch_ref

CASES = [(0, 48, 0.25, 32, 32), (1, 64, 0.6, 32, 32), (3, 56, 0.5, 41, 27)]


def _case(seed, n, sigma0, width, height):
    s, q, t, partial = P.tiny_case(seed, n, sigma0, width, height)
    f, feat_after = P.oracle_frame(s, q, t, partial)
    assert f.pixel_valid_point_count.max() >= 3
    return s, q, t, f, feat_after


def _upstream(s, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, (s.height, s.width, 3)), rng.normal(0, 1, (s.height, s.width)), rng.normal(0, 1, (s.height, s.width)))


@pytest.mark.parametrize("case", CASES)
def test_zero_depth_and_alpha_upstream_is_torch_ref(case):
    """With an image upstream, all-zero depth and alpha upstreams give the same bits as none: the depth and alpha branches of
    the one render add exact zeros to the image's gradient, for the points and for the pose (so every image-only bar of the
    suite is a bar on the render that also carries depth and alpha)."""
    s, q, t, f, feat_after = _case(*case)
    gi, _, _ = _upstream(s, 1)
    zeros = np.zeros((s.height, s.width))
    for gradients in (torch_ref.point_gradients, torch_ref.pose_gradients):
        with_zeros = gradients(s, q, t, f, feat_after, gi, zeros, zeros)
        without = gradients(s, q, t, f, feat_after, gi, None, None)
        assert len(with_zeros) == len(without)
        for a, ref in zip(with_zeros, without):
            assert np.abs(ref).max() > 0
            P.assert_same_bits(a, ref, gradients.__name__)


@pytest.mark.parametrize("case", CASES)
def test_depth_and_alpha_match_the_oracle_forward(case):
    s, q, t, f, feat_after = _case(*case)
    pc = torch.tensor(s.point_cloud, dtype=torch.float64)
    ft = torch.tensor(feat_after, dtype=torch.float64)
    img, dep, alp, _ = torch_ref.render(pc, ft, q, t, s.camera_intrinsics, s.height, s.width, f)
    for name, a, ref in (("depth", dep, f.rasterized_depth), ("alpha", alp, f.pixel_accumulated_alpha)):
        a = a.numpy()
        assert np.abs(a - ref).max() <= 1e-5 * np.abs(ref).max(), name
    assert np.abs(img.numpy() - f.rasterized_image).max() <= 2e-5


@pytest.mark.parametrize("case", CASES)
def test_gradients_match_central_differences(case):
    """The gradient with stops is the plain derivative of the function with the stops replayed: central differences of that
    function (float64, h = 1e-6) at random elements of the positions and features, for depth, alpha and the image together."""
    s, q, t, f, feat_after = _case(*case)
    gi, gd, ga = _upstream(s, 2)
    gp, gf = torch_ref.point_gradients(s, q, t, f, feat_after, gi, gd, ga)
    pc0 = torch.tensor(s.point_cloud, dtype=torch.float64)
    ft0 = torch.tensor(feat_after, dtype=torch.float64)
    stops = torch_ref.render(pc0, ft0, q, t, s.camera_intrinsics, s.height, s.width, f)[3]["stops"]
    G = [torch.as_tensor(x) for x in (gi, gd, ga)]

    def L(pc, ft):
        img, dep, alp, _ = torch_ref.render(pc, ft, q, t, s.camera_intrinsics, s.height, s.width, f, stops=stops)
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
    gp_no_depth, _ = torch_ref.point_gradients(s, q, t, f, feat_after, gi, None, ga)
    assert np.abs(gp_no_depth - gp).max() > 1e-6 * np.abs(gp).max()

