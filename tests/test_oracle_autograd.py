"""CPU: the oracle's analytic backward against float64 torch.autograd on tiny scenes
(tests/torch_ref.py).  Pins what the reference's tests leave open: loop-1 accumulation,
SH colour gradient, opacity gradient, loop-2 chain, band masks and grad factors."""
import numpy as np
import pytest

import parity_util as P
from oracle import oracle


def _case(seed, n, sigma0, width=32, height=None):
    """P.tiny_case and P.random_target -> (scene, q, t, target)"""
    s, q, t, _ = P.tiny_case(seed, n, sigma0, width, height)
    return s, q, t, P.random_target(s, seed + 100)


@pytest.mark.parametrize("seed,n,sigma0,width,height", [(0, 48, 0.25, 32, 32), (1, 64, 0.6, 32, 32), (2, 24, 1.2, 32, 32),
                                                         (3, 56, 0.5, 41, 27)])
def test_backward_matches_autograd(seed, n, sigma0, width, height):
    """The last case is the partial-tile extension (41x27: neither side a multiple of 16)."""
    s, q, t, target = _case(seed, n, sigma0, width, height)
    P.assert_oracle_matches_autograd(s, q, t, target, int(width % 16 != 0 or height % 16 != 0))


def test_band_mask_and_factors():
    """RAST:1102-1125, 1167-1182: masked bands are zero, the rest scaled by 5 / 1 / 0.5 / 1 / 20."""
    s, q, t, target = _case(3, 40, 0.5)
    unit = oracle.default_config(**P.UNIT_FACTORS)
    ref_cfg = oracle.default_config()
    f, _ = oracle.forward(s.point_cloud, s.point_cloud_features, s.point_invalid_mask, s.point_object_id,
                          q, t, s.camera_intrinsics, s.height, s.width, unit)
    g = (2.0 * (f.rasterized_image - target)).astype(np.float32)
    raw = oracle.backward(f, g, 3, unit)["grad_pointcloud_features"]
    for band, keep in [(0, 1), (1, 4), (2, 9), (3, 16), (5, 16)]:
        got = oracle.backward(f, g, band, ref_cfg)["grad_pointcloud_features"]
        exp = raw.copy()
        exp[:, 0:4] *= 1.0
        exp[:, 4:7] *= 0.5
        exp[:, 7] *= 20.0
        for base in (8, 24, 40):
            exp[:, base] *= 5.0
            exp[:, base + keep: base + 16] = 0.0
        assert np.allclose(got, exp, rtol=1e-6, atol=1e-12), band


def test_hook_extras_consistency():
    """num_affected_pixels counts contributions; magnitude image is the per-pixel sum of |d uv|."""
    s, q, t, target = _case(4, 32, 0.5)
    f, _ = oracle.forward(s.point_cloud, s.point_cloud_features, s.point_invalid_mask, s.point_object_id,
                          q, t, s.camera_intrinsics, s.height, s.width)
    g = (2.0 * (f.rasterized_image - target)).astype(np.float32)
    b = oracle.backward(f, g, 3)
    # every blended contribution is revisited in backward unless it straddles the 1/255 edge
    assert abs(int(b["num_affected_pixels"].sum()) - int(f.pixel_valid_point_count.sum())) <= 2
    assert b["magnitude_grad_viewspace_on_image"].min() >= 0
    assert b["magnitude_grad_viewspace"].min() >= 0
    # points outside the frustum get exactly zero gradient (RAST:1051-1058 zero-init)
    out = np.setdiff1d(np.arange(f.N), f.point_id_in_camera_list)
    assert np.all(b["grad_pointcloud"][out] == 0) and np.all(b["grad_pointcloud_features"][out] == 0)


def test_summed_magnitudes_bound_the_gradients():
    """gso_backward_ex's "summed" outputs (the floor of the GPU tests' per-element bar): every gradient element is bounded by
    the magnitude summed to produce it (triangle inequality, up to rounding), is exactly zero where nothing was summed,
    and masked SH bands / rows outside the frustum have nothing summed."""
    s, q, t, target = _case(5, 400, 0.3, 64, 48)
    f, _ = oracle.forward(s.point_cloud, s.point_cloud_features, s.point_invalid_mask, s.point_object_id,
                          q, t, s.camera_intrinsics, s.height, s.width)
    g = (2.0 * (f.rasterized_image - target)).astype(np.float32)
    b = oracle.backward(f, g, 1, want_summed=True)
    plain = oracle.backward(f, g, 1)
    assert np.array_equal(plain["grad_pointcloud_features"], b["grad_pointcloud_features"])
    for gk, sk in [("grad_pointcloud", "summed_pointcloud"), ("grad_pointcloud_features", "summed_pointcloud_features")]:
        G, S = np.abs(b[gk]).astype(np.float64), b[sk].astype(np.float64)
        assert np.all(G <= S * (1 + 1e-5)), gk
        assert not G[S == 0].any(), gk
        assert (S > 0).any()
    Sf = b["summed_pointcloud_features"]
    for base in (8, 24, 40):
        assert not Sf[:, base + 4: base + 16].any()           # band 1 keeps coefficients 0..3
    out = np.setdiff1d(np.arange(f.N), f.point_id_in_camera_list)
    assert not Sf[out].any() and not b["summed_pointcloud"][out].any()
