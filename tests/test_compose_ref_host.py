"""CPU: the float64 reference of the bake (tests/compose_ref.py) against the properties it must have, the package's own SH
matrices against it, and the equivalence 'composition under K pose rows = baked scene under one pose' on the CPU oracle."""
import numpy as np
import pytest
import torch

import compose_ref as R
import parity_util as U


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_rotated_coefficients_reproduce_the_colour(seed):
    """sum f'_k Y_k(R d) = sum f_k Y_k(d) on 1000 random directions; M_l is orthogonal and fits exactly"""
    q, _, _ = R.random_placement(seed)
    Rm = R.rotation(q)
    mats, residual = R.sh_matrices(Rm)
    assert residual < 1e-13
    for M in mats:
        assert np.abs(M @ M.T - np.eye(M.shape[0])).max() < 1e-13
    f = np.random.default_rng(seed).normal(size=16)
    fp = np.concatenate([M @ f[lo:hi] for (lo, hi), M in zip(R.BANDS, mats)])
    d = R.unit_directions(1000, seed + 100)
    assert np.abs(R.sh16(d @ Rm.T) @ fp - R.sh16(d) @ f).max() < 1e-12


def test_package_matrices_equal_the_reference():
    """compose.sh_rotation_matrices (fixed sample directions) against the reference's (random ones), and its basis"""
    from taichi_3d_gaussian_splatting_amd import compose
    d = R.unit_directions(50, 5)
    assert np.abs(compose.sh_basis(d) - R.sh16(d)).max() < 1e-15
    for seed in range(4):
        q, _, _ = R.random_placement(seed)
        mats, _ = R.sh_matrices(R.rotation(q))
        got = compose.sh_rotation_matrices(compose.quaternion_to_matrix(q))
        assert got.shape == (compose.SH_FLOATS,)
        assert np.abs(got - np.concatenate([M.reshape(-1) for M in mats])).max() < 1e-13
    ident = compose.sh_rotation_matrices(np.eye(3))
    assert np.abs(ident - np.concatenate([np.eye(k).reshape(-1) for k in (1, 3, 5, 7)])).max() < 1e-14


@pytest.mark.parametrize("scale", [1.0, 2.5])
def test_baked_covariance_is_the_rotated_covariance(scale):
    xyz, ft = R.random_scene(50, 3)
    q, t, _ = R.random_placement(4)
    _, baked = R.bake(xyz, ft, q, t, scale)
    Rm = R.rotation(q)
    want = scale ** 2 * np.einsum("ij,njk,lk->nil", Rm, R.covariance(ft), Rm)
    got = R.covariance(baked.numpy())
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_composition_law():
    """bake(A) o bake(B) = bake(A o B), up to the sign of the quaternion"""
    xyz, ft = R.random_scene(40, 6)
    A, B = R.random_placement(7, 2.5), R.random_placement(8, 0.4)
    x1, f1 = R.bake(*R.bake(xyz, ft, *B), *A)
    x2, f2 = R.bake(xyz, ft, *R.compose(A, B))
    assert torch.allclose(x1, x2, rtol=0, atol=1e-12)
    sign = torch.sign((f1[:, 0:4] * f2[:, 0:4]).sum(1, keepdim=True))
    assert torch.allclose(f1[:, 0:4], sign * f2[:, 0:4], rtol=0, atol=1e-12)
    assert torch.allclose(f1[:, 4:], f2[:, 4:], rtol=0, atol=1e-12)
    xi, fi = R.bake(x2, f2, *R.inverse(R.compose(A, B)))
    assert torch.allclose(xi, torch.as_tensor(xyz).double(), rtol=0, atol=1e-11)
    assert torch.allclose(fi[:, 4:], torch.as_tensor(ft).double()[:, 4:], rtol=0, atol=1e-11)


def test_rows_without_a_direction_keep_their_quaternion():
    xyz, ft = R.random_scene(4, 9)
    ft[1, 0:4] = 0.0
    ft[2, 1] = np.nan
    q, t, s = R.random_placement(10, 2.5)
    _, baked = R.bake(xyz, ft, q, t, s)
    assert torch.equal(baked[1, 0:4], torch.zeros(4, dtype=torch.float64))
    assert np.array_equal(np.isnan(baked[2, 0:4].numpy()), [False, True, False, False])
    assert torch.isfinite(baked[:, 4:]).all()
    assert torch.allclose(baked[1, 4:7], torch.as_tensor(ft[1, 4:7]).double() + np.log(2.5))


@pytest.mark.parametrize("seed,n,sigma0,width", R.EQUIVALENCE_CASES)
def test_baked_scene_under_one_pose_equals_the_frame_of_three_poses(seed, n, sigma0, width):
    """objects 1 and 2 baked into object 0's frame by the float64 reference (rounded to f32): the oracle's image under the one
    pose against its image of the three-pose frame.  Measured on these inputs: counts equal at every pixel, images within
    1.2e-6."""
    scene, q, t, placements = R.equivalence_case(seed, n, sigma0, width)
    f3, _ = U.run_oracle(scene, q, t)
    f1, _ = U.run_oracle(R.baked_into_first_frame(scene, placements), q[:1], t[:1])
    assert f3.K > 0
    R.assert_same_picture(f1.rasterized_image, f1.pixel_valid_point_count, f3.rasterized_image, f3.pixel_valid_point_count,
                          report=f"oracle {seed}:")


def test_a_non_unit_pose_breaks_the_equivalence():
    """why SceneComposition asks for unit poses: with the deliberately non-unit pose of multi_object_case the same bake no
    longer shows the same picture (the pose's matrix scales)"""
    import parity_util
    scene, q, t, _ = parity_util.multi_object_case(1, 3, 64, 0.5, 32, 32)
    placements = [R.compose((q[0], t[0], 1.0), R.inverse((q[k], t[k], 1.0))) for k in range(3)]
    f3, _ = U.run_oracle(scene, q, t)
    f1, _ = U.run_oracle(R.baked_into_first_frame(scene, placements), q[:1], t[:1])
    assert np.abs(f1.rasterized_image - f3.rasterized_image).max() > 1e-4
