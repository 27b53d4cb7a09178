"""GPU: the scene bake (k_compose.hip through compose.py) against the float64 reference of tests/compose_ref.py, the
properties of the call, SceneComposition, and the equivalence 'K pose rows = baked scene under one pose' on the rasteriser.

The bar of a group of outputs (positions, quaternions, log-scales, colour coefficients) is 4 x the largest error that the same
formulas evaluated with torch in float32 on the CPU make against float64 on that input (compose_ref.bake in the two dtypes),
with half an ulp of the group's largest value as the floor of that error: the margin the mixture-gradient tests use for f32
reordering.  Measured on an MI355X over every case below: the bars come to 3.8e-7 .. 8.6e-6 (positions, |p| up to
20 at scale 2.5), 2.1e-7 .. 5.8e-7 (quaternions), 2.2e-7 .. 1.1e-6 (log-scales) and 2.9e-7 .. 1.6e-6 (colour); the
kernel's largest error over bar is 0.47 for positions (1.8e-7 against 3.8e-7, n = 1), 0.33 for quaternions, 0.22 for
log-scales and 0.28 for colour; the opacity logit is copied bit for bit.  The rasteriser shows the composition and its bake
with equal contributor counts at every pixel and images within 1.5e-6 on all four frames.
"""
import functools

import numpy as np
import pytest
import torch

import compose_ref as R
import parity_util as U
from taichi_3d_gaussian_splatting_amd import CameraInfo, compose

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
GROUPS = {"xyz": None, "q": slice(0, 4), "log_s": slice(4, 7), "alpha": slice(7, 8), "sh": slice(8, 56)}
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
OFFSETS = [0, 1, 3, 257]
HALF_TURN = (np.array([np.sin(np.radians(179.9) / 2) * 0.6, 0.0, np.sin(np.radians(179.9) / 2) * 0.8, np.cos(np.radians(179.9) / 2)]),
             np.array([0.3, -1.0, 2.0]), 1.0)          # a 179.9 degree rotation: w of q_A is almost zero


def _groups(xyz, ft):
    return {name: (xyz if sl is None else ft[:, sl]) for name, sl in GROUPS.items()}


@functools.lru_cache(maxsize=None)
def _case(n, seed, placement_key):
    """-> (xyz, features) f32 numpy, the placement, the float64 reference's groups and the bar of each"""
    xyz, ft = R.random_scene(n, seed)
    placement = HALF_TURN if placement_key == "half_turn" else R.random_placement(seed + 50, scale=placement_key)
    ref = _groups(*R.bake(xyz, ft, *placement))
    f32 = _groups(*R.bake(xyz, ft, *placement, dtype=torch.float32))
    bars = {}
    for name in ref:
        err = float((f32[name].double() - ref[name]).abs().max()) if n else 0.0
        bars[name] = 4.0 * max(err, EPS * float(ref[name].abs().max()) if n else 0.0)
    return xyz, ft, placement, ref, bars


def _assert_within_bars(got_xyz, got_ft, ref, bars, what):
    got = _groups(got_xyz.cpu().double(), got_ft.cpu().double())
    for name in ref:
        err = float((got[name] - ref[name]).abs().max())
        print(f"{what} {name}: kernel error {err:.3e}, bar {bars[name]:.3e}")
        assert err <= bars[name], (what, name, err, bars[name])
    assert torch.equal(got["alpha"], ref["alpha"])                  # the opacity logit is copied


def _guarded(rows, width, seed):
    """a tensor of `rows` rows of a NaN bit pattern that no arithmetic produces"""
    pattern = torch.full((rows, width), 0x7FC0BEEF + seed, dtype=torch.int32, device=DEV)
    return pattern.view(torch.float32)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_the_reference(n, offset):
    scale = 2.5 if (SIZES.index(n) + OFFSETS.index(offset)) % 2 else 1.0
    xyz, ft, placement, ref, bars = _case(n, n, scale)
    tail = 5
    out_xyz, out_ft = _guarded(offset + n + tail, 3, 1), _guarded(offset + n + tail, 56, 2)
    before_xyz, before_ft = out_xyz.clone(), out_ft.clone()
    compose.scene_bake(torch.from_numpy(xyz).to(DEV), torch.from_numpy(ft).to(DEV), *placement, out_xyz, out_ft, row_offset=offset)
    _assert_within_bars(out_xyz[offset:offset + n], out_ft[offset:offset + n], ref, bars, f"n={n} offset={offset} s={scale}")
    # rows outside [offset, offset + n) keep their bits, on both sides
    for got, before in ((out_xyz, before_xyz), (out_ft, before_ft)):
        for rows in (slice(0, offset), slice(offset + n, None)):
            assert torch.equal(got[rows].view(torch.int32), before[rows].view(torch.int32))


@pytest.mark.parametrize("n", [65, 1000])
def test_a_half_turn(n):
    xyz, ft, placement, ref, bars = _case(n, n + 1, "half_turn")
    got = compose.scene_bake(torch.from_numpy(xyz).to(DEV), torch.from_numpy(ft).to(DEV), *placement)
    _assert_within_bars(*got, ref, bars, f"half turn n={n}")


def test_same_bits_every_run_and_unaligned_features():
    xyz, ft, placement, ref, bars = _case(257, 257, 2.5)
    x, f = torch.from_numpy(xyz).to(DEV), torch.from_numpy(ft).to(DEV)
    a = compose.scene_bake(x, f, *placement)
    b = compose.scene_bake(x, f, *placement)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    # features that do not start on a 16-byte boundary take the scalar copies: the same bits
    flat = torch.zeros(257 * 56 + 1, device=DEV)
    flat[1:] = f.reshape(-1)
    c = compose.scene_bake(x, flat[1:].view(257, 56), *placement)
    assert torch.equal(a[1].view(torch.int32), c[1].view(torch.int32)) and torch.equal(a[0].view(torch.int32), c[0].view(torch.int32))


def test_identity_placement_keeps_the_position_bits():
    xyz, ft = R.random_scene(300, 5)
    x, f = torch.from_numpy(xyz).to(DEV), torch.from_numpy(ft).to(DEV)
    out_x, out_f = compose.scene_bake(x, f, [0, 0, 0, 1], [0, 0, 0], 1.0)
    assert torch.equal(out_x.view(torch.int32), x.view(torch.int32))
    assert torch.equal(out_f[:, 4:].view(torch.int32), f[:, 4:].view(torch.int32))           # log-scales, opacity, colour: M_l = 1
    unit = f[:, 0:4] / f[:, 0:4].norm(dim=1, keepdim=True)
    assert float((out_f[:, 0:4] - unit).abs().max()) <= 4 * 2.0 ** -24


def test_rows_without_a_direction_keep_their_quaternion_words():
    xyz, ft = R.random_scene(70, 6)
    ft[3, 0:4] = 0.0
    ft[64, 0:4] = [0.5, np.nan, 0.5, 0.5]
    ft[69, 0:4] = [np.inf, 0.0, 0.0, 1.0]
    placement = R.random_placement(12, 2.5)
    ref = _groups(*R.bake(xyz, ft, *placement))
    out_x, out_f = compose.scene_bake(torch.from_numpy(xyz).to(DEV), torch.from_numpy(ft).to(DEV), *placement)
    for row in (3, 64, 69):
        assert np.array_equal(out_f[row, 0:4].cpu().numpy().view(np.int32), ft[row, 0:4].view(np.int32)), row
        assert torch.allclose(out_f[row, 4:].cpu().double(), R.bake(xyz, ft, *placement)[1][row, 4:], rtol=1e-5, atol=1e-6)
    assert torch.allclose(out_x.cpu().double(), ref["xyz"], rtol=1e-5, atol=1e-5)
    keep = [r for r in range(70) if r not in (3, 64, 69)]
    assert torch.allclose(out_f[keep].cpu().double()[:, 0:4], ref["q"][keep], rtol=0, atol=1e-6)


def _composition(sizes, seed):
    scenes = [R.random_scene(n, seed + k) for k, n in enumerate(sizes)]
    return scenes, compose.SceneComposition(scenes, device=DEV)


@pytest.mark.parametrize("sizes", [(130,), (100, 0, 37)])
def test_composition_bakes_every_object_into_its_rows(sizes):
    scenes, comp = _composition(sizes, 20)
    K = len(sizes)
    assert len(comp) == K and comp.scene.point_cloud.shape[0] == sum(sizes)
    placements = [R.random_placement(30 + k, scale=(1.0, 2.5, 0.5)[k]) for k in range(K)]
    for k, p in enumerate(placements):
        comp.place(k, p[0] * 3.0, p[1], p[2])                      # normalised on entry
    ids = comp.scene.point_object_id.cpu().numpy()
    assert np.array_equal(ids, np.concatenate([np.full(n, k, np.int32) for k, n in enumerate(sizes)]))
    infos = comp.extra_scene_info_dict
    assert [(infos[k].start_offset, infos[k].end_offset, infos[k].visible) for k in range(K)] == \
        [(sum(sizes[:k]), sum(sizes[:k + 1]), True) for k in range(K)]
    assert torch.allclose(infos[0].center.cpu(), torch.from_numpy(scenes[0][0]).mean(dim=0), atol=1e-5)
    baked = comp.bake()
    assert int(baked.point_object_id.abs().max()) == 0 and baked.point_cloud.shape[0] == sum(sizes)
    for k, n in enumerate(sizes):
        if n == 0:
            continue
        a, b = infos[k].start_offset, infos[k].end_offset
        xyz, ft = scenes[k]
        ref = _groups(*R.bake(xyz, ft, *placements[k]))
        f32 = _groups(*R.bake(xyz, ft, *placements[k], dtype=torch.float32))
        bars = {g: 4.0 * max(float((f32[g].double() - ref[g]).abs().max()), EPS * float(ref[g].abs().max())) for g in ref}
        _assert_within_bars(baked.point_cloud.detach()[a:b], baked.point_cloud_features.detach()[a:b], ref, bars, f"object {k}")


def test_composition_visibility_and_pose_rows():
    scenes, comp = _composition((40, 25, 10), 40)
    mask = comp.scene.point_invalid_mask
    assert int(mask.sum()) == 0
    comp.set_visible(1, False)
    assert mask[40:65].eq(1).all() and int(mask.sum()) == 25 and not comp.extra_scene_info_dict[1].visible
    assert int(comp.bake().point_invalid_mask.sum()) == 25
    comp.set_visible(1, True)
    assert int(mask.sum()) == 0 and comp.extra_scene_info_dict[1].visible
    q_cam = torch.tensor([[0.1, -0.2, 0.05, 0.97]])
    q_cam = q_cam / q_cam.norm()
    t_cam = torch.tensor([[0.3, 0.1, -2.0]])
    q_rows, t_rows = comp.camera_rows(q_cam, t_cam)
    assert q_rows.shape == (3, 4) and t_rows.shape == (3, 3) and q_rows.device.type == "cuda" and q_rows.dtype == torch.float32
    assert torch.equal(q_rows.cpu(), q_cam.expand(3, 4)) and torch.equal(t_rows.cpu(), t_cam.expand(3, 3))    # identity: the pose itself
    placements = [R.random_placement(60 + k) for k in range(3)]
    for k, p in enumerate(placements):
        comp.place(k, *p)
    q_rows, t_rows = comp.camera_rows(q_cam, t_cam)
    cam = (q_cam[0].double().numpy(), t_cam[0].double().numpy(), 1.0)
    for k, p in enumerate(placements):
        want_q, want_t, _ = R.compose(R.inverse(p), cam)
        assert np.abs(q_rows[k].cpu().numpy() - want_q).max() < 1e-6 and np.abs(t_rows[k].cpu().numpy() - want_t).max() < 1e-5
    many_q, many_t = comp.camera_rows(q_cam.expand(4, 4), t_cam.expand(4, 3))
    assert many_q.shape == (4, 3, 4) and torch.equal(many_q[2], q_rows) and torch.equal(many_t[3], t_rows)
    comp.place(2, placements[2][0], placements[2][1], 2.5)
    with pytest.raises(ValueError, match="bake"):
        comp.camera_rows(q_cam, t_cam)


@functools.lru_cache(maxsize=None)
def _rasteriser():
    return U.module()


def _render(scene, q, t, info):
    inp = U.Rast.GaussianPointCloudRasterisationInput(
        point_cloud=scene.point_cloud.detach(), point_cloud_features=scene.point_cloud_features.detach(),
        point_object_id=scene.point_object_id, point_invalid_mask=scene.point_invalid_mask, camera_info=info,
        q_pointcloud_camera=q, t_pointcloud_camera=t, color_max_sh_band=3)
    with torch.no_grad():
        image, _, count = _rasteriser()(inp)
    return image.cpu().numpy(), count.cpu().numpy()


@pytest.mark.parametrize("seed,n,sigma0,width", R.EQUIVALENCE_CASES)
def test_composition_under_its_pose_rows_equals_its_bake_under_the_pose(seed, n, sigma0, width):
    """the frames of the CPU test through the real rasteriser: rast(composition, camera_rows(T)) against rast(bake(), T)"""
    scene, q, t, placements = R.equivalence_case(seed, n, sigma0, width)
    sources = [(scene.point_cloud[scene.point_object_id == k], scene.point_cloud_features[scene.point_object_id == k]) for k in range(3)]
    comp = compose.SceneComposition(sources, device=DEV)
    for k, p in enumerate(placements):
        comp.place(k, *p)
    info = CameraInfo(torch.tensor(scene.camera_intrinsics, device=DEV), scene.height, scene.width, 0)
    q_cam, t_cam = torch.from_numpy(q[:1]).to(DEV), torch.from_numpy(t[:1]).to(DEV)
    q_rows, t_rows = comp.camera_rows(q_cam, t_cam)
    assert np.abs(q_rows.cpu().numpy() - q).max() < 1e-6 and np.abs(t_rows.cpu().numpy() - t).max() < 1e-6      # A_k^-1 o T_0 = T_k
    image_rows, count_rows = _render(comp.scene, q_rows, t_rows, info)
    image_baked, count_baked = _render(comp.bake(), q_cam, t_cam, info)
    assert count_rows.max() > 0
    R.assert_same_picture(image_baked, count_baked, image_rows, count_rows, report=f"rasteriser {seed}:")
