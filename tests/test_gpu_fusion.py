"""GPU: TSDF fusion and the isosurface (k_fusion.hip through fusion.py) against the numpy restatement of the header
(tests/fusion_ref.py): the fused volumes bit for bit on every voxel, the mesh's vertices and colours bit for bit and its faces
exactly; then the renderer's fuse() end to end on a small scene.

The isosurface's prefix sums have three levels: the 64 lanes of a wave, the 4 waves of a block of 256 voxels, and the block
sums, which one block scans 256 at a time with a carry between rounds.  5x4x3 (60 voxels) stays inside one wave, 9x8x7 (504)
takes two blocks, and 48x40x36 = 69 120 voxels are 270 blocks: the block-sum scan runs a second round, with a carry."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fusion_ref as R
from taichi_3d_gaussian_splatting_amd import CameraInfo, fusion, mixture, scene_io
from taichi_3d_gaussian_splatting_amd.GaussianPointRenderer import GaussianPointRenderer
from taichi_3d_gaussian_splatting_amd.utils import SE3_to_quaternion_and_translation_torch, quaternion_to_rotation_matrix_torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOLUMES = {(9, 7, 5): ((-0.4, -0.3, -0.2), (0.1, 0.1, 0.1)), (37, 21, 13): ((-0.9, -0.5, -0.3), (0.05, 0.05, 0.05))}
PARAMS = dict(trunc=0.2, max_weight=8.0, min_alpha=0.5, near=0.1)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _gpu_integrate(volume, views, split=None):
    """the views through TSDFVolume.integrate: in one call, or `split` views per call"""
    info = lambda v: CameraInfo(torch.tensor([[v["fx"], 0, v["cx"]], [0, v["fy"], v["cy"]], [0, 0, 1]], dtype=torch.float32), *v["depth"].shape, 0)
    step = split or max(len(views), 1)
    for first in range(0, len(views), step):
        part = views[first:first + step]
        volume.integrate([_dev(v["depth"]) for v in part], [v["q"] for v in part], [v["t"] for v in part], [info(v) for v in part],
                         alpha=[_dev(v["alpha"]) for v in part], image=[_dev(v["image"]) for v in part])
    return volume


def _volume(dims, colour=True, **over):
    origin, voxel = VOLUMES[dims]
    return fusion.TSDFVolume(origin=origin, dims=dims, voxel=voxel, colour=colour, device=DEV, **dict(PARAMS, **over))


def _reference(dims, views, colour=True, stats=None, **over):
    origin, voxel = VOLUMES[dims]
    p = dict(PARAMS, **over)
    tsdf, weight, col = R.new_volume(dims, colour)
    R.integrate(tsdf, weight, col, views, origin, voxel, p["trunc"], p["max_weight"], p["min_alpha"], p["near"], stats=stats)
    return tsdf, weight, col


def _assert_same_volume(volume, want):
    for name, ref in zip(("tsdf", "weight", "colour"), want):
        got = getattr(volume, name)
        assert (got is None) == (ref is None), name
        if ref is not None:
            got = got.cpu().numpy()
            assert got.dtype == np.float32 and got.shape == ref.shape, name
            assert got.tobytes() == ref.tobytes(), f"{name}: {(got != ref).sum()} of {ref.size} values differ"


@functools.lru_cache(maxsize=None)
def _views(dims, size, n, seed=0):
    origin, voxel = VOLUMES[dims]
    return R.ring_of_views(n, dims, origin, voxel, size[0], size[1], 60.0 if dims[0] > 9 else 90.0, np.random.default_rng(seed), plane_z=2.6)


@pytest.mark.parametrize("n_views", [1, 3, fusion.VIEWS_PER_LAUNCH + 1])
@pytest.mark.parametrize("size", [(32, 48), (35, 50)])
@pytest.mark.parametrize("dims", list(VOLUMES))
def test_integrate_equals_the_restatement_on_every_voxel(dims, size, n_views):
    views = _views(dims, size, n_views)
    stats = []
    want = _reference(dims, views, stats=stats)
    _assert_same_volume(_gpu_integrate(_volume(dims), views), want)
    total = {k: sum(s[k] for s in stats) for k in stats[0]}
    assert total["updated"] > 0 and total["no_depth"] > 0 and total["low_alpha"] > 0 and total["at_min_alpha"] > 0 and total["far_behind"] > 0, total
    if dims == (37, 21, 13) and n_views > 1:                # the large volume overflows the image on every side
        assert min(total[k] for k in ("left", "right", "above", "below")) > 0, total


@pytest.mark.parametrize("size", [(32, 48), (35, 50)])
def test_integrate_under_a_camera_whose_four_numbers_differ(size):
    """fy = 0.6 fx, cx = 0.4 w, cy = 0.65 h (the ring's other views have fx = fy and the principal point in the middle, so an
    integration that took one of the four for another would pass them): the smallest volume, three views, every voxel bit for
    bit.  The restatement itself gives another volume with fx and fy exchanged, and with cx and cy exchanged."""
    dims, (h, w) = (9, 7, 5), size
    origin, voxel = VOLUMES[dims]
    views = R.ring_of_views(3, dims, origin, voxel, h, w, (90.0, 54.0), np.random.default_rng(0), plane_z=2.6, principal=(0.4 * w, 0.65 * h))
    assert len({float(views[0][k]) for k in ("fx", "fy", "cx", "cy")}) == 4
    stats = []
    want = _reference(dims, views, stats=stats)
    for a, b in (("fx", "fy"), ("cx", "cy")):
        exchanged = _reference(dims, [dict(v, **{a: v[b], b: v[a]}) for v in views])
        assert not np.array_equal(exchanged[0], want[0]) and not np.array_equal(exchanged[1], want[1]), (a, b)
    _assert_same_volume(_gpu_integrate(_volume(dims), views), want)
    total = {k: sum(s[k] for s in stats) for k in stats[0]}
    assert total["updated"] > 0 and total["no_depth"] > 0 and total["low_alpha"] > 0 and total["at_min_alpha"] > 0 and total["far_behind"] > 0, total


def test_a_camera_with_the_volume_behind_it_changes_nothing():
    dims = (9, 7, 5)
    rng = np.random.default_rng(2)
    away = R.synthetic_view((0.0, 0.0, -2.0), (0.0, 0.0, -4.0), 32, 48, 60.0, (0, 0, 0), 0.3, rng, plane_z=1.0)
    stats = []
    want = _reference(dims, [away], stats=stats)
    assert stats[0]["behind"] == 9 * 7 * 5 and stats[0]["updated"] == 0
    volume = _gpu_integrate(_volume(dims), [away])
    _assert_same_volume(volume, want)
    assert float(volume.weight.max()) == 0.0 and float(volume.tsdf.min()) == 1.0


def test_weights_stop_at_max_weight():
    dims = (37, 21, 13)
    views = _views(dims, (32, 48), 3, seed=5)
    views = [dict(v, alpha=None) for v in views[:1]] * 3            # the same view three times: every voxel it reaches gets three updates
    want = _reference(dims, views, max_weight=2.0)
    assert want[1].max() == 2.0 and (want[1] == 2.0).sum() > 100
    _assert_same_volume(_gpu_integrate(_volume(dims, max_weight=2.0), views), want)


def test_colour_needs_both_the_volume_and_the_image():
    dims = (9, 7, 5)
    views = _views(dims, (35, 50), 3)
    _assert_same_volume(_gpu_integrate(_volume(dims, colour=False), views), _reference(dims, views, colour=False))
    mixed = [dict(v, image=None) if i == 1 else v for i, v in enumerate(views)]     # the middle view brings no image
    want = _reference(dims, mixed)
    assert not np.array_equal(want[2], _reference(dims, views)[2])
    _assert_same_volume(_gpu_integrate(_volume(dims), mixed), want)


def test_two_calls_of_one_view_equal_one_call_of_two():
    dims = (37, 21, 13)
    views = _views(dims, (32, 48), 3)[:2]
    together, apart = _gpu_integrate(_volume(dims), views), _gpu_integrate(_volume(dims), views, split=1)
    for name in ("tsdf", "weight", "colour"):
        assert torch.equal(getattr(together, name), getattr(apart, name)), name
    _assert_same_volume(apart, _reference(dims, views))


def test_empty_volume_and_no_views():
    volume = fusion.TSDFVolume(origin=(0, 0, 0), dims=(4, 0, 3), voxel=0.1, device=DEV)
    view = _views((9, 7, 5), (32, 48), 1)
    _gpu_integrate(volume, view)
    assert volume.tsdf.shape == (4, 0, 3) and volume.extract_mesh().vertices.shape == (0, 3)
    untouched = _volume((9, 7, 5)).integrate([], [], [], [])
    assert float(untouched.weight.max()) == 0.0


# ---- the isosurface ------------------------------------------------------------------------------------------------------
def _smooth(dims, seed):
    """a few random waves over the grid: a smooth volume that crosses 0 in many cells"""
    rng = np.random.default_rng(seed)
    x, y, z = np.meshgrid(*[np.arange(d, dtype=np.float64) for d in dims], indexing="ij")
    out = np.zeros(dims)
    for _ in range(4):
        k = rng.uniform(-1.2, 1.2, 3)
        out += rng.uniform(0.5, 1.0) * np.sin(k[0] * x + k[1] * y + k[2] * z + rng.uniform(0, 6.28))
    return out.astype(np.float32)


def _assert_same_mesh(mesh, want):
    vertices, faces, colours = want
    assert mesh.vertices.dtype == torch.float32 and mesh.faces.dtype == torch.int32
    assert tuple(mesh.vertices.shape) == vertices.shape and tuple(mesh.faces.shape) == faces.shape
    assert mesh.vertices.cpu().numpy().tobytes() == vertices.tobytes()
    assert np.array_equal(mesh.faces.cpu().numpy(), faces)
    assert (mesh.colours is None) == (colours is None)
    if colours is not None:
        assert mesh.colours.cpu().numpy().tobytes() == colours.tobytes()


ISO_CASES = {
    "one_wave": dict(dims=(5, 4, 3), seed=1),
    "one_wave_with_holes": dict(dims=(5, 4, 3), seed=2, holes=True, colour=True),
    "two_blocks": dict(dims=(9, 8, 7), seed=3, colour=True),
    "two_blocks_with_holes_flipped": dict(dims=(9, 8, 7), seed=4, holes=True, flip=True),
    "second_round_of_the_block_scan": dict(dims=(48, 40, 36), seed=5, colour=True),
    "second_round_with_holes": dict(dims=(48, 40, 36), seed=6, holes=True, level=0.25),
    "values_equal_to_the_level": dict(dims=(9, 8, 7), seed=7, snap=True),
    "nothing_crosses": dict(dims=(9, 8, 7), seed=8, level=100.0, colour=True),
    "a_dimension_of_one": dict(dims=(9, 1, 7), seed=9),
    "a_dimension_of_zero": dict(dims=(9, 8, 0), seed=10, colour=True),
}


@pytest.mark.parametrize("case", list(ISO_CASES))
def test_isosurface_equals_the_restatement(case):
    c = ISO_CASES[case]
    dims, rng = c["dims"], np.random.default_rng(c["seed"])
    values = _smooth(dims, c["seed"])
    level = c.get("level", 0.0)
    if c.get("snap") and values.size:                       # a quarter of the corners exactly at the level, and a NaN and an inf elsewhere
        values[rng.uniform(size=dims) < 0.25] = level
        values[1, 2, 3], values[6, 5, 2] = np.nan, np.inf
    valid = None
    if c.get("holes"):
        valid = np.where(rng.uniform(size=dims) < 0.04, rng.choice(np.array([0.0, -1.0, np.nan], np.float32), size=dims), 1.0).astype(np.float32)
    colour = rng.uniform(0, 1, dims + (3,)).astype(np.float32) if c.get("colour") else None
    origin, spacing = (0.3, -1.0, 2.0), (0.11, 0.07, 0.05)
    want = R.isosurface(values, origin, spacing, level, valid=valid, colour=colour, flip=c.get("flip", False))
    if case in ("nothing_crosses", "a_dimension_of_one", "a_dimension_of_zero"):
        assert want[0].shape == want[1].shape == (0, 3)
    else:
        assert len(want[0]) > 0 and len(want[1]) > 0
    if case.startswith("second_round"):
        assert values.size > fusion.ISO_BLOCK * fusion.ISO_BLOCK
    mesh = fusion.isosurface(_dev(values), origin, spacing, level, valid=_dev(valid), colour=_dev(colour), flip=c.get("flip", False))
    _assert_same_mesh(mesh, want)


@pytest.mark.parametrize("flip", [False, True])
def test_sphere_invariants_on_the_kernels_own_mesh(flip):
    values, origin, spacing = R.sphere_values(20)
    mesh = fusion.isosurface(_dev(values), origin, spacing, 0.0, flip=flip)
    V, F, _, _ = R.check_sphere_mesh(mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), 20, flip)
    assert (V, F) == (1928, 3852)


# ---- end to end ----------------------------------------------------------------------------------------------------------
H, W, FOCAL, G, SIGMA = 48, 64, 60.0, 24, 0.05
BOX = np.array([[-0.7, -0.7, -0.7], [0.7, 0.7, 0.7]])


@pytest.fixture(scope="module")
def renderer(tmp_path_factory):
    """3000 small opaque Gaussians on a sphere of radius 0.5 around the origin, six cameras around it at distance 2"""
    rng = np.random.default_rng(0)
    n = 3000
    p = rng.normal(size=(n, 3))
    p = 0.5 * p / np.linalg.norm(p, axis=1, keepdims=True)
    features = np.zeros((n, 56), np.float32)
    features[:, 3] = 1.0
    features[:, 4:7] = np.log(SIGMA)
    features[:, 7] = 6.0
    features[:, 8::16] = rng.uniform(0.0, 1.5, (n, 3)) / 0.2820948
    path = tmp_path_factory.mktemp("fusion") / "sphere.parquet"
    scene_io.save_parquet(str(path), p.astype(np.float32), features)
    cameras = torch.zeros(6, 4, 4)
    for i, eye in enumerate(((0, 0, -2), (2, 0.3, 0), (0, -0.3, 2), (-2, 0.2, 0.4), (0.5, -1.9, 0.3), (0.4, 1.9, -0.3))):
        q, t = R.look_at_pose(eye, (0, 0, 0), up=(0.0, -1.0, 0.0) if abs(eye[1]) < 1 else (0.0, 0.0, 1.0))
        cameras[i, :3, :3] = quaternion_to_rotation_matrix_torch(torch.tensor(q, dtype=torch.float64)).float()
        cameras[i, :3, 3] = torch.tensor(t)
        cameras[i, 3, 3] = 1.0
    config = GaussianPointRenderer.GaussianPointRendererConfig(str(path), cameras, device=DEV, image_height=H, image_width=W,
                                                               camera_intrinsics=torch.tensor([[FOCAL, 0, W / 2], [0, FOCAL, H / 2], [0, 0, 1.0]]))
    return GaussianPointRenderer(config)


def _fused(renderer):
    return renderer.fuse(fusion.TSDFVolume(bbox=BOX, dims=G, near=0.8, device=DEV))


def test_fuse_equals_the_restatement_fed_the_same_frames(renderer):
    volume = _fused(renderer)
    q_rows, t_rows = renderer.pose_rows()
    q_world, t_world = SE3_to_quaternion_and_translation_torch(renderer.config.cameras.detach().to(device="cpu", dtype=torch.float32))
    views = []
    for i in range(q_rows.shape[0]):
        image, depth, alpha = renderer.render(q_rows[i], t_rows[i], depth=True, alpha=True)
        views.append(dict(depth=depth.cpu().numpy(), alpha=alpha.cpu().numpy(), image=image.cpu().numpy(), m=R.world_to_camera(q_world[i].numpy(), t_world[i].numpy()),
                          fx=np.float32(FOCAL), fy=np.float32(FOCAL), cx=np.float32(W / 2), cy=np.float32(H / 2)))
        assert float(alpha.max()) > 0.9 and float(depth.max()) > 1.0
    tsdf, weight, colour = R.new_volume((G, G, G))
    stats = []
    R.integrate(tsdf, weight, colour, views, volume.origin, volume.voxel, volume.trunc, volume.max_weight, volume.min_alpha, volume.near, stats=stats)
    assert all(s["updated"] > 0 for s in stats) and (tsdf < 0).any() and (weight > 0).any()
    _assert_same_volume(volume, (tsdf, weight, colour))
    mesh = volume.extract_mesh()
    V, F = mesh.vertices.shape[0], mesh.faces.shape[0]
    assert V > 100 and F > 100 and mesh.colours.shape == (V, 3)
    faces = mesh.faces.cpu().numpy()
    assert faces.min() >= 0 and faces.max() < V
    _assert_same_mesh(mesh, R.isosurface(tsdf, volume.origin, volume.voxel, 0.0, valid=weight, colour=colour))
    # The mesh is the sphere of Gaussians: a vertex lies on a grid edge (at most sqrt(3) voxels long) that crosses the surface the
    # depth frames saw, and a pixel with accumulated alpha >= 1/2 looks at Gaussians within 4 sigma of their centres (beyond, one
    # contributes less than 4e-4), which lie at radius 0.5.
    slack = 4 * SIGMA + np.sqrt(3.0) * max(volume.voxel)
    radius = mesh.vertices.norm(dim=1)
    assert 0.5 - slack < float(radius.min()) and float(radius.max()) < 0.5 + slack


def test_fusing_twice_gives_identical_bytes(renderer):
    a, b = _fused(renderer), _fused(renderer)
    for name in ("tsdf", "weight", "colour"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    ma, mb = a.extract_mesh(), b.extract_mesh()
    assert torch.equal(ma.vertices, mb.vertices) and torch.equal(ma.faces, mb.faces) and torch.equal(ma.colours, mb.colours)


def test_isosurface_of_density_is_a_closed_mesh(renderer):
    with torch.no_grad():
        peak = float(mixture.density_volume(renderer.scene, G).max())
    mesh = fusion.isosurface_of_density(renderer.scene, G, 0.25 * peak)
    faces = mesh.faces.cpu().numpy()
    assert len(faces) > 100 and faces.max() < mesh.vertices.shape[0] and mesh.colours is None
    closed, _, _, _ = R.edge_report(faces)
    assert closed
    assert R.signed_volume(mesh.vertices.cpu().numpy(), faces) > 0          # flip: faces look out of the dense side
    again = fusion.isosurface_of_density(renderer.scene, G, 0.25 * peak)
    assert torch.equal(mesh.vertices, again.vertices) and torch.equal(mesh.faces, again.faces)


def test_cli_mesh_to_writes_the_mesh_that_fuse_gives(renderer, tmp_path):
    """gaussian_point_render.py --mesh_to in a child, without --output_prefix: the PLY, read back with numpy, holds the V vertices,
    colours and F faces of the same fusion in this process"""
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaussian_point_render.py")
    poses, out = tmp_path / "poses.pt", tmp_path / "out.ply"
    torch.save(renderer.config.cameras, str(poses))
    voxel = 0.0625
    args = ["--device", DEV, "--parquet_path", renderer.config.parquet_path, "--poses", poses, "--mesh_to", out, "--image_height", H,
            "--image_width", W, "--camera_intrinsics", FOCAL, FOCAL, W / 2, H / 2, "--mesh_voxel", voxel, "--mesh_bbox", *BOX.ravel()]
    p = subprocess.run([sys.executable, script] + [str(a) for a in args], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert sorted(f.name for f in tmp_path.iterdir()) == ["out.ply", "poses.pt"]             # no frames without --output_prefix
    volume = renderer.fuse(fusion.TSDFVolume(bbox=BOX, voxel=voxel, device=DEV))
    assert volume.dims == (24, 24, 24) and volume.trunc == fusion.TRUNC_VOXELS * voxel
    mesh = volume.extract_mesh()
    V, F = mesh.vertices.shape[0], mesh.faces.shape[0]
    report = json.loads(p.stdout.strip().splitlines()[-1])
    assert (report["vertices"], report["faces"], report["dims"]) == (V, F, [24, 24, 24]) and V > 100 and F > 100
    data = out.read_bytes()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").splitlines()
    assert f"element vertex {V}" in header and f"element face {F}" in header
    vertex_dtype = np.dtype([("xyz", "<f4", (3,)), ("rgb", "u1", (3,))])
    face_dtype = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    assert len(data) == end + V * vertex_dtype.itemsize + F * face_dtype.itemsize
    got_v = np.frombuffer(data, vertex_dtype, V, end)
    got_f = np.frombuffer(data, face_dtype, F, end + V * vertex_dtype.itemsize)
    assert got_v["xyz"].tobytes() == mesh.vertices.cpu().numpy().tobytes()
    assert (got_f["n"] == 3).all() and np.array_equal(got_f["v"], mesh.faces.cpu().numpy())
    want_rgb = torch.clamp(mesh.colours * 255, 0, 255).byte().cpu().numpy()               # the frames' RGB_TRUNC rule
    assert np.array_equal(got_v["rgb"], want_rgb) and want_rgb.max() > 0
