"""CPU: the numpy restatement of include/gs_fusion.h (tests/fusion_ref.py) checked against what it must satisfy on its own --
the sphere's mesh is closed, oriented, of genus 0 and within the interpolation bound of the sphere; holes give a boundary and
nothing worse; the f32 integration agrees with the same rule in float64 wherever no decision can flip -- and the PLY writer."""
import numpy as np
import pytest
import torch

import fusion_ref as R

# V and F of the sphere's mesh at both sizes, counted once by this restatement; a change of the rule shows here first
SPHERE_COUNTS = {12: (656, 1308), 20: (1928, 3852)}


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("G", [12, 20])
def test_sphere_mesh_is_closed_oriented_and_near_the_sphere(G, flip):
    values, origin, spacing = R.sphere_values(G)
    vertices, faces, colours = R.isosurface(values, origin, spacing, 0.0, flip=flip)
    assert colours is None and vertices.dtype == np.float32 and faces.dtype == np.int32
    V, F, worst, bound = R.check_sphere_mesh(vertices, faces, G, flip)
    assert (V, F) == SPHERE_COUNTS[G]
    print(f"G={G} flip={flip}: V={V} F={F} worst={worst:.4f} bound={bound:.4f}")


def test_flip_reverses_every_triangle_and_nothing_else():
    values, origin, spacing = R.sphere_values(12)
    v0, f0, _ = R.isosurface(values, origin, spacing, 0.0)
    v1, f1, _ = R.isosurface(values, origin, spacing, 0.0, flip=True)
    assert v0.tobytes() == v1.tobytes() and np.array_equal(f0[:, [0, 2, 1]], f1)


def test_holes_give_a_boundary_and_no_unreferenced_vertex():
    G = 12
    values, origin, spacing = R.sphere_values(G)
    valid = np.ones_like(values)
    valid[5:8, 2:7, 4:9] = 0.0                                      # a block of corners that cuts the surface
    valid[0, 0, 0] = -1.0
    values = values.copy()
    values[9, 9, 3] = np.nan                                        # and a corner that is invalid by its value
    vertices, faces, _ = R.isosurface(values, origin, spacing, 0.0, valid=valid)
    whole = R.isosurface(R.sphere_values(G)[0], origin, spacing, 0.0)
    assert 0 < len(faces) < len(whole[1]) and 0 < len(vertices) < len(whole[0])
    closed, most_directed, most_undirected, _ = R.edge_report(faces)
    assert not closed and most_directed == 1 and most_undirected == 2       # once or twice, never twice in one direction
    edges = np.sort(R.directed_edges(faces), axis=1)
    _, counts = np.unique(edges[:, 0] * (edges.max() + 1) + edges[:, 1], return_counts=True)
    assert (counts == 1).any()                                      # there is a boundary
    assert len(np.unique(faces)) == len(vertices) and faces.max() == len(vertices) - 1
    assert np.isfinite(vertices).all()


def test_degenerate_volumes_have_no_mesh():
    for dims in ((0, 4, 4), (1, 5, 5), (5, 1, 5), (5, 5, 1)):
        v, f, c = R.isosurface(np.zeros(dims, np.float32) - 1, (0, 0, 0), (1, 1, 1), 0.0, colour=np.zeros(dims + (3,), np.float32))
        assert v.shape == f.shape == c.shape == (0, 3)
    v, f, _ = R.isosurface(np.ones((4, 4, 4), np.float32), (0, 0, 0), (1, 1, 1), 0.0)        # no crossing
    assert v.shape == f.shape == (0, 3)


def test_colour_is_interpolated_with_the_vertex():
    values, origin, spacing = R.sphere_values(12)
    x, y, z = np.broadcast_arrays(*R.voxel_positions(values.shape, origin, spacing))
    colour = np.stack([x, y, z], -1).astype(np.float32)             # the position as the colour: the two must agree
    vertices, _, colours = R.isosurface(values, origin, spacing, 0.0, colour=colour)
    assert np.abs(vertices - colours).max() < 1e-6


@pytest.mark.parametrize("seed,dims", [(0, (37, 21, 13)), (1, (26, 19, 11)), (4, (37, 21, 13))])
def test_f32_integration_agrees_with_float64_where_no_decision_can_flip(seed, dims):
    """Excluded: voxels with u or v within 1e-3 of an integer, z within 1e-6 of near, or sdf + trunc within 1e-5 trunc of 0 in some
    view -- at most 2 % of the volume (the pixel-edge band alone is about 2 * 2e-3 per view).  Everywhere else within 1e-5."""
    rng = np.random.default_rng(seed)
    origin, voxel = (-0.9, -0.5, -0.3), (0.05, 0.05, 0.05)
    if dims == (26, 19, 11):                                        # another lattice, off the cameras' axes
        origin, voxel = (-0.83, -0.61, -0.37), (0.07, 0.06, 0.065)
    views = R.ring_of_views(3, dims, origin, voxel, 32, 48, 60.0, rng, plane_z=2.6)
    got = {}
    for dtype in (np.float32, np.float64):
        tsdf, weight, colour = R.new_volume(dims, dtype=dtype)
        fragile = np.zeros(dims, bool)
        R.integrate(tsdf, weight, colour, views, origin, voxel, 0.2, 8.0, 0.5, 0.1, dtype=dtype, fragile=fragile)
        got[dtype] = (tsdf, weight, colour, fragile)
    fragile = got[np.float32][3] | got[np.float64][3]
    share = fragile.mean()
    print(f"seed {seed}: {share:.4f} of the voxels excluded")
    assert share <= 0.02
    assert (got[np.float64][1] > 0).mean() > 0.5                    # the views do reach the volume
    for a, b in zip(got[np.float32][:3], got[np.float64][:3]):
        assert a.dtype == np.float32
        assert np.abs(a.astype(np.float64) - b)[~fragile].max() <= 1e-5


def test_integration_rule_by_hand_on_one_voxel():
    """one voxel, two views looking down +z from the origin: the running mean, the weight cap and the skips, worked by hand"""
    m = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)
    view = lambda d, alpha=None: dict(m=m, fx=np.float32(10), fy=np.float32(10), cx=np.float32(2), cy=np.float32(2),
                                      depth=np.full((4, 4), d, np.float32), alpha=None if alpha is None else np.full((4, 4), alpha, np.float32),
                                      image=np.full((4, 4, 3), d, np.float32))
    tsdf, weight, colour = R.new_volume((1, 1, 1))
    args = ((0.0, 0.0, 1.0), (0.1, 0.1, 0.1), 0.5, 2.0, 0.5, 0.1)              # the voxel at z = 1; trunc .5, max_weight 2
    R.integrate(tsdf, weight, colour, [view(1.25)], *args)
    assert tsdf[0, 0, 0] == np.float32(0.5) and weight[0, 0, 0] == 1 and colour[0, 0, 0, 0] == np.float32(1.25)
    R.integrate(tsdf, weight, colour, [view(2.0)], *args)                       # sdf 1 -> clamped to 1: mean of .5 and 1
    assert tsdf[0, 0, 0] == np.float32(0.75) and weight[0, 0, 0] == 2
    R.integrate(tsdf, weight, colour, [view(1.0)], *args)                       # weight stays at the cap: (2 * .75 + 0) / 3
    assert tsdf[0, 0, 0] == np.float32(0.5) and weight[0, 0, 0] == 2
    before = tsdf.copy()
    for skipped in (view(0.4), view(0.0), view(-1.0), view(np.nan), view(np.inf), view(1.0, alpha=0.25)):
        R.integrate(tsdf, weight, colour, [skipped], *args)                     # behind the surface by more than trunc, no depth, low alpha
    assert np.array_equal(tsdf, before) and weight[0, 0, 0] == 2
    R.integrate(tsdf, weight, colour, [view(0.5), view(1.0, alpha=0.5)], *args)  # sdf = -trunc exactly, and alpha at min_alpha: both count
    assert tsdf[0, 0, 0] == np.float32((np.float32((2 * 0.5 - 1) / 3) * 2 + 0) / 3)


def test_a_camera_with_skew_is_refused():
    """fusion._intrinsics hands fx, fy, cx, cy to the library; the rasteriser that rendered the depth multiplies by the whole
    matrix, so a K[0,1] or K[1,0] that is not zero must not be dropped silently"""
    from taichi_3d_gaussian_splatting_amd import CameraInfo, fusion
    K = np.array([[57.6, 0, 19.84], [0, 28.8, 34.56], [0, 0, 1]], np.float32)
    for make in (torch.tensor, np.array):
        assert fusion._intrinsics(CameraInfo(make(K), 48, 64, 0)) == tuple(float(x) for x in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
        for entry in ((0, 1), (1, 0)):
            bad = K.copy()
            bad[entry] = 0.5
            with pytest.raises(ValueError, match="fx, fy, cx, cy only"):
                fusion._intrinsics(CameraInfo(make(bad), 48, 64, 0))


@pytest.mark.parametrize("with_colours", [True, False])
def test_ply_round_trip(tmp_path, with_colours):
    from taichi_3d_gaussian_splatting_amd import fusion
    values, origin, spacing = R.sphere_values(12)
    vertices, faces, _ = R.isosurface(values, origin, spacing, 0.0)
    rng = np.random.default_rng(0)
    colours = rng.uniform(-0.2, 1.2, vertices.shape).astype(np.float32)
    colours[0] = (np.nan, np.inf, -np.inf)
    mesh = fusion.Mesh(torch.from_numpy(vertices), torch.from_numpy(faces), torch.from_numpy(colours) if with_colours else None)
    path = tmp_path / "mesh.ply"
    mesh.to_ply(str(path))
    data = path.read_bytes()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").splitlines()
    assert header[:2] == ["ply", "format binary_little_endian 1.0"]
    assert f"element vertex {len(vertices)}" in header and f"element face {len(faces)}" in header
    assert ("property uchar red" in header) == with_colours
    vertex_dtype = np.dtype([("xyz", "<f4", (3,))] + ([("rgb", "u1", (3,))] if with_colours else []))
    face_dtype = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    assert len(data) == end + len(vertices) * vertex_dtype.itemsize + len(faces) * face_dtype.itemsize
    got_v = np.frombuffer(data, vertex_dtype, len(vertices), end)
    got_f = np.frombuffer(data, face_dtype, len(faces), end + len(vertices) * vertex_dtype.itemsize)
    assert got_v["xyz"].tobytes() == vertices.tobytes()
    assert (got_f["n"] == 3).all() and np.array_equal(got_f["v"], faces)
    if with_colours:
        with np.errstate(invalid="ignore"):
            want = np.clip(np.nan_to_num(colours * np.float32(255), nan=0.0, posinf=255.0, neginf=0.0), 0, 255).astype(np.uint8)
        assert np.array_equal(got_v["rgb"], want) and tuple(got_v["rgb"][0]) == (0, 255, 0)
