"""CPU: the references and the cases of tests/camera_cases.py, before any GPU run.

The oracle and the float64 restatement agree under every camera at the bars of test_oracle_autograd; every camera, on every
scene that test_gpu_cameras.py compares with the oracle, moves the oracle's image and position gradient far beyond the GPU
tests' bars when it is replaced by one a wrong kernel would effectively be using; the planes remove points on both sides; and
the oracle's frame test gives the stated pattern on the points that sit on its edges.  These are conditions on the inputs, not
measurements of the kernels: a case that could hide a wrong kernel fails here first."""
import dataclasses

import numpy as np
import pytest

import camera_cases as CC
import parity_util as P
from oracle import oracle

TINY = [(0, 48, 0.25, 32, 32), (3, 56, 0.5, 41, 27)]


@pytest.mark.parametrize("arg", TINY, ids=["32x32", "41x27"])
@pytest.mark.parametrize("camera", list(CC.CAMERAS))
def test_references_agree_under_every_camera(camera, arg):
    """test_oracle_autograd.test_backward_matches_autograd's comparison and bars (2e-5 absolute on the image, 2e-4 of the
    tensor maximum per group)"""
    s, q, t, partial = P.tiny_case(*arg)
    s = CC.with_camera(s, camera)
    errors = P.assert_oracle_matches_autograd(s, q, t, P.random_target(s, arg[0] + 100), partial)
    print(f"{camera} {s.width}x{s.height}: " + ", ".join(f"{k} {v:.3g}" for k, v in errors.items()))


def _movement_scenes():
    """name -> (scene under the synthetic camera, q, t, oracle config keywords): the scenes of test_gpu_cameras.py that are
    compared with the oracle, and the two tiny ones of its float64 comparisons"""
    q, t = P.tiny_pose()
    out = {}
    for name in CC.ORACLE_SCENES:
        s, partial = CC.oracle_scene(name)
        out[name] = (s, q, t, dict(partial=partial))
    s, partial = CC.planes_scene()
    out["planes"] = (s, q, t, dict(partial=partial, **CC.PLANES))
    for arg in TINY:
        s, tq, tt, partial = P.tiny_case(*arg)
        out[f"tiny{arg[3]}x{arg[4]}"] = (s, tq, tt, dict(partial=partial))
    return out


MOVEMENT_SCENES = ["250x203", "96x64", "planes", "tiny32x32", "tiny41x27"]


def _movement(s, q, t, kw):
    """[(entry of confusable, movement of the image, movement of grad_pointcloud)] for the scene's camera, under one upstream"""
    cfg = P.oracle_config(**kw)
    f, _ = P.run_oracle(s, q, t, cfg)
    assert f.K > 0
    g = (2.0 * (f.rasterized_image - P.random_target(s, 5))).astype(np.float32)
    b = oracle.backward(f, g, 3, cfg)
    out = []
    for name, Kc in CC.confusable(s.camera_intrinsics):
        fc, _ = P.run_oracle(dataclasses.replace(s, camera_intrinsics=Kc), q, t, cfg)
        bc = oracle.backward(fc, g, 3, cfg)
        out.append((name, P.rel_err(fc.rasterized_image, f.rasterized_image), P.rel_err(bc["grad_pointcloud"], b["grad_pointcloud"])))
    return out


@pytest.mark.parametrize("scene", MOVEMENT_SCENES)
@pytest.mark.parametrize("camera", list(CC.CAMERAS))
def test_a_confusable_camera_moves_the_oracle_past_ten_times_the_bars(camera, scene):
    """With fx and fy exchanged, cx and cy exchanged, K[0,1] or K[1,0] dropped or the two exchanged, the oracle's image moves by
    more than 10 IMAGE_TOL and its grad_pointcloud by more than 10 GRAD_TOL (parity_util.rel_err), so a kernel with such an
    error cannot stay inside the bars of test_gpu_cameras.py.  A pair that misses this gets another scene, never another factor."""
    s, q, t, kw = _movement_scenes()[scene]
    s = CC.with_camera(s, camera)
    moved = _movement(s, q, t, kw)
    assert CC.CONFUSABLE_OF[camera] <= {name for name, _, _ in moved}, (camera, [name for name, _, _ in moved])
    for name, image, grad in moved:
        print(f"{camera} on {scene}, {name}: image moves {image:.3g} ({image / P.IMAGE_TOL:.3g} bars), grad_pointcloud {grad:.3g} "
              f"({grad / P.GRAD_TOL:.3g} bars)")
        assert image > 10 * P.IMAGE_TOL, (name, image)
        assert grad > 10 * P.GRAD_TOL, (name, grad)


def test_records_scene_under_general_k10_moves_too():
    """The staged case of test_gpu_cameras.py: records_scene() under general_k10 and view_pose()"""
    from taichi_3d_gaussian_splatting_amd.synthetic import view_pose
    s = CC.with_camera(P.records_scene(), "general_k10")
    moved = _movement(s, *view_pose(), dict(partial=False))
    assert len(moved) == 5
    for name, image, grad in moved:
        assert image > 10 * P.IMAGE_TOL and grad > 10 * P.GRAD_TOL, (name, image, grad)


def test_confusable_skips_what_equals_the_camera():
    synthetic = np.array([[19.2, 0, 16], [0, 19.2, 16], [0, 0, 1]], np.float32)
    assert CC.confusable(synthetic) == []
    assert [n for n, _ in CC.confusable(CC.CAMERAS["general_k10"](250, 203))] == ["fx_fy", "cx_cy", "k01_zero", "k10_zero", "k01_k10"]
    K = CC.CAMERAS["skew"](96, 64)
    got = dict(CC.confusable(K))
    assert set(got) == {"cx_cy", "k01_zero", "k01_k10"}
    assert got["k01_k10"][1, 0] == K[0, 1] and got["k01_k10"][0, 1] == 0 and got["k01_zero"][0, 1] == 0
    for name, Kc in got.items():
        assert Kc.dtype == np.float32 and not np.array_equal(Kc, K), name


def test_with_camera_replaces_the_intrinsics_only():
    s, _, _, _ = P.tiny_case(0, 48, 0.25, 32, 32)
    for name, make in CC.CAMERAS.items():
        c = CC.with_camera(s, name)
        assert c.camera_intrinsics.dtype == np.float32 and np.array_equal(c.camera_intrinsics, make(32, 32))
        assert not np.array_equal(c.camera_intrinsics, s.camera_intrinsics), name
        for field in ("point_cloud", "point_cloud_features", "point_invalid_mask", "point_object_id"):
            assert np.array_equal(getattr(c, field), getattr(s, field)), field
        assert (c.height, c.width) == (s.height, s.width)


@pytest.mark.parametrize("camera", [None] + list(CC.CAMERAS))
def test_planes_remove_points_on_both_sides(camera):
    """Under PLANES the oracle keeps fewer points than under the default planes: some lie at or below the near plane, some at or
    beyond the far one, and what is left still blends.  Under the synthetic camera and the pose of tiny_case: M = 2007 of 4000,
    565 at or below the near plane, 1428 at or beyond the far one."""
    s, partial = CC.planes_scene()
    if camera is not None:
        s = CC.with_camera(s, camera)
    q, t = P.tiny_pose()
    wide, _ = P.run_oracle(s, q, t, P.oracle_config(partial))
    f, _ = P.run_oracle(s, q, t, P.oracle_config(partial, **CC.PLANES))
    z = wide.point_in_camera[:, 2]
    below, above = int((z <= CC.PLANES["near_plane"]).sum()), int((z >= CC.PLANES["far_plane"]).sum())
    print(f"{camera}: M {f.M} of {wide.M} in frame, {below} at or below the near plane, {above} at or beyond the far plane, K {f.K}")
    assert below > 0 and above > 0 and f.K > 0
    assert f.M == wide.M - below - above < wide.M
    assert np.array_equal(f.point_id_in_camera_list, wide.point_id_in_camera_list[(z > 3.0) & (z < 7.0)])


def test_frame_edges_of_the_oracle_are_the_stated_pattern():
    s, q, t, cfg, expected, what = CC.frame_edge_case()
    f, _ = P.run_oracle(s, q, t, cfg)
    assert np.array_equal(f.point_in_camera_mask, expected), [w for w, a, b in zip(what, f.point_in_camera_mask, expected) if a != b]
    assert list(expected) == [1, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 1, 1, 1] and f.M == 8 and f.K > 0
    uv = dict(zip([w for w, e in zip(what, expected) if e], f.point_uv))
    W, H = s.width, s.height
    assert uv["u == -48"][0] == np.float32(-48.0) and uv["v == -48"][1] == np.float32(-48.0)
    assert uv["u == W + 48, one step across"][0] == np.nextafter(np.float32(W + 48), np.float32(0))
    assert uv["v == H + 48, one step across"][1] == np.nextafter(np.float32(H + 48), np.float32(0))
    assert tuple(uv["(u, v) == (W + 40, 10)"]) == (W + 40, 10) and tuple(uv["(u, v) == (10, H + 40)"]) == (10, H + 40)
    # with W and H exchanged in the frame test exactly one of the last two rows would fall out
    assert (W + 40 < H + 48) != (H + 40 < W + 48)
    z = s.point_cloud[:, 2]
    assert z[8] == CC.EDGE_NEAR and z[9] == np.nextafter(CC.EDGE_NEAR, np.float32(np.inf))
    assert z[10] == CC.EDGE_FAR and z[11] == np.nextafter(CC.EDGE_FAR, np.float32(0))
    # each neighbour is one f32 step from its edge row, in the one coordinate that matters
    for k in range(0, 12, 2):
        d = s.point_cloud[k] != s.point_cloud[k + 1]
        assert d.sum() == 1, what[k]
        a, b = s.point_cloud[k][d][0], s.point_cloud[k + 1][d][0]
        assert b in (np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf))), what[k]
