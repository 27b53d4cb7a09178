"""Cameras outside the family of synthetic.synth() (fx = fy = 0.6 W, principal point in the middle, no skew), the planes that
remove points of its scenes, and a scene whose points sit on the edges of the frame test -- stated once for
test_camera_ref_host.py (CPU: the references agree under them and the cases can show a wrong kernel) and test_gpu_cameras.py.
Nothing here touches the GPU at import."""
import dataclasses

import numpy as np

from oracle import oracle
from taichi_3d_gaussian_splatting_amd.synthetic import synth


def _k(rows):
    return np.array(rows, np.float32)


def _general(W, H):
    return _k([[0.8 * W, 0.05 * W, 0.37 * W], [0, 0.5 * W, 0.66 * H], [0, 0, 1]])


def _general_k10(W, H):
    K = _general(W, H)
    K[1, 0] = 0.03 * W          # the references multiply by the whole matrix; the kernels read Km[3] in three places
    return K


# name -> (W, H) -> (3,3) f32
CAMERAS = {
    "anisotropic": lambda W, H: _k([[0.9 * W, 0, W / 2], [0, 0.45 * W, H / 2], [0, 0, 1]]),
    "offcentre": lambda W, H: _k([[0.6 * W, 0, 0.31 * W], [0, 0.6 * W, 0.72 * H], [0, 0, 1]]),
    "skew": lambda W, H: _k([[0.6 * W, 0.08 * W, W / 2], [0, 0.6 * W, H / 2], [0, 0, 1]]),
    "general": _general,
    "general_k10": _general_k10,
}


def with_camera(scene, name):
    """A copy of a SyntheticScene with only camera_intrinsics replaced: the points stay where synth() put them, so some leave
    the frame and others enter its 48-pixel margin"""
    return dataclasses.replace(scene, camera_intrinsics=CAMERAS[name](scene.width, scene.height))


def _swapped(K, a, b):
    out = K.copy()
    out[a], out[b] = K[b], K[a]
    return out


def _zeroed(K, a):
    out = K.copy()
    out[a] = 0.0
    return out


def confusable(K):
    """[(name, K')]: the cameras a kernel with a one-line error would effectively be using -- fx and fy exchanged, cx and cy
    exchanged, K[0,1] dropped, K[1,0] dropped, K[0,1] and K[1,0] exchanged -- without those that equal K"""
    K = np.asarray(K, np.float32)
    entries = [("fx_fy", _swapped(K, (0, 0), (1, 1))), ("cx_cy", _swapped(K, (0, 2), (1, 2))), ("k01_zero", _zeroed(K, (0, 1))),
               ("k10_zero", _zeroed(K, (1, 0))), ("k01_k10", _swapped(K, (0, 1), (1, 0)))]
    return [(name, Kc) for name, Kc in entries if not np.array_equal(Kc, K)]


# the entries of confusable() that each camera must have at any image size (a camera that lost them tests nothing)
CONFUSABLE_OF = {
    "anisotropic": {"fx_fy"},
    "offcentre": {"cx_cy"},
    "skew": {"k01_zero", "k01_k10"},
    "general": {"fx_fy", "cx_cy", "k01_zero", "k01_k10"},
    "general_k10": {"fx_fy", "cx_cy", "k01_zero", "k10_zero", "k01_k10"},
}

# synth() draws z uniformly in 2..10: each plane removes a share of the points
PLANES = dict(near_plane=3.0, far_plane=7.0)

# the scenes of test_gpu_cameras.py that are compared with the oracle: name -> (synth arguments, seed, allow_partial_tiles)
ORACLE_SCENES = {"250x203": ((4000, 250, 203, 0.08), 0, True), "96x64": ((3000, 96, 64, 0.08), 0, False)}
PLANES_SCENE = ((4000, 250, 203, 0.08), 1, True)


def oracle_scene(name):
    """An entry of ORACLE_SCENES -> (scene, allow_partial_tiles)"""
    args, seed, partial = ORACLE_SCENES[name]
    return synth(*args, seed=seed), partial


def planes_scene():
    args, seed, partial = PLANES_SCENE
    return synth(*args, seed=seed), partial


# ---- points on the edges of the frame test ----------------------------------------------------------------------------------
EDGE_W, EDGE_H = 64, 32
EDGE_K = _k([[32, 0, 16], [0, 64, 8], [0, 0, 1]])
EDGE_NEAR, EDGE_FAR = np.float32(0.8), np.float32(8.0)
# Under the identity pose and at z = 2 every product of the projection is exact in f32: u = 16 x + 16, v = 32 y + 8.
# Rows in pairs of adjacent f32 values of the one coordinate that matters: (what, xyz of the row on the edge, is it in camera,
# the coordinate to step, the direction of the step that crosses the edge)
_EDGE_PAIRS = [
    ("u == -48", (-4.0, 0.0, 2.0), True, 0, -1.0),             # the margin's lower edge is inside (>=)
    ("u == W + 48", (6.0, 0.0, 2.0), False, 0, -1.0),          # its upper edge is outside (<)
    ("v == -48", (0.0, -1.75, 2.0), True, 1, -1.0),
    ("v == H + 48", (0.0, 2.25, 2.0), False, 1, -1.0),
    ("z == near_plane", (0.0, 0.0, float(EDGE_NEAR)), False, 2, 1.0),     # both planes are outside (> and <)
    ("z == far_plane", (0.0, 0.0, float(EDGE_FAR)), False, 2, -1.0),
]
# (u, v) = (W + 40, 10) and (10, H + 40): both in; with W and H exchanged in the test exactly one of them would fall out
_EDGE_SINGLES = [("(u, v) == (W + 40, 10)", (5.5, 0.0625, 2.0)), ("(u, v) == (10, H + 40)", (-0.375, 2.0, 2.0))]
EDGE_MAX_STEPS = 4


def _edge_mask(scene, q, t, cfg, xyz):
    """the oracle's point_in_camera_mask of the one point xyz, with the scene's first row of features"""
    f, _ = oracle.forward(np.asarray(xyz, np.float32).reshape(1, 3), scene.point_cloud_features[:1], scene.point_invalid_mask[:1],
                          scene.point_object_id[:1], q, t, scene.camera_intrinsics, scene.height, scene.width, cfg)
    return f.point_in_camera_mask


def frame_edge_case():
    """-> (scene, q, t, oracle config, expected point_in_camera_mask (N) int8, [what each row is]).  Each neighbour is found by
    stepping the f32 coordinate with nextafter until the oracle's own mask flips (computed in float64 the step rounds back onto
    the edge); it must flip within EDGE_MAX_STEPS steps."""
    n = 2 * len(_EDGE_PAIRS) + len(_EDGE_SINGLES)
    scene = synth(n, EDGE_W, EDGE_H, 0.3, sh_deg=3, seed=12)
    scene.camera_intrinsics = EDGE_K.copy()
    q = np.array([[0.0, 0.0, 0.0, 1.0]], np.float32)
    t = np.zeros((1, 3), np.float32)
    cfg = oracle.default_config(near_plane=float(EDGE_NEAR), far_plane=float(EDGE_FAR))
    rows, expected, what = [], [], []
    for name, xyz, inside, axis, direction in _EDGE_PAIRS:
        on_edge = np.array(xyz, np.float32)
        assert int(_edge_mask(scene, q, t, cfg, on_edge)[0]) == int(inside), name
        beside = on_edge.copy()
        for _ in range(EDGE_MAX_STEPS):
            beside[axis] = np.nextafter(beside[axis], np.float32(direction * np.inf), dtype=np.float32)
            if int(_edge_mask(scene, q, t, cfg, beside)[0]) != int(inside):
                break
        else:
            raise AssertionError(f"{name}: the oracle's mask does not flip within {EDGE_MAX_STEPS} f32 steps")
        rows += [on_edge, beside]
        expected += [int(inside), int(not inside)]
        what += [name, name + ", one step across"]
    for name, xyz in _EDGE_SINGLES:
        rows.append(np.array(xyz, np.float32))
        expected.append(1)
        what.append(name)
    scene.point_cloud = np.stack(rows).astype(np.float32)
    return scene, q, t, cfg, np.array(expected, np.int8), what
