"""CPU: the float64 reference of the feature-channel operator (tests/channel_ref.py) against the oracle's own blended outputs,
and against itself: linearity, and the backward as the exact transpose of the forward."""
import numpy as np
import pytest

import channel_ref
import parity_util as P
from taichi_3d_gaussian_splatting_amd.synthetic import CONFIGS, synth, view_pose

BAR = 5e-6          # of the tensor maximum: the oracle sums in f32 and takes exp from its polynomial (3e-7)


def _cases():
    for kind, arg in P.SCENES:
        yield f"{kind}-{arg[0] if kind == 'tiny' else arg}", lambda kind=kind, arg=arg: P.scene_case(kind, arg)
    yield "dense_corner", lambda: (P.dense_corner_scene(), *view_pose(), 0)
    yield "cfg1", lambda: (synth(**CONFIGS["cfg1_plumbing"]), *view_pose(), 0)


CASES = dict(_cases())


@pytest.fixture(scope="module", params=list(CASES))
def frame(request):
    s, q, t, partial = CASES[request.param]()
    f, _ = P.oracle_frame(s, q, t, partial)
    return s, f


def test_reference_reproduces_the_oracle_outputs(frame):
    """values = point_color gives rasterized_image, values = camera depth gives rasterized_depth * max(sum w, 1e-6), values = 1
    gives pixel_accumulated_alpha; and the contributor counts are the oracle's (no marginal pixel on these scenes)."""
    s, f = frame
    N = s.point_cloud.shape[0]
    ids = f.point_id_in_camera_list
    values = np.full((N, 5), np.nan)
    values[ids, :3] = f.point_color
    values[ids, 3] = f.point_in_camera[:, 2]
    values[ids, 4] = 1.0
    r = channel_ref.run(f, values=values)
    assert np.isfinite(r["out"]).all()                       # rows outside the camera are never read
    marginal = channel_ref.marginal_pixels(r["count"], f.pixel_valid_point_count)
    print("marginal pixels", int(marginal.sum()), "of", marginal.size)
    keep = ~marginal
    image, depth_sum, alpha = r["out"][..., :3], r["out"][..., 3], r["out"][..., 4]
    e = np.abs(image - f.rasterized_image)[keep].max() / np.abs(f.rasterized_image).max()
    assert e <= BAR, ("image", e)
    want = f.rasterized_depth.astype(np.float64) * np.maximum(r["weight"], 1e-6)
    e = np.abs(depth_sum - want)[keep].max() / np.abs(want).max()
    assert e <= BAR, ("depth sums", e)
    # 1 - T = sum w: a telescoping sum
    e = np.abs(alpha - f.pixel_accumulated_alpha)[keep].max() / np.abs(f.pixel_accumulated_alpha).max()
    assert e <= BAR, ("accumulated alpha", e)


def test_reference_is_linear(frame):
    s, f = frame
    rng = np.random.default_rng(3)
    N = s.point_cloud.shape[0]
    a, b = rng.normal(0, 1, (N, 4)), rng.normal(0, 1, (N, 4))
    ra, rb = channel_ref.run(f, values=a)["out"], channel_ref.run(f, values=b)["out"]
    rc = channel_ref.run(f, values=2.0 * a - 3.0 * b)["out"]
    assert np.abs(rc - (2.0 * ra - 3.0 * rb)).max() <= 1e-12 * max(np.abs(rc).max(), 1.0)


def test_backward_is_the_transpose_of_the_forward(frame):
    """<G, A V> = <A^T G, V> to 1e-12 relative; rows outside the camera get exactly zero"""
    s, f = frame
    rng = np.random.default_rng(4)
    N = s.point_cloud.shape[0]
    V, G = rng.normal(0, 1, (N, 6)), rng.normal(0, 1, (s.height, s.width, 6))
    r = channel_ref.run(f, values=V, grad_out=G)
    lhs, rhs = float((G * r["out"]).sum()), float((r["grad"] * V).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), float((np.abs(G) * r["out_abs"]).sum())), (lhs, rhs)
    outside = np.setdiff1d(np.arange(N), f.point_id_in_camera_list)
    assert not r["grad"][outside].any() and not r["grad_abs"][outside].any()
    assert (np.abs(r["grad"]) <= r["grad_abs"] * (1 + 1e-12)).all()
