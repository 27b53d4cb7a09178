"""CPU: the float64 pose-gradient reference (tests/torch_ref.py, wrt="pose") that the GPU pose tests compare against is the
derivative of its own render: central finite differences for the oracle's fixed integer structure, with the gradient stops
replayed.  And the reference without a pixel loop (pose_gradients_from_sums, for frames the pixel loop cannot reach) agrees with
it when it is fed the oracle's per-splat sums."""
import numpy as np
import pytest
import torch

import parity_util as P
import torch_ref
from oracle import oracle


def _scene(seed, n, sigma0, width, height, n_objects):
    s, q, t, _ = P.tiny_case(seed, n, sigma0, width, height)
    rng = np.random.default_rng(seed + 100)
    q = q * np.float32(1.3)                                  # not unit
    if n_objects > 1:
        s.point_object_id[:] = (np.arange(n) % n_objects).astype(np.int32)
        q = np.repeat(q, n_objects, 0) + rng.normal(0, 0.01, (n_objects, 4)).astype(np.float32)
        t = np.repeat(t, n_objects, 0) + rng.normal(0, 0.01, (n_objects, 3)).astype(np.float32)
    target = rng.uniform(0, 1, (height, width, 3))
    return s, q, t, target


@pytest.mark.parametrize("seed,n,sigma0,width,height,n_objects", [(0, 40, 0.4, 32, 32, 1), (3, 48, 0.5, 41, 27, 2)])
def test_pose_gradient_matches_finite_differences(seed, n, sigma0, width, height, n_objects):
    s, q, t, target = _scene(seed, n, sigma0, width, height, n_objects)
    cfg = oracle.default_config(allow_partial_tiles=int(width % 16 != 0 or height % 16 != 0))
    f, feat_after = oracle.forward(s.point_cloud, s.point_cloud_features, s.point_invalid_mask, s.point_object_id,
                                   q, t, s.camera_intrinsics, s.height, s.width, cfg)
    assert f.K > 0 and f.pixel_valid_point_count.max() >= 3
    img, _, _, aux = torch_ref.render(s.point_cloud, feat_after, q, t, s.camera_intrinsics, s.height, s.width, f, s.point_object_id,
                                      wrt="pose")
    assert np.allclose(img.detach().numpy(), f.rasterized_image, atol=2e-5)      # the same frame as the f32 oracle
    g_img = 2.0 * (f.rasterized_image.astype(np.float64) - target)
    gq, gt, sq, st = torch_ref.pose_gradients(s, q, t, f, feat_after, g_img)
    assert np.all(np.abs(gq) <= sq * (1 + 1e-12)) and np.all(np.abs(gt) <= st * (1 + 1e-12))
    assert np.abs(gq).max() > 0 and np.abs(gt).max() > 0

    stops = aux["stops"]
    G = torch.as_tensor(g_img)

    def loss(qq, tt):
        with torch.no_grad():
            im = torch_ref.render(s.point_cloud, feat_after, qq, tt, s.camera_intrinsics, s.height, s.width, f,
                                  s.point_object_id, stops=stops, wrt="pose")[0]
            return float((im * G).sum())

    h = 1e-6
    q64, t64 = q.astype(np.float64), t.astype(np.float64)
    for which, base, grad in (("q", q64, gq), ("t", t64, gt)):
        fd = np.zeros_like(base)
        for idx in np.ndindex(base.shape):
            lo, hi = base.copy(), base.copy()
            lo[idx] -= h
            hi[idx] += h
            a = loss(lo, t64) if which == "q" else loss(q64, lo)
            b = loss(hi, t64) if which == "q" else loss(q64, hi)
            fd[idx] = (b - a) / (2 * h)
        err = np.abs(fd - grad).max() / np.abs(grad).max()
        assert err < 1e-6, (which, err, fd, grad)


POSE_CASES = [pytest.param(P.scene_case, (kind, arg), id=f"{kind}-{arg[0] if kind == 'tiny' else arg}") for kind, arg in P.SCENES] \
    + [pytest.param(P.pose_layout_case, (name,), id=name) for name in P.POSE_LAYOUTS]


@pytest.mark.parametrize("make,args", POSE_CASES)
def test_reference_from_sums_matches_the_pixel_loop_reference(make, args):
    """The oracle's f32 sums (oracle.backward_sums) through the float64 per-point chain against float64 throughout: the difference
    is the f32 rounding of the sums, so the bar is the GPU kernels' own tensor bar.  Measured max |a - ref| / max |ref|: at most
    1.6e-5 (soak 54), 1e-7 to 9e-6 on the other scenes and layouts."""
    s, q, t, partial = make(*args)
    f, feat_after = P.oracle_frame(s, q, t, partial)
    g_img = 2.0 * (f.rasterized_image.astype(np.float64) - np.random.default_rng(0).uniform(0, 1, f.rasterized_image.shape))
    ref = torch_ref.pose_gradients(s, q, t, f, feat_after, g_img)
    sums, _ = oracle.backward_sums(f, g_img)
    got = torch_ref.pose_gradients_from_sums(s, q, t, f.point_id_in_camera_list, feat_after, sums)
    for name, a, b in zip(("grad_q", "grad_t", "summed_q", "summed_t"), got, ref):
        assert a.shape == b.shape and np.abs(b).max() > 0, name
        e = P.rel_err(a, b)
        print(f"{name}: max |a - ref| / max |ref| = {e:.3g} (bar {P.GRAD_TOL})")
        assert e < P.GRAD_TOL, (name, e)
    for a, b in zip(got[:2], ref[2:]):                       # rows no touched point depends on: exact zeros in both
        assert not a[b == 0].any()
    if len(args) == 1 and P.POSE_LAYOUTS[args[0]][3]:
        assert not ref[2][-1].any() and not got[2][-1].any()
