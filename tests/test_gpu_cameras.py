"""GPU (-m gpu): the rasteriser under cameras other than the synthetic one (tests/camera_cases.py: fx != fy, a principal point off
the middle, skew, and K[1,0] != 0, which the references multiply by like every other entry), under planes that remove points,
and on points that sit exactly on the edges of the frame test.

Nothing here has a bar of its own: forward and backward against the oracle at the bars of parity_util (integer and per-point f32
exports and the accumulated alpha bit for bit, images within IMAGE_TOL, gradients within GRAD_TOL per group and the per-element
bar, the hook's extras), pose gradients and the depth / alpha gradients against float64 at theirs, the staged path against the
monolithic one bit for bit.  That every camera and scene used here can show a wrong kernel (the oracle itself moves by thousands
of bars under the cameras a one-line error amounts to) is test_camera_ref_host.py.  Each case prints what it uses of its bars."""
import numpy as np
import pytest
import torch

import camera_cases as CC
import parity_util as P
from oracle import oracle
from taichi_3d_gaussian_splatting_amd.stages import StagedRasteriser
from taichi_3d_gaussian_splatting_amd.synthetic import synth, view_pose

pytestmark = pytest.mark.gpu

BAND = 3


def _forward_use(outs, f):
    """what the blended image and depth use of IMAGE_TOL, measured before anything is asserted"""
    image, depth, _ = outs
    return dict(image=P.rel_err(image.detach().cpu().numpy(), f.rasterized_image) / P.IMAGE_TOL,
                depth=P.rel_err(depth.detach().cpu().numpy(), f.rasterized_depth) / P.IMAGE_TOL)


def _backward_use(inp, b):
    """the tensor-level use of GRAD_TOL per group and the worst per-element use of its bar, of a finished backward"""
    gp, gf = inp.point_cloud.grad.cpu().numpy(), inp.point_cloud_features.grad.cpu().numpy()
    use = {"xyz": P.rel_err(gp, b["grad_pointcloud"]) / P.GRAD_TOL}
    for lo, hi, name in P.GROUPS:
        use[name] = P.rel_err(gf[:, lo:hi], b["grad_pointcloud_features"][:, lo:hi]) / P.GRAD_TOL
    use["element"] = max(m["bar_use_max"] for m in P.backward_margins(gp, gf, b).values())
    return use


def _report(what, **uses):
    parts = [f"{k}: " + ", ".join(f"{n} {v:.3g}" for n, v in u.items()) for k, u in uses.items()]
    print(f"camera ratios | {what} | " + " | ".join(parts))


def _fwd_bwd(what, scene, q, t, partial, strict=False, planes=None, seed=0):
    """Forward and backward of the operator against the oracle under the same config, hook extras included -> (module, Forward)"""
    planes = planes or {}
    hooked = []
    module = P.module(partial, strict, hook=hooked.append, **planes)
    ocfg = P.oracle_config(partial, **planes)
    f, feat_after = P.run_oracle(scene, q, t, ocfg)
    assert f.K > 0 and 0 < f.M
    inp = P.make_input(scene, q, t, BAND)
    outs = module(inp)
    fwd = _forward_use(outs, f)
    g = 2.0 * (outs[0].detach() - torch.tensor(P.random_target(scene, seed), device=P.DEV))
    outs[0].backward(g)
    b = oracle.backward(f, g.cpu().numpy(), BAND, ocfg, want_summed=True)
    _report(what, forward=fwd, backward=_backward_use(inp, b))
    P.assert_forward_parity(module, inp, outs, f, feat_after)
    P.assert_backward_parity(module, inp, g.cpu().numpy(), f, BAND, module.last_backward_extras, ocfg)
    assert len(hooked) == 1 and np.array_equal(hooked[0].point_id_in_camera_list.cpu().numpy(), f.point_id_in_camera_list)
    return module, f


@pytest.mark.parametrize("scene,strict", [("250x203", False), ("96x64", False), ("96x64", True)])
@pytest.mark.parametrize("camera", list(CC.CAMERAS))
def test_forward_and_backward_match_the_oracle_under_every_camera(camera, scene, strict):
    """4000 points at 250x203 (partial edge tiles) and 3000 at 96x64, the latter in both forms of the backward, under the
    non-unit pose of tiny_case.  The points stay where the synthetic camera put them: some leave the frame, others enter its
    48-pixel margin."""
    s, partial = CC.oracle_scene(scene)
    s = CC.with_camera(s, camera)
    q, t = P.tiny_pose()
    module, f = _fwd_bwd(f"{camera} {scene}{' reference order' if strict else ''}", s, q, t, partial, strict)
    assert f.M > 1024                      # several blocks of every per-point kernel


def _pose_scene(name):
    if name == "tiny41x27":
        return P.tiny_case(3, 56, 0.5, 41, 27)
    if name == "objects3_41x27":
        return P.multi_object_case(5, 3, 64, 0.5, 41, 27)
    return P.pose_layout_case(name)


@pytest.mark.parametrize("scene", ["tiny41x27", "objects3_41x27", "random3"])
@pytest.mark.parametrize("camera", ["general_k10", "anisotropic"])
def test_pose_gradient_matches_float64_under_a_general_camera(camera, scene):
    """k_pose_points forms d uv / d p from K[0,0], K[0,1], K[1,0], K[1,1] and J(p) from fx, fy: one object, three objects in one
    block, and three objects over several blocks (1200 points at 64x64), under an image upstream"""
    s, q, t, partial = _pose_scene(scene)
    s = CC.with_camera(s, camera)
    f, _ = P.oracle_frame(s, q, t, partial)
    assert f.M > (256 if scene == "random3" else 32), f.M
    inp = P.make_input(s, q, t, pose=True)
    outs = P.module(partial)(inp)
    g = 2.0 * (outs[0].detach() - torch.tensor(P.random_target(s, 0), device=P.DEV))
    outs[0].backward(g)
    gq, gt = inp.q_pointcloud_camera.grad.cpu().numpy(), inp.t_pointcloud_camera.grad.cpu().numpy()
    assert gq.shape == q.shape and gt.shape == t.shape
    _pose_check(f"{camera} {scene} image", s, q, t, partial, gq, gt, g_image=g.cpu().numpy())


def _pose_check(what, s, q, t, partial, gq, gt, **ups):
    """assert_pose_gradient_parity at its full bars; what it uses of them is printed even when it fails"""
    use = {}
    try:
        P.assert_pose_gradient_parity(s, q, t, partial, gq, gt, use=use, **ups)
    finally:
        _report(what, pose=use)


def test_pose_gradient_under_a_depth_upstream_and_a_general_camera():
    """k_pose_points<true> under general_k10, three objects over several blocks; an upstream in [0, 1], as
    test_gpu_pose_grad.test_pose_gradient_across_blocks_under_depth_loss"""
    s, q, t, partial = P.pose_layout_case("random3")
    s = CC.with_camera(s, "general_k10")
    inp = P.make_input(s, q, t, requires_grad=False, pose=True)
    depth = P.module(partial, depth=True)(inp)[1]
    g = torch.tensor(np.random.default_rng(17).uniform(0, 1, depth.shape).astype(np.float32), device=P.DEV)
    depth.backward(g)
    gq, gt = inp.q_pointcloud_camera.grad.cpu().numpy(), inp.t_pointcloud_camera.grad.cpu().numpy()
    _pose_check("general_k10 random3 depth", s, q, t, partial, gq, gt, g_depth=g.cpu().numpy())


@pytest.mark.parametrize("arg", [(0, 48, 0.25, 32, 32), (3, 56, 0.5, 41, 27)], ids=["32x32", "41x27"])
@pytest.mark.parametrize("which", ["depth", "alpha"])
def test_depth_and_alpha_gradients_match_float64_under_general_k10(which, arg):
    """test_gpu_depth_alpha_grad.test_single_output_gradient_matches_float64_reference under general_k10, default waves per tile"""
    s, q, t, partial = P.tiny_case(*arg)
    s = CC.with_camera(s, "general_k10")
    module = P.module(partial, depth=True, **P.UNIT_FACTORS)
    inp = P.make_input(s, q, t)
    ups, _ = P.run_outputs(module, inp, [which])
    gp, gf = inp.point_cloud.grad.cpu().numpy(), inp.point_cloud_features.grad.cpu().numpy()
    assert np.abs(gp).max() > 0 and np.abs(gf[:, 7]).max() > 0
    assert not gf[:, 8:].any()
    tp, tf, ids = P.float64_point_gradients(s, q, t, partial, ups)
    use = {"xyz": P.rel_err(gp.astype(np.float64), tp) / P.GRAD_TOL}
    for lo, hi, name in P.GROUPS[:3]:
        use[name] = P.rel_err(gf[:, lo:hi].astype(np.float64), tf[:, lo:hi]) / P.GRAD_TOL
    _report(f"general_k10 {arg[3]}x{arg[4]} {which}", gradient=use)
    P.check_point_gradients(gp, gf, tp, tf, ids)


def test_staged_path_under_general_k10():
    """records_scene() cut at SHARD_CUTS (a single-row shard, an empty one) under general_k10: the staged chain against the
    monolithic operator bit for bit, the operator against the oracle, and the frame rendered from the records against the
    oracle's forward_from_projected of the same records"""
    s = CC.with_camera(P.records_scene(), "general_k10")
    q, t = view_pose()
    target = torch.tensor(P.random_target(s, 1), device=P.DEV)
    g_fn = lambda image: 2.0 * (image - target)
    hooked = []
    mod = P.module(False, hook=hooked.append)
    mono = P.run_monolithic(mod, s, q, t, BAND, g_fn)
    ocfg = P.oracle_config(False)
    f, feat_after = P.run_oracle(s, q, t, ocfg)
    assert f.K > 0 and f.M > 1024
    b = oracle.backward(f, mono.g.cpu().numpy(), BAND, ocfg, want_summed=True)
    _report("general_k10 records_scene", forward=_forward_use(mono.outs, f), backward=_backward_use(mono.inp, b))
    P.assert_forward_parity(mod, mono.inp, mono.outs, f, feat_after)
    P.assert_backward_parity(mod, mono.inp, mono.g.cpu().numpy(), f, BAND, mod.last_backward_extras, ocfg)
    st = StagedRasteriser(mod.config)
    P.leave_stale_frames(st, synth(5000, 96, 64, 0.12, seed=91), q, t, n_frames=len(P.SHARD_CUTS) + 1)
    staged = P.run_staged(st, s, P.SHARD_CUTS, q, t, BAND, g_fn)
    assert len(hooked) == 1
    P.assert_same_frame(staged, mono, "staged against monolithic")
    P.assert_staged_equals_monolithic(staged, mono, hooked[0], mod.last_backward_extras)
    # the records are the oracle's, and so is the frame made from them
    assert np.array_equal(staged.ids, f.point_id_in_camera_list)
    kept = [c for c in range(16) if c != 11]                   # column 11 is the library's own (alpha_cut); the oracle leaves it zero
    P.assert_same_bits(np.ascontiguousarray(staged.records[:, kept]), np.ascontiguousarray(oracle.pack_records(f)[:, kept]), "projected records")
    fr = oracle.forward_from_projected(staged.records, s.height, s.width, ocfg)
    assert fr.K == staged.n_keys == f.K
    for name in P.RASTER_EXPORTS + ("pixel_offset_of_last_effective_point", "pixel_valid_point_count"):
        assert np.array_equal(staged[name], getattr(fr, name)), name
    P.assert_same_bits(staged.pixel_accumulated_alpha, fr.pixel_accumulated_alpha, "pixel_accumulated_alpha")
    assert P.rel_err(staged.rasterized_image, fr.rasterized_image) < P.IMAGE_TOL
    assert P.rel_err(staged.rasterized_depth, fr.rasterized_depth) < P.IMAGE_TOL


@pytest.mark.parametrize("camera", [None] + list(CC.CAMERAS))
def test_planes_that_remove_points(camera):
    """near_plane = 3 and far_plane = 7 on a scene with z in 2..10: both planes remove points (test_camera_ref_host.py), the
    library and the oracle run under the same config and keep the same ones"""
    s, partial = CC.planes_scene()
    if camera is not None:
        s = CC.with_camera(s, camera)
    q, t = P.tiny_pose()
    wide, _ = P.run_oracle(s, q, t, P.oracle_config(partial))
    module, f = _fwd_bwd(f"{camera or 'synthetic'} planes", s, q, t, partial, planes=CC.PLANES, seed=2)
    assert module.config.near_plane == 3.0 and module.config.far_plane == 7.0
    assert module.last_frame.n_points_in_camera == f.M < wide.M


def test_points_on_the_edges_of_the_frame_test():
    """Points whose u, v or z is exactly an edge of the frame test, each beside its f32 neighbour across the edge, with every
    product of the projection exact in f32: the library and the oracle can differ only in a comparison or a bound."""
    s, q, t, ocfg, expected, what = CC.frame_edge_case()
    module = P.module(False, near_plane=float(CC.EDGE_NEAR), far_plane=float(CC.EDGE_FAR))
    f, feat_after = P.run_oracle(s, q, t, ocfg)
    inp = P.make_input(s, q, t, BAND, requires_grad=False)
    with torch.no_grad():
        outs = module(inp)
    got = module.last_frame.export("point_in_camera_mask").cpu().numpy()
    wrong = [w for w, a, b in zip(what, got, expected) if a != b]
    assert not wrong, wrong
    assert np.array_equal(got, f.point_in_camera_mask)
    assert module.last_frame.n_points_in_camera == f.M == int(expected.sum())
    uv = module.last_frame.export("point_uv").cpu().numpy()
    assert uv[0, 0] == np.float32(-48.0)                      # the first row that is in: u == -48 exactly
    _report("frame edges", forward=_forward_use(outs, f))
    P.assert_forward_parity(module, inp, outs, f, feat_after)
