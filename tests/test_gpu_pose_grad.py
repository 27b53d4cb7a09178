"""GPU (-m gpu): gradients with respect to q_pointcloud_camera and t_pointcloud_camera (k_pose.hip), against the float64
reference of tests/torch_ref.py; that requesting them changes nothing else; the pose-only backward; determinism; pose recovery;
and the staged path's refusal.

The reduction has three levels: a wave (64 in-camera entries) sums each of its distinct objects, thread 0 merges the block's four
waves into at most cap = min(n_objects, 256) records, k_pose_reduce sums an object's record of every block, 1024 blocks per trip.
P.SCENES and test_multi_object_rows stay within one block (and one wave with several objects); the POSE_LAYOUTS of parity_util
cross waves and blocks under the pixel-loop reference, and the large frame (more than 1024 blocks) under the reference that takes
the per-splat sums (torch_ref.pose_gradients_from_sums)."""
import ctypes as C

import numpy as np
import pytest
import torch

import parity_util as P
import torch_ref
from taichi_3d_gaussian_splatting_amd import _host, _native
from taichi_3d_gaussian_splatting_amd.controller_stats import ControllerAccumulators
from taichi_3d_gaussian_splatting_amd.stages import StagedRasteriser
from taichi_3d_gaussian_splatting_amd.synthetic import synth, view_pose

pytestmark = pytest.mark.gpu


def _target(shape, seed=0):
    return torch.tensor(np.random.default_rng(seed).uniform(0, 1, shape).astype(np.float32), device=P.DEV)


def _run(module, inp, seed=0, retain=False):
    """forward + backward of sum(g * image), g = 2 (image - target); returns (outs, g_image)"""
    outs = module(inp)
    g = 2.0 * (outs[0].detach() - _target(outs[0].shape, seed))
    outs[0].backward(g, retain_graph=retain)
    return outs, g


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("kind,arg", P.SCENES)
def test_pose_gradient_matches_float64_reference(kind, arg, strict):
    s, q, t, partial = P.scene_case(kind, arg)
    module = P.module(partial, strict)
    inp = P.make_input(s, q, t, pose=True)
    outs, g = _run(module, inp)
    assert inp.q_pointcloud_camera.grad is not None and inp.t_pointcloud_camera.grad is not None
    assert inp.q_pointcloud_camera.grad.shape == (1, 4) and inp.t_pointcloud_camera.grad.shape == (1, 3)
    P.assert_pose_gradient_parity(s, q, t, partial, inp.q_pointcloud_camera.grad.cpu().numpy(),
                                  inp.t_pointcloud_camera.grad.cpu().numpy(), g.cpu().numpy())


_multi_object = P.multi_object_case


@pytest.mark.parametrize("n_objects,empty_last", [(3, True), (64, False)])
def test_multi_object_rows(n_objects, empty_last):
    """Kobj = 3 at the full bar.  Kobj = 64 (about one point per object, several objects per wave and block) at the tensor
    bar: the per-element floor sums |per-point terms|, and with one point per object that floor is the point's own term,
    while the upstream that term is made from (loop 1's per-splat sums) is accurate relative to ITS summed per-pixel
    magnitude, which can be much larger (the floor of the point-gradient bar, parity_util.ELEM_FLOOR)."""
    s, q, t, partial = _multi_object(11, n_objects, empty_last=empty_last)
    module = P.module(partial)
    inp = P.make_input(s, q, t, pose=True)
    outs, g = _run(module, inp)
    gq, gt = inp.q_pointcloud_camera.grad.cpu().numpy(), inp.t_pointcloud_camera.grad.cpu().numpy()
    assert gq.shape == (n_objects, 4) and gt.shape == (n_objects, 3)
    rq, rt = P.assert_pose_gradient_parity(s, q, t, partial, gq, gt, g.cpu().numpy(), per_element=n_objects <= 3)
    if empty_last:
        assert (s.point_object_id == n_objects - 1).any()
        assert np.all(gq[-1] == 0) and np.all(gt[-1] == 0)
        assert np.abs(gq[:-1]).min(axis=1).max() > 0


def _reduction_shape(s, q, t, partial):
    """(M, parity_util.pose_reduction_shape) of the frame as k_pose_points sees it, from the oracle"""
    f, _ = P.oracle_frame(s, q, t, partial)
    return f.M, P.pose_reduction_shape(s.point_object_id[f.point_id_in_camera_list], P.affected_pixels(f) > 0)


# what makes each layout reach its path: (M, n_objects, shape) -> bool
LAYOUT_PATHS = {
    # every object has points in both blocks, in several waves each
    "random3_empty_last": lambda M, K, sh: sh["blocks"] == 2 and sh["objects"] == sh["objects_in_several_blocks"] == K - 1,
    "random3": lambda M, K, sh: M == 1200 and sh["blocks"] == 5 and sh["objects_in_several_blocks"] == 3 and sh["per_wave"] == 3,
    # cap == 256 < n_objects: records at the full stride, summed over several blocks
    "random300": lambda M, K, sh: K > 256 and sh["blocks"] == 3 and sh["per_block"] > 64 and sh["objects_in_several_blocks"] > 100,
    # a block whose records fill cap
    "one_point_per_object": lambda M, K, sh: K > 256 and sh["blocks"] == 3 and sh["per_block"] == 256,
    # a wave whose records fill sWave, every object in every block
    "modulo64": lambda M, K, sh: sh["per_wave"] == 64 and sh["blocks"] == 5 and sh["objects_in_several_blocks"] == 64,
    # 100 consecutive entries per object: the object at each of the four block edges is in two blocks, no other is
    "contiguous100": lambda M, K, sh: M == 1200 and sh["objects"] == 12 and sh["objects_in_several_blocks"] == sh["blocks"] - 1 == 4,
}


@pytest.mark.parametrize("name", list(P.POSE_LAYOUTS))
def test_pose_gradient_across_waves_blocks_and_objects(name):
    """The bars of test_multi_object_rows: three objects at the full per-element bar, more at the tensor bar."""
    s, q, t, partial = P.pose_layout_case(name)
    n_objects, empty_last = q.shape[0], P.POSE_LAYOUTS[name][3]
    M, shape = _reduction_shape(s, q, t, partial)
    print(f"{name}: M {M}, objects {n_objects}, {shape}")
    assert LAYOUT_PATHS[name](M, n_objects, shape), (M, shape)
    inp = P.make_input(s, q, t, pose=True)
    outs, g = _run(P.module(partial), inp)
    gq, gt = inp.q_pointcloud_camera.grad.cpu().numpy(), inp.t_pointcloud_camera.grad.cpu().numpy()
    assert gq.shape == (n_objects, 4) and gt.shape == (n_objects, 3)
    P.assert_pose_gradient_parity(s, q, t, partial, gq, gt, g.cpu().numpy(), per_element=n_objects <= 3)
    if empty_last:
        assert (s.point_object_id == n_objects - 1).any()
        assert np.all(gq[-1] == 0) and np.all(gt[-1] == 0)
        assert np.abs(gq[:-1]).min(axis=1).max() > 0


def test_pose_gradient_across_blocks_under_depth_loss():
    """k_pose_points<true> (the sums carry d depth) with three objects over five blocks, under a depth upstream in [0, 1] as
    test_gpu_depth_alpha_grad.test_pose_gradient_under_depth_loss: the full per-element bar."""
    s, q, t, partial = P.pose_layout_case("random3")
    M, shape = _reduction_shape(s, q, t, partial)
    assert LAYOUT_PATHS["random3"](M, 3, shape), (M, shape)
    inp = P.make_input(s, q, t, requires_grad=False, pose=True)
    depth = P.module(partial, depth=True)(inp)[1]
    g = torch.tensor(np.random.default_rng(17).uniform(0, 1, depth.shape).astype(np.float32), device=P.DEV)
    depth.backward(g)
    gq, gt = inp.q_pointcloud_camera.grad.cpu().numpy(), inp.t_pointcloud_camera.grad.cpu().numpy()
    P.assert_pose_gradient_parity(s, q, t, partial, gq, gt, g_depth=g.cpu().numpy())


@pytest.mark.parametrize("n_objects", [1, 300])
def test_pose_gradient_past_one_trip_of_the_block_sum(n_objects):
    """More than 1024 x 256 in-camera points: k_pose_reduce's loop over the blocks takes a second trip.  No pixel loop reaches
    that size, so the frame's per-splat sums come from the staged path under the same upstream (its image has the module's bits,
    so they are the sums the module's backward handed k_pose_points) and the float64 reference is
    torch_ref.pose_gradients_from_sums: what is compared is k_pose.hip alone, per-point chain and reduction.
    The per-element bar of parity_util is derived for sums of at most 1e4 terms; here an element sums up to 2.4e5, so its use is
    printed.  Measured (pose gradient): at most 0.0004 of the bar with one object, 0.014 with 300, against the third
    that parity_util states as the bar's margin, so the bar is asserted here as well.  (It is that far away because the
    reference starts from the library's own f32 sums: loop 1's error, which the floor is sized for, is not in the comparison.)
    Tensor level, measured max |a - ref| / max |ref|: 1.4e-7 to 2.7e-7 against the bar of 1e-4."""
    if n_objects == 1:
        s, q, t, partial = P.tiny_case(*P.LARGE_FRAME)
    else:
        s, q, t, partial = P.multi_object_case(P.LARGE_FRAME[0], n_objects, *P.LARGE_FRAME[1:])
    module = P.module(partial)
    inp = P.make_input(s, q, t, pose=True)
    outs, g = _run(module, inp)
    frame = module.last_frame
    M = frame.n_points_in_camera
    assert M > 262144 and -(-M // 256) > 1024, M
    # the same frame through the staged path (fresh tensors: the projection normalises the quaternions in place)
    st = StagedRasteriser(module.config)
    sinp = P.make_input(s, q, t, requires_grad=False)
    rec, ids, _ = st.project_shard(sinp)
    souts, rframe = st.forward_projected(rec.contiguous(), sinp.camera_info)
    P.assert_same_bits(souts.rasterized_image, outs[0], "staged image")
    sums = st.backward_projected(rframe, souts, g)[0].cpu().numpy().astype(np.float64)
    assert sums.shape == (M, 12)
    P.assert_same_bits(ids, frame.export("point_id_in_camera_list"))
    # to the reference's scaling: loop 1 leaves the per-splat factors opacity and opacity / 2 to the per-point kernels
    alpha = frame.export("point_alpha_after_activation").cpu().numpy().astype(np.float64)
    sums[:, 0:2] *= alpha[:, None]
    sums[:, 2:5] *= 0.5 * alpha[:, None]
    sums[:, 11] = 0.0                                                       # no depth upstream: the column is not written
    touched = int((sums[:, 10] != 0).sum())                                  # the count column: integer bits, zero or not
    rq, rt, sq, st_ = torch_ref.pose_gradients_from_sums(s, q, t, ids.cpu().numpy(), inp.point_cloud_features.detach().cpu().numpy(), sums)
    gq, gt = inp.q_pointcloud_camera.grad.cpu().numpy(), inp.t_pointcloud_camera.grad.cpu().numpy()
    assert gq.shape == (n_objects, 4) and gt.shape == (n_objects, 3)
    for name, a, ref, summed in (("q", gq, rq, sq), ("t", gt, rt, st_)):
        scale = np.abs(ref).max()
        assert scale > 0, name
        err = np.abs(a.astype(np.float64) - ref)
        live = summed > 0
        use = (err[live] / (P.ELEM_RTOL * np.abs(ref[live]) + P.ELEM_FLOOR * summed[live])).max()
        print(f"n_objects {n_objects}, M {M}, blocks {-(-M // 256)}, touched {touched}, grad_{name}: max |a - ref| / max |ref| = "
              f"{err.max() / scale:.3g} (bar {P.GRAD_TOL}), largest use of the per-element bar {use:.3g}")
        assert err.max() / scale < P.GRAD_TOL, (name, err.max() / scale, a, ref)
        assert use <= 1.0, (name, use)
        assert not a[~live].any(), name
    assert (sq > 0).all() and (st_ > 0).all()                                # every object has touched points at this size


HOOK_FIELDS = ["point_id_in_camera_list", "grad_point_in_camera", "grad_pointfeatures_in_camera", "grad_viewspace",
               "magnitude_grad_viewspace", "magnitude_grad_viewspace_on_image", "num_overlap_tiles", "num_affected_pixels",
               "point_depth", "point_uv_in_camera"]


def _full_run(scene, q, t, pose):
    got = {}
    ctrl = ControllerAccumulators.zeros(scene.point_cloud.shape[0], P.DEV)
    module = P.module(hook=lambda h: got.setdefault("hook", {k: getattr(h, k).clone() for k in HOOK_FIELDS}), ctrl=ctrl)
    inp = P.make_input(scene, q, t, pose=pose)
    outs, _ = _run(module, inp)
    torch.cuda.synchronize()
    res = {"image": outs[0], "depth": outs[1], "count": outs[2], "grad_pc": inp.point_cloud.grad,
           "grad_feat": inp.point_cloud_features.grad}
    res.update({"hook." + k: v for k, v in got["hook"].items()})
    for k in ("accumulated_num_in_camera", "accumulated_num_pixels", "accumulated_view_space_position_gradients",
              "accumulated_view_space_position_gradients_avg", "accumulated_position_gradients", "accumulated_position_gradients_norm"):
        res["ctrl." + k] = getattr(ctrl, k).clone()
    return res, inp


def test_requesting_pose_gradients_changes_nothing_else():
    s = synth(6000, 256, 192, 0.05, sh_deg=3, seed=5)
    q, t = view_pose(1, 3)
    base, inp0 = _full_run(s, q, t, pose=False)
    with_pose, inp1 = _full_run(s, q, t, pose=True)
    assert inp0.q_pointcloud_camera.grad is None and inp1.q_pointcloud_camera.grad is not None
    assert len(base) == 5 + 10 + 6
    for k in base:
        P.assert_same_bits(base[k], with_pose[k], k)


def test_pose_only_backward():
    s = synth(6000, 256, 192, 0.05, sh_deg=3, seed=6)
    q, t = view_pose(2, 3)
    joint = P.make_input(s, q, t, pose=True)
    _run(P.module(), joint)
    calls = []
    ctrl = ControllerAccumulators.zeros(s.point_cloud.shape[0], P.DEV)
    only = P.make_input(s, q, t, requires_grad=False, pose=True)
    _run(P.module(hook=calls.append, ctrl=ctrl), only)
    torch.cuda.synchronize()
    assert not calls                                                            # the hook belongs to the point gradient (RAST:1028)
    for k in ("accumulated_num_in_camera", "accumulated_num_pixels", "accumulated_view_space_position_gradients",
              "accumulated_view_space_position_gradients_avg", "accumulated_position_gradients", "accumulated_position_gradients_norm"):
        assert not getattr(ctrl, k).any(), k
    assert only.point_cloud.grad is None and only.point_cloud_features.grad is None
    for a, b in ((joint.q_pointcloud_camera, only.q_pointcloud_camera), (joint.t_pointcloud_camera, only.t_pointcloud_camera)):
        P.assert_same_bits(a.grad, b.grad)
        assert b.grad.abs().max() > 0
    # grad factors and the SH band scale / mask feature gradients only
    other = P.make_input(s, q, t, 0, requires_grad=False, pose=True)
    _run(P.module(grad_color_factor=3.0, grad_high_order_color_factor=0.25, grad_s_factor=7.0, grad_q_factor=2.0,
                  grad_alpha_factor=0.1), other)
    for a, b in ((only.q_pointcloud_camera, other.q_pointcloud_camera), (only.t_pointcloud_camera, other.t_pointcloud_camera)):
        P.assert_same_bits(a.grad, b.grad)


@pytest.mark.parametrize("n_objects", [1, 8])
def test_pose_gradient_is_deterministic(n_objects):
    s = synth(40000, 512, 384, 0.02, sh_deg=3, seed=9)
    q, t = view_pose()
    s.point_object_id[:] = np.random.default_rng(3).integers(0, n_objects, s.point_object_id.shape[0]).astype(np.int32)
    q, t = np.repeat(q, n_objects, 0), np.repeat(t, n_objects, 0)
    grads = []
    inp = P.make_input(s, q, t, pose=True)
    module = P.module()
    outs = module(inp)
    g = 2.0 * (outs[0].detach() - _target(outs[0].shape))
    for _ in range(2):                                                          # the same frame twice (retain_graph)
        inp.q_pointcloud_camera.grad = inp.t_pointcloud_camera.grad = None
        outs[0].backward(g, retain_graph=True)
        grads.append((inp.q_pointcloud_camera.grad.clone(), inp.t_pointcloud_camera.grad.clone()))
    for _ in range(2):                                                          # fresh runs
        inp = P.make_input(s, q, t, pose=True)
        _run(P.module(), inp)
        grads.append((inp.q_pointcloud_camera.grad.clone(), inp.t_pointcloud_camera.grad.clone()))
    assert grads[0][0].abs().max() > 0
    for gq, gt in grads[1:]:
        P.assert_same_bits(gq, grads[0][0])
        P.assert_same_bits(gt, grads[0][1])


def _rotation_error(q, q_ref):
    a, b = q / np.linalg.norm(q), q_ref / np.linalg.norm(q_ref)
    return 2.0 * np.arccos(min(1.0, abs(float(np.dot(a, b)))))


def test_pose_recovery():
    """Localise a camera against a fixed scene: only q and t are optimised (q through a differentiable normalisation, i.e. a
    non-leaf pose), with Adam, against the image rendered at the true pose."""
    s = synth(4000, 128, 128, 0.12, sh_deg=3, seed=21)
    q_true, t_true = view_pose()
    module = P.module()
    with torch.no_grad():
        target = module(P.make_input(s, q_true, t_true, 3, requires_grad=False))[0].clone()
    axis = np.array([1.0, 1.0, 0.3]) / np.linalg.norm([1.0, 1.0, 0.3])
    ang = np.deg2rad(2.0)
    dq = np.concatenate([np.sin(ang / 2) * axis, [np.cos(ang / 2)]])          # a 2 degree rotation, composed with the true one
    qt = q_true[0].astype(np.float64)
    q0 = np.concatenate([dq[3] * qt[:3] + qt[3] * dq[:3] + np.cross(dq[:3], qt[:3]), [dq[3] * qt[3] - dq[:3] @ qt[:3]]]).astype(np.float32)
    t0 = (t_true[0] + np.array([0.15, -0.1, 0.12])).astype(np.float32)               # ~3 % of the scene depth (2 .. 10)
    q_param = torch.nn.Parameter(torch.tensor(q0[None], device=P.DEV))
    t_param = torch.nn.Parameter(torch.tensor(t0[None], device=P.DEV))
    opt = torch.optim.Adam([q_param, t_param], lr=2e-3)
    inp = P.make_input(s, q_true, t_true, 3, requires_grad=False)
    r0, e0 = _rotation_error(q0, q_true[0]), float(np.linalg.norm(t0 - t_true[0]))
    for _ in range(300):
        opt.zero_grad()
        inp.q_pointcloud_camera = q_param / q_param.norm(dim=-1, keepdim=True)
        inp.t_pointcloud_camera = t_param
        image = module(inp)[0]
        loss = ((image - target) ** 2).mean()
        loss.backward()
        opt.step()
    r1 = _rotation_error(q_param.detach().cpu().numpy()[0].astype(np.float64), q_true[0])
    e1 = float(np.linalg.norm(t_param.detach().cpu().numpy()[0] - t_true[0]))
    assert r1 * 5 <= r0 and e1 * 5 <= e0, (r0, r1, e0, e1)


def test_staged_path_refuses_pose_gradients():
    s, q, t, partial = P.tiny_case(0, 48, 0.25, 32, 32)
    module = P.module(partial)
    inp = P.make_input(s, q, t, pose=True)
    module(inp)
    fr = module.last_frame
    dev = inp.point_cloud.device
    scene, cam, cfg, _intrinsics = _host._marshal_input(module.config, inp)
    N, M = s.point_cloud.shape[0], fr.n_points_in_camera
    gpc = torch.zeros(N, 3, device=dev)
    gfeat = torch.zeros(N, 56, device=dev)
    gq = torch.zeros(1, 4, device=dev)
    gt = torch.zeros(1, 3, device=dev)
    sums = torch.zeros(max(M, 1), 12, device=dev)
    L = _native.lib()
    ptr = lambda x: C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = _native.GsBackwardOut(ptr(gpc), ptr(gfeat))
    out.grad_q_pointcloud_camera, out.grad_t_pointcloud_camera = gq.data_ptr(), gt.data_ptr()
    rc = L.gs_backward_shard(module._ctx_for(dev), fr.handle, C.byref(scene), C.byref(cam), C.byref(cfg), ptr(sums), 3,
                             C.byref(out), stream)
    assert rc == -1 and b"pose" in L.gs_last_error()
    # gs_backward: both pose pointers or neither
    img = torch.zeros(s.height, s.width, 3, device=dev)
    acc = module.last_forward_outputs["pixel_accumulated_alpha"]
    last = module.last_forward_outputs["pixel_offset_of_last_effective_point"]
    out.grad_t_pointcloud_camera = None
    rc = L.gs_backward(module._ctx_for(dev), fr.handle, C.byref(scene), C.byref(cam), C.byref(cfg), ptr(img), ptr(acc), ptr(last),
                       3, C.byref(out), stream)
    assert rc == -1 and b"together" in L.gs_last_error()
    torch.cuda.synchronize()
