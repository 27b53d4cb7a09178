"""GPU (-m gpu): differentiable depth (config.differentiable_depth) and accumulated alpha (forward(...,
return_accumulated_alpha=True)), i.e. gs_backward_ex, against the float64 reference of tests/torch_ref.py; that the
switch changes nothing while the depth is unused; determinism; the hook, controller and pose paths; heavy tiles.

Bars.  Pose gradients: those of test_gpu_pose_grad (1e-4 of the tensor maximum; per element 2e-5 |ref| + 5e-6 of the summed
per-point magnitude).  Point gradients: 1e-4 of the maximum of each column group (xyz, q, s, opacity, sh) and exact zeros outside
the frustum.  (A per-element bar needs the magnitude summed per contribution, which only the oracle has, for the image alone; a
per-tile sum is not such a bound -- the CPU oracle itself misses it against this float64 reference on the tiny scenes -- and the
f32 keep / skip decisions of splats at the 1/255 edge can differ from float64 ones, so "no contribution" is not compared.)  The
point-gradient references assume all grad factors 1 unless stated, and every SH band."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import parity_util as P
from taichi_3d_gaussian_splatting_amd import _host, _native
from taichi_3d_gaussian_splatting_amd.synthetic import synth, synth_clustered, view_pose

pytestmark = pytest.mark.gpu

_depth_module = functools.partial(P.module, depth=True)          # config.differentiable_depth on, unless a test says otherwise


# the upstreams, the run, the float64 reference and the comparison are parity_util's, shared with test_gpu_cameras.py
_upstream, _run, _check_points, _reference = P.upstream, P.run_outputs, P.check_point_gradients, P.float64_point_gradients


def _scaled(gf, band, factors):
    """the reference's band mask and grad factors applied to a float64 feature gradient (RAST:1102-1125, 1167-1182)"""
    keep = {0: 1, 1: 4, 2: 9}.get(band, 16)
    out = gf.copy()
    out[:, 0:4] *= factors.get("grad_q_factor", 1.0)
    out[:, 4:7] *= factors.get("grad_s_factor", 0.5)
    out[:, 7] *= factors.get("grad_alpha_factor", 20.0)
    for ch in range(3):
        base = 8 + 16 * ch
        out[:, base] *= factors.get("grad_color_factor", 5.0)
        out[:, base + 1:base + keep] *= factors.get("grad_high_order_color_factor", 1.0)
        out[:, base + keep:base + 16] = 0.0
    return out


# Waves per tile of the backward blend (GS_BWD_WAVES_PER_TILE, read by every backward).  These small frames get 4 by default, i.e.
# the one-quadrant AUX kernel; "2" and "1" run the two- and four-quadrant ones (the latter is what frames of 6144 tiles and more,
# 1080p among them, use), and with them the exec-masked AUX block, which quadrants after the first always take.
WAVES_PER_TILE = [None, "2", "1"]


def _waves_per_tile(monkeypatch, wpt):
    if wpt is not None:
        monkeypatch.setenv("GS_BWD_WAVES_PER_TILE", wpt)


@pytest.mark.parametrize("wpt", WAVES_PER_TILE)
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("kind,arg", P.SCENES)
@pytest.mark.parametrize("which", ["depth", "alpha"])
def test_single_output_gradient_matches_float64_reference(which, kind, arg, strict, wpt, monkeypatch):
    """A depth-only (differentiable_depth) or alpha-only loss.  Without this feature the first gives zeros, the second a
    TypeError.  (The colour gradient of both losses is zero: the SH columns are checked to be exactly so.)"""
    _waves_per_tile(monkeypatch, wpt)
    s, q, t, partial = P.scene_case(kind, arg)
    module = _depth_module(partial, strict, **P.UNIT_FACTORS)
    inp = P.make_input(s, q, t)
    ups, _ = _run(module, inp, [which])
    gp, gf = inp.point_cloud.grad.cpu().numpy(), inp.point_cloud_features.grad.cpu().numpy()
    assert np.abs(gp).max() > 0 and np.abs(gf[:, 7]).max() > 0
    assert not gf[:, 8:].any()
    tp, tf, ids = _reference(s, q, t, partial, ups)
    _check_points(gp, gf, tp, tf, ids)


@pytest.mark.parametrize("wpt", WAVES_PER_TILE)
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("kind,arg", P.SCENES[:4])
def test_image_depth_alpha_together_with_default_factors(kind, arg, strict, wpt, monkeypatch):
    """The tiny scenes only: the float64 colour gradient takes the ray origin of the forward, which the reference's backward
    replaces by t_pointcloud_camera (RAST:731-732); the two agree for the near-unit pose quaternions of these scenes."""
    _waves_per_tile(monkeypatch, wpt)
    s, q, t, partial = P.scene_case(kind, arg)
    band = 1
    grads = {}
    for which in (["image", "depth", "alpha"], ["image"], ["depth"], ["alpha"]):
        inp = P.make_input(s, q, t, band)
        ups, _ = _run(_depth_module(partial, strict), inp, which)
        grads[tuple(which)] = (inp.point_cloud.grad.cpu().numpy(), inp.point_cloud_features.grad.cpu().numpy(), ups)
    gp, gf, ups = grads[("image", "depth", "alpha")]
    tp, tf, ids = _reference(s, q, t, partial, ups)
    _check_points(gp, gf, tp, _scaled(tf, band, {}), ids)
    # linear in the upstream: the three single-output backwards add up to the combined one
    for k, a in enumerate((gp, gf)):
        total = sum(grads[(w,)][k] for w in ("image", "depth", "alpha"))
        assert np.abs(total - a).max() <= 1e-5 * np.abs(a).max(), k


@pytest.mark.parametrize("kind,arg", P.SCENES)
def test_pose_gradient_under_depth_loss(kind, arg):
    """A depth loss that pulls every pixel the same way (upstream in [0, 1]): the per-element floor sums |per-point terms|, and a
    zero-mean random upstream cancels inside each point's term, below that floor (the pose bar is set for image losses)."""
    s, q, t, partial = P.scene_case(kind, arg)
    inp = P.make_input(s, q, t, requires_grad=False, pose=True)
    ups, _ = _run(_depth_module(partial), inp, ["depth"], positive=True)
    gq, gt = inp.q_pointcloud_camera.grad.cpu().numpy(), inp.t_pointcloud_camera.grad.cpu().numpy()
    P.assert_pose_gradient_parity(s, q, t, partial, gq, gt, g_depth=ups["depth"])


def test_pose_recovery_from_depth():
    """Offset t by ~3 % of the scene depth and optimise t alone with Adam on an L1 loss against the depth rendered at the
    true pose (lidar-style supervision: pixels the true render covers)."""
    s = synth(4000, 128, 128, 0.12, sh_deg=3, seed=21)
    q_true, t_true = view_pose()
    module = _depth_module()
    with torch.no_grad():
        _, d_true, _, a_true = module(P.make_input(s, q_true, t_true, 3, requires_grad=False), return_accumulated_alpha=True)
        d_true, valid = d_true.clone(), (a_true > 0.5).clone()
    t0 = (t_true[0] + np.array([0.15, -0.1, 0.12])).astype(np.float32)
    t_param = torch.nn.Parameter(torch.tensor(t0[None], device=P.DEV))
    opt = torch.optim.Adam([t_param], lr=2e-3)
    inp = P.make_input(s, q_true, t_true, 3, requires_grad=False)
    e0 = float(np.linalg.norm(t0 - t_true[0]))
    for _ in range(300):
        opt.zero_grad()
        inp.t_pointcloud_camera = t_param
        depth = module(inp)[1]
        loss = ((depth - d_true).abs() * valid).sum() / valid.sum()
        loss.backward()
        opt.step()
    e1 = float(np.linalg.norm(t_param.detach().cpu().numpy()[0] - t_true[0]))
    assert e1 * 5 <= e0, (e0, e1)


def _clustered():
    s = synth_clustered(3000, 64, 64, 0.05, sh_deg=3, seed=4)
    q, t = view_pose(0, 1)
    return s, q, t


@pytest.mark.parametrize("wpt", WAVES_PER_TILE)
def test_heavy_tiles_depth_and_alpha(wpt, monkeypatch):
    """A clustered 64x64 frame (16 tiles) with heavy tiles and lists over 512 entries, so that the forward recorded cuts that the
    depth / alpha backward must not use.  Reference agreement, and an all-zero depth gradient against the image-only backward."""
    _waves_per_tile(monkeypatch, wpt)
    s, q, t = _clustered()
    module = _depth_module(**P.UNIT_FACTORS)
    inp = P.make_input(s, q, t)
    ups, _ = _run(module, inp, ["image", "depth", "alpha"])
    fr = module.last_frame
    assert fr.heavy_tiles() > 0
    ends, starts = fr.export("tile_points_end").cpu().numpy(), fr.export("tile_points_start").cpu().numpy()
    assert (ends - starts).max() > 512
    gp, gf = inp.point_cloud.grad.cpu().numpy(), inp.point_cloud_features.grad.cpu().numpy()
    tp, tf, ids = _reference(s, q, t, False, ups)
    _check_points(gp, gf, tp, tf, ids)
    # image only, then image + an explicit all-zero depth gradient (the AUX walk, without segments)
    base = P.make_input(s, q, t)
    m0 = _depth_module(**P.UNIT_FACTORS)
    img = m0(base)[0]
    g = _upstream(img.shape, 0)
    img.backward(g)
    aux = P.make_input(s, q, t)
    m1 = _depth_module(**P.UNIT_FACTORS)
    outs = m1(aux)
    torch.autograd.backward([outs[0], outs[1]], [g, torch.zeros_like(outs[1])])
    for a, b in ((base.point_cloud.grad, aux.point_cloud.grad), (base.point_cloud_features.grad, aux.point_cloud_features.grad)):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.abs(a - b).max() <= 1e-6 * np.abs(a).max()


def test_switch_without_depth_loss_changes_nothing():
    s = synth(6000, 256, 192, 0.05, sh_deg=3, seed=5)
    q, t = view_pose(1, 3)
    res = []
    for depth in (False, True):
        inp = P.make_input(s, q, t)
        img = _depth_module(depth=depth)(inp)[0]
        img.backward(_upstream(img.shape, 1))
        res.append((inp.point_cloud.grad, inp.point_cloud_features.grad))
    for a, b in zip(*res):
        P.assert_same_bits(a, b)


def test_depth_alpha_backward_is_deterministic():
    s = synth(40000, 512, 384, 0.02, sh_deg=3, seed=9)
    q, t = view_pose()
    inp = P.make_input(s, q, t, pose=True)
    module = _depth_module()
    outs = module(inp, return_accumulated_alpha=True)
    gs = [_upstream(outs[k].shape, k) for k in (0, 1, 3)]
    got = []
    for _ in range(2):
        for x in (inp.point_cloud, inp.point_cloud_features, inp.q_pointcloud_camera, inp.t_pointcloud_camera):
            x.grad = None
        torch.autograd.backward([outs[0], outs[1], outs[3]], gs, retain_graph=True)
        got.append([x.grad.clone() for x in (inp.point_cloud, inp.point_cloud_features, inp.q_pointcloud_camera, inp.t_pointcloud_camera)])
    assert got[0][0].abs().max() > 0
    for a, b in zip(*got):
        P.assert_same_bits(a, b)


def test_hook_and_controller_under_depth_loss():
    """The hook's grad_point_in_camera is the gathered grad_pointcloud; the two controller wirings (rasteriser accumulators and
    the reference's hook-driven update) give identical statistics."""
    from taichi_3d_gaussian_splatting_amd import GaussianPointAdaptiveController as Ctl
    from taichi_3d_gaussian_splatting_amd.scene_io import preallocate
    s = synth(3000, 64, 48, 0.08, sh_deg=3, seed=11)
    q, t = view_pose(0, 1)
    stats = []
    for rasteriser_accumulates in (False, True):
        pc, ft, mask, obj = preallocate(s.point_cloud, s.point_cloud_features, 1.5)
        pc = torch.tensor(pc, device=P.DEV, requires_grad=True)
        ft = torch.tensor(ft, device=P.DEV, requires_grad=True)
        mask, obj = torch.tensor(mask, device=P.DEV), torch.tensor(obj, device=P.DEV)
        ctl = Ctl(Ctl.GaussianPointAdaptiveControllerConfig(), Ctl.GaussianPointAdaptiveControllerMaintainedParameters(pc, ft, mask, obj),
                  seed=5, rasteriser_accumulates=rasteriser_accumulates)
        seen = {}

        def hook(h, ctl=ctl, seen=seen):
            seen["ids"] = h.point_id_in_camera_list.clone()
            seen["gpc"] = h.grad_point_in_camera.clone()
            ctl.update(h)
        module = _depth_module(hook=hook, ctrl=ctl.accumulators if rasteriser_accumulates else None)
        cam = P.CameraInfo(torch.tensor(s.camera_intrinsics, device=P.DEV), s.height, s.width, 0)
        inp = P.Rast.GaussianPointCloudRasterisationInput(pc, ft, obj, mask, cam, torch.tensor(q, device=P.DEV),
                                                         torch.tensor(t, device=P.DEV), color_max_sh_band=3)
        img, depth, _, alpha = module(inp, return_accumulated_alpha=True)
        (((img - 0.3) ** 2).sum() + (depth - 4.0).abs().sum() + ((alpha - 1.0) ** 2).sum()).backward()
        torch.cuda.synchronize()
        ids = seen["ids"].long()
        assert torch.equal(seen["gpc"], pc.grad[ids])
        stats.append({k: getattr(ctl.accumulators, k).clone() for k in ("accumulated_num_in_camera", "accumulated_num_pixels",
                      "accumulated_view_space_position_gradients", "accumulated_view_space_position_gradients_avg",
                      "accumulated_position_gradients", "accumulated_position_gradients_norm")})
    assert stats[0]["accumulated_position_gradients"].abs().max() > 0
    for k in stats[0]:
        P.assert_same_bits(stats[0][k], stats[1][k], k)


def test_argument_errors():
    s, q, t, partial = P.tiny_case(0, 48, 0.25, 32, 32)
    module = _depth_module(partial)
    inp = P.make_input(s, q, t)
    outs = module(inp)
    fr = module.last_frame
    dev = inp.point_cloud.device
    scene, cam, cfg, _intrinsics = _host._marshal_input(module.config, inp)
    N = s.point_cloud.shape[0]
    gpc, gfeat = torch.zeros(N, 3, device=dev), torch.zeros(N, 56, device=dev)
    img = torch.zeros(s.height, s.width, 3, device=dev)
    gd = torch.ones(s.height, s.width, device=dev)
    acc = module.last_forward_outputs["pixel_accumulated_alpha"]
    last = module.last_forward_outputs["pixel_offset_of_last_effective_point"]
    L = _native.lib()
    ptr = lambda x: C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = _native.GsBackwardOut(ptr(gpc), ptr(gfeat))
    call = lambda extra: L.gs_backward_ex(module._ctx_for(dev), fr.handle, C.byref(scene), C.byref(cam), C.byref(cfg), ptr(img),
                                          extra, ptr(acc), ptr(last), 3, C.byref(out), stream)
    rc = call(C.byref(_native.GsBackwardExtra(gd.data_ptr(), None, None)))          # a depth gradient without the depth
    assert rc == -1 and b"rasterized_depth" in L.gs_last_error()
    assert call(None) == 0                                                           # NULL extra: gs_backward
    assert call(C.byref(_native.GsBackwardExtra(None, None, None))) == 0
    assert call(C.byref(_native.GsBackwardExtra(gd.data_ptr(), outs[1].data_ptr(), gd.data_ptr()))) == 0
    torch.cuda.synchronize()
    assert gpc.abs().max() > 0
    with pytest.raises(ValueError):
        cfg2 = P.Rast.GaussianPointCloudRasterisationConfig(rgb_only=True)
        P.Rast(cfg2)(inp, return_accumulated_alpha=True)
