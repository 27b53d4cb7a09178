"""GPU: the zero rows of the feature gradients written by fill blocks of the backward blend's launch (k_backward.hip: GsZeroFill,
k_bwd_points<.., PREZEROED>).  Canary: every output array of a backward is NaN before the call; afterwards no NaN is left and
every array has the bits of the same call under GS_BWD_PREFILL=0 (the points stage writing every row itself).  Through the
library's own call path, _native.call("gs_backward", ...), with caller-allocated outputs."""
import numpy as np
import pytest
import torch

import parity_util as P
from taichi_3d_gaussian_splatting_amd import _native
from taichi_3d_gaussian_splatting_amd.synthetic import synth, view_pose

pytestmark = pytest.mark.gpu

W, H = 64, 48
PER_POINT = dict(grad_pointcloud=3, grad_pointcloud_features=56, grad_viewspace=2, magnitude_grad_viewspace=1)
PER_VISIBLE = dict(num_affected_pixels=1)
HOOK = dict(hook_grad_point_in_camera=3, hook_grad_pointfeatures_in_camera=56, hook_grad_viewspace=2, hook_magnitude_grad_viewspace=1,
            hook_point_id_in_camera_list=1, hook_num_overlap_tiles=1, hook_point_depth=1, hook_point_uv_in_camera=2)


def mixed_scene(n, sigma0=0.25):
    """n splats at 64x48; of every five, one lies behind the camera and one is too faint for any pixel to take (sigmoid(-15) <
    1/255): out-of-camera, in-camera but untouched, and touched rows in one frame.  A single splat sits on the optical axis."""
    s = synth(n, W, H, sigma0, sh_deg=3, seed=n)
    idx = np.arange(n)
    s.point_cloud[idx % 5 == 3, 2] *= -1.0
    s.point_cloud_features[idx % 5 == 4, 7] = -15.0
    if n == 1:
        s.point_cloud[0, :2] = 0.0
        s.point_cloud_features[0, 7] = 2.0
    return s


def forward(s, q, t, partial=False, depth=False):
    """-> (module, inp, outs) with the frame kept for backward"""
    module = P.module(partial, depth=depth, **P.UNIT_FACTORS)
    inp = P.make_input(s, q, t)
    outs = module(inp)
    return module, inp, outs


def upstream(s, seed=5):
    return torch.tensor(np.random.default_rng(seed).normal(0, 1, (s.height, s.width, 3)).astype(np.float32), device=P.DEV)


def nan_outputs(N, M, s, hook=True, points=True, pose=False):
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=P.DEV)
    out = {}
    if points:
        out.update({k: nan(N, c) for k, c in PER_POINT.items()})
        out.update({k: nan(M, c) for k, c in PER_VISIBLE.items()})
        out["magnitude_grad_viewspace_on_image"] = nan(s.height, s.width, 2)
        if hook:
            out.update({k: nan(M, c) for k, c in HOOK.items()})
    if pose:
        out["grad_q_pointcloud_camera"], out["grad_t_pointcloud_camera"] = nan(1, 4), nan(1, 3)
    return out


def backward(module, s, g, hook=True, points=True, pose=False, extra=None, frame=None):
    """One gs_backward (gs_backward_ex with `extra`) through the module's last frame into NaN-filled arrays -> {name: tensor}"""
    fr = frame or module.last_frame
    scene, cam, cfg = fr.marshalled
    out = nan_outputs(s.point_cloud.shape[0], fr.n_points_in_camera, s, hook, points, pose)
    fo = module.last_forward_outputs
    acc, last = fo["pixel_accumulated_alpha"], fo["pixel_offset_of_last_effective_point"]
    ptr, ctx = _native.ptr, module._ctx_for(torch.device(P.DEV))
    o = _native.GsBackwardOut.of(**out)
    if extra is None:
        _native.call("gs_backward", torch.device(P.DEV), ctx, fr.handle, scene, cam, cfg, ptr(g), ptr(acc), ptr(last), 3, o)
    else:
        _native.call("gs_backward_ex", torch.device(P.DEV), ctx, fr.handle, scene, cam, cfg, ptr(g), extra, ptr(acc), ptr(last), 3, o)
    torch.cuda.synchronize()
    return out


def assert_complete(out):
    for name, a in out.items():
        assert not torch.isnan(a).any(), f"{name}: elements the backward did not write"


def both_forms(monkeypatch, module, s, g, **kw):
    """The backward with the fill (the default) and without it -> the filled form's arrays, checked complete and bit-equal"""
    monkeypatch.delenv("GS_BWD_PREFILL", raising=False)
    on = backward(module, s, g, **kw)
    monkeypatch.setenv("GS_BWD_PREFILL", "0")
    off = backward(module, s, g, **kw)
    monkeypatch.delenv("GS_BWD_PREFILL")
    assert_complete(on)
    assert_complete(off)
    assert on.keys() == off.keys()
    for name in on:
        P.assert_same_bits(on[name], off[name], name)
    return on


@pytest.mark.parametrize("hook", [True, False], ids=["hook", "nohook"])
@pytest.mark.parametrize("n", [1, 63, 257, 1000])
def test_sizes(monkeypatch, n, hook):
    """14 n float4 that are no multiple of a fill block's stride; a last wave of the points stage partly past the end; without a
    hook only one range is filled"""
    s = mixed_scene(n)
    module, inp, outs = forward(s, *view_pose())
    assert module.last_frame.n_keys > 0                 # the blend is launched: the fill runs
    both_forms(monkeypatch, module, s, upstream(s), hook=hook)


def test_point_classes(monkeypatch):
    s = mixed_scene(1000)
    module, inp, outs = forward(s, *view_pose())
    got = both_forms(monkeypatch, module, s, upstream(s))
    N, M = s.point_cloud.shape[0], module.last_frame.n_points_in_camera
    ids = got["hook_point_id_in_camera_list"].view(torch.int32).cpu().numpy().ravel()
    npix = got["num_affected_pixels"].view(torch.int32).cpu().numpy().ravel()
    assert np.array_equal(ids, module.last_frame.export("point_id_in_camera_list").cpu().numpy().ravel())
    assert 0 < M < N                                    # out-of-camera rows
    assert (npix == 0).any() and (npix > 0).any()       # in-camera rows no pixel takes, and touched ones
    gf = got["grad_pointcloud_features"].cpu().numpy()
    outside = np.setdiff1d(np.arange(N), ids)
    assert not gf[outside].any() and not gf[ids[npix == 0]].any()
    assert gf[ids[npix > 0]].any(axis=1).all()
    P.assert_same_bits(got["hook_grad_pointfeatures_in_camera"], gf[ids], "the hook's gather")


@pytest.mark.parametrize("waves", [1, 2, 4])
def test_grid_shapes(monkeypatch, waves):
    """the fill blocks behind the grids of the NQ = 4 / 2 / 1 instantiations"""
    monkeypatch.setenv("GS_BWD_WAVES_PER_TILE", str(waves))
    s = mixed_scene(1000)
    module, inp, outs = forward(s, *view_pose())
    both_forms(monkeypatch, module, s, upstream(s))


def test_cut_lists(monkeypatch):
    """heavy items and the item_cap grid sizing in front of the fill blocks, the repair kernel behind"""
    s = P.dense_corner_scene()
    module, inp, outs = forward(s, *view_pose())
    both_forms(monkeypatch, module, s, upstream(s, 11))
    fr = module.last_frame
    if P.default_heavy_policy():
        assert fr.heavy_tiles() > 0 and fr.heavy_tiles(items=True) > fr.heavy_tiles()


def test_no_blend_launch(monkeypatch):
    """M = 0, and K = 0 with M > 0 (splats a pixel wide to the right of the image, inside the three boundary tiles): no blend
    launch, hence no fill -- the points stage writes the zero rows itself"""
    behind = mixed_scene(257)
    behind.point_cloud[:, 2] = -np.abs(behind.point_cloud[:, 2])
    beside = mixed_scene(257)
    fx, cx = beside.camera_intrinsics[0, 0], beside.camera_intrinsics[0, 2]
    beside.point_cloud[:, 2] = np.abs(beside.point_cloud[:, 2])
    beside.point_cloud[:, 0] = (W + 24.0 - cx) * beside.point_cloud[:, 2] / fx
    beside.point_cloud_features[:, 4:7] = np.log(1e-4)
    for s, m_zero in ((behind, True), (beside, False)):
        module, inp, outs = forward(s, *view_pose())
        fr = module.last_frame
        assert fr.n_keys == 0 and (fr.n_points_in_camera == 0) == m_zero
        got = both_forms(monkeypatch, module, s, upstream(s))
        for name, a in got.items():
            if name not in ("hook_point_id_in_camera_list", "hook_num_overlap_tiles", "hook_point_depth", "hook_point_uv_in_camera"):
                assert not a.view(torch.int32).any(), name


def test_stage_api(monkeypatch):
    """gs_backward_projected, then the points stage on its own (gs_backward_shard) on the same frame: nothing was filled for it, and
    it leaves the bits of the fused call"""
    monkeypatch.delenv("GS_BWD_PREFILL", raising=False)
    s = mixed_scene(1000)
    module, inp, outs = forward(s, *view_pose())
    g = upstream(s)
    fused = backward(module, s, g)
    fr = module.last_frame
    scene, cam, cfg = fr.marshalled
    N, M = s.point_cloud.shape[0], fr.n_points_in_camera
    staged = nan_outputs(N, M, s)
    sums = torch.full((M, 12), float("nan"), dtype=torch.float32, device=P.DEV)
    fo = module.last_forward_outputs
    ptr, dev, ctx = _native.ptr, torch.device(P.DEV), module._ctx_for(torch.device(P.DEV))
    _native.call("gs_backward_projected", dev, ctx, fr.handle, ptr(g), ptr(fo["pixel_accumulated_alpha"]),
                 ptr(fo["pixel_offset_of_last_effective_point"]), ptr(sums), ptr(staged["magnitude_grad_viewspace_on_image"]))
    o = _native.GsBackwardOut.of(**{k: v for k, v in staged.items() if k != "magnitude_grad_viewspace_on_image"})
    _native.call("gs_backward_shard", dev, ctx, fr.handle, scene, cam, cfg, ptr(sums), 3, o)
    torch.cuda.synchronize()
    assert_complete(fused)
    assert_complete(staged)
    for name in fused:
        P.assert_same_bits(fused[name], staged[name], name)


def test_depth_gradient(monkeypatch):
    """gs_backward_ex with a depth gradient: the AUX instantiations"""
    s = mixed_scene(1000)
    module, inp, outs = forward(s, *view_pose(), depth=True)
    gd = torch.tensor(np.random.default_rng(6).normal(0, 1, (s.height, s.width)).astype(np.float32), device=P.DEV)
    extra = _native.GsBackwardExtra(grad_rasterized_depth=_native.ptr(gd), rasterized_depth=_native.ptr(outs[1].detach()),
                                    grad_pixel_accumulated_alpha=None)
    with_depth = both_forms(monkeypatch, module, s, upstream(s), extra=extra)
    plain = backward(module, s, upstream(s))
    assert not np.array_equal(P.bits(with_depth["grad_pointcloud"]), P.bits(plain["grad_pointcloud"]))


def test_second_backward_through_a_retained_frame(monkeypatch):
    monkeypatch.delenv("GS_BWD_PREFILL", raising=False)
    s = mixed_scene(257)
    module, inp, outs = forward(s, *view_pose())
    g = upstream(s)
    first = backward(module, s, g)
    second = backward(module, s, g)                     # fresh NaN-filled buffers
    assert_complete(first)
    assert_complete(second)
    for name in first:
        P.assert_same_bits(first[name], second[name], name)


def test_pose_only_backward(monkeypatch):
    """null point-gradient pointers: GS_OK (call() raises otherwise), nothing to fill, the pose gradients of the switch-off call"""
    s = mixed_scene(257)
    module, inp, outs = forward(s, *view_pose())
    got = both_forms(monkeypatch, module, s, upstream(s), points=False, pose=True)
    assert set(got) == {"grad_q_pointcloud_camera", "grad_t_pointcloud_camera"}
    assert got["grad_t_pointcloud_camera"].abs().max() > 0
