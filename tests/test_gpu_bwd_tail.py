"""GPU: the backward's tail.  By default the fill blocks of the blend backward's launch write everything a point without a
contribution receives (k_backward.hip: GsZeroFill -- zeros over every per-point output, the four hook arrays that repeat forward
data, the in-camera count of the controller), k_bwd_points<.., PREZEROED> visits the touched points only, and k_sum_rows sums a
block's live points from compacted lists.  GS_BWD_PREFILL=0 selects the previous tail (four lanes per point over all M; the points
stage writing every value itself).  Every case fills every output with NaN canaries, runs both forms and asserts that nothing is
left unwritten and that the two forms agree bit for bit.

The scene is that of test_gpu_parity.py::test_splats_covering_most_of_the_image at its small size with runs of out-of-camera,
untouched and opaque points added, so that the blocks of 256 in-camera points differ in their live population and every class of
row count (quad, wave up to 256 rows, wave beyond, block) is met.  The CPU oracle says of it, with the upstream gradient of
`upstream`: M = 2588 (M mod 256 = 28), K = 17641, 1739 live points; at four rows per pair 1545 of them with at most 32 rows, 174 with
33..256, 12 with 257..1024, 8 with more; live points per block of 256: 232 221 224 92 0 56 232 216 221 220 25.  The test asserts
at-least bounds on these, from the GPU's own hook_num_overlap_tiles and num_affected_pixels."""
import numpy as np
import pytest
import torch

import parity_util as P
from taichi_3d_gaussian_splatting_amd import _native
from taichi_3d_gaussian_splatting_amd.controller_stats import ControllerAccumulators
from taichi_3d_gaussian_splatting_amd.synthetic import synth, view_pose
from test_gpu_bwd_prefill import HOOK, PER_POINT, PER_VISIBLE, assert_complete, forward, mixed_scene, upstream

pytestmark = pytest.mark.gpu

ACC = ["accumulated_num_in_camera", "accumulated_num_pixels", "accumulated_view_space_position_gradients",
       "accumulated_view_space_position_gradients_avg", "accumulated_position_gradients", "accumulated_position_gradients_norm"]
FEATURE_ROWS = ("grad_pointcloud_features", "hook_grad_pointfeatures_in_camera")      # must stay 16-byte aligned


def tail_scene():
    s = synth(3000, 640, 400, 0.02, sh_deg=3, seed=21)
    f, pc = s.point_cloud_features, s.point_cloud
    f[:6, 4:7] = np.log(2.5); f[:6, 7] = -3.0; pc[:6, :2] *= 0.2          # larger than the image: giants at four rows per pair
    f[6:40, 4:7] = np.log(0.3); f[6:40, 7] = -2.0                         # a few hundred tiles each
    f[40:120, 4:7] = np.log(0.08); f[40:120, 7] = -1.0                    # some dozens
    idx = np.arange(3000)
    pc[(idx >= 120) & (idx % 7 == 3), 2] *= -1.0                          # behind the camera
    f[1000:1700, 7] = -15.0                                               # a run no pixel takes (sigmoid(-15) < 1/255)
    f[2000:2400, 7] = 3.0                                                 # opaque: hides what lies behind
    return s


def canaries(N, M, s, hook=True, offset=0):
    """NaN-filled outputs -> ({name: tensor}, backing).  Every array is a view into a longer buffer with four floats of slack behind
    it; offset = 1: every array but the two of feature rows also starts one float past a 16-byte boundary, so that the scalar head
    and tail stores of the fill's ranges run.  backing: what assert_slack_untouched checks after the call."""
    shapes = {k: (N, c) for k, c in PER_POINT.items()}
    shapes.update({k: (M, c) for k, c in PER_VISIBLE.items()})
    shapes["magnitude_grad_viewspace_on_image"] = (s.height, s.width, 2)
    if hook:
        shapes.update({k: (M, c) for k, c in HOOK.items()})
    out, backing = {}, []
    for name, shape in shapes.items():
        n = int(np.prod(shape))
        o = 0 if name in FEATURE_ROWS else offset
        buf = torch.full((n + o + 4,), float("nan"), dtype=torch.float32, device=P.DEV)
        assert buf.data_ptr() % 16 == 0
        out[name] = buf[o:o + n].view(*shape)
        backing.append((name, buf, o, n))
    return out, backing


def assert_slack_untouched(backing):
    """no store of the backward landed in front of an array or behind it"""
    for name, buf, o, n in backing:
        assert torch.isnan(buf[:o]).all() and torch.isnan(buf[o + n:]).all(), f"{name}: a store outside the array"


def run(module, s, g, hook=True, extra=None, offset=0, ctrl=None):
    """One gs_backward (gs_backward_ex with `extra`) through the module's last frame into canaries -> {name: tensor}"""
    fr = module.last_frame
    scene, cam, cfg = fr.marshalled
    out, backing = canaries(s.point_cloud.shape[0], fr.n_points_in_camera, s, hook, offset)
    fo = module.last_forward_outputs
    acc, last = fo["pixel_accumulated_alpha"], fo["pixel_offset_of_last_effective_point"]
    ptr, dev = _native.ptr, torch.device(P.DEV)
    o = _native.GsBackwardOut.of(controller=_native.GsControllerAccumulators.of(ctrl) if ctrl is not None else None, **out)
    if extra is None:
        _native.call("gs_backward", dev, module._ctx_for(dev), fr.handle, scene, cam, cfg, ptr(g), ptr(acc), ptr(last), 3, o)
    else:
        _native.call("gs_backward_ex", dev, module._ctx_for(dev), fr.handle, scene, cam, cfg, ptr(g), extra, ptr(acc), ptr(last), 3, o)
    torch.cuda.synchronize()
    assert_slack_untouched(backing)
    return out


def both(monkeypatch, module, s, g, **kw):
    """Default tail and GS_BWD_PREFILL=0 -> the default's arrays, both complete and bit-equal"""
    monkeypatch.delenv("GS_BWD_PREFILL", raising=False)
    on = run(module, s, g, **kw)
    monkeypatch.setenv("GS_BWD_PREFILL", "0")
    off = run(module, s, g, **kw)
    monkeypatch.delenv("GS_BWD_PREFILL")
    assert_complete(on)
    assert_complete(off)
    assert on.keys() == off.keys()
    for name in on:
        P.assert_same_bits(on[name], off[name], name)
    return on


def live_rows(got, rows_per_pair):
    """-> (rows of every in-camera point, live mask) from the backward's own outputs"""
    ntiles = got["hook_num_overlap_tiles"].view(torch.int32).cpu().numpy().ravel().astype(np.int64)
    live = got["num_affected_pixels"].view(torch.int32).cpu().numpy().ravel() > 0
    return ntiles * rows_per_pair, live


def assert_scene_classes(got, rows_per_pair):
    rows, live = live_rows(got, rows_per_pair)
    M = rows.size
    assert M > 10 * 256 and M % 256 not in (0, 255), M                 # eleven blocks, a short last one
    r = rows[live]
    assert (r <= 32).sum() >= 1000 and ((r > 32) & (r <= 256)).sum() >= (100 if rows_per_pair == 4 else 10)
    if rows_per_pair == 4:
        assert ((r > 256) & (r <= 1024)).sum() >= 8 and (r > 1024).sum() >= 4, ((r > 256).sum(), (r > 1024).sum())
    else:
        assert (r > 1024).sum() == 0 and (r > 256).sum() >= 4                          # one wave per tile: no giants
    per_block = np.add.reduceat(live.astype(np.int64), np.arange(0, M, 256))
    assert (per_block == 0).any()                                       # an empty block
    assert ((per_block > 0) & (per_block < 64)).any()                   # under one wave's worth
    assert (per_block > 192).sum() >= 4                                 # nearly full ones: several passes of the quad loop
    assert ((per_block > 64) & (per_block <= 192)).any()
    assert 0 < per_block[-1] < M % 256                                  # the short last block, live and untouched points in it


@pytest.mark.parametrize("hook", [True, False], ids=["hook", "nohook"])
def test_tail_scene(monkeypatch, hook):
    s = tail_scene()
    module, inp, outs = forward(s, *view_pose())
    got = both(monkeypatch, module, s, upstream(s), hook=hook)
    if hook:
        assert_scene_classes(got, 4)
        ids = got["hook_point_id_in_camera_list"].view(torch.int32).cpu().numpy().ravel()
        fr = module.last_frame
        assert np.array_equal(ids, fr.export("point_id_in_camera_list").cpu().numpy().ravel())
        assert np.array_equal(got["hook_num_overlap_tiles"].view(torch.int32).cpu().numpy().ravel(), fr.export("num_overlap_tiles").cpu().numpy().ravel())
        assert np.array_equal(got["hook_point_uv_in_camera"].cpu().numpy().ravel(), fr.export("point_uv").cpu().numpy().ravel())
        P.assert_same_bits(got["hook_grad_point_in_camera"], got["grad_pointcloud"][torch.as_tensor(ids, device=P.DEV).long()], "the hook's gather")
        live = got["num_affected_pixels"].view(torch.int32).cpu().numpy().ravel() > 0
        gp = got["grad_pointcloud"].cpu().numpy()
        assert not gp[ids[~live]].any() and not gp[np.setdiff1d(np.arange(gp.shape[0]), ids)].any()
        assert gp[ids[live]].any(axis=1).mean() > 0.99


@pytest.mark.parametrize("waves", [1, 2, 4])
def test_waves_per_tile(monkeypatch, waves):
    """rows per pair 1, 2, 4: other class populations of the same points (1: no giants)"""
    monkeypatch.setenv("GS_BWD_WAVES_PER_TILE", str(waves))
    s = tail_scene()
    module, inp, outs = forward(s, *view_pose())
    got = both(monkeypatch, module, s, upstream(s))
    if waves in (1, 4):
        assert_scene_classes(got, waves)


def test_depth_gradient(monkeypatch):
    """gs_backward_ex with a depth gradient: the AUX instantiations"""
    s = tail_scene()
    module, inp, outs = forward(s, *view_pose(), depth=True)
    gd = torch.tensor(np.random.default_rng(6).normal(0, 1, (s.height, s.width)).astype(np.float32), device=P.DEV)
    extra = _native.GsBackwardExtra(grad_rasterized_depth=_native.ptr(gd), rasterized_depth=_native.ptr(outs[1].detach()),
                                    grad_pixel_accumulated_alpha=None)
    with_depth = both(monkeypatch, module, s, upstream(s), extra=extra)
    plain = run(module, s, upstream(s))
    assert not np.array_equal(P.bits(with_depth["grad_pointcloud"]), P.bits(plain["grad_pointcloud"]))


def test_controller_accumulators_over_two_backwards(monkeypatch):
    """The six accumulators attached, two backward calls that accumulate: the in-camera count comes from the fill blocks, exactly
    once per in-camera point and call; the other five from the touched points"""
    s = tail_scene()
    module, inp, outs = forward(s, *view_pose())
    g, g2 = upstream(s), upstream(s, 7)
    N = s.point_cloud.shape[0]
    acc = {}
    for form in ("on", "off"):
        if form == "off":
            monkeypatch.setenv("GS_BWD_PREFILL", "0")
        else:
            monkeypatch.delenv("GS_BWD_PREFILL", raising=False)
        acc[form] = ControllerAccumulators.zeros(N, torch.device(P.DEV))
        first = run(module, s, g, ctrl=acc[form])
        second = run(module, s, g2, ctrl=acc[form])
        assert_complete(first)
        assert_complete(second)
    monkeypatch.delenv("GS_BWD_PREFILL")
    for name in ACC:
        P.assert_same_bits(getattr(acc["on"], name), getattr(acc["off"], name), name)
    ids = second["hook_point_id_in_camera_list"].view(torch.int32).cpu().numpy().ravel()
    nic = acc["on"].accumulated_num_in_camera.cpu().numpy()
    expect = np.zeros(N, np.int32)
    expect[ids] = 2
    assert np.array_equal(nic, expect)
    npix = first["num_affected_pixels"].view(torch.int32).cpu().numpy().ravel() + second["num_affected_pixels"].view(torch.int32).cpu().numpy().ravel()
    assert np.array_equal(acc["on"].accumulated_num_pixels.cpu().numpy()[ids], npix)


def test_stage_api(monkeypatch):
    """gs_backward_projected (k_sum_rows in its default mapping, no fill) + gs_backward_shard (the points stage writing everything)
    leave the bits of the fused call"""
    monkeypatch.delenv("GS_BWD_PREFILL", raising=False)
    s = tail_scene()
    module, inp, outs = forward(s, *view_pose())
    g = upstream(s)
    fused = run(module, s, g)
    fr = module.last_frame
    scene, cam, cfg = fr.marshalled
    N, M = s.point_cloud.shape[0], fr.n_points_in_camera
    staged, backing = canaries(N, M, s)
    sums = torch.full((M, 12), float("nan"), dtype=torch.float32, device=P.DEV)
    fo = module.last_forward_outputs
    ptr, dev = _native.ptr, torch.device(P.DEV)
    ctx = module._ctx_for(dev)
    _native.call("gs_backward_projected", dev, ctx, fr.handle, ptr(g), ptr(fo["pixel_accumulated_alpha"]),
                 ptr(fo["pixel_offset_of_last_effective_point"]), ptr(sums), ptr(staged["magnitude_grad_viewspace_on_image"]))
    o = _native.GsBackwardOut.of(**{k: v for k, v in staged.items() if k != "magnitude_grad_viewspace_on_image"})
    _native.call("gs_backward_shard", dev, ctx, fr.handle, scene, cam, cfg, ptr(sums), 3, o)
    torch.cuda.synchronize()
    assert not torch.isnan(sums[:, :10]).any()              # every row of the sums written, the untouched points' too
    live = fused["num_affected_pixels"].view(torch.int32).ravel() > 0
    assert not sums[~live].view(torch.int32).any()
    assert_complete(fused)
    assert_complete(staged)
    assert_slack_untouched(backing)
    for name in fused:
        P.assert_same_bits(fused[name], staged[name], name)
    monkeypatch.setenv("GS_BWD_PREFILL", "0")               # the sums of the other mapping
    sums_all = torch.full((M, 12), float("nan"), dtype=torch.float32, device=P.DEV)
    _native.call("gs_backward_projected", dev, ctx, fr.handle, ptr(g), ptr(fo["pixel_accumulated_alpha"]),
                 ptr(fo["pixel_offset_of_last_effective_point"]), ptr(sums_all), ptr(staged["magnitude_grad_viewspace_on_image"]))
    torch.cuda.synchronize()
    monkeypatch.delenv("GS_BWD_PREFILL")
    P.assert_same_bits(sums, sums_all, "per-point sums of the two mappings")


def test_outputs_one_float_past_alignment(monkeypatch):
    """every array but the feature rows offset by one float: heads and tails of the fill's ranges, lengths that are no multiple of
    four floats"""
    s = tail_scene()
    module, inp, outs = forward(s, *view_pose())
    shifted = both(monkeypatch, module, s, upstream(s), offset=1)
    aligned = run(module, s, upstream(s))
    for name in aligned:
        P.assert_same_bits(shifted[name], aligned[name], name)
        if name not in FEATURE_ROWS:
            assert shifted[name].data_ptr() % 16 == 4


@pytest.mark.parametrize("n", [1, 257])
def test_small_scenes(monkeypatch, n):
    """one point; one block and a point of a second one"""
    s = mixed_scene(n)
    module, inp, outs = forward(s, *view_pose())
    assert module.last_frame.n_keys > 0
    both(monkeypatch, module, s, upstream(s))
    both(monkeypatch, module, s, upstream(s), offset=1)


def test_second_backward_through_a_retained_frame(monkeypatch):
    """the tags of the first backward do not count in the second"""
    monkeypatch.delenv("GS_BWD_PREFILL", raising=False)
    s = tail_scene()
    module, inp, outs = forward(s, *view_pose())
    g = upstream(s)
    first = run(module, s, g)
    zero = run(module, s, torch.zeros_like(g))              # another backward in between, with its own tag
    second = run(module, s, g)
    for out in (first, zero, second):
        assert_complete(out)
    for name in first:
        P.assert_same_bits(first[name], second[name], name)
