"""GPU (-m gpu): render_channels (gs_channels_forward / gs_channels_backward) against the float64 reference of
tests/channel_ref.py, against the library's own image and accumulated alpha, and its autograd surface.

The reference is computed once per scene with 64 channels; a channel count C uses the first C columns of the same values and
upstream gradients (both directions are independent per channel)."""
import functools

import numpy as np
import pytest
import torch

import channel_ref
import parity_util as P
from taichi_3d_gaussian_splatting_amd.synthetic import CONFIGS, synth, view_pose

pytestmark = pytest.mark.gpu

# 17: a partial chunk at c0 = 0; 64: two full 32-wide chunks; 33 and 63: a partial chunk at c0 = 32
CHANNELS = [1, 3, 4, 7, 16, 17, 33, 63, 64]


def _scenes():
    d = {}
    for kind, arg in P.SCENES:
        d[f"{kind}-{arg[0] if kind == 'tiny' else arg}"] = functools.partial(P.scene_case, kind, arg)
    d["dense_corner"] = lambda: (P.dense_corner_scene(), *view_pose(), 0)
    d["cfg1"] = lambda: (synth(**CONFIGS["cfg1_plumbing"]), *view_pose(), 0)
    d["cfg2"] = lambda: (synth(**CONFIGS["cfg2_truck7k"]), *view_pose(), 0)
    return d


SCENES = _scenes()
TINY = ["tiny-0", "tiny-1", "tiny-2", "tiny-3", "soak-182"]


def _frozen(name):
    """-> (scene, module, input without grad, forward outputs) with the frame kept"""
    s, q, t, partial = SCENES[name]()
    module = P.module(partial=partial)
    inp = P.make_input(s, q, t, requires_grad=False)
    outs = module(inp, keep_frame=True)
    return s, q, t, partial, module, inp, outs


@functools.lru_cache(maxsize=None)
def _prepared(name):
    """One scene: the kept frame on the GPU, the oracle's frame, 64-channel values and upstream (marginal pixels zeroed) and the
    float64 reference of both directions."""
    s, q, t, partial, module, inp, outs = _frozen(name)
    f, _ = P.oracle_frame(s, q, t, partial)
    assert np.array_equal(outs[2].cpu().numpy(), f.pixel_valid_point_count)
    rng = np.random.default_rng(11)
    N = s.point_cloud.shape[0]
    V = rng.normal(0, 1, (N, 64)).astype(np.float32)
    G = rng.normal(0, 1, (s.height, s.width, 64)).astype(np.float32)
    r = channel_ref.run(f, values=V, grad_out=G)
    marginal = channel_ref.marginal_pixels(r["count"], f.pixel_valid_point_count)
    print(f"{name}: marginal pixels {int(marginal.sum())} of {marginal.size}")
    if marginal.any():
        G[marginal] = 0.0
        r = channel_ref.run(f, values=V, grad_out=G)
    return dict(scene=s, module=module, inp=inp, frame=module.last_frame, f=f, V=V, G=G, ref=r, marginal=marginal)


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=P.DEV)


def _assert_elementwise(a, ref, summed, what):
    a, ref, summed = a.astype(np.float64), ref.astype(np.float64), summed.astype(np.float64)
    err = np.abs(a - ref)
    bar = P.ELEM_RTOL * np.abs(ref) + P.ELEM_FLOOR * summed
    use = float((err / np.maximum(bar, 1e-300))[summed > 0].max()) if (summed > 0).any() else 0.0
    print(f"{what}: tensor rel_err {P.rel_err(a, ref):.3g}, worst use of the per-element bar {use:.3g}")
    assert P.rel_err(a, ref) < P.GRAD_TOL, (what, P.rel_err(a, ref))
    assert np.all(err <= bar), (what, use)
    assert not a[summed == 0].any(), what                 # nothing was summed: exactly zero


@pytest.mark.parametrize("name", list(SCENES))
def test_forward_matches_the_reference(name):
    d = _prepared(name)
    keep = ~d["marginal"]
    for C in CHANNELS:
        out = d["module"].render_channels(_dev(d["V"][:, :C]), d["frame"]).cpu().numpy()
        assert out.shape == (d["scene"].height, d["scene"].width, C)
        _assert_elementwise(out[keep], d["ref"]["out"][..., :C][keep], d["ref"]["out_abs"][..., :C][keep], f"{name} forward C={C}")


@pytest.mark.parametrize("name", list(SCENES))
def test_backward_matches_the_reference(name):
    d = _prepared(name)
    f = d["f"]
    outside = np.setdiff1d(np.arange(f.N), f.point_id_in_camera_list)
    for C in CHANNELS:
        v = _dev(d["V"][:, :C]).requires_grad_(True)
        d["module"].render_channels(v, d["frame"]).backward(_dev(d["G"][..., :C]))
        g = v.grad.cpu().numpy()
        assert g.shape == (f.N, C)
        _assert_elementwise(g, d["ref"]["grad"][:, :C], d["ref"]["grad_abs"][:, :C], f"{name} backward C={C}")
        assert not g[outside].any()


@functools.lru_cache(maxsize=None)
def _kept(name):
    s, q, t, partial, module, inp, outs = _frozen(name)
    rng = np.random.default_rng(13)
    V = rng.normal(0, 1, (s.point_cloud.shape[0], 64)).astype(np.float32)
    G = rng.normal(0, 1, (s.height, s.width, 64)).astype(np.float32)
    return s, module, module.last_frame, V, G


@pytest.mark.parametrize("C", [3, 17, 33, 63])
@pytest.mark.parametrize("name", ["tiny-3", "soak-54"])
def test_raw_calls_write_their_outputs_and_nothing_around_them(name, C):
    """`out` and `grad_values` inside larger sentinel-filled allocations, 67 floats of band on each side (so the outputs are
    4-byte aligned and no more): the bands keep the sentinel, no element inside does, and the inside is render_channels' result
    bit for bit.  tiny-3 is 41 x 27: its edge tiles hold pixels outside the image.

    gs_channels_backward clears all of grad_values before its kernels run, so a chunk that was never summed leaves zeros, not
    the sentinel, and render_channels would leave the same zeros.  Hence the second yardstick: the same columns rendered with
    whole chunks only (4 channels for C = 3, 64 for the others, which share C's chunk width): a channel's arithmetic does not
    depend on the channels beside it, so the first C columns of both directions are the same bits."""
    from taichi_3d_gaussian_splatting_amd import _native
    s, module, frame, V, G = _kept(name)
    band, sentinel = 67, -1.2345678e30
    v = _dev(V[:, :C]).requires_grad_(True)
    g = _dev(G[..., :C])
    want_out = module.render_channels(v, frame)
    want_out.backward(g)
    want = {"gs_channels_forward": want_out.detach(), "gs_channels_backward": v.grad}
    assert want_out.abs().max() > 0 and v.grad.abs().max() > 0
    whole = 4 if C <= 4 else 64
    vw = _dev(V[:, :whole]).requires_grad_(True)
    out_w = module.render_channels(vw, frame)
    out_w.backward(_dev(G[..., :whole]))
    P.assert_same_bits(want_out.detach(), out_w.detach()[..., :C].contiguous(), "forward against whole chunks")
    P.assert_same_bits(v.grad, vw.grad[:, :C].contiguous(), "backward against whole chunks")
    assert (v.grad != 0).any(dim=0).all(), "a channel without any gradient"
    for entry, src in (("gs_channels_forward", v.detach()), ("gs_channels_backward", g)):
        size = want[entry].numel()
        buf = torch.full((size + 2 * band,), sentinel, dtype=torch.float32, device=P.DEV)
        _native.call(entry, buf.device, frame._context.handle, frame.handle, src.data_ptr(), C, frame.last.data_ptr(),
                     buf.data_ptr() + 4 * band)
        assert (buf[:band] == sentinel).all() and (buf[-band:] == sentinel).all(), (entry, "wrote outside its output")
        inside = buf[band:-band]
        assert not (inside == sentinel).any(), (entry, int((inside == sentinel).sum()), "elements were not written")
        P.assert_same_bits(inside.reshape(want[entry].shape), want[entry], entry)


@pytest.mark.parametrize("name", ["tiny-3", "soak-54", "dense_corner", "cfg1"])
def test_forward_reproduces_the_image_and_the_accumulated_alpha(name):
    """C = 3 with the frame's own point_color, C = 1 with ones: f32 sums of the same terms as the module's image and 1 - T, in
    another order; each is within IMAGE_TOL of the exact sum."""
    s, q, t, partial, module, inp, outs = _frozen(name)
    frame = module.last_frame
    ids = frame.export("point_id_in_camera_list").long()
    colour = torch.zeros(s.point_cloud.shape[0], 3, device=P.DEV)
    colour[ids] = frame.export("point_color")
    image = module.render_channels(colour).cpu().numpy()
    e = P.rel_err(image, outs[0].cpu().numpy())
    print(f"{name}: image {e:.3g}")
    assert e < 2 * P.IMAGE_TOL
    ones = torch.ones(s.point_cloud.shape[0], 1, device=P.DEV)
    alpha = module.render_channels(ones)[..., 0].cpu().numpy()
    e = P.rel_err(alpha, module.last_forward_outputs["pixel_accumulated_alpha"].cpu().numpy())
    print(f"{name}: accumulated alpha {e:.3g}")
    assert e < 2 * P.IMAGE_TOL


@pytest.mark.parametrize("name", ["tiny-3", "soak-29", "soak-182"])
def test_nan_rows_of_points_outside_the_camera_are_never_read(name):
    s, q, t, partial = SCENES[name]()
    N = s.point_cloud.shape[0]
    s.point_invalid_mask[np.random.default_rng(1).random(N) < 0.2] = 1           # invalid rows are not in the camera either
    module = P.module(partial=partial)
    module(P.make_input(s, q, t, requires_grad=False), keep_frame=True)
    frame = module.last_frame
    in_camera = torch.zeros(N, dtype=torch.bool, device=P.DEV)
    in_camera[frame.export("point_id_in_camera_list").long()] = True
    assert (~in_camera).any()
    rng = np.random.default_rng(2)
    G = _dev(rng.normal(0, 1, (s.height, s.width, 5)).astype(np.float32))
    results = []
    for poison in (False, True):
        v = _dev(rng.normal(0, 1, (N, 5)).astype(np.float32)) if not poison else results[0][2].detach().clone()
        if poison:
            v[~in_camera] = float("nan")
        v.requires_grad_(True)
        out = module.render_channels(v)
        out.backward(G)
        results.append((out.detach(), v.grad, v))
    assert torch.isfinite(results[1][0]).all() and torch.isfinite(results[1][1]).all()
    P.assert_same_bits(results[0][0], results[1][0], "output")
    P.assert_same_bits(results[0][1], results[1][1], "grad_values")
    assert not results[1][1][~in_camera].any()


@pytest.mark.parametrize("name,C", [("soak-54", 7), ("dense_corner", 16), ("cfg1", 64)])
def test_backward_is_bitwise_reproducible(name, C):
    """two runs on one context and one on a fresh context"""
    rng = np.random.default_rng(6)
    grads = []
    for fresh in range(2):
        s, q, t, partial, module, inp, outs = _frozen(name)
        if fresh == 0:
            V = rng.normal(0, 1, (s.point_cloud.shape[0], C)).astype(np.float32)
            G = rng.normal(0, 1, (s.height, s.width, C)).astype(np.float32)
        for _ in range(2 - fresh):
            v = _dev(V).requires_grad_(True)
            module.render_channels(v).backward(_dev(G))
            grads.append(v.grad.cpu().numpy())
    assert np.abs(grads[0]).max() > 0
    P.assert_same_bits(grads[0], grads[1], "second run on the same context")
    P.assert_same_bits(grads[0], grads[2], "fresh context")


def test_channel_pass_leaves_the_image_backward_scratch_alone():
    """image backward, channel backward, image backward on one kept frame: the two image gradients are bit-identical; the same
    with a larger scene's channel pass on the same context in between"""
    s, q, t, partial = P.scene_case("soak", 54)
    module = P.module(partial=partial)
    inp = P.make_input(s, q, t)
    image = module(inp)[0]
    frame = module.last_frame
    rng = np.random.default_rng(9)
    g = _dev(rng.normal(0, 1, tuple(image.shape)).astype(np.float32))

    def image_grads():
        inp.point_cloud.grad = inp.point_cloud_features.grad = None
        image.backward(g, retain_graph=True)
        return inp.point_cloud.grad.clone(), inp.point_cloud_features.grad.clone()

    first = image_grads()
    v = _dev(rng.normal(0, 1, (s.point_cloud.shape[0], 16)).astype(np.float32)).requires_grad_(True)
    module.render_channels(v, frame).square().sum().backward()
    assert v.grad.abs().max() > 0
    second = image_grads()
    big = P.dense_corner_scene()
    big_inp = P.make_input(big, *view_pose(), requires_grad=False)
    module(big_inp, keep_frame=True)
    vb = _dev(rng.normal(0, 1, (big.point_cloud.shape[0], 64)).astype(np.float32)).requires_grad_(True)
    module.render_channels(vb).square().sum().backward()
    assert vb.grad.abs().max() > 0
    third = image_grads()
    for other, what in ((second, "after a channel pass"), (third, "after a larger scene's channel pass")):
        P.assert_same_bits(first[0], other[0], "xyz " + what)
        P.assert_same_bits(first[1], other[1], "features " + what)


def test_autograd_surface():
    s, q, t, partial = P.scene_case("tiny", (3, 56, 0.5, 41, 27))
    N = s.point_cloud.shape[0]
    rng = np.random.default_rng(1)
    V = rng.normal(0, 1, (N, 6)).astype(np.float32)
    # frozen geometry: nothing requires grad, the frame is kept on request
    module = P.module(partial=partial)
    inp = P.make_input(s, q, t, requires_grad=False)
    with torch.no_grad():
        module(inp, keep_frame=True)
    v = _dev(V).requires_grad_(True)
    out = module.render_channels(v)
    assert out.requires_grad
    out.sum().backward()
    once = v.grad.clone()
    assert once.abs().max() > 0
    module.render_channels(v).sum().backward()                    # .grad accumulates over two calls
    assert torch.equal(v.grad, once + once)
    # a non-contiguous view of the values is made contiguous
    wide = _dev(np.concatenate([V, V], axis=1))
    assert torch.equal(module.render_channels(wide[:, :6]), out.detach())
    # together with an image loss in one backward()
    module = P.module(partial=partial)
    inp = P.make_input(s, q, t)
    image = module(inp)[0]
    v = _dev(V).requires_grad_(True)
    (image.sum() + module.render_channels(v).sum()).backward()
    assert torch.equal(v.grad, once)
    assert inp.point_cloud.grad.abs().max() > 0 and inp.point_cloud_features.grad.abs().max() > 0
    # forward only on a transient frame under no_grad
    module = P.module(partial=partial)
    with torch.no_grad():
        module(P.make_input(s, q, t))
        again = module.render_channels(_dev(V).requires_grad_(True))
    assert not again.requires_grad
    assert torch.equal(again, out.detach())


@pytest.mark.parametrize("name", TINY)
def test_values_can_be_fitted_to_a_rendered_target(name):
    """C = 8, true values N(0,1): from zeros, Adam(lr=0.05), 300 steps on the MSE to the rendered target: the loss falls to 1e-2 of
    its start (the float64 reference operator alone reaches 8.9e-5 .. 4.0e-4 on these scenes)."""
    s, q, t, partial, module, inp, outs = _frozen(name)
    rng = np.random.default_rng(5)
    true = _dev(rng.normal(0, 1, (s.point_cloud.shape[0], 8)).astype(np.float32))
    target = module.render_channels(true)
    v = torch.zeros_like(true, requires_grad=True)
    opt = torch.optim.Adam([v], lr=0.05)
    losses = []
    for _ in range(300):
        opt.zero_grad()
        loss = ((module.render_channels(v) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    final = float(((module.render_channels(v.detach()) - target) ** 2).mean())
    print(f"{name}: loss {losses[0]:.4g} -> {final:.4g} ({final / losses[0]:.3g})")
    assert final <= 1e-2 * losses[0]


def test_errors():
    s, q, t, partial, module, inp, outs = _frozen("tiny-0")
    N = s.point_cloud.shape[0]
    good = torch.zeros(N, 4, device=P.DEV)
    for bad in (good.double(), good.int(), torch.zeros(N + 1, 4, device=P.DEV), torch.zeros(N, device=P.DEV),
                torch.zeros(N, 2, 2, device=P.DEV), torch.zeros(N, 4), torch.zeros(N, 0, device=P.DEV), torch.zeros(N, 65, device=P.DEV)):
        with pytest.raises(ValueError):
            module.render_channels(bad)
    # rgb_only: the frame has no `last`
    cfg = P.Rast.GaussianPointCloudRasterisationConfig(rgb_only=True)
    rgb = P.Rast(cfg)
    with torch.no_grad():
        rgb(P.make_input(s, q, t, requires_grad=False))
    with pytest.raises(ValueError):
        rgb.render_channels(good)
    with pytest.raises(ValueError):
        rgb(P.make_input(s, q, t, requires_grad=False), keep_frame=True)
    # requires_grad on a frame that was not kept
    transient = P.module(partial=partial)
    transient(P.make_input(s, q, t, requires_grad=False))
    with pytest.raises(ValueError):
        transient.render_channels(good.clone().requires_grad_(True))
    assert transient.render_channels(good).shape == (s.height, s.width, 4)
    # the library's own argument checks
    from taichi_3d_gaussian_splatting_amd import _native
    frame = module.last_frame
    with pytest.raises(RuntimeError, match="n_channels"):
        _native.call("gs_channels_forward", good.device, frame._context.handle, frame.handle, good.data_ptr(), 65,
                     frame.last.data_ptr(), good.data_ptr())
    # a released frame: the library's state error
    frame.release()
    with pytest.raises(RuntimeError, match="not a live frame"):
        module.render_channels(good, frame)
    # a transient frame that the next forward recycled
    old = transient.last_frame
    transient(P.make_input(s, q, t, requires_grad=False))
    with pytest.raises(RuntimeError, match="not a live frame"):
        transient.render_channels(good, old)
