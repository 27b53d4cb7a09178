"""GPU (-m gpu): the background behind the splats (include/gs_background.h, background.py) against tests/background_ref.py, bit
for bit: the composite in its three modes, grad_alpha and grad_coef, at bands 0..3, at the shapes where the kernels change path
(one pixel, an odd width, a block of pixels exactly and plus one, more blocks than a finishing block has threads) and in three
layouts (the rasteriser's interleaved view, planar contiguous, a crop of a larger buffer off 16 bytes); then through the
rasteriser against the same chain in torch operations."""
import functools

import numpy as np
import pytest
import torch

import background_ref as ref
import parity_util as PU
from oracle import oracle
from taichi_3d_gaussian_splatting_amd import background

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P, F = background.PIXELS_PER_BLOCK, background.FINISH_THREADS
# (H, W): 1 pixel; the scalar path with W % 4 != 0; P and P + 1 pixels; more than P F pixels (a finishing thread loops)
SHAPES = [(1, 1), (5, 7), (32, 32), (25, 41), (272, 1000)]
BANDS = [0, 1, 2, 3]
LAYOUTS = ["interleaved", "planar", "crop"]
SENTINEL = 7.0


def test_the_shapes_are_the_ones_the_kernels_change_path_at():
    pixels = [h * w for h, w in SHAPES]
    assert pixels[:4] == [1, 35, P, P + 1] and pixels[4] > P * F and pixels[4] // P + 1 < 2 * F
    assert [w % 4 for _, w in SHAPES] == [1, 3, 0, 1, 0]           # planar takes 16-byte loads at 32x32 and 272x1000


@functools.lru_cache(maxsize=None)
def case(shape, bands):
    """inputs and references of a shape and a band count, computed once: an off-centre camera with fx != fy, a quaternion
    that is not unit, alpha in [0, 1] with exact zeros and ones, a zero-mean upstream with unselected pixels"""
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W + 7 * bands)
    c = dict(x=rng.uniform(0.0, 1.0, (3, H, W)).astype(np.float32), coef=rng.normal(0.0, 0.5, 48).astype(np.float32))
    A = rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)
    kind = rng.integers(0, 6, (H, W))
    A[kind == 0], A[kind == 1] = 0.0, 1.0
    A[0, 0] = 0.25
    q = rng.normal(0.0, 1.0, 4)
    c["q"] = (q / np.linalg.norm(q) * 1.25).astype(np.float32)
    c["K"] = ref.camera(H, W, fx=0.8 * max(W, 4), fy=1.1 * max(W, 4), cx=0.37 * W, cy=0.58 * H)
    g = rng.normal(0.0, 1.0, (3, H, W)).astype(np.float32)
    g[:, rng.integers(0, 5, (H, W)) == 0] = 0.0
    g[:, 0, 0] = [0.5, -0.25, 0.75]                                  # the first pixel is selected: the one-pixel image has a gradient
    c["A"], c["g"] = A, g
    cam = (c["q"], c["K"])
    c["out"] = {flags: ref.composite(c["x"], A, c["coef"], bands, *cam, flags) for flags in (0, ref.STRAIGHT)}
    c["colours"] = ref.colours(c["coef"], bands, *cam, H, W)
    c["grad_alpha"] = ref.grad_alpha(g, c["coef"], bands, *cam)
    c["grad_coef"] = ref.grad_coef(g, A, bands, *cam)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def place(a, layout, fill=SENTINEL):
    """a (3,H,W) numpy image on the device in a layout -> (the (3,H,W) view, the buffer it lies in)"""
    t = torch.tensor(np.asarray(a), device=DEV)
    _, H, W = t.shape
    if layout == "interleaved":
        buf = t.permute(1, 2, 0).contiguous()
        view = buf.permute(2, 0, 1)
        assert (view.stride() == (1, 3 * W, 3) or H * W == 1) and view.data_ptr() % 16 == 0
    elif layout == "planar":
        buf = view = t.contiguous()
        assert view.data_ptr() % 16 == 0
    else:
        buf = torch.full((3, H + 3, W + 6), fill, dtype=torch.float32, device=DEV)
        view = buf[:, 2:2 + H, 1:1 + W]
        if view.data_ptr() % 16 == 0:
            view = buf[:, 2:2 + H, 2:2 + W]
        assert view.data_ptr() % 16 != 0 and not view.is_contiguous()
        view.copy_(t)
    return view, buf


def place_plane(a, layout, fill=SENTINEL):
    """an (H,W) plane, contiguous as the header wants it; for "crop" at a base that is off 16 bytes -> (view, buffer)"""
    a = np.asarray(a)
    H, W = a.shape
    if layout != "crop":
        t = torch.tensor(a, device=DEV)
        assert t.data_ptr() % 16 == 0
        return t, t
    buf = torch.full((H * W + 8,), fill, dtype=torch.float32, device=DEV)
    view = buf[1:1 + H * W].view(H, W)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    view.copy_(torch.tensor(a, device=DEV))
    return view, buf


def untouched_around(view, buf):
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(False)
    return bool((buf[outside] == SENTINEL).all())


def bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def same_bits(t, want):
    return np.array_equal(bits(t), np.ascontiguousarray(want).view(np.uint32))


def on_device(c):
    return (torch.tensor(c["coef"], device=DEV), torch.tensor(c["q"], device=DEV), torch.tensor(c["K"], device=DEV))


@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_composite_is_the_reference_bit_for_bit(shape, bands):
    c = case(shape, bands)
    coef, q, K = on_device(c)
    H, W = shape
    assert same_bits(background.colours(coef, bands, q, K, H, W), c["colours"])
    for layout in LAYOUTS:
        x, _ = place(c["x"], layout)
        A, _ = place_plane(c["A"], layout)
        out = background.composite_forward(x, A, coef, bands, q, K)
        assert same_bits(out, c["out"][0]), layout
        if layout != "crop":
            assert out.stride() == x.stride()                      # preserve_format: the loss reads it where it lies
        assert same_bits(background.composite_forward(x, A, coef, bands, q, K, straight=True), c["out"][ref.STRAIGHT]), layout
        rgba = torch.cat([x, A[None]]).contiguous()
        assert same_bits(background.composite_straight(rgba, coef, bands, q, K), c["out"][ref.STRAIGHT]), layout
        # into a buffer of the next layout, which keeps what lies around it; then in place
        other = LAYOUTS[(LAYOUTS.index(layout) + 1) % 3]
        dst, buf = place(np.full((3, H, W), SENTINEL, dtype=np.float32), other)
        background.composite_forward(x, A, coef, bands, q, K, out=dst)
        assert same_bits(dst, c["out"][0]) and (other != "crop" or untouched_around(dst, buf)), (layout, other)
        x2, buf = place(c["x"], layout)
        assert background.composite_forward(x2, A, coef, bands, q, K, out=x2) is x2
        assert same_bits(x2, c["out"][0]) and (layout != "crop" or untouched_around(x2, buf)), layout
    if bands == 0:                                                  # a solid colour reads no camera
        assert same_bits(background.composite_forward(x, A, coef, 0), c["out"][0])
        assert same_bits(background.colours(coef, 0, None, None, H, W), c["colours"])


@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_backward_is_the_reference_bit_for_bit(shape, bands):
    c = case(shape, bands)
    coef, q, K = on_device(c)
    for layout in LAYOUTS:
        g, _ = place(c["g"], layout)
        A, _ = place_plane(c["A"], layout)
        ga, buf = place_plane(np.full(shape, SENTINEL, dtype=np.float32), layout)
        gc = torch.full((48,), float("nan"), device=DEV)           # garbage: written, not added
        background.composite_backward(g, A, coef, bands, q, K, grad_alpha=ga, grad_coef=gc)
        assert same_bits(ga, c["grad_alpha"]), layout
        assert layout != "crop" or untouched_around(ga, buf)
        assert same_bits(gc, c["grad_coef"]), (layout, gc.cpu().numpy(), c["grad_coef"])
        # the same bits on a second run, and with one output at a time
        ga2, gc2 = background.composite_backward(g, A, coef, bands, q, K)
        assert same_bits(ga2, c["grad_alpha"]) and same_bits(gc2, c["grad_coef"])
        only_alpha, none = background.composite_backward(g, A, coef, bands, q, K, grad_coef=False)
        assert none is None and same_bits(only_alpha, c["grad_alpha"])
        none, only_coef = background.composite_backward(g, A, coef, bands, q, K, grad_alpha=False)
        assert none is None and same_bits(only_coef, c["grad_coef"])
    Kn = (bands + 1) ** 2
    want = c["grad_coef"].reshape(3, 16)
    assert not want[:, Kn:].any() and not np.signbit(want[:, Kn:]).any() and np.all(want[:, :Kn] != 0.0)


def test_selection_keeps_alpha_out_of_unselected_pixels():
    shape, bands = (25, 41), 3
    c = case(shape, bands)
    coef, q, K = on_device(c)
    g, A = c["g"].copy(), c["A"].copy()
    unselected = ~ref.selected(g)
    assert unselected.sum() > 50
    ys, xs = np.nonzero(unselected)
    A[ys[0::3], xs[0::3]] = np.nan
    A[ys[1::3], xs[1::3]] = np.inf
    g[:, ys[2], xs[2]] = [0.0, -0.0, 0.0]                            # -0 is 0
    for layout in LAYOUTS:
        gd, _ = place(g, layout)
        Ad, _ = place_plane(A, layout)
        ga, gc = background.composite_backward(gd, Ad, coef, bands, q, K)
        assert same_bits(gc, c["grad_coef"]), layout                  # not a bit of the sums changes
        assert same_bits(ga, c["grad_alpha"]) and not bits(ga)[unselected].any()         # exactly +0
    # a NaN upstream is selected and shows
    ys, xs = np.nonzero(~unselected)
    g[1, ys[0], xs[0]] = np.nan
    gd, _ = place(g, "interleaved")
    ga, gc = background.composite_backward(gd, torch.tensor(c["A"], device=DEV), coef, bands, q, K)
    ga, gc = ga.cpu().numpy(), gc.cpu().numpy().reshape(3, 16)
    assert np.isnan(ga[ys[0], xs[0]]) and np.isnan(ga).sum() == 1
    assert np.all(np.isnan(gc[1])) and np.all(np.isfinite(gc[0])) and np.all(np.isfinite(gc[2]))


def test_autograd_node_returns_the_three_gradients():
    shape, bands = (25, 41), 2
    c = case(shape, bands)
    coef, q, K = on_device(c)
    x, _ = place(c["x"], "interleaved")
    x.requires_grad_(True)
    A = torch.tensor(c["A"], device=DEV, requires_grad=True)
    coef.requires_grad_(True)
    g, _ = place(c["g"], "interleaved")
    out = background.composite(x, A, coef, bands, q[None], K)
    assert same_bits(out, c["out"][0])
    out.backward(g)
    assert same_bits(x.grad, c["g"]) and same_bits(A.grad, c["grad_alpha"]) and same_bits(coef.grad, c["grad_coef"])
    # a model's coefficients have the gradient written into the model, and a fixed colour takes none
    model = background.BackgroundModel("sky", DEV, background.BackgroundConfig(bands=bands))
    model.coef.copy_(torch.tensor(c["coef"], device=DEV))
    model.grad.fill_(float("nan"))
    leaf = model.coef_for_step()
    A2 = torch.tensor(c["A"], device=DEV, requires_grad=True)
    background.composite(x.detach(), A2, leaf, model.bands, q, K).backward(g)
    assert leaf.grad.data_ptr() == model.grad.data_ptr() and same_bits(model.grad, c["grad_coef"]) and same_bits(A2.grad, c["grad_alpha"])
    before = model.coef.clone()
    model.step(0)
    moved = (model.coef != before).cpu().numpy().reshape(3, 16)
    assert moved[:, :9].all() and not moved[:, 9:].any()
    fixed = background.BackgroundModel("colour", DEV, background.BackgroundConfig(colour=(1.0, 1.0, 1.0)))
    assert fixed.bands == 0 and not fixed.coef_for_step().requires_grad and same_bits(fixed.coef, ref.WHITE)
    random_model = background.BackgroundModel("random", DEV, background.BackgroundConfig(colour=(1.0, 1.0, 1.0), seed=3))
    a = random_model.coef_for_step().clone()
    b = random_model.coef_for_step().clone()
    again = background.BackgroundModel("random", DEV, background.BackgroundConfig(seed=3)).coef_for_step()
    assert not torch.equal(a, b) and torch.equal(a, again) and same_bits(random_model.coef, ref.WHITE)
    assert bool(((a.view(3, 16)[:, 0] >= 0) & (a.view(3, 16)[:, 0] < 1)).all()) and not a.view(3, 16)[:, 1:].any()


def test_save_and_load(tmp_path):
    model = background.BackgroundModel("sky", DEV, background.BackgroundConfig(bands=1, colour=(0.2, 0.3, 0.4)))
    model.grad.normal_(generator=torch.Generator(device=DEV).manual_seed(0))
    model.step(5)
    path = str(tmp_path / "background.pt")
    model.save(path)
    back = background.BackgroundModel.load(path, DEV)
    assert (back.kind, back.bands, back.steps) == ("sky", 1, 1)
    for name in ("coef", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(back, name), getattr(model, name)), name


def test_through_the_rasteriser_against_torch_operations():
    """Rast(..., return_accumulated_alpha=True) -> composite -> a sum against random weights -> backward, against the same
    chain with the compositing written in torch operations on background.colours().  The point gradients are held to
    parity_util's per-element bar, 2e-5 |ref| + 5e-6 S, with S the magnitude the CPU checker sums for the image upstream alone
    (the alpha upstream only adds to it: a smaller S is the stricter bar); the images are equal bit for bit."""
    bands = 2
    s, qn, tn, partial = PU.tiny_case(1, 64, 0.6, 32, 32)
    rng = np.random.default_rng(5)
    coef = torch.tensor(rng.uniform(0.1, 0.6, 48).astype(np.float32), device=DEV)
    weights = PU.upstream((3, s.height, s.width), 11)
    module = PU.module(partial, **PU.UNIT_FACTORS)
    got = {}
    for name in ("native", "torch"):
        inp = PU.make_input(s, qn, tn)
        image, _, _, alpha = module(inp, return_accumulated_alpha=True)
        K, q = inp.camera_info.camera_intrinsics, inp.q_pointcloud_camera
        if name == "native":
            out = background.composite(image.permute(2, 0, 1), alpha, coef, bands, q, K)
        else:
            out = image.permute(2, 0, 1) + (1.0 - alpha) * background.colours(coef, bands, q.detach(), K, s.height, s.width)
        (out * weights).sum().backward()
        got[name] = (out.detach(), inp.point_cloud.grad.cpu().numpy(), inp.point_cloud_features.grad.cpu().numpy())
    assert np.array_equal(bits(got["native"][0]), bits(got["torch"][0]))
    assert float((1.0 - alpha.detach()).max()) > 0.5 and float(alpha.detach().max()) > 0.5          # the background shows, and so do the splats
    f, _ = PU.oracle_frame(s, qn, tn, partial)
    b = oracle.backward(f, weights.permute(1, 2, 0).contiguous().cpu().numpy(), 3, PU.oracle_config(partial, **PU.UNIT_FACTORS), want_summed=True)
    for k, summed in ((1, b["summed_pointcloud"]), (2, b["summed_pointcloud_features"])):
        a, want = got["native"][k].astype(np.float64), got["torch"][k].astype(np.float64)
        assert np.abs(want).max() > 0
        bound = PU.ELEM_RTOL * np.abs(want) + PU.ELEM_FLOOR * summed
        worst = float((np.abs(a - want) / np.maximum(bound, 1e-300)).max())
        print(f"gradient {k}: largest |difference| {np.abs(a - want).max():.3e}, {worst:.3f} of the bar")
        assert np.all(np.abs(a - want) <= bound)
