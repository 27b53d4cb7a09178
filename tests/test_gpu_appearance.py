"""GPU (-m gpu): exposure compensation (include/gs_appearance.h, appearance.py) against tests/appearance_ref.py: apply and the
image gradient bit for bit, the sums within the project's per-element gradient bar, at the shapes where the kernels change
path (one pixel, odd widths, a block of pixels minus, exactly and plus one, more blocks than a finishing block has threads)
and in three layouts (the rasteriser's interleaved view, planar contiguous, a crop of a larger buffer off 16 bytes)."""
import functools

import numpy as np
import pytest
import torch

import appearance_ref as ref
from taichi_3d_gaussian_splatting_amd import appearance
from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P, F = appearance.PIXELS_PER_BLOCK, appearance.FINISH_THREADS
# (H, W): 1 pixel; odd W; P - 1, P and P + 1 pixels; more than F blocks (the finish loops); the trainer tests' frame
SHAPES = [(1, 1), (11, 13), (33, 31), (32, 32), (25, 41), (512, 513), (64, 96)]
LAYOUTS = ["interleaved", "planar", "crop"]
SENTINEL = 7.0
ADAM_C = 3e-3                       # tests/test_gpu_loss_kernels.py: |p - p64| <= ADAM_C S + 4 ulp(p)


def test_the_shapes_are_the_ones_the_kernels_change_path_at():
    pixels = [h * w for h, w in SHAPES]
    assert pixels[:5] == [1, 143, P - 1, P, P + 1] and pixels[5] > F * P and (512 * 513) % 4 == 0 and pixels[6] == 64 * 96
    assert [w % 4 for _, w in SHAPES] == [1, 1, 3, 0, 1, 1, 0]         # planar takes 16-byte loads at 32x32 and 64x96 only


@functools.lru_cache(maxsize=None)
def case(shape):
    """inputs and references of a shape, computed once: x in [0, 1), two upstreams (one-signed, where the terms add up, and
    zero-mean, where they cancel), a transform off the identity, a target and a weight with zeros, negatives and NaN"""
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    c = dict(x=rng.uniform(0.0, 1.0, (3, H, W)).astype(np.float32), y=rng.uniform(0.0, 1.0, (3, H, W)).astype(np.float32),
             M=(np.eye(3, 4) + rng.normal(0.0, 0.2, (3, 4))).astype(np.float32).reshape(12))
    c["g"] = {"one_signed": (np.abs(rng.normal(0.0, 1.0, (3, H, W))) * 1e-3).astype(np.float32),
              "zero_mean": rng.normal(0.0, 1.0, (3, H, W)).astype(np.float32)}
    w = rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)
    flat = w.reshape(-1)
    kind = rng.integers(0, 8, flat.shape[0])
    flat[kind == 0], flat[kind == 1], flat[kind == 2] = 0.0, -0.5, np.nan
    c["w"] = w
    c["apply"] = ref.apply(c["x"], c["M"])
    c["grad_image"] = {k: ref.grad_image(g, c["M"]) for k, g in c["g"].items()}
    c["grad_transform"] = {k: ref.grad_transform(c["x"], g) for k, g in c["g"].items()}
    c["moments"] = {"weighted": ref.moments(c["x"], c["y"], w), "plain": ref.moments(c["x"], c["y"], None)}
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
        assert (view.stride() == (1, 3 * W, 3) or H * W == 1) and view.data_ptr() % 16 == 0      # (one pixel: any strides)
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


def empty(shape, layout):
    return place(np.full((3,) + tuple(shape), SENTINEL, dtype=np.float32), layout)


def untouched_around(view, buf, layout):
    """a crop's surroundings still hold the sentinel"""
    if layout != "crop":
        return True
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(False)
    return bool((buf[outside] == SENTINEL).all())


def bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint64)


def same_bits(t, want):
    return np.array_equal(bits(t), np.ascontiguousarray(want).view(np.uint32))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_apply_is_the_reference_bit_for_bit(shape, layout):
    c = case(shape)
    M = torch.tensor(c["M"], device=DEV)
    x, _ = place(c["x"], layout)
    out = appearance.apply_forward(x, M)
    assert same_bits(out, c["apply"])
    if layout != "crop":
        assert out.stride() == x.stride()                          # preserve_format: the loss reads it where it lies
    # into a buffer of another layout, which keeps what lies around it
    for other in LAYOUTS:
        dst, buf = empty(shape, other)
        appearance.apply_forward(x, M, out=dst)
        assert same_bits(dst, c["apply"]) and untouched_around(dst, buf, other), other
    # in place
    x2, buf = place(c["x"], layout)
    assert appearance.apply_forward(x2, M, out=x2) is x2
    assert same_bits(x2, c["apply"]) and untouched_around(x2, buf, layout)
    # a row of a (V,12) table
    table = torch.zeros(3, 12, device=DEV)
    table[1] = M
    assert same_bits(appearance.apply_forward(x, table[1]), c["apply"])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_backward_against_the_reference(shape, layout):
    c = case(shape)
    M = torch.tensor(c["M"], device=DEV)
    x, _ = place(c["x"], layout)
    for name in ("one_signed", "zero_mean"):
        g, _ = place(c["g"][name], layout)
        gi, buf = empty(shape, layout)
        gt = torch.full((12,), float("nan"), device=DEV)           # garbage: written, not added
        appearance.apply_backward(x, g, M, grad_image=gi, grad_transform=gt)
        assert same_bits(gi, c["grad_image"][name]) and untouched_around(gi, buf, layout)
        want, magnitude = c["grad_transform"][name]
        ok, worst = ref.within_bar(gt.cpu().numpy(), want, magnitude)
        print(f"grad_transform {shape} {layout} {name}: {worst:.3f} of the bar")
        assert ok, (name, worst)
        # the same bits on a second run, and with one output at a time
        gi2, gt2 = appearance.apply_backward(x, g, M)
        assert same_bits(gi2, c["grad_image"][name]) and np.array_equal(bits(gt2), bits(gt))
        only_image, none = appearance.apply_backward(x, g, M, grad_transform=False)
        assert none is None and same_bits(only_image, c["grad_image"][name])
        none, only_transform = appearance.apply_backward(x, g, M, grad_image=False)
        assert none is None and np.array_equal(bits(only_transform), bits(gt))
    # an upstream in another layout than the image: the same image gradient and the same bits in the sums (the last gt is zero_mean's)
    g, _ = place(c["g"]["zero_mean"], LAYOUTS[(LAYOUTS.index(layout) + 1) % 3])
    gi, gt_mixed = appearance.apply_backward(x, g, M)
    assert same_bits(gi, c["grad_image"]["zero_mean"])
    assert np.array_equal(bits(gt_mixed), bits(gt))
    # the image gradient written over the upstream itself
    g, _ = place(c["g"]["zero_mean"], layout)
    appearance.apply_backward(x, g, M, grad_image=g, grad_transform=False)
    assert same_bits(g, c["grad_image"]["zero_mean"])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(11, 13), (25, 41), (64, 96)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_selection_keeps_masked_nan_out(shape, layout):
    c = case(shape)
    H, W = shape
    rng = np.random.default_rng(5)
    masked = rng.random((H, W)) < 0.3
    masked[0, 0] = masked[-1, -1] = True
    g = c["g"]["zero_mean"].copy()
    g[:, masked] = 0.0
    g[1, 0, 0] = -0.0
    x = c["x"].copy()
    x[:, masked] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), (3, int(masked.sum())))
    M = torch.tensor(c["M"], device=DEV)
    gi, gt = appearance.apply_backward(place(x, layout)[0], place(g, layout)[0], M)
    gi, gt = gi.cpu().numpy(), gt.cpu().numpy()
    assert np.all(np.isfinite(gi)) and np.all(np.isfinite(gt))
    assert np.all(gi[:, masked] == 0.0) and not np.any(np.signbit(gi[:, masked]))
    assert same_bits(torch.from_numpy(gi), ref.grad_image(g, c["M"]))
    want, magnitude = ref.grad_transform(x, g)
    assert np.all(np.isfinite(want)) and ref.within_bar(gt, want, magnitude)[0]
    # the same bits as with zeros under the mask: what lies there is not read into a sum
    clean = x.copy()
    clean[:, masked] = 0.0
    assert np.array_equal(bits(appearance.apply_backward(place(clean, layout)[0], place(g, layout)[0], M)[1]), gt.view(np.uint32))
    # no upstream at all: twelve exact zeros, and an image gradient of zeros
    gi0, gt0 = appearance.apply_backward(place(x, layout)[0], place(np.zeros_like(g), layout)[0], M)
    assert np.array_equal(bits(gt0), np.zeros(12, np.uint32)) and np.array_equal(bits(gi0), np.zeros(gi0.numel(), np.uint32).reshape(gi0.shape))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_moments_against_the_reference(shape, layout):
    c = case(shape)
    x, _ = place(c["x"], layout)
    y, _ = place(c["y"], "planar")                      # the trainer's case: a (3,H,W) photograph
    w = torch.tensor(c["w"], device=DEV)
    for name, weight in (("weighted", w), ("plain", None)):
        got = appearance.moments(x, y, weight)
        assert got.dtype == torch.float64 and tuple(got.shape) == (23,)
        want, magnitude = c["moments"][name]
        ok, worst = ref.within_bar(got.cpu().numpy().astype(np.float32), want, magnitude)
        print(f"moments {shape} {layout} {name}: {worst:.3f} of the bar")
        assert ok, (name, worst)
        assert np.array_equal(bits(appearance.moments(x, y, weight)), bits(got))              # the same bits again
        assert got[9].item() == got[22].item()                                                # sum w 1 1 and sum w
    # the target in the image's layout, and a weight off 16 bytes
    y2, _ = place(c["y"], layout)
    w2 = torch.zeros(w.numel() + 1, device=DEV)[1:].view_as(w).copy_(w)
    assert w2.data_ptr() % 16 != 0 and w2.is_contiguous()
    assert np.array_equal(bits(appearance.moments(x, y2, w2)), bits(appearance.moments(x, y, w)))         # no result depends on a layout
    # what lies under a zero, negative or NaN weight is not read into a sum
    dirty_x, dirty_y = c["x"].copy(), c["y"].copy()
    with np.errstate(invalid="ignore"):
        off = ~(c["w"] > 0)
    dirty_x[:, off], dirty_y[:, off] = np.nan, np.inf
    got = appearance.moments(place(dirty_x, layout)[0], place(dirty_y, "planar")[0], w)
    assert np.array_equal(bits(got), bits(appearance.moments(x, y, w)))
    # no weight anywhere: zeros, and the fit is the identity
    nothing = torch.full_like(w, -1.0)
    assert np.array_equal(bits(appearance.moments(x, y, nothing)), np.zeros(23, np.uint64))
    assert appearance.fit_affine(x, y, nothing).cpu().tolist() == list(appearance.IDENTITY)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_fit_affine_recovers_a_planted_transform(layout):
    c = case((64, 96))
    x, _ = place(c["x"], layout)
    M = torch.tensor(c["M"], device=DEV)
    y = appearance.apply_forward(x, M).contiguous()
    fit = appearance.fit_affine(x, y)
    assert fit.dtype == torch.float32 and fit.device == x.device and tuple(fit.shape) == (12,)
    # y is M u rounded to f32 (relative 6e-8 per operation) and the fit is rounded to f32: 1e-5 leaves two decades
    assert (fit - M).abs().max().item() < 1e-5
    fit_w = appearance.fit_affine(x, y, torch.tensor(c["w"], device=DEV))
    assert (fit_w - M).abs().max().item() < 1e-5
    # a constant image: singular, the identity
    flat, _ = place(np.full((3, 64, 96), 0.25, dtype=np.float32), layout)
    assert appearance.fit_affine(flat, y).cpu().tolist() == list(appearance.IDENTITY)


def test_autograd_through_the_loss_equals_the_direct_calls():
    H, W = 24, 20
    gen = torch.Generator(device=DEV).manual_seed(3)
    base = torch.rand(H, W, 3, device=DEV, generator=gen).mul_(1.2).sub_(0.1).requires_grad_(True)      # some values outside [0, 1]
    target = torch.rand(3, H, W, device=DEV, generator=gen)
    table = appearance.AppearanceTable(3, DEV)
    table.transforms[1] = torch.tensor(case((64, 96))["M"], device=DEV)
    table.grad.fill_(float("nan"))
    loss_fn = LossFunction(LossFunction.LossFunctionConfig(enable_regularization=False))
    row = table.row(1)
    assert row.is_leaf and row.requires_grad and row.data_ptr() == table.transforms[1].data_ptr() and row.data_ptr() % 16 == 0
    corrected = appearance.apply(base.permute(2, 0, 1), row)
    assert corrected.stride() == (1, 3 * W, 3) and corrected.requires_grad
    L = loss_fn(corrected, target, clamp_predicted=True)[0]
    L.backward()
    # the direct calls: the loss's gradient with respect to the corrected image, then gs_appearance_backward
    leaf = appearance.apply_forward(base.detach().permute(2, 0, 1), table.transforms[1]).requires_grad_(True)
    assert torch.equal(leaf, corrected)
    L2 = loss_fn(leaf, target, clamp_predicted=True)[0]
    L2.backward()
    assert L2.item() == L.item()
    gi, gt = appearance.apply_backward(base.detach().permute(2, 0, 1), leaf.grad, table.transforms[1])
    assert base.grad is not None and torch.equal(base.grad, gi.permute(1, 2, 0)) and bool(base.grad.any())
    assert row.grad is not None and torch.equal(row.grad, gt) and bool(gt.any())
    assert row.grad.data_ptr() == table.grad[1].data_ptr() and torch.equal(table.grad[1], gt)       # it landed in the table
    assert bool(torch.isnan(table.grad[0]).all()) and bool(torch.isnan(table.grad[2]).all())        # and nowhere else
    # an ordinary (12,) leaf gets its gradient the ordinary way, accumulated
    free = table.transforms[1].clone().requires_grad_(True)
    for _ in range(2):
        loss_fn(appearance.apply(base.detach().permute(2, 0, 1), free), target, clamp_predicted=True)[0].backward()
    assert torch.equal(free.grad, gt + gt)
    # image only: a transform that needs no gradient
    image = base.detach().clone().requires_grad_(True)
    loss_fn(appearance.apply(image.permute(2, 0, 1), table.transforms[1]), target, clamp_predicted=True)[0].backward()
    assert torch.equal(image.grad, base.grad)


def _ulp(x):
    a = x.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def test_table_step_moves_one_row_like_adam(tmp_path):
    V, v = 5, 2
    config = appearance.AppearanceConfig(num_iterations=40)
    table = appearance.AppearanceTable(V, DEV, config)
    assert table.transforms.cpu().tolist() == [list(appearance.IDENTITY)] * V and table.steps == [0] * V
    gen = torch.Generator(device=DEV).manual_seed(9)
    table.transforms.add_(torch.randn(V, 12, device=DEV, generator=gen) * 0.1)
    table.grad.copy_(torch.randn(V, 12, device=DEV, generator=gen))                # other rows hold gradients too: they are not used
    before = {name: getattr(table, name).clone() for name in ("transforms", "exp_avg", "exp_avg_sq")}
    p64 = table.transforms[v].double().clone().requires_grad_(True)
    adam = torch.optim.Adam([p64], lr=config.lr, betas=config.betas, eps=config.eps)
    S = torch.zeros(12, dtype=torch.float64, device=DEV)
    iterations = [0, 7, 8, 20, 39]                                                   # the view comes up now and then
    for step, iteration in enumerate(iterations, 1):
        g = torch.randn(12, device=DEV, generator=gen) * torch.tensor([1.0, 1e-3, 10.0] * 4, device=DEV)
        table.grad[v] = g
        table.step(v, iteration)
        assert table.steps[v] == step
        for group in adam.param_groups:
            group["lr"] = ref.lr_at(iteration, config.lr, config.lr_final, config.num_iterations)
        p64.grad = g.double()
        last = p64.detach().clone()
        adam.step()
        S += (p64.detach() - last).abs()
    others = [i for i in range(V) if i != v]
    for name, tensor in before.items():
        assert torch.equal(getattr(table, name)[others], tensor[others]), name
        assert not torch.equal(getattr(table, name)[v], tensor[v]), name
    assert table.steps == [0, 0, 5, 0, 0]
    err = (table.transforms[v].double() - p64.detach()).abs() - 4 * _ulp(p64.detach())
    used = (err / S).max().item()
    print(f"table step: {used / ADAM_C:.3f} of the Adam bar")
    assert bool((S > 0).all()) and used <= ADAM_C
    # save / load
    paths = [f"images/view_{i}.png" for i in range(V)]
    table.save(str(tmp_path / "appearance.pt"), paths)
    loaded, loaded_paths = appearance.AppearanceTable.load(str(tmp_path / "appearance.pt"), DEV)
    assert loaded_paths == paths and loaded.steps == table.steps and loaded.num_views == V
    for name in before:
        assert torch.equal(getattr(loaded, name), getattr(table, name)), name
    assert loaded.transforms.device == table.transforms.device
    assert torch.equal(loaded.by_image_path(paths)["images/view_2.png"], table.transforms[v])
    with pytest.raises(ValueError, match="image paths"):
        table.save(str(tmp_path / "bad.pt"), paths[:-1])
    with pytest.raises(IndexError):
        table.row(V)
