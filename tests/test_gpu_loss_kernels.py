"""GPU (-m gpu): the kernels of k_loss.hip that run on every training iteration after the rasteriser -- fused L1+SSIM
forward and backward, the scale regulariser, Adam -- held to the float64 references of tests/loss_ref.py at the shapes,
layouts and values where such kernels go wrong; and the backward's tagged `visited` buffer under growth.

With GS_LOSS_MARGINS_OUT=<path> set, the share of every bar that the run used is written there as JSON
(profiles/loss_margins.json holds a recorded run)."""
import gc
import json
import os

import numpy as np
import pytest
import torch

import loss_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32

# Per-element bar of the loss gradient: |g - g64| <= 1e-4 |g64| + C_LOSS m, m = loss_ref.grad_magnitude (the derivative chain
# with every term taken by its absolute value).  The kernel's own rounding is a few f32 eps (6e-8) per term of that chain;
# on top, s = E[x^2] - mu^2 cancels in f32 against C2 = 9e-4, which in flat, bright regions scales the error of A, B, D by up
# to E[x^2] / C2 ~ 1e3.  Random content uses ~1e-7; flat images, where the large terms of dS (~1/C2 each) cancel and m is
# ~1e3 times |dS|, stay below 6e-8.  Largest use measured 1.24e-7 (lambda = 1, 41x60; profiles/loss_margins.json).
# C_LOSS is four times that.
C_LOSS = 5e-7
TERM_TOL = 2e-6           # L and LD (L1: 1e-6) against float64, as tests/test_gpu_trainer_step.py
# LD of a constant image: every map pixel carries the same f32 error of E[y^2] - mu^2 (~1e-7 of 0.49) against C2 = 9e-4,
# a systematic ~5e-5 of SSIM that no averaging removes (measured 4.2e-5 at 0.3 against 0.7).  Inherent in the one-pass
# E[x^2] - mu^2 form that pytorch_msssim uses as well; random content stays within TERM_TOL.  For the same reason the
# gradient of a constant image misses the tensor-level 1e-4 (1.1e-4 measured) and is held to the per-element bar alone.
TERM_TOL_FLAT = 2e-4
REG_RTOL = 1e-5           # regulariser value and each gradient element against float64
# Adam: |p - p64| <= ADAM_C S + 4 ulp(p), S = sum over steps of lr_t |m_hat / (sqrt(v_hat) + eps)| (Adam64.S).  An f32 update
# is a few eps off per step, and the f32 parameter itself is rounded at every step (random walk of ~sqrt(steps) half-ulps,
# which in late steps with a decayed lr is a sizeable part of the update); ADAM_C is three times the largest use measured
# (7.6e-4, 28e6 elements at betas (0.9, 0.999)).
ADAM_C = 3e-3

MARGINS = {}


def _record(key, used):
    MARGINS[key] = max(float(used), MARGINS.get(key, 0.0))


@pytest.fixture(scope="module", autouse=True)
def _write_margins():
    yield
    out = os.environ.get("GS_LOSS_MARGINS_OUT")
    if out:
        with open(out, "w") as fh:
            json.dump({"C_LOSS": C_LOSS, "REG_RTOL": REG_RTOL, "ADAM_C": ADAM_C,
                       "used": dict(sorted(MARGINS.items()))}, fh, indent=1)


# ----------------------------------------------------------------------------------------------------------------------
# L1 + SSIM

def _l1ssim():
    from taichi_3d_gaussian_splatting_amd.LossFunction import _L1SSIM
    return _L1SSIM


def run_loss(pred, gt, lam=0.2, clamp=False, up=1.0):
    """(terms, dL/dpred * up) of the fused kernels for a (3,H,W) pred view of any strides; the gradient as (3,H,W) values."""
    p = pred.detach().requires_grad_(True)          # a leaf with pred's storage, offset and strides
    L, terms = _l1ssim().apply(p, gt, lam, clamp)
    L.backward(torch.tensor(up, dtype=F32, device=DEV))
    torch.cuda.synchronize()
    return terms.detach().clone(), p.grad.clone()


def check_loss(pred, gt, terms, grad, lam, clamp, up, key, term_tol=TERM_TOL, tensor_bar=True):
    """Terms within term_tol of float64; every gradient element within its bar; the tensor-level 1e-4 as well (not where the
    exact gradient is zero and the float64 one is rounding noise)."""
    pc, gc_ = pred.detach().cpu(), gt.detach().cpu()
    L64, l1_64, ld64, g64 = loss_ref.l1_ssim_ref(pc, gc_, lam, clamp, up)
    t = terms.double().cpu()
    assert abs(t[1] - l1_64).item() < 1e-6 and abs(t[2] - ld64).item() < term_tol and abs(t[0] - L64).item() < term_tol, \
        (t.tolist(), L64.item(), l1_64.item(), ld64.item())
    m = loss_ref.grad_magnitude(pc, gc_, lam, clamp, up)
    g = grad.double().cpu()
    excess = (g - g64).abs() - 1e-4 * g64.abs()
    zero_m = m == 0
    assert torch.equal(g[zero_m], g64[zero_m]), "a gradient the reference has as exact zero is not zero"
    used = (excess[~zero_m] / m[~zero_m]).max().item() if (~zero_m).any() else 0.0
    _record(key, used / C_LOSS)
    assert used <= C_LOSS, (key, used)
    ref_max = g64.abs().max().item()
    if tensor_bar and ref_max > 0:
        assert (g - g64).abs().max().item() <= 1e-4 * ref_max


def _content(H, W, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    gt = torch.rand(3, H, W, device=DEV, generator=gen)
    pred = (gt + 0.2 * torch.randn(3, H, W, device=DEV, generator=gen)).clamp(0, 1)
    return pred, gt


SIZES = [(11, 11), (11, 300), (300, 11), (12, 12), (21, 31), (22, 32), (23, 33), (53, 63), (54, 64), (55, 65), (1080, 1920),
         (1500, 13), (13, 2000)]


@pytest.mark.parametrize("H,W", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_loss_size_sweep_against_float64(H, W):
    """Forward tiles are 32 x GS_LOSS_MTY (22), backward tiles 32 x 54, the maps padded by 10 rows and 12 columns: sizes
    at the window (11), at 22k+-1, 32k+-1, 54k+-1, tall-narrow, short-wide and true 1080 rows."""
    pred, gt = _content(H, W, H * 7919 + W)
    terms, grad = run_loss(pred, gt, 0.2, False, 1.0)
    check_loss(pred, gt, terms, grad, 0.2, False, 1.0, f"loss/size/{H}x{W}")


def _edge_case(name, H, W):
    gen = torch.Generator(device=DEV).manual_seed(len(name))
    rnd = lambda: torch.rand(3, H, W, device=DEV, generator=gen)
    lam, clamp, up = 0.2, False, 1.0
    if name == "constant_equal":
        pred, gt = torch.full((3, H, W), 0.5, device=DEV), torch.full((3, H, W), 0.5, device=DEV)
    elif name == "constant_different":
        pred, gt = torch.full((3, H, W), 0.3, device=DEV), torch.full((3, H, W), 0.7, device=DEV)
    elif name == "constant_zero_and_one":
        pred, gt = torch.zeros(3, H, W, device=DEV), torch.ones(3, H, W, device=DEV)
    elif name == "pred_equals_gt":
        gt = rnd()
        pred = gt.clone()
    elif name == "saturated_regions":
        gt = rnd()
        gt[:, : H // 2, : W // 3] = 0.0
        gt[:, H // 3:, W // 2:] = 1.0
        pred = (gt + 0.3 * (rnd() - 0.5)).clamp(0, 1)
        pred[:, : H // 4] = 1.0
    elif name == "checkerboard":
        yy, xx = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
        cb = ((yy + xx) % 2).float().expand(3, H, W).contiguous()
        pred, gt = cb, 0.25 + 0.5 * rnd()
    elif name in ("outside_range", "outside_range_clamped"):
        gt = rnd()
        pred = gt * 1.6 - 0.3
        pred[0, :3, :5], pred[1, 4, :7], pred[2, -2:, -3:] = 0.0, 1.0, 0.0          # the closed ends, exactly
        clamp = name.endswith("clamped")
    elif name == "lambda_one":
        pred, gt = _content(H, W, 3)
        lam = 1.0
    elif name == "upstream_negative":
        pred, gt = _content(H, W, 4)
        up = -1.7
    else:
        raise KeyError(name)
    return pred.contiguous(), gt.contiguous(), lam, clamp, up


EDGES = ["constant_equal", "constant_different", "constant_zero_and_one", "pred_equals_gt", "saturated_regions", "checkerboard",
         "outside_range", "outside_range_clamped", "lambda_one", "upstream_negative"]


@pytest.mark.parametrize("H,W", [(41, 60), (37, 45)], ids=["41x60", "37x45"])
@pytest.mark.parametrize("name", EDGES)
def test_loss_content_edges_against_float64(name, H, W):
    pred, gt, lam, clamp, up = _edge_case(name, H, W)
    terms, grad = run_loss(pred, gt, lam, clamp, up)
    flat = name.startswith("constant")
    check_loss(pred, gt, terms, grad, lam, clamp, up, f"loss/edge/{name}/{H}x{W}", TERM_TOL_FLAT if flat else TERM_TOL,
               tensor_bar=not flat and name != "pred_equals_gt")
    if name == "outside_range_clamped":
        outside = (pred < 0) | (pred > 1)
        ends = (pred == 0) | (pred == 1)
        assert outside.float().mean() > 0.1 and not grad[outside].any()
        assert ends.sum() >= 20 and (grad[ends] != 0).all(), "torch.clamp passes the gradient at min and max"
    if name == "pred_equals_gt":
        assert terms[1].item() == 0.0
        t0, g0 = run_loss(pred, gt, 0.0, False, 1.0)           # no SSIM part: sign(0) = 0 leaves nothing
        assert t0[0].item() == 0.0 and not g0.any()


@pytest.mark.parametrize("H,W", [(41, 60), (37, 45), (1080, 1920)], ids=["41x60", "37x45", "1080x1920"])
def test_loss_lambda_zero_gradient_is_exactly_the_l1_sign(H, W):
    """lambda = 0: k_ssim = 0, the gradient must be up * (k_l1 * sign(x - y)) bit for bit, with k_l1 = 1 / (3 H W) in f32."""
    pred, gt = _content(H, W, 11)
    pred[0, 0, :5] = gt[0, 0, :5]                                                  # sign(0) = 0
    up = torch.tensor(-0.8, dtype=F32, device=DEV)
    terms, grad = run_loss(pred, gt, 0.0, False, -0.8)
    k_l1 = torch.tensor(1.0, dtype=F32, device=DEV) / (torch.tensor(3.0, dtype=F32, device=DEV) * H * W)
    assert torch.equal(grad, up * (k_l1 * torch.sign(pred - gt)))
    check_loss(pred, gt, terms, grad, 0.0, False, -0.8, f"loss/lambda0/{H}x{W}")


def test_loss_zero_upstream_gives_exact_zeros():
    pred, gt = _content(54, 64, 12)
    terms, grad = run_loss(pred, gt, 0.2, False, 0.0)
    assert bool((grad == 0).all())
    t1, _ = run_loss(pred, gt, 0.2, False, 1.0)
    assert torch.equal(terms, t1)


@pytest.mark.parametrize("clamp", [False, True], ids=["raw", "clamped"])
def test_loss_nan_pixel_propagates_like_torch(clamp):
    """A NaN pixel of the prediction: the loss terms are NaN, and the gradient is NaN exactly where torch's is -- the pixels
    whose 21x21 neighbourhood (two window widths) holds it -- and within its bar elsewhere.  (torch's abs backward gives
    sign(NaN) = 0; the kernel's sign test gives 0 as well; the NaN at the pixel comes through the SSIM part.  Clamped, the
    pixel itself gets 0 in both: torch.clamp's backward passes nothing where min <= x <= max is false, and so does the kernel.)"""
    H, W = 60, 72
    pred, gt = _content(H, W, 13)
    pred[1, 30, 40] = float("nan")
    terms, grad = run_loss(pred, gt, 0.2, clamp, 1.0)
    pc, gc_ = pred.cpu(), gt.cpu()
    L64, l1_64, ld64, g64 = loss_ref.l1_ssim_ref(pc, gc_, 0.2, clamp, 1.0)
    assert bool(torch.isnan(terms).all()) and bool(torch.isnan(L64)) and bool(torch.isnan(ld64)) and bool(torch.isnan(l1_64))
    g = grad.double().cpu()
    nan_k, nan_t = torch.isnan(g), torch.isnan(g64)
    assert torch.equal(nan_k, nan_t), (int(nan_k.sum()), int(nan_t.sum()))
    assert int(nan_t.sum()) == 21 * 21 - int(clamp) and bool(nan_t[1, 20:41, 30:51].sum() == 21 * 21 - int(clamp))
    if clamp:
        assert g[1, 30, 40].item() == 0.0 and g64[1, 30, 40].item() == 0.0
    m = loss_ref.grad_magnitude(pc, gc_, 0.2, clamp, 1.0)
    ok = ~nan_t
    assert bool(((g[ok] - g64[ok]).abs() <= 1e-4 * g64[ok].abs() + C_LOSS * m[ok]).all())


# -- layouts: the same floats through every load path ------------------------------------------------------------------

LAYOUTS = ["chw", "hwc", "hw4", "off1", "rowcrop"]


def make_layout(img, kind):
    """A (3,H,W) view holding img's values: contiguous, the permuted (H,W,3) buffer, [..., :3] of (H,W,4) (pixel stride 4),
    one float off a 16-byte boundary, and rows cropped out of (3,H,W+4) (aligned pointer, row stride W+4)."""
    C_, H, W = img.shape
    if kind == "chw":
        return img.clone().contiguous()
    if kind == "hwc":
        return img.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    if kind == "hw4":
        buf = torch.full((H, W, 4), 7.0, device=DEV)
        buf[..., :3] = img.permute(1, 2, 0)
        return buf[..., :3].permute(2, 0, 1)
    if kind == "off1":
        flat = torch.full((3 * H * W + 4,), 7.0, device=DEV)
        v = flat[1:1 + 3 * H * W].view(3, H, W)
        v.copy_(img)
        return v
    if kind == "rowcrop":
        buf = torch.full((3, H, W + 4), 7.0, device=DEV)
        buf[:, :, :W] = img
        return buf[:, :, :W]
    raise KeyError(kind)


def loss_mode(t):
    """gs_loss_mode of k_loss.hip, restated."""
    sc, sy, sx = t.stride()
    W = t.shape[2]
    aligned = W % 4 == 0 and sy % 4 == 0 and t.data_ptr() % 16 == 0
    if aligned and sx == 1 and sc % 4 == 0:
        return "VEC"
    if aligned and sx == 3 and sc == 1:
        return "VEC3"
    return "SCALAR"


def instantiation(xm, ym):
    """Which k_loss_ssim_maps<XMODE, YMODE> gs_launch_loss_forward picks."""
    if xm == "VEC" and ym == "VEC":
        return "VEC_VEC"
    if xm == "VEC3" and ym == "VEC":
        return "VEC3_VEC"
    return "SCALAR_SCALAR"


def expected_mode(kind, W):
    if kind in ("chw", "rowcrop"):
        return "VEC" if W % 4 == 0 else "SCALAR"
    if kind == "hwc":
        return "VEC3" if W % 4 == 0 else "SCALAR"
    return "SCALAR"


LAYOUT_SIZES = [(40, 52), (37, 45)]
LAYOUT_CASES = [(pk, gk, H, W, instantiation(expected_mode(pk, W), expected_mode(gk, W)))
                for (H, W) in LAYOUT_SIZES for pk in LAYOUTS for gk in LAYOUTS]
_BASE = {}


def test_layout_cases_reach_all_three_instantiations():
    assert {c[4] for c in LAYOUT_CASES} == {"VEC_VEC", "VEC3_VEC", "SCALAR_SCALAR"}


@pytest.mark.parametrize("pk,gk,H,W,path", LAYOUT_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}x{c[3]}-{c[4]}" for c in LAYOUT_CASES])
def test_loss_layouts_are_bit_identical(pk, gk, H, W, path):
    """Every layout loads the same floats and runs the same arithmetic, so the terms and the gradient are bit-identical to
    the contiguous (3,H,W) pair's, across the VEC / VEC3 / SCALAR loads and W % 4 = 0 or not.  The prediction holds values
    outside [0, 1] and is clamped on the fly."""
    gen = torch.Generator(device=DEV).manual_seed(H * W)
    gt = torch.rand(3, H, W, device=DEV, generator=gen)
    pred = gt * 1.3 - 0.15 + 0.1 * torch.randn(3, H, W, device=DEV, generator=gen)
    if (H, W) not in _BASE:
        _BASE[(H, W)] = run_loss(pred, gt, 0.2, True, 1.3)
        check_loss(pred, gt, *_BASE[(H, W)], 0.2, True, 1.3, f"loss/layout/{H}x{W}")
    x, y = make_layout(pred, pk), make_layout(gt, gk)
    assert torch.equal(x, pred) and torch.equal(y, gt)
    assert instantiation(loss_mode(x), loss_mode(y)) == path
    terms, grad = run_loss(x, y, 0.2, True, 1.3)
    bt, bg = _BASE[(H, W)]
    assert torch.equal(terms, bt), (terms - bt).tolist()
    assert torch.equal(grad, bg), (grad - bg).abs().max().item()


def test_loss_batch_with_mixed_layouts_and_double_backward():
    """B = 3 through LossFunction: the prediction a permuted (B,H,W,3) buffer (VEC3 per image), the ground truth a
    row-cropped (B,3,H,W+4) one (VEC) -- and once more with the ground truth one float off alignment (SCALAR).  L is the mean
    of the per-image losses, each image's gradient the single-image gradient under upstream 1/3, bit for bit.  A second
    backward through the same graph doubles the gradient exactly."""
    from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction
    B, H, W = 3, 44, 56
    lf = LossFunction(LossFunction.LossFunctionConfig(lambda_value=0.2, enable_regularization=False))
    gen = torch.Generator(device=DEV).manual_seed(99)
    gt = torch.rand(B, 3, H, W, device=DEV, generator=gen)
    pred = (gt + 0.2 * torch.randn(B, 3, H, W, device=DEV, generator=gen)).clamp(0, 1)
    third = torch.ones((), dtype=F32, device=DEV) / 3
    singles, grads = [], []
    for i in range(B):
        p = pred[i].clone().requires_grad_(True)
        Li = lf(p, gt[i].clone())[0]
        Li.backward(third)
        singles.append(Li.detach()); grads.append(p.grad)
    for gt_kind in ("rowcrop", "off1"):
        buf = pred.permute(0, 2, 3, 1).contiguous().requires_grad_(True)
        if gt_kind == "rowcrop":
            gbuf = torch.zeros(B, 3, H, W + 4, device=DEV)
            gbuf[..., :W] = gt
            gv = gbuf[..., :W]
        else:
            flat = torch.zeros(B * 3 * H * W + 1, device=DEV)
            gv = flat[1:].view(B, 3, H, W)
            gv.copy_(gt)
        assert torch.equal(gv, gt)
        L = lf(buf.permute(0, 3, 1, 2), gv)[0]
        L.backward(retain_graph=True)
        assert torch.equal(L.detach(), torch.stack(singles).mean())
        first = buf.grad.clone()
        assert torch.equal(first.permute(0, 3, 1, 2), torch.stack(grads))
        L.backward()
        assert torch.equal(buf.grad, 2 * first)


def test_loss_rejects_small_images_and_foreign_devices_before_any_launch():
    """H or W below the window raises a Python exception from check_loss_images, before anything reaches the library.  A
    ground truth on another device (the host) is refused by the same helper, which reads no data: this test calls the helper
    directly and never hands a host pointer to a kernel."""
    from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction, check_loss_images
    lf = LossFunction(LossFunction.LossFunctionConfig(enable_regularization=False))
    for H, W in [(10, 40), (40, 10), (10, 10)]:
        p, g = torch.rand(3, H, W, device=DEV), torch.rand(3, H, W, device=DEV)
        with pytest.raises(ValueError, match="11x11"):
            check_loss_images(p, g)
        with pytest.raises(ValueError, match="11x11"):
            lf(p.requires_grad_(True), g)
    p = torch.rand(3, 20, 24, device=DEV)
    check_loss_images(p, torch.rand(3, 20, 24, device=DEV))                           # accepted
    with pytest.raises(ValueError, match="cpu"):
        check_loss_images(p, torch.rand(3, 20, 24))
    with pytest.raises(TypeError):
        check_loss_images(p.cpu(), torch.rand(3, 20, 24))
    with pytest.raises(TypeError):
        check_loss_images(p, torch.rand(3, 20, 24, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError):
        check_loss_images(p, torch.rand(3, 20, 25, device=DEV))


# ----------------------------------------------------------------------------------------------------------------------
# scale regulariser

def run_reg(feat, mask, up):
    from taichi_3d_gaussian_splatting_amd.LossFunction import _ScaleRegulariser
    f = feat.detach().clone().requires_grad_(True)
    v = _ScaleRegulariser.apply(f, mask)
    (v * up).backward()
    torch.cuda.synchronize()
    return v.detach().clone(), f.grad


def _reg_inputs(N, kind, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    feat = torch.randn(N, 56, device=DEV, generator=gen)
    feat[:, 4:7] = torch.rand(N, 3, device=DEV, generator=gen) * 10 - 8             # log-scales in [-8, 2]
    if kind == "valid":
        inv = torch.zeros(N, dtype=torch.bool, device=DEV)
    elif kind == "invalid":
        inv = torch.ones(N, dtype=torch.bool, device=DEV)
    else:
        inv = torch.rand(N, device=DEV, generator=gen) < 0.3
    return feat, inv


@pytest.mark.parametrize("kind", ["valid", "invalid", "random30"])
@pytest.mark.parametrize("N", [0, 1, 255, 256, 257, 65537, 500000])
def test_regulariser_against_float64(N, kind):
    """Value and every gradient element within REG_RTOL of float64, with upstream -1.3; bool and int8 masks give the same
    bits.  No valid row -- N = 0 included -- gives NaN, as torch's mean of an empty selection does; its gradient is zero."""
    feat, inv = _reg_inputs(N, kind, N + len(kind))
    up = -1.3
    v, g = run_reg(feat, inv, up)
    v8, g8 = run_reg(feat, inv.to(torch.int8), up)
    assert torch.equal(v, v8) or (torch.isnan(v) and torch.isnan(v8))
    assert torch.equal(g, g8)
    v64, g64 = loss_ref.regulariser_ref(feat.cpu(), inv.cpu(), up)
    gk = g.double().cpu()
    if not bool((inv == 0).any()):
        assert torch.isnan(v) and torch.isnan(v64)
        assert not gk.any() and not g64.any()
        return
    rel = abs(v.item() - v64.item()) / abs(v64.item())
    _record(f"reg/value/N{N}/{kind}", rel / REG_RTOL)
    assert rel <= REG_RTOL, rel
    err = (gk - g64).abs()
    nz = g64 != 0
    assert not err[~nz].any(), "a gradient element the reference has as exact zero is not zero"
    used = (err[nz] / g64[nz].abs()).max().item()
    _record(f"reg/grad/N{N}/{kind}", used / REG_RTOL)
    assert used <= REG_RTOL, used


def test_regulariser_overflow_rows_against_torch_f32():
    """Log-scales of 40, 50 and 90 where exp^2 (from 44.4) or exp (from 88.7) overflows f32.  Both torch f32 and the kernel
    give an infinite value.  Gradients:
      40 (exp^2 finite): finite, both agree within REG_RTOL;
      50 (exp finite, exp^2 = inf, norm = inf): 0 in torch (x * (g / inf)) and in the kernel ((g / inf) * e * e) -- they agree;
      90 (exp = inf in torch): torch gives NaN in that component (inf * 0); the kernel 0, because gs_expf clamps its
          argument at 88 and exp stays finite -- a documented deviation; the value is already infinite.
    Every row without overflow keeps its finite gradient, equal to torch's within REG_RTOL."""
    N = 300
    feat, inv = _reg_inputs(N, "valid", 5)
    rows = {0: [40.0] * 3, 1: [50.0] * 3, 2: [90.0] * 3, 3: [50.0, 0.0, 0.0], 4: [90.0, 0.0, 0.0], 5: [0.0, 40.0, 0.0]}
    for r, s in rows.items():
        feat[r, 4:7] = torch.tensor(s, device=DEV)
    up = 2.0
    v, g = run_reg(feat, inv, up)
    ft = feat.clone().requires_grad_(True)
    vt = torch.norm(torch.exp(ft[inv == 0, 4:7]), dim=1).mean()
    (vt * up).backward()
    gt_ = ft.grad
    assert torch.isinf(v) and v > 0 and torch.isinf(vt) and vt > 0
    nan = float("nan")
    expect_kernel = {1: [0, 0, 0], 2: [0, 0, 0], 3: [0, 0, 0], 4: [0, 0, 0]}
    expect_torch = {1: [0, 0, 0], 2: [nan] * 3, 3: [0, 0, 0], 4: [nan, 0, 0]}
    for r in expect_kernel:
        ek, et = torch.tensor(expect_kernel[r]), torch.tensor(expect_torch[r])
        assert torch.equal(torch.isnan(g[r, 4:7].cpu()), torch.isnan(ek)), (r, g[r, 4:7].tolist())
        assert torch.equal(torch.isnan(gt_[r, 4:7].cpu()), torch.isnan(et)), (r, gt_[r, 4:7].tolist())
        fin = ~torch.isnan(ek)
        assert not g[r, 4:7].cpu()[fin].any()
    fin_rows = torch.ones(N, dtype=torch.bool)
    fin_rows[[1, 2, 3, 4]] = False
    a, b = g[fin_rows].cpu().double(), gt_[fin_rows].cpu().double()
    assert torch.isfinite(a).all() and bool((a[:2, 4:7] != 0).all())
    assert bool(((a - b).abs() <= REG_RTOL * b.abs() + 1e-30).all()), (a - b).abs().max().item()


def test_regulariser_mask_validation():
    """check_regulariser_inputs: a mask on another device, of another length, of more dimensions or of a float type raises;
    a non-contiguous mask is made contiguous (and gives the same bits as its contiguous copy); an integer mask counts every
    non-zero value as invalid (256 included, which a cast to int8 would wrap to 0).  No test hands a host pointer to a kernel."""
    from taichi_3d_gaussian_splatting_amd.LossFunction import check_regulariser_inputs
    feat, inv = _reg_inputs(1000, "random30", 3)
    with pytest.raises(ValueError, match="cpu"):
        check_regulariser_inputs(feat, inv.cpu())
    with pytest.raises(ValueError):
        check_regulariser_inputs(feat, inv[:999])
    with pytest.raises(ValueError):
        check_regulariser_inputs(feat, inv.reshape(1000, 1))
    with pytest.raises(TypeError):
        check_regulariser_inputs(feat, inv.float())
    with pytest.raises(TypeError):
        check_regulariser_inputs(feat[:, :55], inv)
    wide = torch.zeros(2000, dtype=torch.int8, device=DEV)
    wide[::2] = inv.to(torch.int8)
    strided = wide[::2]
    assert not strided.is_contiguous()
    m = check_regulariser_inputs(feat, strided)
    assert m.is_contiguous() and m.dtype == torch.int8 and torch.equal(m, inv.to(torch.int8))
    big = inv.to(torch.int32) * 256
    assert torch.equal(check_regulariser_inputs(feat, big), inv.to(torch.int8))
    i8 = inv.to(torch.int8)
    assert check_regulariser_inputs(feat, i8) is i8                                   # nothing copied
    v1, g1 = run_reg(feat, strided, 0.7)
    v2, g2 = run_reg(feat, inv, 0.7)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)


# ----------------------------------------------------------------------------------------------------------------------
# Adam

def _ulp(x):
    a = x.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def check_adam(p, ref, key):
    err = (p.double() - ref.p).abs() - 4 * _ulp(ref.p)
    pos = ref.S > 0
    assert bool((err[~pos] <= 0).all()), "a parameter without any update moved"
    used = (err[pos] / ref.S[pos]).max().item() if bool(pos.any()) else 0.0
    _record(key, used / ADAM_C)
    assert used <= ADAM_C, (key, used)


@pytest.mark.parametrize("betas,eps", [((0.9, 0.999), 1e-8), ((0.5, 0.9), 1e-15)], ids=["b0.9_0.999_eps1e-8", "b0.5_0.9_eps1e-15"])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1_000_003, 28_000_000])
def test_adam_against_float64(n, betas, eps):
    """200 steps with the trainer's per-step exponential lr decay (GaussianPointTrainer.py:136-137, gamma 0.97), against
    Adam64 fed the same f32 gradients; 28e6 is config 3's 5e5 x 56 features."""
    from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
    gen = torch.Generator(device=DEV).manual_seed(n + 1)
    p = torch.randn(n, device=DEV, generator=gen)
    ref = loss_ref.Adam64(p, betas, eps)
    lr = 1e-3
    opt = FusedAdam([p], lr=lr, betas=betas, eps=eps)
    scale = torch.exp(torch.randn(n, device=DEV, generator=gen) * 2)                    # per-element gradient scales
    for t in range(200):
        g = torch.randn(n, device=DEV, generator=gen) * scale
        p.grad = g
        opt.step()
        ref.step(g, opt.lr)
        lr *= 0.97
        opt.lr = lr
    assert opt.state[0]["step"] == 200
    check_adam(p, ref, f"adam/n{n}/b{betas[0]}_{betas[1]}/eps{eps:g}")


def test_adam_zero_gradients_first_and_for_many_steps():
    """A zero gradient on the first step leaves the parameter exactly and creates no NaN (0 / (0 + eps)); rows whose gradient
    stays zero for 150 steps -- density control's free rows -- do not move, then follow float64 once gradients arrive."""
    from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
    gen = torch.Generator(device=DEV).manual_seed(21)
    p = torch.randn(1000, 56, device=DEV, generator=gen)
    p0 = p.clone()
    opt = FusedAdam([p], lr=1e-3)
    ref = loss_ref.Adam64(p, (0.9, 0.999), 1e-8)
    for t in range(200):
        g = torch.randn(1000, 56, device=DEV, generator=gen)
        if t == 0:
            g.zero_()
        elif t < 150:
            g[:500] = 0.0
        p.grad = g
        opt.step()
        ref.step(g, opt.lr)
        if t == 0:
            assert torch.equal(p, p0) and not opt.state[0]["exp_avg"].any() and not opt.state[0]["exp_avg_sq"].any()
        if t == 149:
            assert torch.equal(p[:500], p0[:500])
        assert not torch.isnan(p).any()
    check_adam(p, ref, "adam/zero_rows")


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)], ids=["b0.9_0.999", "b0.5_0.9"])
def test_adam_extreme_gradients_match_torch_f32(betas):
    """Gradients of +-1e20 and +-1e-30, where g^2 overflows or underflows f32, against f32 torch.optim.Adam(foreach=False),
    the single-tensor update the kernel restates: the same elements are infinite, zero and finite in the parameter and both
    moments (g * g is formed first, as torch's GPU addcmul does), and the finite ones agree within 1e-4.  Not closer: the
    kernel takes 1 - beta2 from the f32 beta2 (1 - 0.999f = 0.00099998713), torch from the Python float (0.001), which
    puts exp_avg_sq 1.3e-5 apart."""
    from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
    gen = torch.Generator(device=DEV).manual_seed(31)
    n = 6 * 512
    p0 = torch.randn(n, device=DEV, generator=gen)
    base = torch.randn(n, device=DEV, generator=gen)
    kinds = torch.tensor([1e20, -1e20, 1e-30, -1e-30, 0.0, 1.0], device=DEV).repeat_interleave(512)
    pa, pb = p0.clone().requires_grad_(True), p0.clone()
    ref = torch.optim.Adam([pa], lr=1e-3, betas=betas, eps=1e-8, foreach=False)
    opt = FusedAdam([pb], lr=1e-3, betas=betas, eps=1e-8)
    for t in range(10):
        g = kinds * (1.0 + 0.5 * base.abs() * (t % 3))                                 # one sign per element: no
        g = torch.where(kinds == 1.0, (base.abs() + 0.1) * (t + 1), g)                # cancellation in m
        pa.grad, pb.grad = g.clone(), g.clone()
        ref.step()
        opt.step()
    st = ref.state[pa]
    for name, a, b in [("param", pa.detach(), pb), ("exp_avg", st["exp_avg"], opt.state[0]["exp_avg"]),
                       ("exp_avg_sq", st["exp_avg_sq"], opt.state[0]["exp_avg_sq"])]:
        for cls in (torch.isinf, torch.isnan, lambda x: x == 0):
            assert torch.equal(cls(a), cls(b)), name
        fin = torch.isfinite(a) & (a != 0)
        assert bool(((a[fin] - b[fin]).abs() <= 1e-4 * a[fin].abs() + 1e-9).all()), (name, (a[fin] - b[fin]).abs().max().item())


def test_adam_noncontiguous_grad_none_and_several_params():
    """A non-contiguous gradient updates like its contiguous copy; a parameter whose grad is None is skipped and its step
    count does not advance; several parameters in one optimiser equal one optimiser each -- all bit for bit."""
    from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
    gen = torch.Generator(device=DEV).manual_seed(41)
    a0, b0, c0 = (torch.randn(*s, device=DEV, generator=gen) for s in [(100, 56), (257,), (33, 3)])
    a, b, c = a0.clone(), b0.clone(), c0.clone()
    opt = FusedAdam([a, b, c], lr=1e-2, betas=(0.8, 0.99), eps=1e-7)
    sa, sb, sc = a0.clone(), b0.clone(), c0.clone()
    oa, ob, oc = (FusedAdam([x], lr=1e-2, betas=(0.8, 0.99), eps=1e-7) for x in (sa, sb, sc))
    for t in range(8):
        wide = torch.randn(100, 112, device=DEV, generator=gen)
        ga = wide[:, ::2]                                                               # non-contiguous
        gb = torch.randn(257, device=DEV, generator=gen)
        gc_ = torch.randn(33, 3, device=DEV, generator=gen)
        assert not ga.is_contiguous()
        a.grad, c.grad = ga, gc_
        b.grad = gb if t >= 3 else None                                                 # b: no gradient for three steps
        opt.step()
        sa.grad, sc.grad = ga.contiguous(), gc_
        oa.step(); oc.step()
        if t >= 3:
            sb.grad = gb
            ob.step()
        if t < 3:
            assert torch.equal(b, b0) and opt.state[1]["step"] == 0
    assert [s["step"] for s in opt.state] == [8, 5, 8]
    assert torch.equal(a, sa) and torch.equal(b, sb) and torch.equal(c, sc)
    assert torch.equal(opt.state[0]["exp_avg_sq"], oa.state[0]["exp_avg_sq"])


# ----------------------------------------------------------------------------------------------------------------------
# the backward's tagged `visited` buffer under growth

def test_backward_after_buffer_growth_equals_a_fresh_module():
    """Training-shaped: one rasteriser module for 30 iterations while invalid rows turn valid in steps (M and K grow past the
    buffers' 25 % slack several times) and the resolution switches twice.  Each iteration's point and feature gradients
    equal, bit for bit, those of a fresh module on the same inputs.  The fresh module is dropped before the next iteration.
    prepare_backward_blend clears the tagged `visited` flags when the buffer is reallocated; it used to tell that from a
    changed address, and a grown tail left uncleared would let stray bytes equal to the tag pass as set flags.  That old
    bug shows only when the allocator hands back the same address, which this test cannot force; the fix (the capacity
    decides) is verified by reading."""
    from taichi_3d_gaussian_splatting_amd import CameraInfo, GaussianPointCloudRasterisation as Rast
    from taichi_3d_gaussian_splatting_amd.synthetic import synth, view_pose
    N = 12000
    s = synth(N, 128, 96, 0.08, sh_deg=3, seed=23)
    q, t = view_pose()
    rng = np.random.default_rng(5)
    order = rng.permutation(N)
    cfg = Rast.GaussianPointCloudRasterisationConfig()
    module = Rast(cfg)

    def run(mod, W, H, invalid, it):
        K = s.camera_intrinsics.copy()
        K[0] *= W / 128.0
        K[1] *= H / 96.0
        pc = torch.tensor(s.point_cloud, device=DEV, requires_grad=True)
        feat = torch.tensor(s.point_cloud_features, device=DEV, requires_grad=True)
        img, _, _ = mod(Rast.GaussianPointCloudRasterisationInput(
            point_cloud=pc, point_cloud_features=feat, point_object_id=torch.tensor(s.point_object_id, device=DEV),
            point_invalid_mask=torch.tensor(invalid, device=DEV),
            camera_info=CameraInfo(torch.tensor(K, device=DEV), H, W, 0),
            q_pointcloud_camera=torch.tensor(q, device=DEV), t_pointcloud_camera=torch.tensor(t, device=DEV),
            color_max_sh_band=3))
        gen = torch.Generator(device=DEV).manual_seed(it)
        img.backward(torch.randn(img.shape, device=DEV, generator=gen))
        torch.cuda.synchronize()
        return pc.grad, feat.grad, mod.last_frame.n_points_in_camera, mod.last_frame.n_keys

    seen_M, seen_K = [], []
    for it in range(30):
        W, H = [(128, 96), (256, 192), (192, 144)][it // 10]          # (multiples of the 16x16 tile)
        invalid = np.ones(N, np.int8)
        invalid[order[: 300 + it * 390]] = 0                    # 300 valid rows, then 390 more every iteration
        gp, gf, M, K = run(module, W, H, invalid, it)
        fresh = Rast(cfg)
        fp, ff, M2, K2 = run(fresh, W, H, invalid, it)
        del fresh
        gc.collect()
        assert (M, K) == (M2, K2)
        assert torch.equal(gp, fp), f"iteration {it}: point gradients differ from a fresh module's"
        assert torch.equal(gf, ff), f"iteration {it}: feature gradients differ from a fresh module's"
        seen_M.append(M); seen_K.append(K)
    grow_M = sum(1 for i in range(1, 30) if seen_M[i] > 1.25 * max(seen_M[:i]))
    assert grow_M >= 3 and max(seen_K) > 4 * seen_K[0], (seen_M, seen_K)
