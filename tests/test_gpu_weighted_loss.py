"""GPU (-m gpu): the weighted L1+SSIM loss (include/gs_loss_weighted.h; the WT instantiations of k_loss.hip) held to the
float64 reference of tests/weighted_loss_ref.py, at the tile edges, weight patterns and values where such kernels go wrong.

The bars are those of tests/test_gpu_loss_kernels.py: L1 within 1e-6; L and LD within TERM_TOL = 2e-6 -- or, where few
windows carry weight and the mean no longer averages the per-window f32 error of E[x^2] - mu^2, four times the error of the
same definition evaluated by torch in f32 against float64, whichever is larger; every gradient element within
1e-4 |g64| + C_LOSS m with m = weighted_loss_ref.grad_magnitude, plus the tensor-level 1e-4; what the reference has as exact
zero is exact zero.  A case over a bar is a finding about the kernel, not a reason to widen the bar.

With GS_LOSS_WEIGHTED_MARGINS_OUT=<path> set, the share of every bar that the run used is written there as JSON
(profiles/loss_weighted_margins.json holds a recorded run)."""
import json
import os

import numpy as np
import pytest
import torch

import weighted_loss_ref as wref
from test_gpu_loss_kernels import C_LOSS, LAYOUT_CASES, TERM_TOL, instantiation, loss_mode, make_layout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
L1_TOL = 1e-6

MARGINS = {}


def _record(key, used):
    MARGINS[key] = max(float(used), MARGINS.get(key, 0.0))


@pytest.fixture(scope="module", autouse=True)
def _write_margins():
    yield
    out = os.environ.get("GS_LOSS_WEIGHTED_MARGINS_OUT")
    if out:
        with open(out, "w") as fh:
            json.dump({"C_LOSS": C_LOSS, "TERM_TOL": TERM_TOL, "L1_TOL": L1_TOL, "used": dict(sorted(MARGINS.items()))}, fh, indent=1)


def _fn():
    from taichi_3d_gaussian_splatting_amd.LossFunction import _L1SSIMWeighted
    return _L1SSIMWeighted


def run_weighted(pred, gt, weight, lam=0.2, clamp=False, up=1.0):
    """(terms (5,), dL/dpred * up) of the weighted kernels for a (3,H,W) pred view of any strides"""
    p = pred.detach().requires_grad_(True)
    L, terms = _fn().apply(p, gt, weight, lam, clamp)
    L.backward(torch.tensor(up, dtype=F32, device=DEV))
    torch.cuda.synchronize()
    return terms.detach().clone(), p.grad.clone()


def check_weighted(pred, gt, weight, terms, grad, lam, clamp, up, key, sparse=False):
    pc, gc_, wc = pred.detach().cpu(), gt.detach().cpu(), weight.detach().cpu()
    t64, g64 = wref.weighted_l1_ssim_ref(pc, gc_, wc, lam, clamp, up)
    term_tol = TERM_TOL
    if sparse:
        t32, _ = wref.weighted_l1_ssim_ref(pc, gc_, wc, lam, clamp, up, dtype=torch.float32)
        term_tol = max(TERM_TOL, 4 * (t32.double() - t64)[[0, 2]].abs().max().item())
    t = terms.double().cpu()
    err = (t - t64).abs()
    print(f"{key}: terms {t.tolist()} ref {t64.tolist()} term_tol {term_tol:.3g}")
    _record(key + "/L1", err[1].item() / L1_TOL)
    _record(key + "/L,LD", max(err[0].item(), err[2].item()) / term_tol)
    assert err[1].item() < L1_TOL and err[2].item() < term_tol and err[0].item() < term_tol, (t.tolist(), t64.tolist(), term_tol)
    # S_w and V are sums of f32 weights taken in float64 and rounded once
    assert err[3].item() <= 1e-6 * max(t64[3].item(), 1.0) and err[4].item() <= 1e-6 * max(t64[4].item(), 1.0)
    m = wref.grad_magnitude(pc, gc_, wc, lam, clamp, up)
    g = grad.double().cpu()
    excess = (g - g64).abs() - 1e-4 * g64.abs()
    zero_m = m == 0
    assert torch.equal(g[zero_m], g64[zero_m]), "a gradient the reference has as exact zero is not zero"
    used = (excess[~zero_m] / m[~zero_m]).max().item() if (~zero_m).any() else 0.0
    _record(key + "/grad", used / C_LOSS)
    print(f"{key}: gradient bar used {used / C_LOSS:.3f}")
    assert used <= C_LOSS, (key, used)
    ref_max = g64.abs().max().item()
    if ref_max > 0:
        assert (g - g64).abs().max().item() <= 1e-4 * ref_max


def _content(H, W, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    gt = torch.rand(3, H, W, device=DEV, generator=gen)
    pred = (gt + 0.2 * torch.randn(3, H, W, device=DEV, generator=gen)).clamp(0, 1)
    return pred, gt


PATTERNS = ["ones", "binary_half", "uniform", "rectangle_hole", "one_pixel", "border_only", "zeros"]
SPARSE = {"one_pixel"}


def make_weight(name, H, W, seed=0):
    gen = torch.Generator(device=DEV).manual_seed(1000 + seed)
    if name == "ones":
        return torch.ones(H, W, device=DEV)
    if name == "binary_half":
        return (torch.rand(H, W, device=DEV, generator=gen) < 0.5).float()
    if name == "uniform":
        return torch.rand(H, W, device=DEV, generator=gen)
    if name == "rectangle_hole":         # edges on the forward tiles' column 32 and row 22 and on the backward tiles' row 54
        w = torch.ones(H, W, device=DEV)
        w[22:54, 32:min(W, 64)] = 0.0
        return w
    if name == "one_pixel":
        w = torch.zeros(H, W, device=DEV)
        w[H // 2, W // 2] = 1.0
        return w
    if name == "border_only":
        w = torch.ones(H, W, device=DEV)
        w[5:H - 5, 5:W - 5] = 0.0
        return w
    if name == "zeros":
        return torch.zeros(H, W, device=DEV)
    raise KeyError(name)


SIZES = [(11, 11), (12, 12), (23, 33), (55, 65), (11, 300), (300, 11), (65, 129)]


@pytest.mark.parametrize("H,W", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_size_sweep_against_float64(H, W):
    """Forward tiles are 32x22, backward tiles 32x54, the window is 11: sizes at the window, past one tile in either
    direction, short-wide and tall-narrow.  Uniform weights with a fifth of them switched off.  11x11 and 12x12 have one and
    four windows: the sparse bar; every other size, 11x300 and 300x11 with their 290 windows included, the plain TERM_TOL."""
    pred, gt = _content(H, W, H * 7919 + W)
    gen = torch.Generator(device=DEV).manual_seed(H + W)
    weight = torch.rand(H, W, device=DEV, generator=gen)
    weight[torch.rand(H, W, device=DEV, generator=gen) < 0.2] = 0.0
    if H == 11 or W == 11:
        weight[H // 2, W // 2] = 0.75                      # (11x11 has one window: keep its centre on)
    terms, grad = run_weighted(pred, gt, weight)
    check_weighted(pred, gt, weight, terms, grad, 0.2, False, 1.0, f"weighted/size/{H}x{W}", sparse=max(H, W) <= 12)


@pytest.mark.parametrize("H,W", [(55, 65), (65, 129)], ids=["55x65", "65x129"])
@pytest.mark.parametrize("name", PATTERNS)
def test_weight_patterns_against_float64(name, H, W):
    pred, gt = _content(H, W, 17 + len(name))
    weight = make_weight(name, H, W)
    lam, up = 0.2, -1.3
    terms, grad = run_weighted(pred, gt, weight, lam, False, up)
    assert bool(torch.isfinite(terms).all()) and bool(torch.isfinite(grad).all())
    check_weighted(pred, gt, weight, terms, grad, lam, False, up, f"weighted/pattern/{name}/{H}x{W}", sparse=name in SPARSE)
    if name == "ones":
        assert terms[3].item() == H * W and terms[4].item() == (H - 10) * (W - 10)
    if name == "zeros":
        assert terms.tolist() == [0.0, 0.0, 0.0, 0.0, 0.0] and bool((grad == 0).all())
    if name == "border_only":
        # V == 0 while S_w > 0: LD exactly 0, and the gradient is the L1 term alone, in the kernel's own operation order
        assert terms[2].item() == 0.0 and terms[4].item() == 0.0 and terms[3].item() == weight.sum().item() > 0
        k_l1 = (np.float32(1.0) - np.float32(lam)) / (np.float32(3.0) * np.float32(terms[3].item()))
        want = torch.tensor(up, dtype=F32, device=DEV) * ((torch.tensor(k_l1, device=DEV) * weight) * torch.sign(pred - gt))
        assert torch.equal(grad, want)
        assert bool((grad[:, 5:H - 5, 5:W - 5] == 0).all())


@pytest.mark.parametrize("H,W", [(55, 65), (65, 129)], ids=["55x65", "65x129"])
def test_negative_and_nan_weights_act_as_zeros_bit_for_bit(H, W):
    pred, gt = _content(H, W, 31)
    weight = make_weight("uniform", H, W, 1)
    off = make_weight("binary_half", H, W, 2) > 0
    weight[off] = 0.0
    bad = weight.clone()
    idx = off.nonzero()
    bad[idx[0::3, 0], idx[0::3, 1]] = -1.0
    bad[idx[1::3, 0], idx[1::3, 1]] = float("nan")
    bad[idx[2::3, 0], idx[2::3, 1]] = float("-inf")
    t0, g0 = run_weighted(pred, gt, weight)
    t1, g1 = run_weighted(pred, gt, bad)
    assert bool(torch.isfinite(t1).all()) and torch.equal(t0, t1) and torch.equal(g0, g1)


@pytest.mark.parametrize("clamp", [False, True], ids=["raw", "clamped"])
def test_masked_pixels_are_inert(clamp):
    """NaN, inf and 1e30 in both images under zero weight, at least 6 pixels from any positive weight: every term finite and
    bit-identical to the run with those pixels set to 0.5, the gradient identical too and exactly 0 there."""
    H, W = 65, 129
    pred, gt = _content(H, W, 41)
    weight = torch.zeros(H, W, device=DEV)
    weight[:21, :41] = make_weight("uniform", 21, 41, 3) + 0.01
    far = torch.zeros(H, W, dtype=torch.bool, device=DEV)
    far[27:, :] = True
    far[:, 47:] = True
    assert not weight[far].any()
    gen = torch.Generator(device=DEV).manual_seed(5)
    pick = far & (torch.rand(H, W, device=DEV, generator=gen) < 0.3)
    pick[27, 0] = pick[0, 47] = pick[27, 47] = pick[H - 1, W - 1] = True             # the nearest ones, and the far corner
    kind = torch.randint(0, 4, (H, W), device=DEV, generator=gen)
    clean_p, clean_g = pred.clone(), gt.clone()
    clean_p[:, pick], clean_g[:, pick] = 0.5, 0.5
    dirty_p, dirty_g = pred.clone(), gt.clone()
    dirty_p[:, pick & (kind == 0)] = float("nan")
    dirty_g[:, pick & (kind == 0)] = 0.5
    dirty_p[:, pick & (kind == 1)] = 1e30
    dirty_g[:, pick & (kind == 1)] = float("nan")
    dirty_p[:, pick & (kind == 2)] = float("inf")
    dirty_g[:, pick & (kind == 2)] = -1e30
    dirty_p[:, pick & (kind == 3)] = float("nan")
    dirty_g[:, pick & (kind == 3)] = float("nan")
    t0, g0 = run_weighted(clean_p, clean_g, weight, 0.2, clamp, 1.1)
    t1, g1 = run_weighted(dirty_p, dirty_g, weight, 0.2, clamp, 1.1)
    assert bool(torch.isfinite(t1).all()) and torch.equal(t0, t1), (t0.tolist(), t1.tolist())
    assert bool((g1[:, pick] == 0).all()) and bool((g1[:, far] == 0).all())
    assert torch.equal(g0, g1)
    check_weighted(clean_p, clean_g, weight, t0, g0, 0.2, clamp, 1.1, f"weighted/inert/{'clamped' if clamp else 'raw'}")


def test_clamp_passes_no_gradient_outside_the_range():
    H, W = 55, 65
    gen = torch.Generator(device=DEV).manual_seed(51)
    gt = torch.rand(3, H, W, device=DEV, generator=gen)
    pred = gt * 1.6 - 0.3
    pred[0, :3, :5], pred[1, 4, :7], pred[2, -2:, -3:] = 0.0, 1.0, 0.0          # the closed ends, exactly
    weight = make_weight("uniform", H, W, 4) + 0.05                                # positive everywhere
    terms, grad = run_weighted(pred, gt, weight, 0.2, True, 1.0)
    check_weighted(pred, gt, weight, terms, grad, 0.2, True, 1.0, "weighted/clamp")
    outside = (pred < 0) | (pred > 1)
    ends = (pred == 0) | (pred == 1)
    assert outside.float().mean() > 0.1 and not grad[outside].any()
    assert ends.sum() >= 20 and (grad[ends] != 0).all(), "torch.clamp passes the gradient at min and max"
    # and equals the unclamped call on the clamped image
    t2, _ = run_weighted(pred.clamp(0, 1), gt, weight, 0.2, False, 1.0)
    assert torch.equal(terms, t2)


_BASE = {}


@pytest.mark.parametrize("pk,gk,H,W,path", LAYOUT_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}x{c[3]}-{c[4]}" for c in LAYOUT_CASES])
def test_layouts_are_bit_identical(pk, gk, H, W, path):
    """The three instantiations (planar vector loads, the rasteriser's interleaved (H,W,3), scalar strides) with W % 4 == 0
    (16-byte weight loads) or not: the same floats, the same arithmetic, the same bits."""
    gen = torch.Generator(device=DEV).manual_seed(H * W)
    gt = torch.rand(3, H, W, device=DEV, generator=gen)
    pred = gt * 1.3 - 0.15 + 0.1 * torch.randn(3, H, W, device=DEV, generator=gen)
    weight = torch.rand(H, W, device=DEV, generator=gen)
    weight[torch.rand(H, W, device=DEV, generator=gen) < 0.3] = 0.0
    if (H, W) not in _BASE:
        _BASE[(H, W)] = run_weighted(pred, gt, weight, 0.2, True, 1.3)
        check_weighted(pred, gt, weight, *_BASE[(H, W)], 0.2, True, 1.3, f"weighted/layout/{H}x{W}")
    x, y = make_layout(pred, pk), make_layout(gt, gk)
    assert torch.equal(x, pred) and torch.equal(y, gt)
    assert instantiation(loss_mode(x), loss_mode(y)) == path
    terms, grad = run_weighted(x, y, weight, 0.2, True, 1.3)
    bt, bg = _BASE[(H, W)]
    assert torch.equal(terms, bt), (terms - bt).tolist()
    assert torch.equal(grad, bg), (grad - bg).abs().max().item()


def test_weight_off_a_16_byte_boundary_gives_the_same_bits():
    H, W = 40, 52
    pred, gt = _content(H, W, 61)
    weight = make_weight("uniform", H, W, 5)
    flat = torch.full((H * W + 4,), 7.0, device=DEV)
    shifted = flat[1:1 + H * W].view(H, W)
    shifted.copy_(weight)
    assert weight.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    t0, g0 = run_weighted(pred, gt, weight)
    t1, g1 = run_weighted(pred, gt, shifted)
    assert torch.equal(t0, t1) and torch.equal(g0, g1)


@pytest.mark.parametrize("H,W", [(41, 60), (37, 45)], ids=["41x60", "37x45"])
def test_lambda_zero_gradient_is_exactly_the_weighted_l1_sign(H, W):
    """lambda = 0: k_ssim = 0 and the gradient is up * ((k_l1 * w) * sign(x - y)) bit for bit, k_l1 = 1 / (3 S_w) in f32"""
    pred, gt = _content(H, W, 11)
    pred[0, 0, :5] = gt[0, 0, :5]                                                  # sign(0) = 0
    weight = make_weight("uniform", H, W, 6)
    weight[make_weight("binary_half", H, W, 7) > 0] = 0.0
    terms, grad = run_weighted(pred, gt, weight, 0.0, False, -0.8)
    k_l1 = (np.float32(1.0) - np.float32(0.0)) / (np.float32(3.0) * np.float32(terms[3].item()))
    want = torch.tensor(-0.8, dtype=F32, device=DEV) * ((torch.tensor(k_l1, device=DEV) * weight) * torch.sign(pred - gt))
    assert torch.equal(grad, want)
    assert terms[0].item() == terms[1].item()
    check_weighted(pred, gt, weight, terms, grad, 0.0, False, -0.8, f"weighted/lambda0/{H}x{W}")


def test_zero_upstream_gives_exact_zeros_and_two_runs_the_same_bits():
    H, W = 65, 129
    pred, gt = _content(H, W, 12)
    weight = make_weight("uniform", H, W, 8)
    terms, grad = run_weighted(pred, gt, weight, 0.2, False, 0.0)
    assert bool((grad == 0).all())
    t1, g1 = run_weighted(pred, gt, weight, 0.2, False, 1.0)
    t2, g2 = run_weighted(pred, gt, weight, 0.2, False, 1.0)
    assert torch.equal(terms, t1) and torch.equal(t1, t2) and torch.equal(g1, g2) and bool(g1.any())


def _launches_nothing(monkeypatch, call, error):
    """the call raises `error` without one call into the library: validation comes before any launch"""
    from taichi_3d_gaussian_splatting_amd import _native
    made = []
    real = _native.call
    with monkeypatch.context() as m:
        m.setattr(_native, "call", lambda name, *a, **k: (made.append(name), real(name, *a, **k))[1])
        with pytest.raises(error):
            call()
    assert made == [], made


def test_bad_weights_are_refused_before_any_launch(monkeypatch):
    from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction
    lf = LossFunction(LossFunction.LossFunctionConfig(lambda_value=0.2, enable_regularization=False))
    H, W = 23, 33
    pred, gt = _content(H, W, 71)
    good = torch.ones(H, W, device=DEV)
    cases = [(torch.ones(H, W + 1, device=DEV), ValueError), (torch.ones(3, H, W, device=DEV), ValueError),
             (torch.ones(W, H, device=DEV), ValueError), (torch.ones(H, W, device=DEV, dtype=torch.float64), TypeError),
             (torch.ones(H, W, device=DEV, dtype=torch.uint8), TypeError), (torch.ones(H, W), ValueError),
             (torch.ones(H, 2 * W, device=DEV)[:, ::2], ValueError), ([[1.0] * W] * H, TypeError)]
    for weight, error in cases:
        _launches_nothing(monkeypatch, lambda: lf(pred, gt, pixel_weight=weight), error)
        _launches_nothing(monkeypatch, lambda: _fn().apply(pred, gt, weight, 0.2, False), error)
    _launches_nothing(monkeypatch, lambda: lf(pred, gt, pixel_weight=torch.ones(H, W + 1, device=DEV)), ValueError)
    batch_p, batch_g = torch.stack([pred, pred]), torch.stack([gt, gt])
    # the second image's weight is wrong: nothing runs for the first either
    _launches_nothing(monkeypatch, lambda: lf(batch_p, batch_g, pixel_weight=torch.ones(3, H, W, device=DEV)), ValueError)
    _launches_nothing(monkeypatch, lambda: lf(batch_p, batch_g, pixel_weight=torch.stack([good, good]).double()), TypeError)
    assert bool(torch.isfinite(lf(pred, gt, pixel_weight=good)[0]))


def test_module_without_a_weight_is_the_unweighted_path_bit_for_bit():
    from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction, _L1SSIM
    lf = LossFunction(LossFunction.LossFunctionConfig(lambda_value=0.2, enable_regularization=False))
    H, W = 55, 65
    pred, gt = _content(H, W, 81)
    p0 = pred.clone().requires_grad_(True)
    L0, terms0 = _L1SSIM.apply(p0, gt, 0.2, True)
    L0.backward()
    for kwargs in ({}, {"pixel_weight": None}):
        p = pred.clone().requires_grad_(True)
        L, l1, ld = lf(p, gt, clamp_predicted=True, **kwargs)
        L.backward()
        assert torch.equal(L, L0) and torch.equal(l1, terms0[1]) and torch.equal(ld, terms0[2]) and torch.equal(p.grad, p0.grad)
    # all-ones weights: the same definition through the weighted kernels, within the bars (not necessarily the same bits)
    Lw, l1w, ldw = lf(pred, gt, clamp_predicted=True, pixel_weight=torch.ones(H, W, device=DEV))
    assert abs(Lw - L0).item() < 2 * TERM_TOL and abs(l1w - terms0[1]).item() < 2 * L1_TOL and abs(ldw - terms0[2]).item() < 2 * TERM_TOL


def test_batch_with_a_shared_and_a_per_image_weight():
    from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction
    lf = LossFunction(LossFunction.LossFunctionConfig(lambda_value=0.2, enable_regularization=False))
    B, H, W = 2, 44, 56
    gen = torch.Generator(device=DEV).manual_seed(99)
    gt = torch.rand(B, 3, H, W, device=DEV, generator=gen)
    pred = (gt + 0.2 * torch.randn(B, 3, H, W, device=DEV, generator=gen)).clamp(0, 1)
    per_image = torch.stack([make_weight("uniform", H, W, 9), make_weight("binary_half", H, W, 10)])
    half = torch.ones((), dtype=F32, device=DEV) / 2
    for weight in (per_image[0], per_image):
        singles, grads, terms = [], [], []
        for i in range(B):
            p = pred[i].clone().requires_grad_(True)
            out = lf(p, gt[i].clone(), pixel_weight=weight if weight.dim() == 2 else weight[i])
            out[0].backward(half)
            singles.append(out[0].detach()); grads.append(p.grad); terms.append(torch.stack([out[1], out[2]]).detach())
        buf = pred.permute(0, 2, 3, 1).contiguous().requires_grad_(True)            # (B,H,W,3): the rasteriser's layout per image
        L, l1, ld = lf(buf.permute(0, 3, 1, 2), gt, pixel_weight=weight)
        L.backward()
        assert torch.equal(L, torch.stack(singles).mean())
        assert torch.equal(torch.stack([l1, ld]), torch.stack(terms).mean(dim=0))
        assert torch.equal(buf.grad.permute(0, 3, 1, 2), torch.stack(grads))
    with pytest.raises(ValueError):
        lf(pred, gt, pixel_weight=torch.ones(3, H, W, device=DEV))
    # a batch of one is squeezed, and its (1,H,W) weight with it
    one = lf(pred[:1], gt[:1], pixel_weight=per_image[:1])
    assert all(torch.equal(a, b) for a, b in zip(one, lf(pred[0], gt[0], pixel_weight=per_image[0])))
