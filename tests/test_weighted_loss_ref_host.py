"""CPU: the float64 reference of the weighted L1+SSIM loss (tests/weighted_loss_ref.py) pinned by direct windowed sums,
finite differences, its unweighted limit (loss_ref.l1_ssim_ref) and its empty-mask rules; and the channel-3 case of the
resample reference."""
import numpy as np
import torch

import loss_ref
import resample_ref
import weighted_loss_ref as wref


def _case(H, W, seed, pattern="uniform"):
    gen = torch.Generator().manual_seed(seed)
    gt = torch.rand(3, H, W, generator=gen, dtype=torch.float64)
    pred = (gt + 0.2 * torch.randn(3, H, W, generator=gen, dtype=torch.float64)).clamp(0, 1)
    w = torch.rand(H, W, generator=gen, dtype=torch.float64)
    if pattern == "binary":
        w = (w < 0.5).double()
    return pred, gt, w


def _direct(pred, gt, w, lam):
    """the definition by explicit loops over windows, numpy float64"""
    x, y, w = pred.numpy(), gt.numpy(), np.where(w.numpy() > 0, w.numpy(), 0.0)
    H, W = w.shape
    d = np.arange(11) - 5.0
    g = np.exp(-d * d / (2 * 1.5 ** 2))
    g /= g.sum()
    g2 = np.outer(g, g)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    Sw = w.sum()
    l1 = sum(w[i, j] * abs(x[c, i, j] - y[c, i, j]) for c in range(3) for i in range(H) for j in range(W)) / (3 * Sw)
    V = num = 0.0
    for qy in range(H - 10):
        for qx in range(W - 10):
            v = w[qy + 5, qx + 5]
            V += v
            for c in range(3):
                a, b = x[c, qy:qy + 11, qx:qx + 11], y[c, qy:qy + 11, qx:qx + 11]
                m1, m2 = (g2 * a).sum(), (g2 * b).sum()
                s1, s2, s12 = (g2 * a * a).sum() - m1 * m1, (g2 * b * b).sum() - m2 * m2, (g2 * a * b).sum() - m1 * m2
                num += v * ((2 * m1 * m2 + C1) / (m1 * m1 + m2 * m2 + C1)) * ((2 * s12 + C2) / (s1 + s2 + C2))
    ld = 1 - num / (3 * V)
    return (1 - lam) * l1 + lam * ld, l1, ld, Sw, V


def test_direct_windowed_sums_at_13x14():
    for pattern in ("uniform", "binary"):
        pred, gt, w = _case(13, 14, 5, pattern)
        terms, _ = wref.weighted_l1_ssim_ref(pred, gt, w, 0.2)
        want = _direct(pred, gt, w, 0.2)
        assert np.abs(terms.numpy() - np.array(want)).max() < 1e-12, (terms.tolist(), want)


def test_gradient_against_finite_differences():
    pred, gt, w = _case(14, 15, 6)
    pred = pred * 0.8 + 0.1                      # away from clamp's ends and from x == y
    _, grad = wref.weighted_l1_ssim_ref(pred, gt, w, 0.3, clamp=True, upstream=-1.5)
    h = 1e-6
    for c, i, j in [(0, 0, 0), (1, 7, 7), (2, 13, 14), (0, 5, 9), (1, 12, 2)]:
        hi, lo = pred.clone(), pred.clone()
        hi[c, i, j] += h
        lo[c, i, j] -= h
        fd = -1.5 * (wref.weighted_l1_ssim_ref(hi, gt, w, 0.3, True)[0][0] - wref.weighted_l1_ssim_ref(lo, gt, w, 0.3, True)[0][0]) / (2 * h)
        assert abs(fd - grad[c, i, j]).item() < 1e-7 * max(1.0, abs(fd.item())) + 1e-9, ((c, i, j), fd.item(), grad[c, i, j].item())


def test_unit_weight_is_the_unweighted_loss():
    pred, gt, _ = _case(23, 33, 7)
    ones = torch.ones(23, 33)
    for clamp in (False, True):
        x = pred * 1.4 - 0.2 if clamp else pred
        terms, grad = wref.weighted_l1_ssim_ref(x, gt, ones, 0.2, clamp, 0.7)
        L, l1, ld, g = loss_ref.l1_ssim_ref(x, gt, 0.2, clamp, 0.7)
        assert abs(terms[0] - L) < 1e-12 and abs(terms[1] - l1) < 1e-12 and abs(terms[2] - ld) < 1e-12
        assert terms[3] == 23 * 33 and terms[4] == 13 * 23
        assert (grad - g).abs().max() < 1e-12
        m, m0 = wref.grad_magnitude(x, gt, ones, 0.2, clamp, 0.7), loss_ref.grad_magnitude(x, gt, 0.2, clamp, 0.7)
        assert (m - m0).abs().max() < 1e-12 * m0.abs().max()


def test_magnitude_bounds_the_gradient():
    pred, gt, w = _case(25, 31, 8, "binary")
    _, grad = wref.weighted_l1_ssim_ref(pred, gt, w, 0.2)
    m = wref.grad_magnitude(pred, gt, w, 0.2)
    assert bool((grad.abs() <= m * (1 + 1e-9) + 1e-18).all())
    zero = m == 0
    assert bool(zero.any()) and not grad[zero].any()


def test_multiplying_the_images_by_the_mask_is_a_different_number():
    pred, gt, w = _case(23, 33, 9, "binary")
    terms, _ = wref.weighted_l1_ssim_ref(pred, gt, w, 0.2)
    L, l1, ld = wref.shortcut_multiply_the_images(pred, gt, w, 0.2)
    # masked pixels count as perfect matches in both of the shortcut's means: both terms come out too small
    assert l1 < 0.7 * terms[1] and ld < 0.9 * terms[2] and abs(L - terms[0]) > 1e-2


def test_negative_and_nan_weights_are_zeros():
    pred, gt, w = _case(15, 16, 10, "binary")
    bad = w.clone()
    n = int((w == 0).sum())
    bad[w == 0] = torch.tensor([-1.0, float("nan")], dtype=torch.float64).repeat(n // 2 + 1)[:n]
    a, ga = wref.weighted_l1_ssim_ref(pred, gt, w)
    b, gb = wref.weighted_l1_ssim_ref(pred, gt, bad)
    assert torch.equal(a, b) and torch.equal(ga, gb)


def test_empty_sums_switch_their_term_off():
    pred, gt, _ = _case(23, 33, 11)
    terms, grad = wref.weighted_l1_ssim_ref(pred, gt, torch.zeros(23, 33))
    assert terms.tolist() == [0, 0, 0, 0, 0] and not grad.any()
    border = torch.ones(23, 33, dtype=torch.float64)
    border[5:-5, 5:-5] = 0
    terms, grad = wref.weighted_l1_ssim_ref(pred, gt, border, 0.2)
    Sw = border.sum().double()
    assert terms[2] == 0 and terms[4] == 0 and terms[3] == Sw and terms[1] > 0
    want = 0.8 * border / (3 * Sw) * torch.sign(pred - gt)
    assert (grad - want).abs().max() < 1e-15
    assert not grad[:, 5:-5, 5:-5].any()
    mse = wref.weighted_mse_ref(pred, gt, border)
    assert abs(mse - ((pred - gt) ** 2 * border).sum() / (3 * Sw)) < 1e-15


def test_weight_plane_is_channel_3_through_the_same_filter():
    rng = np.random.default_rng(0)
    u8 = rng.integers(0, 256, (64, 96, 4)).astype(np.uint8)
    assert np.array_equal(wref.weight_plane(u8, (64, 96)), u8[..., 3] / 255.0)          # equal sizes: the identity
    swapped = u8[..., [3, 1, 2, 0]]
    assert np.array_equal(wref.weight_plane(u8, (32, 48)), resample_ref.target(swapped, 2)[0])
    assert np.array_equal(wref.weight_plane(u8, (40, 56), (32, 48)), wref.weight_plane(u8, (40, 56))[:32, :48])
    binary = np.zeros((64, 96, 4), np.uint8)
    binary[16:48, 24:72, 3] = 255
    plane = wref.weight_plane(binary, (32, 48))
    assert plane.min() >= 0 and plane.max() <= 1 + 1e-15 and ((plane > 1e-9) & (plane < 1 - 1e-9)).any()     # soft at its borders
