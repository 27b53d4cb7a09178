"""CPU: the float64 references of tests/loss_ref.py that the GPU loss, regulariser and Adam tests compare against.
ssim_ref is held to a direct (non-separable) 11x11 windowed sum, the loss gradient to central finite differences, the
magnitude to the gradient it bounds, and Adam64 to torch.optim.Adam on float64 tensors."""
import numpy as np
import pytest
import torch

import loss_ref


def _images(H, W, seed):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0, 1, (3, H, W))
    pred = np.clip(gt + rng.normal(0, 0.2, (3, H, W)), 0, 1)
    return torch.tensor(pred), torch.tensor(gt)


def _ssim_direct(x, y):
    """SSIM by its definition: for every valid output pixel the 121 weights w[i] w[j] of the window, summed in a loop."""
    g = loss_ref.gauss_window().numpy()
    w2 = np.outer(g, g)
    _, H, W = x.shape
    total, n = 0.0, 0
    for c in range(3):
        for i in range(H - 10):
            for j in range(W - 10):
                a, b = x[c, i:i + 11, j:j + 11], y[c, i:i + 11, j:j + 11]
                mu1, mu2 = (w2 * a).sum(), (w2 * b).sum()
                s1 = (w2 * a * a).sum() - mu1 * mu1
                s2 = (w2 * b * b).sum() - mu2 * mu2
                s12 = (w2 * a * b).sum() - mu1 * mu2
                total += ((2 * mu1 * mu2 + loss_ref.C1) / (mu1 ** 2 + mu2 ** 2 + loss_ref.C1)) * \
                         ((2 * s12 + loss_ref.C2) / (s1 + s2 + loss_ref.C2))
                n += 1
    return total / n


@pytest.mark.parametrize("H,W", [(11, 11), (12, 17), (23, 30)])
def test_ssim_ref_equals_the_direct_windowed_sum(H, W):
    pred, gt = _images(H, W, H * 100 + W)
    got = loss_ref.ssim_ref(pred[None], gt[None]).item()
    ref = _ssim_direct(pred.numpy(), gt.numpy())
    assert abs(got - ref) < 1e-13, (got, ref)
    assert abs(loss_ref.ssim_ref(gt[None], gt[None]).item() - 1.0) < 1e-13


@pytest.mark.parametrize("H,W,lam,clamp,up", [(11, 11, 1.0, False, 1.0), (12, 17, 0.2, False, -1.7), (14, 13, 0.2, True, 0.5)])
def test_loss_gradient_equals_central_differences(H, W, lam, clamp, up):
    pred, gt = _images(H, W, 7 + H)
    if clamp:
        pred = pred + torch.tensor(np.random.default_rng(3).normal(0, 0.3, pred.shape))
        pred = torch.where((pred - 0.5).abs() > 0.49, pred + torch.sign(pred - 0.5) * 0.05, pred)   # keep off the clamp's kinks
    L, l1, ld, grad = loss_ref.l1_ssim_ref(pred, gt, lam, clamp, up)
    assert abs(L.item() - ((1 - lam) * l1.item() + lam * ld.item())) < 1e-15
    h = 1e-6
    fd = torch.zeros_like(pred)
    flat, fdf = pred.view(-1), fd.view(-1)
    for i in range(flat.numel()):
        keep = flat[i].item()
        flat[i] = keep + h
        Lp = loss_ref.l1_ssim_ref(pred, gt, lam, clamp)[0].item()
        flat[i] = keep - h
        Lm = loss_ref.l1_ssim_ref(pred, gt, lam, clamp)[0].item()
        flat[i] = keep
        fdf[i] = up * (Lp - Lm) / (2 * h)
    err = (grad - fd).abs().max().item()
    assert err < 1e-7 * grad.abs().max().item() + 1e-12, err


@pytest.mark.parametrize("lam,clamp,up", [(0.2, False, 1.0), (1.0, True, -2.0), (0.0, False, 0.5)])
def test_magnitude_bounds_the_gradient(lam, clamp, up):
    pred, gt = _images(21, 26, 11)
    if clamp:
        pred = pred * 1.4 - 0.2
    grad = loss_ref.l1_ssim_ref(pred, gt, lam, clamp, up)[3]
    m = loss_ref.grad_magnitude(pred, gt, lam, clamp, up)
    assert m.shape == grad.shape and bool((grad.abs() <= m * (1 + 1e-12)).all())
    if clamp:
        outside = (pred < 0) | (pred > 1)
        assert outside.any() and not m[outside].any()
    if lam == 0.0:
        assert torch.allclose(m, torch.full_like(m, abs(up) / (3 * 21 * 26)), rtol=1e-15, atol=0)


def test_regulariser_ref_matches_the_reference_lines():
    torch.manual_seed(0)
    f = torch.randn(40, 56, dtype=torch.float64)
    mask = torch.zeros(40, dtype=torch.int8)
    mask[::4] = 1
    v, g = loss_ref.regulariser_ref(f, mask, upstream=-0.5)
    e = torch.exp(f[mask == 0, 4:7])
    assert torch.allclose(v, e.norm(dim=1).mean(), rtol=1e-15)
    n = e.norm(dim=1, keepdim=True)
    assert torch.allclose(g[mask == 0, 4:7], -0.5 * e * e / (n * 30), rtol=1e-13)
    assert not g[mask == 1].any() and not g[:, :4].any() and not g[:, 7:].any()
    assert torch.isnan(loss_ref.regulariser_ref(f[:0], mask[:0])[0])
    assert torch.isnan(loss_ref.regulariser_ref(f, torch.ones(40, dtype=torch.int8))[0])


@pytest.mark.parametrize("betas,eps", [((0.9, 0.999), 1e-8), ((0.5, 0.9), 1e-15)])
def test_adam64_equals_torch_adam_in_float64(betas, eps):
    torch.manual_seed(1)
    p0 = torch.randn(300, dtype=torch.float64)
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=1e-2, betas=betas, eps=eps, foreach=False)
    ref = loss_ref.Adam64(p0, betas, eps)
    lr = 1e-2
    for it in range(50):
        g = torch.randn(300, dtype=torch.float64) * (1 + it % 5)
        g[:30] = 0.0                                           # rows without a gradient
        p.grad = g.clone()
        opt.step()
        ref.step(g, lr)
        if it == 20:
            lr *= 0.3
            opt.param_groups[0]["lr"] = lr
        assert torch.equal(ref.p, p.detach()), (it, (ref.p - p.detach()).abs().max().item())
    st = opt.state[p]
    assert torch.equal(ref.m, st["exp_avg"]) and torch.equal(ref.v, st["exp_avg_sq"])
    assert torch.equal(ref.p[:30], p0[:30]) and not ref.S[:30].any() and bool((ref.S[30:] > 0).all())
