"""Float64 references of the per-iteration kernels after the rasteriser: the fused L1+SSIM loss (k_loss.hip), the
scale regulariser and Adam.  Plain torch on whatever device the inputs live on; tests/test_loss_ref_host.py pins them
on the CPU (direct windowed sums, finite differences, torch.optim.Adam), tests/test_gpu_loss_kernels.py holds the
kernels to them."""
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2
WIN = 11


def gauss_window(dtype=torch.float64, device="cpu"):
    """pytorch_msssim's 1-D window: 11 taps, sigma 1.5, normalised."""
    coords = torch.arange(WIN, dtype=dtype, device=device) - WIN // 2
    g = torch.exp(-(coords ** 2) / (2 * 1.5 ** 2))
    return g / g.sum()


def ssim_ref(X, Y):
    """pytorch_msssim.ssim(X, Y, data_range=1, size_average=True) restated; X, Y (1,3,H,W) float64."""
    coords = torch.arange(11, dtype=X.dtype, device=X.device) - 5
    g = torch.exp(-(coords ** 2) / (2 * 1.5 ** 2))
    g = (g / g.sum()).reshape(1, 1, 1, 11).repeat(3, 1, 1, 1)

    def gf(t):
        t = F.conv2d(t, g.transpose(2, 3), groups=3)       # along H first, then W
        return F.conv2d(t, g, groups=3)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    mu1, mu2 = gf(X), gf(Y)
    s1, s2, s12 = gf(X * X) - mu1 ** 2, gf(Y * Y) - mu2 ** 2, gf(X * Y) - mu1 * mu2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim_map = ((2 * mu1 * mu2 + C1) / (mu1 ** 2 + mu2 ** 2 + C1)) * cs
    return ssim_map.flatten(2).mean(-1).mean()


def l1_ssim_ref(pred, gt, lam=0.2, clamp=False, upstream=1.0):
    """L = (1 - lam) mean|x - y| + lam (1 - SSIM(x, y)), x = clamp(pred, 0, 1) if clamp else pred; (3,H,W) inputs of any
    dtype and strides.  Returns float64 (L, L1, LD, dL/dpred * upstream) with the gradient by autograd, on pred's device."""
    p = pred.detach().double().clone().requires_grad_(True)
    y = gt.detach().double()
    x = torch.clamp(p, 0, 1) if clamp else p
    l1 = (x - y).abs().mean()
    ld = 1 - ssim_ref(x[None], y[None])
    L = (1 - lam) * l1 + lam * ld
    (L * upstream).backward()
    return L.detach(), l1.detach(), ld.detach(), p.grad


def grad_magnitude(pred, gt, lam=0.2, clamp=False, upstream=1.0):
    """Per-pixel magnitude m of the gradient's derivative chain, float64: every term replaced by its absolute value.
    The loss counterpart of the oracle's `summed`.  With A, B, D = dS/dmu1, dS/dE[x^2], dS/dE[xy] of each map pixel
    (as k_loss_ssim_maps forms them) and F^T the transposed (full) window filter,
        m = |up| (k_l1 + k_ssim (F^T |A|' + 2 |x| F^T |B| + |y| F^T |D|)),
    |A|' = 2 |mu2| (|S/A1| + |S/A2|) + 2 |mu1| |S| (|1/B2| + |1/B1|), k_l1 = (1-lam)/(3HW), k_ssim = lam/(3(H-10)(W-10)).
    Zero where torch.clamp passes no gradient.  An f32 kernel's rounding error is bounded by a few eps times this sum
    (plus what the cancellations inside A, B, D add: measured, see the test)."""
    raw = pred.detach().double()
    x = torch.clamp(raw, 0, 1) if clamp else raw
    y = gt.detach().double()
    H, W = x.shape[1], x.shape[2]
    g = gauss_window(device=x.device)
    gv, gh = g.reshape(1, 1, WIN, 1).repeat(3, 1, 1, 1), g.reshape(1, 1, 1, WIN).repeat(3, 1, 1, 1)

    def gf(t):
        return F.conv2d(F.conv2d(t[None], gv, groups=3), gh, groups=3)[0]

    def gft(t):          # transposed filter: map (H-10, W-10) -> image (H, W)
        return F.conv_transpose2d(F.conv_transpose2d(t[None], gh, groups=3), gv, groups=3)[0]
    m1, m2 = gf(x), gf(y)
    s1, s2, s12 = gf(x * x) - m1 * m1, gf(y * y) - m2 * m2, gf(x * y) - m1 * m2
    A1, A2 = 2 * m1 * m2 + C1, 2 * s12 + C2
    B1, B2 = m1 * m1 + m2 * m2 + C1, s1 + s2 + C2
    S = (A1 / B1) * (A2 / B2)
    S_A1, S_A2 = A2 / (B1 * B2), A1 / (B1 * B2)
    Aabs = 2 * m2.abs() * (S_A1.abs() + S_A2.abs()) + 2 * m1.abs() * S.abs() * (1 / B2.abs() + 1 / B1.abs())
    Babs = (S / B2).abs()
    Dabs = 2 * S_A2.abs()
    k_l1 = (1 - lam) / (3 * H * W)
    k_ssim = lam / (3 * (H - WIN + 1) * (W - WIN + 1))
    m = abs(upstream) * (k_l1 + k_ssim * (gft(Aabs) + 2 * x.abs() * gft(Babs) + y.abs() * gft(Dabs)))
    if clamp:
        m = torch.where((raw >= 0) & (raw <= 1), m, torch.zeros_like(m))
    return m


def regulariser_ref(features, invalid_mask, upstream=1.0):
    """mean over valid rows of ||exp(features[:, 4:7])||_2 (LossFunction.py:40-51) in float64, and its gradient times
    upstream.  An empty selection gives NaN, like torch's mean of an empty tensor."""
    f = features.detach().double().clone().requires_grad_(True)
    valid = invalid_mask == 0
    value = torch.norm(torch.exp(f[valid, 4:7]), dim=1).mean()
    (value * upstream).backward()
    return value.detach(), f.grad


class Adam64:
    """torch.optim.Adam's single-tensor update (no weight decay, no amsgrad, not maximize) restated in float64, op for op:
        m.lerp_(g, 1 - b1); v.mul_(b2).addcmul_(g, g, value=1 - b2)
        p.addcdiv_(m, (v.sqrt() / sqrt(1 - b2^t)).add_(eps), value=-lr / (1 - b1^t))
    Also keeps S = sum over steps of lr_t |m_hat / (sqrt(v_hat) + eps)|, the summed size of the updates."""

    def __init__(self, p, betas=(0.9, 0.999), eps=1e-8):
        self.p = p.detach().double().clone()
        self.m = torch.zeros_like(self.p)
        self.v = torch.zeros_like(self.p)
        self.S = torch.zeros_like(self.p)
        self.betas, self.eps, self.t = betas, eps, 0

    def step(self, grad, lr):
        b1, b2 = self.betas
        g = grad.detach().double()
        self.t += 1
        self.m.lerp_(g, 1 - b1)
        self.v.mul_(b2).addcmul_(g, g, value=1 - b2)
        bias_correction1 = 1 - b1 ** self.t
        bias_correction2_sqrt = (1 - b2 ** self.t) ** 0.5
        step_size = lr / bias_correction1
        denom = (self.v.sqrt() / bias_correction2_sqrt).add_(self.eps)
        self.p.addcdiv_(self.m, denom, value=-step_size)
        self.S.add_((self.m / denom).abs_(), alpha=step_size)
        return self.p
