"""Float64 references of the weighted L1+SSIM loss (include/gs_loss_weighted.h) and of the fourth plane of
gs_image_resample_rgba.  The definition, restated with loss_ref's window and autograd:

    w(p) = weight[p] if weight[p] > 0 else 0            (negative and NaN weights count as 0)
    S_w = sum_p w(p);  L1_w = sum_c sum_p w(p) |x_c(p) - y_c(p)| / (3 S_w)
    v(q) = w(q_y + 5, q_x + 5);  V = sum_q v(q);  SSIM_w = sum_c sum_q v(q) s_c(q) / (3 V)
    L = (1 - lam) L1_w + lam (1 - SSIM_w);  terms = {L, L1_w, 1 - SSIM_w, S_w, V}
    S_w == 0: the L1 term is 0.  V == 0: the SSIM term (1 - SSIM_w) is 0.

tests/test_weighted_loss_ref_host.py pins it on the CPU; tests/test_gpu_weighted_loss.py holds the kernels to it.  The
images are finite here: what a masked NaN does is a property of the kernels (selection), tested there without a reference."""
import numpy as np
import torch
import torch.nn.functional as F

import loss_ref
import resample_ref

WIN = loss_ref.WIN
HALF = WIN // 2


def effective_weight(weight, dtype=torch.float64):
    w = weight.detach().to(dtype)
    return torch.where(w > 0, w, torch.zeros_like(w))


def ssim_map(X, Y):
    """the per-window SSIM of loss_ref.ssim_ref before its mean: (3,H,W) -> (3,H-10,W-10), in the inputs' dtype"""
    g = loss_ref.gauss_window(dtype=X.dtype, device=X.device)
    gv, gh = g.reshape(1, 1, WIN, 1).repeat(3, 1, 1, 1), g.reshape(1, 1, 1, WIN).repeat(3, 1, 1, 1)

    def gf(t):
        return F.conv2d(F.conv2d(t[None], gv, groups=3), gh, groups=3)[0]       # along H first, then W
    mu1, mu2 = gf(X), gf(Y)
    s1, s2, s12 = gf(X * X) - mu1 ** 2, gf(Y * Y) - mu2 ** 2, gf(X * Y) - mu1 * mu2
    return ((2 * mu1 * mu2 + loss_ref.C1) / (mu1 ** 2 + mu2 ** 2 + loss_ref.C1)) * ((2 * s12 + loss_ref.C2) / (s1 + s2 + loss_ref.C2))


def window_weight(w):
    """v(q): the weight of every window's centre pixel, (H,W) -> (H-10,W-10)"""
    return w[HALF:w.shape[0] - HALF, HALF:w.shape[1] - HALF]


def weighted_l1_ssim_ref(pred, gt, weight, lam=0.2, clamp=False, upstream=1.0, dtype=torch.float64):
    """-> (terms (5,) = {L, L1_w, 1 - SSIM_w, S_w, V}, dL/dpred * upstream), both in `dtype` (float64: the reference;
    float32: the same definition as torch evaluates it in f32, the yardstick of the sparse cases' term tolerance)."""
    p = pred.detach().to(dtype).clone().requires_grad_(True)
    y = gt.detach().to(dtype)
    w = effective_weight(weight, dtype)
    v = window_weight(w)
    x = torch.clamp(p, 0, 1) if clamp else p
    Sw, V = w.sum(), v.sum()
    zero = (p * 0).sum()                         # keeps the graph when a term is switched off
    l1 = (w * (x - y).abs()).sum() / (3 * Sw) if Sw > 0 else zero
    ld = 1 - (v * ssim_map(x, y)).sum() / (3 * V) if V > 0 else zero
    L = (1 - lam) * l1 + lam * ld
    (L * upstream).backward()
    return torch.stack([L.detach(), l1.detach(), ld.detach(), Sw, V]), p.grad


def grad_magnitude(pred, gt, weight, lam=0.2, clamp=False, upstream=1.0):
    """loss_ref.grad_magnitude with the maps multiplied by v, k_l1 -> (1 - lam) w(p) / (3 S_w) and k_ssim -> lam / (3 V)
    (each 0 where its sum is 0): the per-pixel magnitude of the weighted gradient's derivative chain, float64."""
    raw = pred.detach().double()
    x = torch.clamp(raw, 0, 1) if clamp else raw
    y = gt.detach().double()
    w = effective_weight(weight)
    v = window_weight(w)
    g = loss_ref.gauss_window(device=x.device)
    gv, gh = g.reshape(1, 1, WIN, 1).repeat(3, 1, 1, 1), g.reshape(1, 1, 1, WIN).repeat(3, 1, 1, 1)

    def gf(t):
        return F.conv2d(F.conv2d(t[None], gv, groups=3), gh, groups=3)[0]

    def gft(t):          # transposed filter: map (H-10, W-10) -> image (H, W)
        return F.conv_transpose2d(F.conv_transpose2d(t[None], gh, groups=3), gv, groups=3)[0]
    m1, m2 = gf(x), gf(y)
    s1, s2, s12 = gf(x * x) - m1 * m1, gf(y * y) - m2 * m2, gf(x * y) - m1 * m2
    A1, A2 = 2 * m1 * m2 + loss_ref.C1, 2 * s12 + loss_ref.C2
    B1, B2 = m1 * m1 + m2 * m2 + loss_ref.C1, s1 + s2 + loss_ref.C2
    S = (A1 / B1) * (A2 / B2)
    S_A1, S_A2 = A2 / (B1 * B2), A1 / (B1 * B2)
    Aabs = v * (2 * m2.abs() * (S_A1.abs() + S_A2.abs()) + 2 * m1.abs() * S.abs() * (1 / B2.abs() + 1 / B1.abs()))
    Babs = v * (S / B2).abs()
    Dabs = v * 2 * S_A2.abs()
    Sw, V = w.sum().item(), v.sum().item()
    k_l1 = (1 - lam) * w / (3 * Sw) if Sw > 0 else torch.zeros_like(w)
    k_ssim = lam / (3 * V) if V > 0 else 0.0
    m = abs(upstream) * (k_l1 + k_ssim * (gft(Aabs) + 2 * x.abs() * gft(Babs) + y.abs() * gft(Dabs)))
    if clamp:
        m = torch.where((raw >= 0) & (raw <= 1), m, torch.zeros_like(m))
    return m


def shortcut_multiply_the_images(pred, gt, weight, lam=0.2):
    """the tempting wrong way: the unweighted loss of both images multiplied by the mask.  -> float64 (L, L1, LD)"""
    w = effective_weight(weight)
    L, l1, ld, _ = loss_ref.l1_ssim_ref(pred.double() * w, gt.double() * w, lam)
    return L, l1, ld


def weighted_mse_ref(pred, gt, weight):
    """sum w (x - y)^2 / (3 sum w), float64: the trainer's weighted PSNR is 10 log10(1 / this)"""
    w = effective_weight(weight)
    return (w * (pred.double() - gt.double()) ** 2).sum() / (3 * w.sum())


# ---- the fourth plane of gs_image_resample_rgba ------------------------------------------------------------------------

def channel3_to_float(image_hwc_u8):
    """(H,W,4) uint8 -> (1,H,W) float64 of channel 3 / 255"""
    return np.asarray(image_hwc_u8)[..., 3:4].astype(np.float64).transpose(2, 0, 1) / 255.0


def weight_plane(image_hwc_u8, size_full, size_out=None):
    """plane 3 of gs_image_resample_rgba for a uint8 (H,W,4) source, float64: channel 3 through resample_ref's filter"""
    return resample_ref.resize_antialias(channel3_to_float(image_hwc_u8), size_full, size_out)[0]
