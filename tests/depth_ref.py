"""The float64 reference of depth supervision (include/gs_depth.h), restated in numpy and torch: the depth target with its
validity weight (resample), and selection, moments, fit, loss and gradient of the depth loss (evaluate).  No package import.

evaluate() takes a dtype: float64 is the reference; float32 is "the same formulas in torch f32", whose distance to the
reference sets the bars of the GPU tests."""
import numpy as np
import torch

import resample_ref

FORMAT_U16, FORMAT_F32 = 0, 1
INVERT_PREDICTED, INVERT_TARGET, L2, ALIGN = 1, 2, 4, 8
FLAGS_ALL = 15
PIXELS_PER_BLOCK = 1024
FINISH_THREADS = 256
MOMENTS = 5
LOSS_TERMS = 8
DEGENERATE = 1e-12              # the fit is s = 0, t = mean unless det > DEGENERATE * S_w * S_yy


# ---- the depth target ---------------------------------------------------------------------------------------------------------
def samples(src, fmt, depth_scale=1.0):
    """-> (valid bool (H,W), z float64 (H,W), 0 where invalid) of a source: uint16 (0 is a hole, z = f32(v) * f32(scale), one
    f32 multiply) or f32 (valid iff finite and > 0)"""
    src = np.asarray(src)
    if fmt == FORMAT_U16:
        valid = src != 0
        z = (src.astype(np.float32) * np.float32(depth_scale)).astype(np.float64)
    else:
        with np.errstate(invalid="ignore"):
            valid = np.isfinite(src) & (src > 0)
        z = np.where(valid, src, 0.0).astype(np.float64)
    return valid, np.where(valid, z, 0.0)


def resample(src, fmt, size_full, crop=None, depth_scale=1.0, min_coverage=0.5):
    """-> (depth, weight, den), float64 (h,w): with k the separable filter weight and v the validity, den = sum k v,
    num = sum k v z; weight = den where den > 0 and den >= min_coverage, else 0; depth = num / den where the weight is not 0,
    else 0.  An invalid sample reaches nothing."""
    valid, z = samples(src, fmt, depth_scale)
    H, W = valid.shape
    h_full, w_full = size_full
    h, w = (h_full, w_full) if crop is None else crop
    mx = resample_ref.axis_matrix(W, w_full, w)
    my = resample_ref.axis_matrix(H, h_full, h)
    num = my @ (z @ mx.T)
    den = my @ (valid.astype(np.float64) @ mx.T)
    ok = (den > 0) & (den >= min_coverage)
    return np.where(ok, num / np.where(ok, den, 1.0), 0.0), np.where(ok, den, 0.0), den


# ---- the loss -----------------------------------------------------------------------------------------------------------------
def select(D, Z, w_t, w_p=None):
    """-> (selected bool, w float32) from float32 planes: a = w_t > 0 ? w_t : 0, b likewise (1 without w_p), w = a * b in f32;
    selected iff w > 0 and Z, D finite and > 0.  w is 0 where not selected."""
    D, Z, w_t = (torch.as_tensor(v, dtype=torch.float32) for v in (D, Z, w_t))
    a = torch.where(w_t > 0, w_t, torch.zeros_like(w_t))
    if w_p is None:
        b = torch.ones_like(a)
    else:
        w_p = torch.as_tensor(w_p, dtype=torch.float32)
        b = torch.where(w_p > 0, w_p, torch.zeros_like(w_p))
    w = a * b
    selected = (w > 0) & torch.isfinite(Z) & (Z > 0) & torch.isfinite(D) & (D > 0)
    return selected, torch.where(selected, w, torch.zeros_like(w))


def fit(S_w, S_y, S_x, S_yy, S_xy):
    """(s, t) = argmin sum w (s y + t - x)^2 from the five moments; s = 0, t = S_x / S_w when det is not above
    DEGENERATE * S_w * S_yy (a constant target, a single pixel).  Tensors of one dtype; differentiable."""
    det = S_w * S_yy - S_y * S_y
    if not bool(det > DEGENERATE * (S_w * S_yy)):
        return torch.zeros_like(S_w), S_x / S_w
    s = (S_w * S_xy - S_y * S_x) / det
    return s, (S_x - s * S_y) / S_w


def spaces(D, Z, selected, flags, dtype):
    """-> (x, y) in dtype, 0 where not selected; D may require grad"""
    one = torch.ones((), dtype=dtype)
    Ds = torch.where(selected, D.to(dtype), one)
    Zs = torch.where(selected, torch.as_tensor(Z, dtype=torch.float32).to(dtype), one)
    x = 1.0 / Ds if flags & INVERT_PREDICTED else Ds
    y = 1.0 / Zs if flags & INVERT_TARGET else Zs
    zero = torch.zeros((), dtype=dtype)
    return torch.where(selected, x, zero), torch.where(selected, y, zero)


def moments(w, x, y):
    wy = w * y
    return w.sum(), wy.sum(), (w * x).sum(), (wy * y).sum(), (wy * x).sum()


def loss_through_fit(D, Z, w_t, w_p, flags, dtype=torch.float64):
    """The loss as a differentiable function of D (a tensor of `dtype`, may require grad) with the fit NOT detached and not
    rounded: what autograd differentiates for the envelope check.  Selection is taken from D's float32 value."""
    selected, w32 = select(D.detach().to(torch.float32), Z, w_t, w_p)
    w = w32.to(dtype)
    x, y = spaces(D, Z, selected, flags, dtype)
    if not bool(selected.any()):
        return (D * 0).sum()
    if flags & ALIGN:
        s, t = fit(*moments(w, x, y))
    else:
        s, t = torch.ones((), dtype=dtype), torch.zeros((), dtype=dtype)
    r = torch.where(selected, x - (s * y + t), torch.zeros((), dtype=dtype))
    rho = r * r if flags & L2 else r.abs()
    return (w * rho).sum() / w.sum()


def evaluate(D, Z, w_t, w_p=None, flags=0, upstream=1.0, dtype=torch.float64, round_terms=True):
    """The header, in `dtype`: -> dict(terms (8,) of {L, S_w, s, t, number selected, 0, 0, 0}, grad (H,W), selected, r, w).
    round_terms: s and t are rounded once to f32 before the residual is formed, and the gradient divides by the f32 value of
    S_w, as the library does (its backward reads them from loss_terms); False: nothing is rounded.  The gradient holds s and t
    fixed: grad = upstream * w rho'(r) / S_w * dx/dD, exactly +0 where not selected.  Nothing selected: zeros."""
    D32 = torch.as_tensor(D, dtype=torch.float32)
    selected, w32 = select(D32, Z, w_t, w_p)
    w = w32.to(dtype)
    x, y = spaces(D32, Z, selected, flags, dtype)
    zero = torch.zeros((), dtype=dtype)
    if not bool(selected.any()):
        return dict(terms=torch.zeros(LOSS_TERMS, dtype=dtype), grad=torch.zeros(D32.shape, dtype=dtype), selected=selected,
                    r=torch.zeros(D32.shape, dtype=dtype), w=w)
    if flags & ALIGN:
        s, t = fit(*moments(w, x, y))
    else:
        s, t = torch.ones((), dtype=dtype), zero
    if round_terms:
        s, t = s.to(torch.float32).to(dtype), t.to(torch.float32).to(dtype)
    r = torch.where(selected, x - (s * y + t), zero)
    rho = r * r if flags & L2 else r.abs()
    S_w = w.sum()
    L = (w * rho).sum() / S_w
    slope = 2.0 * r if flags & L2 else torch.sign(r)
    grad = float(upstream) * w * slope / (S_w.to(torch.float32).to(dtype) if round_terms else S_w)
    if flags & INVERT_PREDICTED:
        grad = grad * -(x * x)
    grad = torch.where(selected, grad, zero)
    terms = torch.stack([L, S_w, s, t, selected.sum().to(dtype), zero, zero, zero])
    return dict(terms=terms, grad=grad, selected=selected, r=r, w=w)
