"""The scene as a Gaussian mixture on the GPU (include/gs_mixture.h, csrc/k_mixture.hip): what the reference's FTGMM.py does.

Weights sigmoid(opacity logit), normalised over the rows that take part (mask byte 0, finite position / q / log s / logit,
|q|^2 > 0); means the positions; covariances R S^2 R^T with R the rotation of q / |q| and S = diag(exp(log s)).

log_density() / density() evaluate the mixture at arbitrary points, fourier() its closed-form Fourier transform
sum_i pi_i exp(-1/2 k^T Sigma_i k - i k.(mu_i - centre)) at arbitrary frequencies (radians per unit): brute force, every row in
every output, no cutoff, bit-reproducible.  bounding_box(), sample_grid() and frequency_grid() are the reference's
estimate_gmm_bbox (without the plots), get_sample_coords and get_fourier_coords; density_volume() and fourier_volume() put them
together, and compare_volume_to_transform() (alias ft_grab_scene) returns the reference's two numbers -- the mean absolute
difference and the cosine similarity between the DFT of the sampled volume and the analytic transform -- without printing
or plotting.  The grid helpers are plain torch and work on any device; nothing here reads a value back to the host.

log_density(), density(), fourier() and the two volumes are differentiable to the scene's parameters (and the density to x):
mixture_grad.py, include/gs_mixture_grad.h.

There is no fallback path: the two evaluations go through _native.call(), and a CPU tensor is refused.
"""
import ctypes as C
import math
from dataclasses import dataclass

import torch

from . import _native, mixture_grad

MAX_POINTS = 2 ** 30
MAX_QUERIES = 2 ** 30
# the blocking of the pair kernels (GS_MIX_POINTS_PER_WG, GS_MIX_CHUNK in k_mixture.hip): queries per workgroup, and the unit
# of the component loop -- a chunk of it is a whole number of these
POINTS_PER_WORKGROUP = 512
COMPONENTS_PER_CHUNK = 256
N_FEATURES = 56

_VP, _I64 = C.c_void_p, C.c_int64
ARGTYPES = {
    # (ctx, point_cloud, point_cloud_features, point_invalid_mask, n_points, x, n_x, log_density_out, stream)
    "gs_mixture_log_density": [_VP, _VP, _VP, _VP, _I64, _VP, _I64, _VP, _VP],
    # (ctx, point_cloud, point_cloud_features, point_invalid_mask, n_points, k, n_k, centre, re_im_out, stream)
    "gs_mixture_fourier": [_VP, _VP, _VP, _VP, _I64, _VP, _I64, _VP, _VP, _VP],
}
_bound = False


def _bind():
    """argtypes of the entry points, set once on the loaded library (they are not part of _native.SYMBOLS)"""
    global _bound
    if not _bound:
        L = _native.lib()
        for name, argtypes in ARGTYPES.items():
            if not hasattr(L, name):
                raise _native.NativeLibraryError(f"{_native.LIB_PATH} does not export {name}")
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
        _bound = True


def _tensors(scene_or_tensors):
    """(point_cloud, point_cloud_features, point_invalid_mask or None) of a scene object or of a tuple of two or three tensors"""
    s = scene_or_tensors
    if isinstance(s, (tuple, list)):
        if len(s) not in (2, 3):
            raise ValueError("expected (point_cloud, point_cloud_features[, point_invalid_mask])")
        return s[0], s[1], (s[2] if len(s) == 3 else None)
    return s.point_cloud, s.point_cloud_features, getattr(s, "point_invalid_mask", None)


def _f32(t):
    t = t.detach()
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.to(torch.float32).contiguous()


def _check(scene_or_tensors, queries, what):
    pc, feat, mask = _tensors(scene_or_tensors)
    if not isinstance(pc, torch.Tensor) or pc.dim() != 2 or pc.shape[1] != 3:
        raise ValueError("point_cloud must be an (N,3) tensor")
    if not isinstance(feat, torch.Tensor) or feat.shape != (pc.shape[0], N_FEATURES):
        raise ValueError(f"point_cloud_features must be an (N,{N_FEATURES}) tensor")
    if not isinstance(queries, torch.Tensor) or queries.dim() != 2 or queries.shape[1] != 3:
        raise ValueError(f"{what} must be a (P,3) tensor")
    if not pc.is_cuda:
        raise ValueError(f"the mixture is evaluated on the GPU: point_cloud is on {pc.device}, move the scene to a cuda/hip "
                         "device first (there is no CPU path)")
    if feat.device != pc.device or queries.device != pc.device:
        raise ValueError(f"point_cloud_features and {what} must be on the point cloud's device ({pc.device}): the mixture is "
                         "evaluated on the GPU")
    if pc.shape[0] > MAX_POINTS or queries.shape[0] > MAX_QUERIES:
        raise ValueError(f"at most {MAX_POINTS} rows and {MAX_QUERIES} queries per call")
    if mask is not None:
        if mask.device != pc.device or mask.shape != (pc.shape[0],):
            raise ValueError("point_invalid_mask must be an (N,) tensor on the point cloud's device")
        mask = mask if mask.dtype == torch.int8 and mask.is_contiguous() else (mask != 0).to(torch.int8).contiguous()
    return _f32(pc), _f32(feat), mask, _f32(queries)


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def _log_density(pc, feat, mask, x):
    """the library call on checked f32 tensors"""
    out = torch.full((x.shape[0],), -math.inf, dtype=torch.float32, device=pc.device)
    _native.call("gs_mixture_log_density", pc.device, _native.shared_ctx(pc.device), _native.ptr(pc), _native.ptr(feat),
                 _native.ptr(mask), pc.shape[0], _native.ptr(x), x.shape[0], _native.ptr(out))
    return out


def log_density(scene_or_tensors, x):
    """-> (P,) f32: log sum_i pi_i N(x; mu_i, Sigma_i) at the rows of x (P,3); -inf everywhere if no row takes part, NaN for a
    non-finite row of x.  Queued on the current stream of the scene's device; no host synchronisation.
    Differentiable (mixture_grad.LogDensity, the same bits) when grad mode is on and point_cloud, point_cloud_features or x
    requires a gradient: to the positions, to q / log s / opacity logit (the SH columns get zeros) and to x."""
    _bind()
    pc, feat, mask, x32 = _check(scene_or_tensors, x, "x")
    raw_pc, raw_feat, _ = _tensors(scene_or_tensors)
    if _wants_grad(raw_pc, raw_feat, x):
        return mixture_grad.LogDensity.apply(raw_pc, raw_feat, x, mask)
    return _log_density(pc, feat, mask, x32)


def density(scene_or_tensors, x):
    """-> (P,) f32: exp(log_density); differentiable like it"""
    return log_density(scene_or_tensors, x).exp()


def _centre(centre, device):
    centre = torch.as_tensor(centre, dtype=torch.float32, device=device).detach().reshape(-1).contiguous()
    if centre.shape[0] != 3:
        raise ValueError("centre must hold 3 values")
    return centre


def _fourier(pc, feat, mask, k, centre):
    """the library call on checked f32 tensors -> (P,2) f32, real and imaginary part"""
    out = torch.zeros((k.shape[0], 2), dtype=torch.float32, device=pc.device)
    _native.call("gs_mixture_fourier", pc.device, _native.shared_ctx(pc.device), _native.ptr(pc), _native.ptr(feat),
                 _native.ptr(mask), pc.shape[0], _native.ptr(k), k.shape[0], _native.ptr(centre), _native.ptr(out))
    return out


def fourier(scene_or_tensors, k, centre):
    """-> (P,) complex64: sum_i pi_i exp(-1/2 k^T Sigma_i k - i k.(mu_i - centre)) at the rows of k (P,3), radians per unit;
    centre a tensor of 3 (it stays on the device).  0 everywhere if no row takes part, NaN for a non-finite row of k.
    Differentiable to point_cloud and point_cloud_features (mixture_grad.Fourier, the same bits) when grad mode is on and one
    of them requires a gradient.  k and centre get no gradient: asking for one is an error, not a silent zero."""
    for name, t in (("k", k), ("centre", centre)):
        if _wants_grad(t):
            raise ValueError(f"{name} requires a gradient, and the transform has none to {name}: detach it")
    _bind()
    pc, feat, mask, k32 = _check(scene_or_tensors, k, "k")
    raw_pc, raw_feat, _ = _tensors(scene_or_tensors)
    if _wants_grad(raw_pc, raw_feat):
        return torch.view_as_complex(mixture_grad.Fourier.apply(raw_pc, raw_feat, k, centre, mask))
    return torch.view_as_complex(_fourier(pc, feat, mask, k32, _centre(centre, pc.device)))


def takes_part(scene_or_tensors):
    """-> (N,) bool: the rows that enter the mixture (the rule of gs_mixture.h)"""
    pc, feat, mask = _tensors(scene_or_tensors)
    head = feat[:, :8]
    part = torch.isfinite(pc).all(1) & torch.isfinite(head).all(1) & (head[:, :4].double().square().sum(1) > 0)
    return part if mask is None else part & (mask == 0)


def bounding_box(scene_or_tensors, n_std=3.0):
    """-> (2,3) f32 on the scene's device: per axis, mean -+ n_std population standard deviations of the means of the rows that
    take part (the reference's estimate_gmm_bbox: a normal fit per axis, 3 deviations).  Detached: the box is where the mixture
    is looked at, not a quantity a gradient goes through, so density_volume / fourier_volume differentiate through the two
    evaluations at fixed sample points and frequencies."""
    pc = _tensors(scene_or_tensors)[0]
    part = takes_part(scene_or_tensors)
    w = part.to(torch.float64).unsqueeze(1)
    mu = torch.where(part.unsqueeze(1), pc.detach().to(torch.float64), torch.zeros((), dtype=torch.float64, device=pc.device))
    count = w.sum()
    mean = mu.sum(0) / count
    std = (((mu - mean) * w).square().sum(0) / count).sqrt()
    return torch.stack([mean - n_std * std, mean + n_std * std]).to(torch.float32)


def _linspace(lo, hi, steps):
    """torch.linspace(lo, hi, steps) for 0-dim f32 tensors without reading lo and hi back, in the CPU kernel's arithmetic: an f32
    step, one fused multiply-add from the start up to the middle and from the end beyond it (the product of two f32 is exact
    in float64, so the float64 sum rounded to f32 is that fused operation)"""
    i = torch.arange(steps, device=lo.device, dtype=torch.float64)
    step = ((hi - lo) / (steps - 1 if steps > 1 else 1)).to(torch.float64)
    lo, hi = lo.to(torch.float64), hi.to(torch.float64)
    return torch.where(i < steps // 2, lo + step * i, hi - step * (steps - 1 - i)).to(torch.float32)


def sample_grid(bbox, G):
    """-> (G,G,G,3) f32: the reference's get_sample_coords, G samples per axis from bbox[0] to bbox[1] inclusive, 'ij' order"""
    bbox = bbox.to(torch.float32)
    axes = [_linspace(bbox[0, a], bbox[1, a], G) for a in range(3)]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1)


def frequency_grid(bbox, G, sample_spacing=False, shift=True):
    """-> (G,G,G,3) f32, radians per unit: the reference's get_fourier_coords, fftfreq(G, d = L / G) * 2 pi per axis with
    L = bbox[1] - bbox[0], then fftshift.  sample_spacing=True takes d = L / (G - 1), the spacing sample_grid() really has;
    shift=False leaves the DFT's own order."""
    bbox = bbox.to(torch.float32)
    L = (bbox[1] - bbox[0]).to(torch.float64)
    d = L / (G - 1 if sample_spacing else G)
    scale = (1.0 / (G * d)).to(torch.float32)
    index = torch.arange(G, device=bbox.device, dtype=torch.float32)
    index = torch.where(index >= (G + 1) // 2, index - G, index)
    axes = [index * scale[a] * 2 * math.pi for a in range(3)]
    k = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1)
    return torch.fft.fftshift(k, dim=(0, 1, 2)) if shift else k


def density_volume(scene_or_tensors, G=35, bbox=None):
    """-> (G,G,G) f32: the mixture's density on sample_grid(bbox, G) (the reference's sample_gmm); bbox defaults to
    bounding_box(scene).  Differentiable like density()."""
    bbox = bounding_box(scene_or_tensors) if bbox is None else bbox
    return density(scene_or_tensors, sample_grid(bbox, G).reshape(-1, 3)).reshape(G, G, G)


def fourier_volume(scene_or_tensors, G=35, bbox=None, sample_spacing=False, shift=True, centre=None):
    """-> (G,G,G) complex64: the analytic transform on frequency_grid(bbox, G, ...), phases relative to the middle of the box
    (the reference's transform_gmm_to_fourier1) or to `centre`.  Differentiable like fourier(); a bbox or centre that requires a
    gradient is detached here."""
    bbox = bounding_box(scene_or_tensors) if bbox is None else bbox
    bbox = bbox.detach()
    centre = (bbox[0] + bbox[1]) / 2.0 if centre is None else torch.as_tensor(centre).detach()
    k = frequency_grid(bbox, G, sample_spacing, shift).reshape(-1, 3)
    return fourier(scene_or_tensors, k, centre).reshape(G, G, G)


@dataclass
class MixtureReport:
    """The two numbers of the reference's compare_gmm_volume_to_transforms, as 0-dim tensors on the scene's device"""
    mean_abs_difference: torch.Tensor
    cosine_similarity: torch.Tensor
    grid_size: int
    consistent: bool

    def as_floats(self):
        """(mean_abs_difference, cosine_similarity) on the host: this waits for the device"""
        return float(self.mean_abs_difference), float(self.cosine_similarity)


def compare(volume_dft, transform):
    """mean |a - b| and the cosine similarity Re<a, b> / (|a| |b|) of two complex volumes, as the reference forms them"""
    diff = (volume_dft - transform).abs().mean()
    num = (volume_dft.real * transform.real + volume_dft.imag * transform.imag).sum()
    den = ((volume_dft.real ** 2 + volume_dft.imag ** 2).sum() * (transform.real ** 2 + transform.imag ** 2).sum()).sqrt()
    return diff, num / den


def compare_volume_to_transform(scene_or_tensors, G=35, bbox=None, consistent=False):
    """The reference's ft_grab_scene without prints and plots: sample the density on a G^3 grid, normalise it to sum 1, take
    its DFT (torch.fft.fftn on the device) and compare it with the analytic transform on the matching frequencies.
    consistent=False is the reference's convention as written (spacing L / G, fftshift, phases relative to the middle of the
    box), under which the two volumes differ by construction; consistent=True takes the frequencies of the true sample
    spacing L / (G - 1), unshifted, with phases relative to the first sample, under which they agree up to aliasing."""
    bbox = bounding_box(scene_or_tensors) if bbox is None else bbox
    volume = density_volume(scene_or_tensors, G, bbox)
    dft = torch.fft.fftn(volume / volume.sum())
    if consistent:
        analytic = fourier_volume(scene_or_tensors, G, bbox, sample_spacing=True, shift=False, centre=bbox[0])
    else:
        dft = torch.fft.fftshift(dft, dim=(0, 1, 2))
        analytic = fourier_volume(scene_or_tensors, G, bbox)
    diff, cosine = compare(dft, analytic)
    return MixtureReport(diff, cosine, int(G), bool(consistent))


ft_grab_scene = compare_volume_to_transform
