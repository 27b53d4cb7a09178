"""Geometry regularisers on the rendered depth (include/gs_geometry.h, csrc/k_geometry.hip): the camera-space normal of the
rendered surface, a cosine loss of it against a monocular normal prior (the normal prior of MonoSDF; the depth-to-normal step of
2DGS and GOF), and an edge-aware smoothness of the depth (RegNeRF, DNGaussian, Monodepth) -- what constrains geometry between
the cameras of a sparse-view run, and what keeps depth noise out of a fused mesh.

  n = depth_normals(image_depth, camera_info.camera_intrinsics)                       # (3,h,w), (0,0,-1) faces the camera
  store = NormalStore.from_dataset(train_dataset, device)                            # every normal prior resident
  prior, w_n = store.target(view, downsample_factor)                                 # one launch: (3,h,w) and its weight (h,w)
  a = normal_loss(image_depth, intrinsics, prior, w_n, pixel_weight, unit_range=store.unit_range(view), convention="opengl")
  b = depth_smoothness(image_depth, image_gt, pixel_weight, space="inverse", order=1, edge_lambda=10.0)
  (loss + 0.05 * a + 0.01 * b).backward()                                            # needs rasterisation.config.differentiable_depth
  a.terms, b.terms                                                                   # {L, S_w, number selected, mean cos | 0, 0...}

Both losses are differentiable in the depth only.  A term is selected, not multiplied: a hole in the depth, a zero weight, a
pixel without a prior, a normal across a depth edge add nothing and get a gradient of exactly 0.

There is no fallback path: every call goes through _native.call(), and a CPU tensor is refused.
"""
import ctypes as C
import dataclasses
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native, _terms
from ._terms import check_plane
from .targets import ResidentStore, _pitched, image_resample

PRIOR_UNIT_RANGE, PRIOR_FLIP_YZ, NORMAL_FLAGS_ALL = 1, 2, 3        # GS_GEOM_PRIOR_UNIT_RANGE, _PRIOR_FLIP_YZ, _NORMAL_FLAGS_ALL
INVERSE, SECOND_ORDER, SMOOTH_FLAGS_ALL = 4, 8, 12                  # GS_GEOM_INVERSE, _SECOND_ORDER, _SMOOTH_FLAGS_ALL
TILE_W, TILE_H, HALO = 64, 16, 2                                    # GS_GEOM_TILE_W, _TILE_H, _HALO
FINISH_THREADS = 256                                                # GS_GEOM_FINISH_THREADS
LOSS_TERMS = 8                                                      # GS_GEOM_LOSS_TERMS
FORWARD_LAUNCHES, BACKWARD_LAUNCHES = 2, 1                          # GS_GEOM_*_LAUNCHES
NO_PRIOR_U8 = 128               # what a pixel without a prior is stored as: (128,128,128) decodes to a normal of length ~0

_VP, _I32, _F32 = C.c_void_p, C.c_int32, C.c_float
ARGTYPES = {
    # (ctx, D, H, W, fx, fy, cx, cy, max_rel_jump, normals, stream)
    "gs_depth_normals": [_VP, _VP, _I32, _I32, _F32, _F32, _F32, _F32, _F32, _VP, _VP],
    # (ctx, D, N, w_n, w_p, H, W, fx, fy, cx, cy, max_rel_jump, flags, terms, stream)
    "gs_normal_loss_forward": [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _F32, _F32, _F32, _F32, _F32, _I32, _VP, _VP],
    # (ctx, D, N, w_n, w_p, H, W, fx, fy, cx, cy, max_rel_jump, flags, terms, upstream, grad_D, stream)
    "gs_normal_loss_backward": [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _F32, _F32, _F32, _F32, _F32, _I32, _VP, _VP, _VP, _VP],
    # (ctx, D, I, w_p, H, W, edge_lambda, flags, terms, stream)
    "gs_depth_smooth_forward": [_VP, _VP, _VP, _VP, _I32, _I32, _F32, _I32, _VP, _VP],
    # (ctx, D, I, w_p, H, W, edge_lambda, flags, terms, upstream, grad_D, stream)
    "gs_depth_smooth_backward": [_VP, _VP, _VP, _VP, _I32, _I32, _F32, _I32, _VP, _VP, _VP, _VP],
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


# ---- validation: reads no device data, launches nothing ---------------------------------------------------------------------
def normal_flags(unit_range: bool = True, convention: str = "opencv") -> int:
    """The flag bits of a normal loss.  unit_range: the prior holds (n + 1) / 2 (an 8-bit normal image resampled to [0, 1]).
    convention: the camera frame the prior is in -- "opencv" (x right, y down, z forward: the rasteriser's) or "opengl" (y up,
    z towards the viewer: what most normal networks write)"""
    if convention not in ("opencv", "opengl"):
        raise ValueError(f'convention must be "opencv" or "opengl", got {convention!r}')
    return (PRIOR_UNIT_RANGE if unit_range else 0) | (PRIOR_FLIP_YZ if convention == "opengl" else 0)


def smooth_flags(space: str = "inverse", order: int = 1) -> int:
    """The flag bits of a smoothness term: in "depth" or "inverse" depth, of first or second order"""
    if space not in ("depth", "inverse"):
        raise ValueError(f'space must be "depth" or "inverse", got {space!r}')
    if order not in (1, 2):
        raise ValueError(f"order must be 1 or 2, got {order!r}")
    return (INVERSE if space == "inverse" else 0) | (SECOND_ORDER if order == 2 else 0)


def _non_negative(value, what):
    value = float(value)
    if not (math.isfinite(value) and value >= 0.0):
        raise ValueError(f"{what} must be finite and >= 0, got {value}")
    return value


def intrinsics_tuple(camera_intrinsics) -> Tuple[float, float, float, float]:
    """(fx, fy, cx, cy) as floats, from four numbers or from a 3x3 intrinsics tensor.  A tensor on a device is read by the
    host here: do it once per view and factor, not once per step."""
    if isinstance(camera_intrinsics, torch.Tensor):
        if tuple(camera_intrinsics.shape) != (3, 3):
            raise ValueError(f"camera_intrinsics must be a 3x3 tensor or (fx, fy, cx, cy), got shape {tuple(camera_intrinsics.shape)}")
        k = camera_intrinsics.detach().to("cpu", torch.float32)
        values = (float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2]))
    else:
        values = tuple(float(v) for v in camera_intrinsics)
        if len(values) != 4:
            raise ValueError(f"camera_intrinsics must be a 3x3 tensor or (fx, fy, cx, cy), got {len(values)} numbers")
    fx, fy, cx, cy = values
    if not (math.isfinite(fx) and math.isfinite(fy) and fx > 0.0 and fy > 0.0):
        raise ValueError(f"fx and fy must be finite and > 0, got {fx}, {fy}")
    if not (math.isfinite(cx) and math.isfinite(cy)):
        raise ValueError(f"cx and cy must be finite, got {cx}, {cy}")
    return values


def check_image(image, what, like, device=True):
    """Raise unless `image` is a contiguous float32 (3,H,W) tensor of the depth's size (and, with device=True, on its device)"""
    if not isinstance(image, torch.Tensor):
        raise TypeError(f"{what} must be a tensor")
    if image.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {image.dtype}")
    if image.dim() != 3 or tuple(image.shape) != (3,) + tuple(like.shape):
        raise ValueError(f"{what} must be (3,H,W) of the depth's size {tuple(like.shape)}, got {tuple(image.shape)}")
    if not image.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    if device and image.device != like.device:
        raise ValueError(f"{what} is on {image.device}, the depth on {like.device}")


def _check_flags(flags, allowed):
    flags = int(flags)
    if flags & ~allowed:
        raise ValueError(f"unknown flag bits in {flags}")
    return flags


def _check_normal_inputs(depth, prior, prior_weight, pixel_weight):
    # what is wrong with a tensor is found before any device is looked at
    for device in (False, True):
        check_plane(depth, "depth", device=device)
        check_image(prior, "prior", depth, device=device)
        check_plane(prior_weight, "prior_weight", depth, device=device)
        if pixel_weight is not None:
            check_plane(pixel_weight, "pixel_weight", depth, device=device)


def _check_smooth_inputs(depth, guide, pixel_weight):
    for device in (False, True):
        check_plane(depth, "depth", device=device)
        if guide is not None:
            check_image(guide, "guide", depth, device=device)
        if pixel_weight is not None:
            check_plane(pixel_weight, "pixel_weight", depth, device=device)


def _ptr(tensor):
    return None if tensor is None else tensor.data_ptr()


# ---- the calls --------------------------------------------------------------------------------------------------------------
def depth_normals(depth: torch.Tensor, camera_intrinsics, max_rel_jump: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gs_depth_normals: -> (3,H,W) f32, the camera-space unit normal of the surface a contiguous float32 (H,W) GPU depth map
    shows (x right, y down, z forward; a wall facing the camera is (0,0,-1)), from central differences of the back-projected
    points; (0,0,0) where there is none: at the border, at or next to a hole, and -- with max_rel_jump > 0 -- where the depth
    changes by more than max_rel_jump times itself across the pixel.  camera_intrinsics: the 3x3 tensor of a CameraInfo (read
    by the host: see intrinsics_tuple) or (fx, fy, cx, cy).  Queued on the current stream; no host synchronisation."""
    check_plane(depth, "depth", device=False)
    fx, fy, cx, cy = intrinsics_tuple(camera_intrinsics)
    max_rel_jump = _non_negative(max_rel_jump, "max_rel_jump")
    check_plane(depth, "depth")
    H, W = int(depth.shape[0]), int(depth.shape[1])
    if out is None:
        out = torch.empty((3, H, W), dtype=torch.float32, device=depth.device)
    else:
        check_image(out, "out", depth)
    _bind()
    _native.call("gs_depth_normals", depth.device, _native.shared_ctx(depth.device), depth.data_ptr(), H, W, fx, fy, cx, cy, max_rel_jump,
                 out.data_ptr())
    return out


def normal_loss_forward(depth, intrinsics, prior, prior_weight, pixel_weight=None, max_rel_jump: float = 0.1, flags: int = 0, terms=None):
    """gs_normal_loss_forward, no autograd: -> the 8 terms {L, S_w, number selected, mean cos, 0, 0, 0, 0} on the device"""
    flags = _check_flags(flags, NORMAL_FLAGS_ALL)
    fx, fy, cx, cy = intrinsics_tuple(intrinsics)
    max_rel_jump = _non_negative(max_rel_jump, "max_rel_jump")
    _check_normal_inputs(depth, prior, prior_weight, pixel_weight)
    if terms is None:
        terms = torch.empty(LOSS_TERMS, dtype=torch.float32, device=depth.device)
    _bind()
    H, W = int(depth.shape[0]), int(depth.shape[1])
    _native.call("gs_normal_loss_forward", depth.device, _native.shared_ctx(depth.device), depth.data_ptr(), prior.data_ptr(),
                 prior_weight.data_ptr(), _ptr(pixel_weight), H, W, fx, fy, cx, cy, max_rel_jump, flags, terms.data_ptr())
    return terms


def normal_loss_backward(depth, intrinsics, prior, prior_weight, pixel_weight, max_rel_jump: float, flags: int, terms, upstream=None, out=None):
    """gs_normal_loss_backward, no autograd: -> grad_depth (H,W), every element written.  upstream: one float32 on the device
    (None: 1)"""
    flags = _check_flags(flags, NORMAL_FLAGS_ALL)
    fx, fy, cx, cy = intrinsics_tuple(intrinsics)
    max_rel_jump = _non_negative(max_rel_jump, "max_rel_jump")
    _check_normal_inputs(depth, prior, prior_weight, pixel_weight)
    if out is None:
        out = torch.empty_like(depth)
    else:
        check_plane(out, "out", depth)
    _terms.check_upstream(upstream, depth)
    _bind()
    H, W = int(depth.shape[0]), int(depth.shape[1])
    _native.call("gs_normal_loss_backward", depth.device, _native.shared_ctx(depth.device), depth.data_ptr(), prior.data_ptr(),
                 prior_weight.data_ptr(), _ptr(pixel_weight), H, W, fx, fy, cx, cy, max_rel_jump, flags, terms.data_ptr(), _ptr(upstream),
                 out.data_ptr())
    return out


def depth_smooth_forward(depth, guide=None, pixel_weight=None, edge_lambda: float = 10.0, flags: int = 0, terms=None):
    """gs_depth_smooth_forward, no autograd: -> the 8 terms {L, S_w, number of selected terms, 0, 0, 0, 0, 0} on the device"""
    flags = _check_flags(flags, SMOOTH_FLAGS_ALL)
    edge_lambda = _non_negative(edge_lambda, "edge_lambda")
    _check_smooth_inputs(depth, guide, pixel_weight)
    if terms is None:
        terms = torch.empty(LOSS_TERMS, dtype=torch.float32, device=depth.device)
    _bind()
    H, W = int(depth.shape[0]), int(depth.shape[1])
    _native.call("gs_depth_smooth_forward", depth.device, _native.shared_ctx(depth.device), depth.data_ptr(), _ptr(guide), _ptr(pixel_weight),
                 H, W, edge_lambda, flags, terms.data_ptr())
    return terms


def depth_smooth_backward(depth, guide, pixel_weight, edge_lambda: float, flags: int, terms, upstream=None, out=None):
    """gs_depth_smooth_backward, no autograd: -> grad_depth (H,W), every element written"""
    flags = _check_flags(flags, SMOOTH_FLAGS_ALL)
    edge_lambda = _non_negative(edge_lambda, "edge_lambda")
    _check_smooth_inputs(depth, guide, pixel_weight)
    if out is None:
        out = torch.empty_like(depth)
    else:
        check_plane(out, "out", depth)
    _terms.check_upstream(upstream, depth)
    _bind()
    H, W = int(depth.shape[0]), int(depth.shape[1])
    _native.call("gs_depth_smooth_backward", depth.device, _native.shared_ctx(depth.device), depth.data_ptr(), _ptr(guide), _ptr(pixel_weight),
                 H, W, edge_lambda, flags, terms.data_ptr(), _ptr(upstream), out.data_ptr())
    return out


def normal_loss_flags(depth, intrinsics, prior, prior_weight, pixel_weight=None, max_rel_jump: float = 0.1, flags: int = 0):
    """normal_loss() by its flag bits (normal_flags) and an (fx, fy, cx, cy) tuple: what a caller that fixed them once calls per
    step"""
    flags = _check_flags(flags, NORMAL_FLAGS_ALL)
    intrinsics = intrinsics_tuple(intrinsics)
    max_rel_jump = _non_negative(max_rel_jump, "max_rel_jump")
    _check_normal_inputs(depth, prior, prior_weight, pixel_weight)
    return _terms.depth_term(depth, normal_loss_forward, normal_loss_backward, dict(prior=prior, prior_weight=prior_weight, pixel_weight=pixel_weight),
                             dict(intrinsics=intrinsics, max_rel_jump=max_rel_jump, flags=flags))


def normal_loss(depth, intrinsics, prior, prior_weight, pixel_weight=None, unit_range: bool = True, convention: str = "opencv",
                max_rel_jump: float = 0.1):
    """-> the scalar sum w (1 - n . h) / sum w over the selected pixels: n the depth-derived normal (depth_normals) of the
    contiguous float32 (H,W) GPU plane `depth`, h the unit normal the prior (3,H,W) holds -- as (h + 1) / 2 with unit_range, in
    the camera frame `convention` names -- and w = prior_weight * pixel_weight.  A pixel is selected iff its normal exists (not
    across a depth change of more than max_rel_jump times the depth; 0: no such test), the decoded prior is at least 0.5 long
    and w > 0.  Differentiable in `depth` only; the gradient at a pixel gathers what the normals at its four neighbours owe it.
    The result's `.terms` is the (8,) tensor {L, S_w, number selected, mean n . h, 0, 0, 0, 0} on the device."""
    return normal_loss_flags(depth, intrinsics, prior, prior_weight, pixel_weight, max_rel_jump, normal_flags(unit_range, convention))


def depth_smoothness_flags(depth, guide=None, pixel_weight=None, edge_lambda: float = 10.0, flags: int = 0):
    """depth_smoothness() by its flag bits (smooth_flags)"""
    flags = _check_flags(flags, SMOOTH_FLAGS_ALL)
    edge_lambda = _non_negative(edge_lambda, "edge_lambda")
    _check_smooth_inputs(depth, guide, pixel_weight)
    return _terms.depth_term(depth, depth_smooth_forward, depth_smooth_backward, dict(guide=guide, pixel_weight=pixel_weight),
                             dict(edge_lambda=edge_lambda, flags=flags))


def depth_smoothness(depth, guide=None, pixel_weight=None, space: str = "inverse", order: int = 1, edge_lambda: float = 10.0):
    """-> the scalar sum w e |d x| / sum w: x the depth (space="depth") or its inverse, d x the difference of horizontal and
    vertical neighbours (order=1) or the second difference x(p-1) - 2 x(p) + x(p+1) (order=2: a slanted plane costs nothing in
    depth space), w the product of the pixel weights of the pixels of a term, e = exp(-edge_lambda mean_rgb |d guide|) over
    the term's outer pixels: the smoothness is relaxed across an edge of the (3,H,W) guide image (the colour target).  A term
    with a hole in the depth or a zero weight is left out.  Differentiable in `depth` only.  `.terms` of the result:
    {L, S_w, number of selected terms, 0, ...} on the device."""
    return depth_smoothness_flags(depth, guide, pixel_weight, edge_lambda, smooth_flags(space, order))


# ---- configuration ----------------------------------------------------------------------------------------------------------
@dataclass
class GeometryConfig:
    """The trainer's geometry terms; a weight of 0 switches a term off, and the weights are constant from start_iteration on.
    smooth_*: of depth_smoothness (the guide is the colour target).  normal_*: of normal_loss against the dataset's normal_path
    priors.  consistency_*: of normals.normal_consistency between the rendered Gaussian normals and the normal of the rendered
    depth, which needs no data."""
    smooth_weight: float = 0.0
    smooth_space: str = "inverse"
    smooth_order: int = 1
    smooth_edge_lambda: float = 10.0
    normal_weight: float = 0.0
    normal_convention: str = "opencv"
    normal_max_rel_jump: float = 0.1
    start_iteration: int = 0
    consistency_weight: float = 0.0
    consistency_min_length: float = 0.5
    consistency_max_rel_jump: float = 0.1

    def check(self):
        smooth_flags(self.smooth_space, self.smooth_order)
        normal_flags(True, self.normal_convention)
        _non_negative(self.smooth_weight, "smooth_weight")
        _non_negative(self.normal_weight, "normal_weight")
        _non_negative(self.smooth_edge_lambda, "smooth_edge_lambda")
        _non_negative(self.normal_max_rel_jump, "normal_max_rel_jump")
        if int(self.start_iteration) != self.start_iteration or self.start_iteration < 0:
            raise ValueError(f"start_iteration must be an integer >= 0, got {self.start_iteration}")
        _non_negative(self.consistency_weight, "consistency_weight")
        _non_negative(self.consistency_max_rel_jump, "consistency_max_rel_jump")
        if not (math.isfinite(float(self.consistency_min_length)) and self.consistency_min_length > 0.0):
            raise ValueError(f"consistency_min_length must be finite and > 0, got {self.consistency_min_length}")
        if self.smooth_weight == 0.0 and self.normal_weight == 0.0 and self.consistency_weight == 0.0:
            raise ValueError("a GeometryConfig needs smooth_weight > 0, normal_weight > 0 or consistency_weight > 0")


# ---- the normal priors of a dataset -----------------------------------------------------------------------------------------
def _prior_u8(normal_hw3: np.ndarray) -> torch.Tensor:
    """an 8-bit (H,W,3) normal image as (H,W,4) uint8: channel 3 is 255 where the pixel holds a prior (is not all zero), and a
    pixel without one is NO_PRIOR_U8 grey, so that the filter's mix with it only shortens the decoded normal"""
    has = normal_hw3.any(axis=2)
    out = np.empty(normal_hw3.shape[:2] + (4,), dtype=np.uint8)
    out[:, :, :3] = np.where(has[:, :, None], normal_hw3, NO_PRIOR_U8)
    out[:, :, 3] = np.where(has, 255, 0)
    return torch.from_numpy(out)


def _prior_f32(normal_hw3: np.ndarray, H: int, W: int) -> torch.Tensor:
    """a float (H,W,3) normal map as contiguous (4,H,W) f32 of the dataset's crop: channel 3 is 1 where the pixel holds a prior
    (finite and not all zero); a pixel without one is zero"""
    has = np.isfinite(normal_hw3).all(axis=2) & (normal_hw3 != 0).any(axis=2)
    out = np.zeros((4, H, W), dtype=np.float32)
    out[:3] = np.where(has[:, :, None], normal_hw3, 0.0).transpose(2, 0, 1)[:, :H, :W]
    out[3] = has[:H, :W]
    return torch.from_numpy(out)


class NormalStore(ResidentStore):
    """The normal priors of a dataset resident on one device -- uint8 (H,W,4) with 16-byte aligned rows for 8-bit images, f32
    (4,H,W) for .npy files, the fourth channel the prior's validity -- and the per-step prior made from them there by
    targets.image_resample, with the geometry of the colour target.  A view without a prior holds None.  target() returns the
    store's buffer of that geometry, overwritten by the next target() of the same geometry."""
    column, holds = "normal_path", "normal prior"

    def __init__(self, priors, sizes, device):
        super().__init__(priors, sizes, device)
        self.priors = self.records

    def unit_range(self, i: int) -> bool:
        """whether view i's prior holds (n + 1) / 2 (an 8-bit image) and not n itself (a .npy file)"""
        return self.priors[i].dtype == torch.uint8

    @classmethod
    def from_dataset(cls, dataset, device="cuda", require_all: bool = True) -> "NormalStore":
        """Every record's normal prior (dataset.load_normal), decoded once.  require_all: a record without a normal_path is an
        error (False: its view holds None, as the validation set may)."""
        device = cls.on_gpu(device)
        priors, sizes = [], []
        for normal in cls._decode(dataset.load_normal, len(dataset), require_all):
            if normal is None:
                priors.append(None); sizes.append(None)
                continue
            H, W = normal.shape[0] - normal.shape[0] % 16, normal.shape[1] - normal.shape[1] % 16     # the dataset's crop of the picture
            if normal.dtype == np.uint8:
                priors.append(_pitched(_prior_u8(normal), device))
            else:
                priors.append(_prior_f32(normal, H, W).to(device))
            sizes.append((H, W))
        return cls(priors, sizes, device)

    def target(self, i: int, downsample_factor: int = 1):
        """-> (prior (3,h,w) f32, weight (h,w) f32) of view i at the factor: out[:3] and out[3] of one (4,h,w) buffer, written
        by one launch.  The weight is the share of the filter that pixels with a prior cover.  After the first use of a geometry
        the call allocates nothing on the device and does not synchronise."""
        size_full, size, out = self._buffer(i, downsample_factor, 4)
        image_resample(self._source(i), size_full, size, out=out, alpha=True)
        return out[:3], out[3]


# ---- the trainer's terms ----------------------------------------------------------------------------------------------------
class _GeometryTerm(_terms.TrainerTerm):
    """a term of a checked GeometryConfig: constant weight <name>_weight from start_iteration on"""

    def __init__(self, config: GeometryConfig):
        super().__init__()
        self.config, self.start_iteration, self.weight = config, config.start_iteration, getattr(config, f"{self.name}_weight")

    def weight_at(self, iteration):
        return self.weight

    def bind(self, trainer):
        """called once by the trainer that sums the term, before the first value(): a term that needs more of a step than
        value() is given (normals.ConsistencyTerm) keeps the trainer"""


class SmoothTerm(_GeometryTerm):
    """depth_smoothness of the rendered depth with the colour target as its guide: it needs no data of its own"""
    name = "smooth"

    def __init__(self, config):
        super().__init__(config)
        self.flags = smooth_flags(config.smooth_space, config.smooth_order)

    def value(self, split, view, downsample_factor, image_depth, image_gt, camera_info, pixel_weight):
        return depth_smoothness_flags(image_depth, image_gt, pixel_weight, self.config.smooth_edge_lambda, self.flags)


class NormalTerm(_GeometryTerm):
    """normal_loss of the rendered depth against the dataset's normal_path priors, resident on the device"""
    name = "normal"

    def __init__(self, config):
        super().__init__(config)
        self._intrinsics = {}                       # (split, view, factor) -> (fx, fy, cx, cy), read by the host once

    def load(self, train_dataset, val_dataset, device):
        self.load_stores(NormalStore, train_dataset, val_dataset, device, "geometry.normal_weight > 0")

    def value(self, split, view, downsample_factor, image_depth, image_gt, camera_info, pixel_weight):
        """the cosine loss against the view's prior at the factor (one launch for the prior)"""
        store = self.stores[split]
        if not store.has(view):
            return None
        key = (split, view, downsample_factor)
        intrinsics = self._intrinsics.get(key)
        if intrinsics is None:
            intrinsics = self._intrinsics[key] = intrinsics_tuple(camera_info.camera_intrinsics)
        prior, prior_weight = store.target(view, downsample_factor)
        return normal_loss_flags(image_depth, intrinsics, prior, prior_weight, pixel_weight, self.config.normal_max_rel_jump,
                                 normal_flags(store.unit_range(view), self.config.normal_convention))


def trainer_terms(geometry: Optional[GeometryConfig], train_config) -> list:
    """the terms of a trainer's geometry argument, checked against its TrainConfig, over a copy of it: smoothness, normal prior,
    then normal consistency, each if its weight is > 0; nothing is read from disk and no device is touched before their load()"""
    if geometry is None:
        return []
    if not isinstance(geometry, GeometryConfig):
        raise ValueError(f"geometry must be a GeometryConfig or None, got {type(geometry).__name__}")
    geometry.check()
    _terms.check_depth_is_rendered(train_config, "geometry", "its guide and priors are made on the device")
    config = dataclasses.replace(geometry)
    from .normals import ConsistencyTerm                 # (normals.py builds on this module)
    return [term(config) for term in (SmoothTerm, NormalTerm, ConsistencyTerm) if getattr(config, f"{term.name}_weight") > 0.0]


def normals_to_uint8(normals: torch.Tensor) -> torch.Tensor:
    """(3,H,W) unit normals -> (H,W,3) uint8 holding round((n + 1) / 2 * 255), and (0,0,0) where there is no normal: the 8-bit
    encoding load_normal reads.  Plain torch on whichever device the normals are."""
    has = (normals != 0).any(dim=0, keepdim=True)
    coded = torch.clamp(torch.round((normals + 1.0) * 127.5), 0, 255)
    return torch.where(has, coded, torch.zeros_like(coded)).to(torch.uint8).permute(1, 2, 0).contiguous()
