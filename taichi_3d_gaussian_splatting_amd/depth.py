"""Depth supervision (include/gs_depth.h, csrc/k_depth.hip): depth priors -- lidar or RGB-D depth in metres, or a monocular
network's relative inverse depth -- as training targets on the device, and a fused masked depth loss on the rasteriser's depth
output: the "depth regularisation" of the INRIA trainer and the depth loss of gsplat.

  store = DepthStore.from_dataset(train_dataset, device)                 # every depth map resident, 16 bits a sample
  Z, w_t = store.target(view, downsample_factor, min_coverage=0.5)       # one launch: depth and validity weight, (h,w) each
  term = depth_loss(image_depth, Z, w_t, pixel_weight, space="inverse", norm="l1", align=False)
  (loss + config.weight_at(iteration) * term).backward()                 # needs rasterisation.config.differentiable_depth
  term.terms                                                             # {L, S_w, s, t, selected, 0, 0, 0} on the device

A depth map has holes (a zero in a 16-bit file; anything not finite and > 0 in a float one).  A hole is never interpolated
across: the target is the filtered mean of the valid samples under the antialias filter of the colour target, and its weight is
the share of the filter they cover, zero below min_coverage.  The loss selects the pixels where weight, target and rendered
depth are all usable; every other pixel adds nothing and gets a gradient of exactly 0.

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
from ._terms import MAX_PIXELS, check_plane                # (MAX_PIXELS and ROW_PITCH_ALIGN: the bounds of gs_depth.h, kept as names here)
from .targets import ROW_PITCH_ALIGN, ResidentStore, _pitched

FORMAT_U16, FORMAT_F32 = 0, 1                   # GS_DEPTH_U16, GS_DEPTH_F32
INVERT_PREDICTED, INVERT_TARGET, L2, ALIGN = 1, 2, 4, 8     # GS_DEPTH_INVERT_PREDICTED, _INVERT_TARGET, _L2, _ALIGN
FLAGS_ALL = 15                                  # GS_DEPTH_FLAGS_ALL
PIXELS_PER_BLOCK = 1024                         # GS_DEPTH_PIXELS_PER_BLOCK
FINISH_THREADS = 256                            # GS_DEPTH_FINISH_THREADS
MOMENTS = 5                                     # GS_DEPTH_MOMENTS
LOSS_TERMS = 8                                  # GS_DEPTH_LOSS_TERMS
FORWARD_LAUNCHES, FORWARD_LAUNCHES_ALIGN, BACKWARD_LAUNCHES = 2, 4, 1      # GS_DEPTH_*_LAUNCHES*
DEFAULT_DEPTH_SCALE = 0.001                     # metres per unit of a 16-bit depth file without a depth_scale: millimetres

_VP, _I32, _I64, _F32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
ARGTYPES = {
    # (ctx, src, src_format, H_in, W_in, src_row_pitch_bytes, depth_scale, h_full, w_full, h_out, w_out, min_coverage, dst, stream)
    "gs_depth_resample": [_VP, _VP, _I32, _I32, _I32, _I64, _F32, _I32, _I32, _I32, _I32, _F32, _VP, _VP],
    # (ctx, D, Z, w_t, w_p, H, W, flags, loss_terms, stream)
    "gs_depth_loss_forward": [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _VP, _VP],
    # (ctx, D, Z, w_t, w_p, H, W, flags, loss_terms, upstream, grad_D, stream)
    "gs_depth_loss_backward": [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _VP, _VP, _VP, _VP],
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


# ---- validation: reads no data, launches nothing ----------------------------------------------------------------------------
def loss_flags(space: str = "inverse", norm: str = "l1", align: bool = False, target_is_inverse: bool = False) -> int:
    """The flag bits of a loss: space "depth" | "inverse" is the space the residual is formed in; target_is_inverse says the
    target already holds inverse depth (a monocular prior) and is used as stored, which needs space "inverse"."""
    if space not in ("depth", "inverse"):
        raise ValueError(f'space must be "depth" or "inverse", got {space!r}')
    if norm not in ("l1", "l2"):
        raise ValueError(f'norm must be "l1" or "l2", got {norm!r}')
    if target_is_inverse and space != "inverse":
        raise ValueError('a target that holds inverse depth needs space="inverse"')
    flags = 0
    if space == "inverse":
        flags |= INVERT_PREDICTED
        if not target_is_inverse:
            flags |= INVERT_TARGET
    if norm == "l2":
        flags |= L2
    if align:
        flags |= ALIGN
    return flags


def _check_flags(flags):
    flags = int(flags)
    if flags & ~FLAGS_ALL:
        raise ValueError(f"unknown flag bits in {flags}")
    return flags


def _check_resample_scalars(depth_scale, min_coverage):
    depth_scale, min_coverage = float(depth_scale), float(min_coverage)
    if not (math.isfinite(depth_scale) and depth_scale > 0.0):
        raise ValueError(f"depth_scale must be finite and > 0, got {depth_scale}")
    if not 0.0 <= min_coverage <= 1.0:
        raise ValueError(f"min_coverage must be in [0, 1], got {min_coverage}")
    return depth_scale, min_coverage


def _source_layout(src):
    """-> (format, H, W, row pitch in bytes) of a depth source, or an error"""
    if not isinstance(src, torch.Tensor):
        raise TypeError("the depth source must be a tensor")
    if src.dtype not in (torch.uint16, torch.float32):
        raise TypeError(f"the depth source must be uint16 or float32, got {src.dtype}")
    if src.dim() != 2:
        raise ValueError(f"the depth source must be (H,W), got {tuple(src.shape)}")
    H, W = int(src.shape[0]), int(src.shape[1])
    if src.dtype == torch.uint16:
        if H > 0 and W > 0 and (src.stride(1) != 1 or (H > 1 and src.stride(0) < W)):
            raise ValueError("a uint16 depth source must have dense rows and a row stride >= W")
        fmt, pitch = FORMAT_U16, 2 * (src.stride(0) if H > 1 else W)
    else:
        if not src.is_contiguous():
            raise ValueError("a float32 depth source must be contiguous")
        fmt, pitch = FORMAT_F32, 4 * W
    if not src.is_cuda:
        raise ValueError(f"depth targets are resampled on the GPU: the source is on {src.device}, move it to a cuda/hip device first "
                         "(there is no CPU path)")
    return fmt, H, W, pitch


# ---- the calls --------------------------------------------------------------------------------------------------------------
def depth_resample(src: torch.Tensor, size_full: Tuple[int, int], size_out: Optional[Tuple[int, int]] = None, depth_scale: float = 1.0,
                   min_coverage: float = 0.5, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gs_depth_resample: -> (2, h_out, w_out) f32: plane 0 the depth target, plane 1 its weight, of the top-left size_out crop
    (default: all) of the antialiased resize of src to size_full, holes left out.  src: uint16 (H,W) with any row stride
    (0 is a hole, a sample is v * depth_scale) or contiguous f32 (H,W) (anything not finite and > 0 is a hole).  The weight is
    the share of the filter the valid samples cover, 0 where that is below min_coverage.  Queued on the current stream of the
    source's device; no host synchronisation.  out: the contiguous f32 (2,h_out,w_out) tensor to write."""
    depth_scale, min_coverage = _check_resample_scalars(depth_scale, min_coverage)
    fmt, H, W, pitch = _source_layout(src)
    h_full, w_full = int(size_full[0]), int(size_full[1])
    h_out, w_out = (h_full, w_full) if size_out is None else (int(size_out[0]), int(size_out[1]))
    if out is None:
        if min(h_out, w_out) < 0:
            raise ValueError("the output size must not be negative")
        out = torch.empty((2, h_out, w_out), dtype=torch.float32, device=src.device)
    elif out.dtype != torch.float32 or out.device != src.device or tuple(out.shape) != (2, h_out, w_out) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 (2,{h_out},{w_out}) tensor on {src.device}")
    _bind()
    _native.call("gs_depth_resample", src.device, _native.shared_ctx(src.device), _native.ptr(src), fmt, H, W, pitch, depth_scale,
                 h_full, w_full, h_out, w_out, min_coverage, _native.ptr(out))
    return out


def _check_loss_inputs(depth, target, target_weight, pixel_weight):
    # what is wrong with a tensor is found before any device is looked at
    for device in (False, True):
        check_plane(depth, "depth", device=device)
        check_plane(target, "target", depth, device=device)
        check_plane(target_weight, "target_weight", depth, device=device)
        if pixel_weight is not None:
            check_plane(pixel_weight, "pixel_weight", depth, device=device)


def depth_loss_forward(depth, target, target_weight, pixel_weight=None, flags: int = 0, terms=None):
    """gs_depth_loss_forward, no autograd: -> the 8 loss terms {L, S_w, s, t, number selected, 0, 0, 0} on the device"""
    flags = _check_flags(flags)
    _check_loss_inputs(depth, target, target_weight, pixel_weight)
    if terms is None:
        terms = torch.empty(LOSS_TERMS, dtype=torch.float32, device=depth.device)
    _bind()
    H, W = int(depth.shape[0]), int(depth.shape[1])
    _native.call("gs_depth_loss_forward", depth.device, _native.shared_ctx(depth.device), depth.data_ptr(), target.data_ptr(),
                 target_weight.data_ptr(), None if pixel_weight is None else pixel_weight.data_ptr(), H, W, flags, terms.data_ptr())
    return terms


def depth_loss_backward(depth, target, target_weight, pixel_weight, flags: int, terms, upstream=None, out=None):
    """gs_depth_loss_backward, no autograd: -> grad_depth (H,W), every element written.  upstream: one float32 on the device
    (None: 1).  The fit (terms[2], terms[3]) is held fixed."""
    flags = _check_flags(flags)
    _check_loss_inputs(depth, target, target_weight, pixel_weight)
    if out is None:
        out = torch.empty_like(depth)
    else:
        check_plane(out, "out", depth)
    _terms.check_upstream(upstream, depth)
    _bind()
    H, W = int(depth.shape[0]), int(depth.shape[1])
    _native.call("gs_depth_loss_backward", depth.device, _native.shared_ctx(depth.device), depth.data_ptr(), target.data_ptr(),
                 target_weight.data_ptr(), None if pixel_weight is None else pixel_weight.data_ptr(), H, W, flags, terms.data_ptr(),
                 None if upstream is None else upstream.data_ptr(), out.data_ptr())
    return out


def depth_loss_flags(depth, target, target_weight, pixel_weight=None, flags: int = 0):
    """depth_loss() by its flag bits (loss_flags): what a caller that fixed them once calls per step"""
    flags = _check_flags(flags)
    _check_loss_inputs(depth, target, target_weight, pixel_weight)
    return _terms.depth_term(depth, depth_loss_forward, depth_loss_backward,
                             dict(target=target, target_weight=target_weight, pixel_weight=pixel_weight), dict(flags=flags))


def depth_loss(depth, target, target_weight, pixel_weight=None, space: str = "inverse", norm: str = "l1", align: bool = False,
               target_is_inverse: bool = False):
    """-> the scalar depth loss sum w rho(x - (s y + t)) / sum w over the selected pixels of contiguous float32 (H,W) GPU
    planes: `depth` the rendered depth, `target` and `target_weight` the two planes DepthStore.target() returns, pixel_weight an
    optional second weight (the loss's mask).  Differentiable in `depth` only.  space: the residual in "depth" (x = D, y = Z) or
    "inverse" depth (x = 1/D, y = 1/Z; with target_is_inverse y = Z as stored); norm "l1" or "l2"; align: the closed-form
    scale and shift (s, t) that fit the target to the rendering, held fixed in the backward.  The result's `.terms` is the
    (8,) tensor {L, S_w, s, t, number selected, 0, 0, 0} on the device: s and t can be logged without a second pass.
    A pixel is selected iff its weights are > 0 and target and depth are finite and > 0; nothing selected gives 0."""
    return depth_loss_flags(depth, target, target_weight, pixel_weight, loss_flags(space, norm, align, target_is_inverse))


# ---- configuration ----------------------------------------------------------------------------------------------------------
@dataclass
class DepthConfig:
    """space, norm: of the loss.  The loss's weight falls (or rises) exponentially from weight_init at iteration 0 to
    weight_final at num_iterations (None: the trainer fills in its own).  min_coverage: of the target's weight.  depth_scale:
    metres per unit of a 16-bit file whose record has no depth_scale (None: DEFAULT_DEPTH_SCALE)."""
    space: str = "inverse"
    norm: str = "l1"
    weight_init: float = 1.0
    weight_final: float = 0.01
    num_iterations: Optional[int] = None
    min_coverage: float = 0.5
    depth_scale: Optional[float] = None

    def check(self):
        loss_flags(self.space, self.norm)
        if not (math.isfinite(self.weight_init) and math.isfinite(self.weight_final) and self.weight_init > 0.0 and self.weight_final > 0.0):
            raise ValueError("weight_init and weight_final must be finite and > 0")
        if self.num_iterations is not None and self.num_iterations < 1:
            raise ValueError("num_iterations must be >= 1")
        _check_resample_scalars(1.0 if self.depth_scale is None else self.depth_scale, self.min_coverage)

    def weight_at(self, iteration: int) -> float:
        """exp((1 - t) log weight_init + t log weight_final), t = iteration / num_iterations clipped to [0, 1]"""
        if self.num_iterations is None:
            return float(self.weight_init)
        t = min(max(float(iteration) / float(self.num_iterations), 0.0), 1.0)
        return float(math.exp((1.0 - t) * math.log(self.weight_init) + t * math.log(self.weight_final)))


# ---- the depth maps of a dataset --------------------------------------------------------------------------------------------
class DepthStore(ResidentStore):
    """The depth maps of a dataset resident on one device -- uint16 with 16-byte aligned rows as the 16-bit PNG held them, f32
    for .npy files -- and the per-step depth target made from them there.  A view without a depth file holds None.  target()
    returns the store's buffer of that geometry, overwritten by the next target() of the same geometry."""
    column, holds = "depth_path", "depth map"

    def __init__(self, maps, scales, sizes, device):
        super().__init__(maps, sizes, device)
        self.maps, self.scales = self.records, list(scales)

    @classmethod
    def from_dataset(cls, dataset, device="cuda", depth_scale: Optional[float] = None, require_all: bool = True) -> "DepthStore":
        """Every record's depth map (dataset.load_depth), decoded once.  A 16-bit map's metres per unit: the record's
        depth_scale, else the argument, else DEFAULT_DEPTH_SCALE.  require_all: a record without a depth_path is an error
        (False: its view holds None, as the validation set may)."""
        device = cls.on_gpu(device)
        maps, scales, sizes = [], [], []
        for item in cls._decode(dataset.load_depth, len(dataset), require_all):
            if item is None:
                maps.append(None); scales.append(None); sizes.append(None)
                continue
            depth_hw, scale = item
            H, W = depth_hw.shape
            if depth_hw.dtype == np.uint16:
                scale = scale if scale is not None else (depth_scale if depth_scale is not None else DEFAULT_DEPTH_SCALE)
                maps.append(_pitched(depth_hw, device))
            else:
                scale = 1.0                 # metres as stored; kept as the dataset's crop, which a contiguous plane must be
                maps.append(torch.from_numpy(np.ascontiguousarray(depth_hw[:H - H % 16, :W - W % 16], dtype=np.float32)).to(device))
            scales.append(_check_resample_scalars(scale, 0.0)[0])
            sizes.append((H - H % 16, W - W % 16))                     # the dataset's crop of the picture
        return cls(maps, scales, sizes, device)

    def target(self, i: int, downsample_factor: int = 1, min_coverage: float = 0.5):
        """-> (depth (h,w) f32, weight (h,w) f32) of view i at the factor: the two planes of one (2,h,w) buffer, written by one
        launch, with the geometry of the colour target (targets.downsampled_geometry of the picture's size).  After the first
        use of a geometry the call allocates nothing on the device and does not synchronise."""
        size_full, size, out = self._buffer(i, downsample_factor, 2)
        depth_resample(self._source(i), size_full, size, depth_scale=self.scales[i], min_coverage=min_coverage, out=out)
        return out[0], out[1]


# ---- the trainer's term -----------------------------------------------------------------------------------------------------
class DepthTerm(_terms.TrainerTerm):
    """GaussianPointCloudTrainer's depth term: depth_loss of the rendered depth against the dataset's depth_path maps, by the
    weight schedule of its DepthConfig; with mode "relative" the fitted scale and shift are logged with it"""
    name = "depth"

    def __init__(self, mode: str, config: Optional[DepthConfig], train_config):
        """mode, config: the trainer's depth ("metric" | "relative") and depth_config arguments, checked here against its
        TrainConfig; nothing is read from disk and no device is touched before load()"""
        super().__init__()
        config = config or DepthConfig()
        config.check()
        if mode == "relative" and config.space != "inverse":
            raise ValueError('depth="relative" needs depth_config.space="inverse": the files hold relative inverse depth')
        _terms.check_depth_is_rendered(train_config, f'depth="{mode}"', "depth targets are made on the device")
        if config.num_iterations is None:
            config = dataclasses.replace(config, num_iterations=max(int(train_config.num_iterations), 1))
        self.mode, self.config, self.weight_at = mode, config, config.weight_at
        self.flags = loss_flags(config.space, config.norm, align=mode == "relative", target_is_inverse=mode == "relative")

    def load(self, train_dataset, val_dataset, device):
        self.load_stores(DepthStore, train_dataset, val_dataset, device, f'depth="{self.mode}"', depth_scale=self.config.depth_scale)

    def value(self, split, view, downsample_factor, image_depth, image_gt, camera_info, pixel_weight):
        """the store's target and weight at the factor (one launch) and the fused loss on the rendered depth"""
        store = self.stores[split]
        if not store.has(view):
            return None
        target, target_weight = store.target(view, downsample_factor, self.config.min_coverage)
        return depth_loss_flags(image_depth, target, target_weight, pixel_weight, self.flags)

    def train_scalars(self, terms):
        scalars = super().train_scalars(terms)              # terms: {L, S_w, s, t, ...}
        if self.mode == "relative":
            scalars += [("train/depth scale", terms[2]), ("train/depth shift", terms[3])]
        return scalars


def trainer_terms(mode: str, config: Optional[DepthConfig], train_config) -> list:
    """the terms of a trainer's depth and depth_config arguments: a DepthTerm, or none for depth="none" """
    if mode not in ("none", "metric", "relative"):
        raise ValueError(f'depth must be "none", "metric" or "relative", got {mode!r}')
    if mode == "none" and config is not None:
        raise ValueError('depth_config needs depth="metric" or "relative"')
    return [] if mode == "none" else [DepthTerm(mode, config, train_config)]
