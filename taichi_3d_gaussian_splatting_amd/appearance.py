"""Per-view exposure compensation (include/gs_appearance.h, csrc/k_appearance.hip): a learnable 3x4 affine colour transform
per training image, applied to the rendered image in front of the loss and trained with the scene -- the "exposure
optimisation" of the INRIA trainer -- and the colour-corrected metrics of the NeRF-W / Mip-NeRF 360 protocol for views that
have no trained transform: fit the best affine map from a rendering to its ground truth, then measure.

  table = AppearanceTable(len(train_dataset), device, AppearanceConfig(num_iterations=30_000))
  corrected = apply(image_pred.permute(2, 0, 1), table.row(view))       # read and written where the rasteriser left it
  loss, _, _ = loss_function(corrected, image_gt, clamp_predicted=True)
  loss.backward()                                                         # row.grad lands in row `view` of table.grad
  optimizer.step(); position_optimizer.step(); table.step(view, iteration)

  psnr_cc = psnr(apply(rendered, fit_affine(rendered, image_gt)), image_gt)          # validation

A transform is 12 floats, row-major M = [A | b]: corrected_i = ((A_i0 x_0 + A_i1 x_1) + A_i2 x_2) + b_i.  Scene colours and
transforms are determined only up to a common factor: what a trained table means is the ratio between
views, not a row on its own.

There is no fallback path: every call goes through _native.call(), and a CPU tensor is refused.
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native
from ._native import GsLossImage

PIXELS_PER_BLOCK = 1024                         # GS_APPEARANCE_PIXELS_PER_BLOCK
FINISH_THREADS = 256                            # GS_APPEARANCE_FINISH_THREADS
FINISH_BLOCKS_BACKWARD, FINISH_BLOCKS_MOMENTS = 12, 23      # GS_APPEARANCE_FINISH_BLOCKS_*
TRANSFORM_FLOATS = 12                           # GS_APPEARANCE_TRANSFORM_FLOATS
MOMENTS = 23                                    # GS_APPEARANCE_MOMENTS
MAX_PIXELS = 2 ** 31 - 2048                     # GS_APPEARANCE_MAX_PIXELS
# moments[0..9]: the upper triangle of sum w u u^T, u = (x_0, x_1, x_2, 1), in this order
UPPER_TRIANGLE = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)

_VP, _I32, _IMG = C.c_void_p, C.c_int32, C.POINTER(GsLossImage)
ARGTYPES = {
    # (ctx, image, transform, H, W, corrected, stream)
    "gs_appearance_apply": [_VP, _IMG, _VP, _I32, _I32, _IMG, _VP],
    # (ctx, image, grad_corrected, transform, H, W, grad_image, grad_transform, stream)
    "gs_appearance_backward": [_VP, _IMG, _IMG, _VP, _I32, _I32, _IMG, _VP, _VP],
    # (ctx, image, target, pixel_weight, H, W, moments, stream)
    "gs_appearance_moments": [_VP, _IMG, _IMG, _VP, _I32, _I32, _VP, _VP],
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
def check_image(image, what="image"):
    """Raise unless `image` is a float32 (3,H,W) tensor on a GPU (any strides)"""
    if not isinstance(image, torch.Tensor):
        raise TypeError(f"{what} must be a tensor")
    if image.dim() != 3 or image.shape[0] != 3 or image.shape[1] < 1 or image.shape[2] < 1:
        raise ValueError(f"{what} must be (3,H,W) with H, W >= 1, got {tuple(image.shape)}")
    if image.shape[1] * image.shape[2] > MAX_PIXELS:
        raise ValueError(f"{what} has more than {MAX_PIXELS} pixels")
    if image.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {image.dtype}")
    if not image.is_cuda:
        raise ValueError(f"exposure compensation runs on the GPU: {what} must be on a cuda/hip device (there is no CPU path)")


def check_like(other, image, what):
    """Raise unless `other` is a float32 tensor of image's shape on image's device"""
    check_image(other, what)
    if other.shape != image.shape:
        raise ValueError(f"{what} must have the image's shape {tuple(image.shape)}, got {tuple(other.shape)}")
    if other.device != image.device:
        raise ValueError(f"{what} is on {other.device}, the image on {image.device}")


def check_transform(transform, image):
    """Raise unless `transform` is a contiguous float32 (12,) tensor on the image's device (a row of a (V,12) table is)"""
    if not isinstance(transform, torch.Tensor):
        raise TypeError("transform must be a tensor")
    if tuple(transform.shape) != (TRANSFORM_FLOATS,):
        raise ValueError(f"transform must be ({TRANSFORM_FLOATS},), row-major [A | b], got {tuple(transform.shape)}")
    if transform.dtype != torch.float32:
        raise TypeError(f"transform must be float32, got {transform.dtype}")
    if transform.device != image.device:
        raise ValueError(f"transform is on {transform.device}, the image on {image.device}")
    if not transform.is_contiguous():
        raise ValueError("transform must be contiguous")


def check_weight(pixel_weight, image):
    """Raise unless pixel_weight is a contiguous float32 (H,W) tensor on the image's device"""
    if not isinstance(pixel_weight, torch.Tensor):
        raise TypeError("pixel_weight must be a tensor")
    if tuple(pixel_weight.shape) != tuple(image.shape[1:]):
        raise ValueError(f"pixel_weight must be {tuple(image.shape[1:])}, got {tuple(pixel_weight.shape)}")
    if pixel_weight.dtype != torch.float32:
        raise TypeError(f"pixel_weight must be float32, got {pixel_weight.dtype}")
    if pixel_weight.device != image.device:
        raise ValueError(f"pixel_weight is on {pixel_weight.device}, the image on {image.device}")
    if not pixel_weight.is_contiguous():
        raise ValueError("pixel_weight must be contiguous")


# ---- the three calls --------------------------------------------------------------------------------------------------------
def apply_forward(image, transform, out=None):
    """gs_appearance_apply, no autograd: -> the corrected image, in image's strides when they are dense (preserve_format).
    out: where to write instead -- `image` itself for in place, or any float32 tensor of its shape that does not overlap it."""
    check_image(image)
    check_transform(transform, image)
    if out is None:
        out = torch.empty_like(image, memory_format=torch.preserve_format)
    else:
        check_like(out, image, "out")
    _bind()
    H, W = int(image.shape[1]), int(image.shape[2])
    _native.call("gs_appearance_apply", image.device, _native.shared_ctx(image.device), GsLossImage.of(image), transform.data_ptr(), H, W,
                 GsLossImage.of(out))
    return out


def apply_backward(image, grad_corrected, transform, grad_image=True, grad_transform=True):
    """gs_appearance_backward, no autograd: -> (grad_image or None, grad_transform or None).  Either flag may be a tensor to
    write into: grad_image a float32 tensor of the image's shape (any strides), grad_transform a contiguous (12,) one -- every
    element is written, not added.  A pixel whose three upstream values are exactly 0 is left out of every sum and gets a
    gradient of exactly 0, whatever the image holds there."""
    check_image(image)
    check_like(grad_corrected, image, "grad_corrected")
    check_transform(transform, image)
    if grad_image is True:
        grad_image = torch.empty_like(image, memory_format=torch.preserve_format)
    elif grad_image is False or grad_image is None:
        grad_image = None
    else:
        check_like(grad_image, image, "grad_image")
    if grad_transform is True:
        grad_transform = torch.empty(TRANSFORM_FLOATS, dtype=torch.float32, device=image.device)
    elif grad_transform is False or grad_transform is None:
        grad_transform = None
    else:
        check_transform(grad_transform, image)
    if grad_image is None and grad_transform is None:
        raise ValueError("apply_backward: nothing to compute (grad_image and grad_transform are both off)")
    _bind()
    H, W = int(image.shape[1]), int(image.shape[2])
    _native.call("gs_appearance_backward", image.device, _native.shared_ctx(image.device), GsLossImage.of(image), GsLossImage.of(grad_corrected),
                 transform.data_ptr(), H, W, None if grad_image is None else GsLossImage.of(grad_image),
                 None if grad_transform is None else grad_transform.data_ptr())
    return grad_image, grad_transform


class _Apply(torch.autograd.Function):
    """apply() as an autograd node.  A transform that names a `grad_out` tensor (AppearanceTable.row sets it, and sets the
    row's .grad to the same memory) has its gradient WRITTEN there by the backward's own launch, and autograd is handed
    nothing for it: the gradient is in the table without a copy or an add.  Such a row feeds one apply() per backward.  Any
    other transform gets its gradient the usual way, accumulated into .grad."""

    @staticmethod
    def forward(ctx, image, transform, grad_out):
        corrected = apply_forward(image.detach(), transform.detach())
        ctx.save_for_backward(image, transform)
        ctx.grad_out = grad_out
        return corrected

    @staticmethod
    def backward(ctx, grad_corrected):
        image, transform = ctx.saved_tensors
        want_image, want_transform = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_image or want_transform):
            return None, None, None
        if grad_corrected.dtype != torch.float32:
            grad_corrected = grad_corrected.to(torch.float32)
        direct = want_transform and ctx.grad_out is not None
        grad_image, grad_transform = apply_backward(image.detach(), grad_corrected, transform.detach(), grad_image=want_image,
                                                    grad_transform=ctx.grad_out if direct else want_transform)
        return grad_image, (None if direct else grad_transform), None


def apply(image, transform):
    """-> the corrected image ((A_i0 x_0 + A_i1 x_1) + A_i2 x_2) + b_i of a float32 (3,H,W) GPU image of any strides and a
    (12,) transform [A | b]; differentiable in both.  The result has image's strides when they are dense (the rasteriser's
    (H,W,3) output under permute(2,0,1) stays interleaved), so LossFunction(..., clamp_predicted=True) reads it in place."""
    check_image(image)
    check_transform(transform, image)
    grad_out = getattr(transform, "grad_out", None)
    if grad_out is not None:
        check_transform(grad_out, image)
    return _Apply.apply(image, transform, grad_out)


def moments(image, target, pixel_weight=None):
    """gs_appearance_moments: -> 23 float64 values on the device: the 10 upper-triangle entries of sum w u u^T (UPPER_TRIANGLE,
    u = (x_0, x_1, x_2, 1)), the 12 entries of sum w y_i u_j and sum w.  w = pixel_weight where that is > 0, else 0 (weight 0
    selects: such a pixel is not read into any sum); None: 1."""
    check_image(image)
    check_like(target, image, "target")
    if pixel_weight is not None:
        check_weight(pixel_weight, image)
    _bind()
    out = torch.empty(MOMENTS, dtype=torch.float64, device=image.device)
    H, W = int(image.shape[1]), int(image.shape[2])
    _native.call("gs_appearance_moments", image.device, _native.shared_ctx(image.device), GsLossImage.of(image.detach()),
                 GsLossImage.of(target.detach()), None if pixel_weight is None else pixel_weight.data_ptr(), H, W, out.data_ptr())
    return out


def solve_affine(moments23) -> np.ndarray:
    """The least-squares affine map of 23 moments (any sequence of numbers, on the host): -> (12,) float64, row-major [A | b],
    the solution of (sum w u u^T) M_i^T = sum w y_i u.  The identity when sum w == 0, when a moment is not finite or when the
    4x4 system is singular (a constant image: its condition number is beyond 1e12)."""
    m = np.asarray(moments23, dtype=np.float64).reshape(MOMENTS)
    identity = np.asarray(IDENTITY, dtype=np.float64)
    if not np.all(np.isfinite(m)) or not m[22] > 0.0:
        return identity
    G = np.zeros((4, 4), dtype=np.float64)
    for value, (i, j) in zip(m[:10], UPPER_TRIANGLE):
        G[i, j] = G[j, i] = value
    B = m[10:22].reshape(3, 4)
    # scale-free singularity test: the Gram matrix of the columns scaled to unit diagonal
    d = np.sqrt(np.diag(G))
    if not np.all(d > 0.0):
        return identity
    Gn = G / np.outer(d, d)
    if not np.linalg.cond(Gn) < 1e12:
        return identity
    try:
        M = np.linalg.solve(Gn, (B / d).T).T / d
    except np.linalg.LinAlgError:
        return identity
    return M.reshape(12) if np.all(np.isfinite(M)) else identity


def fit_affine(image, target, pixel_weight=None):
    """-> the (12,) float32 transform on the image's device that maps `image` onto `target` best in the (weighted) least-squares
    sense.  The 23 moments are read to the host -- the one host read -- and the 4x4 system is solved there in float64.  The
    identity when the system is singular or no pixel has a positive weight."""
    m = moments(image, target, pixel_weight).cpu().numpy()
    return torch.from_numpy(solve_affine(m).astype(np.float32)).to(image.device)


# ---- the table of a training set -------------------------------------------------------------------------------------------
@dataclass
class AppearanceConfig:
    """lr falls exponentially from lr at iteration 0 to lr_final at num_iterations (the INRIA trainer's exposure schedule,
    without its warm-up delay).  num_iterations None: the trainer fills in its own.  eps is FusedAdam's."""
    lr: float = 0.01
    lr_final: float = 0.001
    num_iterations: Optional[int] = None
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8

    def check(self):
        if not (math.isfinite(self.lr) and math.isfinite(self.lr_final) and self.lr > 0.0 and self.lr_final > 0.0):
            raise ValueError("lr and lr_final must be finite and > 0")
        if self.num_iterations is not None and self.num_iterations < 1:
            raise ValueError("num_iterations must be >= 1")
        if not (0.0 <= self.betas[0] < 1.0 and 0.0 <= self.betas[1] < 1.0 and self.eps > 0.0):
            raise ValueError("betas must be in [0, 1) and eps > 0")

    def lr_at(self, iteration: int) -> float:
        """exp((1 - t) log lr + t log lr_final), t = iteration / num_iterations clipped to [0, 1]"""
        if self.num_iterations is None:
            return float(self.lr)
        t = min(max(float(iteration) / float(self.num_iterations), 0.0), 1.0)
        return float(math.exp((1.0 - t) * math.log(self.lr) + t * math.log(self.lr_final)))


class AppearanceTable:
    """One transform per training view: transforms, grad, exp_avg and exp_avg_sq are (V,12) float32 on the device, steps the
    host-side Adam step count of every row.  Rows are 48 bytes, so every row is 16-byte aligned."""

    def __init__(self, num_views: int, device, config: Optional[AppearanceConfig] = None):
        self.config = AppearanceConfig() if config is None else config
        self.config.check()
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("exposure compensation runs on the GPU: the table must be on a cuda/hip device (there is no CPU path)")
        if num_views < 1:
            raise ValueError("num_views must be >= 1")
        self.num_views = int(num_views)
        self.transforms = torch.tensor(IDENTITY, dtype=torch.float32, device=device).repeat(self.num_views, 1).contiguous()
        self.grad = torch.zeros_like(self.transforms)
        self.exp_avg = torch.zeros_like(self.transforms)
        self.exp_avg_sq = torch.zeros_like(self.transforms)
        self.steps: List[int] = [0] * self.num_views

    @property
    def device(self):
        return self.transforms.device

    def _view(self, v: int) -> int:
        v = int(v)
        if not 0 <= v < self.num_views:
            raise IndexError(f"view {v} is not in [0, {self.num_views})")
        return v

    def row(self, v: int):
        """-> the (12,) transform of view v: a leaf that shares the table's memory and requires grad.  Its .grad IS row v of
        self.grad, and apply()'s backward writes (not adds) the gradient there (row.grad_out): one apply() per backward."""
        v = self._view(v)
        row = self.transforms[v].detach().requires_grad_(True)
        row.grad = row.grad_out = self.grad[v]
        return row

    def step(self, v: int, iteration: int):
        """One Adam step (gs_adam_step, as FusedAdam.step) on row v alone, with the gradient in row v of self.grad, the row's
        own step count and config.lr_at(iteration).  No other row, and no moment of another row, moves."""
        v = self._view(v)
        self.steps[v] += 1
        dev = self.transforms.device
        with torch.no_grad():
            _native.call("gs_adam_step", dev, _native.shared_ctx(dev), self.transforms[v].data_ptr(), self.grad[v].data_ptr(),
                         self.exp_avg[v].data_ptr(), self.exp_avg_sq[v].data_ptr(), TRANSFORM_FLOATS, self.config.lr_at(iteration),
                         float(self.config.betas[0]), float(self.config.betas[1]), float(self.config.eps), self.steps[v])

    def save(self, path: str, image_paths: Sequence[str]):
        """A .pt of the table and the image paths its rows belong to (row v is image_paths[v])"""
        image_paths = [str(p) for p in image_paths]
        if len(image_paths) != self.num_views:
            raise ValueError(f"{len(image_paths)} image paths for a table of {self.num_views} views")
        torch.save(dict(transforms=self.transforms.cpu(), exp_avg=self.exp_avg.cpu(), exp_avg_sq=self.exp_avg_sq.cpu(), steps=list(self.steps),
                        image_paths=image_paths), path)

    @classmethod
    def load(cls, path: str, device="cuda", config: Optional[AppearanceConfig] = None):
        """-> (table, image_paths) of a file save() wrote"""
        data = torch.load(path, map_location="cpu")
        transforms = data["transforms"]
        if transforms.dim() != 2 or transforms.shape[1] != TRANSFORM_FLOATS or transforms.dtype != torch.float32:
            raise ValueError(f"{path}: transforms must be (V,{TRANSFORM_FLOATS}) float32")
        table = cls(transforms.shape[0], device, config)
        table.transforms.copy_(transforms)
        table.exp_avg.copy_(data["exp_avg"])
        table.exp_avg_sq.copy_(data["exp_avg_sq"])
        table.steps = [int(s) for s in data["steps"]]
        return table, list(data["image_paths"])

    def by_image_path(self, image_paths: Sequence[str]) -> dict:
        """{image path: its (12,) transform}, views of the table"""
        return {str(p): self.transforms[v] for v, p in enumerate(image_paths)}
