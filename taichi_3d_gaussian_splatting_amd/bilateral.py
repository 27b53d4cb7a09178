"""Per-view bilateral grids (include/gs_bilateral.h, csrc/k_bilateral.hip): a small 3-D lattice of 3x4 affine colour
transforms per training image -- two axes over the image plane, one over the luminance of the rendered pixel -- sliced at every
pixel and applied in front of the loss, trained with the scene and kept smooth by a total-variation term.  "Bilateral Guided
Radiance Field Processing" (Wang et al., SIGGRAPH 2024); gsplat's use_bilateral_grid.  It contains appearance.py's affine
table (a constant grid is one transform) and also absorbs what varies across the picture: vignetting, local tone mapping.

  table = BilateralGridTable(len(train_dataset), device, BilateralGridConfig(num_iterations=30_000))
  corrected = slice(image_pred.permute(2, 0, 1), table.row(view))        # read where the rasteriser left it
  loss, _, _ = loss_function(corrected, image_gt, clamp_predicted=True)
  loss.backward()                                                          # the grid's gradient lands in table.grad
  tv(table.grids[view], weight=table.config.tv_weight, grad_grid=table.grad, value=table.tv_value)
  optimizer.step(); position_optimizer.step(); table.step(view, iteration)

A grid is a contiguous float32 (Gy, Gx, L, 12) tensor: vertex (iy, ix, l) holds a row-major M = [A | b].

There is no fallback path: every call goes through _native.call(), and a CPU tensor is refused.
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from . import _native
from ._native import GsLossImage
from .appearance import IDENTITY, check_image, check_like

VERTEX_FLOATS = 12                              # GS_BILATERAL_VERTEX_FLOATS
MIN_GRID, MAX_XY, MAX_L = 2, 64, 8              # GS_BILATERAL_MIN_GRID, _MAX_XY, _MAX_L
THREADS, GATHER_THREADS, TV_THREADS = 256, 256, 1024        # GS_BILATERAL_THREADS, _GATHER_THREADS, _TV_THREADS
TARGET_BLOCKS = 1024                            # GS_BILATERAL_TARGET_BLOCKS
MAX_PIXELS = 2 ** 31 - 2048                     # GS_BILATERAL_MAX_PIXELS
LUMINANCE = (0.299, 0.587, 0.114)

_VP, _I32, _F32, _IMG = C.c_void_p, C.c_int32, C.c_float, C.POINTER(GsLossImage)
ARGTYPES = {
    # (ctx, image, grid, Gx, Gy, L, H, W, corrected, stream)
    "gs_bilateral_slice": [_VP, _IMG, _VP, _I32, _I32, _I32, _I32, _I32, _IMG, _VP],
    # (ctx, image, grad_corrected, grid, Gx, Gy, L, H, W, grad_image, grad_grid, stream)
    "gs_bilateral_slice_backward": [_VP, _IMG, _IMG, _VP, _I32, _I32, _I32, _I32, _I32, _IMG, _VP, _VP],
    # (ctx, grid, Gx, Gy, L, weight, grad_grid, value, stream)
    "gs_bilateral_tv": [_VP, _VP, _I32, _I32, _I32, _F32, _VP, _VP, _VP],
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
def check_shape(grid_x: int, grid_y: int, grid_l: int):
    if not (MIN_GRID <= int(grid_x) <= MAX_XY and MIN_GRID <= int(grid_y) <= MAX_XY):
        raise ValueError(f"grid_x and grid_y must be in [{MIN_GRID}, {MAX_XY}], got {grid_x} and {grid_y}")
    if not MIN_GRID <= int(grid_l) <= MAX_L:
        raise ValueError(f"grid_l must be in [{MIN_GRID}, {MAX_L}], got {grid_l}")


def check_grid(grid, device, what="grid"):
    """Raise unless `grid` is a contiguous, 16-byte aligned float32 (Gy,Gx,L,12) tensor within the limits on `device`; device
    None: on a GPU"""
    if not isinstance(grid, torch.Tensor):
        raise TypeError(f"{what} must be a tensor")
    if grid.dim() != 4 or grid.shape[3] != VERTEX_FLOATS:
        raise ValueError(f"{what} must be (Gy,Gx,L,{VERTEX_FLOATS}), got {tuple(grid.shape)}")
    check_shape(grid.shape[1], grid.shape[0], grid.shape[2])
    if grid.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {grid.dtype}")
    if device is None:
        if not grid.is_cuda:
            raise ValueError(f"bilateral grids run on the GPU: {what} must be on a cuda/hip device (there is no CPU path)")
    elif grid.device != device:
        raise ValueError(f"{what} is on {grid.device}, expected {device}")
    if not grid.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    if grid.device.type == "cuda" and grid.data_ptr() % 16 != 0:
        raise ValueError(f"{what} must be 16-byte aligned")


def _dims(grid):
    return int(grid.shape[1]), int(grid.shape[0]), int(grid.shape[2])       # Gx, Gy, L


# ---- the three calls --------------------------------------------------------------------------------------------------------
def slice_forward(image, grid, out=None):
    """gs_bilateral_slice, no autograd: -> the corrected image, in image's strides when they are dense (preserve_format).
    out: where to write instead -- `image` itself for in place, or any float32 tensor of its shape that does not overlap it."""
    check_image(image)
    check_grid(grid, image.device)
    if out is None:
        out = torch.empty_like(image, memory_format=torch.preserve_format)
    else:
        check_like(out, image, "out")
    _bind()
    H, W = int(image.shape[1]), int(image.shape[2])
    _native.call("gs_bilateral_slice", image.device, _native.shared_ctx(image.device), GsLossImage.of(image), grid.data_ptr(), *_dims(grid), H, W,
                 GsLossImage.of(out))
    return out


def slice_backward(image, grad_corrected, grid, grad_image=True, grad_grid=True):
    """gs_bilateral_slice_backward, no autograd: -> (grad_image or None, grad_grid or None).  Either flag may be a tensor to
    write into: grad_image a float32 tensor of the image's shape (any strides), grad_grid a contiguous one of the grid's shape
    -- every element is written, not added.  A pixel whose three upstream values are exactly 0 is left out of every sum and
    gets a gradient of exactly 0, whatever the image holds there."""
    check_image(image)
    check_like(grad_corrected, image, "grad_corrected")
    check_grid(grid, image.device)
    if grad_image is True:
        grad_image = torch.empty_like(image, memory_format=torch.preserve_format)
    elif grad_image is False or grad_image is None:
        grad_image = None
    else:
        check_like(grad_image, image, "grad_image")
    if grad_grid is True:
        grad_grid = torch.empty_like(grid)
    elif grad_grid is False or grad_grid is None:
        grad_grid = None
    else:
        check_grid(grad_grid, image.device, "grad_grid")
        if grad_grid.shape != grid.shape:
            raise ValueError(f"grad_grid must have the grid's shape {tuple(grid.shape)}, got {tuple(grad_grid.shape)}")
    if grad_image is None and grad_grid is None:
        raise ValueError("slice_backward: nothing to compute (grad_image and grad_grid are both off)")
    _bind()
    H, W = int(image.shape[1]), int(image.shape[2])
    _native.call("gs_bilateral_slice_backward", image.device, _native.shared_ctx(image.device), GsLossImage.of(image), GsLossImage.of(grad_corrected),
                 grid.data_ptr(), *_dims(grid), H, W, None if grad_image is None else GsLossImage.of(grad_image),
                 None if grad_grid is None else grad_grid.data_ptr())
    return grad_image, grad_grid


def tv(grid, weight: float = 0.0, grad_grid=None, value=None):
    """gs_bilateral_tv: -> the total variation of the grid (gsplat's total_variation_loss of one grid) as a (1,) float32 tensor
    on the device (`value`, when given, is written and returned).  With grad_grid, a contiguous float32 tensor of the grid's
    shape, weight * d tv / d grid is ADDED into it in the same launch."""
    check_grid(grid, None)
    if not math.isfinite(float(weight)):
        raise ValueError("weight must be finite")
    if grad_grid is not None:
        check_grid(grad_grid, grid.device, "grad_grid")
        if grad_grid.shape != grid.shape:
            raise ValueError(f"grad_grid must have the grid's shape {tuple(grid.shape)}, got {tuple(grad_grid.shape)}")
    if value is None:
        value = torch.empty(1, dtype=torch.float32, device=grid.device)
    elif not (isinstance(value, torch.Tensor) and value.dtype == torch.float32 and value.numel() == 1 and value.device == grid.device):
        raise ValueError("value must be one float32 on the grid's device")
    _bind()
    _native.call("gs_bilateral_tv", grid.device, _native.shared_ctx(grid.device), grid.data_ptr(), *_dims(grid), float(weight),
                 None if grad_grid is None else grad_grid.data_ptr(), value.data_ptr())
    return value


class _Slice(torch.autograd.Function):
    """slice() as an autograd node.  A grid that names a `grad_out` tensor (BilateralGridTable.row sets it, and sets the row's
    .grad to the same memory) has its gradient WRITTEN there by the backward's own launches, and autograd is handed nothing
    for it.  Such a row feeds one slice() per backward.  Any other grid gets its gradient the usual way."""

    @staticmethod
    def forward(ctx, image, grid, grad_out):
        corrected = slice_forward(image.detach(), grid.detach())
        ctx.save_for_backward(image, grid)
        ctx.grad_out = grad_out
        return corrected

    @staticmethod
    def backward(ctx, grad_corrected):
        image, grid = ctx.saved_tensors
        want_image, want_grid = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_image or want_grid):
            return None, None, None
        if grad_corrected.dtype != torch.float32:
            grad_corrected = grad_corrected.to(torch.float32)
        direct = want_grid and ctx.grad_out is not None
        grad_image, grad_grid = slice_backward(image.detach(), grad_corrected, grid.detach(), grad_image=want_image,
                                               grad_grid=ctx.grad_out if direct else want_grid)
        return grad_image, (None if direct else grad_grid), None


def slice(image, grid):
    """-> the image corrected by the grid's transform at every pixel's (x, y, luminance): a float32 (3,H,W) GPU image of any
    strides and a (Gy,Gx,L,12) grid; differentiable in both, through the luminance guide too.  The result has image's strides
    when they are dense (the rasteriser's (H,W,3) output under permute(2,0,1) stays interleaved), so
    LossFunction(..., clamp_predicted=True) reads it in place."""
    check_image(image)
    check_grid(grid, image.device)
    grad_out = getattr(grid, "grad_out", None)
    if grad_out is not None:
        check_grid(grad_out, image.device, "grad_out")
    return _Slice.apply(image, grid, grad_out)


# ---- the table of a training set -------------------------------------------------------------------------------------------
@dataclass
class BilateralGridConfig:
    """grid_x x grid_y vertices over the image plane, grid_l along the luminance.  tv_weight multiplies the total variation of
    the step's grid (gsplat's bilateral_grid tv loss weight).  lr falls exponentially from lr at iteration 0 to lr_final at
    num_iterations (AppearanceConfig's schedule).  num_iterations None: the trainer fills in its own.  eps is FusedAdam's."""
    grid_x: int = 16
    grid_y: int = 16
    grid_l: int = 8
    tv_weight: float = 10.0
    lr: float = 2e-3
    lr_final: float = 2e-5
    num_iterations: Optional[int] = None
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8

    def check(self):
        check_shape(self.grid_x, self.grid_y, self.grid_l)
        if not (math.isfinite(self.tv_weight) and self.tv_weight >= 0.0):
            raise ValueError("tv_weight must be finite and >= 0")
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


class BilateralGridTable:
    """One grid per training view: grids, exp_avg and exp_avg_sq are (V,Gy,Gx,L,12) float32 on the device, steps the host-side
    Adam step count of every view.  There is ONE gradient buffer, of one grid (grad): a step touches one view.  tv_value is
    the (1,) device scalar the trainer's tv() call writes.  A grid is a multiple of 48 bytes, so every grid is 16-byte aligned."""

    def __init__(self, num_views: int, device, config: Optional[BilateralGridConfig] = None):
        self.config = BilateralGridConfig() if config is None else config
        self.config.check()
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("bilateral grids run on the GPU: the table must be on a cuda/hip device (there is no CPU path)")
        if num_views < 1:
            raise ValueError("num_views must be >= 1")
        self.num_views = int(num_views)
        c = self.config
        identity = torch.tensor(IDENTITY, dtype=torch.float32, device=device)
        self.grids = identity.repeat(self.num_views, c.grid_y, c.grid_x, c.grid_l, 1).contiguous()
        self.grad = torch.zeros_like(self.grids[0])
        self.exp_avg = torch.zeros_like(self.grids)
        self.exp_avg_sq = torch.zeros_like(self.grids)
        self.tv_value = torch.zeros(1, dtype=torch.float32, device=device)
        self.steps: List[int] = [0] * self.num_views

    @property
    def device(self):
        return self.grids.device

    def _view(self, v: int) -> int:
        v = int(v)
        if not 0 <= v < self.num_views:
            raise IndexError(f"view {v} is not in [0, {self.num_views})")
        return v

    def row(self, v: int):
        """-> the (Gy,Gx,L,12) grid of view v: a leaf that shares the table's memory and requires grad.  Its .grad IS self.grad,
        and slice()'s backward writes (not adds) the gradient there (row.grad_out): one slice() per backward."""
        v = self._view(v)
        row = self.grids[v].detach().requires_grad_(True)
        row.grad = row.grad_out = self.grad
        return row

    def step(self, v: int, iteration: int):
        """One Adam step (gs_adam_step, as FusedAdam.step) on the grid of view v alone, with the gradient in self.grad, the
        view's own step count and config.lr_at(iteration).  No other grid, and no moment of another grid, moves."""
        v = self._view(v)
        self.steps[v] += 1
        dev = self.grids.device
        with torch.no_grad():
            _native.call("gs_adam_step", dev, _native.shared_ctx(dev), self.grids[v].data_ptr(), self.grad.data_ptr(),
                         self.exp_avg[v].data_ptr(), self.exp_avg_sq[v].data_ptr(), self.grad.numel(), self.config.lr_at(iteration),
                         float(self.config.betas[0]), float(self.config.betas[1]), float(self.config.eps), self.steps[v])

    def save(self, path: str, image_paths: Sequence[str]):
        """A .pt of the table and the image paths its grids belong to (grid v is image_paths[v])"""
        image_paths = [str(p) for p in image_paths]
        if len(image_paths) != self.num_views:
            raise ValueError(f"{len(image_paths)} image paths for a table of {self.num_views} views")
        torch.save(dict(grids=self.grids.cpu(), exp_avg=self.exp_avg.cpu(), exp_avg_sq=self.exp_avg_sq.cpu(), steps=list(self.steps),
                        image_paths=image_paths), path)

    @classmethod
    def load(cls, path: str, device="cuda", config: Optional[BilateralGridConfig] = None):
        """-> (table, image_paths) of a file save() wrote; the grid shape is the file's"""
        import dataclasses
        data = torch.load(path, map_location="cpu")
        grids = data["grids"]
        if grids.dim() != 5 or grids.shape[4] != VERTEX_FLOATS or grids.dtype != torch.float32:
            raise ValueError(f"{path}: grids must be (V,Gy,Gx,L,{VERTEX_FLOATS}) float32")
        config = dataclasses.replace(BilateralGridConfig() if config is None else config, grid_y=int(grids.shape[1]), grid_x=int(grids.shape[2]),
                                     grid_l=int(grids.shape[3]))
        table = cls(grids.shape[0], device, config)
        table.grids.copy_(grids)
        table.exp_avg.copy_(data["exp_avg"])
        table.exp_avg_sq.copy_(data["exp_avg_sq"])
        table.steps = [int(s) for s in data["steps"]]
        return table, list(data["image_paths"])

    def by_image_path(self, image_paths: Sequence[str]) -> dict:
        """{image path: its (Gy,Gx,L,12) grid}, views of the table"""
        return {str(p): self.grids[v] for v, p in enumerate(image_paths)}
