"""A background behind the splats (include/gs_background.h, csrc/k_background.hip): a solid colour, a random colour per step
or a learnable low-order sky -- real spherical harmonics of the view direction, up to three bands, 48 floats -- composited under
the rendered image with the rasteriser's accumulated alpha.

  model = BackgroundModel("sky", device, BackgroundConfig(bands=2, num_iterations=30_000))
  image, depth, count, alpha = rasterisation(rasterisation_input, return_accumulated_alpha=True)
  coef = model.coef_for_step()
  image = composite(image.permute(2, 0, 1), alpha, coef, model.bands, q_pointcloud_camera, camera_intrinsics)
  loss.backward()                                  # alpha's gradient reaches the scene; coef.grad lands in model.grad
  optimizer.step(); position_optimizer.step(); model.step(iteration)

  target = composite_straight(rgba, coef, model.bands, q, intrinsics)      # an RGBA ground truth over the same background

A background is 48 floats, coef[16 i + k] for channel i; `bands` selects (bands + 1)^2 of them per channel.  The colour of a
pixel is coef[16 i] + sum_{k >= 1} coef[16 i + k] Y_k(d), d the pixel centre's ray in the point-cloud frame: the constant term
is taken without Y_0, so (1, 0, ..., 0) per channel is exactly white.  The gradient of the sky to the camera pose, through d,
is not taken.

There is no fallback path: every call goes through _native.call(), and a CPU tensor is refused.
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from . import _native
from ._native import GsLossImage

PIXELS_PER_BLOCK = 1024                         # GS_BACKGROUND_PIXELS_PER_BLOCK
FINISH_THREADS = 256                            # GS_BACKGROUND_FINISH_THREADS
FINISH_BLOCKS = 48                              # GS_BACKGROUND_FINISH_BLOCKS
COEF_FLOATS = 48                                # GS_BACKGROUND_COEF_FLOATS
MAX_BANDS = 3                                   # GS_BACKGROUND_MAX_BANDS
MAX_PIXELS = 2 ** 31 - 2048                     # GS_BACKGROUND_MAX_PIXELS
STRAIGHT, COLOURS_ONLY = 1, 2                   # GS_BACKGROUND_STRAIGHT, GS_BACKGROUND_COLOURS_ONLY
KINDS = ("colour", "random", "sky")

_VP, _I32, _IMG = C.c_void_p, C.c_int32, C.POINTER(GsLossImage)
ARGTYPES = {
    # (ctx, image, alpha, coef, bands, q, intrinsics, H, W, flags, out, stream)
    "gs_background_composite": [_VP, _IMG, _VP, _VP, _I32, _VP, _VP, _I32, _I32, _I32, _IMG, _VP],
    # (ctx, grad_out, alpha, coef, bands, q, intrinsics, H, W, grad_alpha, grad_coef, stream)
    "gs_background_backward": [_VP, _IMG, _VP, _VP, _I32, _VP, _VP, _I32, _I32, _VP, _VP, _VP],
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
        raise ValueError(f"backgrounds are composited on the GPU: {what} must be on a cuda/hip device (there is no CPU path)")


def _check_vector(t, what, shape, device):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a tensor")
    if t.numel() != math.prod(shape) or tuple(t.shape) not in (tuple(shape), (1,) + tuple(shape), (math.prod(shape),)):
        raise ValueError(f"{what} must be {tuple(shape)}, got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {t.dtype}")
    if t.device != device:
        raise ValueError(f"{what} is on {t.device}, the image on {device}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")


def check_plane(alpha, shape_hw, device, what="alpha"):
    """Raise unless `alpha` is a contiguous float32 (H,W) tensor on `device`"""
    if not isinstance(alpha, torch.Tensor):
        raise TypeError(f"{what} must be a tensor")
    if tuple(alpha.shape) != tuple(shape_hw):
        raise ValueError(f"{what} must be {tuple(shape_hw)}, got {tuple(alpha.shape)}")
    if alpha.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {alpha.dtype}")
    if alpha.device != device:
        raise ValueError(f"{what} is on {alpha.device}, the image on {device}")
    if not alpha.is_contiguous():
        raise ValueError(f"{what} must be contiguous")


def check_background(coef, bands, q, intrinsics, device):
    """Raise unless coef is a contiguous float32 (48,) tensor on `device`, bands is 0..3 and, for bands > 0, q is (4,) or (1,4)
    and intrinsics (3,3), float32, contiguous, on `device`"""
    _check_vector(coef, "coef", (COEF_FLOATS,), device)
    if isinstance(bands, bool) or not isinstance(bands, int) or not 0 <= bands <= MAX_BANDS:
        raise ValueError(f"bands must be an integer in 0..{MAX_BANDS}, got {bands!r}")
    if bands > 0:
        if q is None or intrinsics is None:
            raise ValueError("bands > 0 needs q (the camera's q_pointcloud_camera) and intrinsics")
        _check_vector(q, "q", (4,), device)
        _check_vector(intrinsics, "intrinsics", (3, 3), device)


def _camera(bands, q, intrinsics):
    """the two pointers of the view direction; NULL for a solid colour, which reads neither"""
    if bands == 0:
        return None, None
    return q.data_ptr(), intrinsics.data_ptr()


# ---- the calls ----------------------------------------------------------------------------------------------------------
def composite_forward(image, alpha, coef, bands, q=None, intrinsics=None, out=None, straight=False):
    """gs_background_composite, no autograd: -> image + (1 - alpha) c, or image * alpha + (1 - alpha) c with straight=True, in
    image's strides when they are dense (preserve_format).  out: where to write instead -- `image` itself for in place, or any
    float32 tensor of its shape that does not overlap it."""
    check_image(image)
    check_plane(alpha, image.shape[1:], image.device)
    check_background(coef, bands, q, intrinsics, image.device)
    if out is None:
        out = torch.empty_like(image, memory_format=torch.preserve_format)
    else:
        check_image(out, "out")
        if out.shape != image.shape or out.device != image.device:
            raise ValueError(f"out must have the image's shape {tuple(image.shape)} and device")
    _bind()
    H, W = int(image.shape[1]), int(image.shape[2])
    qp, kp = _camera(bands, q, intrinsics)
    _native.call("gs_background_composite", image.device, _native.shared_ctx(image.device), GsLossImage.of(image), alpha.data_ptr(),
                 coef.data_ptr(), bands, qp, kp, H, W, STRAIGHT if straight else 0, GsLossImage.of(out))
    return out


def composite_backward(grad_out, alpha, coef, bands, q=None, intrinsics=None, grad_alpha=True, grad_coef=True):
    """gs_background_backward, no autograd: -> (grad_alpha (H,W) or None, grad_coef (48,) or None).  grad_coef may be a
    contiguous (48,) tensor to write into -- every element is written, not added.  A pixel whose three upstream values are
    exactly 0 is left out of every sum and gets a gradient of exactly 0, whatever alpha holds there."""
    check_image(grad_out, "grad_out")
    check_plane(alpha, grad_out.shape[1:], grad_out.device)
    check_background(coef, bands, q, intrinsics, grad_out.device)
    if grad_alpha is True:
        grad_alpha = torch.empty_like(alpha)
    elif grad_alpha is False or grad_alpha is None:
        grad_alpha = None
    else:
        check_plane(grad_alpha, grad_out.shape[1:], grad_out.device, "grad_alpha")
    if grad_coef is True:
        grad_coef = torch.empty(COEF_FLOATS, dtype=torch.float32, device=grad_out.device)
    elif grad_coef is False or grad_coef is None:
        grad_coef = None
    else:
        _check_vector(grad_coef, "grad_coef", (COEF_FLOATS,), grad_out.device)
    if grad_alpha is None and grad_coef is None:
        raise ValueError("composite_backward: nothing to compute (grad_alpha and grad_coef are both off)")
    _bind()
    H, W = int(grad_out.shape[1]), int(grad_out.shape[2])
    qp, kp = _camera(bands, q, intrinsics)
    _native.call("gs_background_backward", grad_out.device, _native.shared_ctx(grad_out.device), GsLossImage.of(grad_out), alpha.data_ptr(),
                 coef.data_ptr(), bands, qp, kp, H, W, None if grad_alpha is None else grad_alpha.data_ptr(),
                 None if grad_coef is None else grad_coef.data_ptr())
    return grad_alpha, grad_coef


class _Composite(torch.autograd.Function):
    """composite() as one autograd node.  The image's gradient is the upstream gradient itself.  A coef that names a
    `grad_out` tensor (BackgroundModel.coef_for_step sets it, and sets .grad to the same memory) has its gradient WRITTEN
    there by the backward's own launch, and autograd is handed nothing for it; any other coef gets its gradient the usual way."""

    @staticmethod
    def forward(ctx, image, alpha, coef, bands, q, intrinsics, grad_out):
        out = composite_forward(image.detach(), alpha.detach(), coef.detach(), bands, q, intrinsics)
        ctx.save_for_backward(alpha, coef, q, intrinsics)
        ctx.bands, ctx.grad_out = bands, grad_out
        return out

    @staticmethod
    def backward(ctx, grad):
        alpha, coef, q, intrinsics = ctx.saved_tensors
        want_image, want_alpha, want_coef = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        grad_alpha = grad_coef = None
        if grad.dtype != torch.float32:
            grad = grad.to(torch.float32)
        direct = want_coef and ctx.grad_out is not None
        if want_alpha or want_coef:
            grad_alpha, grad_coef = composite_backward(grad, alpha.detach(), coef.detach(), ctx.bands, q, intrinsics, grad_alpha=want_alpha,
                                                       grad_coef=ctx.grad_out if direct else want_coef)
        return (grad if want_image else None), grad_alpha, (None if direct else grad_coef), None, None, None, None


def composite(image, alpha, coef, bands, q=None, intrinsics=None):
    """-> image + (1 - alpha) * c of a float32 (3,H,W) GPU image of any strides (the rasteriser's premultiplied output under
    permute(2,0,1) is read where it lies), its contiguous (H,W) accumulated alpha and a (48,) background; differentiable in
    image (identity), alpha and coef.  q: the camera's q_pointcloud_camera, (4,) or (1,4); intrinsics: its (3,3) matrix; both
    unused, and may be None, with bands == 0.  No gradient is taken to q or the intrinsics."""
    check_image(image)
    check_plane(alpha, image.shape[1:], image.device)
    check_background(coef, bands, q, intrinsics, image.device)
    grad_out = getattr(coef, "grad_out", None)
    if grad_out is not None:
        _check_vector(grad_out, "coef.grad_out", (COEF_FLOATS,), image.device)
    if bands > 0:
        q, intrinsics = q.detach(), intrinsics.detach()
    else:
        q = intrinsics = None
    return _Composite.apply(image, alpha, coef, bands, q, intrinsics, grad_out)


def composite_straight(rgba, coef, bands, q=None, intrinsics=None, out=None):
    """-> (3,H,W): a decoded (4,H,W) float32 RGBA picture (straight alpha, the last plane contiguous) over the background:
    rgb * a + (1 - a) * c.  No gradient."""
    if not isinstance(rgba, torch.Tensor):
        raise TypeError("rgba must be a tensor")
    if rgba.dim() != 3 or rgba.shape[0] != 4:
        raise ValueError(f"rgba must be (4,H,W), got {tuple(rgba.shape)}")
    with torch.no_grad():
        return composite_forward(rgba[:3].detach(), rgba[3].detach(), coef.detach(), bands, q, intrinsics, out=out, straight=True)


def colours(coef, bands, q, intrinsics, H, W):
    """-> (3,H,W) float32, contiguous: the background's colour at every pixel of an H x W camera"""
    if not isinstance(coef, torch.Tensor):
        raise TypeError("coef must be a tensor")
    if not coef.is_cuda:
        raise ValueError("backgrounds are composited on the GPU: coef must be on a cuda/hip device (there is no CPU path)")
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W > MAX_PIXELS:
        raise ValueError(f"H and W must be >= 1 and H * W <= {MAX_PIXELS}")
    check_background(coef, bands, q, intrinsics, coef.device)
    out = torch.empty(3, H, W, dtype=torch.float32, device=coef.device)
    _bind()
    qp, kp = _camera(bands, q, intrinsics)
    _native.call("gs_background_composite", coef.device, _native.shared_ctx(coef.device), None, None, coef.detach().data_ptr(), bands, qp, kp,
                 H, W, COLOURS_ONLY, GsLossImage.of(out))
    return out


# ---- the background of a training run ---------------------------------------------------------------------------------
@dataclass
class BackgroundConfig:
    """colour: the solid colour ("colour"), the validation colour ("random") or the sky's initial constant term ("sky").
    bands: of the sky.  lr falls exponentially from lr at iteration 0 to lr_final at num_iterations (None: the trainer fills in
    its own).  seed: of the random colours.  betas and eps are FusedAdam's."""
    colour: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    bands: int = 2
    lr: float = 0.01
    lr_final: float = 0.001
    num_iterations: Optional[int] = None
    seed: int = 0
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8

    def check(self):
        if len(tuple(self.colour)) != 3 or not all(math.isfinite(float(c)) for c in self.colour):
            raise ValueError("colour must be three finite numbers")
        if isinstance(self.bands, bool) or not isinstance(self.bands, int) or not 0 <= self.bands <= MAX_BANDS:
            raise ValueError(f"bands must be an integer in 0..{MAX_BANDS}")
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


def colour_coefficients(colour: Sequence[float], device) -> torch.Tensor:
    """-> the (48,) background of a solid colour: coef[16 i] = colour[i], every other entry 0"""
    coef = torch.zeros(3, 16, dtype=torch.float32)
    coef[:, 0] = torch.tensor([float(c) for c in colour], dtype=torch.float32)
    return coef.reshape(COEF_FLOATS).to(device)


class BackgroundModel:
    """The background of a run: coef, grad, exp_avg and exp_avg_sq are (48,) float32 on the device.
      "colour": config.colour, fixed; bands 0.
      "random": a fresh uniform colour per coef_for_step(), drawn on the device by a seeded generator, no host read; bands 0.
                `coef` keeps config.colour: what validation and a later render composite over.
      "sky":    config.bands bands, learnable; starts as the solid config.colour and is stepped by step()."""

    def __init__(self, kind: str, device, config: Optional[BackgroundConfig] = None):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
        self.config = BackgroundConfig() if config is None else config
        self.config.check()
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("backgrounds are composited on the GPU: the model must be on a cuda/hip device (there is no CPU path)")
        self.kind = kind
        self.bands = int(self.config.bands) if kind == "sky" else 0
        self.coef = colour_coefficients(self.config.colour, device)
        self.grad = torch.zeros_like(self.coef)
        self.exp_avg = torch.zeros_like(self.coef)
        self.exp_avg_sq = torch.zeros_like(self.coef)
        self.steps = 0
        self._generator = torch.Generator(device=device).manual_seed(int(self.config.seed)) if kind == "random" else None
        self._drawn = torch.zeros_like(self.coef) if kind == "random" else None

    @property
    def device(self):
        return self.coef.device

    @property
    def learnable(self) -> bool:
        return self.kind == "sky"

    def coef_for_step(self):
        """-> the (48,) background of a training step.  "sky": a leaf that shares the model's memory and requires grad; its
        .grad IS self.grad, and composite()'s backward writes (not adds) the gradient there: one composite() per backward.
        "random": a colour drawn now, on the device.  "colour": the stored coefficients."""
        if self.kind == "sky":
            coef = self.coef.detach().requires_grad_(True)
            coef.grad = coef.grad_out = self.grad
            return coef
        if self.kind == "random":
            self._drawn.view(3, 16)[:, 0] = torch.rand(3, dtype=torch.float32, device=self.device, generator=self._generator)
            return self._drawn
        return self.coef

    def step(self, iteration: int):
        """One Adam step (gs_adam_step, as FusedAdam.step) on the coefficients with the gradient in self.grad and
        config.lr_at(iteration).  The entries beyond the model's bands have a gradient of exactly 0 and stay where they are.
        Nothing happens for a background that is not learnable."""
        if not self.learnable:
            return
        self.steps += 1
        dev = self.coef.device
        with torch.no_grad():
            _native.call("gs_adam_step", dev, _native.shared_ctx(dev), self.coef.data_ptr(), self.grad.data_ptr(), self.exp_avg.data_ptr(),
                         self.exp_avg_sq.data_ptr(), COEF_FLOATS, self.config.lr_at(iteration), float(self.config.betas[0]),
                         float(self.config.betas[1]), float(self.config.eps), self.steps)

    def save(self, path: str):
        """A .pt of the kind, the bands, the coefficients and the optimiser's state"""
        torch.save(dict(kind=self.kind, bands=self.bands, coef=self.coef.cpu(), exp_avg=self.exp_avg.cpu(), exp_avg_sq=self.exp_avg_sq.cpu(),
                        steps=int(self.steps), colour=[float(c) for c in self.config.colour]), path)

    @classmethod
    def from_spec(cls, spec: str, device="cuda"):
        """-> the model a command line names: "black", "white", "R,G,B" (a solid colour) or the path of a file save() wrote"""
        named = {"black": (0.0, 0.0, 0.0), "white": (1.0, 1.0, 1.0)}
        spec = str(spec)
        if spec in named:
            return cls("colour", device, BackgroundConfig(colour=named[spec]))
        parts = spec.split(",")
        if len(parts) == 3:
            try:
                return cls("colour", device, BackgroundConfig(colour=tuple(float(p) for p in parts)))
            except ValueError:
                pass
        return cls.load(spec, device)

    @classmethod
    def load(cls, path: str, device="cuda", config: Optional[BackgroundConfig] = None):
        """-> the model of a file save() wrote"""
        data = torch.load(path, map_location="cpu")
        coef = data["coef"]
        if tuple(coef.shape) != (COEF_FLOATS,) or coef.dtype != torch.float32:
            raise ValueError(f"{path}: coef must be ({COEF_FLOATS},) float32")
        bands = int(data["bands"])
        if config is None:
            config = BackgroundConfig(colour=tuple(data["colour"]), bands=bands if data["kind"] == "sky" else BackgroundConfig.bands)
        model = cls(data["kind"], device, config)
        model.bands = bands
        model.coef.copy_(coef)
        model.exp_avg.copy_(data["exp_avg"])
        model.exp_avg_sq.copy_(data["exp_avg_sq"])
        model.steps = int(data["steps"])
        return model
