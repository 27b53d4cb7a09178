"""Per-Gaussian feature channels rendered over a frame of the rasteriser (include/gs_channels.h, csrc/k_channels.hip).

A frame made by GaussianPointCloudRasterisation.forward holds the sorted pairs, the projected records and the tile ranges;
render_channels blends any C values per Gaussian over it with the weights the colour was blended with, without binning or
sorting again.  The result is differentiable with respect to the values only: geometry is frozen (the regime of feature
distillation onto a trained scene, and all a visualisation needs).  There is no fallback path: both directions are library
calls through _native.call().
"""
import ctypes as C

import torch

from . import _native

GS_CHANNELS_MAX = 64

_VP, _I32 = C.c_void_p, C.c_int32
# (ctx, frame, values | grad_out, n_channels, pixel_offset_of_last_effective_point, out | grad_values, stream)
ARGTYPES = {"gs_channels_forward": [_VP, _VP, _VP, _I32, _VP, _VP, _VP],
            "gs_channels_backward": [_VP, _VP, _VP, _I32, _VP, _VP, _VP]}
_bound = False


def _bind():
    """argtypes of the two entry points, set once on the loaded library (they are not part of _native.SYMBOLS)"""
    global _bound
    if not _bound:
        L = _native.lib()
        for name, argtypes in ARGTYPES.items():
            if not hasattr(L, name):
                raise _native.NativeLibraryError(f"{_native.LIB_PATH} does not export {name}")
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
        _bound = True


def _ticket(frame):
    """The frame's ticket as the library takes it; a released frame's last ticket, which the library refuses by itself."""
    return frame._h if frame._h is not None else getattr(frame, "_stale", None)


class _ChannelsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, frame, last):
        H, W = last.shape
        C_ = values.shape[1]
        out = torch.empty(H, W, C_, dtype=torch.float32, device=values.device)
        _native.call("gs_channels_forward", values.device, frame._context.handle, _ticket(frame), _native.ptr(values), C_,
                     _native.ptr(last), _native.ptr(out))
        # the node owns the _Frame (and through it the context) and the frame's `last` until autograd drops it
        ctx.frame, ctx.last, ctx.shape = frame, last, tuple(values.shape)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        frame, last = ctx.frame, ctx.last
        N, C_ = ctx.shape
        if grad_out.dtype != torch.float32 or tuple(grad_out.shape) != (*last.shape, C_):
            raise ValueError("grad of the channel image must be float32 (H,W,C)")
        grad_out = grad_out.contiguous()
        grad_values = torch.empty(N, C_, dtype=torch.float32, device=grad_out.device)
        _native.call("gs_channels_backward", grad_out.device, frame._context.handle, _ticket(frame), _native.ptr(grad_out), C_,
                     _native.ptr(last), _native.ptr(grad_values))
        return grad_values, None, None


def render_channels(values: torch.Tensor, frame) -> torch.Tensor:
    """values (N,C) float32 on the frame's device, 1 <= C <= GS_CHANNELS_MAX, one row per point-cloud row -> (H,W,C):
    out[y,x,:] = sum_i alpha_i T_i values[id_i,:] over the pixel's contributors in the frame (no division by the accumulated
    alpha).  Differentiable in `values` when the frame was kept (forward(..., keep_frame=True) or a forward whose inputs
    require grad); rows of points outside the camera are never read and get a zero gradient."""
    _bind()
    if frame is None:
        raise ValueError("render_channels needs a frame: run forward() first")
    last = getattr(frame, "last", None)
    if last is None:
        raise ValueError("render_channels needs a frame of a full forward: an rgb_only frame has no pixel_offset_of_last_effective_point")
    if not isinstance(values, torch.Tensor) or values.dtype != torch.float32:
        raise ValueError(f"values must be a float32 tensor, got {getattr(values, 'dtype', type(values))}")
    if values.dim() != 2 or values.shape[0] != frame.n_points:
        raise ValueError(f"values must have shape (N, C) with N = {frame.n_points}, got {tuple(values.shape)}")
    if not 1 <= values.shape[1] <= GS_CHANNELS_MAX:
        raise ValueError(f"values must have 1..{GS_CHANNELS_MAX} channels, got {values.shape[1]}")
    if values.device != last.device:
        raise ValueError(f"values is on {values.device}, the frame on {last.device}")
    if values.requires_grad and torch.is_grad_enabled() and not frame._owned:
        raise ValueError("values requires grad but the frame was not kept: run forward(..., keep_frame=True)")
    if values.shape[0] == 0:
        return torch.zeros(*last.shape, values.shape[1], dtype=torch.float32, device=values.device)
    return _ChannelsFunction.apply(values.contiguous(), frame, last)
