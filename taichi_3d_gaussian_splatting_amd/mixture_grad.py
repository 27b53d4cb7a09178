"""Gradients of the scene-as-mixture evaluations on the GPU (include/gs_mixture_grad.h, csrc/k_mixture_grad.hip).

log_density_backward() / fourier_backward() are the two library calls with their outputs allocated: from the upstream gradient of
mixture.log_density's (P,) result, or of the (P,2) real view of mixture.fourier's, to the gradients of point_cloud (N,3), of
point_cloud_features (N,56: columns 0..7 -- q, log s, opacity logit -- filled, the SH columns zero) and, for the density, of x
(P,3).  LogDensity / Fourier are the autograd Functions mixture.log_density / mixture.fourier go through when a gradient is
asked for; both are once-differentiable.  k and centre get no gradient.

A query whose upstream gradient is exactly zero, whose coordinates are not finite or (density) whose value is not finite
contributes nothing, so a masked loss out[valid].sum() does not turn a NaN or -inf output into NaN gradients.  Everything is
deterministic (no atomics, fixed summation order) and queued on the current stream; there is no fallback path.
"""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _native

# the blocking of k_mixture_grad.hip (GS_MIXG_COMPONENTS_PER_WG, GS_MIXG_QUERY_CHUNK, GS_MIXG_RUN): rows per workgroup of the
# row-sum kernel, the unit of its query loop -- a chunk of it is a whole number of these -- and the longest f32 sum before the
# float64 accumulators take it
COMPONENTS_PER_WORKGROUP = 256
QUERIES_PER_CHUNK = 256
RUN_LENGTH = 32
TARGET_WORKGROUPS = 2048
MAX_QUERY_CHUNKS = 64
N_FEATURES = 56

_VP, _I64 = C.c_void_p, C.c_int64
ARGTYPES = {
    # (ctx, point_cloud, point_cloud_features, point_invalid_mask, n_points, x, n_x, log_density, grad_log_density,
    #  grad_point_cloud, grad_features, grad_x, stream)
    "gs_mixture_log_density_backward": [_VP, _VP, _VP, _VP, _I64, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP],
    # (ctx, point_cloud, point_cloud_features, point_invalid_mask, n_points, k, n_k, centre, grad_re_im, grad_point_cloud,
    #  grad_features, stream)
    "gs_mixture_fourier_backward": [_VP, _VP, _VP, _VP, _I64, _VP, _I64, _VP, _VP, _VP, _VP, _VP],
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


def query_chunks(n_points, n_queries):
    """-> (chunks, queries per chunk): how the row-sum kernel splits its query loop (gs_mixg_query_chunks), a function of the two
    sizes alone"""
    cb = COMPONENTS_PER_WORKGROUP
    row_blocks = max(1, (n_points + cb - 1) // cb)
    units = (n_queries + QUERIES_PER_CHUNK - 1) // QUERIES_PER_CHUNK
    want = max(1, min(TARGET_WORKGROUPS // row_blocks, MAX_QUERY_CHUNKS, units))
    per_chunk = (units + want - 1) // want if units else 0
    return ((units + per_chunk - 1) // per_chunk if units else 0), per_chunk * QUERIES_PER_CHUNK


def _gradient(g, shape, device, what):
    if g.shape != shape:
        raise ValueError(f"{what} must have the shape {tuple(shape)}")
    g = g.detach().to(device=device)
    return g if g.dtype == torch.float32 and g.is_contiguous() else g.to(torch.float32).contiguous()


def log_density_backward(scene_or_tensors, x, log_density, grad_log_density, want_x=True, ctx=None):
    """-> (grad_point_cloud (N,3), grad_point_cloud_features (N,56), grad_x (P,3) or None), f32: the gradients of
    sum_j grad_log_density[j] log p(x_j).  log_density is what mixture.log_density returned for the same inputs.  ctx: a gs_ctx
    handle other than the process-wide one."""
    from . import mixture
    _bind()
    pc, feat, mask, x = mixture._check(scene_or_tensors, x, "x")
    n, p = pc.shape[0], x.shape[0]
    log_density = _gradient(log_density, (p,), pc.device, "log_density")
    g = _gradient(grad_log_density, (p,), pc.device, "grad_log_density")
    grad_pc = torch.zeros((n, 3), dtype=torch.float32, device=pc.device)
    grad_feat = torch.zeros((n, N_FEATURES), dtype=torch.float32, device=pc.device)
    grad_x = torch.zeros((p, 3), dtype=torch.float32, device=pc.device) if want_x else None
    _native.call("gs_mixture_log_density_backward", pc.device, ctx if ctx is not None else _native.shared_ctx(pc.device), _native.ptr(pc),
                 _native.ptr(feat), _native.ptr(mask), n, _native.ptr(x), p, _native.ptr(log_density), _native.ptr(g), _native.ptr(grad_pc),
                 _native.ptr(grad_feat), _native.ptr(grad_x))
    return grad_pc, grad_feat, grad_x


def fourier_backward(scene_or_tensors, k, centre, grad_re_im, ctx=None):
    """-> (grad_point_cloud (N,3), grad_point_cloud_features (N,56)), f32: the gradients of
    sum_j grad_re_im[j,0] Re F(k_j) + grad_re_im[j,1] Im F(k_j)"""
    from . import mixture
    _bind()
    pc, feat, mask, k = mixture._check(scene_or_tensors, k, "k")
    centre = mixture._centre(centre, pc.device)
    n, p = pc.shape[0], k.shape[0]
    g = _gradient(grad_re_im, (p, 2), pc.device, "grad_re_im")
    grad_pc = torch.zeros((n, 3), dtype=torch.float32, device=pc.device)
    grad_feat = torch.zeros((n, N_FEATURES), dtype=torch.float32, device=pc.device)
    _native.call("gs_mixture_fourier_backward", pc.device, ctx if ctx is not None else _native.shared_ctx(pc.device), _native.ptr(pc),
                 _native.ptr(feat), _native.ptr(mask), n, _native.ptr(k), p, _native.ptr(centre), _native.ptr(g), _native.ptr(grad_pc),
                 _native.ptr(grad_feat))
    return grad_pc, grad_feat


def _like(grad, shape_dtype, needed):
    """grad in the (shape, dtype) of its input, or None where no gradient is asked for"""
    return grad.to(shape_dtype[1]).reshape(shape_dtype[0]) if needed and grad is not None else None


class LogDensity(torch.autograd.Function):
    """mixture.log_density with a backward: apply(point_cloud, point_cloud_features, x, mask) -> (P,) f32, the forward's bits"""

    @staticmethod
    def forward(ctx, point_cloud, point_cloud_features, x, mask):
        from . import mixture
        pc, feat, mask, x32 = mixture._check((point_cloud, point_cloud_features, mask), x, "x")
        out = mixture._log_density(pc, feat, mask, x32)
        ctx.save_for_backward(pc, feat, x32, out)
        ctx.mask = mask
        ctx.inputs = tuple((t.shape, t.dtype) for t in (point_cloud, point_cloud_features, x))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        pc, feat, x, out = ctx.saved_tensors
        need = ctx.needs_input_grad
        grads = log_density_backward((pc, feat, ctx.mask), x, out, grad_out, want_x=need[2])
        return tuple(_like(g, t, n) for g, t, n in zip(grads, ctx.inputs, need)) + (None,)


class Fourier(torch.autograd.Function):
    """mixture.fourier's (P,2) real view with a backward: apply(point_cloud, point_cloud_features, k, centre, mask) -> (P,2) f32"""

    @staticmethod
    def forward(ctx, point_cloud, point_cloud_features, k, centre, mask):
        from . import mixture
        pc, feat, mask, k32 = mixture._check((point_cloud, point_cloud_features, mask), k, "k")
        centre = mixture._centre(centre, pc.device)
        out = mixture._fourier(pc, feat, mask, k32, centre)
        ctx.save_for_backward(pc, feat, k32, centre)
        ctx.mask = mask
        ctx.inputs = tuple((t.shape, t.dtype) for t in (point_cloud, point_cloud_features))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        pc, feat, k, centre = ctx.saved_tensors
        need = ctx.needs_input_grad
        grads = fourier_backward((pc, feat, ctx.mask), k, centre, grad_out)
        return tuple(_like(g, t, n) for g, t, n in zip(grads, ctx.inputs, need)) + (None, None, None)
