"""The rows a backward touched, as a list on the device, and what consumes it (include/gs_sparse.h, csrc/k_sparse.hip).

At a training view most in-camera points get no contribution from any pixel: the backward skips them and their gradient
rows are exact zeros.  touched_rows() asks the library for the ascending list of the other rows -- those with
num_affected_pixels > 0 -- without a host synchronisation; FusedAdam.step(rows=...) (optim.py) updates only them.  With
GaussianPointCloudRasterisation.track_touched_rows set, every backward leaves its list in rast.last_touched_rows.

The list describes ONE backward: the tags it is built from belong to the library context and are overwritten by the
context's next backward, so it is taken directly after the backward it describes.  There is no fallback path: both calls go
through _native.call().
"""
import ctypes as C

import torch

from . import _native

# points per workgroup of the compaction (GS_ROWS_BLOCK in k_sparse.hip): one workgroup and one launch up to this many
# in-camera points, a count launch and a scatter launch beyond
COMPACT_BLOCK = 1024

_VP, _I32, _I64, _F32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
ARGTYPES = {
    # (ctx, frame, ids_out, capacity, count_out, stream)
    "gs_touched_rows": [_VP, _VP, _VP, _I64, _VP, _VP],
    # (ctx, param, grad, exp_avg, exp_avg_sq, n_rows, row_len, ids, count, max_count, lr, beta1, beta2, eps, step, stream)
    "gs_adam_step_rows": [_VP, _VP, _VP, _VP, _VP, _I64, _I32, _VP, _VP, _I64, _F32, _F32, _F32, _F32, _I64, _VP],
}
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


class TouchedRows:
    """ids: int32 device tensor of capacity >= max_count, ascending point-cloud rows in ids[:count]; count: 0-dim int32
    device tensor; n_points: N, the rows of the point cloud the list indexes; max_count: M, the frame's in-camera points,
    a host-side bound of count that sizes the consumers' launches."""
    __slots__ = ("ids", "count", "n_points", "max_count")

    def __init__(self, ids: torch.Tensor, count: torch.Tensor, n_points: int, max_count: int):
        if ids.dtype != torch.int32 or count.dtype != torch.int32 or not ids.is_cuda or count.device != ids.device:
            raise TypeError("TouchedRows takes int32 tensors on one GPU")
        if not ids.is_contiguous() or ids.dim() != 1 or count.numel() != 1 or ids.shape[0] < max_count:
            raise ValueError("ids must be a contiguous vector of at least max_count entries, count a single element")
        self.ids, self.count, self.n_points, self.max_count = ids, count, int(n_points), int(max_count)

    def tensor(self) -> torch.Tensor:
        """ids[:count].  Reads the count on the host, i.e. SYNCHRONISES with the device: for tests and debugging, never on
        the training path."""
        return self.ids[:int(self.count.item())]


def touched_rows(frame) -> TouchedRows:
    """The TouchedRows of the last backward on `frame` (a kept frame of GaussianPointCloudRasterisation.forward), queued on
    the current stream.  RuntimeError when no backward has run on the frame or another one has run on its context since."""
    _bind()
    M = frame.n_points_in_camera
    # ids (M) and the count behind them: one allocation
    buf = torch.empty(M + 1, dtype=torch.int32, device=frame.device)
    _native.call("gs_touched_rows", frame.device, frame._context.handle, frame.handle, buf.data_ptr(), M, buf.data_ptr() + 4 * M)
    return TouchedRows(buf[:M], buf[M], frame.n_points, M)


def adam_step_rows(p, grad, exp_avg, exp_avg_sq, rows: TouchedRows, lr, beta1, beta2, eps, step):
    """gs_adam_step_rows on one (n_points, ...) parameter: gs_adam_step's update on the listed rows only."""
    _bind()
    n = p.shape[0]
    _native.call("gs_adam_step_rows", p.device, _native.shared_ctx(p.device), _native.ptr(p), _native.ptr(grad), _native.ptr(exp_avg),
                 _native.ptr(exp_avg_sq), n, p.numel() // n if n else 1, rows.ids.data_ptr(), rows.count.data_ptr(), rows.max_count,
                 lr, beta1, beta2, eps, step)
