"""The touched rows of the point gradients as one packed buffer, and the fixed-order merge of several such buffers
(include/gs_exchange.h, csrc/k_exchange.hip): the device half of a sparse gradient exchange.

At a training view nine gradient rows in ten are exact zeros, and sparse.touched_rows() lists the others.  pack_rows()
gathers the listed rows of grad_pointcloud_features (N,56) and grad_pointcloud (N,3) into packed rows of 60 words -- 56
feature gradients, 3 position gradients, the row id as int32 bits -- one buffer that one collective can move.  merge_rows()
takes several such lists (one per rank after an all-gather: distributed.sparse_reduce_point_gradients; or one per view
rendered on this GPU) and leaves the ascending union of their ids as a sparse.TouchedRows and, on the union rows, the sum
over the lists in list order, ready for FusedAdam.step(rows=union).

Neither call synchronises with the host, no atomic is used and every sum has a fixed order.  There is no fallback path:
both calls go through _native.call().
"""
import ctypes as C

import torch

from . import _native
from .sparse import TouchedRows

# words of a packed row (GS_PACKED_ROW_WORDS) and the largest number of lists one merge takes (GS_MERGE_MAX_LISTS)
ROW_WORDS = 60
ROW_BYTES = 4 * ROW_WORDS
MAX_LISTS = 64

_VP, _I32, _I64 = C.c_void_p, C.c_int32, C.c_int64
ARGTYPES = {
    # (ctx, grad_features, grad_pointcloud, n_rows, ids, count, max_count, packed_out, stream)
    "gs_pack_rows": [_VP, _VP, _VP, _I64, _VP, _VP, _I64, _VP, _VP],
    # (ctx, packed, counts, n_lists, list_stride, n_rows, grad_features_out, grad_pointcloud_out, union_ids_out, union_capacity,
    #  union_count_out, stream)
    "gs_merge_rows": [_VP, _VP, _VP, _I32, _I64, _I64, _VP, _VP, _VP, _I64, _VP, _VP],
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


class PackedRows:
    """data: (capacity, 60) float32 device tensor, capacity >= max_count, whose rows [0, count) are packed rows ascending in id
    (the rows behind the count are never written); count: 0-dim int32 device tensor; n_points: N, the rows of the point cloud
    the ids index; max_count: a host-side bound of count.  The float32 dtype only names the width: a row also holds an int32,
    so the buffer is moved as bytes or int32 words (data.view(torch.int32)), never through float arithmetic."""
    __slots__ = ("data", "count", "n_points", "max_count")

    def __init__(self, data: torch.Tensor, count: torch.Tensor, n_points: int, max_count: int):
        if data.dtype != torch.float32 or count.dtype != torch.int32 or not data.is_cuda or count.device != data.device:
            raise TypeError("PackedRows takes a float32 and an int32 tensor on one GPU")
        if not data.is_contiguous() or data.dim() != 2 or data.shape[1] != ROW_WORDS or count.numel() != 1 or data.shape[0] < max_count:
            raise ValueError("data must be a contiguous (capacity >= max_count, 60) tensor, count a single element")
        self.data, self.count, self.n_points, self.max_count = data, count, int(n_points), int(max_count)


def _check_gradients(grad_pointcloud, grad_features):
    n = grad_pointcloud.shape[0]
    for g, width in ((grad_pointcloud, 3), (grad_features, 56)):
        if g.dtype != torch.float32 or not g.is_cuda or not g.is_contiguous() or tuple(g.shape) != (n, width):
            raise ValueError(f"the gradients are contiguous float32 GPU tensors of shape (N, 3) and (N, 56), got {tuple(g.shape)}")
    if grad_features.device != grad_pointcloud.device:
        raise ValueError("the two gradients live on different devices")
    return n


def pack_rows(grad_pointcloud: torch.Tensor, grad_features: torch.Tensor, rows: TouchedRows, out: torch.Tensor = None) -> PackedRows:
    """The rows `rows` lists of the two dense gradients as PackedRows, queued on the current stream.  The count tensor is the
    list's own.  A listed id outside [0, N) gives a row of zeros with the id word -1.
    out: where the packed rows go, a contiguous (capacity >= rows.max_count, 60) float32 tensor -- e.g. slice l of one
    (n_lists, list_stride, 60) buffer that merge_rows then takes as it is, with no copy in between; without it a new tensor of
    rows.max_count rows."""
    _bind()
    n = _check_gradients(grad_pointcloud, grad_features)
    if n != rows.n_points:
        raise ValueError(f"the list indexes {rows.n_points} rows, the gradients have {n}")
    dev = grad_features.device
    if out is None:
        out = torch.empty(rows.max_count, ROW_WORDS, dtype=torch.float32, device=dev)
    elif out.device != dev:
        raise ValueError("out lives on another device than the gradients")
    packed = PackedRows(out, rows.count, n, rows.max_count)                # (checks dtype, shape and capacity of `out`)
    _native.call("gs_pack_rows", dev, _native.shared_ctx(dev), _native.ptr(grad_features), _native.ptr(grad_pointcloud), n,
                 _native.ptr(rows.ids), rows.count.data_ptr(), rows.max_count, _native.ptr(out))
    return packed


def stack_packed(lists):
    """Several PackedRows of one GPU and one point cloud (one per view rendered here) -> (packed (n_lists, list_stride, 60),
    counts (n_lists,) int32) as merge_rows takes them; list_stride is the largest capacity among them (torch.stack of the
    data tensors when all capacities are equal).  This copies every list at its capacity, not at its count: a loop that knows
    a bound of the capacities beforehand packs straight into the slices of one buffer instead (pack_rows(..., out=buffer[l]))."""
    lists = list(lists)
    stride = max(p.data.shape[0] for p in lists)
    if all(p.data.shape[0] == stride for p in lists):
        packed = torch.stack([p.data for p in lists])
    else:
        packed = lists[0].data.new_empty((len(lists), stride, ROW_WORDS))
        for l, p in enumerate(lists):
            packed[l, :p.data.shape[0]].view(torch.int32).copy_(p.data.view(torch.int32))      # (as words: bits, not floats)
    return packed, torch.stack([p.count.reshape(()) for p in lists])


def merge_rows(packed: torch.Tensor, counts: torch.Tensor, n_points: int, out: torch.Tensor = None, zero: bool = False):
    """packed: (n_lists, list_stride, 60) float32, list l in packed[l, :counts[l]] (e.g. torch.stack of PackedRows.data of equal
    capacity, or the result of an all-gather); counts: (n_lists,) int32 on the same GPU; 1 <= n_lists <= 64.
    -> (grad_pointcloud (N,3), grad_pointcloud_features (N,56), union: TouchedRows with max_count = min(N, n_lists * list_stride)).

    On every row of the union the two gradients hold the sum of that row over the lists that contain it, in list order and
    seeded by the first one ((g0 + g2) + g5 for a row of lists 0, 2 and 5; a row of one list bit for bit).  Every other row
    keeps what the buffer held: `out`, a contiguous float32 vector of 59 * N elements that the two gradients become views of
    in the operator's [features | positions] layout (distributed._flat_base recognises them); without `out` a torch.empty
    buffer, i.e. rows outside the union are UNDEFINED, which is all FusedAdam.step(rows=union) needs, or a torch.zeros one
    with zero=True for a consumer that reads every row."""
    _bind()
    if packed.dtype != torch.float32 or not packed.is_cuda or packed.dim() != 3 or packed.shape[2] != ROW_WORDS or not packed.is_contiguous():
        raise ValueError("packed is a contiguous (n_lists, list_stride, 60) float32 GPU tensor")
    n_lists, stride = packed.shape[0], packed.shape[1]
    if counts.dtype != torch.int32 or counts.device != packed.device or counts.numel() != n_lists or not counts.is_contiguous():
        raise ValueError("counts is a contiguous int32 tensor of n_lists elements on packed's GPU")
    n, dev = int(n_points), packed.device
    if out is None:
        out = (torch.zeros if zero else torch.empty)(59 * n, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.device != dev or out.dim() != 1 or out.shape[0] != 59 * n or not out.is_contiguous():
        raise ValueError("out is a contiguous float32 vector of 59 * n_points elements on packed's GPU")
    elif zero:
        out.zero_()
    grad_features, grad_pointcloud = out[:56 * n].view(n, 56), out[56 * n:].view(n, 3)
    cap = min(n, n_lists * stride)
    buf = torch.empty(cap + 1, dtype=torch.int32, device=dev)           # ids (cap) and the count behind them: one allocation
    _native.call("gs_merge_rows", dev, _native.shared_ctx(dev), _native.ptr(packed), counts.data_ptr(), n_lists, stride, n,
                 _native.ptr(grad_features), _native.ptr(grad_pointcloud), _native.ptr(buf[:cap]), cap, buf.data_ptr() + 4 * cap)
    return grad_pointcloud, grad_features, TouchedRows(buf[:cap], buf[cap], n, cap)
