"""Exact k nearest neighbours over a point cloud on the GPU (include/gs_knn.h, csrc/k_knn.hip).

nearest_neighbours() returns, per row, the k smallest f32 squared distances ((dx*dx + dy*dy) + dz*dz, every operation rounded
once) to the other rows and, when asked, those rows; ties go to the smaller row, a row is excluded by its index and not by its
distance (a duplicate is a neighbour at distance 0), and rows that are masked or hold a non-finite coordinate neither ask nor
answer: their outputs are +inf / -1.  The result is bit-identical to brute force over the same expression.
mean_neighbour_distance() is what GaussianPointCloudScene.initialize() needs: the reference's
np.mean(cKDTree(x).query(x, k + 1)[0][:, 1:], axis=1), without leaving the device.

There is no fallback path: every call goes through _native.call(), and a CPU tensor is refused.
"""
import ctypes as C

import torch

from . import _native

MAX_K = 8
# rows per leaf of the search tree (GS_KNN_LEAF in k_knn.hip): one wave
LEAF = 64

_VP, _I32, _I64 = C.c_void_p, C.c_int32, C.c_int64
ARGTYPES = {
    # (ctx, xyz, invalid_mask, n_points, k, d2_out, idx_out, stream)
    "gs_knn": [_VP, _VP, _VP, _I64, _I32, _VP, _VP, _VP],
}
_bound = False


def _bind():
    """argtypes of the entry point, set once on the loaded library (it is not part of _native.SYMBOLS)"""
    global _bound
    if not _bound:
        L = _native.lib()
        for name, argtypes in ARGTYPES.items():
            if not hasattr(L, name):
                raise _native.NativeLibraryError(f"{_native.LIB_PATH} does not export {name}")
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
        _bound = True


def _check(point_cloud, k, point_invalid_mask):
    if not isinstance(point_cloud, torch.Tensor) or point_cloud.dim() != 2 or point_cloud.shape[1] != 3:
        raise ValueError("point_cloud must be an (N,3) tensor")
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
    if not point_cloud.is_cuda:
        raise ValueError(f"nearest neighbours are searched on the GPU: point_cloud is on {point_cloud.device}, move it to a "
                         "cuda/hip device first (there is no CPU path)")
    pc = point_cloud.detach()
    pc = pc if pc.dtype == torch.float32 and pc.is_contiguous() else pc.to(torch.float32).contiguous()
    mask = point_invalid_mask
    if mask is not None:
        if mask.device != pc.device or mask.shape != (pc.shape[0],):
            raise ValueError("point_invalid_mask must be an (N,) tensor on the point cloud's device")
        mask = mask if mask.dtype == torch.int8 and mask.is_contiguous() else (mask != 0).to(torch.int8).contiguous()
    return pc, mask


def nearest_neighbours(point_cloud, k=3, point_invalid_mask=None, return_indices=False):
    """-> d2 (N,k) f32 ascending squared distances [, idx (N,k) int32 rows]; +inf / -1 where there is no neighbour.
    Queued on the current stream of the point cloud's device; no host synchronisation."""
    _bind()
    pc, mask = _check(point_cloud, k, point_invalid_mask)
    n = pc.shape[0]
    d2 = torch.empty((n, k), dtype=torch.float32, device=pc.device)
    idx = torch.empty((n, k), dtype=torch.int32, device=pc.device) if return_indices else None
    _native.call("gs_knn", pc.device, _native.shared_ctx(pc.device), _native.ptr(pc), _native.ptr(mask), n, int(k),
                 _native.ptr(d2), _native.ptr(idx))
    return (d2, idx) if return_indices else d2


def mean_neighbour_distance(point_cloud, k=3, point_invalid_mask=None):
    """-> (N,) f32: the mean distance to the k nearest other rows (inf where a row has fewer, or takes no part)"""
    return nearest_neighbours(point_cloud, k, point_invalid_mask).sqrt().mean(1)
