"""Vector quantisation on the GPU (include/gs_vq.h, csrc/k_vq.hip): the two halves of a k-means iteration and the loop around them.

  labels, dist = assign(x, codebook)              # nearest centroid per row, on the matrix cores, pinned to the last bit
  counts, sums = update(x, labels, codebook)      # every centroid to the weighted mean of its rows, in place, float64 in row order
  codebook, labels, history = kmeans(x, 4096)     # Lloyd's iterations from rows drawn by seed

x is (N, D) float32 with D <= 64, a codebook (K, D) float32 with K <= 65536.  Both are copied into rows padded to a multiple of
four floats when D is not one (the library reads 16 bytes at a time); a tensor that already is passes as it is.  The rules, to
the parenthesis, are the header's.  There is no fallback path: every call goes through _native.call(), and a CPU tensor is
refused.
"""
import ctypes as C

import torch

from . import _native

MAX_DIM = 64                                    # GS_VQ_MAX_DIM
MAX_CODES = 65536                               # GS_VQ_MAX_CODES

_VP, _I32, _I64 = C.c_void_p, C.c_int32, C.c_int64

ARGTYPES = {
    # (ctx, x, ldx, n_rows, dim, codebook, ldc, n_codes, labels, dist, scratch, stream)
    "gs_vq_assign": [_VP, _VP, _I64, _I64, _I32, _VP, _I64, _I32, _VP, _VP, _VP, _VP],
    # (ctx, x, ldx, n_rows, dim, weights, labels, codebook, ldc, n_codes, counts, weight_sums, scratch, stream)
    "gs_vq_update": [_VP, _VP, _I64, _I64, _I32, _VP, _VP, _VP, _I64, _I32, _VP, _VP, _VP, _VP],
}
_bound = False


def _bind():
    """argtypes of the entry points, set once on the loaded library (they are not part of _native.SYMBOLS)"""
    global _bound
    if not _bound:
        L = _native.lib()
        for name in list(ARGTYPES) + ["gs_vq_scratch_bytes"]:
            if not hasattr(L, name):
                raise _native.NativeLibraryError(f"{_native.LIB_PATH} does not export {name}")
        for name, argtypes in ARGTYPES.items():
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
        L.gs_vq_scratch_bytes.argtypes, L.gs_vq_scratch_bytes.restype = [_I64, _I32, _I32], _I64
        _bound = True


def scratch_bytes(n_rows: int, n_codes: int, dim: int) -> int:
    _bind()
    return int(_native.lib().gs_vq_scratch_bytes(int(n_rows), int(n_codes), int(dim)))


def _matrix(t, what, device=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"vector quantisation runs on the GPU: {what} must be a tensor on a cuda/hip device (there is no CPU path)")
    if t.dtype != torch.float32 or t.dim() != 2 or not 1 <= t.shape[1] <= MAX_DIM:
        raise ValueError(f"{what} must be a float32 tensor of shape (rows, 1..{MAX_DIM})")
    if device is not None and t.device != device:
        raise ValueError(f"{what} must be on {device}")
    return t.detach()


def _vector(t, what, n, dtype, device):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"vector quantisation runs on the GPU: {what} must be a tensor on a cuda/hip device (there is no CPU path)")
    if t.dtype != dtype or tuple(t.shape) != (n,) or t.device != device:
        raise ValueError(f"{what} must be a {dtype} tensor of shape ({n},) on {device}")
    return t.detach().contiguous()


def padded(t):
    """t (rows, D) as the library reads it: rows of a multiple of four floats, 16-byte aligned.  -> (tensor, leading dimension);
    t itself when it already is that."""
    d = t.shape[1]
    if t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= d and t.data_ptr() % 16 == 0 and t.shape[0] > 0:
        return t, t.stride(0)
    ld = (d + 3) // 4 * 4
    out = torch.zeros(max(t.shape[0], 1), ld, dtype=torch.float32, device=t.device)
    out[:t.shape[0], :d] = t
    return out, ld


def _scratch(n, k, d, device):
    return torch.empty((scratch_bytes(n, k, d) + 7) // 8, dtype=torch.int64, device=device)


def assign(x, codebook, with_dist: bool = True):
    """gs_vq_assign: -> (labels (N) int32, dist (N) float32 or None).  labels[n] is the centroid nearest to row n, the smaller index
    on a tie, -1 for a row with a non-finite value (or when no centroid is finite); dist[n] the squared distance to it."""
    _bind()
    x = _matrix(x, "x")
    codebook = _matrix(codebook, "codebook", x.device)
    n, d = x.shape
    k = codebook.shape[0]
    if codebook.shape[1] != d or not 1 <= k <= MAX_CODES:
        raise ValueError(f"codebook must be (1..{MAX_CODES}, {d})")
    xp, ldx = padded(x)
    cp, ldc = padded(codebook)
    labels = torch.empty(n, dtype=torch.int32, device=x.device)
    dist = torch.empty(n, dtype=torch.float32, device=x.device) if with_dist else None
    scratch = _scratch(n, k, d, x.device)
    _native.call("gs_vq_assign", x.device, _native.shared_ctx(x.device), _native.ptr(xp), ldx, n, d, _native.ptr(cp), ldc, k,
                 _native.ptr(labels), _native.ptr(dist), scratch.data_ptr())
    return labels, dist


def update(x, labels, codebook, weights=None):
    """gs_vq_update: every centroid with members becomes their weighted mean, IN PLACE in codebook (K, D); one without keeps
    every bit.  A row counts when its label is in [0, K) and its weight (1 without weights) is positive and finite.
    -> (counts (K) int32, weight_sums (K) float64)."""
    _bind()
    x = _matrix(x, "x")
    codebook = _matrix(codebook, "codebook", x.device)
    n, d = x.shape
    k = codebook.shape[0]
    if codebook.shape[1] != d or not 1 <= k <= MAX_CODES:
        raise ValueError(f"codebook must be (1..{MAX_CODES}, {d})")
    labels = _vector(labels, "labels", n, torch.int32, x.device)
    weights = None if weights is None else _vector(weights, "weights", n, torch.float32, x.device)
    xp, ldx = padded(x)
    cp, ldc = padded(codebook)
    counts = torch.empty(k, dtype=torch.int32, device=x.device)
    sums = torch.empty(k, dtype=torch.float64, device=x.device)
    _native.call("gs_vq_update", x.device, _native.shared_ctx(x.device), _native.ptr(xp), ldx, n, d, _native.ptr(weights), _native.ptr(labels),
                 cp.data_ptr(), ldc, k, counts.data_ptr(), sums.data_ptr(), None)
    if cp is not codebook:
        codebook.copy_(cp[:, :d])
    return counts, sums


def initial_rows(n: int, k: int, seed: int = 0):
    """the rows kmeans() starts from: the first min(k, n) of a permutation drawn on the host from seed"""
    return torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))[:min(int(k), n)]


def kmeans(x, k: int, iters: int = 10, weights=None, seed: int = 0, reseed_empty: bool = True):
    """Lloyd's iterations: assign, update, and (reseed_empty) every code left without members takes one of the rows farthest from
    their centroids, which costs one read of the empty count per iteration.  -> (codebook (k', D), labels (N) int32 of the last
    assignment against the returned codebook, history: the weighted distortion sum w_n dist_n of every iteration's assignment,
    a list of floats summed in float64 on the device and read once at the end).  k' = min(k, N)."""
    x = _matrix(x, "x")
    n, d = x.shape
    if n < 1 or k < 1:
        raise ValueError("kmeans needs at least one row and one code")
    if weights is not None:
        weights = _vector(weights, "weights", n, torch.float32, x.device)
    xp, _ = padded(x)
    xp = xp[:, :d]                                                   # a view of padded rows: passes through padded() as it is
    rows = initial_rows(n, k, seed).to(x.device)
    k = rows.numel()
    ld = (d + 3) // 4 * 4
    codebook = torch.zeros(k, ld, dtype=torch.float32, device=x.device)[:, :d]
    codebook.copy_(x[rows])
    history = torch.zeros(max(iters, 0) + 1, dtype=torch.float64, device=x.device)

    def distortion(dist):
        dd = torch.nan_to_num(dist.double(), nan=0.0)
        return (dd * weights.double().clamp_min(0.0)).sum() if weights is not None else dd.sum()
    def reseed(counts, dist):
        empty = torch.nonzero(counts == 0)[:, 0]
        if empty.numel() > 0:                                        # the host read
            far = torch.topk(torch.nan_to_num(dist, nan=-1.0), min(empty.numel(), n)).indices
            codebook[empty[:far.numel()]] = x[far]
        return empty.numel()
    for it in range(iters):
        labels, dist = assign(xp, codebook)
        history[it] = distortion(dist)
        counts, _ = update(xp, labels, codebook, weights)
        if reseed_empty:
            reseed(counts, dist)
    labels, dist = assign(xp, codebook)
    for _ in range(3 if reseed_empty else 0):                        # codes the last move emptied, if any
        if not reseed(torch.bincount(labels.clamp_min(0).long(), minlength=k), dist):
            break
        labels, dist = assign(xp, codebook)
    history[max(iters, 0)] = distortion(dist)
    return codebook.contiguous(), labels, [float(v) for v in history.cpu()]
