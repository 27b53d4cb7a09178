"""include/gs_vq.h restated on the host.  The assignment is vq_ref.c (libm's fmaf: numpy has no fused multiply-add and a float64
emulation rounds twice), compiled on first use into the directory the caller gives; the update is a numpy loop in float64; the
k-means loop around them is vq.kmeans' without the reseeding.  Nothing here imports the package."""
import ctypes as C
import os
import subprocess

import numpy as np

MAX_DIM = 64                    # GS_VQ_MAX_DIM
MAX_CODES = 65536               # GS_VQ_MAX_CODES
_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib(build_dir):
    """vq_ref.c compiled with gcc -O2 -ffp-contract=off into build_dir (once per process)"""
    global _lib
    if _lib is None:
        out = os.path.join(str(build_dir), "libvq_ref.so")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-std=c99", "-shared", "-fPIC", os.path.join(_HERE, "vq_ref.c"), "-o", out, "-lm"])
        L = C.CDLL(out)
        L.vq_ref_assign.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vq_ref_assign.restype = None
        _lib = L
    return _lib


def padded(a):
    """(rows, D) float32 -> (a C-contiguous copy with rows of a multiple of four floats, that leading dimension)"""
    a = np.asarray(a, np.float32)
    ld = (a.shape[1] + 3) // 4 * 4
    out = np.zeros((a.shape[0], ld), np.float32)
    out[:, :a.shape[1]] = a
    return out, ld


def assign(build_dir, x, codebook, ldx=None, ldc=None, dim=None):
    """-> (labels (N) int32, dist (N) float32).  x (N, D) and codebook (K, D); or, with ldx / ldc / dim given, arrays of that
    leading dimension whose columns >= dim must not matter."""
    x, codebook = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(codebook, np.float32)
    dim = x.shape[1] if dim is None else dim
    ldx = x.shape[1] if ldx is None else ldx
    ldc = codebook.shape[1] if ldc is None else ldc
    n, k = x.shape[0], codebook.shape[0]
    labels, dist, cc = np.empty(n, np.int32), np.empty(n, np.float32), np.empty(k, np.float32)
    lib(build_dir).vq_ref_assign(x.ctypes.data, ldx, n, dim, codebook.ctypes.data, ldc, k, cc.ctypes.data, labels.ctypes.data, dist.ctypes.data)
    return labels, dist


def update(x, labels, codebook, weights=None):
    """-> (new codebook, counts (K) int32, weight_sums (K) float64): members in ascending row order, float64, one after the other"""
    x, codebook = np.asarray(x, np.float32), np.array(codebook, np.float32, copy=True)
    k, d = codebook.shape
    counts, W = np.zeros(k, np.int32), np.zeros(k, np.float64)
    S = np.zeros((k, d), np.float64)
    with np.errstate(all="ignore"):
        for n in range(x.shape[0]):
            c = int(labels[n])
            if not 0 <= c < k:
                continue
            w = np.float32(1.0) if weights is None else np.float32(weights[n])
            if not (w > 0 and np.isfinite(w)):
                continue
            counts[c] += 1
            W[c] = W[c] + np.float64(w)
            S[c] = S[c] + np.float64(w) * x[n].astype(np.float64)
        for c in range(k):
            if counts[c] > 0:
                codebook[c] = (S[c] / W[c]).astype(np.float32)
    return codebook, counts, W


def kmeans(build_dir, x, rows, iters, weights=None):
    """`iters` times assign and update from the centroids x[rows], then one more assignment -> (codebook, labels, dist, counts of
    the last update)"""
    x = np.asarray(x, np.float32)
    codebook = x[np.asarray(rows)].copy()
    counts = None
    for _ in range(iters):
        labels, _ = assign(build_dir, x, codebook)
        codebook, counts, _ = update(x, labels, codebook, weights)
    labels, dist = assign(build_dir, x, codebook)
    return codebook, labels, dist, counts


def brute_force(x, codebook):
    """float64: (d2 (N,K), tol (N)) with tol_n = 2 (Dp + 3) 2^-24 (max_k (2 sum_j |x_j c_kj| + sum_j c_kj^2) + sum_j x_j^2), the
    bound of the f32 chains of the header: each of the Dp + 1 roundings of s and the Dp + 1 of xx + best errs by at most 2^-24
    of a partial sum no larger than that bracket"""
    x, c = np.asarray(x, np.float64), np.asarray(codebook, np.float64)
    dp = (x.shape[1] + 3) // 4 * 4
    d2, tol = np.empty((x.shape[0], c.shape[0])), np.empty(x.shape[0])
    for lo in range(0, x.shape[0], 128):
        xs = x[lo:lo + 128]
        d2[lo:lo + 128] = ((xs[:, None, :] - c[None, :, :]) ** 2).sum(-1)
        size = 2.0 * (np.abs(xs) @ np.abs(c).T) + (c * c).sum(-1)[None, :]
        tol[lo:lo + 128] = 2.0 * (dp + 3) * 2.0 ** -24 * (size.max(1) + (xs * xs).sum(-1))
    return d2, tol
