"""numpy statement of the two contracts of include/gs_exchange.h (exchange.pack_rows, exchange.merge_rows).
tests/test_exchange_ref_host.py pins it on the CPU against the dense rank-ordered sum, tests/test_gpu_exchange.py holds the
kernels to it bit for bit.

A packed row is 60 32-bit words: words 0..55 the feature-gradient row, words 56..58 the position-gradient row, word 59 the
point-cloud row id as int32 bits.  Everything here works on uint32 views, so no value passes through float arithmetic except
the adds of the merge."""
import numpy as np

ROW_WORDS, FEATURE_WORDS, POSITION_WORDS, ID_WORD = 60, 56, 3, 59


def pack(grad_features, grad_pointcloud, ids):
    """grad_features (N,56) f32, grad_pointcloud (N,3) f32, ids: the listed rows -> (len(ids), 60) uint32.  An id outside
    [0, N) gives 59 zero words and the id word -1."""
    gf, gp = np.ascontiguousarray(grad_features, np.float32), np.ascontiguousarray(grad_pointcloud, np.float32)
    n = gf.shape[0]
    out = np.zeros((len(ids), ROW_WORDS), np.uint32)
    for r, i in enumerate(np.asarray(ids, np.int64)):
        if 0 <= i < n:
            out[r, :FEATURE_WORDS] = gf[i].view(np.uint32)
            out[r, FEATURE_WORDS:ID_WORD] = gp[i].view(np.uint32)
            out[r, ID_WORD] = np.int32(i).view(np.uint32)
        else:
            out[r, ID_WORD] = 0xFFFFFFFF
    return out


def ids_of(packed_rows):
    return np.ascontiguousarray(packed_rows)[:, ID_WORD].view(np.int32)


def merge(lists, n_points, grad_features_out, grad_pointcloud_out):
    """lists: a sequence of (count_l, 60) uint32 arrays (only the rows inside each count), each ascending and unique in the ids
    it keeps; rows whose id word is outside [0, n_points) are skipped.  The two outputs, (N,56) and (N,3) f32, are updated in
    place on the union rows and keep every other bit.  -> the union, ascending int32.

    Per union row: a loop over the lists in order, f32 adds seeded by the first list that holds the row (no zero seed)."""
    kept = []
    for rows in lists:
        i = ids_of(rows) if len(rows) else np.zeros(0, np.int32)
        ok = (i >= 0) & (i < n_points)
        kept.append({int(k): r for r, k in enumerate(i) if ok[r]})
    union = np.unique(np.concatenate([np.fromiter(k.keys(), np.int64, len(k)) for k in kept] + [np.zeros(0, np.int64)])).astype(np.int32)
    gf, gp = grad_features_out, grad_pointcloud_out
    assert gf.dtype == gp.dtype == np.float32 and gf.shape == (n_points, FEATURE_WORDS) and gp.shape == (n_points, POSITION_WORDS)
    with np.errstate(all="ignore"):
        for row in union:
            acc = None
            for rows, k in zip(lists, kept):
                at = k.get(int(row))
                if at is None:
                    continue
                v = np.ascontiguousarray(rows[at, :ID_WORD]).view(np.float32)
                acc = v.copy() if acc is None else (acc + v).astype(np.float32)
            gf[row].view(np.uint32)[:] = acc[:FEATURE_WORDS].view(np.uint32)
            gp[row].view(np.uint32)[:] = acc[FEATURE_WORDS:].view(np.uint32)
    return union


def dense_rank_ordered_sum(lists, n_points):
    """What a dense exchange computes: every list scattered into a zero (N,59) f32 buffer, the buffers added in list order
    ((d0 + d1) + d2) ... -> (N,59) f32 [features | positions]"""
    total = None
    with np.errstate(all="ignore"):
        for rows in lists:
            d = np.zeros((n_points, ID_WORD), np.float32)
            if len(rows):
                i = ids_of(rows)
                ok = (i >= 0) & (i < n_points)
                d[i[ok]] = np.ascontiguousarray(rows[ok][:, :ID_WORD]).view(np.float32)
            total = d if total is None else (total + d).astype(np.float32)
    return total
