/* gs_knn.h -- exact k nearest neighbours over a point cloud on the device: what a scene initialised from a bare x,y,z cloud
 * needs (every Gaussian's first scale is the mean distance to its three nearest neighbours), and the neighbour rows
 * themselves for anything else that wants them (neighbour-based regularisers, pruning heuristics).
 *
 *   gs_knn(ctx, xyz, invalid_mask, N, 3, d2, idx, stream);      // d2[n][0..3) ascending squared distances, idx[n][0..3) their rows
 *
 * Same library, same rules as gs_rasterizer.h: status codes, gs_last_error(), the call's stream last.  Not part of
 * GS_ABI_VERSION's function list.
 *
 * What is computed
 *  - A row TAKES PART if its mask byte is 0 (or invalid_mask is NULL) and its three coordinates are finite.  A row with a
 *    NaN or infinite coordinate is treated as masked.  A row that does not take part is neither a query nor a neighbour:
 *    its k outputs are +inf / -1, and it moves no other row's result.
 *  - The squared distance of rows q and p is the f32 value ((dx*dx + dy*dy) + dz*dz) with dx = x_q - x_p (dy, dz alike):
 *    every operation rounded once to f32, no fused multiply-add.  It is symmetric in q and p.  (Large finite coordinates
 *    may overflow it to +inf; such a pair is still a pair and is reported with its row.)
 *  - For a row q that takes part, the output is the k smallest pairs (d2, p) over the rows p != q that take part, pairs
 *    ordered lexicographically: ties in distance go to the smaller row.  Ascending.  q itself is excluded by ROW, not by
 *    distance: a duplicate of q is a neighbour at distance 0 (as scipy's cKDTree.query(k + 1)[:, 1:] has it).  With fewer
 *    than k other rows taking part, the tail is +inf / -1.
 *  - The result is a function of the input alone -- it does not depend on any traversal or scheduling order, two calls
 *    give the same bits -- and is bit-identical to a brute-force evaluation of the same f32 expression.
 *
 * How (csrc/k_knn.hip): Morton order inside the bounding box of the rows taking part, a complete binary tree of f32 boxes
 * over runs of 64 sorted rows, one wave per run.  Near O(N log N) also when outliers inflate the box by orders of magnitude.
 *
 * Work memory belongs to the context (buffers of its own, counted by gs_ctx_device_bytes, about 44 bytes per row; never a
 * buffer that a kept frame or a pending backward reads), so a call may sit between a forward and its backward.  The call
 * is meant for initialisation, not for the per-iteration path.  It does NOT synchronise with the host and copies nothing
 * to it: everything is queued on `stream`.
 */
#ifndef GS_KNN_H
#define GS_KNN_H
#include "gs_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest n_points of one call (2^30): row numbers carry a flag bit inside the library.  This is the limit of the
 * index arithmetic, not a measured size: times exist up to 10^6 rows (profiles/knn_init_bench.json).  The digit table of
 * the sort (256 words per 1024 rows) is scanned by one workgroup, eight times per call -- 244 steps of 1024 words at
 * 10^6 rows, 2.6e5 steps over a 1 GB table at the limit -- so the cost far beyond 10^7 rows is not measured and is
 * expected to be dominated by that scan. */
#define GS_KNN_MAX_POINTS 1073741824

/* xyz (n_points,3) f32, invalid_mask n_points int8 or NULL, d2_out (n_points,k) f32, idx_out (n_points,k) int32 or NULL
 * (distances only): all device memory, row-major.
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx NULL, k outside [1, 8], n_points outside
 * [0, GS_KNN_MAX_POINTS], xyz or d2_out NULL with n_points > 0.  n_points == 0 is GS_OK with no launch. */
int gs_knn(gs_ctx* ctx, const float* xyz, const int8_t* invalid_mask, int64_t n_points, int32_t k, float* d2_out,
           int32_t* idx_out, gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
