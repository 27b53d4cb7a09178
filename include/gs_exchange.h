/* gs_exchange.h -- the touched rows of the point gradients as ONE packed buffer, and the fixed-order merge of several such
 * buffers: the device half of a sparse gradient exchange (view-parallel training: pack, all-gather, merge), and of the
 * several-views-per-step merge on one GPU.
 *
 *   gs_touched_rows(ctx, frame, ids, M, count, stream);                                  // include/gs_sparse.h
 *   gs_pack_rows(ctx, grad_features, grad_pointcloud, N, ids, count, M, packed, stream); // packed[0 .. *count)
 *   ... move `packed` and `count` of every rank / view into one (n_lists, list_stride) buffer ...
 *   gs_merge_rows(ctx, packed_all, counts, n_lists, list_stride, N, grad_features_out, grad_pointcloud_out,
 *                 union_ids, capacity, union_count, stream);
 *   gs_adam_step_rows(ctx, ..., union_ids, union_count, capacity, ...);                  // include/gs_sparse.h
 *
 * A packed row is GS_PACKED_ROW_WORDS = 60 32-bit words, 240 bytes (fifteen 16-byte quads, so every row of a 16-byte
 * aligned buffer is 16-byte aligned):
 *   words  0..55  the row of grad_features    (N,56)
 *   words 56..58  the row of grad_pointcloud  (N,3)
 *   word   59     the point-cloud row id, the bits of an int32
 * A list is `count` packed rows, ascending in id and unique.  It is moved as bytes or int32 words, never as floats.
 *
 * Same library, same rules as gs_sparse.h: status codes, gs_last_error(), the call's stream last.  Not part of
 * GS_ABI_VERSION's function list.  Neither call synchronises with the host or copies anything to it, no float or integer
 * atomic is used, and two runs give the same bits.
 */
#ifndef GS_EXCHANGE_H
#define GS_EXCHANGE_H
#include "gs_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_PACKED_ROW_WORDS 60
#define GS_MERGE_MAX_LISTS 64

/* Gathers rows ids[0 .. *count) of grad_features (n_rows,56) and grad_pointcloud (n_rows,3), f32 row-major, into
 * packed_out[0 .. *count).  ids and count are device memory; *count <= max_count, a host-side upper bound that sizes the
 * launch (as in gs_adam_step_rows).  Rows of packed_out at and beyond *count are not written.  An id outside [0, n_rows)
 * within the count gives a packed row of 59 zero words and the id word -1, which gs_merge_rows skips.  packed_out is 16-byte
 * aligned and holds max_count rows.
 * GS_ERR_INVALID_ARGUMENT: a NULL pointer (when n_rows > 0 and max_count > 0), n_rows < 0 or max_count < 0, n_rows above
 * 2^31 - 1, a packed_out that is not 16-byte aligned.  No launch when max_count == 0 or n_rows == 0. */
int gs_pack_rows(gs_ctx* ctx, const float* grad_features, const float* grad_pointcloud, int64_t n_rows, const int32_t* ids,
                 const int32_t* count, int64_t max_count, float* packed_out, gs_stream stream);

/* Merges n_lists packed lists: list l is rows packed[l * list_stride .. l * list_stride + counts[l]) (counts: int32[n_lists]
 * in device memory, each clamped to [0, list_stride]; the values of the rows behind a count are never used).
 *   union_ids_out[0 .. *union_count_out): the ascending, unique union of the lists' ids (device memory; entries at and
 *     beyond the count are not written).  A row whose id word is outside [0, n_rows) is skipped.
 *   For every union row, the sum of that row over the lists that hold it, in list order, seeded by the first holder's
 *     values (no zero seed): a row held by one list is copied bit for bit, one held by lists 0, 2 and 5 is (g0 + g2) + g5 in
 *     f32.  The sums are stored at the row's own place in grad_features_out (n_rows,56) and grad_pointcloud_out (n_rows,3);
 *     rows outside the union keep every bit of what the two outputs held.
 * A run of r skipped rows inside a count costs r^2 / 2 loads in the merge: cheap for the odd bad id, not for a list of them.
 * Scratch (one tag byte per point-cloud row, the ids of all lists, the compaction's block totals) belongs to the context
 * and grows on demand.  With n_rows == 0 or list_stride == 0 there is nothing to merge: *union_count_out = 0 is the only
 * effect (none when union_count_out is NULL).
 * GS_ERR_INVALID_ARGUMENT: n_lists outside [1, GS_MERGE_MAX_LISTS], list_stride < 0, n_rows < 0 or above 2^31 - 2^12,
 * union_capacity below min(n_rows, n_lists * list_stride), a NULL pointer with something to merge, a packed that is not
 * 16-byte aligned. */
int gs_merge_rows(gs_ctx* ctx, const float* packed, const int32_t* counts, int32_t n_lists, int64_t list_stride, int64_t n_rows,
                  float* grad_features_out, float* grad_pointcloud_out, int32_t* union_ids_out, int64_t union_capacity,
                  int32_t* union_count_out, gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
