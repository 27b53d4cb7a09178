/* gs_sparse.h -- the rows of the point cloud a backward touched, as a list on the device, and an Adam step over such a list.
 *
 * At a training view most in-camera points get no contribution from any pixel; gs_backward knows which (it skips them,
 * and their gradient rows are exact zeros).  gs_touched_rows hands that knowledge out as an ascending list of point-cloud
 * rows in device memory, and gs_adam_step_rows is its first consumer: gs_adam_step's update on the listed rows only.
 *
 *   gs_backward(ctx, frame, ..., &out, stream);                  // dense gradients, as always
 *   gs_touched_rows(ctx, frame, ids, M, count, stream);          // ids[0 .. *count): rows with num_affected_pixels > 0
 *   gs_adam_step_rows(ctx, features, grad_features, m, v, N, 56, ids, count, M, lr, b1, b2, eps, step, stream);
 *
 * The list describes ONE backward: the tags it is built from belong to the context and are overwritten by the context's
 * next backward, whichever frame that one runs on.  Rows not listed keep their parameters AND their moments (no decay):
 * torch.optim.Adam restricted to the listed rows with the global step in the bias correction.
 *
 * Same library, same rules as gs_rasterizer.h: status codes, gs_last_error(), the call's stream last.  Not part of
 * GS_ABI_VERSION's function list.  Neither call synchronises with the host or copies anything to it, and no float or
 * integer atomic decides a position: two runs give the same list.
 */
#ifndef GS_SPARSE_H
#define GS_SPARSE_H
#include "gs_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The point-cloud rows n whose point took a contribution from at least one pixel in the LAST backward run on `frame`
 * (exactly the rows with num_affected_pixels > 0), ascending, ids_out[0 .. *count_out).  Both outputs are device memory;
 * entries at and beyond *count_out are not written.  No host synchronisation, no device-to-host copy.
 * GS_ERR_INVALID_ARGUMENT: a NULL pointer, capacity below the frame's n_points_in_camera, a frame that does not hold
 * GS_STAGE_PROJECT (frames made from records are refused).  GS_ERR_STATE: not a live frame of the context, no backward
 * (gs_backward, gs_backward_ex, gs_backward_projected) has run on the frame, or another backward has run on the context
 * since the frame's.  A frame with no in-camera point or no pair gives *count_out = 0. */
int gs_touched_rows(gs_ctx* ctx, const gs_frame* frame, int32_t* ids_out, int64_t capacity, int32_t* count_out, gs_stream stream);

/* gs_adam_step's update, element for element the same arithmetic, applied to the listed rows only: rows ids[0 .. *count)
 * of param / grad / exp_avg / exp_avg_sq, each (n_rows, row_len) f32 row-major.  Rows not listed keep every bit of param
 * and of both moments.  `step` is the caller's global step count (bias correction as in gs_adam_step).  ids ascending and
 * unique, *count <= max_count (a host-side upper bound that sizes the launch, e.g. the frame's M); ids and count are
 * device memory, an id outside [0, n_rows) is skipped.
 * GS_ERR_INVALID_ARGUMENT: a NULL pointer (when n_rows > 0 and max_count > 0), row_len < 1, step < 1, n_rows < 0 or
 * max_count < 0.  No launch when max_count == 0 or n_rows == 0. */
int gs_adam_step_rows(gs_ctx* ctx, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n_rows,
                      int32_t row_len, const int32_t* ids, const int32_t* count, int64_t max_count,
                      float lr, float beta1, float beta2, float eps, int64_t step, gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
