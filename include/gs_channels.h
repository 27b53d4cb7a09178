/* gs_channels.h -- per-Gaussian feature channels rendered over a frame of libgsrast.so.
 *
 * A frame made by gs_forward already holds everything a further blend pass needs: the sorted pairs, the projected
 * records, the tile ranges.  With the forward's pixel_offset_of_last_effective_point these two calls blend any C
 * values per Gaussian (semantic features, labels, normals, a scalar field) with the weights the colour was blended
 * with, and take the gradient of the result back to the values:
 *
 *   out[y, x, c]       = sum_i w_i * values[id_i, c]                      w_i = alpha_i * T_i
 *   grad_values[id, c] = sum over pixels of w_i(pixel) * grad_out[pixel, c]
 *
 * over the contributors i of the pixel, exactly the forward's own (same alpha >= 1/255 decision, same clamp at 0.99,
 * same transmittance).  No normalisation by the accumulated alpha.  GEOMETRY IS FROZEN: no gradient reaches means,
 * covariances, opacities or poses.  Rows of `values` for points outside the camera are never read.  The backward uses
 * no float atomics: two runs give the same bits.
 *
 * Same library, same rules as gs_rasterizer.h: status codes, gs_last_error(), the call's stream last.  Not part of
 * GS_ABI_VERSION's function list; GS_ERR_INVALID_ARGUMENT for a NULL pointer, n_channels outside 1..GS_CHANNELS_MAX, an
 * rgb_only frame or a frame that does not hold both GS_STAGE_PROJECT and GS_STAGE_RASTER (frames made from records or
 * shards are refused); GS_ERR_STATE for a handle that is not a live frame of the context.
 */
#ifndef GS_CHANNELS_H
#define GS_CHANNELS_H
#include "gs_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_CHANNELS_MAX 64

/* values: device (N,C) f32 row-major, one row per point-cloud row.  out: device (H,W,C) f32, every element written
 * (zeros when the frame has no pairs).  frame: from gs_forward, kept or transient.
 * pixel_offset_of_last_effective_point: that forward's output, (H,W) int32. */
int gs_channels_forward(gs_ctx* ctx, const gs_frame* frame, const float* values, int32_t n_channels,
                        const int32_t* pixel_offset_of_last_effective_point, float* out, gs_stream stream);

/* grad_out: device (H,W,C) f32.  grad_values: device (N,C) f32, every row written; a row outside the camera, or one no
 * pixel took a contribution from, is exactly zero.  Scratch is the context's own, apart from gs_backward's. */
int gs_channels_backward(gs_ctx* ctx, const gs_frame* frame, const float* grad_out, int32_t n_channels,
                         const int32_t* pixel_offset_of_last_effective_point, float* grad_values, gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
