/* gs_targets_rgba.h -- gs_image_resample (gs_targets.h) for a four-channel source, with the fourth channel kept: the training
 * target of one view AND its per-pixel weight (an RGBA capture's alpha, or a mask packed into channel 3) in the same launch.
 *
 *   gs_image_resample_rgba(ctx, src, GS_IMAGE_U8_HWC, 4, H, W, pitch, H / f, W / f, h, w, dst, stream);   // dst (4,h,w) f32
 *
 * Planes 0..2 of dst are bit for bit what gs_image_resample writes for the same arguments.  Plane 3 is channel 3 through the
 * same filter: (float)v / 255.0f for uint8, the same cached tables, the same chains of fused multiply-adds in the same order.
 * A resized binary mask therefore comes out fractional along its borders: a soft weight.  Equal sizes are the identity.
 *
 * Arguments, bounds, tables and status codes are gs_image_resample's, except: src_channels must be 4
 * (GS_ERR_INVALID_ARGUMENT otherwise, before anything needs a device), and dst is f32 (4, h_out, w_out) contiguous.
 * Not part of GS_ABI_VERSION's function list.
 */
#ifndef GS_TARGETS_RGBA_H
#define GS_TARGETS_RGBA_H
#include "gs_targets.h"

#ifdef __cplusplus
extern "C" {
#endif

int gs_image_resample_rgba(gs_ctx* ctx, const void* src, int32_t src_format, int32_t src_channels, int32_t H_in, int32_t W_in,
                           int64_t src_row_pitch_bytes, int32_t h_full, int32_t w_full, int32_t h_out, int32_t w_out, float* dst,
                           gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
