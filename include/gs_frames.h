/* gs_frames.h -- a rendered frame as the 8-bit image that leaves the device: f32 (h,w,3) colour or (h,w) depth in, uint8
 * (h,w,3) with a row pitch out, and optionally the exact sum of squared 8-bit differences against a resident ground truth,
 * as one kernel launch.  What the reference renderer does per frame with three torch kernels on the f32 image
 * (torch.clamp(image * 255, 0, 255).byte()) before a copy four times the size.
 *
 *   gs_frame_to_u8(ctx, image, GS_FRAME_RGB_TRUNC, h, w, out, pitch, gt, 3, gt_pitch, sse, stream);
 *
 * Same library, same rules as gs_rasterizer.h: status codes, gs_last_error(), the call's stream last.  Not part of
 * GS_ABI_VERSION's function list.
 *
 * What is computed, per output byte, in f32 with every operation rounded on its own (no contraction):
 *  - GS_FRAME_RGB_TRUNC   (uint8)min(max(v * 255.0f, 0), 255): torch.clamp(image * 255, 0, 255).byte(), bit for bit for every
 *                         input that is not NaN (+-inf and denormals included); NaN gives 0.
 *  - GS_FRAME_RGB_ROUND   (uint8)min(max(floorf(v * 255.0f + 0.5f), 0), 255): for images that were resized in f32 from bytes.
 *  - GS_FRAME_DEPTH_CMAP  src is an (h,w) depth d; the pixel's three values are
 *                             1.0f - min(max(d, 0), 10) / 10.0f,   1.0f - min(max(d - 10.0f, 0), 50) / 50.0f,
 *                             1.0f - min(max(d - 60.0f, 0), 200) / 200.0f          (true divisions),
 *                         the reference trainer's _easy_cmap, then GS_FRAME_RGB_TRUNC.
 *  - with gt and sse given: *sse += sum over the frame of (out - gt)^2, out and gt as integers.  A term is at most 65025 and
 *    a workgroup's sum fits 32 bits, so the sum is exact and independent of order: one 64-bit integer atomic per workgroup.
 *    The caller zeroes the word.
 *
 * How (csrc/k_frames.hip): a thread owns 16 consecutive bytes of an output row: four 16-byte loads, one 16-byte store (scalar
 * loads and byte stores where the sizes, the pitch or the pointers do not allow it, and at the end of a row).  Any h, w >= 0,
 * any pitch >= 3 w.  The call does NOT synchronise with the host and allocates nothing.
 */
#ifndef GS_FRAMES_H
#define GS_FRAMES_H
#include "gs_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mode */
#define GS_FRAME_RGB_TRUNC 0
#define GS_FRAME_RGB_ROUND 1
#define GS_FRAME_DEPTH_CMAP 2

#define GS_FRAME_MAX_SIZE 32768
#define GS_FRAME_BYTES_PER_THREAD 16

/* src: device memory, f32 (h,w,3) contiguous (the RGB modes) or f32 (h,w) contiguous (GS_FRAME_DEPTH_CMAP).  dst: device
 * memory, uint8, row r at dst + r * dst_row_pitch_bytes, 3 w bytes of it written.  gt (may be NULL: no sum): device memory,
 * uint8 (>= h, >= w, gt_channels) with rows gt_row_pitch_bytes apart, of which the top-left h x w and channels 0..2 are read;
 * sse: one int64 in device memory.
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx NULL; an unknown mode; h or w negative or above
 * GS_FRAME_MAX_SIZE; dst_row_pitch_bytes < 3 w; with gt: gt_channels not 3 or 4, gt_row_pitch_bytes < w * gt_channels, sse
 * NULL; sse without gt; with h > 0 and w > 0 also: src or dst NULL.  h == 0 or w == 0 is GS_OK with no launch. */
int gs_frame_to_u8(gs_ctx* ctx, const float* src, int32_t mode, int32_t h, int32_t w, uint8_t* dst, int64_t dst_row_pitch_bytes,
                   const uint8_t* gt, int32_t gt_channels, int64_t gt_row_pitch_bytes, int64_t* sse, gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
