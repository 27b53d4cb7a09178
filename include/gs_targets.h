/* gs_targets.h -- the training target of one view, made on the device: an antialiased bilinear down-resize of a resident
 * image and its top-left crop, as one kernel launch.  What the reference trainer does per iteration on the host (PIL decode,
 * to_tensor, torchvision resize(antialias=True), crop to a multiple of 16, .cuda()) becomes: decode once, keep the uint8
 * image on the device, and call this per step.
 *
 *   gs_image_resample(ctx, src, GS_IMAGE_U8_HWC, 3, H, W, pitch, H / f, W / f, h, w, dst, stream);   // dst (3,h,w) f32
 *
 * Same library, same rules as gs_rasterizer.h: status codes, gs_last_error(), the call's stream last.  Not part of
 * GS_ABI_VERSION's function list.
 *
 * What is computed
 *  - ATen's _upsample_bilinear2d_aa with align_corners = false (torchvision.transforms.functional.resize(antialias=True) and
 *    F.interpolate(mode="bilinear", antialias=True) on a float tensor), for down-scaling.  Per axis, with scale = in / out >= 1,
 *    support = scale and center = scale * (i + 0.5), output i reads the inputs j in [xmin, xmax),
 *        xmin = max(int(center - support + 0.5), 0),  xmax = min(int(center + support + 0.5), in)      (int() truncates),
 *    with the weights w_j = max(0, 1 - |(j - center + 0.5) / scale|) divided by their sum.  The horizontal pass runs first,
 *    then the vertical pass.
 *  - The tables (xmin, tap count, weights) are made on the host in float64, rounded once to f32, uploaded once per geometry
 *    (H_in, W_in, h_full, w_full) and cached in the context; taps of weight zero at either end of a window are dropped
 *    (equal sizes: one tap of weight 1, the identity, bit for bit).  No weight is computed in f32: in/out is inexact there.
 *  - A uint8 sample v becomes (float)v / 255.0f (true division: torchvision's to_tensor) before filtering.  Each pass is a
 *    chain of fused multiply-adds in ascending j; no atomics; the same bits on every run.
 *  - dst is the top-left (h_out, w_out) crop of the (h_full, w_full) resize; only the crop is computed and written.
 *
 * How (csrc/k_targets.hip): one launch; a workgroup owns a GS_RESAMPLE_TILE_H x GS_RESAMPLE_TILE_W output tile, walks the
 * input rows it needs in chunks (uint8 rows staged in LDS with 16-byte loads, the horizontal pass from there into LDS as
 * f32), and the vertical pass accumulates in registers from LDS and ends in 16-byte stores per channel plane.
 *
 * Work memory (the tables, a few KB per geometry; at most GS_RESAMPLE_MAX_GEOMETRIES are kept, the oldest goes first) belongs
 * to the context and is counted by gs_ctx_device_bytes.  The call does NOT synchronise with the host; the first call of a
 * geometry allocates and uploads its tables, every later one only launches.
 */
#ifndef GS_TARGETS_H
#define GS_TARGETS_H
#include "gs_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* src_format */
#define GS_IMAGE_U8_HWC 0   /* uint8 (H_in, W_in, src_channels), rows src_row_pitch_bytes apart */
#define GS_IMAGE_F32_CHW 1  /* f32 (src_channels, H_in, W_in) contiguous */

/* the output tile of one workgroup (rows x columns) and the bounds of a call */
#define GS_RESAMPLE_TILE_H 16
#define GS_RESAMPLE_TILE_W 64
#define GS_RESAMPLE_MAX_SCALE 8
#define GS_RESAMPLE_MAX_SIZE 32768
#define GS_RESAMPLE_MAX_GEOMETRIES 32

/* src: device memory in src_format; src_channels 3 or 4 (only channels 0..2 are read).  GS_IMAGE_U8_HWC: any
 * src_row_pitch_bytes >= W_in * src_channels, any alignment (16-byte aligned rows are the fast case).  GS_IMAGE_F32_CHW:
 * src_row_pitch_bytes must be W_in * 4.  dst: device memory, f32 (3, h_out, w_out) contiguous.
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx NULL; an unknown src_format; src_channels not 3 or 4; a
 * negative size or one above GS_RESAMPLE_MAX_SIZE; h_out > h_full or w_out > w_full; a row pitch too small (or, for f32,
 * not W_in * 4); with h_out > 0 and w_out > 0 also: src or dst NULL, and a scale H_in / h_full or W_in / w_full outside
 * [1, GS_RESAMPLE_MAX_SCALE].  h_out == 0 or w_out == 0 is GS_OK with no launch. */
int gs_image_resample(gs_ctx* ctx, const void* src, int32_t src_format, int32_t src_channels, int32_t H_in, int32_t W_in,
                      int64_t src_row_pitch_bytes, int32_t h_full, int32_t w_full, int32_t h_out, int32_t w_out, float* dst,
                      gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
