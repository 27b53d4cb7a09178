/* gs_background.h -- a background behind the splats: a solid colour or a low-order, view-direction-dependent sky (real
 * spherical harmonics of up to three bands per channel, 48 floats) composited under a rendered image with the rasteriser's
 * accumulated alpha, and the gradient of that to the alpha and to the 48 coefficients.
 *
 *   gs_background_composite(ctx, &image_or_NULL, alpha, coef, bands, q, intrinsics, H, W, flags, &out, stream);
 *   gs_background_backward (ctx, &grad_out, alpha, coef, bands, q, intrinsics, H, W, grad_alpha, grad_coef, stream);
 *
 * Same library, same rules as gs_rasterizer.h: status codes, gs_last_error(), the call's stream last.  Not part of
 * GS_ABI_VERSION's function list.  No call synchronises with the host or allocates caller-visible memory; the host never
 * reads the data.  No float atomic anywhere: every output is bit-reproducible.  Every f32 and f64 operation below is rounded
 * on its own (no contraction), in the order the parentheses give; division and sqrtf are correctly rounded.
 * (csrc/k_background.hip)
 *
 * ---- images, alpha and the background ----
 * An image is a gs_loss_image: base pointer and the strides, in floats, of (channel, row, column); three channels of H x W
 * f32 on the device.  The rasteriser's (H,W,3) output is {1, 3W, 3} and is read where it lies.  `alpha` is a contiguous
 * (H,W) f32 plane, A(p), the pixels numbered p = y W + x; t(p) = 1.0f - A(p).  x_i(p) is channel i of `image` at pixel p.
 * A background is GS_BACKGROUND_COEF_FLOATS = 48 floats of device memory, coef[16 i + k] for channel i < 3.  `bands` in
 * 0 .. GS_BACKGROUND_MAX_BANDS selects K = (bands + 1)^2 of them per channel; the others are not read.  For the pixel
 * p = (x, y), in f32:
 *   a   = (((float)x + 0.5f) - cx) / fx        b = (((float)y + 0.5f) - cy) / fy
 *   n   = sqrtf((a * a + b * b) + 1.0f)
 *   dc  = (a / n, b / n, 1.0f / n)                                    the pixel centre's ray in the camera frame
 *   d_j = (R[3j] * dc_0 + R[3j+1] * dc_1) + R[3j+2] * dc_2            j = 0, 1, 2: that ray in the point-cloud frame
 *   Y   = the 16 basis values of d, as the rasteriser evaluates them for a splat's colour (same constants, same order)
 *   c_i = (..((coef[16i] + coef[16i+1] * Y_1) + coef[16i+2] * Y_2) ..) + coef[16i+K-1] * Y_{K-1}
 * fx = K[0], cx = K[2], fy = K[4], cy = K[5] of `intrinsics`, 9 floats of device memory, the row-major (3,3) camera matrix;
 * pixel centres are at +0.5, as in gs_geometry.h.  R is the row-major rotation matrix of the quaternion `q`, 4 floats of
 * device memory xyzw, NOT normalised, by the formula the rasteriser uses.  q is a row of the rasteriser's
 * q_pointcloud_camera: the pose of the camera in the point-cloud frame, which takes camera coordinates to point-cloud
 * coordinates.  The rasteriser inverts that pose to project points; the sky goes the other way and uses it as it is given.
 * The constant term is taken WITHOUT Y_0, so coef = (1, 0, ..., 0) per channel is exactly white; there is no activation and
 * no clamp.  With bands == 0, c_i = coef[16 i]: no direction is computed, and q and intrinsics are not read and may be NULL.
 *
 * ---- gs_background_composite ----
 *   premultiplied (flags == 0; `image` is the rasteriser's):     out_i = x_i + t * c_i
 *   GS_BACKGROUND_STRAIGHT (`image` is a decoded RGBA's colour): out_i = x_i * A + t * c_i
 *   GS_BACKGROUND_COLOURS_ONLY:                                  out_i = c_i       image and alpha are not read, may be NULL
 * `out` has its own strides.  In place (out->data == image->data with the same strides) is allowed; any other overlap of
 * the two is not.
 *
 * ---- gs_background_backward ----
 * The premultiplied mode only.  The image's gradient is grad_out itself, so the call does not write it.  g_i(p) is channel
 * i of grad_out.  A pixel is SELECTED when at least one of g_0, g_1, g_2 is not exactly 0 (-0 is 0, a NaN is not 0).
 *   grad_alpha(p)        = -((g_0 * c_0 + g_1 * c_1) + g_2 * c_2)          in f32 for a selected pixel; exactly +0 otherwise
 *   grad_coef[16 i + k]  = sum over the selected p of (g_i * t) * Y_k       for k < K, with Y_0 := 1 (the term is g_i * t)
 *   grad_coef[16 i + k]  = +0                                               for K <= k < 16
 * Selection, not multiplication: a pixel that is not selected adds nothing to any sum whatever alpha holds there, NaN and
 * inf included.  grad_alpha is a contiguous (H,W) f32 plane; the 48 floats of grad_coef are written, not added.
 * The sums: each term is rounded to f32 as written.  A block owns GS_BACKGROUND_PIXELS_PER_BLOCK consecutive pixels, thread
 * u of block b the four pixels 4 (256 b + u) ..., and adds its terms in f32 in a fixed order inside the pass that reads
 * grad_out: per thread over its four pixels in ascending order starting from +0, then over the 64 lanes of a wave as a
 * butterfly (v_l <- v_l + v_{l ^ 32}, then ^ 16, 8, 4, 2, 1), then the four waves in order.  GS_BACKGROUND_FINISH_BLOCKS
 * blocks of GS_BACKGROUND_FINISH_THREADS threads, one per output, add the per-block sums in float64 in a fixed order (thread
 * u takes the blocks u, u + threads, ... in ascending order from 0, then the same butterfly and the waves in order) and round
 * once to f32.  The same values give the same bits on every run and in every layout: which pixel goes to which thread does
 * not depend on the strides.
 * grad_alpha may be NULL (the coefficients' gradient only), grad_coef may be NULL (a fixed colour: no workspace is taken and
 * no finishing kernel runs); not both.
 *
 * ---- layouts ----
 * The two dense layouts are treated as a flat run of pixels, each lane moving four consecutive pixels through 16-byte loads
 * and stores: interleaved {1, 3W, 3} with a 16-byte aligned base, and planar contiguous {H W, W, 1} with a 16-byte aligned base
 * and W % 4 == 0.  Every other set of strides (a crop of a larger buffer, an unaligned base) takes a scalar path; so does a
 * plane (alpha, grad_alpha) whose base is not 16-byte aligned.  The layouts of the images of one call need not agree, and no
 * result depends on them.
 *
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx NULL; an image struct or its data NULL (the composite's
 * `image` may be under GS_BACKGROUND_COLOURS_ONLY, and only then); alpha NULL (except under GS_BACKGROUND_COLOURS_ONLY); coef
 * NULL; bands outside 0 .. GS_BACKGROUND_MAX_BANDS; bands > 0 with q or intrinsics NULL; a flag bit that is not defined, or
 * GS_BACKGROUND_STRAIGHT together with GS_BACKGROUND_COLOURS_ONLY; H or W below 1, or more than GS_BACKGROUND_MAX_PIXELS
 * pixels; both outputs of the backward NULL.
 */
#ifndef GS_BACKGROUND_H
#define GS_BACKGROUND_H
#include "gs_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_BACKGROUND_PIXELS_PER_BLOCK 1024         /* pixels of one block of the image passes: 256 threads x 4 */
#define GS_BACKGROUND_FINISH_THREADS 256            /* threads of a finishing block: it loops past this many per-block sums */
#define GS_BACKGROUND_FINISH_BLOCKS 48              /* finishing blocks of gs_background_backward: one per output */
#define GS_BACKGROUND_COEF_FLOATS 48                /* 3 channels x 16 */
#define GS_BACKGROUND_MAX_BANDS 3
#define GS_BACKGROUND_MAX_PIXELS 2147481600         /* 2^31 - 2048: a pixel index and its block's end fit int32 */

#define GS_BACKGROUND_STRAIGHT 1                    /* flags: `image` is not premultiplied by alpha */
#define GS_BACKGROUND_COLOURS_ONLY 2                /* flags: write the background's colours alone */

int gs_background_composite(gs_ctx* ctx, const gs_loss_image* image, const float* alpha, const float* coef, int32_t bands,
                            const float* q, const float* intrinsics, int32_t H, int32_t W, int32_t flags,
                            const gs_loss_image* out, gs_stream stream);

int gs_background_backward(gs_ctx* ctx, const gs_loss_image* grad_out, const float* alpha, const float* coef, int32_t bands,
                           const float* q, const float* intrinsics, int32_t H, int32_t W, float* grad_alpha, float* grad_coef,
                           gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
