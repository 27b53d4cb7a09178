/* gs_appearance.h -- per-view exposure compensation: a 3x4 affine colour transform applied to a rendered image in front of
 * the loss, its gradient to the image and to the transform, and the normal equations of the least-squares affine map from a
 * rendering to its ground truth (the "colour-corrected" metrics of the NeRF-W / Mip-NeRF 360 protocol).
 *
 *   gs_appearance_apply   (ctx, &image, transform, H, W, &corrected, stream);                       // before the loss
 *   gs_appearance_backward(ctx, &image, &grad_corrected, transform, H, W, &grad_image, grad_transform, stream);
 *   gs_appearance_moments (ctx, &image, &target, pixel_weight_or_NULL, H, W, moments, stream);     // validation: the fit
 *
 * Same library, same rules as gs_rasterizer.h: status codes, gs_last_error(), the call's stream last.  Not part of
 * GS_ABI_VERSION's function list.  No call synchronises with the host or allocates caller-visible memory; the host never
 * reads the data.  No float atomic anywhere: every output is bit-reproducible.  Every f32 and f64 operation below is rounded
 * on its own (no contraction), in the order the parentheses give.  (csrc/k_appearance.hip)
 *
 * ---- images and transforms ----
 * An image is a gs_loss_image: base pointer and the strides, in floats, of (channel, row, column); three channels of H x W
 * f32 on the device.  The rasteriser's (H,W,3) output is {1, 3W, 3} and is read where it lies.  A transform is 12 floats of
 * device memory, row-major M = [A | b] (3x4): M[4 i + j] = A_ij for j < 3, M[4 i + 3] = b_i.  The pointer may point into a
 * row of a (V,12) table.  x_j(p) is channel j of `image` at pixel p, the pixels numbered p = y W + x.
 *
 * ---- gs_appearance_apply ----
 *   c_i(p) = ((A_i0 * x_0 + A_i1 * x_1) + A_i2 * x_2) + b_i                     in f32, for i = 0, 1, 2
 * corrected has its own strides.  In place (corrected->data == image->data with the same strides) is allowed; any other
 * overlap of the two is not.
 *
 * ---- gs_appearance_backward ----
 * g_i(p) is channel i of grad_corrected.  A pixel is SELECTED when at least one of g_0, g_1, g_2 is not exactly 0 (-0 is 0,
 * a NaN is not 0).
 *   grad_image_j(p)      = (A_0j * g_0 + A_1j * g_1) + A_2j * g_2               in f32 for a selected pixel; exactly +0 otherwise
 *   grad_transform[4i+j] = sum over the selected p of g_i(p) * x_j(p)           (j < 3)
 *   grad_transform[4i+3] = sum over the selected p of g_i(p)
 * Selection, not multiplication: a pixel that is not selected adds nothing to any sum whatever x holds there, NaN and inf
 * included -- the rule of gs_loss_weighted.h, whose gradient is exactly 0 under a mask.  The 12 floats are written, not added.
 * The sums: each product g_i * x_j is rounded to f32; a block of GS_APPEARANCE_PIXELS_PER_BLOCK consecutive pixels adds its
 * terms in f32 in a fixed order (per thread, then a butterfly over the wave, then the four waves in order) inside the pass
 * that moves the image; GS_APPEARANCE_FINISH_BLOCKS_BACKWARD blocks of GS_APPEARANCE_FINISH_THREADS threads, one per
 * output, add the per-block sums in float64 in a fixed order (thread t takes the blocks t, t + threads, ...) and round once
 * to f32.  The same values give the same bits on every run and in every layout: which pixel goes to which thread does not
 * depend on the strides.
 * grad_image may be NULL (the transform's gradient only), grad_transform may be NULL (the image's only; `image` is then not
 * read); not both.  grad_image may be grad_corrected itself (same strides).
 *
 * ---- gs_appearance_moments ----
 * y_i(p) is channel i of `target`; w(p) = pixel_weight[p] if that is > 0, else 0 (a negative or NaN weight counts as 0, by
 * one comparison on the device); a NULL pixel_weight is w = 1.  pixel_weight is a contiguous (H,W) f32 plane.  Weight zero
 * selects: a pixel with w = 0 adds nothing, whatever x and y hold there.  With u = (x_0, x_1, x_2, 1), all in float64:
 *   moments[0..9]      = sum_p (w u_i) u_j   for (i,j) = 00 01 02 03 11 12 13 22 23 33      (the upper triangle of sum w u u^T)
 *   moments[10 + 4i+j] = sum_p y_i (w u_j)   for i < 3, j < 4
 *   moments[22]        = sum_p w
 * 23 float64 values of device memory, written, not added.  Each thread adds its pixels in float64, the block and the
 * finishing blocks (GS_APPEARANCE_FINISH_BLOCKS_MOMENTS of them) as for the backward, all in float64.  No selected pixel
 * gives 23 zeros.  These are the normal equations of min_M sum_p w |M u - y|^2:  (sum w u u^T) M_i^T = sum w y_i u.
 *
 * ---- layouts ----
 * The two dense layouts are treated as a flat run of pixels, each lane moving four consecutive pixels through 16-byte loads
 * and stores: interleaved {1, 3W, 3} with a 16-byte aligned base, and planar contiguous {H W, W, 1} with a 16-byte aligned base
 * and W % 4 == 0.  Every other set of strides (a crop of a larger buffer, an unaligned base) takes a scalar path.  The layouts
 * of the images of one call need not agree, and no result depends on them.
 *
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx NULL; an image struct or its data NULL (the backward's grad_image alone
 * may be); transform NULL; target or moments NULL; moments not 8-byte aligned; H or W below 1, or more than
 * GS_APPEARANCE_MAX_PIXELS pixels; both outputs of the backward NULL.
 */
#ifndef GS_APPEARANCE_H
#define GS_APPEARANCE_H
#include "gs_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_APPEARANCE_PIXELS_PER_BLOCK 1024         /* pixels of one block of the image passes: 256 threads x 4 */
#define GS_APPEARANCE_FINISH_THREADS 256            /* threads of a finishing block: it loops past this many per-block sums */
#define GS_APPEARANCE_FINISH_BLOCKS_BACKWARD 12     /* finishing blocks of gs_appearance_backward: one per output */
#define GS_APPEARANCE_FINISH_BLOCKS_MOMENTS 23      /* finishing blocks of gs_appearance_moments: one per output */
#define GS_APPEARANCE_TRANSFORM_FLOATS 12
#define GS_APPEARANCE_MOMENTS 23
#define GS_APPEARANCE_MAX_PIXELS 2147481600         /* 2^31 - 2048: a pixel index and its block's end fit int32 */

int gs_appearance_apply(gs_ctx* ctx, const gs_loss_image* image, const float* transform, int32_t H, int32_t W,
                        const gs_loss_image* corrected, gs_stream stream);

int gs_appearance_backward(gs_ctx* ctx, const gs_loss_image* image, const gs_loss_image* grad_corrected, const float* transform,
                           int32_t H, int32_t W, const gs_loss_image* grad_image, float* grad_transform, gs_stream stream);

int gs_appearance_moments(gs_ctx* ctx, const gs_loss_image* image, const gs_loss_image* target, const float* pixel_weight,
                          int32_t H, int32_t W, double* moments, gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
