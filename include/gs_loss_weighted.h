/* gs_loss_weighted.h -- the fused L1 + SSIM loss of gs_rasterizer.h with a weight per pixel: masked training (moving
 * objects, sky, an RGBA capture's alpha as the foreground mask), forward and gradient in the same three launches.
 *
 *   gs_loss_l1_ssim_weighted_forward (ctx, pred, gt, weight, H, W, clamp, lambda, maps, terms, stream);
 *   gs_loss_l1_ssim_weighted_backward(ctx, pred, gt, weight, H, W, clamp, lambda, maps, terms, upstream, grad, stream);
 *
 * Same library, same rules as gs_rasterizer.h: status codes, gs_last_error(), the call's stream last.  Not part of
 * GS_ABI_VERSION's function list.
 *
 * What is computed.  w(p) = pixel_weight[p] if that is > 0, else 0: a negative or NaN weight counts as 0, by one comparison
 * on the device; the host never looks at the data.  With x = predicted (clamped to [0, 1] first if clamp_predicted),
 * y = ground_truth and s_c(q) the SSIM map gs_loss_l1_ssim_forward computes (11-tap Gaussian window, sigma 1.5, "valid"
 * filtering: (H - 10) x (W - 10) window positions q):
 *     S_w    = sum_p w(p)                                   over the H x W pixels
 *     L1_w   = sum_c sum_p w(p) |x_c(p) - y_c(p)| / (3 S_w)
 *     v(q)   = w(q_y + 5, q_x + 5)                          a window counts with the weight of its centre pixel
 *     V      = sum_q v(q)
 *     SSIM_w = sum_c sum_q v(q) s_c(q) / (3 V)
 *     L      = (1 - lambda) L1_w + lambda (1 - SSIM_w)
 *     loss_terms[5] = { L, L1_w, 1 - SSIM_w, S_w, V }
 *  - S_w == 0: the L1 term and its gradient are exactly 0.  V == 0: the SSIM term (loss_terms[2]) and its gradient are
 *    exactly 0.  An empty mask gives { 0, 0, 0, 0, 0 } and a gradient of zeros; nothing is NaN.
 *  - Weight zero selects, it does not multiply: a pixel with w = 0 adds nothing to the L1 sum whatever it holds, a window
 *    with v = 0 adds nothing to the SSIM sum and leaves exact zeros in the derivative maps.  A pixel with w = 0 that lies in
 *    no window with v > 0 (none within 5 pixels of a positive weight) affects no term and gets a gradient of exactly 0,
 *    even if it holds NaN or inf.  (A masked pixel inside a weighted window is still read by that window's SSIM.)
 *  - The weights are not differentiated.  No float atomics: per-block partial sums, added in float64 in a fixed order; the
 *    same inputs give the same bits.
 *
 * Arguments.  predicted, ground_truth, grad_predicted: gs_loss_image, any strides, as for gs_loss_l1_ssim_forward /
 * _backward.  pixel_weight: device memory, f32 (H, W) contiguous, shared by the three channels (rows that start on 16-byte
 * boundaries -- W % 4 == 0 and an aligned base -- are the fast case).  maps: gs_loss_maps_floats(H, W) floats of device
 * memory, written by the forward (already multiplied by v) and read by the backward.  loss_terms: five floats of device
 * memory, written by the forward; the backward reads S_w and V from it on the device (no host synchronisation).  upstream:
 * one float of device memory (dL_total / dL), or NULL for 1.
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx, pixel_weight, maps, loss_terms, an image or its data NULL
 * (the backward: grad_predicted too); H or W below 11.
 */
#ifndef GS_LOSS_WEIGHTED_H
#define GS_LOSS_WEIGHTED_H
#include "gs_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

int gs_loss_l1_ssim_weighted_forward(gs_ctx* ctx, const gs_loss_image* predicted, const gs_loss_image* ground_truth,
                                     const float* pixel_weight, int32_t H, int32_t W, int32_t clamp_predicted, float lambda_value,
                                     float* maps, float* loss_terms, gs_stream stream);

int gs_loss_l1_ssim_weighted_backward(gs_ctx* ctx, const gs_loss_image* predicted, const gs_loss_image* ground_truth,
                                      const float* pixel_weight, int32_t H, int32_t W, int32_t clamp_predicted, float lambda_value,
                                      const float* maps, const float* loss_terms, const float* upstream,
                                      const gs_loss_image* grad_predicted, gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
