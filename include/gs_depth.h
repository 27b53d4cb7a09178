/* gs_depth.h -- depth supervision: the depth target of one view made on the device from a resident depth map, with a validity
 * weight, and a fused masked depth loss on the rasteriser's depth output with its gradient.
 *
 *   gs_depth_resample     (ctx, src, GS_DEPTH_U16, H, W, pitch, 0.001f, H / f, W / f, h, w, 0.5f, dst, stream);   // dst (2,h,w)
 *   gs_depth_loss_forward (ctx, D, dst, dst + h * w, pixel_weight_or_NULL, h, w, flags, loss_terms, stream);
 *   gs_depth_loss_backward(ctx, D, dst, dst + h * w, pixel_weight_or_NULL, h, w, flags, loss_terms, upstream_or_NULL, grad_D, stream);
 *
 * Same library, same rules as gs_rasterizer.h: status codes, gs_last_error(), the call's stream last.  Not part of
 * GS_ABI_VERSION's function list.  No call synchronises with the host or allocates caller-visible memory; the host never
 * reads the data.  No float atomic anywhere: the same inputs give the same bits on every run.  Every f32 and f64 operation
 * below is rounded on its own (no contraction) unless it is written fmaf, in the order the parentheses give; every division
 * is correctly rounded.  (csrc/k_depth.hip)
 *
 * ---- gs_depth_resample ----
 * The depth target of one view at a downsample factor: the geometry, taps and weights of gs_image_resample (gs_targets.h: the
 * ATen antialias triangle filter for down-scaling, tables made in float64 on the host, cached in the context -- the same cache,
 * a geometry seen by either call is known to both), applied to a depth map WITH HOLES.
 *   source   GS_DEPTH_U16: uint16 (H_in, W_in), rows src_row_pitch_bytes apart, any pitch >= 2 W_in and any alignment (16-byte
 *            aligned rows are the fast case).  A sample v is VALID iff v != 0, and is z = (float)v * depth_scale (one f32 multiply).
 *            GS_DEPTH_F32: contiguous f32 (H_in, W_in), src_row_pitch_bytes == 4 W_in.  A sample z is valid iff z > 0 and
 *            z <= FLT_MAX, by comparison on the device (a NaN, an inf, zero and anything negative are holes); depth_scale is
 *            checked and not used.
 *   filter   With k the tap weights and the sums over VALID samples only (an invalid sample is selected out: whatever it holds
 *            reaches nothing), horizontal pass per input row, a chain in ascending input column j starting from 0:
 *                n = fmaf(k_j, z_j, n),  d = d + k_j
 *            then the vertical pass per output pixel, a chain in ascending input row i starting from 0:
 *                num = fmaf(k_i, n_i, num),  den = fmaf(k_i, d_i, den)
 *   output   dst is f32 (2, h_out, w_out) contiguous, the top-left crop of the (h_full, w_full) resize; only the crop is computed.
 *            Plane 1 (weight) = den if den > 0 && den >= min_coverage, else exactly +0.
 *            Plane 0 (depth)  = num / den where the weight is not 0, else exactly +0.
 *            Equal sizes are the identity, bit for bit: z and a weight of 1, or 0 and 0 at a hole.  (den is an f32 sum of f32
 *            weights: at a non-integer scale a window without a hole may come out one ulp below 1, so min_coverage = 1 is
 *            exact only at equal sizes; use a value a little below 1 to mean "no hole under the filter".)
 * A depth map is never interpolated across a hole: the mean is over the valid samples under the filter, and the weight is the
 * share of the filter they cover -- fractional at a hole's border, which down-weights mixed pixels (the rule by which the
 * mask of gs_image_resample_rgba comes out soft).  One launch; the first call of a geometry also uploads its tables.
 *
 * ---- gs_depth_loss_forward / gs_depth_loss_backward ----
 * D (rendered depth), Z (target), w_t (the target's weight plane) and the optional w_p (a second weight plane: the loss's
 * pixel_weight; NULL: 1) are contiguous f32 (H, W) planes on the device; pixels are numbered p = y W + x.
 *   selection  a = w_t > 0 ? w_t : 0, b likewise from w_p (1 without it), w = a * b (one f32 multiply).  Pixel p is SELECTED iff
 *              w > 0, and Z > 0 && Z <= FLT_MAX, and D > 0 && D <= FLT_MAX (an empty pixel renders D = 0 and is not selected; a
 *              negative or NaN weight counts as 0).  Selection, not multiplication: a pixel that is not selected adds nothing
 *              to any sum, whatever it holds, and gets a gradient of exactly +0.
 *   space      From here on everything is float64 on the f32 inputs (the passes are bound by memory, not by arithmetic): x = 1 / D
 *              with GS_DEPTH_INVERT_PREDICTED, else x = D.  y = 1 / Z with GS_DEPTH_INVERT_TARGET, else y = Z.
 *   alignment  Without GS_DEPTH_ALIGN s = 1, t = 0.  With it (s, t) = argmin sum w (s y + t - x)^2 over the selected pixels,
 *              from five float64 moments, each product rounded on its own:
 *                  S_w = sum w,  S_y = sum w y,  S_x = sum w x,  S_yy = sum (w y) y,  S_xy = sum (w y) x
 *              det = S_w S_yy - S_y S_y.  If !(det > 1e-12 (S_w S_yy)) -- a constant target, a single pixel --:
 *                  s = 0, t = S_x / S_w
 *              else s = (S_w S_xy - S_y S_x) / det,  t = (S_x - s S_y) / S_w  (s not yet rounded), all in float64; then s and t
 *              are rounded once to f32.
 *   residual   r = x - (s * y + t) in float64, s and t the rounded f32 values.  rho(r) = |r|, or r * r with GS_DEPTH_L2.
 *   loss       L = (sum w * rho) / S_w in float64, rounded once to f32; so are S_w and the number of selected pixels.
 *   loss_terms 8 floats of device memory, written: { L, S_w, s, t, number of selected pixels, 0, 0, 0 }.  No selected pixel:
 *              eight zeros (s and t too), and every gradient is +0; nothing is NaN.
 *   sums       a block of GS_DEPTH_PIXELS_PER_BLOCK consecutive pixels (256 threads, thread i the pixels 4 i .. 4 i + 3 of the
 *              block) adds in float64 in a fixed order: each thread its pixels in ascending order, a butterfly over the wave (xor
 *              32, 16, ..., 1), the four waves in order; then one finishing block per sum, GS_DEPTH_FINISH_THREADS threads, thread
 *              i adding the per-block sums i, i + threads, ... and the same butterfly and wave order.  Which pixel belongs to
 *              which thread does not depend on the alignment of any plane: a 16-byte aligned plane is moved four pixels per
 *              lane, any other one pixel by pixel, with equal bits.
 *   launches   forward: GS_DEPTH_FORWARD_LAUNCHES (2: residual pass, finish) without GS_DEPTH_ALIGN,
 *              GS_DEPTH_FORWARD_LAUNCHES_ALIGN (4: moments pass, finish, residual pass, finish) with it: the fit must be known
 *              before the first residual is formed.  backward: 1.
 *   backward   reads loss_terms on the device (the f32 values of S_w, s, t) and selects anew by the same rule.  With
 *              u = *upstream (NULL: 1) and c = u / S_w:   grad_D(p) = (w * rho'(r)) * c,   times -(x * x) with
 *              GS_DEPTH_INVERT_PREDICTED (dx/dD = -1/D^2 = -x^2), where rho'(r) = (r > 0) - (r < 0) for L1 (0 at 0) and 2 r for
 *              L2; in float64, rounded once to f32.  Every element of grad_D is written.
 *              s and t are HELD FIXED: the gradient does not run through the fit.  For L2 this is nevertheless the exact total derivative of L in D: (s, t) minimise the same sum that L is, so dL/ds = dL/dt = 0 there
 *              (envelope theorem; S_w does not depend on D).  For L1 the fit minimises another sum than the loss, and the
 *              result is the gradient with the fit detached, as trainers that align monocular depth by least squares use it.
 *
 * Work memory (per-block sums, a few KB) belongs to the context and is counted by gs_ctx_device_bytes.
 *
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx NULL; a NULL plane (w_p alone may be), loss_terms or grad_D;
 * H or W below 1, or more than GS_APPEARANCE_MAX_PIXELS pixels; flag bits outside GS_DEPTH_FLAGS_ALL; for the resample: an
 * unknown src_format; min_coverage outside [0, 1] or NaN; depth_scale not finite or not > 0; and the geometry errors of
 * gs_image_resample: a negative size or one above GS_RESAMPLE_MAX_SIZE, h_out > h_full or w_out > w_full, a row pitch too
 * small (or, for f32, not 4 W_in); with h_out > 0 and w_out > 0 also src or dst NULL and a scale H_in / h_full or W_in / w_full
 * outside [1, GS_RESAMPLE_MAX_SCALE].  h_out == 0 or w_out == 0 is GS_OK with no launch.
 */
#ifndef GS_DEPTH_H
#define GS_DEPTH_H
#include "gs_rasterizer.h"
#include "gs_targets.h"
#include "gs_appearance.h"

#ifdef __cplusplus
extern "C" {
#endif

/* src_format of gs_depth_resample */
#define GS_DEPTH_U16 0   /* uint16 (H_in, W_in), rows src_row_pitch_bytes apart; 0 is a hole */
#define GS_DEPTH_F32 1   /* f32 (H_in, W_in) contiguous; anything not finite and > 0 is a hole */

/* flags of the loss */
#define GS_DEPTH_INVERT_PREDICTED 1
#define GS_DEPTH_INVERT_TARGET 2
#define GS_DEPTH_L2 4
#define GS_DEPTH_ALIGN 8
#define GS_DEPTH_FLAGS_ALL 15

#define GS_DEPTH_PIXELS_PER_BLOCK 1024       /* pixels of one block of the loss passes: 256 threads x 4 */
#define GS_DEPTH_FINISH_THREADS 256          /* threads of a finishing block: it loops past this many per-block sums */
#define GS_DEPTH_MOMENTS 5                   /* S_w, S_y, S_x, S_yy, S_xy */
#define GS_DEPTH_LOSS_TERMS 8
#define GS_DEPTH_FORWARD_LAUNCHES 2
#define GS_DEPTH_FORWARD_LAUNCHES_ALIGN 4
#define GS_DEPTH_BACKWARD_LAUNCHES 1

int gs_depth_resample(gs_ctx* ctx, const void* src, int32_t src_format, int32_t H_in, int32_t W_in, int64_t src_row_pitch_bytes,
                      float depth_scale, int32_t h_full, int32_t w_full, int32_t h_out, int32_t w_out, float min_coverage,
                      float* dst, gs_stream stream);

int gs_depth_loss_forward(gs_ctx* ctx, const float* D, const float* Z, const float* w_t, const float* w_p, int32_t H, int32_t W,
                          int32_t flags, float* loss_terms, gs_stream stream);

int gs_depth_loss_backward(gs_ctx* ctx, const float* D, const float* Z, const float* w_t, const float* w_p, int32_t H, int32_t W,
                           int32_t flags, const float* loss_terms, const float* upstream, float* grad_D, gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
