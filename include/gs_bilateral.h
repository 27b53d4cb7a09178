/* gs_bilateral.h -- per-view bilateral grids: a spatially varying 3x4 affine colour transform of a rendered image in front of
 * the loss ("Bilateral Guided Radiance Field Processing", Wang et al., SIGGRAPH 2024; gsplat's use_bilateral_grid), its
 * gradient to the image and to the grid, and the total-variation regulariser of a grid.
 *
 *   gs_bilateral_slice         (ctx, &image, grid, Gx, Gy, L, H, W, &corrected, stream);                  // before the loss
 *   gs_bilateral_slice_backward(ctx, &image, &grad_corrected, grid, Gx, Gy, L, H, W, &grad_image, grad_grid, stream);
 *   gs_bilateral_tv            (ctx, grid, Gx, Gy, L, weight, grad_grid, value, stream);                  // after the backward
 *
 * Same library, same rules as gs_appearance.h: status codes, gs_last_error(), the call's stream last.  Not part of
 * GS_ABI_VERSION's function list.  No call synchronises with the host or allocates caller-visible memory; the host never
 * reads the data.  No float atomic anywhere: every output is bit-reproducible and independent of the images' strides.  Every
 * f32 and f64 operation below is rounded on its own (no contraction), in the order the parentheses give.  Where a term is
 * left out it is SELECTED out, never multiplied by 0.  (csrc/k_bilateral.hip)
 *
 * ---- images and grids ----
 * An image is a gs_loss_image: three channels of H x W f32 on the device under arbitrary strides; x_j(p) is channel j of
 * `image` at pixel p = (x, y).  Every pixel is addressed through the strides, one pixel per thread: no layout is special.
 * A grid is Gy x Gx x L vertices of 12 floats, f32 on the device, contiguous in the order (iy, ix, l, 12):
 *   vertex (iy, ix, l) begins at float 12 * ((iy * Gx + ix) * L + l)
 * so the L levels of one image-plane vertex are one run of 12 L floats.  The 12 floats of a vertex are a row-major
 * M = [A | b] as in gs_appearance.h.  The grid pointer must be 16-byte aligned (every vertex then is).
 * 2 <= Gx, Gy <= GS_BILATERAL_MAX_XY, 2 <= L <= GS_BILATERAL_MAX_L.
 *
 * ---- coordinates (align-corners), all f32 ----
 *   sx = W > 1 ? (float)(Gx - 1) / (float)(W - 1) : 0        sy likewise from Gy, H        (formed once, on the host)
 *   gx = (float)x * sx        ix0 = min((int)gx, Gx - 2)      tx = gx - (float)ix0           gy, iy0, ty likewise
 *   lum = (0.299f * x_0 + 0.587f * x_1) + 0.114f * x_2                                       (from the INPUT image)
 *   lc  = lum > 0 ? (lum < 1 ? lum : 1) : 0                  (a NaN fails lum > 0: level 0 with tz = 0)
 *   gz  = lc * (float)(L - 1) iz0 = min((int)gz, L - 2)       tz = gz - (float)iz0
 * gx = Gx - 1 is valid with tx = 1.  `inside` is lum > 0 && lum < 1.
 *
 * ---- the interpolated transform ----
 * lerp(a, b, t) = a + t * (b - a).  For each of the 12 coefficients k and the level l in {iz0, iz0 + 1}
 *   P_l[k] = lerp(lerp(v(iy0, ix0, l), v(iy0, ix0+1, l), tx), lerp(v(iy0+1, ix0, l), v(iy0+1, ix0+1, l), tx), ty)
 *   dM[k]  = P_{iz0+1}[k] - P_{iz0}[k]                       M[k] = P_{iz0}[k] + tz * dM[k]
 * (x, then y, then z.)  A constant grid gives exactly its transform.
 *
 * ---- gs_bilateral_slice ----
 *   c_i(p) = ((M_i0 * x_0 + M_i1 * x_1) + M_i2 * x_2) + M_i3
 * corrected has its own strides.  In place (corrected->data == image->data with the same strides) is allowed; any other
 * overlap is not.
 *
 * ---- gs_bilateral_slice_backward ----
 * g_i(p) is channel i of grad_corrected.  A pixel is SELECTED when at least one of g_0, g_1, g_2 is not exactly 0 (-0 is 0,
 * a NaN is not 0).  A pixel that is not selected gets a gradient of exactly +0 and adds nothing to any sum, whatever the
 * image holds there.  For a selected pixel, with u = (x_0, x_1, x_2, 1):
 *   a_j = (M_0j * g_0 + M_1j * g_1) + M_2j * g_2
 *   D_i = ((dM_i0 * x_0 + dM_i1 * x_1) + dM_i2 * x_2) + dM_i3           S = (g_0 * D_0 + g_1 * D_1) + g_2 * D_2
 *   grad_image_j = inside ? a_j + ((float)(L - 1) * c_j) * S : a_j       c = (0.299f, 0.587f, 0.114f)
 * the second term being the derivative through the luminance guide.
 *
 *   grad_grid[vertex (iy, ix, l)][4 i + j] = sum over the selected p that reach the vertex of ((wx * wy) * wz) * g_i * u_j
 * rounded as   w = (wx * wy) * wz;  a = w * g_i;  term = j < 3 ? a * x_j : a.   A pixel reaches the vertices of its cell only:
 *   wx = 1 - tx for ix == ix0, tx for ix == ix0 + 1;  wy likewise;  wz = 1 - tz for l == iz0, tz for l == iz0 + 1.
 * The floats are written, not added; a vertex no pixel reaches gets exact +0.
 *
 * The sum is a gather.  The pixels of column cell c are the run xs[c] <= x < xs[c+1], where xs[c] is the first x with
 * ix0(x) >= c (xs[0] = 0, xs[Gx-1] = W; found on the host with the f32 expression above), rows likewise.  Image-plane vertex
 * (iy, ix) owns the rectangle FOOTPRINT = [xs[max(ix-1,0)], xs[min(ix+1,Gx-1)]) x [ys[max(iy-1,0)], ys[min(iy+1,Gy-1)]).
 * Its rows are split over S = max(1, GS_BILATERAL_TARGET_BLOCKS / (Gx Gy)) blocks (integer division): with
 * R = ceil(rows / S), block s takes the rows [s R, min((s+1) R, rows)) of the footprint.  A block of
 * GS_BILATERAL_GATHER_THREADS threads numbers the pixels of its rows row-major, q = 0, 1, ...; thread t adds the terms of the
 * pixels q = t, t + threads, ... in that order into 12 L f32 sums that start at +0 (all L levels of the vertex at once; a
 * level the pixel does not reach is left alone).  Then a butterfly over the wave (v += lane ^ 32, ^ 16, ... ^ 1: every lane
 * ends with the same bits), then the waves in order ((w0 + w1) + w2) + w3, all f32.  Where S > 1 the S block sums of an
 * output are added in float64 in the order s = 0, 1, ... starting from 0.0 and rounded once to f32; with S = 1 the block's
 * sum is the output.  Which pixel goes to which thread depends on H, W, Gx, Gy alone.
 * grad_image may be NULL (the grid's gradient only), grad_grid may be NULL; not both.  grad_image may be grad_corrected
 * itself (same strides).  grad_grid is Gy Gx L 12 floats laid out as the grid; it must not overlap the grid.
 *
 * ---- gs_bilateral_tv ----
 * gsplat's total_variation_loss of one grid.  With n = 12 Gy Gx L values v, and for each axis a in (x, y, z) the
 * count_a = 12 * (number of neighbouring vertex pairs along a), d_a(e) = v(next along a) - v(e) in f32:
 *   T_a   = sum in float64 over the values e that have a next along a, of (double)d_a(e) * (double)d_a(e)
 *   value = (float)((T_x / count_x + T_y / count_y) + T_z / count_z)
 * One block of GS_BILATERAL_TV_THREADS threads: thread t adds the values e = t, t + threads, ... (e the float index into the
 * grid) in float64, then the butterfly and the waves in order as above, in float64.  `value` is one f32 of device memory,
 * written.  With grad_grid given, for every value e, in f32:
 *   r_a = 2.0f / (float)count_a                                           (formed on the host)
 *   q_a = (e has a previous along a ? v(e) - v(previous) : 0) - (e has a next along a ? v(next) - v(e) : 0)
 *   grad_grid[e] = grad_grid[e] + weight * ((r_x * q_x + r_y * q_y) + r_z * q_z)
 * that is weight * d tv / d grid ADDED in place.  One launch.
 *
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx NULL; an image struct or its data NULL (the backward's
 * grad_image alone may be); grid NULL or not 16-byte aligned; value NULL; H or W below 1, or more than
 * GS_BILATERAL_MAX_PIXELS pixels; Gx, Gy or L outside their limits; both outputs of the backward NULL; weight not finite.
 */
#ifndef GS_BILATERAL_H
#define GS_BILATERAL_H
#include "gs_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_BILATERAL_VERTEX_FLOATS 12
#define GS_BILATERAL_MIN_GRID 2                     /* every axis has at least one cell */
#define GS_BILATERAL_MAX_XY 64                      /* Gx, Gy */
#define GS_BILATERAL_MAX_L 8                        /* L: 12 * 8 = 96 sums per thread of the gather */
#define GS_BILATERAL_THREADS 256                    /* threads of a block of the image passes: one pixel each */
#define GS_BILATERAL_GATHER_THREADS 256             /* threads of a block of the grid gradient's gather */
#define GS_BILATERAL_TARGET_BLOCKS 1024             /* a vertex's footprint is split over max(1, this / (Gx Gy)) blocks */
#define GS_BILATERAL_TV_THREADS 1024                /* the one block of gs_bilateral_tv */
#define GS_BILATERAL_MAX_PIXELS 2147481600          /* 2^31 - 2048, as GS_APPEARANCE_MAX_PIXELS */

int gs_bilateral_slice(gs_ctx* ctx, const gs_loss_image* image, const float* grid, int32_t Gx, int32_t Gy, int32_t L, int32_t H,
                       int32_t W, const gs_loss_image* corrected, gs_stream stream);

int gs_bilateral_slice_backward(gs_ctx* ctx, const gs_loss_image* image, const gs_loss_image* grad_corrected, const float* grid,
                                int32_t Gx, int32_t Gy, int32_t L, int32_t H, int32_t W, const gs_loss_image* grad_image,
                                float* grad_grid, gs_stream stream);

int gs_bilateral_tv(gs_ctx* ctx, const float* grid, int32_t Gx, int32_t Gy, int32_t L, float weight, float* grad_grid, float* value,
                    gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
