/* gs_mixture.h -- the scene read as a Gaussian mixture, on the device: its log-density at arbitrary points and its
 * closed-form Fourier transform at arbitrary frequencies.  What the reference's FTGMM.py evaluates slice by slice in torch
 * (sample_gmm, transform_gmm_to_fourier1), and what an occupancy grid, a scene-bounds estimate or a floater inspection needs.
 *
 *   gs_mixture_log_density(ctx, xyz, features, mask, N, x, P, log_p, stream);          // log_p[P]
 *   gs_mixture_fourier(ctx, xyz, features, mask, N, k, P, centre, re_im, stream);      // re_im[P][2]
 *
 * Same library, same rules as gs_rasterizer.h: status codes, gs_last_error(), the call's stream last.  Not part of
 * GS_ABI_VERSION's function list.
 *
 * The mixture
 *  - A row of the scene is position mu (point_cloud, 3 floats) and a 56-float feature row: q as xyzw, log s (3), the opacity
 *    logit alpha, then SH (not read).
 *  - A row TAKES PART if its mask byte is 0 (or point_invalid_mask is NULL) and all of mu, q, log s and alpha are finite and
 *    |q|^2 > 0.  Any other row takes no part: it enters no sum and moves no output -- the outputs are bit-identical to those of
 *    the same call with that row masked.  (Taking rows OUT of the arrays moves the chunk boundaries of the component loop and
 *    the order in which the weights are summed, so it gives the same values to rounding, not to the bit; rows appended after
 *    the last one that takes part change nothing at all as long as the number of chunks is the same.)
 *  - Weights: pi_i = sigmoid(alpha_i) / sum_j sigmoid(alpha_j) over the rows that take part.  The sum is formed in float64 in
 *    one fixed order (blocks of 256 rows as a tree, the block sums in ascending order); there are no float atomics anywhere.
 *    If no row takes part, every log-density is -inf and every transform value is 0 + 0i.
 *  - Rotation: R is the rotation of q / |q|, i.e. the matrix 1 - (2/|q|^2) [...] that pytorch3d's quaternion_to_matrix returns
 *    and the reference's quaternions_to_scale_tril builds its covariances from.  rotation_from_quaternion in gs_point_math.h
 *    (the rasteriser's, as the reference's rasteriser has it) does NOT normalise and is NOT this matrix.  S = diag(exp(log s)).
 *  - Log-density: log p(x) = log sum_i pi_i N(x; mu_i, R S^2 R^T), evaluated in the whitened form
 *    -1/2 |S^-1 R^T (x - mu)|^2 + log pi - sum log s - 3/2 log 2 pi.  No Cholesky factor, no covariance or precision matrix is
 *    ever formed (in f32 those cancel when the scales are anisotropic).  The sum is a log-sum-exp with a running maximum: a
 *    point far from every component gives a large negative number or -inf, never NaN.
 *  - Transform: F(k) = sum_i pi_i exp(-1/2 |S R^T k|^2) (cos phi_i - i sin phi_i), phi_i = k . (mu_i - centre), k in radians
 *    per unit.  phi is reduced by a three-constant Cody-Waite step to [-pi/4, pi/4] before the sine and cosine polynomials, so
 *    hundreds or thousands of radians cost no accuracy beyond phi's own rounding.
 *    (Beyond 1e9 radians, where that rounding alone is over 60 radians, the phase is taken as 0.)
 *  - Exact: every row that takes part enters every output.  There is no cutoff radius; a term is left out only where its
 *    weight is exactly zero in f32.
 *  - A non-finite row of x or k gives NaN in its own output (both halves of a transform value) and nowhere else.
 *  - Deterministic: the result is a function of the inputs alone, two calls give the same bits.  The component loop is split
 *    into chunks by a rule that reads (n_points, n_x) only; the chunk partials are merged in ascending chunk order.
 *  - Numbers: the per-row records (whitening matrix, constant, weight) are computed in float64 and rounded once to f32;
 *    magnitudes beyond the f32 range are clamped to it.  The pair arithmetic is f32 with fused multiply-adds where written.
 *
 * How (csrc/k_mixture.hip): the weight sum, then one 64-byte record per row in the context's work memory, then a streaming
 * kernel over (query blocks) x (component chunks) with the records wave-uniform, then a merge of the chunk partials.
 *
 * Work memory belongs to the context (buffers of its own, counted by gs_ctx_device_bytes: 64 bytes per row, 8 bytes per
 * query and chunk; never a buffer that a kept frame or a pending backward reads), so a call may sit between a forward and
 * its backward, and it stops growing once it is large enough.  Nothing is copied to the host and nothing waits for it:
 * everything is queued on `stream`.
 */
#ifndef GS_MIXTURE_H
#define GS_MIXTURE_H
#include "gs_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest n_points and largest n_x / n_k of one call (2^30 each): the limits of the index arithmetic, not measured sizes. */
#define GS_MIXTURE_MAX_POINTS 1073741824
#define GS_MIXTURE_MAX_QUERIES 1073741824

/* point_cloud (n_points,3) f32, point_cloud_features (n_points,56) f32, point_invalid_mask n_points int8 or NULL,
 * x (n_x,3) f32, log_density_out n_x f32: all device memory, row-major.
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx NULL, n_points outside [0, GS_MIXTURE_MAX_POINTS], n_x outside
 * [0, GS_MIXTURE_MAX_QUERIES], any array but the mask NULL with n_points > 0 and n_x > 0.  n_x == 0 or n_points == 0 is GS_OK with no launch and no write (mixture.py fills -inf for an empty scene). */
int gs_mixture_log_density(gs_ctx* ctx, const float* point_cloud, const float* point_cloud_features,
                           const int8_t* point_invalid_mask, int64_t n_points, const float* x, int64_t n_x,
                           float* log_density_out, gs_stream stream);

/* k (n_k,3) f32 in radians per unit, centre 3 floats in DEVICE memory (a bounding box computed on the device never has to
 * come back to the host), re_im_out (n_k,2) f32: real and imaginary part.
 * Refused like the call above, centre NULL with n_k > 0 too.  n_k == 0 or n_points == 0 is GS_OK with no launch and no write (mixture.py fills 0 + 0i for an empty scene). */
int gs_mixture_fourier(gs_ctx* ctx, const float* point_cloud, const float* point_cloud_features,
                       const int8_t* point_invalid_mask, int64_t n_points, const float* k, int64_t n_k, const float* centre,
                       float* re_im_out, gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
