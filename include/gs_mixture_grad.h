/* gs_mixture_grad.h -- the gradients of the two evaluations of gs_mixture.h to the scene's parameters, on the device: what an
 * optimiser needs to use the log-density (a likelihood term that keeps Gaussians on SfM or lidar points, moving points along
 * grad_x log p) or the transform (a Fourier-space regulariser) in a loss.
 *
 *   gs_mixture_log_density_backward(ctx, xyz, features, mask, N, x, P, log_p, g, grad_xyz, grad_features, grad_x, stream);
 *   gs_mixture_fourier_backward(ctx, xyz, features, mask, N, k, P, centre, g_re_im, grad_xyz, grad_features, stream);
 *
 * Same library, same rules as gs_mixture.h: status codes, gs_last_error(), the call's stream last.  Not part of
 * GS_ABI_VERSION's function list.
 *
 * What is computed
 *  - The mixture, the rows that take part, the weights pi, R and S are those of gs_mixture.h.  With g the upstream gradient
 *    (dL/d log p(x_j), or dL/dRe F(k_j) and dL/dIm F(k_j)), the calls write dL/d mu into grad_point_cloud and dL/d(q xyzw, log s,
 *    opacity logit) into columns 0..7 of grad_features.  Columns 8..55 (SH) are not touched: hand in a zero-filled array.
 *  - Every element of grad_point_cloud and columns 0..7 of every row of grad_features are written.  A row that takes no part
 *    gets zeros, and its presence changes no bit of another row's gradient compared with the same row masked.
 *  - The quaternion's gradient goes through R(q / |q|): it is orthogonal to q and scales with 1 / |q|.
 *  - k and centre get no gradient.
 *  - A query contributes nothing (and its row of grad_x is 0) if its upstream gradient is exactly 0 (both halves, for the
 *    transform), if its coordinates are not finite or, for the density, if its forward value is not finite: a masked loss
 *    out[valid].sum() does not turn a NaN or -inf output into NaN gradients.  A NON-FINITE, NON-ZERO upstream gradient is the
 *    caller's mistake and may make every gradient NaN.
 *  - Deterministic: no atomics, the result is a function of the inputs alone.  The query loop is split into chunks by a rule
 *    that reads (n_points, n_x) only; the chunk partials are merged in ascending order.
 *  - Numbers: the pair arithmetic is f32 on the forward's records; no f32 sum is longer than 32 terms -- every 32 queries the
 *    ten sums of a row are added into float64 ones, the chunk partials are float64, and the per-row step from the sums to the
 *    gradients is float64, rounded once.  The sums over the queries (sum g) and over the rows (sum A) are float64 in one fixed order.
 *    The density's call computes log2 p(x_j) again, its terms added in float64: the share of a pair, pi N / p, is formed against
 *    that sum, and log_density only decides which queries are finite (its rounding to f32 would be in every share otherwise).
 *
 * Work memory belongs to the context (buffers of its own and the record buffers of gs_mixture.h, counted by
 * gs_ctx_device_bytes: 64 bytes per row, 32 bytes per query, 80 bytes per row and query chunk, for the density 24 bytes per query
 * and component chunk; never a buffer that a kept frame or a pending backward reads), and it stops growing once it is
 * large enough.  Nothing is copied to the host: everything is queued on `stream`.
 */
#ifndef GS_MIXTURE_GRAD_H
#define GS_MIXTURE_GRAD_H
#include "gs_mixture.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The arrays of gs_mixture_log_density, then log_density (n_x f32: what that call returned for these inputs),
 * grad_log_density (n_x f32), the outputs grad_point_cloud (n_points,3), grad_features (n_points,56) and grad_x (n_x,3) or NULL.
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx NULL, n_points outside [0, GS_MIXTURE_MAX_POINTS], n_x outside
 * [0, GS_MIXTURE_MAX_QUERIES], any array but the mask and grad_x NULL with n_points > 0 and n_x > 0.  n_x == 0 or n_points == 0
 * is GS_OK with no launch and no write (mixture_grad.py has zero-filled the outputs). */
int gs_mixture_log_density_backward(gs_ctx* ctx, const float* point_cloud, const float* point_cloud_features,
                                    const int8_t* point_invalid_mask, int64_t n_points, const float* x, int64_t n_x,
                                    const float* log_density, const float* grad_log_density, float* grad_point_cloud,
                                    float* grad_features, float* grad_x, gs_stream stream);

/* The arrays of gs_mixture_fourier, then grad_re_im (n_k,2) f32: dL/dRe F and dL/dIm F.  Refused and found empty like the call
 * above (centre NULL with n_k > 0 too). */
int gs_mixture_fourier_backward(gs_ctx* ctx, const float* point_cloud, const float* point_cloud_features,
                                const int8_t* point_invalid_mask, int64_t n_points, const float* k, int64_t n_k, const float* centre,
                                const float* grad_re_im, float* grad_point_cloud, float* grad_features, gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
