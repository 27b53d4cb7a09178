/* gs_compose.h -- baking a placed scene: one similarity transform applied to the rows of a scene, positions, covariance
 * quaternions, log-scales and the spherical-harmonic colour coefficients of bands 1..3, as one kernel launch.  What a viewer
 * needs to save objects it has moved: the rasteriser shows K objects under K pose rows, and this call writes the same picture
 * back as one ordinary scene in the world frame.
 *
 *   for k in objects:  gs_scene_bake(ctx, xyz_k, feat_k, n_k, q_k, t_k, s_k, sh_k, xyz_out, feat_out, offset_k, stream);
 *
 * Each call writes rows [row_offset, row_offset + n) of the outputs, so merging K objects is K launches and no concatenation.
 * Same library, same rules as gs_rasterizer.h: status codes, gs_last_error(), the call's stream last.  Not part of
 * GS_ABI_VERSION's function list.
 *
 * What is computed, per row (x,y,z | q xyzw, log-scale[3], opacity logit, R,G,B x 16 SH coefficients), with A = (q_A, t_A, s):
 *  - p' = s R_A p + t_A.  The nine entries of s R_A and log(s) are made on the host in float64 from q_A / |q_A| and rounded
 *    once to f32; each coordinate is one chain  fma(m_i2, z, fma(m_i1, y, m_i0 * x)) + t_i.
 *  - q' = q_A (x) (q / |q|): the Hamilton product in xyzw, |q| = sqrtf of the ascending sum of squares, true divisions.  A row
 *    whose |q| is zero or not finite keeps its four quaternion words as they are; everything else of it is still transformed.
 *  - log-scale' = log-scale + log(s); the opacity logit is copied.
 *  - every colour channel's 16 coefficients are multiplied band by band by the matrices M_0 (1x1), M_1 (3x3), M_2 (5x5),
 *    M_3 (7x7) of sh_matrices: f'_i = sum_j M_l[i][j] f_j as one fma chain in ascending j.  M_l is the matrix with
 *    Y_l(R_A d) = M_l Y_l(d) for the basis the rasteriser shades with; it is orthogonal, so the baked coefficients satisfy
 *    sum_k f'_k Y_k(R_A d) = sum_k f_k Y_k(d).  The caller makes the GS_BAKE_SH_FLOATS entries in float64 and rounds them once;
 *    the kernel evaluates no basis function.
 *  No atomics; the same bits on every run.
 *
 * How (csrc/k_compose.hip): a one-wave workgroup owns 64 consecutive rows; their 56-float feature rows pass through LDS
 * (coalesced loads and stores, a padded row per lane in between), the 12-byte positions go as scalars: they are not 16-byte
 * aligned at odd rows.  The call does NOT synchronise with the host and allocates nothing.
 */
#ifndef GS_COMPOSE_H
#define GS_COMPOSE_H
#include "gs_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_BAKE_FEATURES 56     /* floats of a feature row */
#define GS_BAKE_SH_FLOATS 84    /* 1 + 9 + 25 + 49: M_0, M_1, M_2, M_3, each row-major, in this order */
#define GS_BAKE_ROWS_PER_BLOCK 64

/* xyz_in (n,3), features_in (n,56): device memory, read.  xyz_out, features_out: device memory of at least row_offset + n
 * rows; rows [row_offset, row_offset + n) are written, no other.  q_A (4, xyzw; normalised here in float64), t_A (3) and
 * sh_matrices (GS_BAKE_SH_FLOATS) are HOST arrays, read before the call returns.
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx NULL; n or row_offset negative, or row_offset + n >= 2^31;
 * q_A, t_A or sh_matrices NULL; scale not finite or <= 0; a q_A of norm zero or not finite, a t_A or matrix entry not finite;
 * with n > 0 also: a NULL array, or an input range that overlaps an output range that is written (the call runs out of
 * place).  n == 0 is GS_OK with no launch. */
int gs_scene_bake(gs_ctx* ctx, const float* xyz_in, const float* features_in, int64_t n, const float* q_A, const float* t_A,
                  float scale, const float* sh_matrices, float* xyz_out, float* features_out, int64_t row_offset,
                  gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
