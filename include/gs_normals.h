/* gs_normals.h -- a normal per Gaussian, with its gradient to the quaternion, and the consistency of the rendered Gaussian
 * normals with the normal of the rendered depth (2DGS, GOF, PGSR), with its gradients to the depth and to the rendered normals.
 *
 *   gs_gaussian_normals_forward   (ctx, point_cloud, features, point_object_id_or_NULL, q_pointcloud_camera, t_pointcloud_camera,
 *                                  N, K, normals, stream);                                                   // normals (N,3)
 *   gs_gaussian_normals_backward  (ctx, point_cloud, features, point_object_id_or_NULL, q_pointcloud_camera, t_pointcloud_camera,
 *                                  N, K, grad_normals, grad_features, stream);                               // grad_features (N,56)
 *   gs_normal_consistency_forward (ctx, D, R, w_p_or_NULL, H, W, fx, fy, cx, cy, max_rel_jump, min_length, terms, stream);
 *   gs_normal_consistency_backward(ctx, D, R, w_p_or_NULL, H, W, fx, fy, cx, cy, max_rel_jump, min_length, terms, upstream_or_NULL,
 *                                  grad_D, grad_R, stream);
 *
 * Same library, same rules as gs_geometry.h: status codes, gs_last_error(), the call's stream last.  Not part of GS_ABI_VERSION's
 * function list.  No call synchronises with the host or allocates caller-visible memory; the host never reads the data.  No
 * float atomic anywhere: the same inputs give the same bits on every run.  Past the f32 loads everything is float64, every
 * operation rounded on its own (no contraction) in the order the parentheses give, division and square root correctly rounded;
 * a result is rounded once to f32.  Selection, not multiplication: what is not selected adds nothing, whatever it holds, and
 * what only unselected terms reach is exactly +0.  (csrc/k_normals.hip)
 *
 * ---- the normal of a Gaussian ----
 * Row i of point_cloud (N,3) is x; row i of features (N,56) holds the quaternion q = (x, y, z, w) in columns 0..3 as stored, NOT
 * normalised, and the log-scales in columns 4..6.  The row's object is o = point_object_id[i] (int32; 0 for every row when the
 * array is NULL; an id outside [0, K) zeroes the row), its pose q_o = row o of q_pointcloud_camera (K,4), xyzw, and t_o = row o
 * of t_pointcloud_camera (K,3).
 *   R(q)   the rasteriser's rotation_from_quaternion (csrc/gs_point_math.h), of the float64 values of q:
 *              R00 = 1 - 2 (yy + zz)   R01 = 2 (xy - wz)       R02 = 2 (xz + wy)
 *              R10 = 2 (xy + wz)       R11 = 1 - 2 (xx + zz)   R12 = 2 (yz - wx)
 *              R20 = 2 (xz - wy)       R21 = 2 (yz + wx)       R22 = 1 - 2 (xx + yy)         with xx = x x, xy = x y, ...
 *   k      the index of the smallest of the three log-scales (compared as f32), ties to the smaller index:
 *              k = 0;  if (s_1 < s_k) k = 1;  if (s_2 < s_k) k = 2.
 *   c      column k of R(q): c = (R0k, R1k, R2k).   l2 = (c.x c.x + c.y c.y) + c.z c.z,   l = sqrt(l2),   u = c / l.
 *   pose   P = R(q_o) of the float64 values of the pose quaternion as stored (the projection rotates by R of its conjugate,
 *          which is the transpose of P, bit for bit).  For j = 0, 1, 2:
 *              m_j = (P0j u.x + P1j u.y) + P2j u.z                          m = P^T u
 *              d   = x - t_o  (three subtractions),   p_j = (P0j d.x + P1j d.y) + P2j d.z      p = P^T (x - t_o)
 *   sign   a = (m.x p.x + m.y p.y) + m.z p.z;   n = m if a <= 0, else n = -m.  The normal faces the camera, as gs_depth_normals
 *          gives (0, 0, -1) for a wall seen head on.
 * A row is ZEROED -- (+0, +0, +0) -- unless its four q, three log-scales and three coordinates are finite, q is not the zero
 * quaternion (((xx + yy) + zz) + ww > 0: R(0) is the identity, but a zero quaternion is no rotation and has a zero gradient) and
 * l2 > 0 && l2 <= DBL_MAX.  Every row of normals is written.
 *
 * For a quaternion far from unit length R(q) is not a rotation, and its columns are not the principal axes of R S^2 R^T: the
 * normal is that of the stored parametrisation, as the rasteriser's covariance is.  A pose quaternion is used as stored too:
 * for one that is not of unit length n is not either.
 *
 * ---- gs_gaussian_normals_backward ----
 * The exact derivative of n in q with k and the sign held fixed, g = the float64 values of the row of grad_normals (N,3):
 *   gm   = g if a <= 0, else -g
 *   gu_j = (Pj0 gm.x + Pj1 gm.y) + Pj2 gm.z                                 through m = P^T u (P is constant)
 *   b    = (gu.x u.x + gu.y u.y) + gu.z u.z,   gc_j = (gu_j - b u_j) / l      through the normalisation
 *   grad_features[i, e] = (J_e0 gc.x + J_e1 gc.y) + J_e2 gc.z,  e = 0..3      J_e = d c / d q_e, the four partials of the column:
 *              k = 0:  J_x = (0, 2y, 2z)      J_y = (-4y, 2x, -2w)    J_z = (-4z, 2w, 2x)     J_w = (0, 2z, -2y)
 *              k = 1:  J_x = (2y, -4x, 2w)    J_y = (2x, 0, 2z)       J_z = (-2w, -4z, 2y)    J_w = (-2z, 0, 2x)
 *              k = 2:  J_x = (2z, -2w, -4x)   J_y = (2w, 2z, -4y)     J_z = (2x, 2y, 0)       J_w = (2y, -2x, 0)
 *          (a product by 2 or 4 and a negation are exact; a zero entry multiplies like any other).
 * Columns 0..3 of every row of grad_features (N,56) are written so, columns 4..55 as +0, and a zeroed row is +0 throughout.
 * No gradient goes to the position, the scales (the axis is a selection) or the pose.
 * Rows are in lanes: thread t of a 256-thread block works on row 256 block + t, one block per 256 rows.
 *
 * ---- gs_normal_consistency_forward / gs_normal_consistency_backward ----
 * D is the (H,W) depth plane of gs_geometry.h; R is (H,W,3) f32, INTERLEAVED as gs_channels_forward writes it: channel j of
 * pixel p = y W + x is element 3 p + j.  It is read, and grad_R written, where it lies: no permuted copy of either is made.
 *   depth normal   n, len and whether the normal EXISTS at a pixel: those of gs_geometry.h ("the normal at (x, y)"), with fx, fy,
 *                  cx, cy and max_rel_jump as there.
 *   rendered       m = (double)R(p), the alpha-weighted blend, not normalised.  k = sqrt((m.x m.x + m.y m.y) + m.z m.z).  m is
 *                  USABLE iff k >= (double)min_length && k <= DBL_MAX, and then h = m / k.  (Where the blend is thin, or opposing
 *                  normals cancelled, the pixel is left out, not normalised.)
 *   selection      w = a(w_p) of gs_geometry.h (w > 0 ? w : 0; NULL counts as 1).  Pixel p is SELECTED iff its depth normal
 *                  exists, m is usable and w > 0.
 *   loss           cos = (n.x h.x + n.y h.y) + n.z h.z.   L = (sum w (1 - cos)) / (sum w) =: S_l / S_w.
 *   terms          8 floats of device memory, written: { L, S_w, number selected, (sum cos) / number selected, 0, 0, 0, 0 }, each a
 *                  float64 value rounded once.  Nothing selected: eight zeros, every gradient +0, nothing NaN.
 *   backward       reads terms[1] (the f32 S_w) on the device and selects anew.  With t = *upstream (NULL: 1), s = t / S_w:
 *                  grad_D is the gather of gs_normal_loss_backward with this h, w and s: g = -(s w) (h - cos n) / len, gx, gy, what
 *                  the normal owes its four neighbours, and the order of the gather, all as stated there.
 *                  grad_R(p)_j = (-(s w) (n_j - cos h_j)) / k at a selected pixel, +0 elsewhere: through h = m / k.
 *                  Both are written by one launch, every element.  The selections are held fixed.
 * The derivative of R through the blend weights (the means, covariances and opacities of the Gaussians) is not part of this
 * library: gs_channels.h blends over a frozen geometry.  The term reaches rotations through grad_R and gs_channels_backward,
 * and positions, scales and opacities through grad_D and the depth backward.
 *
 * Kernel shape: that of gs_geometry.h -- one 256-thread block per GS_GEOM_TILE_H x GS_GEOM_TILE_W tile, D and w_p staged in LDS
 * with the halo (four pixels per lane where the plane allows, with equal bits), R staged for the tile grown by one pixel, per-tile
 * float64 sums in the fixed order, the finishing block of gs_geometry.h.  Launches: forward GS_NORMALS_FORWARD_LAUNCHES (tile
 * pass, finish), backward 1.  Work memory (per-tile sums) belongs to the context and is counted by gs_ctx_device_bytes.
 *
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx NULL; any array NULL but point_object_id, w_p and upstream (with
 * N == 0 the per-row arrays may be NULL and the call does nothing); N outside [0, 2^31 - 256]; K < 1; H or W below 1, or more than
 * GS_NORMALS_MAX_PIXELS pixels (3 H W must index as int32); fx or fy not finite or not > 0; cx or cy not finite; max_rel_jump not
 * finite or negative; min_length not finite or not > 0.  An image too small to hold a normal (2x2) is GS_OK with zero terms and
 * zero gradients.
 */
#ifndef GS_NORMALS_H
#define GS_NORMALS_H
#include "gs_rasterizer.h"
#include "gs_geometry.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_NORMALS_FEATURES 56              /* floats of a feature row */
#define GS_NORMALS_BLOCK 256                /* rows per block of the per-row kernels */
#define GS_NORMALS_MAX_PIXELS 715827200     /* 3 H W + 3 * 64 < 2^31 */
#define GS_NORMALS_LOSS_TERMS 8
#define GS_NORMALS_FORWARD_LAUNCHES 2
#define GS_NORMALS_BACKWARD_LAUNCHES 1

int gs_gaussian_normals_forward(gs_ctx* ctx, const float* point_cloud, const float* features, const int32_t* point_object_id,
                                const float* q_pointcloud_camera, const float* t_pointcloud_camera, int64_t N, int32_t K, float* normals,
                                gs_stream stream);

int gs_gaussian_normals_backward(gs_ctx* ctx, const float* point_cloud, const float* features, const int32_t* point_object_id,
                                 const float* q_pointcloud_camera, const float* t_pointcloud_camera, int64_t N, int32_t K,
                                 const float* grad_normals, float* grad_features, gs_stream stream);

int gs_normal_consistency_forward(gs_ctx* ctx, const float* D, const float* R, const float* w_p, int32_t H, int32_t W, float fx, float fy,
                                  float cx, float cy, float max_rel_jump, float min_length, float* terms, gs_stream stream);

int gs_normal_consistency_backward(gs_ctx* ctx, const float* D, const float* R, const float* w_p, int32_t H, int32_t W, float fx, float fy,
                                   float cx, float cy, float max_rel_jump, float min_length, const float* terms, const float* upstream,
                                   float* grad_D, float* grad_R, gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
