/* gs_pose_table.h -- per-view camera pose corrections: six floats per training view, composed onto the dataset's pose in
 * front of the rasteriser, and the gradient of the composed pose carried back to the six floats.
 *
 *   gs_pose_compose         (ctx, delta, q_base, t_base, V, K, q_out, t_out, stream);                 // before the forward
 *   gs_pose_compose_backward(ctx, delta, q_base, grad_q, grad_t, V, K, reg, grad_delta, stream);      // after the backward
 *
 * Same library, same rules as gs_rasterizer.h: status codes, gs_last_error(), the call's stream last.  Not part of
 * GS_ABI_VERSION's function list.  No call synchronises with the host or allocates memory; the host never reads the data.
 * No atomic anywhere: every output is bit-reproducible.  Every operation below is an IEEE float64 operation on the f32 values as
 * loaded, rounded on its own (no contraction) in the order the parentheses give, and every output is rounded to f32 once, on
 * store.  (csrc/k_posetable.hip)
 *
 * ---- layouts ----
 * delta (V,6) f32: row v is (w_0, w_1, w_2, u_0, u_1, u_2) -- a rotation vector w and a translation u, both in the camera's own
 * frame.  q_base (V,K,4) f32 xyzw and t_base (V,K,3) f32: the K object poses (q_pointcloud_camera, t_pointcloud_camera rows) of
 * every view, as the rasteriser reads them; the quaternions are NOT normalised, here as there.  A camera-frame correction is the
 * same for every object, so all K rows of view v take row v of delta.  Everything is contiguous device memory.
 *
 * ---- gs_pose_compose: T' = T_base * D(delta) ----
 * One thread per view, the rows k = 0 .. K-1 in order, blocks of GS_POSE_THREADS.
 *   s = (w_0 w_0 + w_1 w_1) + w_2 w_2,   th = sqrt(s)
 *   s >= GS_POSE_SERIES_S:   A = sin(th / 2) / th,                      C = cos(th / 2)
 *   s <  GS_POSE_SERIES_S:   A = 1/2 + s (-1/48 + s / 3840),            C = 1 + s (-1/8 + s / 384)
 *   dq = (A w_0, A w_1, A w_2, C)
 *   q' = q (x) dq, the product of quat_mul (k_project.hip), a = q, b = dq, each component summed left to right:
 *        q'_0 = w x1 + x w1 + y z1 - z y1      q'_1 = w y1 - x z1 + y w1 + z x1
 *        q'_2 = w z1 + x y1 - y x1 + z w1      q'_3 = w w1 - x x1 - y y1 - z z1          (q = x y z w, dq = x1 y1 z1 w1)
 *   R  = rotation_from_quaternion (gs_point_math.h) of q as stored:
 *        R_00 = 1 - 2 (yy + zz)   R_01 = 2 (xy - wz)       R_02 = 2 (xz + wy)
 *        R_10 = 2 (xy + wz)       R_11 = 1 - 2 (xx + zz)   R_12 = 2 (yz - wx)
 *        R_20 = 2 (xz - wy)       R_21 = 2 (yz + wx)       R_22 = 1 - 2 (xx + yy)
 *   t'_i = t_i + ((R_i0 u_0 + R_i1 u_1) + R_i2 u_2)
 * For a unit q this is T' = T D with D = [exp(w^) | u]: the correction acts on the right, in the camera's frame.  The series are
 * exact to float64 below the threshold (the next terms are below 1e-20) and meet the closed forms there.
 * SELECTION: a view whose six floats are all exactly zero (-0 is zero) gets its base rows copied bit for bit, whatever they
 * hold -- an untrained table is the dataset's poses to the last bit.  A view with a non-finite float among its six gets NaN in
 * every output of its own; no other view is touched by it.  q_out and t_out may be q_base and t_base themselves (in place);
 * any other overlap is not allowed.
 *
 * ---- gs_pose_compose_backward ----
 * g_q (V,K,4) and g_t (V,K,3) are dL/dq' and dL/dt'.  One thread per view, blocks of GS_POSE_THREADS; the sums over k run from
 * k = 0 up, starting from 0, one row added at a time: a fixed order.
 *   G_u[j] = sum_k ((R_0j g_t0 + R_1j g_t1) + R_2j g_t2)                                    = sum_k (R(q_k)^T g_t,k)_j
 *   G_dq   = sum_k L(q_k)^T g_q,k, component by component, each summed left to right:
 *        x1:  w g0 + z g1 - y g2 - x g3       y1: -z g0 + w g1 + x g2 - y g3
 *        z1:  y g0 - x g1 + w g2 - z g3       w1:  x g0 + y g1 + z g2 + w g3
 *   B = (C / 2 - A) / s for s >= GS_POSE_SERIES_S, else -1/24 + s / 960            (d(A w_i)/dw_j = A [i = j] + B w_i w_j)
 *   d = (w_0 G_dq[0] + w_1 G_dq[1]) + w_2 G_dq[2]
 *   G_w[j] = (A G_dq[j] + (B w_j) d) - ((A w_j) / 2) G_dq[3]                                 (dC/dw_j = -A w_j / 2)
 *   grad_delta[v] = (G_w + reg w, G_u + reg u)
 * WRITTEN, not added.  reg * delta is the gradient of (reg / 2) |delta|^2, an L2 pull to the dataset's pose.  A view of zeros
 * has A = 1/2, B = -1/24 like any other view below the threshold: selection is the forward's alone.  A view with a non-finite
 * float among its six has a non-finite value in its own row (reg * delta alone makes one: 0 * inf is NaN) and touches no other.
 * Base poses are data: they get no gradient.
 *
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx NULL; V or K negative, V above GS_POSE_MAX_VIEWS, K above
 * GS_POSE_MAX_OBJECTS; with V > 0 and K > 0, a NULL array; reg not finite.  V == 0 or K == 0 is GS_OK and launches nothing.
 */
#ifndef GS_POSE_TABLE_H
#define GS_POSE_TABLE_H
#include "gs_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_POSE_DELTA_FLOATS 6
#define GS_POSE_THREADS 256                 /* threads of a block: one per view */
#define GS_POSE_SERIES_S 1e-8               /* on |w|^2: below it sin(th/2)/th, cos(th/2) and their derivative are series */
#define GS_POSE_MAX_VIEWS 16777216          /* 2^24 */
#define GS_POSE_MAX_OBJECTS 64

int gs_pose_compose(gs_ctx* ctx, const float* delta, const float* q_base, const float* t_base, int32_t V, int32_t K,
                    float* q_out, float* t_out, gs_stream stream);

int gs_pose_compose_backward(gs_ctx* ctx, const float* delta, const float* q_base, const float* grad_q, const float* grad_t,
                             int32_t V, int32_t K, float reg, float* grad_delta, gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
