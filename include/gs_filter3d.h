/* gs_filter3d.h -- the 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024): every Gaussian gets an isotropic low-pass
 * whose width is the finest pixel footprint any training view had of it.  The largest sampling rate of every row over a table
 * of views, the transform of a feature row under that filter, and the gradient of the transform.
 *
 *   gs_filter3d_rate          (ctx, point_cloud, point_invalid_mask, n_points, views, n_views, W, H, near, margin, rate_out, stream);
 *   gs_filter3d_apply         (ctx, features, rate, n_points, k, features_out, stream);
 *   gs_filter3d_apply_backward(ctx, grad_out, features, rate, n_points, k, grad_in, stream);
 *
 * Same library, same rules as gs_rasterizer.h: status codes, gs_last_error(), the call's stream last.  Not part of
 * GS_ABI_VERSION's function list.  No call synchronises with the host or allocates caller-visible memory; the host never
 * reads the data.  No float atomic anywhere: every output is bit-reproducible and does not depend on how the rows are spread
 * over blocks.  Every f32 and f64 operation below is rounded on its own (no contraction), in the order the parentheses give;
 * division, sqrtf and sqrt are correctly rounded.  (csrc/k_filter3d.hip)
 *
 * ---- rows and views ----
 * point_cloud is (n_points,3) f32, point_invalid_mask (n_points) int8 (0: the row is valid), features (n_points,56) f32 in the
 * rasteriser's layout: columns 0..3 the rotation quaternion xyzw, 4..6 the log-scales ls_0..ls_2, 7 the opacity logit a,
 * 8..55 the colour.  A view is GS_FILTER3D_VIEW_FLOATS = 16 floats of device memory:
 *   R[0..8]   the row-major rotation, camera from point cloud          view[0..8]
 *   t[0..2]   its translation                                          view[9..11]
 *   fx fy cx cy                                                        view[12..15]
 * The caller makes R and t on the host (float64, rounded once) from the dataset's T_pointcloud_camera; they are what the
 * rasteriser's pose record holds for the same camera, up to that rounding.  W and H, in pixels, are shared by the views of a
 * call.
 *
 * ---- gs_filter3d_rate ----
 * For a valid row n at x = point_cloud[n] and a view, in f32:
 *   p_j  = ((R[3j] * x_0 + R[3j+1] * x_1) + R[3j+2] * x_2) + t[j]          j = 0, 1, 2: the rasteriser's project_point
 *   u    = (fx * p_0) / p_2 + cx            v = (fy * p_1) / p_2 + cy
 *   fm   = fx > fy ? fx : fy
 *   c    = fm / p_2
 * The view SEES the row when every one of these comparisons is true (a comparison with a NaN is not):
 *   p_2 > near      lo_x <= u      u <= hi_x      lo_y <= v      v <= hi_y      c > 0.0f
 * with lo_x = (-margin) * (float)W, hi_x = (1.0f + margin) * (float)W, and lo_y, hi_y the same of H.
 *   rate_out[n] = the largest c over the views that see the row                    for a valid row some view sees
 *   rate_out[n] = the smallest rate_out of any such row                            for a valid row no view sees
 *   rate_out[n] = +inf                                                             for an invalid row
 * When no row is seen by any view (n_views == 0 included) every rate is +inf, under which gs_filter3d_apply is the identity.
 * The maximum and the minimum are exact, so no order of rows or views enters the result; the minimum is taken with an integer
 * atomic on the bit patterns, which order as the positive floats do.  The three divisions are made per pair as written: no
 * cheaper test that is exactly equivalent to them was found.
 *
 * ---- gs_filter3d_apply ----
 * k = sqrtf(variance) * factor: variance the filter's variance in square pixels (Mip-Splatting: 0.2), factor the downsample
 * factor of the frame the features are rendered into.  Per row:
 *   f = k / rate[n]                                                        f32: the filter's standard deviation in the scene
 * A row with !(f > 0.0f) -- a rate of +inf, k == 0, a NaN -- is an IDENTITY row: its 56 floats are copied to features_out bit
 * for bit and the input row is not touched.  Every other row:
 *   1. its quaternion is normalised IN THE INPUT ROW with the rasteriser's operations (k_project):
 *        n = sqrtf(((q_0 * q_0 + q_1 * q_1) + q_2 * q_2) + q_3 * q_3)      q_i <- q_i / n
 *      and written back only when a bit of the four changed.  features_out[n][0..3] are the normalised values.  Without this
 *      the rasteriser's own in-place normalisation would land on features_out, and the caller's parameter would never be
 *      normalised.  The rasteriser normalises features_out once more, which may move it by one more ulp: normalising is not
 *      exactly idempotent.
 *   2. in float64 behind the f32 loads, rounded once where (float) stands:
 *        v    = (double)f * (double)f
 *        e_j  = exp((double)ls_j)       s_j = e_j * e_j       t_j = s_j + v       r_j = s_j / t_j          j = 0, 1, 2
 *        ls'_j = (float)(0.5 * log(t_j))
 *        c    = sqrt((r_0 * r_1) * r_2)
 *        a'   = (float)(log(c) - log((1.0 - c) + exp(-(double)a)))
 *      a' is logit(sigmoid(a) c) in a form that neither saturates nor cancels: c^2 = det S^2 / det(S^2 + v).
 *   3. columns 8..55 are copied bit for bit.
 * exp and log are the device library's float64 functions (below one ulp of float64): a result may differ from another
 * float64 evaluation by one f32 ulp where the exact value lies next to a rounding boundary.  features_out must not overlap
 * features.
 *
 * ---- gs_filter3d_apply_backward ----
 * g' = grad_out[n], g = grad_in[n]; features, rate and k as they were given to gs_filter3d_apply (the quaternion is not read).
 * An identity row passes its 56 gradients through bit for bit.  Every other row, with r_j and c as above, in float64:
 *   E    = exp(-(double)a)        D = (1.0 - c) + E
 *   g_a  = (float)((g'_a * E) / D)                                         exactly +0 when g'_a == 0
 *   g_ls_j = (float)(A_j + B_j)   A_j = g'_ls_j * r_j                      A_j is exactly +0 when g'_ls_j == 0
 *                                 B_j = (g'_a * (1.0 + c / D)) * (1.0 - r_j)      B_j is exactly +0 when g'_a == 0
 * Selection, not multiplication: a zero upstream value (-0 is 0, a NaN is not) gives a zero term whatever the row holds.
 * Every other column passes through bit for bit.  The filter itself (rate, k) gets no gradient.  grad_in may be grad_out
 * itself (the same pointer: the pass-through columns are then left where they are); any other overlap is not allowed.
 *
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx NULL; n_points outside 0 .. GS_FILTER3D_MAX_POINTS; n_views
 * outside 0 .. GS_FILTER3D_MAX_VIEWS; W or H below 1; near not finite or not > 0; margin not finite or < 0; k not finite or
 * < 0; a NULL array with n_points > 0 (views with n_views > 0); features, features_out, grad_out or grad_in not 16-byte
 * aligned; features_out == features.
 */
#ifndef GS_FILTER3D_H
#define GS_FILTER3D_H
#include "gs_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_FILTER3D_VIEW_FLOATS 16                  /* R (9), t (3), fx, fy, cx, cy */
#define GS_FILTER3D_FEATURES 56                     /* floats of a feature row */
#define GS_FILTER3D_ROWS_PER_BLOCK 256              /* rows of one block of every kernel: one per thread */
#define GS_FILTER3D_MAX_POINTS 1073741824           /* 2^30 */
#define GS_FILTER3D_MAX_VIEWS 1048576               /* 2^20 */

int gs_filter3d_rate(gs_ctx* ctx, const float* point_cloud, const int8_t* point_invalid_mask, int64_t n_points, const float* views,
                     int32_t n_views, int32_t W, int32_t H, float near, float margin, float* rate_out, gs_stream stream);

int gs_filter3d_apply(gs_ctx* ctx, float* features, const float* rate, int64_t n_points, float k, float* features_out,
                      gs_stream stream);

int gs_filter3d_apply_backward(gs_ctx* ctx, const float* grad_out, const float* features, const float* rate, int64_t n_points, float k,
                               float* grad_in, gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
