// gs_api_calls.hip -- the entry points of libgsrast.so's C ABI that hold no frame: each checks its arguments (touching nothing
// of the context), then queues its launch through queued_call (gs_host.h).  A new feature's entry points go here, under a
// section of their own; what knows a Frame is gs_api.hip's.
#include "../../include/gs_sparse.h"
#include "../../include/gs_knn.h"
#include "../../include/gs_exchange.h"
#include "../../include/gs_targets.h"
#include "../../include/gs_targets_rgba.h"
#include "../../include/gs_loss_weighted.h"
#include "../../include/gs_mixture.h"
#include "../../include/gs_mixture_grad.h"
#include "../../include/gs_compose.h"
#include "../../include/gs_frames.h"
#include "../../include/gs_fusion.h"
#include "../../include/gs_mcmc.h"
#include "../../include/gs_appearance.h"
#include "../../include/gs_background.h"
#include "../../include/gs_bilateral.h"
#include "../../include/gs_filter3d.h"
#include "../../include/gs_vq.h"
#include "../../include/gs_depth.h"
#include "../../include/gs_geometry.h"
#include "../../include/gs_normals.h"
#include "../../include/gs_pose_table.h"
#include "gs_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>

// ---- the fused loss, the scale regulariser and Adam (k_loss.hip) ----------------------------------------------------------------
static GsLossImage loss_image(const gs_loss_image* im, int clamp)
{
    GsLossImage r; r.p = im->data; r.sc = im->stride_channel; r.sy = im->stride_row; r.sx = im->stride_column; r.clamp = clamp;
    return r;
}
static int loss_check(const char* who, const gs_loss_image* a, const gs_loss_image* b, int32_t H, int32_t W)
{
    if (!a || !b || !a->data || !b->data) return fail(GS_ERR_INVALID_ARGUMENT, who, "NULL image");
    if (H < 11 || W < 11) return fail(GS_ERR_INVALID_ARGUMENT, who, "image smaller than the 11x11 SSIM window");
    return GS_OK;
}

// H and W of an image-sized call: both at least 1, and no more pixels than the kernels' indices hold
static int image_size_check(const char* who, int32_t H, int32_t W, int64_t max_pixels)
{
    if (H < 1 || W < 1) return fail(GS_ERR_INVALID_ARGUMENT, who, "H and W must be >= 1");
    if ((int64_t)H * (int64_t)W > max_pixels) return fail(GS_ERR_INVALID_ARGUMENT, who, "too many pixels");
    return GS_OK;
}

extern "C" int64_t gs_loss_maps_floats(int32_t H, int32_t W) { return (H < 1 || W < 1) ? 0 : (int64_t)gs_loss_maps_size((int)H, (int)W); }

extern "C" int gs_loss_l1_ssim_forward(gs_ctx* c, const gs_loss_image* pred, const gs_loss_image* gt, int32_t H, int32_t W, int32_t clamp_pred,
                                       float lambda_value, float* maps, float* loss_terms, gs_stream stream_)
{
    if (!c || !maps || !loss_terms) return fail(GS_ERR_INVALID_ARGUMENT, "gs_loss_l1_ssim_forward: NULL argument");
    if (int rc = loss_check("gs_loss_l1_ssim_forward", pred, gt, H, W)) return rc;
    return queued_call(c, stream_, "gs_loss_l1_ssim_forward", { NEED(c->loss_ws, gs_loss_partials_floats(H, W) * sizeof(float)) },
                       [&](hipStream_t s) {
        gs_launch_loss_forward(loss_image(pred, clamp_pred != 0), loss_image(gt, 0), H, W, lambda_value, maps, c->loss_ws.as<float>(), loss_terms, s);
    });
}

extern "C" int gs_loss_l1_ssim_backward(gs_ctx* c, const gs_loss_image* pred, const gs_loss_image* gt, int32_t H, int32_t W, int32_t clamp_pred,
                                        float lambda_value, const float* maps, const float* upstream, const gs_loss_image* grad_pred,
                                        gs_stream stream_)
{
    if (!c || !maps || !grad_pred || !grad_pred->data) return fail(GS_ERR_INVALID_ARGUMENT, "gs_loss_l1_ssim_backward: NULL argument");
    if (int rc = loss_check("gs_loss_l1_ssim_backward", pred, gt, H, W)) return rc;
    return queued_call(c, stream_, "gs_loss_l1_ssim_backward", {}, [&](hipStream_t s) {
        gs_launch_loss_backward(loss_image(pred, clamp_pred != 0), loss_image(gt, 0), H, W, lambda_value, maps, upstream, loss_image(grad_pred, 0), s);
    });
}

// ---- per-pixel weights (include/gs_loss_weighted.h) ----
extern "C" int gs_loss_l1_ssim_weighted_forward(gs_ctx* c, const gs_loss_image* pred, const gs_loss_image* gt, const float* pixel_weight,
                                                int32_t H, int32_t W, int32_t clamp_pred, float lambda_value, float* maps, float* loss_terms,
                                                gs_stream stream_)
{
    if (!c || !pixel_weight || !maps || !loss_terms) return fail(GS_ERR_INVALID_ARGUMENT, "gs_loss_l1_ssim_weighted_forward: NULL argument");
    if (int rc = loss_check("gs_loss_l1_ssim_weighted_forward", pred, gt, H, W)) return rc;
    return queued_call(c, stream_, "gs_loss_l1_ssim_weighted_forward",
                       { NEED(c->loss_ws, gs_loss_weighted_partials_floats(H, W) * sizeof(float)) }, [&](hipStream_t s) {
        gs_launch_loss_weighted_forward(loss_image(pred, clamp_pred != 0), loss_image(gt, 0), pixel_weight, H, W, lambda_value, maps,
                                        c->loss_ws.as<float>(), loss_terms, s);
    });
}

extern "C" int gs_loss_l1_ssim_weighted_backward(gs_ctx* c, const gs_loss_image* pred, const gs_loss_image* gt, const float* pixel_weight,
                                                 int32_t H, int32_t W, int32_t clamp_pred, float lambda_value, const float* maps,
                                                 const float* loss_terms, const float* upstream, const gs_loss_image* grad_pred,
                                                 gs_stream stream_)
{
    if (!c || !pixel_weight || !maps || !loss_terms || !grad_pred || !grad_pred->data)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_loss_l1_ssim_weighted_backward: NULL argument");
    if (int rc = loss_check("gs_loss_l1_ssim_weighted_backward", pred, gt, H, W)) return rc;
    return queued_call(c, stream_, "gs_loss_l1_ssim_weighted_backward", {}, [&](hipStream_t s) {
        gs_launch_loss_weighted_backward(loss_image(pred, clamp_pred != 0), loss_image(gt, 0), pixel_weight, H, W, lambda_value, maps, loss_terms,
                                         upstream, loss_image(grad_pred, 0), s);
    });
}

// the one-call form: contiguous (3,H,W) images, the maps in the context's own workspace, upstream = 1
extern "C" int gs_loss_l1_ssim(gs_ctx* c, const float* pred, const float* gt, int32_t H, int32_t W, float lambda_value,
                               float* loss_terms, float* grad_pred, gs_stream stream_)
{
    if (!c || !pred || !gt || !loss_terms) return fail(GS_ERR_INVALID_ARGUMENT, "gs_loss_l1_ssim: NULL argument");
    if (H < 11 || W < 11) return fail(GS_ERR_INVALID_ARGUMENT, "gs_loss_l1_ssim: image smaller than the 11x11 SSIM window");
    const size_t maps_floats = gs_loss_maps_size(H, W);
    return queued_call(c, stream_, "gs_loss_l1_ssim", { NEED(c->loss_ws, (maps_floats + gs_loss_partials_floats(H, W)) * sizeof(float)) },
                       [&](hipStream_t s) {
        GsLossImage X{ pred, (long long)H * W, (long long)W, 1, 0 }, Y{ gt, (long long)H * W, (long long)W, 1, 0 };
        float* maps = c->loss_ws.as<float>();
        gs_launch_loss_forward(X, Y, H, W, lambda_value, maps, maps + maps_floats, loss_terms, s);
        if (grad_pred) {
            GsLossImage G{ grad_pred, (long long)H * W, (long long)W, 1, 0 };
            gs_launch_loss_backward(X, Y, H, W, lambda_value, maps, nullptr, G, s);
        }
    });
}

extern "C" int gs_scale_regulariser(gs_ctx* c, const float* feat, const int8_t* mask, int64_t n, float* out, gs_stream stream_)
{
    if (!c || !out || (n > 0 && (!feat || !mask))) return fail(GS_ERR_INVALID_ARGUMENT, "gs_scale_regulariser: NULL argument");
    if (n < 0) return fail(GS_ERR_INVALID_ARGUMENT, "gs_scale_regulariser: n_points < 0");
    return queued_call(c, stream_, "gs_scale_regulariser", { NEED(c->loss_ws, (size_t)(2 * ((n + 255) / 256) + 16) * sizeof(float)) },
                       [&](hipStream_t s) { gs_launch_reg_value(feat, mask, n, c->loss_ws.as<float>(), out, s); });
}

extern "C" int gs_scale_regulariser_grad(gs_ctx* c, const float* feat, const int8_t* mask, int64_t n, const float* value_and_count,
                                         const float* upstream, float* grad, gs_stream stream_)
{
    if (!c || (n > 0 && (!feat || !mask || !value_and_count || !upstream || !grad)))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_scale_regulariser_grad: NULL argument");
    if (grad && ((uintptr_t)grad & 15u) != 0) return fail(GS_ERR_INVALID_ARGUMENT, "gs_scale_regulariser_grad: grad must be 16-byte aligned");
    return queued_call(c, stream_, "gs_scale_regulariser_grad", {},
                       [&](hipStream_t s) { gs_launch_reg_grad(feat, mask, n, value_and_count, upstream, grad, s); });
}

extern "C" int gs_adam_step(gs_ctx* c, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                            float lr, float beta1, float beta2, float eps, int64_t step, gs_stream stream_)
{
    if (!c || (n > 0 && (!param || !grad || !exp_avg || !exp_avg_sq))) return fail(GS_ERR_INVALID_ARGUMENT, "gs_adam_step: NULL argument");
    if (n < 0 || step < 1) return fail(GS_ERR_INVALID_ARGUMENT, "gs_adam_step: n must be >= 0 and step >= 1");
    return queued_call(c, stream_, "gs_adam_step", {},
                       [&](hipStream_t s) { gs_launch_adam(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, s); });
}

// ---- the row-selective Adam step (include/gs_sparse.h, k_sparse.hip; its row list: gs_touched_rows, gs_api.hip) -----------------
// No host synchronisation and no device-to-host copy: the count stays on the device.
extern "C" int gs_adam_step_rows(gs_ctx* c, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n_rows,
                                 int32_t row_len, const int32_t* ids, const int32_t* count, int64_t max_count,
                                 float lr, float beta1, float beta2, float eps, int64_t step, gs_stream stream_)
{
    if (!c || (n_rows > 0 && max_count > 0 && (!param || !grad || !exp_avg || !exp_avg_sq || !ids || !count)))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_adam_step_rows: NULL argument");
    if (row_len < 1 || step < 1 || n_rows < 0 || max_count < 0)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_adam_step_rows: row_len and step must be >= 1, n_rows and max_count >= 0");
    if (n_rows == 0 || max_count == 0) return GS_OK;
    return queued_call(c, stream_, "gs_adam_step_rows", {}, [&](hipStream_t s) {
        gs_launch_adam_rows(param, grad, exp_avg, exp_avg_sq, n_rows, row_len, ids, count, max_count, lr, beta1, beta2, eps, step, s);
    });
}

// ---- packed rows and their merge (include/gs_exchange.h, k_exchange.hip) -----------------------------------------------------
// No host synchronisation and no device-to-host copy in either: every count stays on the device.
extern "C" int gs_pack_rows(gs_ctx* c, const float* grad_features, const float* grad_pointcloud, int64_t n_rows, const int32_t* ids,
                            const int32_t* count, int64_t max_count, float* packed_out, gs_stream stream_)
{
    if (!c || (n_rows > 0 && max_count > 0 && (!grad_features || !grad_pointcloud || !ids || !count || !packed_out)))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_pack_rows: NULL argument");
    if (n_rows < 0 || max_count < 0 || n_rows > 0x7fffffffll)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_pack_rows: n_rows and max_count must be >= 0, n_rows <= 2^31 - 1");
    if (n_rows == 0 || max_count == 0) return GS_OK;
    if ((uintptr_t)packed_out & 15u) return fail(GS_ERR_INVALID_ARGUMENT, "gs_pack_rows: packed_out must be 16-byte aligned");
    return queued_call(c, stream_, "gs_pack_rows", {},
                       [&](hipStream_t s) { gs_launch_pack_rows(grad_features, grad_pointcloud, n_rows, ids, count, max_count, packed_out, s); });
}

extern "C" int gs_merge_rows(gs_ctx* c, const float* packed, const int32_t* counts, int32_t n_lists, int64_t list_stride, int64_t n_rows,
                             float* grad_features_out, float* grad_pointcloud_out, int32_t* union_ids_out, int64_t union_capacity,
                             int32_t* union_count_out, gs_stream stream_)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "gs_merge_rows: NULL argument");
    if (n_lists < 1 || n_lists > GS_MERGE_MAX_LISTS) return fail(GS_ERR_INVALID_ARGUMENT, "gs_merge_rows: n_lists must be >= 1 and <= 64");
    if (list_stride < 0 || n_rows < 0 || n_rows > 0x7fffffffll - 4096 || list_stride > (int64_t)1 << 40)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_merge_rows: list_stride and n_rows must be >= 0, n_rows <= 2^31 - 2^12");
    const int64_t entries = (int64_t)n_lists * list_stride, max_union = n_rows < entries ? n_rows : entries;
    if (union_capacity < max_union)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_merge_rows: union_capacity must be >= min(n_rows, n_lists * list_stride)");
    if (max_union == 0) {                       // nothing to merge: an empty union
        if (!union_count_out) return GS_OK;
        std::lock_guard<std::mutex> lock(c->mu);
        hipStream_t s;
        if (const int rc = enter_call(c, stream_, &s)) return rc;
        HIP_TRY(hipMemsetAsync(union_count_out, 0, sizeof(int32_t), s));
        return GS_OK;
    }
    if (!packed || !counts || !grad_features_out || !grad_pointcloud_out || !union_ids_out || !union_count_out)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_merge_rows: NULL argument");
    if ((uintptr_t)packed & 15u) return fail(GS_ERR_INVALID_ARGUMENT, "gs_merge_rows: packed must be 16-byte aligned");
    return queued_call(c, stream_, "gs_merge_rows",
                       { NEED(c->merge_tags, gs_merge_tag_bytes(n_rows)), NEED(c->merge_ids, (size_t)entries * sizeof(int32_t)),
                         NEED(c->row_block_totals, (size_t)(gs_rows_blocks((int)n_rows) + 1) * sizeof(uint32_t)) }, [&](hipStream_t s) {
        gs_launch_merge_rows(packed, counts, n_lists, list_stride, n_rows, grad_features_out, grad_pointcloud_out, union_ids_out, union_capacity,
                             union_count_out, c->merge_tags.as<uint8_t>(), c->merge_ids.as<int32_t>(), c->row_block_totals.as<uint32_t>(), s);
    });
}

// ---- exact k nearest neighbours (include/gs_knn.h, k_knn.hip) --------------------------------------------------------------
// Everything is queued on the call's stream; nothing is read back.
extern "C" int gs_knn(gs_ctx* c, const float* xyz, const int8_t* invalid_mask, int64_t n_points, int32_t k, float* d2_out,
                      int32_t* idx_out, gs_stream stream_)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "gs_knn: ctx is NULL");
    if (k < 1 || k > 8) return fail(GS_ERR_INVALID_ARGUMENT, "gs_knn: k must be in [1, 8]");
    if (n_points < 0 || n_points > (int64_t)GS_KNN_MAX_POINTS)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_knn: n_points must be in [0, 2^30]");
    if (n_points > 0 && (!xyz || !d2_out)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_knn: NULL xyz or d2_out with n_points > 0");
    if (n_points == 0) return GS_OK;
    return queued_call(c, stream_, "gs_knn",
                       { NEED(c->knn_sort, gs_knn_sort_bytes(n_points)), NEED(c->knn_hist, gs_knn_hist_bytes(n_points)),
                         NEED(c->knn_points, gs_knn_points_bytes(n_points)), NEED(c->knn_tree, gs_knn_tree_bytes(n_points)) }, [&](hipStream_t s) {
        gs_launch_knn(xyz, invalid_mask, n_points, k, d2_out, idx_out, c->knn_sort.p, c->knn_hist.p, c->knn_points.p, c->knn_tree.p, s);
    });
}

// ---- the scene as a Gaussian mixture (include/gs_mixture.h, k_mixture.hip) ----------------------------------------------------
// Everything is queued on the call's stream; nothing is read back.
static int mixture_call(const char* who, gs_ctx* c, const float* point_cloud, const float* features, const int8_t* invalid_mask,
                        int64_t n_points, const float* queries, int64_t n_q, int fourier, const float* centre, float* out, gs_stream stream_)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, who, "ctx is NULL");
    if (n_points < 0 || n_points > (int64_t)GS_MIXTURE_MAX_POINTS)
        return fail(GS_ERR_INVALID_ARGUMENT, who, "n_points must be in [0, 2^30]");
    if (n_q < 0 || n_q > (int64_t)GS_MIXTURE_MAX_QUERIES)
        return fail(GS_ERR_INVALID_ARGUMENT, who, fourier ? "n_k must be in [0, 2^30]" : "n_x must be in [0, 2^30]");
    if (n_points == 0 || n_q == 0) return GS_OK;
    if (!point_cloud || !features || !queries || !out || (fourier && !centre))
        return fail(GS_ERR_INVALID_ARGUMENT, who, fourier ? "NULL array with n_points > 0 and n_k > 0" : "NULL array with n_points > 0 and n_x > 0");
    return queued_call(c, stream_, who,
                       { NEED(c->mix_records, gs_mix_record_bytes(n_points)), NEED(c->mix_sums, gs_mix_sum_bytes(n_points)),
                         NEED(c->mix_partial, gs_mix_partial_bytes(n_points, n_q)) }, [&](hipStream_t s) {
        gs_launch_mixture(point_cloud, features, invalid_mask, n_points, queries, n_q, fourier, centre, out, c->mix_records.p, c->mix_sums.p,
                          c->mix_partial.p, s);
    });
}

extern "C" int gs_mixture_log_density(gs_ctx* c, const float* point_cloud, const float* point_cloud_features, const int8_t* point_invalid_mask,
                                      int64_t n_points, const float* x, int64_t n_x, float* log_density_out, gs_stream stream_)
{
    return mixture_call("gs_mixture_log_density", c, point_cloud, point_cloud_features, point_invalid_mask, n_points, x, n_x, 0, nullptr,
                        log_density_out, stream_);
}

extern "C" int gs_mixture_fourier(gs_ctx* c, const float* point_cloud, const float* point_cloud_features, const int8_t* point_invalid_mask,
                                  int64_t n_points, const float* k, int64_t n_k, const float* centre, float* re_im_out, gs_stream stream_)
{
    return mixture_call("gs_mixture_fourier", c, point_cloud, point_cloud_features, point_invalid_mask, n_points, k, n_k, 1, centre,
                        re_im_out, stream_);
}

// ---- its gradients (include/gs_mixture_grad.h, k_mixture_grad.hip) ------------------------------------------------------------
static int mixture_grad_call(const char* who, gs_ctx* c, const float* point_cloud, const float* features, const int8_t* invalid_mask,
                             int64_t n_points, const float* queries, int64_t n_q, int fourier, const float* centre, const float* log_density,
                             const float* grad_out, float* grad_point_cloud, float* grad_features, float* grad_x, gs_stream stream_)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, who, "ctx is NULL");
    if (n_points < 0 || n_points > (int64_t)GS_MIXTURE_MAX_POINTS)
        return fail(GS_ERR_INVALID_ARGUMENT, who, "n_points must be in [0, 2^30]");
    if (n_q < 0 || n_q > (int64_t)GS_MIXTURE_MAX_QUERIES)
        return fail(GS_ERR_INVALID_ARGUMENT, who, fourier ? "n_k must be in [0, 2^30]" : "n_x must be in [0, 2^30]");
    if (n_points == 0 || n_q == 0) return GS_OK;
    if (!point_cloud || !features || !queries || !grad_out || !grad_point_cloud || !grad_features || (fourier ? !centre : !log_density))
        return fail(GS_ERR_INVALID_ARGUMENT, who, fourier ? "NULL array with n_points > 0 and n_k > 0" : "NULL array with n_points > 0 and n_x > 0");
    return queued_call(c, stream_, who,
                       { NEED(c->mix_records, gs_mix_record_bytes(n_points)), NEED(c->mix_sums, gs_mix_sum_bytes(n_points)),
                         NEED(c->mixg_queries, gs_mixg_query_bytes(n_q)), NEED(c->mixg_partial, gs_mixg_partial_bytes(n_points, n_q)),
                         NEED(c->mixg_sums, gs_mixg_sum_bytes(n_points, n_q)),
                         NEED(c->mixg_x_partial, fourier ? 0 : gs_mixg_x_partial_bytes(n_points, n_q)) }, [&](hipStream_t s) {
        gs_launch_mixture_grad(point_cloud, features, invalid_mask, n_points, queries, n_q, fourier, centre, log_density, grad_out,
                               grad_point_cloud, grad_features, grad_x, c->mix_records.p, c->mix_sums.p, c->mixg_queries.p, c->mixg_partial.p,
                               c->mixg_sums.p, c->mixg_x_partial.p, s);
    });
}

extern "C" int gs_mixture_log_density_backward(gs_ctx* c, const float* point_cloud, const float* point_cloud_features,
                                               const int8_t* point_invalid_mask, int64_t n_points, const float* x, int64_t n_x,
                                               const float* log_density, const float* grad_log_density, float* grad_point_cloud,
                                               float* grad_features, float* grad_x, gs_stream stream_)
{
    return mixture_grad_call("gs_mixture_log_density_backward", c, point_cloud, point_cloud_features, point_invalid_mask, n_points, x, n_x, 0,
                             nullptr, log_density, grad_log_density, grad_point_cloud, grad_features, grad_x, stream_);
}

extern "C" int gs_mixture_fourier_backward(gs_ctx* c, const float* point_cloud, const float* point_cloud_features,
                                           const int8_t* point_invalid_mask, int64_t n_points, const float* k, int64_t n_k, const float* centre,
                                           const float* grad_re_im, float* grad_point_cloud, float* grad_features, gs_stream stream_)
{
    return mixture_grad_call("gs_mixture_fourier_backward", c, point_cloud, point_cloud_features, point_invalid_mask, n_points, k, n_k, 1,
                             centre, nullptr, grad_re_im, grad_point_cloud, grad_features, nullptr, stream_);
}

// ---- training targets (include/gs_targets.h, k_targets.hip) -------------------------------------------------------------------
// One axis of ATen's _upsample_bilinear2d_aa (align_corners = false) for in >= out, in float64: window and normalised weights of
// every output, the zero weights at either end of a window dropped.  -> the largest tap count.
static int resample_axis(int in, int out, std::vector<int32_t>& start, std::vector<int32_t>& count, std::vector<std::vector<double>>& weights)
{
    const double scale = (double)in / (double)out, support = scale;
    int taps = 0;
    start.resize(out); count.resize(out); weights.resize(out);
    for (int i = 0; i < out; ++i) {
        const double center = scale * (i + 0.5);
        const int64_t lo = std::max<int64_t>((int64_t)(center - support + 0.5), 0);
        const int64_t hi = std::min<int64_t>((int64_t)(center + support + 0.5), in);
        std::vector<double> w;
        double sum = 0.0;
        for (int64_t j = lo; j < hi; ++j) {
            const double x = ((double)j - center + 0.5) / scale;
            w.push_back(std::max(0.0, 1.0 - std::fabs(x)));
            sum += w.back();
        }
        for (double& v : w) v /= sum;
        size_t a = 0, b = w.size();
        while (b - a > 1 && w[b - 1] == 0.0) --b;
        while (b - a > 1 && w[a] == 0.0) ++a;
        start[i] = (int32_t)(lo + (int64_t)a); count[i] = (int32_t)(b - a);
        weights[i].assign(w.begin() + a, w.begin() + b);
        taps = std::max(taps, count[i]);
    }
    return taps;
}

// what k_image_resample relies on: windows inside the input, moving right, at most GS_RS_MAX_TAPS wide, and a tile's span bounded
static bool resample_axis_ok(int in, const std::vector<int32_t>& start, const std::vector<int32_t>& count, int tile)
{
    const int out = (int)start.size();
    for (int i = 0; i < out; ++i) {
        if (count[i] < 1 || count[i] > GS_RS_MAX_TAPS || start[i] < 0 || start[i] + count[i] > in) return false;
        if (i > 0 && (start[i] < start[i - 1] || start[i] + count[i] < start[i - 1] + count[i - 1])) return false;
    }
    for (int i0 = 0; i0 < out; i0 += tile) {
        const int i1 = std::min(out, i0 + tile) - 1;
        if (start[i1] + count[i1] - start[i0] > GS_RS_MAX_SPAN) return false;
    }
    return true;
}

// the cached tables of a geometry, or new ones: made, allocated and queued for upload on s (mutex held, device current)
static int resample_tables(gs_ctx* c, int H_in, int W_in, int h_full, int w_full, hipStream_t s, ResampleTable** out)
{
    for (ResampleTable* rt : c->resample_tables)
        if (rt->H_in == H_in && rt->W_in == W_in && rt->h_full == h_full && rt->w_full == w_full) { *out = rt; return GS_OK; }
    std::vector<int32_t> xs, xc, ys, yc;
    std::vector<std::vector<double>> xw, yw;
    const int tx = resample_axis(W_in, w_full, xs, xc, xw), ty = resample_axis(H_in, h_full, ys, yc, yw);
    if (!resample_axis_ok(W_in, xs, xc, GS_RESAMPLE_TILE_W) || !resample_axis_ok(H_in, ys, yc, GS_RESAMPLE_TILE_H))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_image_resample: the windows of this geometry do not fit the kernel's tile");
    // layout (4-byte words): x start, x count, x weights (w_full * tx), y start, y count, y weights (h_full * ty)
    const size_t words = 2 * (size_t)w_full + (size_t)w_full * tx + 2 * (size_t)h_full + (size_t)h_full * ty;
    ResampleTable* rt = new ResampleTable();
    rt->H_in = H_in; rt->W_in = W_in; rt->h_full = h_full; rt->w_full = w_full;
    rt->host.assign(words * 4, 0);
    int32_t* hi = reinterpret_cast<int32_t*>(rt->host.data());
    float* hf = reinterpret_cast<float*>(rt->host.data());
    size_t o = 0;
    const size_t o_xs = o; for (int i = 0; i < w_full; ++i) hi[o++] = xs[i];
    const size_t o_xc = o; for (int i = 0; i < w_full; ++i) hi[o++] = xc[i];
    const size_t o_xw = o; for (int i = 0; i < w_full; ++i) for (int k = 0; k < tx; ++k) hf[o++] = k < xc[i] ? (float)xw[i][k] : 0.0f;
    const size_t o_ys = o; for (int i = 0; i < h_full; ++i) hi[o++] = ys[i];
    const size_t o_yc = o; for (int i = 0; i < h_full; ++i) hi[o++] = yc[i];
    const size_t o_yw = o; for (int i = 0; i < h_full; ++i) for (int k = 0; k < ty; ++k) hf[o++] = k < yc[i] ? (float)yw[i][k] : 0.0f;
    if (rt->buf.ensure(words * 4, &c->device_bytes) != hipSuccess) { delete rt; return fail(GS_ERR_OUT_OF_MEMORY, "device allocation failed: resample tables"); }
    const hipError_t e = hipMemcpyAsync(rt->buf.p, rt->host.data(), words * 4, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { rt->buf.release(&c->device_bytes); delete rt; return fail(GS_ERR_HIP, std::string("resample tables: ") + hipGetErrorString(e)); }
    const int32_t* di = rt->buf.as<int32_t>();
    const float* df = rt->buf.as<float>();
    rt->ax = GsResampleAxis{ di + o_xs, di + o_xc, df + o_xw, tx };
    rt->ay = GsResampleAxis{ di + o_ys, di + o_yc, df + o_yw, ty };
    if (c->resample_tables.size() >= GS_RESAMPLE_MAX_GEOMETRIES) {       // the oldest goes (hipFree waits for what still reads it)
        ResampleTable* old = c->resample_tables.front();
        c->resample_tables.erase(c->resample_tables.begin());
        old->buf.release(&c->device_bytes);
        delete old;
    }
    c->resample_tables.push_back(rt);
    *out = rt;
    return GS_OK;
}

// gs_image_resample (dst_channels 3) and gs_image_resample_rgba (4, include/gs_targets_rgba.h): the same checks, tables and launch
static int image_resample(const char* who, int dst_channels, gs_ctx* c, const void* src, int32_t src_format, int32_t src_channels, int32_t H_in,
                          int32_t W_in, int64_t src_row_pitch_bytes, int32_t h_full, int32_t w_full, int32_t h_out, int32_t w_out, float* dst,
                          gs_stream stream_)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, who, "ctx is NULL");
    if (src_format != GS_IMAGE_U8_HWC && src_format != GS_IMAGE_F32_CHW) return fail(GS_ERR_INVALID_ARGUMENT, who, "unknown src_format");
    if (src_channels != 4 && (dst_channels == 4 || src_channels != 3))
        return fail(GS_ERR_INVALID_ARGUMENT, who, dst_channels == 4 ? "src_channels must be 4" : "src_channels must be 3 or 4");
    for (int32_t v : { H_in, W_in, h_full, w_full, h_out, w_out })
        if (v < 0 || v > GS_RESAMPLE_MAX_SIZE) return fail(GS_ERR_INVALID_ARGUMENT, who, "every size must be in [0, 32768]");
    if (h_out > h_full || w_out > w_full) return fail(GS_ERR_INVALID_ARGUMENT, who, "the crop (h_out, w_out) exceeds the resize (h_full, w_full)");
    if (src_format == GS_IMAGE_U8_HWC ? src_row_pitch_bytes < (int64_t)W_in * src_channels : src_row_pitch_bytes != (int64_t)W_in * 4)
        return fail(GS_ERR_INVALID_ARGUMENT, who, "src_row_pitch_bytes must be >= W_in * src_channels (uint8), W_in * 4 (f32)");
    if (h_out == 0 || w_out == 0) return GS_OK;
    if (!src || !dst) return fail(GS_ERR_INVALID_ARGUMENT, who, "NULL src or dst");
    if (H_in < h_full || W_in < w_full || (int64_t)H_in > (int64_t)GS_RESAMPLE_MAX_SCALE * h_full || (int64_t)W_in > (int64_t)GS_RESAMPLE_MAX_SCALE * w_full)
        return fail(GS_ERR_INVALID_ARGUMENT, who, "the scale in / out must be in [1, 8] on both axes (no upscaling)");
    std::lock_guard<std::mutex> lock(c->mu);
    hipStream_t s;
    int rc;
    if ((rc = enter_call(c, stream_, &s)) != GS_OK) return rc;
    ResampleTable* rt = nullptr;
    if ((rc = resample_tables(c, H_in, W_in, h_full, w_full, s, &rt)) != GS_OK) return rc;
    gs_launch_image_resample(src, src_format, src_channels, H_in, W_in, src_row_pitch_bytes, rt->ax, rt->ay, h_out, w_out, dst, dst_channels, s);
    HIP_TRY(hipGetLastError());
    return GS_OK;
}

extern "C" int gs_image_resample(gs_ctx* c, const void* src, int32_t src_format, int32_t src_channels, int32_t H_in, int32_t W_in,
                                 int64_t src_row_pitch_bytes, int32_t h_full, int32_t w_full, int32_t h_out, int32_t w_out, float* dst,
                                 gs_stream stream_)
{
    return image_resample("gs_image_resample", 3, c, src, src_format, src_channels, H_in, W_in, src_row_pitch_bytes, h_full, w_full, h_out, w_out,
                          dst, stream_);
}

extern "C" int gs_image_resample_rgba(gs_ctx* c, const void* src, int32_t src_format, int32_t src_channels, int32_t H_in, int32_t W_in,
                                      int64_t src_row_pitch_bytes, int32_t h_full, int32_t w_full, int32_t h_out, int32_t w_out, float* dst,
                                      gs_stream stream_)
{
    return image_resample("gs_image_resample_rgba", 4, c, src, src_format, src_channels, H_in, W_in, src_row_pitch_bytes, h_full, w_full, h_out,
                          w_out, dst, stream_);
}

// ---- baking a placed scene (k_compose.hip) ----------------------------------------------------------------------------
static bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

extern "C" int gs_scene_bake(gs_ctx* c, const float* xyz_in, const float* features_in, int64_t n, const float* q_A, const float* t_A,
                             float scale, const float* sh_matrices, float* xyz_out, float* features_out, int64_t row_offset,
                             gs_stream stream_)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "gs_scene_bake: ctx is NULL");
    if (n < 0 || row_offset < 0 || n > INT32_MAX || row_offset > INT32_MAX || n + row_offset > INT32_MAX)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_scene_bake: n and row_offset must not be negative, and row_offset + n below 2^31");
    if (!q_A || !t_A || !sh_matrices) return fail(GS_ERR_INVALID_ARGUMENT, "gs_scene_bake: NULL q_A, t_A or sh_matrices");
    if (!std::isfinite(scale) || !(scale > 0.0f)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_scene_bake: scale must be finite and > 0");
    const double qn = std::sqrt((double)q_A[0] * q_A[0] + (double)q_A[1] * q_A[1] + (double)q_A[2] * q_A[2] + (double)q_A[3] * q_A[3]);
    if (!std::isfinite(qn) || !(qn > 0.0)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_scene_bake: q_A must have a finite norm > 0");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(t_A[k])) return fail(GS_ERR_INVALID_ARGUMENT, "gs_scene_bake: t_A must be finite");
    for (int k = 0; k < GS_BAKE_SH_FLOATS; ++k)
        if (!std::isfinite(sh_matrices[k])) return fail(GS_ERR_INVALID_ARGUMENT, "gs_scene_bake: sh_matrices must be finite");
    if (n == 0) return GS_OK;
    if (!xyz_in || !features_in || !xyz_out || !features_out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_scene_bake: NULL array");
    const size_t xyz_bytes = (size_t)n * 3 * sizeof(float), feat_bytes = (size_t)n * GS_BAKE_FEATURES * sizeof(float);
    const float* xyz_w = xyz_out + row_offset * 3;
    const float* feat_w = features_out + row_offset * GS_BAKE_FEATURES;
    if (ranges_overlap(xyz_in, xyz_bytes, xyz_w, xyz_bytes) || ranges_overlap(xyz_in, xyz_bytes, feat_w, feat_bytes) ||
        ranges_overlap(features_in, feat_bytes, xyz_w, xyz_bytes) || ranges_overlap(features_in, feat_bytes, feat_w, feat_bytes) ||
        ranges_overlap(xyz_w, xyz_bytes, feat_w, feat_bytes))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_scene_bake: the rows read and the rows written overlap (the call runs out of place)");
    // the transform in float64, rounded once
    GsBakeTransform A;
    const double x = q_A[0] / qn, y = q_A[1] / qn, z = q_A[2] / qn, w = q_A[3] / qn, s = (double)scale;
    const double R[9] = { 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                          2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                          2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y) };
    for (int k = 0; k < 9; ++k) A.m[k] = (float)(s * R[k]);
    for (int k = 0; k < 3; ++k) A.t[k] = t_A[k];
    A.q[0] = (float)x; A.q[1] = (float)y; A.q[2] = (float)z; A.q[3] = (float)w;
    A.log_scale = (float)std::log(s);
    std::memcpy(A.sh, sh_matrices, sizeof(A.sh));
    return queued_call(c, stream_, "gs_scene_bake", {},
                       [&](hipStream_t st) { gs_launch_scene_bake(xyz_in, features_in, n, A, xyz_out, features_out, row_offset, st); });
}

// ---- frames out (k_frames.hip) ------------------------------------------------------------------------------------------
extern "C" int gs_frame_to_u8(gs_ctx* c, const float* src, int32_t mode, int32_t h, int32_t w, uint8_t* dst, int64_t dst_row_pitch_bytes,
                              const uint8_t* gt, int32_t gt_channels, int64_t gt_row_pitch_bytes, int64_t* sse, gs_stream stream_)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "gs_frame_to_u8: ctx is NULL");
    if (mode != GS_FRAME_RGB_TRUNC && mode != GS_FRAME_RGB_ROUND && mode != GS_FRAME_DEPTH_CMAP)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_frame_to_u8: unknown mode");
    if (h < 0 || w < 0 || h > GS_FRAME_MAX_SIZE || w > GS_FRAME_MAX_SIZE)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_frame_to_u8: every size must be in [0, 32768]");
    if (dst_row_pitch_bytes < (int64_t)3 * w) return fail(GS_ERR_INVALID_ARGUMENT, "gs_frame_to_u8: dst_row_pitch_bytes must be >= 3 * w");
    if (gt) {
        if (gt_channels != 3 && gt_channels != 4) return fail(GS_ERR_INVALID_ARGUMENT, "gs_frame_to_u8: gt_channels must be 3 or 4");
        if (gt_row_pitch_bytes < (int64_t)w * gt_channels) return fail(GS_ERR_INVALID_ARGUMENT, "gs_frame_to_u8: gt_row_pitch_bytes must be >= w * gt_channels");
        if (!sse) return fail(GS_ERR_INVALID_ARGUMENT, "gs_frame_to_u8: a ground truth needs the sse word");
    } else if (sse) {
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_frame_to_u8: the sse word needs a ground truth");
    }
    if (h == 0 || w == 0) return GS_OK;
    if (!src || !dst) return fail(GS_ERR_INVALID_ARGUMENT, "gs_frame_to_u8: NULL src or dst");
    return queued_call(c, stream_, "gs_frame_to_u8", {}, [&](hipStream_t s) {
        gs_launch_frame_to_u8(src, mode, h, w, dst, dst_row_pitch_bytes, gt, gt_channels, gt_row_pitch_bytes, sse, s);
    });
}

// ---- meshes from a scene (k_fusion.hip) --------------------------------------------------------------------------------------
static bool positive_finite(float v) { return std::isfinite(v) && v > 0.0f; }

// the checks the three calls share on (nx, ny, nz, origin, step); *n_out = nx ny nz
static int fusion_grid(const char* who, int32_t nx, int32_t ny, int32_t nz, const float* origin, const float* step, const char* step_name,
                       int64_t* n_out)
{
    if (nx < 0 || ny < 0 || nz < 0) return fail(GS_ERR_INVALID_ARGUMENT, who, "a dimension is negative");
    // each factor is below 2^31: the product of two fits 63 bits, and is compared before the third enters
    const int64_t nxy = (int64_t)nx * ny;
    if (nxy > GS_FUSION_MAX_VOXELS || (nz > 0 && nxy > GS_FUSION_MAX_VOXELS / nz))
        return fail(GS_ERR_INVALID_ARGUMENT, who, "nx * ny * nz exceeds GS_FUSION_MAX_VOXELS (2^30)");
    for (int a = 0; a < 3; ++a) {
        if (!positive_finite(step[a])) return fail(GS_ERR_INVALID_ARGUMENT, who, std::string(step_name) + " must be finite and > 0");
        if (!std::isfinite(origin[a])) return fail(GS_ERR_INVALID_ARGUMENT, who, "origin must be finite");
    }
    *n_out = nxy * nz;
    return GS_OK;
}

extern "C" int gs_tsdf_integrate(gs_ctx* c, const gs_tsdf_volume* vol, const gs_tsdf_view* views, int32_t n_views, gs_stream stream_)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "gs_tsdf_integrate: ctx is NULL");
    if (!vol) return fail(GS_ERR_INVALID_ARGUMENT, "gs_tsdf_integrate: volume is NULL");
    if (n_views < 0) return fail(GS_ERR_INVALID_ARGUMENT, "gs_tsdf_integrate: n_views is negative");
    int64_t n = 0;
    if (const int rc = fusion_grid("gs_tsdf_integrate", vol->nx, vol->ny, vol->nz, vol->origin, vol->voxel, "voxel", &n)) return rc;
    if (!positive_finite(vol->trunc)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_tsdf_integrate: trunc must be finite and > 0");
    if (!positive_finite(vol->max_weight)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_tsdf_integrate: max_weight must be finite and > 0");
    if (!std::isfinite(vol->min_alpha) || !std::isfinite(vol->near)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_tsdf_integrate: min_alpha and near must be finite");
    if (n > 0 && (!vol->tsdf || !vol->weight)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_tsdf_integrate: NULL tsdf or weight");
    if (n_views > 0 && !views) return fail(GS_ERR_INVALID_ARGUMENT, "gs_tsdf_integrate: views is NULL");
    for (int32_t v = 0; v < n_views; ++v) {
        const gs_tsdf_view& V = views[v];
        if (!V.depth) return fail(GS_ERR_INVALID_ARGUMENT, "gs_tsdf_integrate: view " + std::to_string(v) + " has a NULL depth");
        if (V.h < 0 || V.w < 0 || V.h > GS_FUSION_MAX_IMAGE_SIZE || V.w > GS_FUSION_MAX_IMAGE_SIZE)
            return fail(GS_ERR_INVALID_ARGUMENT, "gs_tsdf_integrate: view " + std::to_string(v) + ": h and w must be in [0, 32768]");
        bool finite = std::isfinite(V.fx) && std::isfinite(V.fy) && std::isfinite(V.cx) && std::isfinite(V.cy);
        for (int k = 0; k < 12; ++k) finite = finite && std::isfinite(V.m[k / 4][k % 4]);
        if (!finite) return fail(GS_ERR_INVALID_ARGUMENT, "gs_tsdf_integrate: view " + std::to_string(v) + ": fx, fy, cx, cy and m must be finite");
    }
    if (n == 0 || n_views == 0) return GS_OK;
    return queued_call(c, stream_, "gs_tsdf_integrate", {}, [&](hipStream_t s) { gs_launch_tsdf_integrate(*vol, views, n_views, s); });
}

static int iso_volume_checks(const char* who, gs_ctx* c, const gs_iso_volume* vol, const void* cell_ws, const void* block_ws, int64_t* n_out)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, who, "ctx is NULL");
    if (!vol) return fail(GS_ERR_INVALID_ARGUMENT, who, "volume is NULL");
    if (const int rc = fusion_grid(who, vol->nx, vol->ny, vol->nz, vol->origin, vol->spacing, "spacing", n_out)) return rc;
    if (!std::isfinite(vol->level)) return fail(GS_ERR_INVALID_ARGUMENT, who, "level must be finite");
    if (*n_out > 0 && !vol->values) return fail(GS_ERR_INVALID_ARGUMENT, who, "NULL values");
    if (*n_out > 0 && (!cell_ws || !block_ws)) return fail(GS_ERR_INVALID_ARGUMENT, who, "NULL work buffer");
    return GS_OK;
}

extern "C" int gs_isosurface_plan(gs_ctx* c, const gs_iso_volume* vol, void* cell_ws, void* block_ws, int64_t* totals, gs_stream stream_)
{
    int64_t n = 0;
    if (const int rc = iso_volume_checks("gs_isosurface_plan", c, vol, cell_ws, block_ws, &n)) return rc;
    if (n == 0) return GS_OK;
    if (!totals) return fail(GS_ERR_INVALID_ARGUMENT, "gs_isosurface_plan: NULL totals");
    return queued_call(c, stream_, "gs_isosurface_plan", {}, [&](hipStream_t s) { gs_launch_iso_plan(*vol, cell_ws, block_ws, totals, s); });
}

extern "C" int gs_isosurface_emit(gs_ctx* c, const gs_iso_volume* vol, const void* cell_ws, const void* block_ws, void* voxel_ws,
                                  int64_t n_vertices, int64_t n_faces, float* vertices, float* colours, int32_t* faces, gs_stream stream_)
{
    int64_t n = 0;
    if (const int rc = iso_volume_checks("gs_isosurface_emit", c, vol, cell_ws, block_ws, &n)) return rc;
    if (n_vertices < 0 || n_faces < 0 || n_vertices > INT32_MAX || n_faces > INT32_MAX)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_isosurface_emit: n_vertices and n_faces must be in [0, 2^31 - 1]");
    if (n == 0 || (n_vertices == 0 && n_faces == 0)) return GS_OK;
    if (!voxel_ws) return fail(GS_ERR_INVALID_ARGUMENT, "gs_isosurface_emit: NULL work buffer");
    if ((n_vertices > 0 && !vertices) || (n_faces > 0 && !faces)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_isosurface_emit: NULL vertices or faces");
    return queued_call(c, stream_, "gs_isosurface_emit", {}, [&](hipStream_t s) {
        gs_launch_iso_emit(*vol, cell_ws, block_ws, voxel_ws, n_vertices, n_faces, vertices, colours, faces, s);
    });
}


// ---- fixed-budget densification (k_mcmc.hip) ------------------------------------------------------------------------------
extern "C" int64_t gs_mcmc_scratch_bytes(int64_t n_points) { return n_points < 0 ? 0 : (int64_t)gs_mcmc_scratch_size(n_points); }

static int mcmc_rows_check(const char* who, gs_ctx* c, int64_t N)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, who, "ctx is NULL");
    if (N < 0 || N > INT32_MAX) return fail(GS_ERR_INVALID_ARGUMENT, who, "n_points must be in [0, 2^31)");
    return GS_OK;
}

extern "C" int gs_mcmc_noise(gs_ctx* c, float* point_cloud, const float* features, const int8_t* mask, int64_t N, float noise_scale,
                             float gate_k, float gate_x0, uint64_t seed, uint32_t step_index, gs_stream stream_)
{
    if (const int rc = mcmc_rows_check("gs_mcmc_noise", c, N)) return rc;
    if (N > 0 && (!point_cloud || !features || !mask)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_mcmc_noise: NULL array");
    if (((uintptr_t)features & 15u) != 0) return fail(GS_ERR_INVALID_ARGUMENT, "gs_mcmc_noise: features must be 16-byte aligned");
    if (!std::isfinite(noise_scale) || !std::isfinite(gate_k) || !std::isfinite(gate_x0))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_mcmc_noise: noise_scale, gate_k and gate_x0 must be finite");
    if (N == 0) return GS_OK;
    return queued_call(c, stream_, "gs_mcmc_noise", {}, [&](hipStream_t s) {
        gs_launch_mcmc_noise(point_cloud, features, mask, N, noise_scale, gate_k, gate_x0, seed, step_index, s);
    });
}

extern "C" int gs_mcmc_regulariser(gs_ctx* c, const float* features, const int8_t* mask, int64_t N, float lambda_opacity, float lambda_scale,
                                   const float* upstream, float* grad_features, float* value_and_count, gs_stream stream_)
{
    if (const int rc = mcmc_rows_check("gs_mcmc_regulariser", c, N)) return rc;
    if (N > 0 && (!features || !mask)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_mcmc_regulariser: NULL array");
    if ((((uintptr_t)features | (uintptr_t)grad_features) & 15u) != 0)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_mcmc_regulariser: features and grad_features must be 16-byte aligned");
    if (!std::isfinite(lambda_opacity) || !std::isfinite(lambda_scale))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_mcmc_regulariser: lambda_opacity and lambda_scale must be finite");
    return queued_call(c, stream_, "gs_mcmc_regulariser", { NEED(c->mcmc_ws, gs_mcmc_reg_ws_size(N)) }, [&](hipStream_t s) {
        gs_launch_mcmc_regulariser(features, mask, N, lambda_opacity, lambda_scale, upstream, grad_features, value_and_count, c->mcmc_ws.p, s);
    });
}

extern "C" int gs_mcmc_relocate(gs_ctx* c, const gs_density_scene* scene, float* features_exp_avg, float* features_exp_avg_sq,
                                float* point_cloud_exp_avg, float* point_cloud_exp_avg_sq, const gs_mcmc_config* cfg,
                                const gs_mcmc_plan* plan, uint64_t seed, uint32_t call_index, gs_stream stream_)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "gs_mcmc_relocate: ctx is NULL");
    if (!scene || !cfg || !plan || !plan->counts) return fail(GS_ERR_INVALID_ARGUMENT, "gs_mcmc_relocate: NULL scene, config, plan or plan->counts");
    const int64_t N = scene->n_points;
    if (const int rc = mcmc_rows_check("gs_mcmc_relocate", c, N)) return rc;
    if (plan->n_points < N) return fail(GS_ERR_INVALID_ARGUMENT, "gs_mcmc_relocate: plan is smaller than the scene");
    if (N > 0 && (!scene->point_cloud || !scene->point_cloud_features || !scene->point_invalid_mask || !scene->point_object_id))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_mcmc_relocate: NULL scene array");
    if (N > 0 && (!plan->source_of || !plan->dest_row || !plan->multiplicity || !plan->scratch))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_mcmc_relocate: NULL plan array");
    if ((((uintptr_t)scene->point_cloud_features | (uintptr_t)features_exp_avg | (uintptr_t)features_exp_avg_sq) & 15u) != 0 ||
        ((uintptr_t)plan->scratch & 7u) != 0)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_mcmc_relocate: features and their moments must be 16-byte aligned, scratch 8-byte aligned");
    if (cfg->n_max < 1 || cfg->n_max > GS_MCMC_N_MAX) return fail(GS_ERR_INVALID_ARGUMENT, "gs_mcmc_relocate: n_max must be in [1, 51]");
    if (cfg->grow_permille < 0 || cfg->cap_max < 0) return fail(GS_ERR_INVALID_ARGUMENT, "gs_mcmc_relocate: grow_permille and cap_max must be >= 0");
    if (std::isnan(cfg->min_opacity_logit)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_mcmc_relocate: min_opacity_logit is NaN");
    float* const moments[4] = { features_exp_avg, features_exp_avg_sq, point_cloud_exp_avg, point_cloud_exp_avg_sq };
    return queued_call(c, stream_, "gs_mcmc_relocate", {},
                       [&](hipStream_t s) { gs_launch_mcmc_relocate(*scene, moments, *cfg, *plan, seed, call_index, s); });
}

// ---- per-view exposure compensation (include/gs_appearance.h, k_appearance.hip) ---------------------------------------------
static int appearance_check(const char* who, gs_ctx* c, const gs_loss_image* image, int32_t H, int32_t W)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, who, "ctx is NULL");
    if (!image || !image->data) return fail(GS_ERR_INVALID_ARGUMENT, who, "NULL image");
    return image_size_check(who, H, W, GS_APPEARANCE_MAX_PIXELS);
}

extern "C" int gs_appearance_apply(gs_ctx* c, const gs_loss_image* image, const float* transform, int32_t H, int32_t W,
                                   const gs_loss_image* corrected, gs_stream stream_)
{
    if (const int rc = appearance_check("gs_appearance_apply", c, image, H, W)) return rc;
    if (!transform) return fail(GS_ERR_INVALID_ARGUMENT, "gs_appearance_apply: transform is NULL");
    if (!corrected || !corrected->data) return fail(GS_ERR_INVALID_ARGUMENT, "gs_appearance_apply: NULL corrected image");
    return queued_call(c, stream_, "gs_appearance_apply", {},
                       [&](hipStream_t s) { gs_launch_appearance_apply(loss_image(image, 0), transform, H, W, loss_image(corrected, 0), s); });
}

extern "C" int gs_appearance_backward(gs_ctx* c, const gs_loss_image* image, const gs_loss_image* grad_corrected, const float* transform,
                                      int32_t H, int32_t W, const gs_loss_image* grad_image, float* grad_transform, gs_stream stream_)
{
    if (const int rc = appearance_check("gs_appearance_backward", c, image, H, W)) return rc;
    if (!grad_corrected || !grad_corrected->data) return fail(GS_ERR_INVALID_ARGUMENT, "gs_appearance_backward: NULL grad_corrected");
    if (!transform) return fail(GS_ERR_INVALID_ARGUMENT, "gs_appearance_backward: transform is NULL");
    const bool want_image = grad_image && grad_image->data;
    if (!want_image && !grad_transform) return fail(GS_ERR_INVALID_ARGUMENT, "gs_appearance_backward: grad_image and grad_transform are both NULL");
    // (the block sums only when the parameter gradient is wanted)
    return queued_call(c, stream_, "gs_appearance_backward", { NEED(c->appearance_ws, grad_transform ? gs_appearance_ws_size(H, W) : 0) },
                       [&](hipStream_t s) {
        const GsLossImage none{ nullptr, 0, 0, 0, 0 };
        gs_launch_appearance_backward(loss_image(image, 0), loss_image(grad_corrected, 0), transform, H, W,
                                      want_image ? loss_image(grad_image, 0) : none, grad_transform, c->appearance_ws.p, s);
    });
}

extern "C" int gs_appearance_moments(gs_ctx* c, const gs_loss_image* image, const gs_loss_image* target, const float* pixel_weight,
                                     int32_t H, int32_t W, double* moments, gs_stream stream_)
{
    if (const int rc = appearance_check("gs_appearance_moments", c, image, H, W)) return rc;
    if (!target || !target->data) return fail(GS_ERR_INVALID_ARGUMENT, "gs_appearance_moments: NULL target");
    if (!moments || ((uintptr_t)moments & 7u) != 0) return fail(GS_ERR_INVALID_ARGUMENT, "gs_appearance_moments: moments must be 8-byte aligned and not NULL");
    return queued_call(c, stream_, "gs_appearance_moments", { NEED(c->appearance_ws, gs_appearance_ws_size(H, W)) }, [&](hipStream_t s) {
        gs_launch_appearance_moments(loss_image(image, 0), loss_image(target, 0), pixel_weight, H, W, moments, c->appearance_ws.p, s);
    });
}

// ---- a background behind the splats (include/gs_background.h, k_background.hip) ---------------------------------------------
static int background_check(const char* who, gs_ctx* c, const float* coef, int32_t bands, const float* q, const float* intrinsics, int32_t H,
                            int32_t W)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, who, "ctx is NULL");
    if (!coef) return fail(GS_ERR_INVALID_ARGUMENT, who, "coef is NULL");
    if (bands < 0 || bands > GS_BACKGROUND_MAX_BANDS) return fail(GS_ERR_INVALID_ARGUMENT, who, "bands must be 0 .. 3");
    if (bands > 0 && (!q || !intrinsics)) return fail(GS_ERR_INVALID_ARGUMENT, who, "bands > 0 needs q and intrinsics");
    return image_size_check(who, H, W, GS_BACKGROUND_MAX_PIXELS);
}

extern "C" int gs_background_composite(gs_ctx* c, const gs_loss_image* image, const float* alpha, const float* coef, int32_t bands,
                                       const float* q, const float* intrinsics, int32_t H, int32_t W, int32_t flags,
                                       const gs_loss_image* out, gs_stream stream_)
{
    if (const int rc = background_check("gs_background_composite", c, coef, bands, q, intrinsics, H, W)) return rc;
    if ((flags & ~(GS_BACKGROUND_STRAIGHT | GS_BACKGROUND_COLOURS_ONLY)) != 0 || flags == (GS_BACKGROUND_STRAIGHT | GS_BACKGROUND_COLOURS_ONLY))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_background_composite: flags must be 0, GS_BACKGROUND_STRAIGHT or GS_BACKGROUND_COLOURS_ONLY");
    const bool colours_only = (flags & GS_BACKGROUND_COLOURS_ONLY) != 0;
    if (!colours_only && (!image || !image->data)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_background_composite: NULL image");
    if (!colours_only && !alpha) return fail(GS_ERR_INVALID_ARGUMENT, "gs_background_composite: alpha is NULL");
    if (!out || !out->data) return fail(GS_ERR_INVALID_ARGUMENT, "gs_background_composite: NULL out image");
    return queued_call(c, stream_, "gs_background_composite", {}, [&](hipStream_t s) {
        const GsLossImage none{ nullptr, 0, 0, 0, 0 };
        gs_launch_background_composite(colours_only ? none : loss_image(image, 0), colours_only ? nullptr : alpha, coef, bands, q, intrinsics, H, W,
                                       flags, loss_image(out, 0), s);
    });
}

extern "C" int gs_background_backward(gs_ctx* c, const gs_loss_image* grad_out, const float* alpha, const float* coef, int32_t bands,
                                      const float* q, const float* intrinsics, int32_t H, int32_t W, float* grad_alpha, float* grad_coef,
                                      gs_stream stream_)
{
    if (const int rc = background_check("gs_background_backward", c, coef, bands, q, intrinsics, H, W)) return rc;
    if (!grad_out || !grad_out->data) return fail(GS_ERR_INVALID_ARGUMENT, "gs_background_backward: NULL grad_out");
    if (!alpha) return fail(GS_ERR_INVALID_ARGUMENT, "gs_background_backward: alpha is NULL");
    if (!grad_alpha && !grad_coef) return fail(GS_ERR_INVALID_ARGUMENT, "gs_background_backward: grad_alpha and grad_coef are both NULL");
    // (the block sums only when the coefficients' gradient is wanted)
    return queued_call(c, stream_, "gs_background_backward", { NEED(c->background_ws, grad_coef ? gs_background_ws_size(H, W) : 0) },
                       [&](hipStream_t s) {
        gs_launch_background_backward(loss_image(grad_out, 0), alpha, coef, bands, q, intrinsics, H, W, grad_alpha, grad_coef,
                                      c->background_ws.p, s);
    });
}

// ---- the 3D smoothing filter (include/gs_filter3d.h, k_filter3d.hip) ------------------------------------------------------------
static int filter3d_rows_check(const char* who, gs_ctx* c, int64_t n)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, who, "ctx is NULL");
    if (n < 0 || n > (int64_t)GS_FILTER3D_MAX_POINTS) return fail(GS_ERR_INVALID_ARGUMENT, who, "n_points must be in [0, 2^30]");
    return GS_OK;
}

static int filter3d_k_check(const char* who, float k)
{
    if (!std::isfinite(k) || k < 0.0f) return fail(GS_ERR_INVALID_ARGUMENT, who, "k must be finite and >= 0");
    return GS_OK;
}

extern "C" int gs_filter3d_rate(gs_ctx* c, const float* point_cloud, const int8_t* mask, int64_t n, const float* views, int32_t n_views,
                                int32_t W, int32_t H, float near, float margin, float* rate_out, gs_stream stream_)
{
    if (const int rc = filter3d_rows_check("gs_filter3d_rate", c, n)) return rc;
    if (n_views < 0 || n_views > GS_FILTER3D_MAX_VIEWS) return fail(GS_ERR_INVALID_ARGUMENT, "gs_filter3d_rate: n_views must be in [0, 2^20]");
    if (W < 1 || H < 1) return fail(GS_ERR_INVALID_ARGUMENT, "gs_filter3d_rate: W and H must be >= 1");
    if (!std::isfinite(near) || !(near > 0.0f)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_filter3d_rate: near must be finite and > 0");
    if (!std::isfinite(margin) || margin < 0.0f) return fail(GS_ERR_INVALID_ARGUMENT, "gs_filter3d_rate: margin must be finite and >= 0");
    if (n == 0) return GS_OK;
    if (!point_cloud || !mask || !rate_out || (n_views > 0 && !views)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_filter3d_rate: NULL array");
    return queued_call(c, stream_, "gs_filter3d_rate", { NEED(c->filter3d_ws, gs_filter3d_ws_size()) }, [&](hipStream_t s) {
        gs_launch_filter3d_rate(point_cloud, mask, n, views, n_views, W, H, near, margin, rate_out, c->filter3d_ws.p, s);
    });
}

extern "C" int gs_filter3d_apply(gs_ctx* c, float* features, const float* rate, int64_t n, float k, float* features_out, gs_stream stream_)
{
    if (const int rc = filter3d_rows_check("gs_filter3d_apply", c, n)) return rc;
    if (const int rc = filter3d_k_check("gs_filter3d_apply", k)) return rc;
    if (n == 0) return GS_OK;
    if (!features || !rate || !features_out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_filter3d_apply: NULL array");
    if ((((uintptr_t)features | (uintptr_t)features_out) & 15u) != 0)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_filter3d_apply: features and features_out must be 16-byte aligned");
    const size_t bytes = (size_t)n * GS_FILTER3D_FEATURES * sizeof(float);
    if (ranges_overlap(features, bytes, features_out, bytes))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_filter3d_apply: features_out overlaps features (the call runs out of place)");
    return queued_call(c, stream_, "gs_filter3d_apply", {}, [&](hipStream_t s) { gs_launch_filter3d_apply(features, rate, n, k, features_out, s); });
}

extern "C" int gs_filter3d_apply_backward(gs_ctx* c, const float* grad_out, const float* features, const float* rate, int64_t n, float k,
                                          float* grad_in, gs_stream stream_)
{
    if (const int rc = filter3d_rows_check("gs_filter3d_apply_backward", c, n)) return rc;
    if (const int rc = filter3d_k_check("gs_filter3d_apply_backward", k)) return rc;
    if (n == 0) return GS_OK;
    if (!grad_out || !features || !rate || !grad_in) return fail(GS_ERR_INVALID_ARGUMENT, "gs_filter3d_apply_backward: NULL array");
    if ((((uintptr_t)grad_out | (uintptr_t)features | (uintptr_t)grad_in) & 15u) != 0)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_filter3d_apply_backward: grad_out, features and grad_in must be 16-byte aligned");
    const size_t bytes = (size_t)n * GS_FILTER3D_FEATURES * sizeof(float);
    if ((grad_in != grad_out && ranges_overlap(grad_out, bytes, grad_in, bytes)) || ranges_overlap(features, bytes, grad_in, bytes))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_filter3d_apply_backward: grad_in overlaps grad_out (other than being it) or features");
    return queued_call(c, stream_, "gs_filter3d_apply_backward", {},
                       [&](hipStream_t s) { gs_launch_filter3d_backward(grad_out, features, rate, n, k, grad_in, s); });
}

// ---- per-view bilateral grids (include/gs_bilateral.h, k_bilateral.hip)-----------------------------------------------------
static int bilateral_grid_check(const char* who, gs_ctx* c, const float* grid, int32_t Gx, int32_t Gy, int32_t L)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, who, "ctx is NULL");
    if (!grid || ((uintptr_t)grid & 15u) != 0) return fail(GS_ERR_INVALID_ARGUMENT, who, "grid must be 16-byte aligned and not NULL");
    if (Gx < GS_BILATERAL_MIN_GRID || Gx > GS_BILATERAL_MAX_XY || Gy < GS_BILATERAL_MIN_GRID || Gy > GS_BILATERAL_MAX_XY ||
        L < GS_BILATERAL_MIN_GRID || L > GS_BILATERAL_MAX_L)
        return fail(GS_ERR_INVALID_ARGUMENT, who, "grid dimensions outside their limits");
    return GS_OK;
}

static int bilateral_check(const char* who, gs_ctx* c, const gs_loss_image* image, const float* grid, int32_t Gx, int32_t Gy, int32_t L,
                           int32_t H, int32_t W)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, who, "ctx is NULL");
    if (!image || !image->data) return fail(GS_ERR_INVALID_ARGUMENT, who, "NULL image");
    if (const int rc = bilateral_grid_check(who, c, grid, Gx, Gy, L)) return rc;
    return image_size_check(who, H, W, GS_BILATERAL_MAX_PIXELS);
}

extern "C" int gs_bilateral_slice(gs_ctx* c, const gs_loss_image* image, const float* grid, int32_t Gx, int32_t Gy, int32_t L, int32_t H,
                                  int32_t W, const gs_loss_image* corrected, gs_stream stream_)
{
    if (const int rc = bilateral_check("gs_bilateral_slice", c, image, grid, Gx, Gy, L, H, W)) return rc;
    if (!corrected || !corrected->data) return fail(GS_ERR_INVALID_ARGUMENT, "gs_bilateral_slice: NULL corrected image");
    return queued_call(c, stream_, "gs_bilateral_slice", {}, [&](hipStream_t s) {
        gs_launch_bilateral_slice(loss_image(image, 0), grid, Gx, Gy, L, H, W, loss_image(corrected, 0), s);
    });
}

extern "C" int gs_bilateral_slice_backward(gs_ctx* c, const gs_loss_image* image, const gs_loss_image* grad_corrected, const float* grid,
                                           int32_t Gx, int32_t Gy, int32_t L, int32_t H, int32_t W, const gs_loss_image* grad_image,
                                           float* grad_grid, gs_stream stream_)
{
    if (const int rc = bilateral_check("gs_bilateral_slice_backward", c, image, grid, Gx, Gy, L, H, W)) return rc;
    if (!grad_corrected || !grad_corrected->data) return fail(GS_ERR_INVALID_ARGUMENT, "gs_bilateral_slice_backward: NULL grad_corrected");
    const bool want_image = grad_image && grad_image->data;
    if (!want_image && !grad_grid) return fail(GS_ERR_INVALID_ARGUMENT, "gs_bilateral_slice_backward: grad_image and grad_grid are both NULL");
    // (the block sums only when the parameter gradient is wanted)
    return queued_call(c, stream_, "gs_bilateral_slice_backward", { NEED(c->bilateral_ws, grad_grid ? gs_bilateral_ws_size(Gx, Gy, L) : 0) },
                       [&](hipStream_t s) {
        const GsLossImage none{ nullptr, 0, 0, 0, 0 };
        gs_launch_bilateral_backward(loss_image(image, 0), loss_image(grad_corrected, 0), grid, Gx, Gy, L, H, W,
                                     want_image ? loss_image(grad_image, 0) : none, grad_grid, c->bilateral_ws.p, s);
    });
}

extern "C" int gs_bilateral_tv(gs_ctx* c, const float* grid, int32_t Gx, int32_t Gy, int32_t L, float weight, float* grad_grid, float* value,
                               gs_stream stream_)
{
    if (const int rc = bilateral_grid_check("gs_bilateral_tv", c, grid, Gx, Gy, L)) return rc;
    if (!value) return fail(GS_ERR_INVALID_ARGUMENT, "gs_bilateral_tv: value is NULL");
    if (!std::isfinite(weight)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_bilateral_tv: weight must be finite");
    return queued_call(c, stream_, "gs_bilateral_tv", {},
                       [&](hipStream_t s) { gs_launch_bilateral_tv(grid, Gx, Gy, L, weight, grad_grid, value, s); });
}

// ---- depth supervision (include/gs_depth.h, k_depth.hip) ------------------------------------------------------------------------
extern "C" int gs_depth_resample(gs_ctx* c, const void* src, int32_t src_format, int32_t H_in, int32_t W_in, int64_t src_row_pitch_bytes,
                                 float depth_scale, int32_t h_full, int32_t w_full, int32_t h_out, int32_t w_out, float min_coverage,
                                 float* dst, gs_stream stream_)
{
    const char* const who = "gs_depth_resample";
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, who, "ctx is NULL");
    if (src_format != GS_DEPTH_U16 && src_format != GS_DEPTH_F32) return fail(GS_ERR_INVALID_ARGUMENT, who, "unknown src_format");
    if (!(min_coverage >= 0.0f && min_coverage <= 1.0f)) return fail(GS_ERR_INVALID_ARGUMENT, who, "min_coverage must be in [0, 1]");
    if (!(depth_scale > 0.0f && std::isfinite(depth_scale))) return fail(GS_ERR_INVALID_ARGUMENT, who, "depth_scale must be finite and > 0");
    for (int32_t v : { H_in, W_in, h_full, w_full, h_out, w_out })
        if (v < 0 || v > GS_RESAMPLE_MAX_SIZE) return fail(GS_ERR_INVALID_ARGUMENT, who, "every size must be in [0, 32768]");
    if (h_out > h_full || w_out > w_full) return fail(GS_ERR_INVALID_ARGUMENT, who, "the crop (h_out, w_out) exceeds the resize (h_full, w_full)");
    if (src_format == GS_DEPTH_U16 ? src_row_pitch_bytes < (int64_t)W_in * 2 : src_row_pitch_bytes != (int64_t)W_in * 4)
        return fail(GS_ERR_INVALID_ARGUMENT, who, "src_row_pitch_bytes must be >= W_in * 2 (uint16), W_in * 4 (f32)");
    if (h_out == 0 || w_out == 0) return GS_OK;
    if (!src || !dst) return fail(GS_ERR_INVALID_ARGUMENT, who, "NULL src or dst");
    if (H_in < h_full || W_in < w_full || (int64_t)H_in > (int64_t)GS_RESAMPLE_MAX_SCALE * h_full || (int64_t)W_in > (int64_t)GS_RESAMPLE_MAX_SCALE * w_full)
        return fail(GS_ERR_INVALID_ARGUMENT, who, "the scale in / out must be in [1, 8] on both axes (no upscaling)");
    std::lock_guard<std::mutex> lock(c->mu);
    hipStream_t s;
    int rc;
    if ((rc = enter_call(c, stream_, &s)) != GS_OK) return rc;
    ResampleTable* rt = nullptr;
    if ((rc = resample_tables(c, H_in, W_in, h_full, w_full, s, &rt)) != GS_OK) return rc;
    gs_launch_depth_resample(src, src_format, H_in, W_in, src_row_pitch_bytes, depth_scale, rt->ax, rt->ay, h_out, w_out, min_coverage, dst, s);
    HIP_TRY(hipGetLastError());
    return GS_OK;
}

static int depth_loss_check(const char* who, gs_ctx* c, const float* D, const float* Z, const float* w_t, int32_t H, int32_t W, int32_t flags,
                            const float* terms)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, who, "ctx is NULL");
    if (!D || !Z || !w_t) return fail(GS_ERR_INVALID_ARGUMENT, who, "NULL plane (D, Z or w_t)");
    if (!terms) return fail(GS_ERR_INVALID_ARGUMENT, who, "loss_terms is NULL");
    if (const int rc = image_size_check(who, H, W, GS_APPEARANCE_MAX_PIXELS)) return rc;
    if ((flags & ~GS_DEPTH_FLAGS_ALL) != 0) return fail(GS_ERR_INVALID_ARGUMENT, who, "unknown flag bits");
    return GS_OK;
}

extern "C" int gs_depth_loss_forward(gs_ctx* c, const float* D, const float* Z, const float* w_t, const float* w_p, int32_t H, int32_t W,
                                     int32_t flags, float* loss_terms, gs_stream stream_)
{
    if (const int rc = depth_loss_check("gs_depth_loss_forward", c, D, Z, w_t, H, W, flags, loss_terms)) return rc;
    return queued_call(c, stream_, "gs_depth_loss_forward", { NEED(c->depth_ws, gs_depth_ws_size(H, W)) },
                       [&](hipStream_t s) { gs_launch_depth_loss_forward(D, Z, w_t, w_p, H, W, flags, loss_terms, c->depth_ws.p, s); });
}

extern "C" int gs_depth_loss_backward(gs_ctx* c, const float* D, const float* Z, const float* w_t, const float* w_p, int32_t H, int32_t W,
                                      int32_t flags, const float* loss_terms, const float* upstream, float* grad_D, gs_stream stream_)
{
    if (const int rc = depth_loss_check("gs_depth_loss_backward", c, D, Z, w_t, H, W, flags, loss_terms)) return rc;
    if (!grad_D) return fail(GS_ERR_INVALID_ARGUMENT, "gs_depth_loss_backward: grad_D is NULL");
    return queued_call(c, stream_, "gs_depth_loss_backward", {},
                       [&](hipStream_t s) { gs_launch_depth_loss_backward(D, Z, w_t, w_p, H, W, flags, loss_terms, upstream, grad_D, s); });
}

// ---- geometry regularisers (include/gs_geometry.h, k_geometry.hip) ---------------------------------------------------------------
static int geometry_check(const char* who, gs_ctx* c, const float* D, int32_t H, int32_t W, int32_t flags, int32_t flags_all)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, who, "ctx is NULL");
    if (!D) return fail(GS_ERR_INVALID_ARGUMENT, who, "D is NULL");
    if (const int rc = image_size_check(who, H, W, GS_APPEARANCE_MAX_PIXELS)) return rc;
    if ((flags & ~flags_all) != 0) return fail(GS_ERR_INVALID_ARGUMENT, who, "unknown flag bits");
    return GS_OK;
}

static int geometry_check_camera(const char* who, float fx, float fy, float cx, float cy, float max_rel_jump)
{
    if (!(std::isfinite(fx) && std::isfinite(fy) && fx > 0.0f && fy > 0.0f)) return fail(GS_ERR_INVALID_ARGUMENT, who, "fx and fy must be finite and > 0");
    if (!(std::isfinite(cx) && std::isfinite(cy))) return fail(GS_ERR_INVALID_ARGUMENT, who, "cx and cy must be finite");
    if (!(std::isfinite(max_rel_jump) && max_rel_jump >= 0.0f)) return fail(GS_ERR_INVALID_ARGUMENT, who, "max_rel_jump must be finite and >= 0");
    return GS_OK;
}

extern "C" int gs_depth_normals(gs_ctx* c, const float* D, int32_t H, int32_t W, float fx, float fy, float cx, float cy, float max_rel_jump,
                                float* normals, gs_stream stream_)
{
    if (const int rc = geometry_check("gs_depth_normals", c, D, H, W, 0, 0)) return rc;
    if (!normals) return fail(GS_ERR_INVALID_ARGUMENT, "gs_depth_normals: normals is NULL");
    if (const int rc = geometry_check_camera("gs_depth_normals", fx, fy, cx, cy, max_rel_jump)) return rc;
    return queued_call(c, stream_, "gs_depth_normals", {},
                       [&](hipStream_t s) { gs_launch_depth_normals(D, H, W, fx, fy, cx, cy, max_rel_jump, normals, s); });
}

static int normal_loss_check(const char* who, gs_ctx* c, const float* D, const float* N, const float* w_n, int32_t H, int32_t W, float fx,
                             float fy, float cx, float cy, float max_rel_jump, int32_t flags, const float* terms)
{
    if (const int rc = geometry_check(who, c, D, H, W, flags, GS_GEOM_NORMAL_FLAGS_ALL)) return rc;
    if (!N || !w_n) return fail(GS_ERR_INVALID_ARGUMENT, who, "NULL plane (N or w_n)");
    if (!terms) return fail(GS_ERR_INVALID_ARGUMENT, who, "terms is NULL");
    return geometry_check_camera(who, fx, fy, cx, cy, max_rel_jump);
}

extern "C" int gs_normal_loss_forward(gs_ctx* c, const float* D, const float* N, const float* w_n, const float* w_p, int32_t H, int32_t W,
                                      float fx, float fy, float cx, float cy, float max_rel_jump, int32_t flags, float* terms, gs_stream stream_)
{
    if (const int rc = normal_loss_check("gs_normal_loss_forward", c, D, N, w_n, H, W, fx, fy, cx, cy, max_rel_jump, flags, terms)) return rc;
    return queued_call(c, stream_, "gs_normal_loss_forward", { NEED(c->geometry_ws, gs_geometry_ws_size(H, W)) }, [&](hipStream_t s) {
        gs_launch_normal_loss_forward(D, N, w_n, w_p, H, W, fx, fy, cx, cy, max_rel_jump, flags, terms, c->geometry_ws.p, s);
    });
}

extern "C" int gs_normal_loss_backward(gs_ctx* c, const float* D, const float* N, const float* w_n, const float* w_p, int32_t H, int32_t W,
                                       float fx, float fy, float cx, float cy, float max_rel_jump, int32_t flags, const float* terms,
                                       const float* upstream, float* grad_D, gs_stream stream_)
{
    if (const int rc = normal_loss_check("gs_normal_loss_backward", c, D, N, w_n, H, W, fx, fy, cx, cy, max_rel_jump, flags, terms)) return rc;
    if (!grad_D) return fail(GS_ERR_INVALID_ARGUMENT, "gs_normal_loss_backward: grad_D is NULL");
    return queued_call(c, stream_, "gs_normal_loss_backward", {}, [&](hipStream_t s) {
        gs_launch_normal_loss_backward(D, N, w_n, w_p, H, W, fx, fy, cx, cy, max_rel_jump, flags, terms, upstream, grad_D, s);
    });
}

static int depth_smooth_check(const char* who, gs_ctx* c, const float* D, int32_t H, int32_t W, float edge_lambda, int32_t flags,
                              const float* terms)
{
    if (const int rc = geometry_check(who, c, D, H, W, flags, GS_GEOM_SMOOTH_FLAGS_ALL)) return rc;
    if (!terms) return fail(GS_ERR_INVALID_ARGUMENT, who, "terms is NULL");
    if (!(std::isfinite(edge_lambda) && edge_lambda >= 0.0f)) return fail(GS_ERR_INVALID_ARGUMENT, who, "edge_lambda must be finite and >= 0");
    return GS_OK;
}

extern "C" int gs_depth_smooth_forward(gs_ctx* c, const float* D, const float* I, const float* w_p, int32_t H, int32_t W, float edge_lambda,
                                       int32_t flags, float* terms, gs_stream stream_)
{
    if (const int rc = depth_smooth_check("gs_depth_smooth_forward", c, D, H, W, edge_lambda, flags, terms)) return rc;
    return queued_call(c, stream_, "gs_depth_smooth_forward", { NEED(c->geometry_ws, gs_geometry_ws_size(H, W)) },
                       [&](hipStream_t s) { gs_launch_depth_smooth_forward(D, I, w_p, H, W, edge_lambda, flags, terms, c->geometry_ws.p, s); });
}

extern "C" int gs_depth_smooth_backward(gs_ctx* c, const float* D, const float* I, const float* w_p, int32_t H, int32_t W, float edge_lambda,
                                        int32_t flags, const float* terms, const float* upstream, float* grad_D, gs_stream stream_)
{
    if (const int rc = depth_smooth_check("gs_depth_smooth_backward", c, D, H, W, edge_lambda, flags, terms)) return rc;
    if (!grad_D) return fail(GS_ERR_INVALID_ARGUMENT, "gs_depth_smooth_backward: grad_D is NULL");
    return queued_call(c, stream_, "gs_depth_smooth_backward", {},
                       [&](hipStream_t s) { gs_launch_depth_smooth_backward(D, I, w_p, H, W, edge_lambda, flags, terms, upstream, grad_D, s); });
}

// ---- Gaussian normals and their consistency with the depth normal (include/gs_normals.h, k_normals.hip) --------------------------
static int gaussian_normals_check(const char* who, gs_ctx* c, const float* pc, const float* feat, const float* q_pc, const float* t_pc,
                                  int64_t N, int32_t K, const void* a, const void* b)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, who, "ctx is NULL");
    if (N < 0 || N > (int64_t)INT32_MAX - GS_NORMALS_BLOCK) return fail(GS_ERR_INVALID_ARGUMENT, who, "N must be in [0, 2^31 - 256]");
    if (K < 1) return fail(GS_ERR_INVALID_ARGUMENT, who, "K must be >= 1");
    if (!q_pc || !t_pc) return fail(GS_ERR_INVALID_ARGUMENT, who, "NULL pose array");
    if (N > 0 && (!pc || !feat || !a || !b)) return fail(GS_ERR_INVALID_ARGUMENT, who, "NULL array");
    return GS_OK;
}

extern "C" int gs_gaussian_normals_forward(gs_ctx* c, const float* pc, const float* feat, const int32_t* obj, const float* q_pc,
                                           const float* t_pc, int64_t N, int32_t K, float* normals, gs_stream stream_)
{
    if (const int rc = gaussian_normals_check("gs_gaussian_normals_forward", c, pc, feat, q_pc, t_pc, N, K, normals, normals)) return rc;
    if (N == 0) return GS_OK;
    return queued_call(c, stream_, "gs_gaussian_normals_forward", {},
                       [&](hipStream_t s) { gs_launch_gaussian_normals_forward(pc, feat, obj, q_pc, t_pc, N, K, normals, s); });
}

extern "C" int gs_gaussian_normals_backward(gs_ctx* c, const float* pc, const float* feat, const int32_t* obj, const float* q_pc,
                                            const float* t_pc, int64_t N, int32_t K, const float* grad_normals, float* grad_features,
                                            gs_stream stream_)
{
    if (const int rc = gaussian_normals_check("gs_gaussian_normals_backward", c, pc, feat, q_pc, t_pc, N, K, grad_normals, grad_features)) return rc;
    if (N == 0) return GS_OK;
    return queued_call(c, stream_, "gs_gaussian_normals_backward", {}, [&](hipStream_t s) {
        gs_launch_gaussian_normals_backward(pc, feat, obj, q_pc, t_pc, N, K, grad_normals, grad_features, s);
    });
}

static int normal_consistency_check(const char* who, gs_ctx* c, const float* D, const float* R, int32_t H, int32_t W, float fx, float fy,
                                    float cx, float cy, float max_rel_jump, float min_length, const float* terms)
{
    if (const int rc = geometry_check(who, c, D, H, W, 0, 0)) return rc;
    if ((int64_t)H * (int64_t)W > (int64_t)GS_NORMALS_MAX_PIXELS) return fail(GS_ERR_INVALID_ARGUMENT, who, "too many pixels");
    if (!R) return fail(GS_ERR_INVALID_ARGUMENT, who, "R is NULL");
    if (!terms) return fail(GS_ERR_INVALID_ARGUMENT, who, "terms is NULL");
    if (!(std::isfinite(min_length) && min_length > 0.0f)) return fail(GS_ERR_INVALID_ARGUMENT, who, "min_length must be finite and > 0");
    return geometry_check_camera(who, fx, fy, cx, cy, max_rel_jump);
}

extern "C" int gs_normal_consistency_forward(gs_ctx* c, const float* D, const float* R, const float* w_p, int32_t H, int32_t W, float fx,
                                             float fy, float cx, float cy, float max_rel_jump, float min_length, float* terms,
                                             gs_stream stream_)
{
    if (const int rc = normal_consistency_check("gs_normal_consistency_forward", c, D, R, H, W, fx, fy, cx, cy, max_rel_jump, min_length, terms))
        return rc;
    return queued_call(c, stream_, "gs_normal_consistency_forward", { NEED(c->geometry_ws, gs_geometry_ws_size(H, W)) }, [&](hipStream_t s) {
        gs_launch_normal_consistency_forward(D, R, w_p, H, W, fx, fy, cx, cy, max_rel_jump, min_length, terms, c->geometry_ws.p, s);
    });
}

extern "C" int gs_normal_consistency_backward(gs_ctx* c, const float* D, const float* R, const float* w_p, int32_t H, int32_t W, float fx,
                                              float fy, float cx, float cy, float max_rel_jump, float min_length, const float* terms,
                                              const float* upstream, float* grad_D, float* grad_R, gs_stream stream_)
{
    if (const int rc = normal_consistency_check("gs_normal_consistency_backward", c, D, R, H, W, fx, fy, cx, cy, max_rel_jump, min_length, terms))
        return rc;
    if (!grad_D || !grad_R) return fail(GS_ERR_INVALID_ARGUMENT, "gs_normal_consistency_backward: grad_D or grad_R is NULL");
    return queued_call(c, stream_, "gs_normal_consistency_backward", {}, [&](hipStream_t s) {
        gs_launch_normal_consistency_backward(D, R, w_p, H, W, fx, fy, cx, cy, max_rel_jump, min_length, terms, upstream, grad_D, grad_R, s);
    });
}

// ---- vector quantisation (include/gs_vq.h, k_vq.hip) --------------------------------------------------------------------------
static int vq_check(const char* who, gs_ctx* c, const float* x, int64_t ldx, int64_t N, int32_t dim, const float* codebook, int64_t ldc,
                    int32_t K)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, who, "ctx is NULL");
    if (N < 0 || N > INT32_MAX) return fail(GS_ERR_INVALID_ARGUMENT, who, "n_rows must be in [0, 2^31)");
    if (dim < 1 || dim > GS_VQ_MAX_DIM) return fail(GS_ERR_INVALID_ARGUMENT, who, "dim must be in [1, 64]");
    if (K < 1 || K > GS_VQ_MAX_CODES) return fail(GS_ERR_INVALID_ARGUMENT, who, "n_codes must be in [1, 65536]");
    if (ldx < dim || (ldx & 3) != 0) return fail(GS_ERR_INVALID_ARGUMENT, who, "ldx must be a multiple of 4 and >= dim");
    if (ldc < dim || (ldc & 3) != 0) return fail(GS_ERR_INVALID_ARGUMENT, who, "ldc must be a multiple of 4 and >= dim");
    if ((((uintptr_t)x | (uintptr_t)codebook) & 15u) != 0) return fail(GS_ERR_INVALID_ARGUMENT, who, "x and codebook must be 16-byte aligned");
    return GS_OK;
}

extern "C" int64_t gs_vq_scratch_bytes(int64_t n_rows, int32_t n_codes, int32_t dim)
{
    if (n_rows < 0 || n_rows > INT32_MAX || n_codes < 1 || n_codes > GS_VQ_MAX_CODES || dim < 1 || dim > GS_VQ_MAX_DIM) return 0;
    return (int64_t)gs_vq_scratch_size(n_rows, n_codes, dim);
}

extern "C" int gs_vq_assign(gs_ctx* c, const float* x, int64_t ldx, int64_t N, int32_t dim, const float* codebook, int64_t ldc, int32_t K,
                            int32_t* labels, float* dist, void* scratch, gs_stream stream_)
{
    if (const int rc = vq_check("gs_vq_assign", c, x, ldx, N, dim, codebook, ldc, K)) return rc;
    if (N > 0 && (!x || !codebook || !labels || !scratch)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_vq_assign: NULL array");
    if (((uintptr_t)scratch & 7u) != 0) return fail(GS_ERR_INVALID_ARGUMENT, "gs_vq_assign: scratch must be 8-byte aligned");
    if (N == 0) return GS_OK;
    return queued_call(c, stream_, "gs_vq_assign", {},
                       [&](hipStream_t s) { gs_launch_vq_assign(x, ldx, N, dim, codebook, ldc, K, labels, dist, scratch, s); });
}

extern "C" int gs_vq_update(gs_ctx* c, const float* x, int64_t ldx, int64_t N, int32_t dim, const float* weights, const int32_t* labels,
                            float* codebook, int64_t ldc, int32_t K, int32_t* counts, double* weight_sums, void* scratch, gs_stream stream_)
{
    (void)scratch;
    if (const int rc = vq_check("gs_vq_update", c, x, ldx, N, dim, codebook, ldc, K)) return rc;
    if (!codebook || !counts || (N > 0 && (!x || !labels))) return fail(GS_ERR_INVALID_ARGUMENT, "gs_vq_update: NULL array");
    if (((uintptr_t)weight_sums & 7u) != 0) return fail(GS_ERR_INVALID_ARGUMENT, "gs_vq_update: weight_sums must be 8-byte aligned");
    return queued_call(c, stream_, "gs_vq_update", {},
                       [&](hipStream_t s) { gs_launch_vq_update(x, ldx, N, dim, weights, labels, codebook, ldc, K, counts, weight_sums, s); });
}

// ---- per-view camera pose corrections (include/gs_pose_table.h, k_posetable.hip) ------------------------------------------
static int pose_table_check(const char* who, gs_ctx* c, int32_t V, int32_t K)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, who, "ctx is NULL");
    if (V < 0 || V > GS_POSE_MAX_VIEWS) return fail(GS_ERR_INVALID_ARGUMENT, who, "V must be in [0, 2^24]");
    if (K < 0 || K > GS_POSE_MAX_OBJECTS) return fail(GS_ERR_INVALID_ARGUMENT, who, "K must be in [0, 64]");
    return GS_OK;
}

extern "C" int gs_pose_compose(gs_ctx* c, const float* delta, const float* q_base, const float* t_base, int32_t V, int32_t K, float* q_out,
                               float* t_out, gs_stream stream_)
{
    if (const int rc = pose_table_check("gs_pose_compose", c, V, K)) return rc;
    if (V == 0 || K == 0) return GS_OK;
    if (!delta || !q_base || !t_base || !q_out || !t_out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_pose_compose: NULL array");
    return queued_call(c, stream_, "gs_pose_compose", {},
                       [&](hipStream_t s) { gs_launch_pose_compose(delta, q_base, t_base, V, K, q_out, t_out, s); });
}

extern "C" int gs_pose_compose_backward(gs_ctx* c, const float* delta, const float* q_base, const float* grad_q, const float* grad_t, int32_t V,
                                        int32_t K, float reg, float* grad_delta, gs_stream stream_)
{
    if (const int rc = pose_table_check("gs_pose_compose_backward", c, V, K)) return rc;
    if (!std::isfinite(reg)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_pose_compose_backward: reg must be finite");
    if (V == 0 || K == 0) return GS_OK;
    if (!delta || !q_base || !grad_q || !grad_t || !grad_delta) return fail(GS_ERR_INVALID_ARGUMENT, "gs_pose_compose_backward: NULL array");
    return queued_call(c, stream_, "gs_pose_compose_backward", {},
                       [&](hipStream_t s) { gs_launch_pose_compose_backward(delta, q_base, grad_q, grad_t, V, K, reg, grad_delta, s); });
}

// ---- adaptive density control (k_density.hip) -------------------------------------------------------------------------
extern "C" int64_t gs_density_scratch_bytes(int64_t n_points) { return n_points < 0 ? 0 : (int64_t)gs_density_scratch_size(n_points); }

static int density_plan_check(const char* who, const gs_density_plan* p, int64_t N)
{
    if (!p || !p->counts) return fail(GS_ERR_INVALID_ARGUMENT, who, "plan or plan->counts is NULL");
    if (N < 0 || N > INT32_MAX) return fail(GS_ERR_INVALID_ARGUMENT, who, "n_points must be in [0, 2^31)");
    if (p->n_points < N) return fail(GS_ERR_INVALID_ARGUMENT, who, "plan is smaller than the scene");
    if (N > 0 && (!p->flags || !p->densify_point_id || !p->densify_point_position_before_optimization || !p->densify_point_grad_position ||
                  !p->densify_size_reduction_factor || !p->fill_point_id || !p->scratch))
        return fail(GS_ERR_INVALID_ARGUMENT, who, "NULL plan array");
    return GS_OK;
}

extern "C" int gs_density_select(gs_ctx* c, const gs_scene* scene, const gs_controller_accumulators* acc, const int32_t* ids,
                                 const int32_t* npix, const float* depth, const float* mag, int64_t M, int32_t remove_floaters,
                                 const gs_density_config* cfg, const gs_density_plan* plan, gs_stream stream_)
{
    if (!c || !scene || !acc || !cfg) return fail(GS_ERR_INVALID_ARGUMENT, "gs_density_select: NULL argument");
    const int64_t N = scene->n_points;
    if (int rc = density_plan_check("gs_density_select", plan, N)) return rc;
    if (M < 0 || M > N) return fail(GS_ERR_INVALID_ARGUMENT, "gs_density_select: n_in_camera must be in [0, n_points]");
    if (M > 0 && (!ids || !npix || !depth || !mag)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_density_select: NULL hook array");
    if (N > 0 && (!scene->point_cloud || !scene->point_cloud_features || !scene->point_invalid_mask))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_density_select: NULL scene array");
    if (N > 0 && (!acc->accumulated_num_in_camera || !acc->accumulated_num_pixels || !acc->accumulated_view_space_position_gradients ||
                  !acc->accumulated_view_space_position_gradients_avg || !acc->accumulated_position_gradients ||
                  !acc->accumulated_position_gradients_norm))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_density_select: the controller accumulators must all be given");
    return queued_call(c, stream_, "gs_density_select", {}, [&](hipStream_t s) {
        gs_launch_density_select(*scene, *acc, ids, npix, depth, mag, M, remove_floaters != 0, *cfg, *plan, s);
    });
}

extern "C" int gs_density_apply(gs_ctx* c, const gs_density_scene* scene, const gs_density_config* cfg, const gs_density_plan* plan,
                                uint64_t seed, uint32_t call_index, gs_stream stream_)
{
    if (!c || !scene || !cfg) return fail(GS_ERR_INVALID_ARGUMENT, "gs_density_apply: NULL argument");
    const int64_t N = scene->n_points;
    if (int rc = density_plan_check("gs_density_apply", plan, N)) return rc;
    if (N > 0 && (!scene->point_cloud || !scene->point_cloud_features || !scene->point_invalid_mask || !scene->point_object_id))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_density_apply: NULL scene array");
    return queued_call(c, stream_, "gs_density_apply", {},
                       [&](hipStream_t s) { gs_launch_density_apply(*scene, *cfg, *plan, seed, call_index, s); });
}

extern "C" int gs_controller_accumulate(gs_ctx* c, const int32_t* ids, const int32_t* npix, const float* mag, const float* gpc, int64_t M,
                                        int64_t N, const gs_controller_accumulators* acc, gs_stream stream_)
{
    if (!c || !acc) return fail(GS_ERR_INVALID_ARGUMENT, "gs_controller_accumulate: NULL argument");
    if (N < 0 || N > INT32_MAX || M < 0 || M > N) return fail(GS_ERR_INVALID_ARGUMENT, "gs_controller_accumulate: need 0 <= n_in_camera <= n_points < 2^31");
    if (M > 0 && (!ids || !npix || !mag || !gpc)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_controller_accumulate: NULL hook array");
    if (M > 0 && (!acc->accumulated_num_in_camera || !acc->accumulated_num_pixels || !acc->accumulated_view_space_position_gradients ||
                  !acc->accumulated_view_space_position_gradients_avg || !acc->accumulated_position_gradients ||
                  !acc->accumulated_position_gradients_norm))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_controller_accumulate: the controller accumulators must all be given");
    return queued_call(c, stream_, "gs_controller_accumulate", {},
                       [&](hipStream_t s) { gs_launch_controller_accumulate(ids, npix, mag, gpc, M, N, *acc, s); });
}

