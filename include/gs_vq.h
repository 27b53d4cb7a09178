/* gs_vq.h -- vector quantisation of rows of floats: the two halves of a Lloyd (k-means) iteration.  gs_vq_assign gives every
 * row the nearest centroid of a codebook, gs_vq_update moves every centroid to the weighted mean of its rows.  The package
 * uses them to put the 45 higher-band SH coefficients of a scene behind a codebook (compression.py), after Niedermayr et al.,
 * "Compressed 3D Gaussian Splatting for Accelerated Novel View Synthesis" (CVPR 2024).
 *
 *   gs_vq_assign(ctx, x, ldx, N, D, codebook, ldc, K, labels, dist, scratch, stream);
 *   gs_vq_update(ctx, x, ldx, N, D, weights, labels, codebook, ldc, K, counts, weight_sums, scratch, stream);
 *
 * Same library, same rules as gs_rasterizer.h: status codes, gs_last_error(), the call's stream last.  Not part of
 * GS_ABI_VERSION's function list.  No call synchronises with the host or allocates; no float atomic anywhere: every output is
 * bit-reproducible and independent of the launch shape.  Every f32 and f64 operation below is rounded on its own (no
 * contraction) in the order written; fmaf(a, b, c) is a * b + c rounded once.  (csrc/k_vq.hip)
 *
 * ---- arrays ----
 * x is (n_rows, ldx) f32 and codebook (n_codes, ldc) f32, row-major, both 16-byte aligned, on the device; ldx and ldc are
 * multiples of 4 and >= dim.  The value of a column j >= dim is never used: a NaN there changes nothing (the bytes up to the
 * row's next multiple of 4 may be loaded).  Dp = dim rounded up to a multiple of 4; the columns dim <= j < Dp count as +0.0f
 * in every chain below.  x_nj is x[n * ldx + j], c_kj is codebook[k * ldc + j].
 *
 * ---- gs_vq_assign ----
 *   xx_n = 0;     for j = 0 .. Dp-1:  xx_n = fmaf(x_nj, x_nj, xx_n)
 *   cc_k = 0;     for j = 0 .. Dp-1:  cc_k = fmaf(c_kj, c_kj, cc_k)
 *   s_nk = cc_k;  for j = 0 .. Dp-1:  s_nk = fmaf(x_nj, -2.0f * c_kj, s_nk)          (|x - c|^2 - |x|^2; -2.0f * c_kj is exact)
 *   best = +inf, label = -1;  for k = 0 .. n_codes-1:  if cc_k is finite and s_nk < best:  best = s_nk, label = k
 *   if xx_n is not finite:  label = -1
 *   labels[n] = label;   dist[n] = label < 0 ? NaN : fmaxf(0.0f, xx_n + best)
 * Ties go to the smaller k (+0 and -0 are equal); a NaN s_nk never wins; a centroid with a non-finite cc_k is never chosen.
 * dist may be NULL.  The chain of s_nk is what the f32-input matrix instruction of gfx950 computes (D = A B + C adds its
 * products to C in ascending k, each fused and rounded once), so the kernel runs it on the matrix cores: C holds cc_k, A
 * holds -2 c, B holds x.
 *
 * ---- gs_vq_update ----
 * Row n is a member of code k when labels[n] == k and (weights is NULL, or w_n = weights[n] > 0 and finite).  A label outside
 * [0, n_codes) belongs to nobody.  counts[k] = the number of members of k.  With the members of k in ascending row order, in
 * float64, added strictly one after the other from 0.0 (w_n = 1 when weights is NULL):
 *   W_k  = W_k + (double)w_n
 *   S_kj = S_kj + (double)w_n * (double)x_nj                                            (the product is exact)
 * weight_sums[k] = W_k when weight_sums is given (0.0 for a code without members).  When counts[k] > 0:
 *   codebook[k * ldc + j] = (float)(S_kj / W_k)   for j < dim
 * otherwise the centroid keeps every bit.  Columns j >= dim of the codebook are never written.
 * How: a wave owns a few consecutive codes, walks all labels in ascending order, and adds the matching rows one by one into
 * float64 registers, one lane per column.  How many codes a wave owns does not change a bit of the result.
 *
 * ---- scratch ----
 * Caller-owned device memory of gs_vq_scratch_bytes(n_rows, n_codes, dim) bytes, 8-byte aligned: gs_vq_assign keeps cc there.
 * gs_vq_update takes it for symmetry and does not use it (it may be NULL there).
 */
#ifndef GS_VQ_H
#define GS_VQ_H
#include "gs_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_VQ_MAX_DIM 64             /* the most columns of a row */
#define GS_VQ_MAX_CODES 65536        /* the most centroids of a codebook */

/* bytes of scratch for a call with these sizes; 0 when a size is out of range */
int64_t gs_vq_scratch_bytes(int64_t n_rows, int32_t n_codes, int32_t dim);

/* labels (N) int32 out, dist (N) f32 out or NULL.
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx NULL; n_rows negative or above 2^31 - 1; dim outside
 * [1, GS_VQ_MAX_DIM]; n_codes outside [1, GS_VQ_MAX_CODES]; ldx or ldc below dim or not a multiple of 4; with n_rows > 0 a NULL
 * x, codebook, labels or scratch; x or codebook not 16-byte aligned, scratch not 8-byte aligned.  n_rows == 0 is GS_OK with no
 * launch. */
int gs_vq_assign(gs_ctx* ctx, const float* x, int64_t ldx, int64_t n_rows, int32_t dim, const float* codebook, int64_t ldc,
                 int32_t n_codes, int32_t* labels, float* dist, void* scratch, gs_stream stream);

/* weights (N) f32 or NULL (= 1), labels (N) int32, codebook in/out, counts (K) int32 out, weight_sums (K) f64 out or NULL.
 * GS_ERR_INVALID_ARGUMENT as above; NULL codebook or counts; with n_rows > 0 a NULL x or labels; weight_sums not 8-byte
 * aligned.  n_rows == 0 is GS_OK: counts and weight_sums are written as zeros, the codebook is left alone. */
int gs_vq_update(gs_ctx* ctx, const float* x, int64_t ldx, int64_t n_rows, int32_t dim, const float* weights, const int32_t* labels,
                 float* codebook, int64_t ldc, int32_t n_codes, int32_t* counts, double* weight_sums, void* scratch, gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
