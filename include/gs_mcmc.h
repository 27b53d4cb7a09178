/* gs_mcmc.h -- fixed-budget densification after 3DGS-MCMC (Kheradmand et al., "3D Gaussian Splatting as Markov Chain Monte
 * Carlo", NeurIPS 2024): position noise shaped by each Gaussian's covariance and the two L1 regularisers on every step, and
 * the relocation of dead Gaussians onto live ones with growth up to a cap every refinement.
 *
 *   loss.backward();
 *   gs_mcmc_regulariser(ctx, features, mask, N, lambda_o, lambda_s, NULL, grad_features, value_and_count, stream);
 *   ... the optimiser steps ...
 *   gs_mcmc_noise(ctx, point_cloud, features, mask, N, noise_lr * position_lr, 100, 0.995f, seed, step, stream);
 *   gs_mcmc_relocate(ctx, &scene, m_f, v_f, m_x, v_x, &config, &plan, seed, call, stream);        // every refine_every steps
 *
 * Same library, same rules as gs_rasterizer.h: status codes, gs_last_error(), the call's stream last.  Not part of
 * GS_ABI_VERSION's function list.  No call synchronises with the host or allocates caller-visible memory; no float atomic
 * anywhere: every output is bit-reproducible and independent of the launch shape.  Every f32 and f64 operation below is rounded
 * on its own (no contraction), in the order the parentheses give.  (csrc/k_mcmc.hip)
 *
 * ---- rows ----
 * A 56-float feature row is q xyzw (0..3), log s (4..6), the opacity logit (7), SH (8..55).  A row is VALID when
 * point_invalid_mask == 0, FREE when it is exactly 1; a row with any other mask value is neither, and no call touches it.
 * N = 0 is valid everywhere.  gs_expf and gs_sigmoid(x) = 1.0f / (1.0f + gs_expf(-x)) are the library's (gs_expf clamps its
 * argument to [-86, 88], a NaN stays a NaN).
 *
 * ---- gs_mcmc_noise: every step, after the optimiser step ----
 * For every valid row n, all in f32:
 *   o = gs_sigmoid(logit)
 *   g = 1.0f / (1.0f + gs_expf(-(gate_k * ((1.0f - o) - gate_x0))))
 *   s = g * noise_scale                                  (the caller passes noise_scale = noise_lr x current position lr)
 *   u = Philox4x32-10(counter (n, step_index, 2, 0), key (low, high word of seed))
 *   U_k = (float)((u_k >> 8) + 1) * 2^-24  for the four words;  two_pi = (float)(2.0 * 3.141592653589)
 *   r1 = sqrtf(-2.0f * logf(U_0));  r3 = sqrtf(-2.0f * logf(U_2))
 *   z = (r1 * cosf(two_pi * U_1), r1 * sinf(two_pi * U_1), r3 * cosf(two_pi * U_3))        (gs_density_apply's Box-Muller)
 *   Sigma = R S S R^T of the row: ((R S) S) R^T, R from q as stored (not normalised), S = diag(gs_expf(log s)); every
 *           3x3 product sums its terms k = 0, 1, 2 in order (gs_rasterizer.h's covariance)
 *   v = z * s
 *   delta_i = (Sigma_i0 * v_0 + Sigma_i1 * v_1) + Sigma_i2 * v_2
 *   x_i = x_i + delta_i
 * A row whose delta has a non-finite component is left as it is.  The result for row n depends on (n, step_index, seed) and
 * the row's own values only.  The third counter word keeps the stream apart from the split samples of gs_density_apply (0, 1)
 * and from the relocation's draw (3).
 *
 * ---- gs_mcmc_regulariser: every step, between the backward and the optimiser step ----
 * V = the number of valid rows.  With o = gs_sigmoid(logit) and e_j = gs_expf(log s_j), both f32:
 *   value_and_count = { (float)(lambda_opacity * So / V), (float)(lambda_scale * Ss / (3 V)), (float)V }
 *     So = sum over valid rows of (double)o, Ss = sum over valid rows of ((double)e_0 + (double)e_1) + (double)e_2: float64 sums
 *     in an order fixed by the row id -- per block of GS_MCMC_BLOCK rows, then one block over the partials -- so every run
 *     gives the same bits.  The value of the regulariser is the sum of the first two.  V = 0: {0, 0, 0}, no gradient.
 *   the gradient is ADDED into grad_features (N,56), in f32, up = *upstream (1.0f when upstream is NULL), Vf = (float)V:
 *     g[n,7]   = g[n,7]   + ((up * lambda_opacity) / Vf) * (o * (1.0f - o))
 *     g[n,4+j] = g[n,4+j] + ((up * lambda_scale) / (3.0f * Vf)) * e_j
 *   No other column of a valid row and no element of any other row is written.  grad_features NULL: the value alone;
 *   value_and_count NULL: the gradient alone.
 *
 * ---- gs_mcmc_relocate: every refine_every steps ----
 * 1 classify.  A valid row is DEAD when !(logit > min_opacity_logit) (a NaN logit is dead), ALIVE otherwise.  An alive row has
 *     the integer weight w = clamp((int)floorf(gs_sigmoid(logit) * 2^24), 1, 2^24 - 1); every other row has weight 0.
 *     W = sum w, a uint64: exact, so independent of any order.  Counted: valid, dead, alive, free rows.
 * 2 budget, in int64:  target = min(cap_max, valid + valid * grow_permille / 1000)      (floor division)
 *                      n_new  = min(free, max(0, target - valid));   D = dead + n_new
 *     If alive == 0 then D = 0, n_new = 0 and nothing is written but the counts.
 * 3 destinations.  dest_row[j], j < dead, is the j-th dead row, ascending; for j >= dead the (j - dead)-th free row, ascending.
 * 4 sample.  For destination j: u = Philox4x32-10(counter (j, call_index, 3, 0), key of seed);  r = u_0 + 2^32 * u_1;
 *     t = floor(r * W / 2^64) (the high half of the 64x64 product).  source_of[j] is the row n with C(n) <= t < C(n) + w_n, C the
 *     exclusive prefix sum of w in row order.  multiplicity[n] = the number of destinations that drew n (0 for every other row
 *     of the scene).  All D destinations draw from the opacities before the call, in one round.
 * 5 apply.  For a source n, m = multiplicity[n] > 0:  M = min(m + 1, n_max),  o = (double)gs_sigmoid(logit), in float64:
 *       p = 1 - pow(1 - o, 1.0 / M);   p = p < 0.005 ? 0.005 : (p > 1 - 2^-24 ? 1 - 2^-24 : p)        (a NaN stays)
 *       d = sum_{i=1..M} sum_{k=0..i-1} C(i-1,k) * (-1)^k * p^(k+1) / sqrt(k+1), one running sum, i outer, k inner, each term
 *           (C(i-1,k) * p^(k+1)) / sqrt((double)(k+1)) added for even k and subtracted for odd k; C(i-1,k) is exact (below
 *           2^53) and p^(k+1) = p^k * p by repeated multiplication from p^1 = p
 *       new logit   = (float)log(p / (1 - p))
 *       new log s_j = (float)((double)log s_j + log(o / d))
 *     The source and each of its destinations end up with the source's position, object id, q and SH bit for bit, the new logit
 *     and log-scales (the same bits within the group) and mask 0.  The rows of the source and of its destinations are zeroed in
 *     each of the four moment tensors that is given.  Every other row of the scene and of the moments keeps every bit.
 * 6 counts = { valid_before, dead, alive, free, n_new, D, sources (rows with m > 0), valid_after = valid_before + n_new }.
 * Deviation from the paper, which relocates the dead rows first and then draws a second time for the added ones: one joint draw.
 * How: N-passes of GS_MCMC_BLOCK-thread blocks with in-block ranks and prefix sums (uint32 holds a block's weights:
 * 256 (2^24 - 1) < 2^32; across blocks the prefix is uint64), one block over the per-block sums, a binary search per destination,
 * the destinations' rows written before the sources' in a launch of their own (a destination reads its source's old values),
 * float64 in the apply pass only.  Integer atomics count the multiplicities and the sources.
 */
#ifndef GS_MCMC_H
#define GS_MCMC_H
#include "gs_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_MCMC_BLOCK 256            /* rows per block of every N-pass */
#define GS_MCMC_N_MAX 51             /* the largest n_max: C(50,25) < 2^53 */
#define GS_MCMC_WEIGHT_ONE 16777216  /* 2^24: the weight of opacity 1, before the clamp */
#define GS_MCMC_STREAM_NOISE 2       /* third counter word of gs_mcmc_noise */
#define GS_MCMC_STREAM_RELOCATE 3    /* third counter word of gs_mcmc_relocate */

/* plan->counts, int32 each */
typedef enum gs_mcmc_count {
    GS_MC_VALID_BEFORE = 0,
    GS_MC_DEAD = 1,
    GS_MC_ALIVE = 2,
    GS_MC_FREE = 3,
    GS_MC_NEW = 4,                   /* free rows brought in */
    GS_MC_DESTINATIONS = 5,          /* D = dead + n_new */
    GS_MC_SOURCES = 6,               /* rows drawn at least once */
    GS_MC_VALID_AFTER = 7,
    GS_MC_COUNT_
} gs_mcmc_count;

typedef struct gs_mcmc_config {
    float   min_opacity_logit;       /* the f32 logit of the smallest opacity that lives (0.005) */
    int32_t n_max;                   /* 1 .. GS_MCMC_N_MAX */
    int32_t grow_permille;           /* >= 0; 50 grows by 5 % */
    int32_t reserved;                /* 0 */
    int64_t cap_max;                 /* >= 0: the most valid rows the growth may reach */
} gs_mcmc_config;

/* Caller-owned device memory, every array with (at least) n_points entries. */
typedef struct gs_mcmc_plan {
    int32_t* source_of;              /* (N) source row of destination j, counts[GS_MC_DESTINATIONS] of them */
    int32_t* dest_row;               /* (N) row of destination j */
    int32_t* multiplicity;           /* (N) per row: how many destinations drew it */
    void*    scratch;                /* gs_mcmc_scratch_bytes(n_points) bytes, 8-byte aligned */
    int32_t* counts;                 /* (GS_MC_COUNT_) */
    int64_t  n_points;               /* rows the arrays were sized for, >= the scene's */
} gs_mcmc_plan;

int64_t gs_mcmc_scratch_bytes(int64_t n_points);

/* point_cloud (N,3) f32 in/out, point_cloud_features (N,56) f32 16-byte aligned, point_invalid_mask (N) i8, all on the device.
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx NULL; n_points negative or above 2^31 - 1; a NULL array with
 * n_points > 0; features not 16-byte aligned; noise_scale, gate_k or gate_x0 not finite.  n_points == 0 is GS_OK with no launch. */
int gs_mcmc_noise(gs_ctx* ctx, float* point_cloud, const float* point_cloud_features, const int8_t* point_invalid_mask,
                  int64_t n_points, float noise_scale, float gate_k, float gate_x0, uint64_t seed, uint32_t step_index,
                  gs_stream stream);

/* upstream: one f32 on the device or NULL (= 1); grad_features (N,56) f32 in/out or NULL; value_and_count: f32[3] on the device
 * or NULL.  GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx NULL; n_points negative or above 2^31 - 1; NULL features
 * or mask with n_points > 0; lambda_opacity or lambda_scale not finite.  n_points == 0 writes {0, 0, 0}. */
int gs_mcmc_regulariser(gs_ctx* ctx, const float* point_cloud_features, const int8_t* point_invalid_mask, int64_t n_points,
                        float lambda_opacity, float lambda_scale, const float* upstream, float* grad_features,
                        float* value_and_count, gs_stream stream);

/* scene: edited in place.  The four moment tensors -- exp_avg and exp_avg_sq of the features (N,56) and of the positions (N,3)
 * -- are optional: any may be NULL.
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx, scene, config or plan NULL; plan->counts NULL; n_points negative
 * or above 2^31 - 1; a plan smaller than the scene; a NULL scene or plan array with n_points > 0; n_max outside
 * [1, GS_MCMC_N_MAX]; grow_permille or cap_max negative; a NaN min_opacity_logit.  n_points == 0 writes counts of zero. */
int gs_mcmc_relocate(gs_ctx* ctx, const gs_density_scene* scene, float* features_exp_avg, float* features_exp_avg_sq,
                     float* point_cloud_exp_avg, float* point_cloud_exp_avg_sq, const gs_mcmc_config* config,
                     const gs_mcmc_plan* plan, uint64_t seed, uint32_t call_index, gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
