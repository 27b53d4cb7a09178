// gs_mixture_math.h -- the arithmetic of the scene-as-mixture kernels (k_mixture.hip, include/gs_mixture.h), each piece stated
// once and callable from the host as well, so that a CPU program can walk the same operation sequence as the kernels.
//
// Per row (float64, rounded once to f32): does the row take part, its sigmoid, its 16-float record.
//   density record    mu (3) | c2 | A' (9, row-major) | 0 0 0      A' = sqrt(log2(e)/2) S^-1 R^T,
//                                                                   c2 = log2(e) (log pi - sum log s - 3/2 log 2 pi)
//   transform record  mu - centre (3) | pi | B' (9) | 0 0 0         B' = sqrt(log2(e)/2) S R^T
// so that a pair costs  t = c2 - |A'(x - mu)|^2  (a base-2 exponent)  or  pi 2^(-|B'k|^2) (cos phi - i sin phi).
// A row that takes no part has the record 0 0 0 | -inf | 0...  or  0 0 0 | 0 | 0...: its term is exactly zero whether a kernel
// skips it or not.
//
// The gradients (k_mixture_grad.hip, include/gs_mixture_grad.h) read the same records.  Per pair: the weight of the pair times
// (1, y', y' y'^T) added to ten f32 sums of the row (gs_mix_density_grad_term / gs_mix_fourier_grad_term), or the pair's share of
// d log p / dx (gs_mix_density_grad_x_term).  Per row (float64, rounded once): the ten sums to the gradients of mu, q, log s
// and the opacity logit (gs_mix_grad_row).
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#define GS_MIX_HD __host__ __device__ __forceinline__
#define GS_MIX_NFEAT 56            // floats of a feature row: q xyzw | log s | opacity logit | SH
#define GS_MIX_REC_FLOATS 16

GS_MIX_HD bool gs_mix_finite(float v) { return fabsf(v) <= FLT_MAX; }       // false for NaN and for +-inf

// mask byte 0 (or no mask), position / q / log s / opacity logit finite, |q|^2 > 0
GS_MIX_HD bool gs_mix_takes_part(const float* mu, const float* feat, const int8_t* mask, int64_t i)
{
    if (mask && mask[i] != 0) return false;
    bool ok = gs_mix_finite(mu[0]) && gs_mix_finite(mu[1]) && gs_mix_finite(mu[2]);
    for (int j = 0; j < 8; ++j) ok = ok && gs_mix_finite(feat[j]);
    const double qq = (double)feat[0] * feat[0] + (double)feat[1] * feat[1] + (double)feat[2] * feat[2] + (double)feat[3] * feat[3];
    return ok && qq > 0.0;
}

GS_MIX_HD double gs_mix_sigmoid(double a) { return 1.0 / (1.0 + exp(-a)); }

GS_MIX_HD float gs_mix_round(double v)      // one rounding to f32, magnitudes beyond its range clamped to it
{
    v = v > (double)FLT_MAX ? (double)FLT_MAX : v;
    v = v < -(double)FLT_MAX ? -(double)FLT_MAX : v;
    return (float)v;
}

// R of q / |q| (q = xyzw), row-major: pytorch3d's quaternion_to_matrix, 2 / |q|^2 where the unnormalised form has 2
GS_MIX_HD void gs_mix_rotation(const float* q, double R[9])
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double ts = 2.0 / (x * x + y * y + z * z + w * w);
    R[0] = 1.0 - ts * (y * y + z * z); R[1] = ts * (x * y - z * w);       R[2] = ts * (x * z + y * w);
    R[3] = ts * (x * y + z * w);       R[4] = 1.0 - ts * (x * x + z * z); R[5] = ts * (y * z - x * w);
    R[6] = ts * (x * z - y * w);       R[7] = ts * (y * z + x * w);       R[8] = 1.0 - ts * (x * x + y * y);
}

// The record of one row.  fourier == false: density, centre unused; total = the sum of the sigmoids of the rows that take part.
GS_MIX_HD void gs_mix_record(const float* mu, const float* feat, bool part, double total, bool fourier, const float* centre,
                             float rec[GS_MIX_REC_FLOATS])
{
    for (int j = 0; j < GS_MIX_REC_FLOATS; ++j) rec[j] = 0.0f;
    rec[3] = fourier ? 0.0f : -INFINITY;
    if (!part || !(total > 0.0)) return;
    const double sig = gs_mix_sigmoid((double)feat[7]);
    const double root = 0.84932180028801904272;                       // sqrt(log2(e) / 2)
    double R[9];
    gs_mix_rotation(feat, R);
    if (fourier) {
        const float pi = gs_mix_round(sig / total);
        if (!(pi > 0.0f)) return;                                      // a weight of exactly zero in f32: no term
        for (int j = 0; j < 3; ++j) rec[j] = gs_mix_round((double)mu[j] - (double)centre[j]);
        rec[3] = pi;
        for (int r = 0; r < 3; ++r) {
            const double s = exp((double)feat[4 + r]) * root;
            for (int c = 0; c < 3; ++c) rec[4 + 3 * r + c] = gs_mix_round(s * R[3 * c + r]);      // (S R^T)[r][c] = s_r R[c][r]
        }
    } else {
        const double log_pi = log(sig) - log(total);                   // sig > 0 here, or the row's constant is -inf: no term
        const double c = log_pi - ((double)feat[4] + (double)feat[5] + (double)feat[6]) - 2.75681559961402421;   // 3/2 log(2 pi)
        const double c2 = c * 1.44269504088896340736;
        if (!(c2 >= -(double)FLT_MAX)) return;
        for (int j = 0; j < 3; ++j) rec[j] = mu[j];
        rec[3] = gs_mix_round(c2);
        for (int r = 0; r < 3; ++r) {
            const double s = exp(-(double)feat[4 + r]) * root;
            for (int c_ = 0; c_ < 3; ++c_) rec[4 + 3 * r + c_] = gs_mix_round(s * R[3 * c_ + r]);
        }
    }
}

GS_MIX_HD float gs_mix_exp2(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_exp2f(v);            // v_exp_f32: 1 ulp; results below the normal range are zero
#else
    return exp2f(v);
#endif
}

// |M v|^2 of a row-major 3x3 M: three fused dot products, then the sum of squares
GS_MIX_HD float gs_mix_sq_norm(const float M[9], float vx, float vy, float vz)
{
    const float w0 = __builtin_fmaf(M[0], vx, __builtin_fmaf(M[1], vy, M[2] * vz));
    const float w1 = __builtin_fmaf(M[3], vx, __builtin_fmaf(M[4], vy, M[5] * vz));
    const float w2 = __builtin_fmaf(M[6], vx, __builtin_fmaf(M[7], vy, M[8] * vz));
    return __builtin_fmaf(w0, w0, __builtin_fmaf(w1, w1, w2 * w2));
}

// the base-2 exponent of one (point, component) pair of the density
GS_MIX_HD float gs_mix_density_term(const float rec[GS_MIX_REC_FLOATS], float x, float y, float z)
{
    return rec[3] - gs_mix_sq_norm(rec + 4, x - rec[0], y - rec[1], z - rec[2]);
}

// sin and cos of phi: n = round(phi 2/pi), r = phi - n pi/2 with pi/2 in three f32 pieces (each step one fma, exact while
// |n| < 2^22 or so; beyond that phi's own rounding is radians wide anyway), the cephes polynomials on [-pi/4, pi/4] (both within
// 1 ulp there), then the quadrant.  |phi| > 1e9 (or NaN) is taken as 0, so the result is always finite.
GS_MIX_HD void gs_mix_sincos(float phi, float* sin_out, float* cos_out)
{
    phi = fabsf(phi) <= 1.0e9f ? phi : 0.0f;      // beyond: phi's own rounding is over 60 radians wide (and n would not fit), no phase is meant
    const float n = rintf(phi * 0.636619772367581343f);
    const int quadrant = (int)n;
    float r = __builtin_fmaf(-n, 1.57079637050628662109375f, phi);
    r = __builtin_fmaf(-n, -4.37113900018624283e-8f, r);
    r = __builtin_fmaf(-n, -1.71512451701245256e-15f, r);
    const float z = r * r;
    float ps = __builtin_fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f);
    ps = __builtin_fmaf(ps, z, -1.6666654611e-1f);
    const float s = __builtin_fmaf(ps * z, r, r);
    float pc = __builtin_fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f);
    pc = __builtin_fmaf(pc, z, 4.166664568298827e-2f);
    const float c = __builtin_fmaf(pc * z, z, __builtin_fmaf(-0.5f, z, 1.0f));
    const float ss = (quadrant & 1) ? c : s, cc = (quadrant & 1) ? s : c;
    *sin_out = (quadrant & 2) ? -ss : ss;
    *cos_out = ((quadrant + 1) & 2) ? -cc : cc;
}

// one (frequency, component) pair of the transform, added to (re, im)
GS_MIX_HD void gs_mix_fourier_term(const float rec[GS_MIX_REC_FLOATS], float kx, float ky, float kz, float* re, float* im)
{
    const float phi = __builtin_fmaf(kx, rec[0], __builtin_fmaf(ky, rec[1], kz * rec[2]));
    const float e = rec[3] * gs_mix_exp2(-gs_mix_sq_norm(rec + 4, kx, ky, kz));
    float s, c;
    gs_mix_sincos(phi, &s, &c);
    *re = __builtin_fmaf(e, c, *re);
    *im = __builtin_fmaf(-e, s, *im);
}

// ---- gradients ------------------------------------------------------------------------------------------------------------------
#define GS_MIX_GRAD_SUMS 10        // per row: W | v (3) | M as 00 01 02 11 12 22, the weight of each pair times (1, y', y' y'^T)

// w = M v of a row-major 3x3 M: three fused dot products (the ones of gs_mix_sq_norm)
GS_MIX_HD void gs_mix_mat_vec(const float M[9], float vx, float vy, float vz, float w[3])
{
    w[0] = __builtin_fmaf(M[0], vx, __builtin_fmaf(M[1], vy, M[2] * vz));
    w[1] = __builtin_fmaf(M[3], vx, __builtin_fmaf(M[4], vy, M[5] * vz));
    w[2] = __builtin_fmaf(M[6], vx, __builtin_fmaf(M[7], vy, M[8] * vz));
}

// acc += weight (1, v, y y^T)
GS_MIX_HD void gs_mix_add_sums(float weight, const float v[3], const float y[3], float acc[GS_MIX_GRAD_SUMS])
{
    const float w0 = weight * y[0], w1 = weight * y[1], w2 = weight * y[2];
    acc[0] += weight;
    acc[1] += v[0]; acc[2] += v[1]; acc[3] += v[2];
    acc[4] = __builtin_fmaf(w0, y[0], acc[4]); acc[5] = __builtin_fmaf(w0, y[1], acc[5]); acc[6] = __builtin_fmaf(w0, y[2], acc[6]);
    acc[7] = __builtin_fmaf(w1, y[1], acc[7]); acc[8] = __builtin_fmaf(w1, y[2], acc[8]);
    acc[9] = __builtin_fmaf(w2, y[2], acc[9]);
}

// The share of component `rec` in the density at (x, y, z), pi N / p = 2^(t - log2 p): log2 p arrives in two f32 pieces (hi + lo),
// so the difference is formed to the last bit of t.  y_out = A'(x - mu), set to 0 where the share is exactly zero (a far pair whose
// y' overflowed must not make 0 x inf).
GS_MIX_HD float gs_mix_density_share(const float rec[GS_MIX_REC_FLOATS], float x, float y, float z, float l2p_hi, float l2p_lo,
                                     float y_out[3])
{
    gs_mix_mat_vec(rec + 4, x - rec[0], y - rec[1], z - rec[2], y_out);
    const float t = rec[3] - __builtin_fmaf(y_out[0], y_out[0], __builtin_fmaf(y_out[1], y_out[1], y_out[2] * y_out[2]));
    const float e = gs_mix_exp2((t - l2p_hi) - l2p_lo);
    const bool live = e > 0.0f;                       // false for NaN as well
    for (int a = 0; a < 3; ++a) y_out[a] = live ? y_out[a] : 0.0f;
    return live ? e : 0.0f;
}

// one (query, component) pair of the density's backward: w = g pi N / p, acc += w (1, y', y' y'^T)
GS_MIX_HD void gs_mix_density_grad_term(const float rec[GS_MIX_REC_FLOATS], float x, float y, float z, float g, float l2p_hi,
                                        float l2p_lo, float acc[GS_MIX_GRAD_SUMS])
{
    float yy[3];
    const float w = g * gs_mix_density_share(rec, x, y, z, l2p_hi, l2p_lo, yy);
    const float v[3] = { w * yy[0], w * yy[1], w * yy[2] };
    gs_mix_add_sums(w, v, yy, acc);
}

// the pair's share of sum_i (pi N / p) A'^T y' at the query: d log p / dx is -2 ln 2 times the sum over the components
GS_MIX_HD void gs_mix_density_grad_x_term(const float rec[GS_MIX_REC_FLOATS], float x, float y, float z, float l2p_hi, float l2p_lo,
                                          float acc[3])
{
    float yy[3];
    const float e = gs_mix_density_share(rec, x, y, z, l2p_hi, l2p_lo, yy);
    const float* A = rec + 4;
    const float u0 = __builtin_fmaf(A[0], yy[0], __builtin_fmaf(A[3], yy[1], A[6] * yy[2]));
    const float u1 = __builtin_fmaf(A[1], yy[0], __builtin_fmaf(A[4], yy[1], A[7] * yy[2]));
    const float u2 = __builtin_fmaf(A[2], yy[0], __builtin_fmaf(A[5], yy[1], A[8] * yy[2]));
    acc[0] = __builtin_fmaf(e, u0, acc[0]); acc[1] = __builtin_fmaf(e, u1, acc[1]); acc[2] = __builtin_fmaf(e, u2, acc[2]);
}

// one (frequency, component) pair of the transform's backward: A = E (g_re cos phi - g_im sin phi), B = -E (g_re sin phi +
// g_im cos phi); acc += (A, B k, A z' z'^T).  The phase and E are formed as gs_mix_fourier_term forms them.
GS_MIX_HD void gs_mix_fourier_grad_term(const float rec[GS_MIX_REC_FLOATS], float kx, float ky, float kz, float g_re, float g_im,
                                        float acc[GS_MIX_GRAD_SUMS])
{
    const float phi = __builtin_fmaf(kx, rec[0], __builtin_fmaf(ky, rec[1], kz * rec[2]));
    float z[3];
    gs_mix_mat_vec(rec + 4, kx, ky, kz, z);
    const float e = rec[3] * gs_mix_exp2(-__builtin_fmaf(z[0], z[0], __builtin_fmaf(z[1], z[1], z[2] * z[2])));
    const bool live = e > 0.0f;
    for (int a = 0; a < 3; ++a) z[a] = live ? z[a] : 0.0f;
    float s, c;
    gs_mix_sincos(phi, &s, &c);
    const float A = live ? e * __builtin_fmaf(g_re, c, -(g_im * s)) : 0.0f;
    const float B = live ? -e * __builtin_fmaf(g_re, s, g_im * c) : 0.0f;
    const float v[3] = { B * kx, B * ky, B * kz };
    gs_mix_add_sums(A, v, z, acc);
}

// The gradients of one row from its ten sums (float64, each output rounded once).
//   density    sums = sum_p w (1, y', y' y'^T), scalar = sum_p g_p over the queries that contribute
//   transform  sums = sum_k (A, B k, A z' z'^T), scalar = sum over the rows of sum_k A
// y' and z' carry the records' factor sqrt(log2(e) / 2); it is taken out here.  grad_head = d/d(q xyzw, log s, opacity logit).
// The quaternion's gradient goes through R(q / |q|): it is orthogonal to q and scales with 1 / |q|.
GS_MIX_HD void gs_mix_grad_row(const float* feat, bool part, double total, bool fourier, const double sums[GS_MIX_GRAD_SUMS],
                               double scalar, float grad_mu[3], float grad_head[8])
{
    for (int j = 0; j < 3; ++j) grad_mu[j] = 0.0f;
    for (int j = 0; j < 8; ++j) grad_head[j] = 0.0f;
    if (!part || !(total > 0.0)) return;
    const double root = 0.84932180028801904272, inv2 = 1.38629436111989061883;     // sqrt(log2(e) / 2), 2 ln 2
    const double sig = gs_mix_sigmoid((double)feat[7]), pi = sig / total;
    double R[9], s[3], u[3];
    gs_mix_rotation(feat, R);
    for (int a = 0; a < 3; ++a) { s[a] = exp((double)feat[4 + a]); u[a] = fourier ? 1.0 / s[a] : s[a]; }
    const double W = sums[0];
    const double M[9] = { sums[4] * inv2, sums[5] * inv2, sums[6] * inv2, sums[5] * inv2, sums[7] * inv2, sums[8] * inv2,
                          sums[6] * inv2, sums[8] * inv2, sums[9] * inv2 };
    for (int i = 0; i < 3; ++i) {
        double m = sums[1 + i];                                         // transform: sum B k
        if (!fourier) {                                                 // density: R S^-1 m
            m = 0.0;
            for (int a = 0; a < 3; ++a) m += R[3 * i + a] * (sums[1 + a] / root) / s[a];
        }
        grad_mu[i] = gs_mix_round(m);
        grad_head[4 + i] = gs_mix_round(fourier ? -M[4 * i] : M[4 * i] - W);
    }
    grad_head[7] = gs_mix_round((1.0 - sig) * (W - pi * scalar));
    double G[9];                                                        // dL/dR = -R U M U^-1, U = S (density) or S^-1 (transform)
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double g = 0.0;
            for (int a = 0; a < 3; ++a) g += R[3 * i + a] * u[a] * M[3 * a + j];
            G[3 * i + j] = -g / u[j];
        }
    // R = 1 + ts N(q), ts = 2 / |q|^2, N quadratic in q: dL/dq = ts sum G dN/dq - ts^2 q sum G N
    const double x = feat[0], y = feat[1], z = feat[2], w = feat[3];
    const double ts = 2.0 / (x * x + y * y + z * z + w * w);
    double GN = 0.0;
    for (int j = 0; j < 9; ++j) GN += G[j] * (R[j] - (j % 4 == 0 ? 1.0 : 0.0));      // ts N = R - 1
    const double dq[4] = {
        (G[1] + G[3]) * y + (G[2] + G[6]) * z + (G[7] - G[5]) * w - 2.0 * x * (G[4] + G[8]),
        (G[1] + G[3]) * x + (G[5] + G[7]) * z + (G[2] - G[6]) * w - 2.0 * y * (G[0] + G[8]),
        (G[2] + G[6]) * x + (G[5] + G[7]) * y + (G[3] - G[1]) * w - 2.0 * z * (G[0] + G[4]),
        (G[3] - G[1]) * z + (G[2] - G[6]) * y + (G[7] - G[5]) * x };
    const double q[4] = { x, y, z, w };
    for (int j = 0; j < 4; ++j) grad_head[j] = gs_mix_round(ts * dq[j] - ts * q[j] * GN);     // GN already holds one factor ts
}

// ---- device-side pieces shared by k_mixture.hip and k_mixture_grad.hip -------------------------------------------------------
#if defined(__HIPCC__)
#define GS_MIX_BATCH 4                  // records per step of the loops that read records at wave-uniform addresses

// the sum of v over a workgroup of 256 lanes, as a tree in LDS: one fixed order
__device__ __forceinline__ double gs_mix_block_sum(double v, double* lds)
{
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) lds[threadIdx.x] += lds[threadIdx.x + w];
        __syncthreads();
    }
    return lds[0];
}

// GS_MIX_BATCH records from a wave-uniform index on, as arrays the pair functions read with constant subscripts
__device__ __forceinline__ void gs_mix_load_batch(const float4* __restrict__ rec, int64_t i, float (&r)[GS_MIX_BATCH][GS_MIX_REC_FLOATS])
{
#pragma unroll
    for (int u = 0; u < GS_MIX_BATCH; ++u) {
        const float4 a = rec[4 * (i + u)], b = rec[4 * (i + u) + 1], c = rec[4 * (i + u) + 2];
        const float last = rec[4 * (i + u) + 3].x;
        r[u][0] = a.x; r[u][1] = a.y; r[u][2] = a.z; r[u][3] = a.w;
        r[u][4] = b.x; r[u][5] = b.y; r[u][6] = b.z; r[u][7] = b.w;
        r[u][8] = c.x; r[u][9] = c.y; r[u][10] = c.z; r[u][11] = c.w;
        r[u][12] = last; r[u][13] = 0.0f; r[u][14] = 0.0f; r[u][15] = 0.0f;
    }
}
#endif
