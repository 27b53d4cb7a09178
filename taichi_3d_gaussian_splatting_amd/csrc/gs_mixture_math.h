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
