// gs_point_math.h -- the per-point math the projection (k_project.hip), loop 2 of the backward (k_backward.hip: k_bwd_points), the
// pose gradient (k_pose.hip) and the density controller (k_density.hip) share, each piece stated once.  These expressions decide
// indices (gs_common.h, "Arithmetic contract"): the operation order, to the parenthesis, is part of their definition.
#pragma once
#include "gs_common.h"

// One 56-float feature row (q xyzw | log s | opacity logit | 3 x 16 SH coefficients) into registers: fourteen 16-byte loads.
__device__ __forceinline__ void gs_load_feat_row(const float4* row4, float (&row)[GS_NFEAT])
{
#pragma unroll
    for (int k = 0; k < GS_NFEAT / 4; ++k) {
        const float4 v = row4[k];
        row[4 * k] = v.x; row[4 * k + 1] = v.y; row[4 * k + 2] = v.z; row[4 * k + 3] = v.w;
    }
}

// rotation_matrix_from_quaternion, GP3D:30-48: q = xyzw as stored (not normalised, as in the reference), R row-major
__device__ __forceinline__ void rotation_from_quaternion(const float q[4], float R[9])
{
    float x = q[0], y = q[1], z = q[2], w = q[3];
    float xx = x * x, yy = y * y, zz = z * z;
    float xy = x * y, xz = x * z, yz = y * z;
    float wx = w * x, wy = w * y, wz = w * z;
    R[0] = 1.0f - 2.0f * (yy + zz); R[1] = 2.0f * (xy - wz);        R[2] = 2.0f * (xz + wy);
    R[3] = 2.0f * (xy + wz);        R[4] = 1.0f - 2.0f * (xx + zz); R[5] = 2.0f * (yz - wx);
    R[6] = 2.0f * (xz - wy);        R[7] = 2.0f * (yz + wx);        R[8] = 1.0f - 2.0f * (xx + yy);
}

// Sigma = R S S R^T of a feature row (q = row[0..3], S = diag(exp(row[4..6]))), GP3D:161-191: the same three-product chain as
// the Python
__device__ __forceinline__ void gs_sigma_from_row(const float* row, float Sigma[9])
{
    float R[9];
    rotation_from_quaternion(row, R);
    float es0 = gs_expf(row[4]), es1 = gs_expf(row[5]), es2 = gs_expf(row[6]);
    float S[9] = { es0, 0.0f, 0.0f, 0.0f, es1, 0.0f, 0.0f, 0.0f, es2 };   // S == S^T
    float Rt[9] = { R[0], R[3], R[6], R[1], R[4], R[7], R[2], R[5], R[8] };
    float RS[9], RSS[9];
    gs_mm<3, 3, 3>(R, S, RS);
    gs_mm<3, 3, 3>(RS, S, RSS);
    gs_mm<3, 3, 3>(RSS, Rt, Sigma);
}

// The 2x3 Jacobian of the perspective projection at the camera-space point p (GP3D:161-191, 237-331), row-major
__device__ __forceinline__ void gs_projection_jacobian(float fx, float fy, float px, float py, float pz, float J[6])
{
    J[0] = fx / pz; J[1] = 0.0f; J[2] = -(fx * px) / (pz * pz);
    J[3] = 0.0f; J[4] = fy / pz; J[5] = -(fy * py) / (pz * pz);
}

// The 16 real spherical-harmonics basis values of a unit direction, SH:10-53
__device__ __forceinline__ void gs_sh16(float x, float y, float z, float sh[16])
{
    sh[0] = 0.28209479177387814f;
    sh[1] = -0.48860251190291987f * y;
    sh[2] = 0.48860251190291987f * z;
    sh[3] = -0.48860251190291987f * x;
    sh[4] = 1.0925484305920792f * x * y;
    sh[5] = -1.0925484305920792f * y * z;
    sh[6] = 0.94617469575755997f * z * z - 0.31539156525251999f;
    sh[7] = -1.0925484305920792f * x * z;
    sh[8] = 0.54627421529603959f * x * x - 0.54627421529603959f * y * y;
    sh[9] = 0.59004358992664352f * y * (-3.0f * x * x + y * y);
    sh[10] = 2.8906114426405538f * x * y * z;
    sh[11] = 0.45704579946446572f * y * (1.0f - 5.0f * z * z);
    sh[12] = 0.3731763325901154f * z * (5.0f * z * z - 3.0f);
    sh[13] = 0.45704579946446572f * x * (1.0f - 5.0f * z * z);
    sh[14] = 1.4453057213202769f * z * (x * x - y * y);
    sh[15] = 0.59004358992664352f * x * (-x * x + 3.0f * y * y);
}

// ---- rows of per-splat sums ---------------------------------------------------------------------------------------
// A row of `partial` (per point and tile) or of the per-point sums, as the three float4 it is loaded and stored as, column by
// column; the layout is PW's (k_backward.hip) = GS_SPLAT_SUM_FLOATS' (gs_rasterizer.h).  The count is an integer end to end.
struct GsRow { float vs0, vs1, cov00, cov01, cov11, col[3], opacity, mag; int count; float depth; };
__device__ __forceinline__ int gs_row_count(const float4 c) { return __float_as_int(c.z); }
__device__ __forceinline__ GsRow gs_row(const float4 a, const float4 b, const float4 c)
{
    return GsRow{ a.x, a.y, a.z, a.w, b.x, { b.y, b.z, b.w }, c.x, c.y, gs_row_count(c), c.w };
}
// a row added to ten running values + the integer count (AUX: column 11, d depth, into w[10] too)
template <bool AUX>
__device__ __forceinline__ void gs_row_add(float (&w)[11], int& count, const float4 a, const float4 b, const float4 c)
{
    const GsRow r = gs_row(a, b, c);
    w[0] += r.vs0; w[1] += r.vs1; w[2] += r.cov00; w[3] += r.cov01; w[4] += r.cov11; w[5] += r.col[0]; w[6] += r.col[1]; w[7] += r.col[2];
    w[8] += r.opacity; w[9] += r.mag; count += r.count;
    if constexpr (AUX) w[10] += r.depth;
}
// those values as a row of the sums (column 11: 0 unless AUX -- the staged path's sums keep it so)
template <bool AUX>
__device__ __forceinline__ void gs_row_store(float4* row, const float (&w)[11], const int count)
{
    row[0] = make_float4(w[0], w[1], w[2], w[3]);
    row[1] = make_float4(w[4], w[5], w[6], w[7]);
    row[2] = make_float4(w[8], w[9], __int_as_float(count), AUX ? w[10] : 0.0f);
}

// ---- pose gradient (k_pose.hip) ---------------------------------------------------------------------------------
// d/d(unit direction) of those 16 values as the forward evaluates them (GP3D:333-349), contracted with gY = dL/dY:
// g = sum_k gY[k] * dY_k/d(x, y, z), the derivative of the polynomial, not of its projection onto the sphere.
__device__ __forceinline__ void gs_sh16_grad_dir(float x, float y, float z, const float gY[16], float g[3])
{
    const float c1 = 0.48860251190291987f, c4 = 1.0925484305920792f, c6 = 0.94617469575755997f, c8 = 0.54627421529603959f;
    const float c9 = 0.59004358992664352f, c10 = 2.8906114426405538f, c11 = 0.45704579946446572f, c12 = 0.3731763325901154f;
    const float c14 = 1.4453057213202769f;
    const float xx = x * x, yy = y * y, zz = z * z;
    float gx = -c1 * gY[3], gy = -c1 * gY[1], gz = c1 * gY[2];
    gx += c4 * y * gY[4];                      gy += c4 * x * gY[4];
    gy += -c4 * z * gY[5];                     gz += -c4 * y * gY[5];
    gz += 2.0f * c6 * z * gY[6];
    gx += -c4 * z * gY[7];                     gz += -c4 * x * gY[7];
    gx += 2.0f * c8 * x * gY[8];               gy += -2.0f * c8 * y * gY[8];
    gx += -6.0f * c9 * x * y * gY[9];          gy += 3.0f * c9 * (yy - xx) * gY[9];
    gx += c10 * y * z * gY[10];                gy += c10 * x * z * gY[10];               gz += c10 * x * y * gY[10];
    gy += c11 * (1.0f - 5.0f * zz) * gY[11];   gz += -10.0f * c11 * y * z * gY[11];
    gz += c12 * (15.0f * zz - 3.0f) * gY[12];
    gx += c11 * (1.0f - 5.0f * zz) * gY[13];   gz += -10.0f * c11 * x * z * gY[13];
    gx += 2.0f * c14 * x * z * gY[14];         gy += -2.0f * c14 * y * z * gY[14];       gz += c14 * (xx - yy) * gY[14];
    gx += 3.0f * c9 * (yy - xx) * gY[15];      gy += 6.0f * c9 * x * y * gY[15];
    g[0] = gx; g[1] = gy; g[2] = gz;
}
