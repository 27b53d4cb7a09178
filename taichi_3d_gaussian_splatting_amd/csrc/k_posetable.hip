// k_posetable.hip -- per-view camera pose corrections (include/gs_pose_table.h): compose a view's six floats onto its K base
// poses, and carry the gradient of the composed poses back to the six floats.  One thread per view, float64 behind the f32
// loads, one rounding on store.  Latency-bound launches of one wave at V = 1: nothing here is tuned for throughput.  The
// operation order, to the parenthesis, is the header's.
#include "gs_common.h"
#include "../../include/gs_pose_table.h"

// A = sin(th/2)/th, C = cos(th/2), B = (C/2 - A)/s of s = |w|^2, closed form or series (GS_POSE_SERIES_S)
template <bool WITH_B>
__device__ __forceinline__ void pose_coefficients(double s, double& A, double& C, double& B)
{
    if (s >= GS_POSE_SERIES_S) {
        const double th = sqrt(s);
        A = sin(th / 2.0) / th;
        C = cos(th / 2.0);
        if constexpr (WITH_B) B = (C / 2.0 - A) / s;
    } else {
        A = 1.0 / 2.0 + s * (-1.0 / 48.0 + s / 3840.0);
        C = 1.0 + s * (-1.0 / 8.0 + s / 384.0);
        if constexpr (WITH_B) B = -1.0 / 24.0 + s / 960.0;
    }
}

// rotation_from_quaternion (gs_point_math.h) in float64, q as stored
__device__ __forceinline__ void pose_rotation(double x, double y, double z, double w, double R[9])
{
    const double xx = x * x, yy = y * y, zz = z * z;
    const double xy = x * y, xz = x * z, yz = y * z;
    const double wx = w * x, wy = w * y, wz = w * z;
    R[0] = 1.0 - 2.0 * (yy + zz); R[1] = 2.0 * (xy - wz);       R[2] = 2.0 * (xz + wy);
    R[3] = 2.0 * (xy + wz);       R[4] = 1.0 - 2.0 * (xx + zz); R[5] = 2.0 * (yz - wx);
    R[6] = 2.0 * (xz - wy);       R[7] = 2.0 * (yz + wx);       R[8] = 1.0 - 2.0 * (xx + yy);
}

__global__ void __launch_bounds__(GS_POSE_THREADS)
k_pose_compose(const float* __restrict__ delta, const float* q_base, const float* t_base, int V, int K, float* q_out, float* t_out)
{
    const int v = blockIdx.x * GS_POSE_THREADS + threadIdx.x;
    if (v >= V) return;
    float d[GS_POSE_DELTA_FLOATS];
    bool all_zero = true, finite = true;
#pragma unroll
    for (int i = 0; i < GS_POSE_DELTA_FLOATS; ++i) {
        d[i] = delta[(size_t)v * GS_POSE_DELTA_FLOATS + i];
        all_zero = all_zero && d[i] == 0.0f;
        finite = finite && isfinite(d[i]);
    }
    const size_t row0 = (size_t)v * (size_t)K;
    if (all_zero) {                                             // selection: the base rows, bit for bit
        if (q_out != q_base)
            for (size_t i = row0 * 4; i < (row0 + K) * 4; ++i) q_out[i] = q_base[i];
        if (t_out != t_base)
            for (size_t i = row0 * 3; i < (row0 + K) * 3; ++i) t_out[i] = t_base[i];
        return;
    }
    if (!finite) {
        const float nan = __int_as_float(0x7fc00000);
        for (size_t i = row0 * 4; i < (row0 + K) * 4; ++i) q_out[i] = nan;
        for (size_t i = row0 * 3; i < (row0 + K) * 3; ++i) t_out[i] = nan;
        return;
    }
    const double w0 = d[0], w1 = d[1], w2 = d[2], u0 = d[3], u1 = d[4], u2 = d[5];
    const double s = (w0 * w0 + w1 * w1) + w2 * w2;
    double A, C, B;
    pose_coefficients<false>(s, A, C, B);
    const double x1 = A * w0, y1 = A * w1, z1 = A * w2, ww1 = C;
    for (int k = 0; k < K; ++k) {
        const float* q = q_base + (row0 + k) * 4;
        const float* t = t_base + (row0 + k) * 3;
        const double x = q[0], y = q[1], z = q[2], w = q[3];
        const double t0 = t[0], t1 = t[1], t2 = t[2];
        double R[9];
        pose_rotation(x, y, z, w, R);
        float* qo = q_out + (row0 + k) * 4;
        float* to = t_out + (row0 + k) * 3;
        qo[0] = (float)(((w * x1 + x * ww1) + y * z1) - z * y1);
        qo[1] = (float)(((w * y1 - x * z1) + y * ww1) + z * x1);
        qo[2] = (float)(((w * z1 + x * y1) - y * x1) + z * ww1);
        qo[3] = (float)(((w * ww1 - x * x1) - y * y1) - z * z1);
        to[0] = (float)(t0 + ((R[0] * u0 + R[1] * u1) + R[2] * u2));
        to[1] = (float)(t1 + ((R[3] * u0 + R[4] * u1) + R[5] * u2));
        to[2] = (float)(t2 + ((R[6] * u0 + R[7] * u1) + R[8] * u2));
    }
}

__global__ void __launch_bounds__(GS_POSE_THREADS)
k_pose_compose_backward(const float* __restrict__ delta, const float* __restrict__ q_base, const float* __restrict__ grad_q,
                        const float* __restrict__ grad_t, int V, int K, float reg, float* __restrict__ grad_delta)
{
    const int v = blockIdx.x * GS_POSE_THREADS + threadIdx.x;
    if (v >= V) return;
    double d[GS_POSE_DELTA_FLOATS];
#pragma unroll
    for (int i = 0; i < GS_POSE_DELTA_FLOATS; ++i) d[i] = delta[(size_t)v * GS_POSE_DELTA_FLOATS + i];
    const size_t row0 = (size_t)v * (size_t)K;
    double Gu[3] = { 0.0, 0.0, 0.0 }, Gdq[4] = { 0.0, 0.0, 0.0, 0.0 };
    for (int k = 0; k < K; ++k) {                               // fixed order: k = 0 up
        const float* q = q_base + (row0 + k) * 4;
        const float* gq = grad_q + (row0 + k) * 4;
        const float* gt = grad_t + (row0 + k) * 3;
        const double x = q[0], y = q[1], z = q[2], w = q[3];
        const double g0 = gq[0], g1 = gq[1], g2 = gq[2], g3 = gq[3];
        const double h0 = gt[0], h1 = gt[1], h2 = gt[2];
        double R[9];
        pose_rotation(x, y, z, w, R);
        Gu[0] += (R[0] * h0 + R[3] * h1) + R[6] * h2;
        Gu[1] += (R[1] * h0 + R[4] * h1) + R[7] * h2;
        Gu[2] += (R[2] * h0 + R[5] * h1) + R[8] * h2;
        Gdq[0] += ((w * g0 + z * g1) - y * g2) - x * g3;
        Gdq[1] += ((w * g1 - z * g0) + x * g2) - y * g3;
        Gdq[2] += ((y * g0 - x * g1) + w * g2) - z * g3;
        Gdq[3] += ((x * g0 + y * g1) + z * g2) + w * g3;
    }
    const double s = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    double A, C, B;
    pose_coefficients<true>(s, A, C, B);
    const double dot = (d[0] * Gdq[0] + d[1] * Gdq[1]) + d[2] * Gdq[2];
    const double r = (double)reg;
    float* out = grad_delta + (size_t)v * GS_POSE_DELTA_FLOATS;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double Gw = (A * Gdq[j] + (B * d[j]) * dot) - ((A * d[j]) / 2.0) * Gdq[3];
        out[j] = (float)(Gw + r * d[j]);
        out[3 + j] = (float)(Gu[j] + r * d[3 + j]);
    }
}

void gs_launch_pose_compose(const float* delta, const float* q_base, const float* t_base, int V, int K, float* q_out, float* t_out, hipStream_t s)
{
    const int blocks = (V + GS_POSE_THREADS - 1) / GS_POSE_THREADS;
    hipLaunchKernelGGL(k_pose_compose, dim3(blocks), dim3(GS_POSE_THREADS), 0, s, delta, q_base, t_base, V, K, q_out, t_out);
}

void gs_launch_pose_compose_backward(const float* delta, const float* q_base, const float* grad_q, const float* grad_t, int V, int K, float reg,
                                     float* grad_delta, hipStream_t s)
{
    const int blocks = (V + GS_POSE_THREADS - 1) / GS_POSE_THREADS;
    hipLaunchKernelGGL(k_pose_compose_backward, dim3(blocks), dim3(GS_POSE_THREADS), 0, s, delta, q_base, grad_q, grad_t, V, K, reg, grad_delta);
}
