// k_normals.hip -- include/gs_normals.h: the normal of every Gaussian (the shortest axis of its stored parametrisation, in the
// camera frame, facing the camera) with its gradient to the quaternion, and the consistency of the rendered Gaussian normals
// with the normal of the rendered depth, with its gradients to the depth and to the rendered normals.
//
// The per-row kernels have rows in lanes, one 256-thread block per 256 rows; both form the row's values by gn_row, so the
// backward holds fixed exactly the axis and the sign the forward chose.  The backward's (N,56) rows leave through LDS: the four
// quaternion gradients of the block's rows are parked there and the block writes its 256 x 56 floats as one contiguous run,
// consecutive floats in consecutive lanes, the columns 4..55 as zeros.
//
// The consistency passes are tile passes of gs_geometry_tile.h, with the normal loss's shape: the depth and the weight staged
// with a halo of 2, the interleaved rendered normals staged for the tile grown by 1 into three LDS planes (consecutive floats of
// a picture row in consecutive lanes), and in the backward what the normal at every pixel of the grown tile owes its
// neighbours formed once per block.  grad_R is written by the thread that formed the pixel's term, three floats to where they
// lie; nothing is scattered, so there is no atomic, and the order of every sum is fixed.
#include "gs_geometry_tile.h"
#include "../../include/gs_normals.h"

#include <cmath>

#define GN_BLOCK GS_NORMALS_BLOCK
#define GN_FEAT GS_NORMALS_FEATURES
static_assert(GN_BLOCK == 256 && GN_FEAT == GS_NFEAT, "a row per lane of a 256-thread block; the rasteriser's feature row");

// ---- the normal of a Gaussian ---------------------------------------------------------------------------------------------------
// R(q) of the float64 values of a stored quaternion, row-major: rotation_from_quaternion (gs_point_math.h) in float64
__device__ __forceinline__ void gn_rotation(const double q[4], double R[9])
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double xx = x * x, yy = y * y, zz = z * z;
    const double xy = x * y, xz = x * z, yz = y * z;
    const double wx = w * x, wy = w * y, wz = w * z;
    R[0] = 1.0 - 2.0 * (yy + zz); R[1] = 2.0 * (xy - wz);       R[2] = 2.0 * (xz + wy);
    R[3] = 2.0 * (xy + wz);       R[4] = 1.0 - 2.0 * (xx + zz); R[5] = 2.0 * (yz - wx);
    R[6] = 2.0 * (xz - wy);       R[7] = 2.0 * (yz + wx);       R[8] = 1.0 - 2.0 * (xx + yy);
}

// what forward and backward need of row i: the axis k, the stored quaternion, u, l, the pose rotation P and whether n = -m
struct GnRow { int k; double q[4], u[3], l, P[9], m[3]; bool flip; };

// false: the row is zeroed
__device__ __forceinline__ bool gn_row(const float* __restrict__ pc, const float* __restrict__ feat, const int32_t* __restrict__ obj,
                                       const float* __restrict__ q_pc, const float* __restrict__ t_pc, int64_t i, int K, GnRow& o)
{
    const float* f = feat + i * GN_FEAT;
    const float qf[4] = { f[0], f[1], f[2], f[3] }, s[3] = { f[4], f[5], f[6] };
    const float xf[3] = { pc[3 * i], pc[3 * i + 1], pc[3 * i + 2] };
    const int oid = obj ? obj[i] : 0;
    if (oid < 0 || oid >= K) return false;
    bool finite = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) finite = finite && fabsf(qf[j]) <= FLT_MAX;
#pragma unroll
    for (int j = 0; j < 3; ++j) finite = finite && fabsf(s[j]) <= FLT_MAX && fabsf(xf[j]) <= FLT_MAX;
    if (!finite) return false;
    int k = 0;
    if (s[1] < s[k]) k = 1;
    if (s[2] < s[k]) k = 2;
    o.k = k;
#pragma unroll
    for (int j = 0; j < 4; ++j) o.q[j] = (double)qf[j];
    if (!(((o.q[0] * o.q[0] + o.q[1] * o.q[1]) + o.q[2] * o.q[2]) + o.q[3] * o.q[3] > 0.0)) return false;
    double R[9];
    gn_rotation(o.q, R);
    const double c[3] = { k == 0 ? R[0] : k == 1 ? R[1] : R[2], k == 0 ? R[3] : k == 1 ? R[4] : R[5], k == 0 ? R[6] : k == 1 ? R[7] : R[8] };
    const double l2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
    if (!(l2 > 0.0 && l2 <= DBL_MAX)) return false;
    o.l = sqrt(l2);
#pragma unroll
    for (int j = 0; j < 3; ++j) o.u[j] = c[j] / o.l;
    const double qo[4] = { (double)q_pc[4 * oid], (double)q_pc[4 * oid + 1], (double)q_pc[4 * oid + 2], (double)q_pc[4 * oid + 3] };
    gn_rotation(qo, o.P);
    const double d[3] = { (double)xf[0] - (double)t_pc[3 * oid], (double)xf[1] - (double)t_pc[3 * oid + 1], (double)xf[2] - (double)t_pc[3 * oid + 2] };
    double p[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        o.m[j] = (o.P[j] * o.u[0] + o.P[3 + j] * o.u[1]) + o.P[6 + j] * o.u[2];
        p[j] = (o.P[j] * d[0] + o.P[3 + j] * d[1]) + o.P[6 + j] * d[2];
    }
    const double a = (o.m[0] * p[0] + o.m[1] * p[1]) + o.m[2] * p[2];
    o.flip = !(a <= 0.0);
    return true;
}

__global__ __launch_bounds__(GN_BLOCK) void k_gaussian_normals(const float* __restrict__ pc, const float* __restrict__ feat,
                                                              const int32_t* __restrict__ obj, const float* __restrict__ q_pc,
                                                              const float* __restrict__ t_pc, int64_t N, int K, float* __restrict__ normals)
{
    const int64_t i = (int64_t)blockIdx.x * GN_BLOCK + threadIdx.x;
    if (i >= N) return;
    GnRow r;
    float n[3] = { 0.0f, 0.0f, 0.0f };
    if (gn_row(pc, feat, obj, q_pc, t_pc, i, K, r)) {
#pragma unroll
        for (int j = 0; j < 3; ++j) n[j] = (float)(r.flip ? -r.m[j] : r.m[j]);
    }
    normals[3 * i] = n[0]; normals[3 * i + 1] = n[1]; normals[3 * i + 2] = n[2];
}

// J[e][j] = d c_j / d q_e of column k of R(q), e = x, y, z, w
__device__ __forceinline__ void gn_column_partials(int k, const double q[4], double J[4][3])
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    if (k == 0) {
        J[0][0] = 0.0;      J[0][1] = 2.0 * y;  J[0][2] = 2.0 * z;
        J[1][0] = -4.0 * y; J[1][1] = 2.0 * x;  J[1][2] = -2.0 * w;
        J[2][0] = -4.0 * z; J[2][1] = 2.0 * w;  J[2][2] = 2.0 * x;
        J[3][0] = 0.0;      J[3][1] = 2.0 * z;  J[3][2] = -2.0 * y;
    } else if (k == 1) {
        J[0][0] = 2.0 * y;  J[0][1] = -4.0 * x; J[0][2] = 2.0 * w;
        J[1][0] = 2.0 * x;  J[1][1] = 0.0;      J[1][2] = 2.0 * z;
        J[2][0] = -2.0 * w; J[2][1] = -4.0 * z; J[2][2] = 2.0 * y;
        J[3][0] = -2.0 * z; J[3][1] = 0.0;      J[3][2] = 2.0 * x;
    } else {
        J[0][0] = 2.0 * z;  J[0][1] = -2.0 * w; J[0][2] = -4.0 * x;
        J[1][0] = 2.0 * w;  J[1][1] = 2.0 * z;  J[1][2] = -4.0 * y;
        J[2][0] = 2.0 * x;  J[2][1] = 2.0 * y;  J[2][2] = 0.0;
        J[3][0] = 2.0 * y;  J[3][1] = -2.0 * x; J[3][2] = 0.0;
    }
}

__global__ __launch_bounds__(GN_BLOCK) void k_gaussian_normals_grad(const float* __restrict__ pc, const float* __restrict__ feat,
                                                                   const int32_t* __restrict__ obj, const float* __restrict__ q_pc,
                                                                   const float* __restrict__ t_pc, int64_t N, int K,
                                                                   const float* __restrict__ grad_normals, float* __restrict__ grad_feat)
{
    __shared__ float sG[GN_BLOCK][4];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * GN_BLOCK, i = row0 + t;
    float gq[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    GnRow r;
    if (i < N && gn_row(pc, feat, obj, q_pc, t_pc, i, K, r)) {
        double gm[3], gu[3], gc[3], J[4][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) { const double g = (double)grad_normals[3 * i + j]; gm[j] = r.flip ? -g : g; }
#pragma unroll
        for (int j = 0; j < 3; ++j) gu[j] = (r.P[3 * j] * gm[0] + r.P[3 * j + 1] * gm[1]) + r.P[3 * j + 2] * gm[2];
        const double b = (gu[0] * r.u[0] + gu[1] * r.u[1]) + gu[2] * r.u[2];
#pragma unroll
        for (int j = 0; j < 3; ++j) gc[j] = (gu[j] - b * r.u[j]) / r.l;
        gn_column_partials(r.k, r.q, J);
#pragma unroll
        for (int e = 0; e < 4; ++e) gq[e] = (float)((J[e][0] * gc[0] + J[e][1] * gc[1]) + J[e][2] * gc[2]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) sG[t][e] = gq[e];
    __syncthreads();
    // the block's rows are one contiguous run of floats: consecutive floats in consecutive lanes
    const int64_t rows = N - row0 < GN_BLOCK ? N - row0 : GN_BLOCK;
    float* out = grad_feat + row0 * GN_FEAT;
    for (int idx = t; idx < (int)rows * GN_FEAT; idx += GN_BLOCK) {
        const int row = idx / GN_FEAT, col = idx % GN_FEAT;
        out[idx] = col < 4 ? sG[row][col] : 0.0f;
    }
}

// ---- the consistency loss -------------------------------------------------------------------------------------------------------
#define GC_RP ((GT_H + 2) * GT_P)                  // floats of a staged plane of R: the rows of the tile grown by 1
#define GC_RW (GT_W + 2)                           // its columns

// the interleaved R of the tile grown by 1 -> three planes sR[j * GC_RP + (ly - 1) * GT_P + lx]; outside the picture 0 (not usable)
__device__ __forceinline__ void gc_stage_rendered(const float* __restrict__ R, int H, int W, GtTile tl, float* __restrict__ sR)
{
    for (int item = threadIdx.x; item < (GT_H + 2) * GC_RW * 3; item += GT_THREADS) {
        const int ry = item / (GC_RW * 3), j = item % (GC_RW * 3), rx = j / 3, ch = j % 3;
        const int y = tl.y0 - 1 + ry, x = tl.x0 - 1 + rx;
        const float v = (y >= 0 && y < H && x >= 0 && x < W) ? R[((size_t)y * W + x) * 3 + ch] : 0.0f;
        sR[ch * GC_RP + ry * GT_P + (GT_PAD - 1) + rx] = v;
    }
}

// a selected pixel: the normal loss's term with h = R / |R|, and |R|
struct GcTerm { GtNormalTerm t; double k; };

// staged at (lx, ly) with GT_PAD - 1 <= lx <= GT_PAD + GT_W and 1 <= ly <= GT_R - 2
__device__ __forceinline__ bool gc_term(const float* __restrict__ sD, const float* __restrict__ sW, const float* __restrict__ sR,
                                        const double* __restrict__ sA, const double* __restrict__ sB, int lx, int ly, int x, int y, int H, int W,
                                        float jump, float min_length, GcTerm& o)
{
    const float w = sW[ly * GT_P + lx];
    if (!(w > 0.0f)) return false;
    if (!gt_normal(sD, sA, sB, lx, ly, x, y, H, W, jump, o.t.g)) return false;
    const int ri = (ly - 1) * GT_P + lx;
    const double m[3] = { (double)sR[ri], (double)sR[GC_RP + ri], (double)sR[2 * GC_RP + ri] };
    const double kk = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
    if (!(kk >= (double)min_length && kk <= DBL_MAX)) return false;
#pragma unroll
    for (int j = 0; j < 3; ++j) { o.t.h[j] = m[j] / kk; o.t.n[j] = o.t.g.c[j] / o.t.g.len; }
    o.t.cos = (o.t.n[0] * o.t.h[0] + o.t.n[1] * o.t.h[1]) + o.t.n[2] * o.t.h[2];
    o.t.w = w;
    o.k = kk;
    return true;
}

template <bool BACKWARD>
__global__ __launch_bounds__(GT_THREADS) void k_normal_consistency(const float* __restrict__ D, const float* __restrict__ R, const float* __restrict__ wp,
                                                                  int vec, int H, int W, GtCam K, float jump, float min_length,
                                                                  double* __restrict__ partial, int nb, const float* __restrict__ terms,
                                                                  const float* __restrict__ upstream, float* __restrict__ G, float* __restrict__ GR)
{
    __shared__ __align__(16) float sD[GT_R * GT_P];
    __shared__ __align__(16) float sW[GT_R * GT_P];
    __shared__ float sR[3 * GC_RP];
    __shared__ __align__(16) float sO[BACKWARD ? GT_H * GT_W : 4];
    __shared__ double sA[GT_P], sB[GT_R];
    __shared__ double sOwes[BACKWARD ? 4 * GN_TERMS : 1];
    __shared__ uint8_t sSel[BACKWARD ? GN_TERMS : 1];
    const GtTile tl = gt_tile(W);
    gt_stage<0>(D, (vec & GT_VEC_D) != 0, H, W, tl, sD);
    gt_stage<1>(wp, (vec & GT_VEC_WP) != 0, H, W, tl, sW);
    gc_stage_rendered(R, H, W, tl, sR);
    gt_stage_camera(K, tl, sA, sB);
    __syncthreads();

    if constexpr (!BACKWARD) {
        double acc[GT_SUMS] = { 0.0, 0.0, 0.0, 0.0 };
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            GT_PIXEL(k);
            (void)li;
            GcTerm o;
            if (inside && gc_term(sD, sW, sR, sA, sB, lx, ly, x, y, H, W, jump, min_length, o)) {
                acc[0] += (double)o.t.w * (1.0 - o.t.cos); acc[1] += (double)o.t.w; acc[2] += 1.0; acc[3] += o.t.cos;
            }
        }
        gt_block_sums(acc, partial, nb);
    } else {
        const float Sw = terms[1];
        const float u = upstream ? upstream[0] : 1.0f;
        const double s = Sw > 0.0f ? (double)u / (double)Sw : 0.0;
        // every term the tile's pixels gather from, once: item = (hy, hx) of the tile grown by 1 on every side; the term of a pixel
        // of the tile itself also gives that pixel's grad_R
#pragma unroll 1
        for (int item = threadIdx.x; item < GN_TERMS; item += GT_THREADS) {
            const int hy = item / GN_W, hx = item % GN_W;
            const int lx = hx + GT_PAD - 1, ly = hy + GT_HALO - 1;
            const int x = tl.x0 + hx - 1, y = tl.y0 + hy - 1;
            GcTerm o;
            double owes[4] = { 0.0, 0.0, 0.0, 0.0 };
            const bool sel = Sw > 0.0f && gc_term(sD, sW, sR, sA, sB, lx, ly, x, y, H, W, jump, min_length, o);
            if (sel) gt_owes(o.t, sA, sB, lx, ly, s, owes);
            sSel[item] = sel ? 1 : 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) sOwes[j * GN_TERMS + item] = owes[j];
            if (hx >= 1 && hx <= GT_W && hy >= 1 && hy <= GT_H && x < W && y < H) {       // (x, y >= 0 there)
                float gr[3] = { 0.0f, 0.0f, 0.0f };
                if (sel) {
                    const double coef = -(s * (double)o.t.w);
#pragma unroll
                    for (int j = 0; j < 3; ++j) gr[j] = (float)((coef * (o.t.n[j] - o.t.cos * o.t.h[j])) / o.k);
                }
                float* dst = GR + ((size_t)y * W + x) * 3;
                dst[0] = gr[0]; dst[1] = gr[1]; dst[2] = gr[2];
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            GT_PIXEL(k);
            (void)li; (void)lx; (void)ly; (void)x; (void)y;
            double acc = 0.0;
            bool any = false;
            if (inside) {
                const int c = (ty + 1) * GN_W + tx + 1;             // this pixel among the terms
                if (sSel[c - 1]) { acc += sOwes[0 * GN_TERMS + c - 1]; any = true; }            // the left neighbour owes its right
                if (sSel[c + 1]) { acc += sOwes[1 * GN_TERMS + c + 1]; any = true; }            // the right neighbour its left
                if (sSel[c - GN_W]) { acc += sOwes[2 * GN_TERMS + c - GN_W]; any = true; }      // the upper neighbour its down
                if (sSel[c + GN_W]) { acc += sOwes[3 * GN_TERMS + c + GN_W]; any = true; }      // the lower neighbour its up
            }
            sO[ty * GT_W + tx] = any ? (float)acc : 0.0f;
        }
        __syncthreads();
        gt_store(sO, G, (vec & GT_VEC_G) != 0, H, W, tl);
    }
}

// ---- the launchers --------------------------------------------------------------------------------------------------------------
static int gc_vec(int W, const float* D, const float* wp, const float* G)
{
    return (gt_vec_ok(W, D) ? GT_VEC_D : 0) | (gt_vec_ok(W, wp) ? GT_VEC_WP : 0) | (gt_vec_ok(W, G) ? GT_VEC_G : 0);
}

void gs_launch_gaussian_normals_forward(const float* pc, const float* feat, const int32_t* obj, const float* q_pc, const float* t_pc, int64_t N,
                                        int K, float* normals, hipStream_t s)
{
    k_gaussian_normals<<<(unsigned)((N + GN_BLOCK - 1) / GN_BLOCK), GN_BLOCK, 0, s>>>(pc, feat, obj, q_pc, t_pc, N, K, normals);
}

void gs_launch_gaussian_normals_backward(const float* pc, const float* feat, const int32_t* obj, const float* q_pc, const float* t_pc, int64_t N,
                                         int K, const float* grad_normals, float* grad_feat, hipStream_t s)
{
    k_gaussian_normals_grad<<<(unsigned)((N + GN_BLOCK - 1) / GN_BLOCK), GN_BLOCK, 0, s>>>(pc, feat, obj, q_pc, t_pc, N, K, grad_normals, grad_feat);
}

void gs_launch_normal_consistency_forward(const float* D, const float* R, const float* wp, int H, int W, float fx, float fy, float cx, float cy,
                                          float jump, float min_length, float* terms, void* ws, hipStream_t s)
{
    const int nb = gt_tiles(H, W);
    double* partial = static_cast<double*>(ws);
    k_normal_consistency<false><<<nb, GT_THREADS, 0, s>>>(D, R, wp, gc_vec(W, D, wp, nullptr), H, W, gt_cam(fx, fy, cx, cy), jump, min_length, partial,
                                                          nb, nullptr, nullptr, nullptr, nullptr);
    gs_launch_geometry_finish(partial, nb, 1, terms, s);
}

void gs_launch_normal_consistency_backward(const float* D, const float* R, const float* wp, int H, int W, float fx, float fy, float cx, float cy,
                                           float jump, float min_length, const float* terms, const float* upstream, float* G, float* GR,
                                           hipStream_t s)
{
    k_normal_consistency<true><<<gt_tiles(H, W), GT_THREADS, 0, s>>>(D, R, wp, gc_vec(W, D, wp, G), H, W, gt_cam(fx, fy, cx, cy), jump, min_length,
                                                                     nullptr, 0, terms, upstream, G, GR);
}
