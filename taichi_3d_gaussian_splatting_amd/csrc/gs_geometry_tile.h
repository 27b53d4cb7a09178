// gs_geometry_tile.h -- what the tile passes over the rendered depth share (k_geometry.hip, k_normals.hip), each piece stated
// once: the staging of a plane's tile with its halo in LDS, the depth normal of include/gs_geometry.h and what it owes its
// neighbours, the smoothness terms, and the fixed-order float64 sums.  The layout is described at the head of k_geometry.hip.
#pragma once
#include "gs_common.h"
#include "../../include/gs_geometry.h"

#include <cfloat>

#define GT_W GS_GEOM_TILE_W
#define GT_H GS_GEOM_TILE_H
#define GT_HALO GS_GEOM_HALO
#define GT_THREADS 256
#define GT_WAVES (GT_THREADS / 64)
#define GT_PAD 4                                   // floats left of the tile in a staged row
#define GT_P (GT_W + 2 * GT_PAD)                   // floats of a staged row
#define GT_R (GT_H + 2 * GT_HALO)                  // staged rows
#define GT_FIN GS_GEOM_FINISH_THREADS
#define GT_SUMS 4                                  // sum w v, sum w, the number of selected terms, sum cos
#define GN_W (GT_W + 2)                            // the normals a tile's gradient gathers from: the tile grown by 1 on every side
#define GN_TERMS ((GT_H + 2) * GN_W)
static_assert(GT_W == 64 && GT_H * GT_W == 4 * GT_THREADS, "a wave per tile row, four rows per thread");
static_assert(GT_HALO <= GT_PAD && GT_PAD % 4 == 0 && GT_P % 4 == 0, "the tile's columns are 16-byte aligned in a staged row");
static_assert(GT_FIN % 64 == 0 && GT_FIN <= 1024, "whole waves in the finishing block");

// bits of `vec`: the plane is 16-byte aligned (and W a multiple of 4)
#define GT_VEC_D 1
#define GT_VEC_A 2          // N or I
#define GT_VEC_WN 4
#define GT_VEC_WP 8
#define GT_VEC_G 16

struct GtCam { double fx, fy, cx, cy; };
struct GtTile { int x0, y0; };

__device__ __forceinline__ GtTile gt_tile(int W)
{
    const int tiles_x = (W + GT_W - 1) / GT_W;
    GtTile t;
    t.x0 = (int)(blockIdx.x % (unsigned)tiles_x) * GT_W;
    t.y0 = (int)(blockIdx.x / (unsigned)tiles_x) * GT_H;
    return t;
}

// MODE 0: the value as stored; 1: a = v > 0 ? v : 0; 2: what LDS holds times a
template <int MODE>
__device__ __forceinline__ void gt_put(float* __restrict__ lds, int i, float v)
{
    if (MODE == 0) { lds[i] = v; return; }
    const float a = v > 0.0f ? v : 0.0f;
    if (MODE == 1) lds[i] = a; else lds[i] = lds[i] * a;
}

// the tile of plane q with its halo -> lds[GT_R * GT_P]; outside the picture 0.  q == NULL: 1 everywhere (a weight that is not there)
template <int MODE>
__device__ __forceinline__ void gt_stage(const float* __restrict__ q, bool vec, int H, int W, GtTile tl, float* __restrict__ lds)
{
    const int t = threadIdx.x;
    if (!q) {
        if (MODE != 2)
            for (int i = t; i < GT_R * GT_P; i += GT_THREADS) lds[i] = 1.0f;
        return;
    }
    if (vec) {
        for (int item = t; item < GT_R * (GT_W / 4); item += GT_THREADS) {
            const int ly = item / (GT_W / 4), g = item % (GT_W / 4);
            const int y = tl.y0 - GT_HALO + ly, x = tl.x0 + 4 * g;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (y >= 0 && y < H && x < W) v = *reinterpret_cast<const float4*>(q + (size_t)y * W + x);      // W % 4 == 0: x + 3 < W
            const int i = ly * GT_P + GT_PAD + 4 * g;
            gt_put<MODE>(lds, i, v.x); gt_put<MODE>(lds, i + 1, v.y); gt_put<MODE>(lds, i + 2, v.z); gt_put<MODE>(lds, i + 3, v.w);
        }
        for (int item = t; item < GT_R * 2 * GT_HALO; item += GT_THREADS) {
            const int ly = item / (2 * GT_HALO), c = item % (2 * GT_HALO);
            const int lx = c < GT_HALO ? GT_PAD - GT_HALO + c : GT_PAD + GT_W + (c - GT_HALO);
            const int y = tl.y0 - GT_HALO + ly, x = tl.x0 - GT_PAD + lx;
            const float v = (y >= 0 && y < H && x >= 0 && x < W) ? q[(size_t)y * W + x] : 0.0f;
            gt_put<MODE>(lds, ly * GT_P + lx, v);
        }
    } else {
        for (int item = t; item < GT_R * (GT_W + 2 * GT_HALO); item += GT_THREADS) {
            const int ly = item / (GT_W + 2 * GT_HALO), lx = GT_PAD - GT_HALO + item % (GT_W + 2 * GT_HALO);
            const int y = tl.y0 - GT_HALO + ly, x = tl.x0 - GT_PAD + lx;
            const float v = (y >= 0 && y < H && x >= 0 && x < W) ? q[(size_t)y * W + x] : 0.0f;
            gt_put<MODE>(lds, ly * GT_P + lx, v);
        }
    }
}

// a result tile out[GT_H * GT_W] (rows of GT_W) -> plane G
__device__ __forceinline__ void gt_store(const float* __restrict__ out, float* __restrict__ G, bool vec, int H, int W, GtTile tl)
{
    const int t = threadIdx.x, row = t / (GT_W / 4), g = t % (GT_W / 4);
    const int y = tl.y0 + row, x = tl.x0 + 4 * g;
    if (y >= H || x >= W) return;
    const float* o = out + row * GT_W + 4 * g;
    float* dst = G + (size_t)y * W + x;
    if (vec) {
        *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(o);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x + j < W) dst[j] = o[j];
    }
}

__device__ __forceinline__ bool gt_valid(float d) { return d > 0.0f && d <= FLT_MAX; }

// a_x of the staged columns and b_y of the staged rows, once per block: sA[lx] belongs to x = x0 - GT_PAD + lx, sB[ly] to
// y = y0 - GT_HALO + ly (a division each; a normal reads six of them)
__device__ __forceinline__ void gt_stage_camera(const GtCam& K, GtTile tl, double* __restrict__ sA, double* __restrict__ sB)
{
    const int t = threadIdx.x;
    if (t < GT_P) sA[t] = ((double)(tl.x0 - GT_PAD + t) + 0.5 - K.cx) / K.fx;
    else if (t < GT_P + GT_R) sB[t - GT_P] = ((double)(tl.y0 - GT_HALO + (t - GT_P)) + 0.5 - K.cy) / K.fy;
}
__device__ __forceinline__ double gt_sign(double r) { return (double)(r > 0.0) - (double)(r < 0.0); }

// ---- the normal ---------------------------------------------------------------------------------------------------------------
struct GtNormal { double px[3], py[3], c[3], len; };

// the normal at picture pixel (x, y), staged at column lx of row ly; false: it does not exist
__device__ __forceinline__ bool gt_normal(const float* __restrict__ sD, const double* __restrict__ sA, const double* __restrict__ sB, int lx, int ly,
                                          int x, int y, int H, int W, float jump, GtNormal& o)
{
    if (x < 1 || x > W - 2 || y < 1 || y > H - 2) return false;
    const int li = ly * GT_P + lx;
    const float l = sD[li - 1], r = sD[li + 1], u = sD[li - GT_P], d = sD[li + GT_P], m = sD[li];
    if (!(gt_valid(l) && gt_valid(r) && gt_valid(u) && gt_valid(d) && gt_valid(m))) return false;
    const double dx = (double)r - (double)l, dy = (double)d - (double)u;
    if (jump > 0.0f) {
        const double lim = (double)jump * (double)m;
        if (!(fabs(dx) <= lim && fabs(dy) <= lim)) return false;
    }
    o.px[0] = sA[lx + 1] * (double)r - sA[lx - 1] * (double)l; o.px[1] = sB[ly] * dx; o.px[2] = dx;
    o.py[0] = sA[lx] * dy; o.py[1] = sB[ly + 1] * (double)d - sB[ly - 1] * (double)u; o.py[2] = dy;
    o.c[0] = o.py[1] * o.px[2] - o.py[2] * o.px[1];
    o.c[1] = o.py[2] * o.px[0] - o.py[0] * o.px[2];
    o.c[2] = o.py[0] * o.px[1] - o.py[1] * o.px[0];
    const double q = (o.c[0] * o.c[0] + o.c[1] * o.c[1]) + o.c[2] * o.c[2];
    if (!(q > 0.0 && q <= DBL_MAX)) return false;
    o.len = sqrt(q);
    return true;
}

// a selected pixel of the normal loss: its normal, the unit prior h, n, cos and the weight
struct GtNormalTerm { GtNormal g; double n[3], h[3], cos; float w; };

__device__ __forceinline__ bool gt_normal_term(const float* __restrict__ sD, const float* __restrict__ sW, const float* __restrict__ sN,
                                               const double* __restrict__ sA, const double* __restrict__ sB, int lx, int ly, int x, int y, int H, int W,
                                               float jump, int flags, GtNormalTerm& o)
{
    const int li = ly * GT_P + lx;
    const float w = sW[li];
    if (!(w > 0.0f)) return false;
    if (!gt_normal(sD, sA, sB, lx, ly, x, y, H, W, jump, o.g)) return false;
    double m[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double v = (double)sN[k * (GT_R * GT_P) + li];
        m[k] = (flags & GS_GEOM_PRIOR_UNIT_RANGE) ? 2.0 * v - 1.0 : v;
    }
    if (flags & GS_GEOM_PRIOR_FLIP_YZ) { m[1] = -m[1]; m[2] = -m[2]; }
    const double kk = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
    if (!(kk >= 0.5 && kk <= DBL_MAX)) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) { o.h[k] = m[k] / kk; o.n[k] = o.g.c[k] / o.g.len; }
    o.cos = (o.n[0] * o.h[0] + o.n[1] * o.h[1]) + o.n[2] * o.h[2];
    o.w = w;
    return true;
}

// what the normal of term o, staged at (lx, ly), owes its neighbours: owes[0] right, [1] left, [2] down, [3] up
__device__ __forceinline__ void gt_owes(const GtNormalTerm& o, const double* __restrict__ sA, const double* __restrict__ sB, int lx, int ly, double s,
                                        double owes[4])
{
    const double coef = -(s * (double)o.w);
    double g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = (coef * (o.h[k] - o.cos * o.n[k])) / o.g.len;
    const double* px = o.g.px;
    const double* py = o.g.py;
    const double gx0 = g[1] * py[2] - g[2] * py[1], gx1 = g[2] * py[0] - g[0] * py[2], gx2 = g[0] * py[1] - g[1] * py[0];
    const double gy0 = px[1] * g[2] - px[2] * g[1], gy1 = px[2] * g[0] - px[0] * g[2], gy2 = px[0] * g[1] - px[1] * g[0];
    owes[0] = (gx0 * sA[lx + 1] + gx1 * sB[ly]) + gx2;
    owes[1] = -((gx0 * sA[lx - 1] + gx1 * sB[ly]) + gx2);
    owes[2] = (gy0 * sA[lx] + gy1 * sB[ly + 1]) + gy2;
    owes[3] = -((gy0 * sA[lx] + gy1 * sB[ly - 1]) + gy2);
}

// ---- the smoothness -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double gt_space(float d, int flags) { return (flags & GS_GEOM_INVERSE) ? 1.0 / (double)d : (double)d; }

// e of the staged guide pixels i, j (sI == NULL: 1); false: the guide unselects the term
__device__ __forceinline__ bool gt_edge(const float* __restrict__ sI, int i, int j, float lambda, double& e)
{
    if (!sI) { e = 1.0; return true; }
    const double dr = fabs((double)sI[j] - (double)sI[i]);
    const double dg = fabs((double)sI[GT_R * GT_P + j] - (double)sI[GT_R * GT_P + i]);
    const double db = fabs((double)sI[2 * GT_R * GT_P + j] - (double)sI[2 * GT_R * GT_P + i]);
    const double t = ((dr + dg) + db) / 3.0;
    if (!(t <= DBL_MAX)) return false;
    e = exp(-((double)lambda * t));
    return true;
}

// the pair (i, j) of staged pixels: false if not selected, else w, w e and r
__device__ __forceinline__ bool gt_pair(const float* __restrict__ sD, const float* __restrict__ sW, const float* __restrict__ sI, int i, int j,
                                        float lambda, int flags, float& w, double& we, double& r)
{
    const float di = sD[i], dj = sD[j];
    if (!(gt_valid(di) && gt_valid(dj))) return false;
    w = sW[i] * sW[j];
    if (!(w > 0.0f)) return false;
    double e;
    if (!gt_edge(sI, i, j, lambda, e)) return false;
    we = (double)w * e;
    r = gt_space(dj, flags) - gt_space(di, flags);
    return true;
}

// the triple (c - step, c, c + step)
__device__ __forceinline__ bool gt_triple(const float* __restrict__ sD, const float* __restrict__ sW, const float* __restrict__ sI, int c, int step,
                                          float lambda, int flags, float& w, double& we, double& r)
{
    const int i = c - step, j = c + step;
    const float di = sD[i], dc = sD[c], dj = sD[j];
    if (!(gt_valid(di) && gt_valid(dc) && gt_valid(dj))) return false;
    w = (sW[i] * sW[c]) * sW[j];
    if (!(w > 0.0f)) return false;
    double e;
    if (!gt_edge(sI, i, j, lambda, e)) return false;
    we = (double)w * e;
    r = (gt_space(di, flags) - 2.0 * gt_space(dc, flags)) + gt_space(dj, flags);
    return true;
}

// ---- the sums -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double gt_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the GT_SUMS sums of a block -> partial[k * nb + block], the waves added in order
__device__ __forceinline__ void gt_block_sums(double (&acc)[GT_SUMS], double* __restrict__ partial, int nb)
{
    __shared__ double lds[GT_WAVES][GT_SUMS];
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < GT_SUMS; ++k) acc[k] = gt_wave_sum(acc[k]);
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < GT_SUMS; ++k) lds[t >> 6][k] = acc[k];
    }
    __syncthreads();
    if (t < GT_SUMS) {
        double sum = lds[0][t];
#pragma unroll
        for (int w = 1; w < GT_WAVES; ++w) sum += lds[w][t];
        partial[(size_t)t * nb + blockIdx.x] = sum;
    }
}

// thread t, round k -> tile pixel (tx, ty), its picture pixel (x, y) and its staged index li
#define GT_PIXEL(k)                                                                              \
    const int tx = (int)threadIdx.x & 63, ty = ((int)threadIdx.x >> 6) + GT_WAVES * (k);        \
    const int x = tl.x0 + tx, y = tl.y0 + ty;                                                    \
    const int lx = tx + GT_PAD, ly = ty + GT_HALO, li = ly * GT_P + lx;                          \
    const bool inside = x < W && y < H

// ---- host side ----------------------------------------------------------------------------------------------------------------
static inline int gt_tiles(int H, int W) { return (int)((((long long)W + GT_W - 1) / GT_W) * (((long long)H + GT_H - 1) / GT_H)); }
static inline GtCam gt_cam(float fx, float fy, float cx, float cy) { GtCam K; K.fx = fx; K.fy = fy; K.cx = cx; K.cy = cy; return K; }
static inline bool gt_vec_ok(int W, const float* p) { return p && W % 4 == 0 && ((uintptr_t)p & 15u) == 0; }

// k_geometry.hip: the finishing block over nb per-tile sums [sum][tile] -> the eight terms (mean_cos: terms[3] = sum 3 / sum 2)
void gs_launch_geometry_finish(const double* partial, int nb, int mean_cos, float* terms, hipStream_t s);
