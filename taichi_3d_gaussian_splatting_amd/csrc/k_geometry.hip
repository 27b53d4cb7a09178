// k_geometry.hip -- geometry regularisers on the rendered depth (include/gs_geometry.h): the depth-derived normal, the cosine
// loss against a normal prior and the edge-aware smoothness, each loss with its gradient.
//
// Every pass is a stencil over the depth plane: a normal reads the four neighbours of its pixel, and the gradient at a pixel is
// a GATHER over the normals (or pairs, or triples) that read it -- the normals at its four neighbours, each formed from its own
// neighbours -- so a pixel's gradient reaches two pixels out.  One block of 256 threads owns a tile of GT_H x GT_W pixels and
// stages the depth tile with a halo of 2, and the planes the selection needs, in LDS once; every neighbourhood is then read
// from LDS, lanes along x (64 consecutive floats of one row per wave instruction: no bank conflict).  Nothing is scattered, so
// there is no atomic, and the order of every sum is fixed.
//
// The passes are bound by their float64 divisions and square roots, not by memory, so what several pixels of
// a block need is formed once per block and kept in LDS: a_x and b_y of the staged columns and rows, and in the normal loss's
// backward what the normal at every pixel of the tile grown by 1 owes its four neighbours -- the gather then reads four float64
// values.  Whoever forms a value forms it by the header's operations, so no bit depends on this.  (x = 1 / D is NOT staged that
// way: the smoothness passes spend their time in exp, and the LDS would cost them blocks in flight.)
//
// A staged row is GT_P = 72 floats: 4 of padding left (the halo in its last two), the 64 of the tile, 4 right, so that the
// tile's columns are 16-byte aligned in LDS as they are in a 16-byte aligned plane whose width is a multiple of 4; such a plane
// moves as one float4 per lane, any other pixel by pixel, into the same LDS image.  What lies outside the picture is staged as 0:
// an invalid depth, a zero weight.  Results leave through an LDS tile in the same two ways.
//
// Sums as in k_depth.hip, all float64: per thread over its pixels in order, a butterfly over the wave, the four waves in order
// -> one partial per tile and sum, laid out [sum][tile]; one finishing block, thread t adding the tiles t, t + 256, ...
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

// one block: the rows of per-tile sums in one loop, then the eight terms
__global__ __launch_bounds__(GT_FIN) void k_geometry_finish(const double* __restrict__ partial, int nb, int mean_cos, float* __restrict__ terms)
{
    __shared__ double lds[GT_FIN / 64][GT_SUMS];
    const int t = threadIdx.x;
    double a[GT_SUMS] = { 0.0, 0.0, 0.0, 0.0 };
    for (int i = t; i < nb; i += GT_FIN) {
#pragma unroll
        for (int k = 0; k < GT_SUMS; ++k) a[k] += partial[(size_t)k * nb + i];
    }
#pragma unroll
    for (int k = 0; k < GT_SUMS; ++k) a[k] = gt_wave_sum(a[k]);
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < GT_SUMS; ++k) lds[t >> 6][k] = a[k];
    }
    __syncthreads();
    if (t == 0) {
        double sums[GT_SUMS];
#pragma unroll
        for (int k = 0; k < GT_SUMS; ++k) {
            sums[k] = lds[0][k];
            for (int w = 1; w < GT_FIN / 64; ++w) sums[k] += lds[w][k];
        }
        const bool any = sums[1] > 0.0;
        terms[0] = any ? (float)(sums[0] / sums[1]) : 0.0f;
        terms[1] = any ? (float)sums[1] : 0.0f;
        terms[2] = any ? (float)sums[2] : 0.0f;
        terms[3] = any && mean_cos ? (float)(sums[3] / sums[2]) : 0.0f;
        terms[4] = terms[5] = terms[6] = terms[7] = 0.0f;
    }
}

// ---- the passes ---------------------------------------------------------------------------------------------------------------
// thread t, round k -> tile pixel (tx, ty), its picture pixel (x, y) and its staged index li
#define GT_PIXEL(k)                                                                              \
    const int tx = (int)threadIdx.x & 63, ty = ((int)threadIdx.x >> 6) + GT_WAVES * (k);        \
    const int x = tl.x0 + tx, y = tl.y0 + ty;                                                    \
    const int lx = tx + GT_PAD, ly = ty + GT_HALO, li = ly * GT_P + lx;                          \
    const bool inside = x < W && y < H

__global__ __launch_bounds__(GT_THREADS) void k_depth_normals(const float* __restrict__ D, int vec, int H, int W, GtCam K, float jump,
                                                             float* __restrict__ normals)
{
    __shared__ __align__(16) float sD[GT_R * GT_P];
    __shared__ __align__(16) float sO[3][GT_H * GT_W];
    __shared__ double sA[GT_P], sB[GT_R];
    const GtTile tl = gt_tile(W);
    gt_stage<0>(D, (vec & GT_VEC_D) != 0, H, W, tl, sD);
    gt_stage_camera(K, tl, sA, sB);
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        GT_PIXEL(k);
        GtNormal n;
        const bool ok = inside && gt_normal(sD, sA, sB, lx, ly, x, y, H, W, jump, n);
        (void)li;
#pragma unroll
        for (int j = 0; j < 3; ++j) sO[j][ty * GT_W + tx] = ok ? (float)(n.c[j] / n.len) : 0.0f;
    }
    __syncthreads();
    for (int j = 0; j < 3; ++j) gt_store(sO[j], normals + (size_t)j * H * W, (vec & GT_VEC_G) != 0, H, W, tl);
}

template <bool BACKWARD>
__global__ __launch_bounds__(GT_THREADS) void k_normal_loss(const float* __restrict__ D, const float* __restrict__ N, const float* __restrict__ wn,
                                                           const float* __restrict__ wp, int vec, int H, int W, GtCam K, float jump, int flags,
                                                           double* __restrict__ partial, int nb, const float* __restrict__ terms,
                                                           const float* __restrict__ upstream, float* __restrict__ G)
{
    __shared__ __align__(16) float sD[GT_R * GT_P];
    __shared__ __align__(16) float sW[GT_R * GT_P];
    __shared__ __align__(16) float sN[3 * GT_R * GT_P];
    __shared__ __align__(16) float sO[BACKWARD ? GT_H * GT_W : 4];
    __shared__ double sA[GT_P], sB[GT_R];
    // backward: what the normal at every pixel of the tile and of a halo of 1 owes its four neighbours, formed once, and whether it
    // is selected
    __shared__ double sOwes[BACKWARD ? 4 * GN_TERMS : 1];
    __shared__ uint8_t sSel[BACKWARD ? GN_TERMS : 1];
    const GtTile tl = gt_tile(W);
    gt_stage<0>(D, (vec & GT_VEC_D) != 0, H, W, tl, sD);
    for (int j = 0; j < 3; ++j) gt_stage<0>(N + (size_t)j * H * W, (vec & GT_VEC_A) != 0, H, W, tl, sN + j * (GT_R * GT_P));
    gt_stage<1>(wn, (vec & GT_VEC_WN) != 0, H, W, tl, sW);
    gt_stage_camera(K, tl, sA, sB);
    __syncthreads();                    // the second weight multiplies what the first left, whichever thread staged it
    gt_stage<2>(wp, (vec & GT_VEC_WP) != 0, H, W, tl, sW);
    __syncthreads();

    if constexpr (!BACKWARD) {
        double acc[GT_SUMS] = { 0.0, 0.0, 0.0, 0.0 };
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            GT_PIXEL(k);
            (void)li;
            GtNormalTerm o;
            if (inside && gt_normal_term(sD, sW, sN, sA, sB, lx, ly, x, y, H, W, jump, flags, o)) {
                acc[0] += (double)o.w * (1.0 - o.cos); acc[1] += (double)o.w; acc[2] += 1.0; acc[3] += o.cos;
            }
        }
        gt_block_sums(acc, partial, nb);
    } else {
        const float Sw = terms[1];
        const float u = upstream ? upstream[0] : 1.0f;
        const double s = Sw > 0.0f ? (double)u / (double)Sw : 0.0;
        // every normal the tile's pixels gather from, once: item = (hy, hx) of the tile grown by 1 on every side
#pragma unroll 1
        for (int item = threadIdx.x; item < GN_TERMS; item += GT_THREADS) {
            const int hy = item / GN_W, hx = item % GN_W;
            const int lx = hx + GT_PAD - 1, ly = hy + GT_HALO - 1;
            GtNormalTerm o;
            double owes[4] = { 0.0, 0.0, 0.0, 0.0 };
            const bool sel = Sw > 0.0f && gt_normal_term(sD, sW, sN, sA, sB, lx, ly, tl.x0 + hx - 1, tl.y0 + hy - 1, H, W, jump, flags, o);
            if (sel) gt_owes(o, sA, sB, lx, ly, s, owes);
            sSel[item] = sel ? 1 : 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) sOwes[j * GN_TERMS + item] = owes[j];
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

template <bool BACKWARD>
__global__ __launch_bounds__(GT_THREADS) void k_depth_smooth(const float* __restrict__ D, const float* __restrict__ I, const float* __restrict__ wp,
                                                            int vec, int H, int W, float lambda, int flags, double* __restrict__ partial, int nb,
                                                            const float* __restrict__ terms, const float* __restrict__ upstream,
                                                            float* __restrict__ G)
{
    __shared__ __align__(16) float sD[GT_R * GT_P];
    __shared__ __align__(16) float sW[GT_R * GT_P];
    __shared__ __align__(16) float sG[3 * GT_R * GT_P];
    __shared__ __align__(16) float sO[BACKWARD ? GT_H * GT_W : 4];
    const GtTile tl = gt_tile(W);
    gt_stage<0>(D, (vec & GT_VEC_D) != 0, H, W, tl, sD);
    gt_stage<1>(wp, (vec & GT_VEC_WP) != 0, H, W, tl, sW);
    if (I)
        for (int j = 0; j < 3; ++j) gt_stage<0>(I + (size_t)j * H * W, (vec & GT_VEC_A) != 0, H, W, tl, sG + j * (GT_R * GT_P));
    __syncthreads();
    const float* sI = I ? sG : nullptr;
    const bool second = (flags & GS_GEOM_SECOND_ORDER) != 0;
    float w; double we, r;

    if constexpr (!BACKWARD) {
        double acc[GT_SUMS] = { 0.0, 0.0, 0.0, 0.0 };
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            GT_PIXEL(k);
            if (!inside) continue;
#pragma unroll 1
            for (int dir = 0; dir < 2; ++dir) {
                const int step = dir == 0 ? 1 : GT_P;
                const bool sel = second ? gt_triple(sD, sW, sI, li, step, lambda, flags, w, we, r) : gt_pair(sD, sW, sI, li, li + step, lambda, flags, w, we, r);
                if (sel) { acc[0] += we * fabs(r); acc[1] += (double)w; acc[2] += 1.0; }
            }
        }
        gt_block_sums(acc, partial, nb);
    } else {
        const float Sw = terms[1];
        const float u = upstream ? upstream[0] : 1.0f;
        const double s = Sw > 0.0f ? (double)u / (double)Sw : 0.0;
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            GT_PIXEL(k);
            double acc = 0.0;
            bool any = false;
            if (inside && Sw > 0.0f) {
#pragma unroll 1
                for (int dir = 0; dir < 2; ++dir) {
                    const int step = dir == 0 ? 1 : GT_P;
                    if (second) {
                        if (gt_triple(sD, sW, sI, li - step, step, lambda, flags, w, we, r)) { acc += we * gt_sign(r); any = true; }
                        if (gt_triple(sD, sW, sI, li, step, lambda, flags, w, we, r)) { acc += -(2.0 * (we * gt_sign(r))); any = true; }
                        if (gt_triple(sD, sW, sI, li + step, step, lambda, flags, w, we, r)) { acc += we * gt_sign(r); any = true; }
                    } else {
                        if (gt_pair(sD, sW, sI, li - step, li, lambda, flags, w, we, r)) { acc += we * gt_sign(r); any = true; }
                        if (gt_pair(sD, sW, sI, li, li + step, lambda, flags, w, we, r)) { acc += -(we * gt_sign(r)); any = true; }
                    }
                }
            }
            float g = 0.0f;
            if (any) {
                double g64 = acc * s;
                if (flags & GS_GEOM_INVERSE) { const double xx = gt_space(sD[li], flags); g64 = g64 * -(xx * xx); }
                g = (float)g64;
            }
            sO[ty * GT_W + tx] = g;
        }
        __syncthreads();
        gt_store(sO, G, (vec & GT_VEC_G) != 0, H, W, tl);
    }
}

// ---- the launchers --------------------------------------------------------------------------------------------------------------
static int gt_tiles(int H, int W) { return (int)((((long long)W + GT_W - 1) / GT_W) * (((long long)H + GT_H - 1) / GT_H)); }

static int gt_vec(int W, const float* D, const float* A, const float* wn, const float* wp, const float* G)
{
    auto ok = [W](const float* p) { return p && W % 4 == 0 && ((uintptr_t)p & 15u) == 0; };
    return (ok(D) ? GT_VEC_D : 0) | (ok(A) ? GT_VEC_A : 0) | (ok(wn) ? GT_VEC_WN : 0) | (ok(wp) ? GT_VEC_WP : 0) | (ok(G) ? GT_VEC_G : 0);
}

static GtCam gt_cam(float fx, float fy, float cx, float cy) { GtCam K; K.fx = fx; K.fy = fy; K.cx = cx; K.cy = cy; return K; }

size_t gs_geometry_ws_size(int H, int W) { return (size_t)gt_tiles(H, W) * GT_SUMS * sizeof(double); }

void gs_launch_depth_normals(const float* D, int H, int W, float fx, float fy, float cx, float cy, float jump, float* normals, hipStream_t s)
{
    k_depth_normals<<<gt_tiles(H, W), GT_THREADS, 0, s>>>(D, gt_vec(W, D, nullptr, nullptr, nullptr, normals), H, W, gt_cam(fx, fy, cx, cy), jump, normals);
}

void gs_launch_normal_loss_forward(const float* D, const float* N, const float* wn, const float* wp, int H, int W, float fx, float fy, float cx,
                                   float cy, float jump, int flags, float* terms, void* ws, hipStream_t s)
{
    const int nb = gt_tiles(H, W);
    double* partial = static_cast<double*>(ws);
    k_normal_loss<false><<<nb, GT_THREADS, 0, s>>>(D, N, wn, wp, gt_vec(W, D, N, wn, wp, nullptr), H, W, gt_cam(fx, fy, cx, cy), jump, flags, partial, nb,
                                                   nullptr, nullptr, nullptr);
    k_geometry_finish<<<1, GT_FIN, 0, s>>>(partial, nb, 1, terms);
}

void gs_launch_normal_loss_backward(const float* D, const float* N, const float* wn, const float* wp, int H, int W, float fx, float fy, float cx,
                                    float cy, float jump, int flags, const float* terms, const float* upstream, float* G, hipStream_t s)
{
    k_normal_loss<true><<<gt_tiles(H, W), GT_THREADS, 0, s>>>(D, N, wn, wp, gt_vec(W, D, N, wn, wp, G), H, W, gt_cam(fx, fy, cx, cy), jump, flags,
                                                              nullptr, 0, terms, upstream, G);
}

void gs_launch_depth_smooth_forward(const float* D, const float* I, const float* wp, int H, int W, float lambda, int flags, float* terms, void* ws,
                                    hipStream_t s)
{
    const int nb = gt_tiles(H, W);
    double* partial = static_cast<double*>(ws);
    k_depth_smooth<false><<<nb, GT_THREADS, 0, s>>>(D, I, wp, gt_vec(W, D, I, nullptr, wp, nullptr), H, W, lambda, flags, partial, nb, nullptr, nullptr,
                                                    nullptr);
    k_geometry_finish<<<1, GT_FIN, 0, s>>>(partial, nb, 0, terms);
}

void gs_launch_depth_smooth_backward(const float* D, const float* I, const float* wp, int H, int W, float lambda, int flags, const float* terms,
                                     const float* upstream, float* G, hipStream_t s)
{
    k_depth_smooth<true><<<gt_tiles(H, W), GT_THREADS, 0, s>>>(D, I, wp, gt_vec(W, D, I, nullptr, wp, G), H, W, lambda, flags, nullptr, 0, terms,
                                                               upstream, G);
}
