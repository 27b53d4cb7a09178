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
//
// The staging, the normal, the smoothness terms and the sums are in gs_geometry_tile.h, which k_normals.hip builds on too.
#include "gs_geometry_tile.h"

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
static int gt_vec(int W, const float* D, const float* A, const float* wn, const float* wp, const float* G)
{
    auto ok = [W](const float* p) { return gt_vec_ok(W, p); };
    return (ok(D) ? GT_VEC_D : 0) | (ok(A) ? GT_VEC_A : 0) | (ok(wn) ? GT_VEC_WN : 0) | (ok(wp) ? GT_VEC_WP : 0) | (ok(G) ? GT_VEC_G : 0);
}

size_t gs_geometry_ws_size(int H, int W) { return (size_t)gt_tiles(H, W) * GT_SUMS * sizeof(double); }

void gs_launch_geometry_finish(const double* partial, int nb, int mean_cos, float* terms, hipStream_t s)
{
    k_geometry_finish<<<1, GT_FIN, 0, s>>>(partial, nb, mean_cos, terms);
}

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
