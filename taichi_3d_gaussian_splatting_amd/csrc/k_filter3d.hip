// k_filter3d.hip -- the 3D smoothing filter (include/gs_filter3d.h): the largest sampling rate of every row over a table of
// views, the transform of a feature row under the filter, and its gradient.
//
//   k_filter3d_rate      a row per lane, the views in a loop: a view's 16 floats are read at a wave-uniform address, so they
//                        arrive by scalar loads and sit in scalar registers as operands of the vector arithmetic (k_mixture.hip).
//                        About forty f32 operations and three divisions per pair, nearly no memory traffic.  A valid row no
//                        view sees is stored as 0 (no rate is 0); the block's smallest seen rate goes to one word by an
//                        integer atomic minimum on the bit pattern.
//   k_filter3d_fill      the rows stored as 0 take that word.
//   k_filter3d_apply     a block owns 256 rows, 57 KB, and moves them through LDS: every thread loads 14 of the block's 3584
//                        float4 as one flat, coalesced run, then transforms columns 0..7 of its own row in LDS in float64,
//                        then stores 14 float4 of the flat run.  Global memory sees one coalesced read and one coalesced write
//                        (and the rare quaternion write-back).
//   k_filter3d_backward  the same walk over the gradient rows; columns 4..7 are the only ones computed.  In place, only those
//                        float4 are read and written, without LDS.
//
// Nothing here uses a float atomic, and no result depends on the grid.
#include "gs_common.h"
#include "../../include/gs_filter3d.h"

#define GS_F3D_THREADS GS_FILTER3D_ROWS_PER_BLOCK
#define GS_F3D_ROW4 (GS_FILTER3D_FEATURES / 4)              // float4 of a row: 14
static_assert(GS_F3D_THREADS == 256, "a block is four waves");
static_assert(GS_FILTER3D_FEATURES == GS_NFEAT, "the rasteriser's feature row");

#define GS_F3D_INF_BITS 0x7f800000u

// ---- the sampling rate ------------------------------------------------------------------------------------------------------
struct GsFilter3dWindow { float lo_x, hi_x, lo_y, hi_y, near; };

__global__ void __launch_bounds__(GS_F3D_THREADS) k_filter3d_rate(const float* __restrict__ pc, const int8_t* __restrict__ mask, int64_t n,
                                                                  const float* __restrict__ views, int n_views, GsFilter3dWindow win,
                                                                  float* __restrict__ rate, unsigned int* __restrict__ min_bits)
{
    __shared__ unsigned int wave_min[GS_F3D_THREADS / 64];
    const int64_t i = (int64_t)blockIdx.x * GS_F3D_THREADS + threadIdx.x;
    const bool inside = i < n;
    const int64_t row = inside ? i : n - 1;                    // a lane past the end computes the last row and stores nothing
    const bool valid = inside && mask[row] == 0;
    const float x = pc[3 * row], y = pc[3 * row + 1], z = pc[3 * row + 2];
    float best = 0.0f;                                          // no view yet: every c that counts is > 0
    for (int v = 0; v < n_views; ++v) {
        const float* __restrict__ w = views + (size_t)GS_FILTER3D_VIEW_FLOATS * v;      // wave-uniform
        const float p0 = ((w[0] * x + w[1] * y) + w[2] * z) + w[9];
        const float p1 = ((w[3] * x + w[4] * y) + w[5] * z) + w[10];
        const float p2 = ((w[6] * x + w[7] * y) + w[8] * z) + w[11];
        const float fx = w[12], fy = w[13], cx = w[14], cy = w[15];
        const float u = (fx * p0) / p2 + cx, vv = (fy * p1) / p2 + cy;
        const float fm = fx > fy ? fx : fy;
        const float c = fm / p2;
        const bool sees = p2 > win.near && win.lo_x <= u && u <= win.hi_x && win.lo_y <= vv && vv <= win.hi_y && c > 0.0f;
        best = sees && c > best ? c : best;
    }
    const bool seen = valid && best > 0.0f;
    if (inside) rate[i] = valid ? best : __uint_as_float(GS_F3D_INF_BITS);
    // the smallest seen rate of the block: positive floats order as their bits do
    unsigned int m = seen ? __float_as_uint(best) : GS_F3D_INF_BITS;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned int other = (unsigned int)__shfl_xor((int)m, o, 64);
        m = other < m ? other : m;
    }
    if ((threadIdx.x & 63) == 0) wave_min[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < GS_F3D_THREADS / 64; ++k) m = wave_min[k] < m ? wave_min[k] : m;
        if (m != GS_F3D_INF_BITS) atomicMin(min_bits, m);
    }
}

__global__ void __launch_bounds__(GS_F3D_THREADS) k_filter3d_fill(float* __restrict__ rate, int64_t n, const unsigned int* __restrict__ min_bits)
{
    const int64_t i = (int64_t)blockIdx.x * GS_F3D_THREADS + threadIdx.x;
    if (i < n && rate[i] == 0.0f) rate[i] = __uint_as_float(min_bits[0]);
}

// ---- the transform -------------------------------------------------------------------------------------------------------
// r_j = s_j / (s_j + v) and t_j = s_j + v of a row's three log-scales, and c = sqrt((r_0 r_1) r_2), in float64
struct GsFilter3dRow { double t[3], r[3], c; };

__device__ __forceinline__ GsFilter3dRow gs_filter3d_row(float ls0, float ls1, float ls2, float f)
{
    GsFilter3dRow R;
    const double v = (double)f * (double)f;
    const float ls[3] = { ls0, ls1, ls2 };
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double e = exp((double)ls[j]);
        const double s = e * e;
        R.t[j] = s + v;
        R.r[j] = s / R.t[j];
    }
    R.c = sqrt((R.r[0] * R.r[1]) * R.r[2]);
    return R;
}

// the block's rows as one flat run of float4 between global memory and LDS: float4 j of the run is thread j % 256's in round j / 256
__device__ __forceinline__ void gs_filter3d_load_tile(const float4* in, float4* tile, int64_t row0, int rows)
{
#pragma unroll
    for (int k = 0; k < GS_F3D_ROW4; ++k) {
        const int j = k * GS_F3D_THREADS + (int)threadIdx.x;
        if (j < rows * GS_F3D_ROW4) tile[j] = in[(size_t)row0 * GS_F3D_ROW4 + j];
    }
}

__device__ __forceinline__ void gs_filter3d_store_tile(const float4* tile, float4* out, int64_t row0, int rows)
{
#pragma unroll
    for (int k = 0; k < GS_F3D_ROW4; ++k) {
        const int j = k * GS_F3D_THREADS + (int)threadIdx.x;
        if (j < rows * GS_F3D_ROW4) out[(size_t)row0 * GS_F3D_ROW4 + j] = tile[j];
    }
}

__global__ void __launch_bounds__(GS_F3D_THREADS) k_filter3d_apply(float4* __restrict__ feat, const float* __restrict__ rate, int64_t n, float k,
                                                                   float4* __restrict__ out)
{
    __shared__ float4 tile[GS_F3D_THREADS * GS_F3D_ROW4];
    const int64_t row0 = (int64_t)blockIdx.x * GS_F3D_THREADS;
    const int rows = (int)(n - row0 < GS_F3D_THREADS ? n - row0 : GS_F3D_THREADS);
    gs_filter3d_load_tile(feat, tile, row0, rows);
    __syncthreads();
    if ((int)threadIdx.x < rows) {
        const int at = (int)threadIdx.x * GS_F3D_ROW4;
        float4 q = tile[at];
        float4 g = tile[at + 1];                              // ls_0, ls_1, ls_2, a
        const float f = k / rate[row0 + threadIdx.x];
        if (f > 0.0f) {
            // the rasteriser's normalisation (k_project.hip), written back only when the division changed a bit
            const float nrm = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
            const float q0 = q.x / nrm, q1 = q.y / nrm, q2 = q.z / nrm, q3 = q.w / nrm;
            const bool changed = __float_as_int(q0) != __float_as_int(q.x) || __float_as_int(q1) != __float_as_int(q.y) ||
                                 __float_as_int(q2) != __float_as_int(q.z) || __float_as_int(q3) != __float_as_int(q.w);
            q = make_float4(q0, q1, q2, q3);
            if (changed) feat[(size_t)(row0 + threadIdx.x) * GS_F3D_ROW4] = q;
            const GsFilter3dRow R = gs_filter3d_row(g.x, g.y, g.z, f);
            const double logit = log(R.c) - log((1.0 - R.c) + exp(-(double)g.w));
            g = make_float4((float)(0.5 * log(R.t[0])), (float)(0.5 * log(R.t[1])), (float)(0.5 * log(R.t[2])), (float)logit);
            tile[at] = q;
            tile[at + 1] = g;
        }
    }
    __syncthreads();
    gs_filter3d_store_tile(tile, out, row0, rows);
}

// g'_ls, g'_a of a row and its ls, a -> g_ls, g_a (the row is not an identity row)
__device__ __forceinline__ float4 gs_filter3d_row_backward(float4 gp, float4 s, float f)
{
    const GsFilter3dRow R = gs_filter3d_row(s.x, s.y, s.z, f);
    const double E = exp(-(double)s.w), D = (1.0 - R.c) + E;
    const double through = (double)gp.w * (1.0 + R.c / D);
    const float up[3] = { gp.x, gp.y, gp.z };
    float down[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double A = up[j] == 0.0f ? 0.0 : (double)up[j] * R.r[j];
        const double B = gp.w == 0.0f ? 0.0 : through * (1.0 - R.r[j]);
        down[j] = (float)(A + B);
    }
    const float ga = gp.w == 0.0f ? 0.0f : (float)(((double)gp.w * E) / D);
    return make_float4(down[0], down[1], down[2], ga);
}

__global__ void __launch_bounds__(GS_F3D_THREADS) k_filter3d_backward(const float4* __restrict__ grad_out, const float4* __restrict__ feat,
                                                                      const float* __restrict__ rate, int64_t n, float k,
                                                                      float4* __restrict__ grad_in)
{
    __shared__ float4 tile[GS_F3D_THREADS * GS_F3D_ROW4];
    const int64_t row0 = (int64_t)blockIdx.x * GS_F3D_THREADS;
    const int rows = (int)(n - row0 < GS_F3D_THREADS ? n - row0 : GS_F3D_THREADS);
    gs_filter3d_load_tile(grad_out, tile, row0, rows);
    __syncthreads();
    if ((int)threadIdx.x < rows) {
        const float f = k / rate[row0 + threadIdx.x];
        if (f > 0.0f) {
            const int at = (int)threadIdx.x * GS_F3D_ROW4 + 1;
            tile[at] = gs_filter3d_row_backward(tile[at], feat[(size_t)(row0 + threadIdx.x) * GS_F3D_ROW4 + 1], f);
        }
    }
    __syncthreads();
    gs_filter3d_store_tile(tile, grad_in, row0, rows);
}

// grad is grad_out and grad_in at once: the pass-through columns stay where they are
__global__ void __launch_bounds__(GS_F3D_THREADS) k_filter3d_backward_in_place(float4* grad, const float4* __restrict__ feat,
                                                                               const float* __restrict__ rate, int64_t n, float k)
{
    const int64_t i = (int64_t)blockIdx.x * GS_F3D_THREADS + threadIdx.x;
    if (i >= n) return;
    const float f = k / rate[i];
    if (!(f > 0.0f)) return;
    const size_t at = (size_t)i * GS_F3D_ROW4 + 1;
    grad[at] = gs_filter3d_row_backward(grad[at], feat[at], f);
}

// ---- launch ------------------------------------------------------------------------------------------------------------------
size_t gs_filter3d_ws_size() { return 16; }

static unsigned gs_filter3d_blocks(int64_t n) { return (unsigned)((n + GS_F3D_THREADS - 1) / GS_F3D_THREADS); }

// n > 0.  ws: gs_filter3d_ws_size() bytes of the context's (the smallest seen rate's bits)
void gs_launch_filter3d_rate(const float* point_cloud, const int8_t* mask, int64_t n, const float* views, int n_views, int W, int H, float near,
                             float margin, float* rate, void* ws, hipStream_t s)
{
    unsigned int* min_bits = reinterpret_cast<unsigned int*>(ws);
    (void)hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(min_bits), (int)GS_F3D_INF_BITS, 1, s);
    GsFilter3dWindow win;
    win.lo_x = (-margin) * (float)W; win.hi_x = (1.0f + margin) * (float)W;
    win.lo_y = (-margin) * (float)H; win.hi_y = (1.0f + margin) * (float)H;
    win.near = near;
    k_filter3d_rate<<<gs_filter3d_blocks(n), GS_F3D_THREADS, 0, s>>>(point_cloud, mask, n, views, n_views, win, rate, min_bits);
    k_filter3d_fill<<<gs_filter3d_blocks(n), GS_F3D_THREADS, 0, s>>>(rate, n, min_bits);
}

void gs_launch_filter3d_apply(float* features, const float* rate, int64_t n, float k, float* features_out, hipStream_t s)
{
    k_filter3d_apply<<<gs_filter3d_blocks(n), GS_F3D_THREADS, 0, s>>>(reinterpret_cast<float4*>(features), rate, n, k,
                                                                      reinterpret_cast<float4*>(features_out));
}

void gs_launch_filter3d_backward(const float* grad_out, const float* features, const float* rate, int64_t n, float k, float* grad_in,
                                 hipStream_t s)
{
    if (grad_in == grad_out)
        k_filter3d_backward_in_place<<<gs_filter3d_blocks(n), GS_F3D_THREADS, 0, s>>>(reinterpret_cast<float4*>(grad_in),
                                                                                      reinterpret_cast<const float4*>(features), rate, n, k);
    else
        k_filter3d_backward<<<gs_filter3d_blocks(n), GS_F3D_THREADS, 0, s>>>(reinterpret_cast<const float4*>(grad_out),
                                                                             reinterpret_cast<const float4*>(features), rate, n, k,
                                                                             reinterpret_cast<float4*>(grad_in));
}
