// k_depth.hip -- depth supervision (include/gs_depth.h): the depth target of one view with its validity weight, and the fused
// masked depth loss with its gradient.
//
// k_depth_resample is k_image_resample (k_targets.hip) for a map with holes: the same tile, chunks, staging and tables, two
// planes through the two passes -- the filtered depth of the valid samples and the filter weight they cover -- and a division
// at the end.  An invalid sample is never read into a sum.
//
// The loss passes are memory bound (forward: three or four planes read per pass; backward: the same and one written), so each
// moves its planes once and the sums ride in the same pass.  A block of 256 threads owns DP_PIXELS consecutive pixels, thread t
// of block b the four pixels 4 (256 b + t) ..., whatever the alignment of the planes: a 16-byte aligned plane is read as one
// float4 per thread, any other (and the tail of a plane whose pixel count is no multiple of four) pixel by pixel, so the order
// of every sum -- and with it every bit of the result -- does not depend on the path.
//
// Sums, all float64: per thread over its four pixels in order, a butterfly over the wave, the four waves in order through LDS
// -> one partial per block and sum, laid out [sum][block]; a finishing block per sum, thread t adding the blocks t, t + 256,
// ..., then the same butterfly and wave order.  No atomics.
#include "gs_common.h"
#include "../../include/gs_depth.h"

#include <cfloat>

// ---- the depth target ----------------------------------------------------------------------------------------------------------
#define DR_TILE_H GS_RESAMPLE_TILE_H
#define DR_TILE_W GS_RESAMPLE_TILE_W
#define DR_THREADS 256
#define DR_CHUNK_ROWS 16
// bytes of one staged row: GS_RS_MAX_SPAN samples of 2 bytes behind an offset of up to 15, in whole 16-byte slots
#define DR_RAW_PITCH ((GS_RS_MAX_SPAN * 2 + 15 + 15) / 16 * 16)
static_assert(DR_TILE_W % 4 == 0 && DR_TILE_H * (DR_TILE_W / 4) == DR_THREADS, "one thread per tile row and four columns");
static_assert(DR_THREADS % DR_TILE_W == 0 && DR_CHUNK_ROWS % (DR_THREADS / DR_TILE_W) == 0, "the horizontal pass covers a chunk in whole rounds");

template <bool U16>
__global__ __launch_bounds__(DR_THREADS) void k_depth_resample(const uint8_t* __restrict__ src, int H_in, int W_in, int64_t pitch, float depth_scale,
                                                              GsResampleAxis ax, GsResampleAxis ay, int h_out, int w_out, float min_coverage,
                                                              float* __restrict__ dst, int vec_store)
{
    __shared__ __align__(16) float hbuf[DR_CHUNK_ROWS][2][DR_TILE_W];
    __shared__ __align__(16) uint8_t raw[U16 ? DR_CHUNK_ROWS * DR_RAW_PITCH : 16];
    __shared__ float wx[DR_TILE_W * GS_RS_MAX_TAPS], wy[DR_TILE_H * GS_RS_MAX_TAPS];
    __shared__ int sx[DR_TILE_W], cx[DR_TILE_W], sy[DR_TILE_H], cy[DR_TILE_H];

    const int t = threadIdx.x;
    const int tx0 = blockIdx.x * DR_TILE_W, ty0 = blockIdx.y * DR_TILE_H;
    // the tile's windows and weights; columns / rows past the crop get an empty window
    if (t < DR_TILE_W) {
        const int x = tx0 + t;
        const int n = x < w_out ? min(ax.count[x], GS_RS_MAX_TAPS) : 0;
        sx[t] = x < w_out ? ax.start[x] : 0; cx[t] = n;
        for (int k = 0; k < n; ++k) wx[t * GS_RS_MAX_TAPS + k] = ax.weight[(size_t)x * ax.taps + k];
    } else if (t < DR_TILE_W + DR_TILE_H) {
        const int i = t - DR_TILE_W, y = ty0 + i;
        const int n = y < h_out ? min(ay.count[y], GS_RS_MAX_TAPS) : 0;
        sy[i] = y < h_out ? ay.start[y] : 0; cy[i] = n;
        for (int k = 0; k < n; ++k) wy[i * GS_RS_MAX_TAPS + k] = ay.weight[(size_t)y * ay.taps + k];
    }
    __syncthreads();
    const int x_last = min(DR_TILE_W, w_out - tx0) - 1, y_last = min(DR_TILE_H, h_out - ty0) - 1;
    const int px0 = sx[0], px1 = min(sx[x_last] + cx[x_last], W_in);      // input columns [px0, px1) and
    const int R0 = sy[0], R1 = min(sy[y_last] + cy[y_last], H_in);        // rows [R0, R1) the tile reads
    const int span_bytes = (px1 - px0) * 2;
    const int slots = (span_bytes + 15 + 15) / 16;                        // 16-byte slots of a row at the worst offset
    const uintptr_t buf_begin = (uintptr_t)src, buf_end = buf_begin + (uintptr_t)(H_in - 1) * (uintptr_t)pitch + (uintptr_t)W_in * 2;

    const int vy = t / (DR_TILE_W / 4), vg = t % (DR_TILE_W / 4);       // vertical pass: tile row, group of four columns
    const int hx = t % DR_TILE_W, hr0 = t / DR_TILE_W;                     // horizontal pass: tile column, first chunk row
    float4 num = make_float4(0.0f, 0.0f, 0.0f, 0.0f), den = make_float4(0.0f, 0.0f, 0.0f, 0.0f);

    for (int r0 = R0; r0 < R1; r0 += DR_CHUNK_ROWS) {
        const int n_rows = min(DR_CHUNK_ROWS, R1 - r0);
        if constexpr (U16) {
            // the bytes the tile's columns read, as they lie, by whole aligned 16-byte slots; a slot that is not wholly inside
            // the buffer (its very first and last bytes) byte by byte
            for (int item = t; item < n_rows * slots; item += DR_THREADS) {
                const int rr = item / slots, s = item % slots;
                const uintptr_t a = buf_begin + (uintptr_t)(r0 + rr) * (uintptr_t)pitch + (uintptr_t)px0 * 2, e = a + span_bytes;
                const uintptr_t sa = (a & ~(uintptr_t)15) + 16u * (uintptr_t)s;
                if (sa >= e || 16 * s + 16 > DR_RAW_PITCH) continue;
                uint8_t* out = &raw[rr * DR_RAW_PITCH + 16 * s];
                if (sa >= buf_begin && sa + 16 <= buf_end) {
                    *reinterpret_cast<uint4*>(out) = *reinterpret_cast<const uint4*>(sa);
                } else {
                    for (int b = 0; b < 16; ++b)
                        if (sa + b >= a && sa + b < e) out[b] = *reinterpret_cast<const uint8_t*>(sa + b);
                }
            }
            __syncthreads();
        }
        // horizontal pass of the chunk's rows: the valid samples only
        for (int rr = hr0; rr < DR_CHUNK_ROWS; rr += DR_THREADS / DR_TILE_W) {
            float hn = 0.0f, hd = 0.0f;
            if (rr < n_rows) {
                const int n = cx[hx];
                const float* w = &wx[hx * GS_RS_MAX_TAPS];
                if constexpr (U16) {
                    const uintptr_t a = buf_begin + (uintptr_t)(r0 + rr) * (uintptr_t)pitch + (uintptr_t)px0 * 2;
                    const uint8_t* p = &raw[rr * DR_RAW_PITCH + (int)(a & 15) + (sx[hx] - px0) * 2];
                    for (int k = 0; k < n; ++k, p += 2) {
                        const unsigned v = (unsigned)p[0] | ((unsigned)p[1] << 8);       // (a row may start at an odd address)
                        if (v != 0u) { hn = fmaf(w[k], (float)v * depth_scale, hn); hd = hd + w[k]; }
                    }
                } else {
                    const float* p = reinterpret_cast<const float*>(src) + (size_t)(r0 + rr) * W_in + sx[hx];
                    for (int k = 0; k < n; ++k) {
                        const float z = p[k];
                        if (z > 0.0f && z <= FLT_MAX) { hn = fmaf(w[k], z, hn); hd = hd + w[k]; }
                    }
                }
            }
            hbuf[rr][0][hx] = hn; hbuf[rr][1][hx] = hd;
        }
        __syncthreads();
        // vertical pass: the taps of this thread's output row that lie in the chunk
        {
            const int first = sy[vy], n = cy[vy];
            const int k0 = max(0, r0 - first), k1 = min(n, r0 + n_rows - first);
            for (int k = k0; k < k1; ++k) {
                const float w = wy[vy * GS_RS_MAX_TAPS + k];
                const int rr = first + k - r0;
                const float4 a = *reinterpret_cast<const float4*>(&hbuf[rr][0][4 * vg]);
                const float4 b = *reinterpret_cast<const float4*>(&hbuf[rr][1][4 * vg]);
                num.x = fmaf(w, a.x, num.x); num.y = fmaf(w, a.y, num.y); num.z = fmaf(w, a.z, num.z); num.w = fmaf(w, a.w, num.w);
                den.x = fmaf(w, b.x, den.x); den.y = fmaf(w, b.y, den.y); den.z = fmaf(w, b.z, den.z); den.w = fmaf(w, b.w, den.w);
            }
        }
        __syncthreads();        // the next chunk overwrites both buffers
    }

    const int oy = ty0 + vy, ox = tx0 + 4 * vg;
    if (oy >= h_out || ox >= w_out) return;
    const float n4[4] = { num.x, num.y, num.z, num.w }, d4[4] = { den.x, den.y, den.z, den.w };
    float z4[4], w4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool ok = d4[j] > 0.0f && d4[j] >= min_coverage;
        w4[j] = ok ? d4[j] : 0.0f;
        z4[j] = ok ? n4[j] / d4[j] : 0.0f;
    }
    float* dz = dst + (size_t)oy * w_out + ox;
    float* dw = dz + (size_t)h_out * w_out;
    if (vec_store && ox + 3 < w_out) {
        *reinterpret_cast<float4*>(dz) = make_float4(z4[0], z4[1], z4[2], z4[3]);
        *reinterpret_cast<float4*>(dw) = make_float4(w4[0], w4[1], w4[2], w4[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (ox + j < w_out) { dz[j] = z4[j]; dw[j] = w4[j]; }
    }
}

void gs_launch_depth_resample(const void* src, int src_format, int H_in, int W_in, int64_t pitch_bytes, float depth_scale, GsResampleAxis ax,
                              GsResampleAxis ay, int h_out, int w_out, float min_coverage, float* dst, hipStream_t s)
{
    const dim3 grid((w_out + DR_TILE_W - 1) / DR_TILE_W, (h_out + DR_TILE_H - 1) / DR_TILE_H);
    // both planes take 16-byte stores: the second begins h_out * w_out floats behind the first
    const int vec_store = (w_out % 4 == 0 && ((uintptr_t)dst & 15) == 0) ? 1 : 0;
    const uint8_t* p = reinterpret_cast<const uint8_t*>(src);
    if (src_format == GS_DEPTH_U16)
        hipLaunchKernelGGL((k_depth_resample<true>), grid, dim3(DR_THREADS), 0, s, p, H_in, W_in, pitch_bytes, depth_scale, ax, ay, h_out, w_out,
                           min_coverage, dst, vec_store);
    else
        hipLaunchKernelGGL((k_depth_resample<false>), grid, dim3(DR_THREADS), 0, s, p, H_in, W_in, pitch_bytes, depth_scale, ax, ay, h_out, w_out,
                           min_coverage, dst, vec_store);
}

// ---- the loss ------------------------------------------------------------------------------------------------------------------
#define DP_THREADS 256
#define DP_WAVES (DP_THREADS / 64)
#define DP_PIXELS GS_DEPTH_PIXELS_PER_BLOCK
#define DP_FIN GS_DEPTH_FINISH_THREADS
#define DP_RESIDUAL_SUMS 3        // sum w rho, sum w, the number of selected pixels
static_assert(DP_PIXELS == 4 * DP_THREADS, "four pixels per thread");
static_assert(DP_FIN % 64 == 0 && DP_FIN <= 1024, "whole waves in the finishing block");

// bits of `vec`: the plane is 16-byte aligned
#define DP_VEC_D 1
#define DP_VEC_Z 2
#define DP_VEC_WT 4
#define DP_VEC_WP 8
#define DP_VEC_G 16

// the thread's four pixels of a contiguous plane: v[k] as stored; 0 for a slot past the image
__device__ __forceinline__ void dp_load(const float* __restrict__ q, bool vec, int n, int p0, float v[4])
{
    float4 r;
    if (vec && p0 + 3 < n) {
        r = *reinterpret_cast<const float4*>(q + p0);
    } else {
        const int p1 = p0 + 1, p2 = p0 + 2, p3 = p0 + 3;
        r = make_float4(p0 < n ? q[p0] : 0.0f, p1 < n ? q[p1] : 0.0f, p2 < n ? q[p2] : 0.0f, p3 < n ? q[p3] : 0.0f);
    }
    v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
}

// what a thread knows of its four pixels: the weight (0: not selected) and x, y of the selected ones.  From here on everything is
// float64: the passes are bound by memory, and the result is then the header's formula rounded once.
struct DpPixels { float w[4]; double x[4], y[4]; };

__device__ __forceinline__ DpPixels dp_pixels(const float* __restrict__ D, const float* __restrict__ Z, const float* __restrict__ wt,
                                              const float* __restrict__ wp, int vec, int flags, int n, int p0)
{
    float d[4], z[4], a[4], b[4];
    dp_load(D, (vec & DP_VEC_D) != 0, n, p0, d);
    dp_load(Z, (vec & DP_VEC_Z) != 0, n, p0, z);
    dp_load(wt, (vec & DP_VEC_WT) != 0, n, p0, a);
    if (wp) {
        dp_load(wp, (vec & DP_VEC_WP) != 0, n, p0, b);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) b[k] = 1.0f;
    }
    DpPixels r;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float ak = a[k] > 0.0f ? a[k] : 0.0f, bk = b[k] > 0.0f ? b[k] : 0.0f;       // a negative or NaN weight is 0
        const float w = ak * bk;
        const bool sel = w > 0.0f && z[k] > 0.0f && z[k] <= FLT_MAX && d[k] > 0.0f && d[k] <= FLT_MAX && p0 + k < n;
        r.w[k] = sel ? w : 0.0f;
        r.x[k] = sel ? ((flags & GS_DEPTH_INVERT_PREDICTED) ? 1.0 / (double)d[k] : (double)d[k]) : 0.0;
        r.y[k] = sel ? ((flags & GS_DEPTH_INVERT_TARGET) ? 1.0 / (double)z[k] : (double)z[k]) : 0.0;
    }
    return r;
}

__device__ __forceinline__ double dp_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// NS sums of a block of DP_THREADS threads -> partial[k * nb + block], the waves added in order
template <int NS>
__device__ __forceinline__ void dp_block_sums(double (&acc)[NS], double* __restrict__ partial, int nb)
{
    __shared__ double lds[DP_WAVES][NS];
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = dp_wave_sum(acc[k]);
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) lds[t >> 6][k] = acc[k];
    }
    __syncthreads();
    if (t < NS) {
        double sum = lds[0][t];
#pragma unroll
        for (int w = 1; w < DP_WAVES; ++w) sum += lds[w][t];
        partial[(size_t)t * nb + blockIdx.x] = sum;
    }
}

// the sum of one row of per-block sums by a finishing block; every thread returns with it
__device__ __forceinline__ double dp_finish_row(const double* __restrict__ row, int nb, double* lds)
{
    const int t = threadIdx.x;
    double a = 0.0;
    for (int i = t; i < nb; i += DP_FIN) a += row[i];
    a = dp_wave_sum(a);
    __syncthreads();                    // the block may still read lds of the row before
    if ((t & 63) == 0) lds[t >> 6] = a;
    __syncthreads();
    double sum = lds[0];
    for (int w = 1; w < DP_FIN / 64; ++w) sum += lds[w];
    return sum;
}

// (s, t) of the five moments, rounded once to f32; s = t = 0 when nothing is selected
__device__ __forceinline__ void dp_fit(const double* __restrict__ m, float* s_out, float* t_out)
{
    const double Sw = m[0], Sy = m[1], Sx = m[2], Syy = m[3], Sxy = m[4];
    double s = 0.0, t = 0.0;
    if (Sw > 0.0) {
        const double det = Sw * Syy - Sy * Sy;
        if (!(det > 1e-12 * (Sw * Syy))) {
            t = Sx / Sw;
        } else {
            s = (Sw * Sxy - Sy * Sx) / det;
            t = (Sx - s * Sy) / Sw;
        }
    }
    *s_out = (float)s; *t_out = (float)t;
}

__global__ __launch_bounds__(DP_THREADS) void k_depth_moments(const float* __restrict__ D, const float* __restrict__ Z, const float* __restrict__ wt,
                                                              const float* __restrict__ wp, int vec, int flags, int n,
                                                              double* __restrict__ partial, int nb)
{
    const DpPixels px = dp_pixels(D, Z, wt, wp, vec, flags, n, (int)blockIdx.x * DP_PIXELS + 4 * (int)threadIdx.x);
    double acc[GS_DEPTH_MOMENTS];
#pragma unroll
    for (int i = 0; i < GS_DEPTH_MOMENTS; ++i) acc[i] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (px.w[k] == 0.0f) continue;                                    // selection: nothing of this pixel is read into a sum
        const double w = (double)px.w[k], x = px.x[k], y = px.y[k];
        const double wy = w * y;
        acc[0] += w; acc[1] += wy; acc[2] += w * x; acc[3] += wy * y; acc[4] += wy * x;
    }
    dp_block_sums<GS_DEPTH_MOMENTS>(acc, partial, nb);
}

// one block per moment
__global__ __launch_bounds__(DP_FIN) void k_depth_finish_moments(const double* __restrict__ partial, int nb, double* __restrict__ moments)
{
    __shared__ double lds[DP_FIN / 64];
    const double sum = dp_finish_row(partial + (size_t)blockIdx.x * nb, nb, lds);
    if (threadIdx.x == 0) moments[blockIdx.x] = sum;
}

// moments: the five finished moments (GS_DEPTH_ALIGN), or NULL: s = 1, t = 0
__global__ __launch_bounds__(DP_THREADS) void k_depth_residual(const float* __restrict__ D, const float* __restrict__ Z, const float* __restrict__ wt,
                                                               const float* __restrict__ wp, int vec, int flags, int n,
                                                               const double* __restrict__ moments, double* __restrict__ partial, int nb)
{
    float s = 1.0f, t = 0.0f;
    if (moments) dp_fit(moments, &s, &t);
    const DpPixels px = dp_pixels(D, Z, wt, wp, vec, flags, n, (int)blockIdx.x * DP_PIXELS + 4 * (int)threadIdx.x);
    double acc[DP_RESIDUAL_SUMS] = { 0.0, 0.0, 0.0 };
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (px.w[k] == 0.0f) continue;
        const double r = px.x[k] - ((double)s * px.y[k] + (double)t);
        const double rho = (flags & GS_DEPTH_L2) ? r * r : fabs(r);
        acc[0] += (double)px.w[k] * rho; acc[1] += (double)px.w[k]; acc[2] += 1.0;
    }
    dp_block_sums<DP_RESIDUAL_SUMS>(acc, partial, nb);
}

// one block: the three rows of per-block sums in one loop (their loads in flight together), then the eight terms
__global__ __launch_bounds__(DP_FIN) void k_depth_finish_loss(const double* __restrict__ partial, int nb, const double* __restrict__ moments,
                                                              float* __restrict__ terms)
{
    __shared__ double lds[DP_FIN / 64][DP_RESIDUAL_SUMS];
    const int t_ = threadIdx.x;
    double a[DP_RESIDUAL_SUMS] = { 0.0, 0.0, 0.0 };
    for (int i = t_; i < nb; i += DP_FIN) {
#pragma unroll
        for (int k = 0; k < DP_RESIDUAL_SUMS; ++k) a[k] += partial[(size_t)k * nb + i];
    }
#pragma unroll
    for (int k = 0; k < DP_RESIDUAL_SUMS; ++k) a[k] = dp_wave_sum(a[k]);
    if ((t_ & 63) == 0) {
#pragma unroll
        for (int k = 0; k < DP_RESIDUAL_SUMS; ++k) lds[t_ >> 6][k] = a[k];
    }
    __syncthreads();
    double sums[DP_RESIDUAL_SUMS];
#pragma unroll
    for (int k = 0; k < DP_RESIDUAL_SUMS; ++k) {
        sums[k] = lds[0][k];
        for (int w = 1; w < DP_FIN / 64; ++w) sums[k] += lds[w][k];
    }
    if (threadIdx.x == 0) {
        float s = 1.0f, t = 0.0f;
        if (moments) dp_fit(moments, &s, &t);
        const bool any = sums[1] > 0.0;
        terms[0] = any ? (float)(sums[0] / sums[1]) : 0.0f;
        terms[1] = any ? (float)sums[1] : 0.0f;
        terms[2] = any ? s : 0.0f;
        terms[3] = any ? t : 0.0f;
        terms[4] = any ? (float)sums[2] : 0.0f;
        terms[5] = terms[6] = terms[7] = 0.0f;
    }
}

__global__ __launch_bounds__(DP_THREADS) void k_depth_loss_backward(const float* __restrict__ D, const float* __restrict__ Z, const float* __restrict__ wt,
                                                                    const float* __restrict__ wp, int vec, int flags, int n,
                                                                    const float* __restrict__ terms, const float* __restrict__ upstream,
                                                                    float* __restrict__ G)
{
    const int p0 = (int)blockIdx.x * DP_PIXELS + 4 * (int)threadIdx.x;
    if (p0 >= n) return;
    const float Sw = terms[1], s = terms[2], t = terms[3];
    const float u = upstream ? upstream[0] : 1.0f;
    const double c = Sw > 0.0f ? (double)u / (double)Sw : 0.0;
    const DpPixels px = dp_pixels(D, Z, wt, wp, vec, flags, n, p0);
    float g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float gk = 0.0f;
        if (px.w[k] != 0.0f && Sw > 0.0f) {
            const double r = px.x[k] - ((double)s * px.y[k] + (double)t);
            const double d = (flags & GS_DEPTH_L2) ? 2.0 * r : (double)(r > 0.0) - (double)(r < 0.0);
            double g64 = ((double)px.w[k] * d) * c;
            if (flags & GS_DEPTH_INVERT_PREDICTED) g64 = g64 * -(px.x[k] * px.x[k]);
            gk = (float)g64;
        }
        g[k] = gk;
    }
    if ((vec & DP_VEC_G) && p0 + 3 < n) {
        *reinterpret_cast<float4*>(G + p0) = make_float4(g[0], g[1], g[2], g[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (p0 + k < n) G[p0 + k] = g[k];
    }
}

static int dp_blocks(int H, int W) { return (int)(((long long)H * W + DP_PIXELS - 1) / DP_PIXELS); }

static int dp_vec(const float* D, const float* Z, const float* wt, const float* wp, const float* G)
{
    auto ok = [](const float* p) { return p && ((uintptr_t)p & 15u) == 0; };
    return (ok(D) ? DP_VEC_D : 0) | (ok(Z) ? DP_VEC_Z : 0) | (ok(wt) ? DP_VEC_WT : 0) | (ok(wp) ? DP_VEC_WP : 0) | (ok(G) ? DP_VEC_G : 0);
}

// 8 doubles for the finished moments, then the per-block sums of the larger pass
size_t gs_depth_ws_size(int H, int W)
{
    return (8 + (size_t)dp_blocks(H, W) * GS_DEPTH_MOMENTS) * sizeof(double);
}

void gs_launch_depth_loss_forward(const float* D, const float* Z, const float* wt, const float* wp, int H, int W, int flags, float* terms, void* ws,
                                  hipStream_t s)
{
    const int nb = dp_blocks(H, W), n = H * W, vec = dp_vec(D, Z, wt, wp, nullptr);
    double* moments = static_cast<double*>(ws);
    double* partial = moments + 8;
    const bool align = (flags & GS_DEPTH_ALIGN) != 0;
    if (align) {
        k_depth_moments<<<nb, DP_THREADS, 0, s>>>(D, Z, wt, wp, vec, flags, n, partial, nb);
        k_depth_finish_moments<<<GS_DEPTH_MOMENTS, DP_FIN, 0, s>>>(partial, nb, moments);
    }
    k_depth_residual<<<nb, DP_THREADS, 0, s>>>(D, Z, wt, wp, vec, flags, n, align ? moments : nullptr, partial, nb);
    k_depth_finish_loss<<<1, DP_FIN, 0, s>>>(partial, nb, align ? moments : nullptr, terms);
}

void gs_launch_depth_loss_backward(const float* D, const float* Z, const float* wt, const float* wp, int H, int W, int flags, const float* terms,
                                   const float* upstream, float* G, hipStream_t s)
{
    const int nb = dp_blocks(H, W), n = H * W, vec = dp_vec(D, Z, wt, wp, G);
    k_depth_loss_backward<<<nb, DP_THREADS, 0, s>>>(D, Z, wt, wp, vec, flags, n, terms, upstream, G);
}
