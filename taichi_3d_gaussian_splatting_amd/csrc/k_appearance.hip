// k_appearance.hip -- per-view exposure compensation (include/gs_appearance.h): the 3x4 affine colour transform of a rendered
// image, its backward and the normal equations of the best affine map onto a target.
//
// Every pass is memory bound (apply: 2 images, backward: 3, moments: 2 and a plane), so each moves its images once and the
// sums ride in the same pass.  A block of 256 threads owns AP_PIXELS consecutive pixels, thread t of block b the four pixels
// 4 (256 b + t) ... in every layout, so the order of every sum -- and with it every bit of the result -- is the same whatever
// the layouts of a call's images are.  A dense 16-byte layout moves them as three float4 (interleaved: 12 floats of 4 pixels)
// or one float4 per channel (planar).  An image that is not dense (a crop, an unaligned base) is addressed pixel by pixel
// through its strides, beside vectorised ones where the layouts of a call differ; so is the tail of a dense image whose pixel
// count is no multiple of four.  A pixel belongs to exactly one thread, which reads all it needs before it writes: in place
// is safe.
//
// Sums: per thread over its four pixels in slot order, a butterfly over the wave (every lane ends with the same bits), the
// four waves in order through LDS -> one partial per block and output, laid out [output][block]; k_appearance_finish_* has one
// block per output, thread t adds the blocks t, t + 256, ... in float64, then the same butterfly and wave order.  No atomics.
#include "gs_common.h"
#include "../../include/gs_appearance.h"

#define AP_THREADS 256
#define AP_WAVES (AP_THREADS / 64)
#define AP_PIXELS GS_APPEARANCE_PIXELS_PER_BLOCK
#define AP_FIN GS_APPEARANCE_FINISH_THREADS
static_assert(AP_PIXELS == 4 * AP_THREADS, "four pixels per thread");
static_assert(AP_FIN % 64 == 0 && AP_FIN <= 1024, "whole waves in the finishing block");

#define AP_SCALAR 0           // any strides
#define AP_VEC3 1             // interleaved {1, 3W, 3}, base 16-byte aligned
#define AP_PLANAR 2           // planar contiguous {HW, W, 1}, base 16-byte aligned, W % 4 == 0

struct ApImage { float* p; long long sc, sy, sx; int mode; };
struct ApTransform { float m[12]; };

// the four pixels of a thread: p0 + k, k < 4
struct ApSlots { int p0; };

__device__ __forceinline__ ApSlots ap_slots()
{
    ApSlots s;
    s.p0 = (int)blockIdx.x * AP_PIXELS + 4 * (int)threadIdx.x;
    return s;
}

__device__ __forceinline__ long long ap_offset(const ApImage& im, int W, int p)
{
    const int y = (int)((unsigned)p / (unsigned)W), x = p - y * W;
    return (long long)y * im.sy + (long long)x * im.sx;
}

// one pixel through the strides; zeros for a slot past the image
__device__ __forceinline__ float3 ap_pixel(const ApImage& im, int W, int n, int p)
{
    float3 r = make_float3(0.0f, 0.0f, 0.0f);
    if (p < n) {
        const float* q = im.p + ap_offset(im, W, p);
        r.x = q[0]; r.y = q[im.sc]; r.z = q[2 * im.sc];
    }
    return r;
}

// v[c][k] = channel c of the thread's pixel k; 0 for a slot past the image.  (Each path builds the three channel vectors as
// values and v is written once behind them: stores to v inside the branches end up in scratch memory.)
__device__ __forceinline__ void ap_load(const ApImage& im, int W, int n, const ApSlots& s, float v[3][4])
{
    float4 r0, r1, r2;
    if (im.mode != AP_SCALAR && s.p0 + 3 < n) {
        if (im.mode == AP_VEC3) {
            const float4* q = reinterpret_cast<const float4*>(im.p + 3ll * s.p0);
            const float4 a = q[0], b = q[1], c = q[2];
            r0 = make_float4(a.x, a.w, b.z, c.y);
            r1 = make_float4(a.y, b.x, b.w, c.z);
            r2 = make_float4(a.z, b.y, c.x, c.w);
        } else {
            r0 = *reinterpret_cast<const float4*>(im.p + s.p0);
            r1 = *reinterpret_cast<const float4*>(im.p + im.sc + s.p0);
            r2 = *reinterpret_cast<const float4*>(im.p + 2 * im.sc + s.p0);
        }
    } else {
        const float3 a = ap_pixel(im, W, n, s.p0), b = ap_pixel(im, W, n, s.p0 + 1), c = ap_pixel(im, W, n, s.p0 + 2),
                     d = ap_pixel(im, W, n, s.p0 + 3);
        r0 = make_float4(a.x, b.x, c.x, d.x);
        r1 = make_float4(a.y, b.y, c.y, d.y);
        r2 = make_float4(a.z, b.z, c.z, d.z);
    }
    v[0][0] = r0.x; v[0][1] = r0.y; v[0][2] = r0.z; v[0][3] = r0.w;
    v[1][0] = r1.x; v[1][1] = r1.y; v[1][2] = r1.z; v[1][3] = r1.w;
    v[2][0] = r2.x; v[2][1] = r2.y; v[2][2] = r2.z; v[2][3] = r2.w;
}

__device__ __forceinline__ void ap_store(const ApImage& im, int W, int n, const ApSlots& s, const float v[3][4])
{
    if (im.mode != AP_SCALAR && s.p0 + 3 < n) {
        if (im.mode == AP_VEC3) {
            float4* q = reinterpret_cast<float4*>(im.p + 3ll * s.p0);
            q[0] = make_float4(v[0][0], v[1][0], v[2][0], v[0][1]);
            q[1] = make_float4(v[1][1], v[2][1], v[0][2], v[1][2]);
            q[2] = make_float4(v[2][2], v[0][3], v[1][3], v[2][3]);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                *reinterpret_cast<float4*>(im.p + (long long)c * im.sc + s.p0) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = s.p0 + k;
        if (p < n) {
            float* q = im.p + ap_offset(im, W, p);
            q[0] = v[0][k]; q[im.sc] = v[1][k]; q[2 * im.sc] = v[2][k];
        }
    }
}

// the (H,W) weight plane: w[k] as stored; 0 for a slot past the image
__device__ __forceinline__ void ap_load_plane(const float* __restrict__ wp, bool vec, int n, const ApSlots& s, float w[4])
{
    float4 r;
    if (vec && s.p0 + 3 < n) {
        r = *reinterpret_cast<const float4*>(wp + s.p0);
    } else {
        const int p1 = s.p0 + 1, p2 = s.p0 + 2, p3 = s.p0 + 3;
        r = make_float4(s.p0 < n ? wp[s.p0] : 0.0f, p1 < n ? wp[p1] : 0.0f, p2 < n ? wp[p2] : 0.0f, p3 < n ? wp[p3] : 0.0f);
    }
    w[0] = r.x; w[1] = r.y; w[2] = r.z; w[3] = r.w;
}

template <class T>
__device__ __forceinline__ T ap_wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// NS sums of a block of AP_THREADS threads -> partial[k * nb + block], the waves added in order
template <class T, int NS>
__device__ __forceinline__ void ap_block_sums(T (&acc)[NS], T* __restrict__ partial, int nb)
{
    __shared__ T lds[AP_WAVES][NS];
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = ap_wave_sum(acc[k]);
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) lds[t >> 6][k] = acc[k];
    }
    __syncthreads();
    if (t < NS) {
        T sum = lds[0][t];
#pragma unroll
        for (int w = 1; w < AP_WAVES; ++w) sum += lds[w][t];
        partial[(size_t)t * nb + blockIdx.x] = sum;
    }
}

__global__ __launch_bounds__(AP_THREADS) void k_appearance_apply(const ApImage X, const ApImage C, const float* __restrict__ M, int W, int n)
{
    ApTransform T;
#pragma unroll
    for (int i = 0; i < 12; ++i) T.m[i] = M[i];
    const ApSlots s = ap_slots();
    if (s.p0 >= n) return;
    float x[3][4], c[3][4];
    ap_load(X, W, n, s, x);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
            c[i][k] = ((T.m[4 * i] * x[0][k] + T.m[4 * i + 1] * x[1][k]) + T.m[4 * i + 2] * x[2][k]) + T.m[4 * i + 3];
    }
    ap_store(C, W, n, s, c);
}

// X.p NULL: no sums (partial unused); GI.p NULL: no image gradient
__global__ __launch_bounds__(AP_THREADS) void k_appearance_backward(const ApImage X, const ApImage G, const ApImage GI, const float* __restrict__ M,
                                                                    int W, int n, float* __restrict__ partial, int nb)
{
    ApTransform T;
#pragma unroll
    for (int i = 0; i < 12; ++i) T.m[i] = M[i];
    const bool sums = partial != nullptr;
    const ApSlots s = ap_slots();
    float x[3][4], g[3][4], acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 0.0f;
    // (no early return: every thread of the block takes part in the block's sums; the slots past the image hold g = 0)
    ap_load(G, W, n, s, g);
    if (sums) ap_load(X, W, n, s, x);
    bool sel[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) sel[k] = !(g[0][k] == 0.0f && g[1][k] == 0.0f && g[2][k] == 0.0f);
    if (sums) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (sel[k]) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) acc[4 * i + j] += g[i][k] * x[j][k];
                    acc[4 * i + 3] += g[i][k];
                }
            }
        }
    }
    if (GI.p) {
        float gi[3][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                gi[j][k] = sel[k] ? (T.m[j] * g[0][k] + T.m[4 + j] * g[1][k]) + T.m[8 + j] * g[2][k] : 0.0f;
        }
        ap_store(GI, W, n, s, gi);
    }
    if (sums) ap_block_sums<float, 12>(acc, partial, nb);
}

__global__ __launch_bounds__(AP_THREADS) void k_appearance_moments(const ApImage X, const ApImage Y, const float* __restrict__ weight, int weight_vec,
                                                                   int W, int n, double* __restrict__ partial, int nb)
{
    const ApSlots s = ap_slots();
    float x[3][4], y[3][4], w[4];
    double acc[GS_APPEARANCE_MOMENTS];
#pragma unroll
    for (int i = 0; i < GS_APPEARANCE_MOMENTS; ++i) acc[i] = 0.0;
    ap_load(X, W, n, s, x);
    ap_load(Y, W, n, s, y);
    if (weight) {
        ap_load_plane(weight, weight_vec != 0, n, s, w);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = s.p0 + k < n ? 1.0f : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float wk = w[k] > 0.0f ? w[k] : 0.0f;                      // a negative or NaN weight is 0
        if (wk == 0.0f) continue;                                          // selection: nothing of this pixel is read into a sum
        const double wd = (double)wk;
        const double u[4] = { (double)x[0][k], (double)x[1][k], (double)x[2][k], 1.0 };
        double wu[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) wu[j] = wd * u[j];
        int o = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = i; j < 4; ++j) acc[o++] += wu[i] * u[j];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[10 + 4 * i + j] += (double)y[i][k] * wu[j];
        }
        acc[22] += wd;
    }
    ap_block_sums<double, GS_APPEARANCE_MOMENTS>(acc, partial, nb);
}

// one block per output k: out[k] = (OUT) sum over the nb blocks of partial[k * nb + b], in float64
template <class IN, class OUT>
__global__ __launch_bounds__(AP_FIN) void k_appearance_finish(const IN* __restrict__ partial, int nb, OUT* __restrict__ out)
{
    __shared__ double lds[AP_FIN / 64];
    const int t = threadIdx.x;
    const IN* row = partial + (size_t)blockIdx.x * nb;
    double a = 0.0;
    for (int i = t; i < nb; i += AP_FIN) a += (double)row[i];
    a = ap_wave_sum(a);
    if ((t & 63) == 0) lds[t >> 6] = a;
    __syncthreads();
    if (t == 0) {
        double sum = lds[0];
        for (int w = 1; w < AP_FIN / 64; ++w) sum += lds[w];
        out[blockIdx.x] = (OUT)sum;
    }
}

static int ap_mode(const GsLossImage& im, int H, int W)
{
    if (((uintptr_t)im.p & 15u) != 0) return AP_SCALAR;
    if (im.sc == 1 && im.sx == 3 && im.sy == 3ll * W) return AP_VEC3;
    if ((W & 3) == 0 && im.sx == 1 && im.sy == (long long)W && im.sc == (long long)H * W) return AP_PLANAR;
    return AP_SCALAR;
}

static ApImage ap_image(const GsLossImage& im, int H, int W)
{
    ApImage r; r.p = const_cast<float*>(im.p); r.sc = im.sc; r.sy = im.sy; r.sx = im.sx; r.mode = im.p ? ap_mode(im, H, W) : AP_SCALAR;
    return r;
}

static int ap_blocks(int H, int W) { return (int)(((long long)H * W + AP_PIXELS - 1) / AP_PIXELS); }

size_t gs_appearance_ws_size(int H, int W)
{
    return (size_t)ap_blocks(H, W) * GS_APPEARANCE_MOMENTS * sizeof(double);        // the larger of the two: 12 floats or 23 doubles per block
}

void gs_launch_appearance_apply(const GsLossImage& X, const float* M, int H, int W, const GsLossImage& C, hipStream_t s)
{
    k_appearance_apply<<<ap_blocks(H, W), AP_THREADS, 0, s>>>(ap_image(X, H, W), ap_image(C, H, W), M, W, H * W);
}

void gs_launch_appearance_backward(const GsLossImage& X, const GsLossImage& G, const float* M, int H, int W, const GsLossImage& GI,
                                   float* grad_transform, void* ws, hipStream_t s)
{
    const int nb = ap_blocks(H, W);
    float* partial = grad_transform ? static_cast<float*>(ws) : nullptr;
    k_appearance_backward<<<nb, AP_THREADS, 0, s>>>(ap_image(X, H, W), ap_image(G, H, W), ap_image(GI, H, W), M, W, H * W, partial, nb);
    if (grad_transform)
        k_appearance_finish<float, float><<<GS_APPEARANCE_FINISH_BLOCKS_BACKWARD, AP_FIN, 0, s>>>(partial, nb, grad_transform);
}

void gs_launch_appearance_moments(const GsLossImage& X, const GsLossImage& Y, const float* weight, int H, int W, double* moments, void* ws,
                                  hipStream_t s)
{
    const int nb = ap_blocks(H, W);
    double* partial = static_cast<double*>(ws);
    const int weight_vec = weight && ((uintptr_t)weight & 15u) == 0 ? 1 : 0;
    k_appearance_moments<<<nb, AP_THREADS, 0, s>>>(ap_image(X, H, W), ap_image(Y, H, W), weight, weight_vec, W, H * W, partial, nb);
    k_appearance_finish<double, double><<<GS_APPEARANCE_FINISH_BLOCKS_MOMENTS, AP_FIN, 0, s>>>(partial, nb, moments);
}
