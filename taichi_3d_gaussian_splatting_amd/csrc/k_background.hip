// k_background.hip -- a background behind the splats (include/gs_background.h): a solid colour or a spherical-harmonics sky
// composited under an image with its accumulated alpha, and the gradient of that to the alpha and to the 48 coefficients.
//
// Both passes are streaming passes over the image.  As in k_appearance.hip a block of 256 threads owns BG_PIXELS consecutive
// pixels, thread t of block b the four pixels 4 (256 b + t) ... in every layout, so the order of every sum -- and with it
// every bit of the result -- is the same whatever the layouts of a call's images are.  A dense 16-byte layout moves them as
// three float4 (interleaved) or one float4 per channel (planar); any other image is addressed pixel by pixel through its
// strides, and so is the tail of a dense image whose pixel count is no multiple of four.  A pixel belongs to exactly one
// thread, which reads all it needs before it writes: in place is safe.
//
// The kernels are instantiated per `bands`, so a solid colour (bands 0) computes no direction and keeps 3 sums where the
// full sky keeps 48.  The block's sums: per thread over its four pixels, then over the wave.  The wave step is the butterfly
// the header states (v + v[lane ^ 32], ^ 16, ...), but each of its levels is run on half of the values only: a lane whose bit
// is clear keeps the lower half of what it holds and hands the upper half to its partner, the partner the other way round, so
// 48 sums cost 24 + 12 + 6 + 3 + 2 + 1 exchanges instead of 6 x 48.  An f32 add commutes, so every value has the bits of the
// full butterfly.  Then the four waves in order through LDS -> one partial per block and output, laid out [output][block];
// k_background_finish has one block per output, thread t adds the blocks t, t + 256, ... in float64.  No atomics.
#include "gs_point_math.h"
#include "../../include/gs_background.h"

#define BG_THREADS 256
#define BG_WAVES (BG_THREADS / 64)
#define BG_PIXELS GS_BACKGROUND_PIXELS_PER_BLOCK
#define BG_FIN GS_BACKGROUND_FINISH_THREADS
static_assert(BG_PIXELS == 4 * BG_THREADS, "four pixels per thread");
static_assert(BG_FIN % 64 == 0 && BG_FIN <= 1024, "whole waves in the finishing block");
static_assert(GS_BACKGROUND_FINISH_BLOCKS == GS_BACKGROUND_COEF_FLOATS && GS_BACKGROUND_COEF_FLOATS == 48, "one finishing block per coefficient");

#define BG_SCALAR 0           // any strides
#define BG_VEC3 1             // interleaved {1, 3W, 3}, base 16-byte aligned
#define BG_PLANAR 2           // planar contiguous {HW, W, 1}, base 16-byte aligned, W % 4 == 0

struct BgImage { float* p; long long sc, sy, sx; int mode; };
// what a sky needs of the camera: the intrinsics and the quaternion, read by every thread from the same addresses
struct BgView { const float* q; const float* Km; };

__device__ __forceinline__ long long bg_offset(const BgImage& im, int W, int p)
{
    const int y = (int)((unsigned)p / (unsigned)W), x = p - y * W;
    return (long long)y * im.sy + (long long)x * im.sx;
}

// one pixel through the strides; zeros for a slot past the image
__device__ __forceinline__ float3 bg_pixel(const BgImage& im, int W, int n, int p)
{
    float3 r = make_float3(0.0f, 0.0f, 0.0f);
    if (p < n) {
        const float* q = im.p + bg_offset(im, W, p);
        r.x = q[0]; r.y = q[im.sc]; r.z = q[2 * im.sc];
    }
    return r;
}

// v[c][k] = channel c of the thread's pixel p0 + k; 0 for a slot past the image.  (Each path builds the three channel vectors
// as values and v is written once behind them: stores to v inside the branches end up in scratch memory.)
__device__ __forceinline__ void bg_load(const BgImage& im, int W, int n, int p0, float v[3][4])
{
    float4 r0, r1, r2;
    if (im.mode != BG_SCALAR && p0 + 3 < n) {
        if (im.mode == BG_VEC3) {
            const float4* q = reinterpret_cast<const float4*>(im.p + 3ll * p0);
            const float4 a = q[0], b = q[1], c = q[2];
            r0 = make_float4(a.x, a.w, b.z, c.y);
            r1 = make_float4(a.y, b.x, b.w, c.z);
            r2 = make_float4(a.z, b.y, c.x, c.w);
        } else {
            r0 = *reinterpret_cast<const float4*>(im.p + p0);
            r1 = *reinterpret_cast<const float4*>(im.p + im.sc + p0);
            r2 = *reinterpret_cast<const float4*>(im.p + 2 * im.sc + p0);
        }
    } else {
        const float3 a = bg_pixel(im, W, n, p0), b = bg_pixel(im, W, n, p0 + 1), c = bg_pixel(im, W, n, p0 + 2),
                     d = bg_pixel(im, W, n, p0 + 3);
        r0 = make_float4(a.x, b.x, c.x, d.x);
        r1 = make_float4(a.y, b.y, c.y, d.y);
        r2 = make_float4(a.z, b.z, c.z, d.z);
    }
    v[0][0] = r0.x; v[0][1] = r0.y; v[0][2] = r0.z; v[0][3] = r0.w;
    v[1][0] = r1.x; v[1][1] = r1.y; v[1][2] = r1.z; v[1][3] = r1.w;
    v[2][0] = r2.x; v[2][1] = r2.y; v[2][2] = r2.z; v[2][3] = r2.w;
}

__device__ __forceinline__ void bg_store(const BgImage& im, int W, int n, int p0, const float v[3][4])
{
    if (im.mode != BG_SCALAR && p0 + 3 < n) {
        if (im.mode == BG_VEC3) {
            float4* q = reinterpret_cast<float4*>(im.p + 3ll * p0);
            q[0] = make_float4(v[0][0], v[1][0], v[2][0], v[0][1]);
            q[1] = make_float4(v[1][1], v[2][1], v[0][2], v[1][2]);
            q[2] = make_float4(v[2][2], v[0][3], v[1][3], v[2][3]);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                *reinterpret_cast<float4*>(im.p + (long long)c * im.sc + p0) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = p0 + k;
        if (p < n) {
            float* q = im.p + bg_offset(im, W, p);
            q[0] = v[0][k]; q[im.sc] = v[1][k]; q[2 * im.sc] = v[2][k];
        }
    }
}

// a contiguous (H,W) plane: w[k] as stored; 0 for a slot past the image
__device__ __forceinline__ void bg_load_plane(const float* __restrict__ wp, bool vec, int n, int p0, float w[4])
{
    float4 r;
    if (vec && p0 + 3 < n) {
        r = *reinterpret_cast<const float4*>(wp + p0);
    } else {
        const int p1 = p0 + 1, p2 = p0 + 2, p3 = p0 + 3;
        r = make_float4(p0 < n ? wp[p0] : 0.0f, p1 < n ? wp[p1] : 0.0f, p2 < n ? wp[p2] : 0.0f, p3 < n ? wp[p3] : 0.0f);
    }
    w[0] = r.x; w[1] = r.y; w[2] = r.z; w[3] = r.w;
}

__device__ __forceinline__ void bg_store_plane(float* __restrict__ wp, bool vec, int n, int p0, const float w[4])
{
    if (vec && p0 + 3 < n) {
        *reinterpret_cast<float4*>(wp + p0) = make_float4(w[0], w[1], w[2], w[3]);
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (p0 + k < n) wp[p0 + k] = w[k];
}

// ---- the background's colour at a pixel -------------------------------------------------------------------------------
// The camera of a call, in registers: R of the quaternion as given (camera -> point-cloud frame) and fx, fy, cx, cy.
struct BgCamera { float R[9], fx, fy, cx, cy; };

template <int BANDS>
__device__ __forceinline__ BgCamera bg_camera(const BgView& V)
{
    BgCamera c = {};
    if constexpr (BANDS > 0) {
        const float q[4] = { V.q[0], V.q[1], V.q[2], V.q[3] };
        rotation_from_quaternion(q, c.R);
        c.fx = V.Km[0]; c.cx = V.Km[2]; c.fy = V.Km[4]; c.cy = V.Km[5];
    }
    return c;
}

// Y[0 .. K) of pixel p; Y[0] = 1 (the constant term is taken without the basis' own Y_0)
template <int BANDS>
__device__ __forceinline__ void bg_basis(const BgCamera& cam, int W, int p, float (&Y)[16])
{
    Y[0] = 1.0f;
    if constexpr (BANDS > 0) {
        const int y = (int)((unsigned)p / (unsigned)W), x = p - y * W;
        const float a = (((float)x + 0.5f) - cam.cx) / cam.fx, b = (((float)y + 0.5f) - cam.cy) / cam.fy;
        const float nrm = sqrtf((a * a + b * b) + 1.0f);
        const float d0 = a / nrm, d1 = b / nrm, d2 = 1.0f / nrm;
        const float dx = (cam.R[0] * d0 + cam.R[1] * d1) + cam.R[2] * d2;
        const float dy = (cam.R[3] * d0 + cam.R[4] * d1) + cam.R[5] * d2;
        const float dz = (cam.R[6] * d0 + cam.R[7] * d1) + cam.R[8] * d2;
        float sh[16];
        gs_sh16(dx, dy, dz, sh);
#pragma unroll
        for (int k = 1; k < (BANDS + 1) * (BANDS + 1); ++k) Y[k] = sh[k];
    }
}

template <int BANDS>
__device__ __forceinline__ void bg_colour(const float* __restrict__ coef, const float (&Y)[16], float c[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float v = coef[16 * i];
#pragma unroll
        for (int k = 1; k < (BANDS + 1) * (BANDS + 1); ++k) v = v + coef[16 * i + k] * Y[k];
        c[i] = v;
    }
}

// ---- composite ------------------------------------------------------------------------------------------------------
// MODE 0: x + t c;  1 (GS_BACKGROUND_STRAIGHT): x A + t c;  2 (GS_BACKGROUND_COLOURS_ONLY): c
template <int BANDS, int MODE>
__global__ __launch_bounds__(BG_THREADS) void k_background_composite(const BgImage X, const float* __restrict__ alpha, int alpha_vec,
                                                                    const float* __restrict__ coef, const BgView V, int W, int n, const BgImage O)
{
    const int p0 = (int)blockIdx.x * BG_PIXELS + 4 * (int)threadIdx.x;
    if (p0 >= n) return;
    const BgCamera cam = bg_camera<BANDS>(V);
    float x[3][4], A[4], o[3][4];
    if constexpr (MODE != 2) {
        bg_load(X, W, n, p0, x);
        bg_load_plane(alpha, alpha_vec != 0, n, p0, A);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float Y[16], c[3];
        bg_basis<BANDS>(cam, W, p0 + k, Y);
        bg_colour<BANDS>(coef, Y, c);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if constexpr (MODE == 2) {
                o[i][k] = c[i];
            } else {
                const float t = 1.0f - A[k];
                const float fg = MODE == 1 ? x[i][k] * A[k] : x[i][k];
                o[i][k] = fg + t * c[i];
            }
        }
    }
    bg_store(O, W, n, p0, o);
}

// ---- backward -------------------------------------------------------------------------------------------------------
// One level of the wave butterfly over the N values a lane holds, run on half of them: afterwards the lane holds the sums
// [base, base + cnt) of the 64 >> ... lanes it has met, in v[0 .. cnt).  N == 1: the plain butterfly step.
template <int N, int O>
__device__ __forceinline__ void bg_wave_level(float* v, int& base, int& cnt)
{
    if constexpr (N == 1) {
        v[0] = v[0] + __shfl_xor(v[0], O, 64);
    } else {
        constexpr int HALF = (N + 1) / 2;
        const bool up = ((int)threadIdx.x & O) != 0;
#pragma unroll
        for (int j = 0; j < HALF; ++j) {
            const float hi = HALF + j < N ? v[HALF + j] : 0.0f;
            const float keep = up ? hi : v[j], give = up ? v[j] : hi;
            v[j] = keep + __shfl_xor(give, O, 64);
        }
        if (up) { base += HALF; cnt -= HALF; }
        else cnt = cnt < HALF ? cnt : HALF;
    }
}

// NS sums of a block of BG_THREADS threads -> partial[row(k) * nb + block], row(k) = 16 (k / K) + k % K, the waves added in order
template <int NS, int K>
__device__ __forceinline__ void bg_block_sums(float (&acc)[NS], float* __restrict__ partial, int nb)
{
    __shared__ float lds[BG_WAVES][NS];
    const int t = threadIdx.x;
    int base = 0, cnt = NS;
    constexpr int N1 = (NS + 1) / 2, N2 = (N1 + 1) / 2, N3 = (N2 + 1) / 2, N4 = (N3 + 1) / 2, N5 = (N4 + 1) / 2;
    static_assert((N5 + 1) / 2 == 1, "six levels bring the values of a lane down to one");
    bg_wave_level<NS, 32>(acc, base, cnt);
    bg_wave_level<N1, 16>(acc, base, cnt);
    bg_wave_level<N2, 8>(acc, base, cnt);
    bg_wave_level<N3, 4>(acc, base, cnt);
    bg_wave_level<N4, 2>(acc, base, cnt);
    bg_wave_level<N5, 1>(acc, base, cnt);
    if (cnt >= 1) lds[t >> 6][base] = acc[0];          // (lanes that hold the same sum hold the same bits)
    __syncthreads();
    if (t < NS) {
        float sum = lds[0][t];
#pragma unroll
        for (int w = 1; w < BG_WAVES; ++w) sum += lds[w][t];
        partial[(size_t)(16 * (t / K) + t % K) * nb + blockIdx.x] = sum;
    }
}

// partial NULL: no sums (alpha is not read); grad_alpha NULL: no alpha gradient
template <int BANDS>
__global__ __launch_bounds__(BG_THREADS) void k_background_backward(const BgImage G, const float* __restrict__ alpha, int alpha_vec,
                                                                   const float* __restrict__ coef, const BgView V, int W, int n,
                                                                   float* __restrict__ grad_alpha, int grad_alpha_vec,
                                                                   float* __restrict__ partial, int nb)
{
    constexpr int K = (BANDS + 1) * (BANDS + 1);
    const bool sums = partial != nullptr;
    const int p0 = (int)blockIdx.x * BG_PIXELS + 4 * (int)threadIdx.x;
    const BgCamera cam = bg_camera<BANDS>(V);
    float g[3][4], A[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, ga[4], acc[3 * K];
#pragma unroll
    for (int i = 0; i < 3 * K; ++i) acc[i] = 0.0f;
    // (no early return: every thread of the block takes part in the block's sums; the slots past the image hold g = 0)
    bg_load(G, W, n, p0, g);
    if (sums) bg_load_plane(alpha, alpha_vec != 0, n, p0, A);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool sel = !(g[0][k] == 0.0f && g[1][k] == 0.0f && g[2][k] == 0.0f);
        float Y[16], c[3];
        // (a slot past the image is not selected; its basis is that of a pixel below the image and goes nowhere)
        bg_basis<BANDS>(cam, W, p0 + k, Y);
        bg_colour<BANDS>(coef, Y, c);
        ga[k] = sel ? -((g[0][k] * c[0] + g[1][k] * c[1]) + g[2][k] * c[2]) : 0.0f;
        if (sums && sel) {
            const float t = 1.0f - A[k];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float gt = g[i][k] * t;
                acc[i * K] += gt;
#pragma unroll
                for (int j = 1; j < K; ++j) acc[i * K + j] += gt * Y[j];
            }
        }
    }
    if (grad_alpha && p0 < n) bg_store_plane(grad_alpha, grad_alpha_vec != 0, n, p0, ga);
    if (sums) bg_block_sums<3 * K, K>(acc, partial, nb);
}

// one block per output o = 16 i + k: grad_coef[o] = (float) sum over the nb blocks of partial[o * nb + b], in float64; +0 for k >= K
__global__ __launch_bounds__(BG_FIN) void k_background_finish(const float* __restrict__ partial, int nb, int K, float* __restrict__ out)
{
    __shared__ double lds[BG_FIN / 64];
    const int t = threadIdx.x;
    if ((int)(blockIdx.x & 15u) >= K) {
        if (t == 0) out[blockIdx.x] = 0.0f;
        return;
    }
    const float* row = partial + (size_t)blockIdx.x * nb;
    double a = 0.0;
    for (int i = t; i < nb; i += BG_FIN) a += (double)row[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if ((t & 63) == 0) lds[t >> 6] = a;
    __syncthreads();
    if (t == 0) {
        double sum = lds[0];
        for (int w = 1; w < BG_FIN / 64; ++w) sum += lds[w];
        out[blockIdx.x] = (float)sum;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------
static int bg_mode(const GsLossImage& im, int H, int W)
{
    if (((uintptr_t)im.p & 15u) != 0) return BG_SCALAR;
    if (im.sc == 1 && im.sx == 3 && im.sy == 3ll * W) return BG_VEC3;
    if ((W & 3) == 0 && im.sx == 1 && im.sy == (long long)W && im.sc == (long long)H * W) return BG_PLANAR;
    return BG_SCALAR;
}

static BgImage bg_image(const GsLossImage& im, int H, int W)
{
    BgImage r; r.p = const_cast<float*>(im.p); r.sc = im.sc; r.sy = im.sy; r.sx = im.sx; r.mode = im.p ? bg_mode(im, H, W) : BG_SCALAR;
    return r;
}

static int bg_plane_vec(const float* p) { return p && ((uintptr_t)p & 15u) == 0 ? 1 : 0; }
static int bg_blocks(int H, int W) { return (int)(((long long)H * W + BG_PIXELS - 1) / BG_PIXELS); }

size_t gs_background_ws_size(int H, int W) { return (size_t)bg_blocks(H, W) * GS_BACKGROUND_COEF_FLOATS * sizeof(float); }

template <int BANDS>
static void bg_composite(const GsLossImage& X, const float* alpha, const float* coef, const BgView V, int H, int W, int flags, const GsLossImage& O,
                         hipStream_t s)
{
    const int nb = bg_blocks(H, W), n = H * W, av = bg_plane_vec(alpha);
    const BgImage x = bg_image(X, H, W), o = bg_image(O, H, W);
    if (flags & GS_BACKGROUND_COLOURS_ONLY) k_background_composite<BANDS, 2><<<nb, BG_THREADS, 0, s>>>(x, alpha, av, coef, V, W, n, o);
    else if (flags & GS_BACKGROUND_STRAIGHT) k_background_composite<BANDS, 1><<<nb, BG_THREADS, 0, s>>>(x, alpha, av, coef, V, W, n, o);
    else k_background_composite<BANDS, 0><<<nb, BG_THREADS, 0, s>>>(x, alpha, av, coef, V, W, n, o);
}

void gs_launch_background_composite(const GsLossImage& X, const float* alpha, const float* coef, int bands, const float* q, const float* Km,
                                    int H, int W, int flags, const GsLossImage& O, hipStream_t s)
{
    const BgView V{ q, Km };
    switch (bands) {
    case 0: bg_composite<0>(X, alpha, coef, V, H, W, flags, O, s); break;
    case 1: bg_composite<1>(X, alpha, coef, V, H, W, flags, O, s); break;
    case 2: bg_composite<2>(X, alpha, coef, V, H, W, flags, O, s); break;
    default: bg_composite<3>(X, alpha, coef, V, H, W, flags, O, s); break;
    }
}

void gs_launch_background_backward(const GsLossImage& G, const float* alpha, const float* coef, int bands, const float* q, const float* Km,
                                   int H, int W, float* grad_alpha, float* grad_coef, void* ws, hipStream_t s)
{
    const int nb = bg_blocks(H, W), n = H * W, av = bg_plane_vec(alpha), gv = bg_plane_vec(grad_alpha);
    const BgView V{ q, Km };
    const BgImage g = bg_image(G, H, W);
    float* partial = grad_coef ? static_cast<float*>(ws) : nullptr;
    switch (bands) {
    case 0: k_background_backward<0><<<nb, BG_THREADS, 0, s>>>(g, alpha, av, coef, V, W, n, grad_alpha, gv, partial, nb); break;
    case 1: k_background_backward<1><<<nb, BG_THREADS, 0, s>>>(g, alpha, av, coef, V, W, n, grad_alpha, gv, partial, nb); break;
    case 2: k_background_backward<2><<<nb, BG_THREADS, 0, s>>>(g, alpha, av, coef, V, W, n, grad_alpha, gv, partial, nb); break;
    default: k_background_backward<3><<<nb, BG_THREADS, 0, s>>>(g, alpha, av, coef, V, W, n, grad_alpha, gv, partial, nb); break;
    }
    if (grad_coef)
        k_background_finish<<<GS_BACKGROUND_FINISH_BLOCKS, BG_FIN, 0, s>>>(partial, nb, (bands + 1) * (bands + 1), grad_coef);
}
