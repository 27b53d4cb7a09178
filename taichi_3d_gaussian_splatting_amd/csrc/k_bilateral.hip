// k_bilateral.hip -- per-view bilateral grids (include/gs_bilateral.h): the slice of a grid of 3x4 colour transforms at
// (x, y, luminance) applied to a rendered image, its backward to the image and to the grid, and the grid's total variation.
//
// The image passes (slice, backward to the image) are one pixel per thread through the strides: a pixel gathers the 24 floats
// of two levels at each of the four image-plane vertices of its cell (six 16-byte loads per vertex, served by L1/L2: a whole
// default grid is 96 KiB), which outweighs its own six floats, so no layout gets a vector path and none is special.  A pixel
// belongs to one thread, which reads all it needs before it writes: in place is safe.
//
// The grid's gradient is a gather, not a scatter (no float atomic in this library): a block owns one image-plane vertex (or a
// run of rows of its footprint, where the grid is small), walks the pixels of the at most 2x2 cells around it and keeps the
// 12 L sums of all L levels in registers -- the level loop is unrolled at compile time (L is a template argument), a level
// the pixel does not reach adds a selected +0, so no register array is indexed at run time.  Then the fixed order of
// k_appearance.hip: thread, butterfly over the wave, waves in order through LDS; where blocks meet, k_bilateral_gather_finish
// adds them in float64 in block order.
#include "gs_common.h"
#include "../../include/gs_bilateral.h"
#include <cstring>

#define BG_THREADS GS_BILATERAL_THREADS
#define BG_GATHER GS_BILATERAL_GATHER_THREADS
#define BG_TV GS_BILATERAL_TV_THREADS
#define BG_MAX_XY GS_BILATERAL_MAX_XY
static_assert(BG_THREADS % 64 == 0 && BG_GATHER % 64 == 0 && BG_TV % 64 == 0 && BG_TV <= 1024, "whole waves");
static_assert(12 * GS_BILATERAL_MAX_L <= BG_GATHER, "one thread per sum writes the block's result");

struct BgImage { float* p; long long sc, sy, sx; };
struct BgGrid { const float* v; int Gx, Gy, L; float sx, sy; };       // sx, sy: the two scale factors of the header
// xs[c]: the first column of column cell c (xs[Gx-1] = W); ys likewise
struct BgCells { int xs[BG_MAX_XY]; int ys[BG_MAX_XY]; };

// where a coordinate falls along an image-plane axis: the lower vertex and the fraction
__host__ __device__ __forceinline__ int bg_cell(int x, float scale, int G, float* t)
{
    const float g = (float)x * scale;
    int i0 = (int)g;
    i0 = i0 < G - 2 ? i0 : G - 2;
    *t = g - (float)i0;
    return i0;
}

// along the guide: lum -> level and fraction; *inside: the clamp does not hold the luminance
__device__ __forceinline__ int bg_level(float x0, float x1, float x2, int L, float* t, bool* inside)
{
    const float lum = (0.299f * x0 + 0.587f * x1) + 0.114f * x2;
    const float lc = lum > 0.0f ? (lum < 1.0f ? lum : 1.0f) : 0.0f;
    *inside = lum > 0.0f && lum < 1.0f;
    const float g = lc * (float)(L - 1);
    int i0 = (int)g;
    i0 = i0 < L - 2 ? i0 : L - 2;
    *t = g - (float)i0;
    return i0;
}

__device__ __forceinline__ float bg_lerp(float a, float b, float t) { return a + t * (b - a); }

__device__ __forceinline__ void bg_load24(const float* __restrict__ q, float v[24])
{
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float4 a = reinterpret_cast<const float4*>(q)[i];
        v[4 * i] = a.x; v[4 * i + 1] = a.y; v[4 * i + 2] = a.z; v[4 * i + 3] = a.w;
    }
}

// M and dM of the header at pixel (x, y) with input colour (x0, x1, x2)
__device__ __forceinline__ void bg_transform(const BgGrid& g, int x, int y, float x0, float x1, float x2, float M[12], float dM[12], bool* inside)
{
    float tx, ty, tz;
    const int ix0 = bg_cell(x, g.sx, g.Gx, &tx), iy0 = bg_cell(y, g.sy, g.Gy, &ty), iz0 = bg_level(x0, x1, x2, g.L, &tz, inside);
    const float* base = g.v + 12 * ((iy0 * g.Gx + ix0) * g.L + iz0);
    const int dx = 12 * g.L, dy = dx * g.Gx;
    float v00[24], v01[24], v10[24], v11[24];
    bg_load24(base, v00);
    bg_load24(base + dx, v01);
    bg_load24(base + dy, v10);
    bg_load24(base + dy + dx, v11);
    float P[24];
#pragma unroll
    for (int k = 0; k < 24; ++k) P[k] = bg_lerp(bg_lerp(v00[k], v01[k], tx), bg_lerp(v10[k], v11[k], tx), ty);
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        dM[k] = P[12 + k] - P[k];
        M[k] = P[k] + tz * dM[k];
    }
}

__device__ __forceinline__ long long bg_offset(const BgImage& im, int x, int y) { return (long long)y * im.sy + (long long)x * im.sx; }

__global__ __launch_bounds__(BG_THREADS) void k_bilateral_slice(const BgImage X, const BgImage C, const BgGrid g, int W, int n)
{
    const int p = (int)blockIdx.x * BG_THREADS + (int)threadIdx.x;
    if (p >= n) return;
    const int y = (int)((unsigned)p / (unsigned)W), x = p - y * W;
    const float* q = X.p + bg_offset(X, x, y);
    const float x0 = q[0], x1 = q[X.sc], x2 = q[2 * X.sc];
    float M[12], dM[12];
    bool inside;
    bg_transform(g, x, y, x0, x1, x2, M, dM, &inside);
    float c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = ((M[4 * i] * x0 + M[4 * i + 1] * x1) + M[4 * i + 2] * x2) + M[4 * i + 3];
    float* o = C.p + bg_offset(C, x, y);
    o[0] = c[0]; o[C.sc] = c[1]; o[2 * C.sc] = c[2];
}

__global__ __launch_bounds__(BG_THREADS) void k_bilateral_backward_image(const BgImage X, const BgImage G, const BgImage GI, const BgGrid g, int W, int n)
{
    const int p = (int)blockIdx.x * BG_THREADS + (int)threadIdx.x;
    if (p >= n) return;
    const int y = (int)((unsigned)p / (unsigned)W), x = p - y * W;
    const float* gq = G.p + bg_offset(G, x, y);
    const float g0 = gq[0], g1 = gq[G.sc], g2 = gq[2 * G.sc];
    float r[3] = { 0.0f, 0.0f, 0.0f };
    if (!(g0 == 0.0f && g1 == 0.0f && g2 == 0.0f)) {
        const float* q = X.p + bg_offset(X, x, y);
        const float x0 = q[0], x1 = q[X.sc], x2 = q[2 * X.sc];
        float M[12], dM[12];
        bool inside;
        bg_transform(g, x, y, x0, x1, x2, M, dM, &inside);
#pragma unroll
        for (int j = 0; j < 3; ++j) r[j] = (M[j] * g0 + M[4 + j] * g1) + M[8 + j] * g2;
        if (inside) {
            float D[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) D[i] = ((dM[4 * i] * x0 + dM[4 * i + 1] * x1) + dM[4 * i + 2] * x2) + dM[4 * i + 3];
            const float S = (g0 * D[0] + g1 * D[1]) + g2 * D[2];
            const float Lm1 = (float)(g.L - 1);
            r[0] = r[0] + (Lm1 * 0.299f) * S;
            r[1] = r[1] + (Lm1 * 0.587f) * S;
            r[2] = r[2] + (Lm1 * 0.114f) * S;
        }
    }
    float* o = GI.p + bg_offset(GI, x, y);
    o[0] = r[0]; o[GI.sc] = r[1]; o[2 * GI.sc] = r[2];
}

template <class T>
__device__ __forceinline__ T bg_wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct BgPixel { float g[3], u[3]; int x, y; bool sel; };

// pixel q of the block's rows (row-major over [xa, xa + fw) from row ya on), loaded whether or not it is selected: both images'
// loads leave together.  A q past the rows re-reads pixel `last` and is not selected.
__device__ __forceinline__ BgPixel bg_gather_load(const BgImage& X, const BgImage& G, int q, int npix, int last, int xa, int ya, int fw)
{
    BgPixel p;
    const bool valid = q < npix;
    const int qq = valid ? q : last;
    const int ry = (int)((unsigned)qq / (unsigned)fw);
    p.x = xa + (qq - ry * fw); p.y = ya + ry;
    const float* gq = G.p + bg_offset(G, p.x, p.y);
    const float* xq = X.p + bg_offset(X, p.x, p.y);
    p.g[0] = gq[0]; p.g[1] = gq[G.sc]; p.g[2] = gq[2 * G.sc];
    p.u[0] = xq[0]; p.u[1] = xq[X.sc]; p.u[2] = xq[2 * X.sc];
    p.sel = valid && !(p.g[0] == 0.0f && p.g[1] == 0.0f && p.g[2] == 0.0f);
    return p;
}

// the pixel's terms into the sums of vertex (iy, ix): selection, so a pixel that is not selected adds +0 whatever it holds
template <int L>
__device__ __forceinline__ void bg_gather_add(float (&acc)[12 * L], const BgPixel& p, const BgGrid& g, int ix, int iy)
{
    float tx, ty, tz;
    bool inside;
    const int ix0 = bg_cell(p.x, g.sx, g.Gx, &tx), iy0 = bg_cell(p.y, g.sy, g.Gy, &ty), iz0 = bg_level(p.u[0], p.u[1], p.u[2], L, &tz, &inside);
    const float wx = ix == ix0 ? 1.0f - tx : tx, wy = iy == iy0 ? 1.0f - ty : ty;
    const float wxy = wx * wy;
    const float w0 = wxy * (1.0f - tz), w1 = wxy * tz;
    float t0[12], t1[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float a0 = w0 * p.g[i], a1 = w1 * p.g[i];
#pragma unroll
        for (int j = 0; j < 3; ++j) { t0[4 * i + j] = a0 * p.u[j]; t1[4 * i + j] = a1 * p.u[j]; }
        t0[4 * i + 3] = a0; t1[4 * i + 3] = a1;
    }
#pragma unroll
    for (int l = 0; l < L; ++l) {
        const bool lo = p.sel && l == iz0, hi = p.sel && l == iz0 + 1;
#pragma unroll
        for (int k = 0; k < 12; ++k) acc[12 * l + k] += lo ? t0[k] : (hi ? t1[k] : 0.0f);
    }
}

// block b = v * S + s: rows [s R, (s+1) R) of the footprint of image-plane vertex v -> out[b * 12 L + ...].  The loop is free of
// branches and takes two of the thread's pixels per turn, so that four images' loads are in flight before the first is used:
// the pass is bound by their latency, not by its arithmetic.
template <int L>
__global__ __launch_bounds__(BG_GATHER) void k_bilateral_gather(const BgImage X, const BgImage G, const BgGrid g, const BgCells cells, int S,
                                                                float* __restrict__ out)
{
    constexpr int NS = 12 * L;
    __shared__ float lds[BG_GATHER / 64][NS];
    const int t = threadIdx.x;
    const int v = (int)blockIdx.x / S, s = (int)blockIdx.x - v * S;
    const int iy = v / g.Gx, ix = v - iy * g.Gx;
    const int xa = cells.xs[ix > 0 ? ix - 1 : 0], xb = cells.xs[ix + 1 < g.Gx ? ix + 1 : g.Gx - 1];
    const int y0 = cells.ys[iy > 0 ? iy - 1 : 0], y1 = cells.ys[iy + 1 < g.Gy ? iy + 1 : g.Gy - 1];
    const int rows = y1 - y0, R = (rows + S - 1) / S;
    const int ya = y0 + s * R, yb = ya + R < y1 ? ya + R : y1;
    const int fw = xb - xa;
    const int npix = (yb > ya && fw > 0) ? fw * (yb - ya) : 0;

    float acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0f;
    for (int q = t; q < npix; q += 2 * BG_GATHER) {
        const BgPixel a = bg_gather_load(X, G, q, npix, q, xa, ya, fw), b = bg_gather_load(X, G, q + BG_GATHER, npix, q, xa, ya, fw);
        bg_gather_add<L>(acc, a, g, ix, iy);
        bg_gather_add<L>(acc, b, g, ix, iy);
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = bg_wave_sum(acc[k]);
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) lds[t >> 6][k] = acc[k];
    }
    __syncthreads();
    if (t < NS) {
        float sum = lds[0][t];
#pragma unroll
        for (int w = 1; w < BG_GATHER / 64; ++w) sum += lds[w][t];
        out[(size_t)blockIdx.x * NS + t] = sum;
    }
}

// grad[o] = (float) sum over s, in order, of (double)partial[(v S + s) ns + r], o = v ns + r
__global__ __launch_bounds__(256) void k_bilateral_gather_finish(const float* __restrict__ partial, int S, int ns, int n_out, float* __restrict__ grad)
{
    const int o = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (o >= n_out) return;
    const int v = o / ns, r = o - v * ns;
    const float* q = partial + ((size_t)v * S) * ns + r;
    double a = 0.0;
    for (int s = 0; s < S; ++s) a += (double)q[(size_t)s * ns];
    grad[o] = (float)a;
}

__global__ __launch_bounds__(BG_TV) void k_bilateral_tv(const float* __restrict__ grid, int Gx, int Gy, int L, float weight, float rx, float ry, float rz,
                                                        double cx, double cy, double cz, float* __restrict__ grad, float* __restrict__ value)
{
    __shared__ double lds[BG_TV / 64][3];
    const int t = threadIdx.x;
    const int n = 12 * Gx * Gy * L, dz = 12, dx = 12 * L, dy = dx * Gx;
    double T[3] = { 0.0, 0.0, 0.0 };
    for (int e = t; e < n; e += BG_TV) {
        const int vtx = e / 12, r = vtx / L, l = vtx - r * L, iy = r / Gx, ix = r - iy * Gx;
        const float v = grid[e];
        const float nx = ix + 1 < Gx ? grid[e + dx] - v : 0.0f;
        const float ny = iy + 1 < Gy ? grid[e + dy] - v : 0.0f;
        const float nz = l + 1 < L ? grid[e + dz] - v : 0.0f;
        if (ix + 1 < Gx) T[0] += (double)nx * (double)nx;
        if (iy + 1 < Gy) T[1] += (double)ny * (double)ny;
        if (l + 1 < L) T[2] += (double)nz * (double)nz;
        if (grad) {
            const float qx = (ix > 0 ? v - grid[e - dx] : 0.0f) - nx;
            const float qy = (iy > 0 ? v - grid[e - dy] : 0.0f) - ny;
            const float qz = (l > 0 ? v - grid[e - dz] : 0.0f) - nz;
            grad[e] = grad[e] + weight * ((rx * qx + ry * qy) + rz * qz);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) T[a] = bg_wave_sum(T[a]);
    if ((t & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) lds[t >> 6][a] = T[a];
    }
    __syncthreads();
    if (t == 0) {
        double sum[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            sum[a] = lds[0][a];
            for (int w = 1; w < BG_TV / 64; ++w) sum[a] += lds[w][a];
        }
        *value = (float)((sum[0] / cx + sum[1] / cy) + sum[2] / cz);
    }
}

static BgImage bg_image(const GsLossImage& im)
{
    BgImage r; r.p = const_cast<float*>(im.p); r.sc = im.sc; r.sy = im.sy; r.sx = im.sx;
    return r;
}

static float bg_scale(int G, int n) { return n > 1 ? (float)(G - 1) / (float)(n - 1) : 0.0f; }

static BgGrid bg_grid(const float* grid, int Gx, int Gy, int L, int H, int W)
{
    BgGrid g; g.v = grid; g.Gx = Gx; g.Gy = Gy; g.L = L; g.sx = bg_scale(Gx, W); g.sy = bg_scale(Gy, H);
    return g;
}

// first[c] = the first x of [0, n) whose cell is >= c (n when none is), c = 0 .. G-1: cells are runs, the cell index being monotonic in x
static void bg_cells(int n, float scale, int G, int* first)
{
    first[0] = 0;
    first[G - 1] = n;
    for (int c = 1; c < G - 1; ++c) {
        int lo = first[c - 1], hi = n;                 // the answer lies in [lo, hi]
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            float t;
            if (bg_cell(mid, scale, G, &t) >= c) hi = mid; else lo = mid + 1;
        }
        first[c] = lo;
    }
}

static int bg_split(int Gx, int Gy) { const int s = GS_BILATERAL_TARGET_BLOCKS / (Gx * Gy); return s > 1 ? s : 1; }

size_t gs_bilateral_ws_size(int Gx, int Gy, int L)
{
    const int S = bg_split(Gx, Gy);
    return S > 1 ? (size_t)Gx * Gy * S * 12 * L * sizeof(float) : 0;
}

void gs_launch_bilateral_slice(const GsLossImage& X, const float* grid, int Gx, int Gy, int L, int H, int W, const GsLossImage& C, hipStream_t s)
{
    const int n = H * W;
    k_bilateral_slice<<<(n + BG_THREADS - 1) / BG_THREADS, BG_THREADS, 0, s>>>(bg_image(X), bg_image(C), bg_grid(grid, Gx, Gy, L, H, W), W, n);
}

template <int L>
static void bg_launch_gather(const BgImage& X, const BgImage& G, const BgGrid& g, const BgCells& cells, int S, float* out, hipStream_t s)
{
    k_bilateral_gather<L><<<g.Gx * g.Gy * S, BG_GATHER, 0, s>>>(X, G, g, cells, S, out);
}

void gs_launch_bilateral_backward(const GsLossImage& X, const GsLossImage& G, const float* grid, int Gx, int Gy, int L, int H, int W,
                                  const GsLossImage& GI, float* grad_grid, void* ws, hipStream_t s)
{
    const int n = H * W;
    const BgGrid g = bg_grid(grid, Gx, Gy, L, H, W);
    if (grad_grid) {
        // the gather first: it reads grad_corrected, which the image pass may overwrite in place
        BgCells cells;
        std::memset(&cells, 0, sizeof cells);
        bg_cells(W, g.sx, Gx, cells.xs);
        bg_cells(H, g.sy, Gy, cells.ys);
        const int S = bg_split(Gx, Gy);
        float* out = S > 1 ? static_cast<float*>(ws) : grad_grid;
        const BgImage x = bg_image(X), gc = bg_image(G);
        switch (L) {
        case 2: bg_launch_gather<2>(x, gc, g, cells, S, out, s); break;
        case 3: bg_launch_gather<3>(x, gc, g, cells, S, out, s); break;
        case 4: bg_launch_gather<4>(x, gc, g, cells, S, out, s); break;
        case 5: bg_launch_gather<5>(x, gc, g, cells, S, out, s); break;
        case 6: bg_launch_gather<6>(x, gc, g, cells, S, out, s); break;
        case 7: bg_launch_gather<7>(x, gc, g, cells, S, out, s); break;
        default: bg_launch_gather<8>(x, gc, g, cells, S, out, s); break;
        }
        if (S > 1) {
            const int ns = 12 * L, n_out = Gx * Gy * ns;
            k_bilateral_gather_finish<<<(n_out + 255) / 256, 256, 0, s>>>(out, S, ns, n_out, grad_grid);
        }
    }
    if (GI.p)
        k_bilateral_backward_image<<<(n + BG_THREADS - 1) / BG_THREADS, BG_THREADS, 0, s>>>(bg_image(X), bg_image(G), bg_image(GI), g, W, n);
}

void gs_launch_bilateral_tv(const float* grid, int Gx, int Gy, int L, float weight, float* grad_grid, float* value, hipStream_t s)
{
    const double cx = 12.0 * Gy * (Gx - 1) * L, cy = 12.0 * (Gy - 1) * Gx * L, cz = 12.0 * Gy * Gx * (L - 1);
    k_bilateral_tv<<<1, BG_TV, 0, s>>>(grid, Gx, Gy, L, weight, 2.0f / (float)cx, 2.0f / (float)cy, 2.0f / (float)cz, cx, cy, cz, grad_grid, value);
}
