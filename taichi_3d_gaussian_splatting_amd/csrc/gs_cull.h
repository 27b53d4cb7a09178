// gs_cull.h -- what the kernels that walk a tile's list per 8x8 quadrant share (k_blend_fwd, k_channels, k_backward): the
// quadrant's pixels (GsQuadPixel), one blend step's alpha (gs_splat_alpha, gs_alpha_clamp) and the conservative cull.
//
// A splat is dropped for an 8x8 pixel quadrant only when alpha = exp(e) * rescale * opacity is
// certainly below 1/255 at every pixel centre of the quadrant, i.e. when the reference's own test
// (RAST:451-452 forward, RAST:634 backward) would skip it for all 64 pixels.  The bound is the exact
// maximum of the Gaussian exponent over the quadrant's rectangle (minimum of the conic quadratic
// over the four edges), compared in the log domain with a slack that covers every rounding error
// of the per-pixel f32 evaluation.  Culling therefore never changes a result.
#pragma once
#include "gs_common.h"

// min over the rectangle [X0,X1]x[Y0,Y1] (pixel centre minus mean) of q = a x^2 + 2 b x y + c y^2, for a,c > 0.
// nb_c = -b/c and nb_a = -b/a are precomputed per splat (approximate reciprocals are fine: the
// caller adds a slack that dwarfs their error).
__device__ __forceinline__ float gs_rect_min_quadratic(float a, float b, float c, float nb_c, float nb_a,
                                                      float X0, float X1, float Y0, float Y1)
{
    if (X0 <= 0.0f && X1 >= 0.0f && Y0 <= 0.0f && Y1 >= 0.0f) return 0.0f;
    float best;
    {
        float y = __builtin_amdgcn_fmed3f(nb_c * X0, Y0, Y1);
        best = X0 * (a * X0 + 2.0f * b * y) + c * y * y;
        y = __builtin_amdgcn_fmed3f(nb_c * X1, Y0, Y1);
        best = fminf(best, X1 * (a * X1 + 2.0f * b * y) + c * y * y);
        float x = __builtin_amdgcn_fmed3f(nb_a * Y0, X0, X1);
        best = fminf(best, Y0 * (c * Y0 + 2.0f * b * x) + a * x * x);
        x = __builtin_amdgcn_fmed3f(nb_a * Y1, X0, X1);
        best = fminf(best, Y1 * (c * Y1 + 2.0f * b * x) + a * x * x);
    }
    return best;
}

struct CullSplat { float u, v, a, b, c, nb_c, nb_a, cut, sa, sb, sc; bool pd; };

__device__ __forceinline__ CullSplat gs_cull_prepare(float4 A, float4 B, float4 C)
{
    CullSplat s;
    s.u = A.x; s.v = A.y; s.a = A.z; s.b = A.w; s.c = B.x; s.cut = C.w;
    s.pd = s.a > 0.0f && s.c > 0.0f && s.a * s.c > s.b * s.b;
    s.nb_c = -s.b * __builtin_amdgcn_rcpf(s.c);
    s.nb_a = -s.b * __builtin_amdgcn_rcpf(s.a);
    s.sa = 4.0e-6f * fabsf(s.a); s.sb = 8.0e-6f * fabsf(s.b); s.sc = 4.0e-6f * fabsf(s.c);
    return s;
}

// The rectangle of an 8x8 quadrant's pixels that are still of interest (wave-uniform, from a 64-bit lane mask with
// lane = 8 * row + column): first column / row and extent in pixels.  A splat only has to be kept if it can reach
// 1/255 at one of THOSE pixels -- the others have saturated (forward) or lie beyond their last contributor (backward)
// and take nothing from it -- so the cull rectangle shrinks with the mask and the late part of a walk, where a few
// pixels keep a wave going, evaluates a fraction of the splats.  Exactly as invisible in the results as the quadrant cull.
struct CullRect { float x0, y0, wx, wy; };
__device__ __forceinline__ CullRect gs_live_rect(unsigned long long mask, float qx0, float qy0)
{
    // rows: which bytes of the mask are non-zero; columns: the OR of the eight bytes
    const int ymin = __builtin_ctzll(mask) >> 3, ymax = (63 - __builtin_clzll(mask)) >> 3;
    uint32_t c = (uint32_t)mask | (uint32_t)(mask >> 32);
    c |= c >> 16; c |= c >> 8; c &= 0xffu;
    const int xmin = __builtin_ctz(c), xmax = 31 - __builtin_clz(c);
    CullRect r;
    r.x0 = qx0 + (float)xmin; r.y0 = qy0 + (float)ymin; r.wx = (float)(xmax - xmin); r.wy = (float)(ymax - ymin);
    return r;
}

// true when the splat cannot reach alpha >= 1/255 anywhere in the rectangle of pixel centres [rx0, rx0 + wx] x [ry0, ry0 + wy]
// (wx = wy = 7: a whole 8x8 quadrant whose first pixel centre is (rx0, ry0)).  Any NaN makes the test false (= keep the splat).
__device__ __forceinline__ bool gs_cull(const CullSplat& s, float rx0, float ry0, float wx = 7.0f, float wy = 7.0f)
{
    const float X0 = rx0 - s.u, X1 = X0 + wx, Y0 = ry0 - s.v, Y1 = Y0 + wy;
    const float ax = fmaxf(fabsf(X0), fabsf(X1)), ay = fmaxf(fabsf(Y0), fabsf(Y1));
    // rounding slack of the f32 exponent evaluated per pixel (terms can cancel for skewed conics)
    const float slack = 0.02f + (s.sa * ax * ax + s.sc * ay * ay + s.sb * ax * ay);
    const float qmin = gs_rect_min_quadratic(s.a, s.b, s.c, s.nb_c, s.nb_a, X0, X1, Y0, Y1);
    return s.pd && (-0.5f * qmin + slack < s.cut);
}

// One lane's pixel of an 8x8 quadrant (quadrant bit 0 = right half of the 16x16 tile, bit 1 = lower half; lane = 8 * row + column).
// A pixel of a partial edge tile that lies outside the image does not exist (extension; W, H % 16 == 0 in the reference): !inside.
struct GsQuadPixel {
    int tile_u, tile_v, qx, qy, pixel_u, pixel_v;   // the tile, the quadrant's first pixel, this lane's pixel
    bool inside; size_t o;                          // o = pixel_v * W + pixel_u (an address only when inside)
    float px, py, rx0, ry0;                         // pixel centre; centre of the quadrant's first pixel (origin of the cull rectangle)
};
__device__ __forceinline__ GsQuadPixel gs_quad_pixel(int tile, int quadrant, int lane, int tiles_x, int W, int H)
{
    GsQuadPixel q;
    q.tile_u = tile % tiles_x; q.tile_v = tile / tiles_x;
    q.qx = q.tile_u * 16 + (quadrant & 1) * 8; q.qy = q.tile_v * 16 + (quadrant >> 1) * 8;
    q.pixel_u = q.qx + (lane & 7); q.pixel_v = q.qy + (lane >> 3);
    q.inside = q.pixel_u < W && q.pixel_v < H; q.o = (size_t)q.pixel_v * (size_t)W + (size_t)q.pixel_u;
    q.px = (float)q.pixel_u + 0.5f; q.py = (float)q.pixel_v + 0.5f; q.rx0 = (float)q.qx + 0.5f; q.ry0 = (float)q.qy + 0.5f;
    return q;
}
// a pixel's pixel_offset_of_last_effective_point as the end of its walk: inside the tile's range whatever the caller passed
__device__ __forceinline__ int gs_clamp_last(int last, int start, int end) { return last < start ? start : (last > end ? end : last); }

// alpha of splat (a4 = {u, v, conic a, conic b}, b4 = {conic c, rescale, opacity, depth}) at pixel centre (px, py), before the clamp, in two
// halves: the exponent, get_point_probability_density_from_conic_and_rescale UTIL:275-284 (same op order), and exp(e) * rescale * opacity
// (RAST:449-450).  k_blend_fwd calls the halves itself, for two splats side by side as in its schedule; gs_splat_alpha is the two in a row.
__device__ __forceinline__ float gs_splat_exponent(float px, float py, float4 a4, float4 b4)
{
    const float dx = px - a4.x, dy = py - a4.y;
    return -0.5f * (dx * dx * a4.z + dy * dy * b4.x) - dx * dy * a4.w;
}
__device__ __forceinline__ float gs_alpha_of_exponent(float e, float4 b4) { return gs_exp_blend(e) * b4.y * b4.z; }
__device__ __forceinline__ float gs_splat_alpha(float px, float py, float4 a4, float4 b4) { return gs_alpha_of_exponent(gs_splat_exponent(px, py, a4, b4), b4); }
// min(alpha, 0.99), RAST:453, as the UNSIGNED minimum of the bit patterns: one instruction (the float form costs a canonicalising
// v_max first).  Same value for every alpha >= 0; a NaN of either sign gives 0.99 like the compare-and-select of the oracle; a
// negative alpha (never blended: it fails the 1/255 test) may come out as 0.99.
// (gs_clamp_alpha of k_backward.hip is not this one: it clamps a product known to be positive, with the SIGNED minimum.)
__device__ __forceinline__ float gs_alpha_clamp(float alpha) { return __uint_as_float(min(__float_as_uint(alpha), __float_as_uint(GS_ALPHA_MAX))); }
