// k_channels.hip -- per-Gaussian feature channels blended over a frame that gs_forward made (include/gs_channels.h).
//
//   out[y, x, c]         = sum_i w_i * values[id_i, c]             (k_channels_fwd)
//   grad_values[id, c]   = sum_pixels w_i(pixel) * grad_out[pixel, c]   (k_channels_bwd -> k_channels_sum)
//
// with w_i = alpha_i * T_i over the contributors of the pixel: the entries of its tile's sorted list before the pixel's
// pixel_offset_of_last_effective_point whose alpha reaches 1/255.  Geometry is frozen: only `values` carries a gradient.
//
// Both directions share ONE walk (gs_channel_walk): one wave per 8x8 quadrant, 64-entry batches, the gs_cull.h cull against the
// rectangle of the pixels whose `last` lies beyond the batch, records through a wave-private LDS slab, and per surviving splat
// the functions k_blend_fwd calls for alpha and the 0.99 clamp (gs_cull.h: gs_splat_alpha, gs_alpha_clamp), its 1/255 test, w and T -- so the
// contributor set, and every w, is the forward's own, bit for bit.  No saturation test: `last` ends a pixel's list before the entry that saturated it.
//
// Channels are processed CH at a time (gs_channels_chunk: 4, 16 or 32).  The forward keeps CH accumulators per lane (pixel) and
// reads the splat's value row, gathered by the lane that gathered its record, as LDS broadcasts; chunks are grid.y.
//
// The backward is a small matrix product per wave: W (pixels x splats) times grad_out (pixels x channels).  The walk has the
// pixels on the lanes and stores each contributing splat's w as a COLUMN of an LDS matrix; after GS_CH_COLS columns the wave
// turns round -- splats (and channel quarters) on the lanes -- and every lane sums its column against the quadrant's grad_out
// rows (LDS broadcasts) over the 64 pixels in pixel order, then stores its part of the splat's partial row itself: no
// cross-lane reduction per channel, no atomics, a fixed order of additions.  Partial rows sit at the pair's pre-sort slot
// (offsets[p] + position of the tile in the point's box), four per pair (one per quadrant); k_channels_sum adds a point's
// flagged rows in slot order.  Two runs therefore give the same bits.
#include "gs_common.h"
#include "gs_cull.h"

#define GS_CH_COLS 16                         // columns of W a wave gathers before it sums them (64 / GS_CH_COLS channel groups)
#define GS_CH_WSTRIDE (GS_CH_COLS + 1)        // row stride of W in LDS: odd, so that the walk's column stores are conflict-free

// The walk of one quadrant.  lim: this lane's (pixel's) end of list, in [start, end]; a pixel outside the image has lim = start.
// op.gather(keep, p): per batch, lane-wise, for the record this lane fetched; op.splat(j, use, w): per surviving splat, batch
// position j (wave-uniform), use / w lane-wise (w = 0 where the pixel takes nothing).
template <typename Op>
__device__ __forceinline__ void gs_channel_walk(int start, int lim, const GsQuadPixel& qp, int lane,
                                                const int32_t* __restrict__ sorted_vals, const float4* __restrict__ PA,
                                                const float4* __restrict__ PB, const float4* __restrict__ PC,
                                                float4 (*sRec)[2], Op& op)
{
    const int lim_max = gs_wave_max_i(lim);
    float T_i = 1.0f;
    for (int base = start; base < lim_max; base += 64) {
        const unsigned long long live = gs_ballot(lim > base);      // pixels that can still take a contribution (never empty here)
        const int i = base + lane;
        const bool valid = i < lim_max;
        const int p = valid ? sorted_vals[i] : 0;
        const float4 A = GS_REC(PA, p), B = GS_REC(PB, p), C = GS_REC(PC, p);
        const CullRect lr = gs_live_rect(live, qp.rx0, qp.ry0);
        const bool keep = valid && !gs_cull(gs_cull_prepare(A, B, C), lr.x0, lr.y0, lr.wx, lr.wy);
        unsigned long long mask = gs_ballot(keep);
        if (mask == 0ull) continue;
        sRec[lane][0] = A; sRec[lane][1] = B;
        op.gather(keep, p);
        __builtin_amdgcn_wave_barrier();
        while (mask) {
            const int j = __builtin_ctzll(mask);
            mask &= mask - 1ull;
            const float4 a4 = sRec[j][0], b4 = sRec[j][1];
            // alpha and the clamp are the forward's own functions; the 1/255 test, w and T as in its GS_FWD_STEP
            float alpha = gs_splat_alpha(qp.px, qp.py, a4, b4);
            const bool use = !(alpha < GS_ALPHA_EPS) && base + j < lim;
            alpha = gs_alpha_clamp(alpha);
            const float w = use ? alpha * T_i : 0.0f;
            T_i = use ? T_i * (1.0f - alpha) : T_i;
            op.splat(j, use, w);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- forward ----------------------------------------------------------------------------------------------------------
template <int CH>
struct GsChannelFwdOp {
    const int32_t* __restrict__ ids; const float* __restrict__ values; int C, c0, lane;
    float (*sVal)[CH];
    float acc[CH];
    __device__ __forceinline__ void gather(bool keep, int p)
    {
        if (!keep) return;                      // rows of culled splats (and of points outside the camera) are never read
        const float* row = values + (size_t)ids[p] * (size_t)C + c0;
#pragma unroll
        for (int c = 0; c < CH; ++c) sVal[lane][c] = c0 + c < C ? row[c] : 0.0f;
    }
    __device__ __forceinline__ void splat(int j, bool use, float w)
    {
        if (use) {
#pragma unroll
            for (int c = 0; c < CH; ++c) acc[c] = __builtin_fmaf(sVal[j][c], w, acc[c]);
        }
    }
};

template <int CH>
__global__ __launch_bounds__(256) void k_channels_fwd(const int32_t* __restrict__ tile_start, const int32_t* __restrict__ tile_end,
                                                      const int32_t* __restrict__ sorted_vals, const float4* __restrict__ PA,
                                                      const float4* __restrict__ PB, const float4* __restrict__ PC,
                                                      const int32_t* __restrict__ ids, const int32_t* __restrict__ last,
                                                      const float* __restrict__ values, int C, int W, int H, int tiles_x,
                                                      float* __restrict__ out)
{
    __shared__ float4 sRec[4][64][2];
    __shared__ __attribute__((aligned(16))) float sVal[4][64][CH];
    const int tile = (int)blockIdx.x, c0 = (int)blockIdx.y * CH;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const GsQuadPixel qp = gs_quad_pixel(tile, wave, lane, tiles_x, W, H);
    const int start = tile_start[tile], end = tile_end[tile];
    const int lim = gs_clamp_last(qp.inside ? last[qp.o] : start, start, end);
    GsChannelFwdOp<CH> op;
    op.ids = ids; op.values = values; op.C = C; op.c0 = c0; op.lane = lane; op.sVal = sVal[wave];
#pragma unroll
    for (int c = 0; c < CH; ++c) op.acc[c] = 0.0f;
    gs_channel_walk(start, lim, qp, lane, sorted_vals, PA, PB, PC, sRec[wave], op);
    if (!qp.inside) return;
    float* dst = out + qp.o * (size_t)C + c0;
#pragma unroll
    for (int c = 0; c < CH; ++c)
        if (c0 + c < C) dst[c] = op.acc[c];
}

// ---- backward -----------------------------------------------------------------------------------------------------------
template <int CH>
struct GsChannelBwdOp {
    static constexpr int CPL = CH / (64 / GS_CH_COLS);      // channels per lane when the wave sums its columns
    const ushort4* __restrict__ box; const uint32_t* __restrict__ offsets;
    float* __restrict__ partial; uint8_t* __restrict__ flags; uint8_t* __restrict__ touched;
    uint32_t K; int tile_u, tile_v, quad, lane;
    float* sW; float (*sG)[CH];
    int cnt;                    // columns gathered so far (wave-uniform)
    uint32_t slot; int point;   // of the record this lane fetched in the current batch
    uint32_t col_slot; int col_point;   // of column (lane % GS_CH_COLS)

    __device__ __forceinline__ void gather(bool keep, int p)
    {
        slot = 0xffffffffu; point = p;
        if (!keep) return;
        const ushort4 bx = box[p];              // pre-sort slot of this (point, tile) pair, as in k_blend_bwd_tile
        slot = offsets[p] + (uint32_t)(((int)bx.w - (int)bx.z) * (tile_u - (int)bx.x) + (tile_v - (int)bx.z));
    }
    __device__ __forceinline__ void splat(int j, bool use, float w)
    {
        if (gs_ballot(use) == 0ull) return;     // no pixel of the quadrant takes anything from it: no column, no row
        sW[lane * GS_CH_WSTRIDE + cnt] = w;
        const uint32_t sj = (uint32_t)__builtin_amdgcn_readlane((int)slot, j);
        const int pj = __builtin_amdgcn_readlane(point, j);
        if ((lane & (GS_CH_COLS - 1)) == cnt) { col_slot = sj; col_point = pj; }
        cnt += 1;
        if (cnt == GS_CH_COLS) flush();
    }
    // lane = (column r, channel group h): sum_pixels W[pixel][r] * G[pixel][h * CPL ...], pixels in order 0..63
    __device__ __forceinline__ void flush()
    {
        __builtin_amdgcn_wave_barrier();
        const int r = lane & (GS_CH_COLS - 1), h = lane / GS_CH_COLS;
        float acc[CPL];
#pragma unroll
        for (int c = 0; c < CPL; ++c) acc[c] = 0.0f;
        for (int pix = 0; pix < 64; ++pix) {
            const float wv = sW[pix * GS_CH_WSTRIDE + r];
#pragma unroll
            for (int c = 0; c < CPL; ++c) acc[c] = __builtin_fmaf(wv, sG[pix][h * CPL + c], acc[c]);
        }
        if (r < cnt && col_slot < K) {
            const size_t row = (size_t)col_slot * 4 + (size_t)quad;
            float* dst = partial + row * CH + h * CPL;
#pragma unroll
            for (int c = 0; c < CPL; ++c) dst[c] = acc[c];
            if (h == 0) { flags[row] = 1; touched[col_point] = 1; }
        }
        cnt = 0;
        __builtin_amdgcn_wave_barrier();
    }
};

// one wave (= one workgroup) per quadrant: blockIdx.x = 4 * tile + quadrant
template <int CH>
__global__ __launch_bounds__(64) void k_channels_bwd(const int32_t* __restrict__ tile_start, const int32_t* __restrict__ tile_end,
                                                     const int32_t* __restrict__ sorted_vals, const float4* __restrict__ PA,
                                                     const float4* __restrict__ PB, const float4* __restrict__ PC,
                                                     const ushort4* __restrict__ box, const uint32_t* __restrict__ offsets, uint32_t K,
                                                     const int32_t* __restrict__ last, const float* __restrict__ grad_out, int C, int c0,
                                                     int W, int H, int tiles_x, float* __restrict__ partial,
                                                     uint8_t* __restrict__ flags, uint8_t* __restrict__ touched)
{
    __shared__ float4 sRec[64][2];
    __shared__ float sW[64 * GS_CH_WSTRIDE];
    __shared__ __attribute__((aligned(16))) float sG[64][CH];
    const int tile = (int)(blockIdx.x >> 2), quad = (int)(blockIdx.x & 3u);
    const int lane = threadIdx.x;
    const GsQuadPixel qp = gs_quad_pixel(tile, quad, lane, tiles_x, W, H);
    const int start = tile_start[tile], end = tile_end[tile];
    const int lim = gs_clamp_last(qp.inside ? last[qp.o] : start, start, end);
    if (gs_ballot(lim > start) == 0ull) return;             // nothing was blended into this quadrant
#pragma unroll
    for (int c = 0; c < CH; ++c) sG[lane][c] = (qp.inside && c0 + c < C) ? grad_out[qp.o * (size_t)C + c0 + c] : 0.0f;
    GsChannelBwdOp<CH> op;
    op.box = box; op.offsets = offsets; op.partial = partial; op.flags = flags; op.touched = touched;
    op.K = K; op.tile_u = qp.tile_u; op.tile_v = qp.tile_v; op.quad = quad; op.lane = lane;
    op.sW = sW; op.sG = sG; op.cnt = 0; op.slot = 0xffffffffu; op.point = 0; op.col_slot = 0xffffffffu; op.col_point = 0;
    __builtin_amdgcn_wave_barrier();
    gs_channel_walk(start, lim, qp, lane, sorted_vals, PA, PB, PC, sRec, op);
    if (op.cnt > 0) op.flush();
}

// One wave per in-camera point: its 4 * ntiles partial rows in slot order, 64 / CH rows side by side (lane = row group * CH +
// channel), the groups then folded by a fixed butterfly.  Which rows exist and in which order they are added depends on the
// point's tile count alone.  A point no pixel took anything from writes zeros without looking at a row.
template <int CH>
__global__ __launch_bounds__(256) void k_channels_sum(int M, const uint32_t* __restrict__ offsets, const int32_t* __restrict__ ntiles,
                                                      const int32_t* __restrict__ ids, const float* __restrict__ partial,
                                                      const uint8_t* __restrict__ flags, const uint8_t* __restrict__ touched,
                                                      int C, int c0, float* __restrict__ grad_values)
{
    constexpr int NG = 64 / CH;
    const int wave = (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int m = (int)blockIdx.x * 4 + wave;
    if (m >= M) return;                                      // (wave-uniform)
    const int g = lane / CH, c = lane % CH;
    float v = 0.0f;
    if (touched[m]) {                                        // (wave-uniform)
        const size_t off = (size_t)offsets[m] * 4;
        const int cnt = ntiles[m] * 4;
        for (int i = g; i < cnt; i += NG)
            if (flags[off + i]) v += partial[(off + i) * CH + c];
#pragma unroll
        for (int d = CH; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    }
    if (g == 0 && c0 + c < C) grad_values[(size_t)ids[m] * (size_t)C + c0 + c] = v;
}

// ---- launches -----------------------------------------------------------------------------------------------------------
int gs_channels_chunk(int C)
{
    return C <= 4 ? 4 : (C <= 16 ? 16 : 32);
}

template <int CH>
static void channels_fwd(const GsChannelsArgs& a, hipStream_t s)
{
    const GsFrameView& v = a.v;
    const dim3 grid((unsigned)v.T, (unsigned)((a.C + CH - 1) / CH));
    k_channels_fwd<CH><<<grid, 256, 0, s>>>(v.tile_start, v.tile_end, v.vals_sorted, v.PA, v.PB, v.PC, v.ids, a.last, a.values, a.C,
                                            a.W, a.H, a.tiles_x, a.out);
}

void gs_launch_channels_fwd(const GsChannelsArgs& a, hipStream_t s)
{
    if (a.v.T <= 0) return;
    switch (gs_channels_chunk(a.C)) {
    case 4: channels_fwd<4>(a, s); break;
    case 16: channels_fwd<16>(a, s); break;
    default: channels_fwd<32>(a, s); break;
    }
}

// one chunk after the other through the same scratch: flags cleared, blend, per-point sum
template <int CH>
static hipError_t channels_bwd(const GsChannelsArgs& a, hipStream_t s)
{
    const GsFrameView& v = a.v;
    for (int c0 = 0; c0 < a.C; c0 += CH) {
        const hipError_t e = hipMemsetAsync(a.flags, 0, a.flag_bytes, s);
        if (e != hipSuccess) return e;
        k_channels_bwd<CH><<<(unsigned)v.T * 4u, 64, 0, s>>>(v.tile_start, v.tile_end, v.vals_sorted, v.PA, v.PB, v.PC, v.box, v.offsets, a.K,
                                                            a.last, a.grad_out, a.C, c0, a.W, a.H, a.tiles_x, a.partial, a.flags, a.touched);
        k_channels_sum<CH><<<(unsigned)((a.M + 3) / 4), 256, 0, s>>>(a.M, v.offsets, v.ntiles, v.ids, a.partial, a.flags, a.touched,
                                                                    a.C, c0, a.grad_values);
    }
    return hipSuccess;
}

hipError_t gs_launch_channels_bwd(const GsChannelsArgs& a, hipStream_t s)
{
    if (a.v.T <= 0 || a.M <= 0) return hipSuccess;
    switch (gs_channels_chunk(a.C)) {
    case 4: return channels_bwd<4>(a, s);
    case 16: return channels_bwd<16>(a, s);
    default: return channels_bwd<32>(a, s);
    }
}
