// k_targets.hip -- the training target of one view (include/gs_targets.h): antialiased bilinear down-resize of a resident
// uint8 HWC (or f32 CHW) image and its top-left crop, f32 CHW out, in one launch.
//
// A workgroup of 256 threads owns a TILE_H x TILE_W output tile.  It walks the input rows the tile reads in chunks of
// CHUNK_ROWS:
//   stage     (uint8 only) the bytes of the chunk's rows that the tile's columns read go to LDS as they lie, by 16-byte loads
//             of the aligned 16-byte slots that cover them; a slot that is not wholly inside the image buffer (only possible
//             at its very first and last bytes) is read byte by byte.  A row keeps its address modulo 16 in LDS, so any pitch
//             and any base alignment take the same path.
//   rows      horizontal pass: one thread per (chunk row, tile column), three channels, fmaf chain in ascending input column;
//             uint8 -> (float)v / 255.0f first.  The result stays in LDS as f32 [row][channel][column].
//   columns   vertical pass: one thread per (tile row, four columns), three float4 accumulators that live across the chunks;
//             the taps that fall into this chunk are added in ascending input row (ds_read_b128).
// and ends in one 16-byte store per channel plane and thread (scalar stores where w_out or dst do not allow it).
// Static LDS: 33792 (staged bytes) + 12288 (f32 rows) + 5760 (the tile's weights) + 640 (its windows) = 52480 bytes at any
// scale; the f32 source stages nothing and uses 18704.
// NC = 4 (gs_image_resample_rgba, include/gs_targets_rgba.h): channel 3 of a four-channel source runs through the same two
// passes into plane 3 -- one more fmaf chain per pass and one more plane of stores; the f32 rows take 16384 bytes then.
#include "gs_common.h"
#include "../../include/gs_targets.h"

#define RS_TILE_H GS_RESAMPLE_TILE_H
#define RS_TILE_W GS_RESAMPLE_TILE_W
#define RS_THREADS 256
#define RS_CHUNK_ROWS 16
// bytes of one staged row: GS_RS_MAX_SPAN pixels of 4 channels behind an offset of up to 15, in whole 16-byte slots
#define RS_RAW_PITCH ((GS_RS_MAX_SPAN * 4 + 15 + 15) / 16 * 16)
static_assert(RS_TILE_W % 4 == 0 && RS_TILE_H * (RS_TILE_W / 4) == RS_THREADS, "one thread per tile row and four columns");
static_assert(RS_THREADS % RS_TILE_W == 0 && RS_CHUNK_ROWS % (RS_THREADS / RS_TILE_W) == 0, "the horizontal pass covers a chunk in whole rounds");

template <bool U8, int NC>
__global__ __launch_bounds__(RS_THREADS) void k_image_resample(const uint8_t* __restrict__ src, int C, int H_in, int W_in, int64_t pitch,
                                                              GsResampleAxis ax, GsResampleAxis ay, int h_out, int w_out,
                                                              float* __restrict__ dst, int vec_store)
{
    __shared__ __align__(16) float hbuf[RS_CHUNK_ROWS][NC][RS_TILE_W];
    __shared__ __align__(16) uint8_t raw[U8 ? RS_CHUNK_ROWS * RS_RAW_PITCH : 16];
    __shared__ float wx[RS_TILE_W * GS_RS_MAX_TAPS], wy[RS_TILE_H * GS_RS_MAX_TAPS];
    __shared__ int sx[RS_TILE_W], cx[RS_TILE_W], sy[RS_TILE_H], cy[RS_TILE_H];

    const int t = threadIdx.x;
    const int tx0 = blockIdx.x * RS_TILE_W, ty0 = blockIdx.y * RS_TILE_H;
    // the tile's windows and weights; columns / rows past the crop get an empty window
    if (t < RS_TILE_W) {
        const int x = tx0 + t;
        const int n = x < w_out ? min(ax.count[x], GS_RS_MAX_TAPS) : 0;
        sx[t] = x < w_out ? ax.start[x] : 0; cx[t] = n;
        for (int k = 0; k < n; ++k) wx[t * GS_RS_MAX_TAPS + k] = ax.weight[(size_t)x * ax.taps + k];
    } else if (t < RS_TILE_W + RS_TILE_H) {
        const int i = t - RS_TILE_W, y = ty0 + i;
        const int n = y < h_out ? min(ay.count[y], GS_RS_MAX_TAPS) : 0;
        sy[i] = y < h_out ? ay.start[y] : 0; cy[i] = n;
        for (int k = 0; k < n; ++k) wy[i * GS_RS_MAX_TAPS + k] = ay.weight[(size_t)y * ay.taps + k];
    }
    __syncthreads();
    const int x_last = min(RS_TILE_W, w_out - tx0) - 1, y_last = min(RS_TILE_H, h_out - ty0) - 1;
    const int px0 = sx[0], px1 = min(sx[x_last] + cx[x_last], W_in);      // input columns [px0, px1) and
    const int R0 = sy[0], R1 = min(sy[y_last] + cy[y_last], H_in);        // rows [R0, R1) the tile reads
    const int span_bytes = (px1 - px0) * C;
    const int slots = (span_bytes + 15 + 15) / 16;                        // 16-byte slots of a row at the worst offset
    const uintptr_t buf_begin = (uintptr_t)src, buf_end = buf_begin + (uintptr_t)(H_in - 1) * (uintptr_t)pitch + (uintptr_t)W_in * C;

    const int vy = t / (RS_TILE_W / 4), vg = t % (RS_TILE_W / 4);       // vertical pass: tile row, group of four columns
    const int hx = t % RS_TILE_W, hr0 = t / RS_TILE_W;                     // horizontal pass: tile column, first chunk row
    float4 acc[NC];
    for (int c = 0; c < NC; ++c) acc[c] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);

    for (int r0 = R0; r0 < R1; r0 += RS_CHUNK_ROWS) {
        const int n_rows = min(RS_CHUNK_ROWS, R1 - r0);
        if constexpr (U8) {
            for (int item = t; item < n_rows * slots; item += RS_THREADS) {
                const int rr = item / slots, s = item % slots;
                const uintptr_t a = buf_begin + (uintptr_t)(r0 + rr) * (uintptr_t)pitch + (uintptr_t)px0 * C, e = a + span_bytes;
                const uintptr_t sa = (a & ~(uintptr_t)15) + 16u * (uintptr_t)s;
                if (sa >= e || 16 * s + 16 > RS_RAW_PITCH) continue;
                uint8_t* out = &raw[rr * RS_RAW_PITCH + 16 * s];
                if (sa >= buf_begin && sa + 16 <= buf_end) {
                    *reinterpret_cast<uint4*>(out) = *reinterpret_cast<const uint4*>(sa);
                } else {
                    for (int b = 0; b < 16; ++b)
                        if (sa + b >= a && sa + b < e) out[b] = *reinterpret_cast<const uint8_t*>(sa + b);
                }
            }
            __syncthreads();
        }
        // horizontal pass of the chunk's rows
        for (int rr = hr0; rr < RS_CHUNK_ROWS; rr += RS_THREADS / RS_TILE_W) {
            float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f, h3 = 0.0f;
            if (rr < n_rows) {
                const int n = cx[hx];
                const float* w = &wx[hx * GS_RS_MAX_TAPS];
                if constexpr (U8) {
                    const uintptr_t a = buf_begin + (uintptr_t)(r0 + rr) * (uintptr_t)pitch + (uintptr_t)px0 * C;
                    const uint8_t* p = &raw[rr * RS_RAW_PITCH + (int)(a & 15) + (sx[hx] - px0) * C];
                    for (int k = 0; k < n; ++k, p += C) {
                        h0 = fmaf(w[k], (float)p[0] / 255.0f, h0);
                        h1 = fmaf(w[k], (float)p[1] / 255.0f, h1);
                        h2 = fmaf(w[k], (float)p[2] / 255.0f, h2);
                        if constexpr (NC == 4) h3 = fmaf(w[k], (float)p[3] / 255.0f, h3);
                    }
                } else {
                    const size_t plane = (size_t)H_in * W_in;
                    const float* p = reinterpret_cast<const float*>(src) + (size_t)(r0 + rr) * W_in + sx[hx];
                    for (int k = 0; k < n; ++k) {
                        h0 = fmaf(w[k], p[k], h0);
                        h1 = fmaf(w[k], p[plane + k], h1);
                        h2 = fmaf(w[k], p[2 * plane + k], h2);
                        if constexpr (NC == 4) h3 = fmaf(w[k], p[3 * plane + k], h3);
                    }
                }
            }
            hbuf[rr][0][hx] = h0; hbuf[rr][1][hx] = h1; hbuf[rr][2][hx] = h2;
            if constexpr (NC == 4) hbuf[rr][3][hx] = h3;
        }
        __syncthreads();
        // vertical pass: the taps of this thread's output row that lie in the chunk
        {
            const int first = sy[vy], n = cy[vy];
            const int k0 = max(0, r0 - first), k1 = min(n, r0 + n_rows - first);
            for (int k = k0; k < k1; ++k) {
                const float w = wy[vy * GS_RS_MAX_TAPS + k];
                const int rr = first + k - r0;
                for (int c = 0; c < NC; ++c) {
                    const float4 h = *reinterpret_cast<const float4*>(&hbuf[rr][c][4 * vg]);
                    acc[c].x = fmaf(w, h.x, acc[c].x); acc[c].y = fmaf(w, h.y, acc[c].y);
                    acc[c].z = fmaf(w, h.z, acc[c].z); acc[c].w = fmaf(w, h.w, acc[c].w);
                }
            }
        }
        __syncthreads();        // the next chunk overwrites both buffers
    }

    const int oy = ty0 + vy, ox = tx0 + 4 * vg;
    if (oy >= h_out || ox >= w_out) return;
    for (int c = 0; c < NC; ++c) {
        float* d = dst + ((size_t)c * h_out + oy) * w_out + ox;
        if (vec_store && ox + 3 < w_out) {
            *reinterpret_cast<float4*>(d) = acc[c];
        } else {
            const float v[4] = { acc[c].x, acc[c].y, acc[c].z, acc[c].w };
            for (int j = 0; j < 4; ++j) if (ox + j < w_out) d[j] = v[j];
        }
    }
}

void gs_launch_image_resample(const void* src, int src_format, int channels, int H_in, int W_in, int64_t pitch_bytes, GsResampleAxis ax,
                              GsResampleAxis ay, int h_out, int w_out, float* dst, int dst_channels, hipStream_t s)
{
    const dim3 grid((w_out + RS_TILE_W - 1) / RS_TILE_W, (h_out + RS_TILE_H - 1) / RS_TILE_H);
    const int vec_store = (w_out % 4 == 0 && ((uintptr_t)dst & 15) == 0) ? 1 : 0;
    const uint8_t* p = reinterpret_cast<const uint8_t*>(src);
#define RS_LAUNCH(U8_, NC_) hipLaunchKernelGGL((k_image_resample<U8_, NC_>), grid, dim3(RS_THREADS), 0, s, p, channels, H_in, W_in, pitch_bytes, ax, ay, h_out, w_out, dst, vec_store)
    if (dst_channels == 4) {
        if (src_format == GS_IMAGE_U8_HWC) RS_LAUNCH(true, 4); else RS_LAUNCH(false, 4);
    } else {
        if (src_format == GS_IMAGE_U8_HWC) RS_LAUNCH(true, 3); else RS_LAUNCH(false, 3);
    }
#undef RS_LAUNCH
}
