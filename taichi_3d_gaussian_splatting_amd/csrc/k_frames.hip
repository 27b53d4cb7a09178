// k_frames.hip -- a rendered frame as the uint8 image that leaves the device (include/gs_frames.h): f32 (h,w,3) colour or (h,w)
// depth in, uint8 (h,w,3) with a row pitch out, and optionally the exact sum of squared differences against resident bytes.
//
// An item is 16 consecutive bytes of one output row; a row has ceil(3w / 16) items and thread i of the grid owns item i of the
// frame (row-major).  The fast case -- a whole item, w % 4 == 0 and a 16-byte aligned src (every row of 3w floats then starts
// on a 16-byte boundary), dst and pitch 16-byte aligned -- is four 16-byte loads and one 16-byte store; everything else goes
// float by float and byte by byte with the same arithmetic.  The ground truth is read the same way (16-byte load for a dense
// aligned 3-channel row).  Squared differences are summed as uint32 per thread (<= 16 * 65025), per wave by shuffles, per
// workgroup through LDS (<= 4096 * 65025 < 2^32), and added to the 64-bit word by one integer atomic per workgroup.
#include "gs_common.h"
#include "../../include/gs_frames.h"

#define FR_THREADS 256
#define FR_ITEM GS_FRAME_BYTES_PER_THREAD

__device__ __forceinline__ uint32_t fr_trunc(float v)
{
    // fmaxf(NaN, 0) = 0: NaN gives 0; +inf * 255 = inf -> 255
    return (uint32_t)fminf(fmaxf(v * 255.0f, 0.0f), 255.0f);
}
__device__ __forceinline__ uint32_t fr_round(float v)
{
    return (uint32_t)fminf(fmaxf(floorf(v * 255.0f + 0.5f), 0.0f), 255.0f);
}
// channel c of _easy_cmap(d): NaN stays NaN through min/max written as comparisons, and ends as 0 in fr_trunc
__device__ __forceinline__ float fr_cmap(float d, int c)
{
    const float off = c == 0 ? 0.0f : (c == 1 ? 10.0f : 60.0f), range = c == 0 ? 10.0f : (c == 1 ? 50.0f : 200.0f);
    float x = c == 0 ? d : d - off;
    x = x < 0.0f ? 0.0f : (x > range ? range : x);
    return 1.0f - x / range;
}

template <int MODE>
__device__ __forceinline__ uint32_t fr_byte(const float* __restrict__ src, int64_t row, int w, int b)
{
    if constexpr (MODE == GS_FRAME_DEPTH_CMAP) return fr_trunc(fr_cmap(src[row * w + b / 3], b % 3));
    else if constexpr (MODE == GS_FRAME_RGB_ROUND) return fr_round(src[row * 3 * w + b]);
    else return fr_trunc(src[row * 3 * w + b]);
}

template <int MODE>
__global__ __launch_bounds__(FR_THREADS) void k_frame_to_u8(const float* __restrict__ src, int h, int w, uint8_t* __restrict__ dst, int64_t pitch,
                                                           const uint8_t* __restrict__ gt, int gt_channels, int64_t gt_pitch,
                                                           unsigned long long* __restrict__ sse, int items_per_row, int vec_src, int vec_dst, int vec_gt)
{
    __shared__ uint32_t wave_sum[FR_THREADS / 64];
    const int64_t item = (int64_t)blockIdx.x * FR_THREADS + threadIdx.x;
    const int row_bytes = 3 * w;
    uint32_t sq = 0;
    if (item < (int64_t)h * items_per_row) {
        const int64_t row = item / items_per_row;
        const int b0 = (int)(item % items_per_row) * FR_ITEM;
        const int nb = min(FR_ITEM, row_bytes - b0);
        uint32_t v[FR_ITEM];
        if (MODE != GS_FRAME_DEPTH_CMAP && vec_src && nb == FR_ITEM) {
            const float4* p = reinterpret_cast<const float4*>(src + row * row_bytes + b0);
#pragma unroll
            for (int k = 0; k < FR_ITEM / 4; ++k) {
                const float4 f = p[k];
                if constexpr (MODE == GS_FRAME_RGB_ROUND) {
                    v[4 * k] = fr_round(f.x); v[4 * k + 1] = fr_round(f.y); v[4 * k + 2] = fr_round(f.z); v[4 * k + 3] = fr_round(f.w);
                } else {
                    v[4 * k] = fr_trunc(f.x); v[4 * k + 1] = fr_trunc(f.y); v[4 * k + 2] = fr_trunc(f.z); v[4 * k + 3] = fr_trunc(f.w);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < FR_ITEM; ++k) v[k] = k < nb ? fr_byte<MODE>(src, row, w, b0 + k) : 0u;
        }
        uint8_t* out = dst + row * pitch + b0;
        if (vec_dst && nb == FR_ITEM) {
            uint4 o;
            o.x = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
            o.y = v[4] | v[5] << 8 | v[6] << 16 | v[7] << 24;
            o.z = v[8] | v[9] << 8 | v[10] << 16 | v[11] << 24;
            o.w = v[12] | v[13] << 8 | v[14] << 16 | v[15] << 24;
            *reinterpret_cast<uint4*>(out) = o;
        } else {
#pragma unroll
            for (int k = 0; k < FR_ITEM; ++k) if (k < nb) out[k] = (uint8_t)v[k];
        }
        if (gt) {
            const uint8_t* g = gt + row * gt_pitch;
            if (vec_gt && nb == FR_ITEM) {
                const uint4 q = *reinterpret_cast<const uint4*>(g + b0);
                const uint32_t word[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
                for (int k = 0; k < FR_ITEM; ++k) {
                    const int d = (int)v[k] - (int)((word[k / 4] >> (8 * (k % 4))) & 255u);
                    sq += (uint32_t)(d * d);
                }
            } else {
#pragma unroll
                for (int k = 0; k < FR_ITEM; ++k)
                    if (k < nb) {
                        const int b = b0 + k;
                        const int d = (int)v[k] - (int)g[(int64_t)(b / 3) * gt_channels + b % 3];
                        sq += (uint32_t)(d * d);
                    }
            }
        }
    }
    if (!gt) return;                        // uniform over the grid
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_down(sq, o, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (int k = 0; k < FR_THREADS / 64; ++k) total += wave_sum[k];
        if (total) atomicAdd(sse, (unsigned long long)total);
    }
}

void gs_launch_frame_to_u8(const float* src, int mode, int h, int w, uint8_t* dst, int64_t pitch, const uint8_t* gt, int gt_channels,
                           int64_t gt_pitch, int64_t* sse, hipStream_t s)
{
    const int items_per_row = (3 * w + FR_ITEM - 1) / FR_ITEM;
    const int64_t items = (int64_t)h * items_per_row;
    const dim3 grid((unsigned)((items + FR_THREADS - 1) / FR_THREADS));
    const int vec_src = (w % 4 == 0 && ((uintptr_t)src & 15) == 0) ? 1 : 0;
    const int vec_dst = (((uintptr_t)dst & 15) == 0 && pitch % 16 == 0) ? 1 : 0;
    const int vec_gt = (gt && gt_channels == 3 && ((uintptr_t)gt & 15) == 0 && gt_pitch % 16 == 0) ? 1 : 0;
    unsigned long long* word = reinterpret_cast<unsigned long long*>(sse);
#define FR_LAUNCH(MODE) hipLaunchKernelGGL(k_frame_to_u8<MODE>, grid, dim3(FR_THREADS), 0, s, src, h, w, dst, pitch, gt, gt_channels, gt_pitch, \
                                           word, items_per_row, vec_src, vec_dst, vec_gt)
    if (mode == GS_FRAME_RGB_TRUNC) FR_LAUNCH(GS_FRAME_RGB_TRUNC);
    else if (mode == GS_FRAME_RGB_ROUND) FR_LAUNCH(GS_FRAME_RGB_ROUND);
    else FR_LAUNCH(GS_FRAME_DEPTH_CMAP);
#undef FR_LAUNCH
}
