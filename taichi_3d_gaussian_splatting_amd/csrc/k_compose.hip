// k_compose.hip -- baking a placed scene (include/gs_compose.h): one similarity transform (q_A, t_A, s) applied to n rows,
// out of place, into rows [row_offset, row_offset + n) of the outputs.
//
// A workgroup is one wave and owns BK_ROWS = 64 consecutive rows, one per lane.
//   load      the rows' 56-float feature rows are contiguous: the wave copies them to LDS with coalesced loads (16 bytes per
//             lane where both feature pointers allow it), each row behind a pitch of 57 floats so that the lanes' walks over
//             their own rows fall into different banks;
//   rows      lane r reads its row from LDS, transforms it in registers (fixed-order fma chains, the matrices are kernel
//             arguments: wave-uniform) and writes it back in place;
//   store     the wave copies the tile to the output rows, coalesced again.
// The 12-byte positions are read and written as scalars by the row's lane: three consecutive floats per lane, and a row at an
// odd index is not 16-byte aligned.  No atomics, no cross-lane sums: the same bits on every run.
#include "gs_common.h"
#include "../../include/gs_compose.h"

#define BK_ROWS GS_BAKE_ROWS_PER_BLOCK
#define BK_F GS_BAKE_FEATURES
#define BK_PITCH (BK_F + 1)
static_assert(BK_ROWS == 64, "one wave per workgroup, one row per lane");

// f'[i] = sum_j M[i][j] f[j], ascending j, for one band of one colour channel
template <int D>
__device__ __forceinline__ void bk_band(const float* __restrict__ M, const float* f, float* out)
{
#pragma unroll
    for (int i = 0; i < D; ++i) {
        float a = M[i * D] * f[0];
#pragma unroll
        for (int j = 1; j < D; ++j) a = fmaf(M[i * D + j], f[j], a);
        out[i] = a;
    }
}

__global__ __launch_bounds__(BK_ROWS) void k_scene_bake(const float* __restrict__ xyz_in, const float* __restrict__ feat_in, int64_t n,
                                                        GsBakeTransform A, float* __restrict__ xyz_out, float* __restrict__ feat_out,
                                                        int64_t row_offset, int vec)
{
    __shared__ __align__(16) float tile[BK_ROWS * BK_PITCH];
    const int lane = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * BK_ROWS;
    const int rows = (int)min((int64_t)BK_ROWS, n - r0);
    const int floats = rows * BK_F;
    const float* in = feat_in + r0 * BK_F;
    float* out = feat_out + (row_offset + r0) * BK_F;

    // 224-byte rows: a 16-byte aligned base keeps every row, and so every block's first float, 16-byte aligned
    if (vec) {
        for (int i = 4 * lane; i < floats; i += 4 * BK_ROWS) {          // BK_F % 4 == 0: a float4 never straddles two rows
            const float4 v = *reinterpret_cast<const float4*>(in + i);
            float* t = &tile[(i / BK_F) * BK_PITCH + i % BK_F];
            t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
        }
    } else {
        for (int i = lane; i < floats; i += BK_ROWS) tile[(i / BK_F) * BK_PITCH + i % BK_F] = in[i];
    }
    __syncthreads();

    if (lane < rows) {
        const int64_t r = r0 + lane;
        const float x = xyz_in[3 * r], y = xyz_in[3 * r + 1], z = xyz_in[3 * r + 2];
        float* o = xyz_out + 3 * (row_offset + r);
        o[0] = fmaf(A.m[2], z, fmaf(A.m[1], y, A.m[0] * x)) + A.t[0];
        o[1] = fmaf(A.m[5], z, fmaf(A.m[4], y, A.m[3] * x)) + A.t[1];
        o[2] = fmaf(A.m[8], z, fmaf(A.m[7], y, A.m[6] * x)) + A.t[2];

        float* f = &tile[lane * BK_PITCH];
        // q' = q_A (x) q / |q| (xyzw, Hamilton); a row without a direction keeps its words
        const float qx = f[0], qy = f[1], qz = f[2], qw = f[3];
        const float nn = sqrtf(fmaf(qw, qw, fmaf(qz, qz, fmaf(qy, qy, qx * qx))));
        if (nn > 0.0f && nn < INFINITY) {
            const float bx = qx / nn, by = qy / nn, bz = qz / nn, bw = qw / nn;
            const float ax = A.q[0], ay = A.q[1], az = A.q[2], aw = A.q[3];
            f[0] = fmaf(ay, bz, fmaf(-az, by, fmaf(bw, ax, aw * bx)));
            f[1] = fmaf(az, bx, fmaf(-ax, bz, fmaf(bw, ay, aw * by)));
            f[2] = fmaf(ax, by, fmaf(-ay, bx, fmaf(bw, az, aw * bz)));
            f[3] = fmaf(-az, bz, fmaf(-ay, by, fmaf(-ax, bx, aw * bw)));
        }
        f[4] += A.log_scale; f[5] += A.log_scale; f[6] += A.log_scale;
        // f[7], the opacity logit, is copied
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* sh = f + 8 + 16 * c;
            float src[16], res[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) src[k] = sh[k];
            bk_band<1>(A.sh, src, res);
            bk_band<3>(A.sh + 1, src + 1, res + 1);
            bk_band<5>(A.sh + 10, src + 4, res + 4);
            bk_band<7>(A.sh + 35, src + 9, res + 9);
#pragma unroll
            for (int k = 0; k < 16; ++k) sh[k] = res[k];
        }
    }
    __syncthreads();

    if (vec) {
        for (int i = 4 * lane; i < floats; i += 4 * BK_ROWS) {
            const float* t = &tile[(i / BK_F) * BK_PITCH + i % BK_F];
            *reinterpret_cast<float4*>(out + i) = make_float4(t[0], t[1], t[2], t[3]);
        }
    } else {
        for (int i = lane; i < floats; i += BK_ROWS) out[i] = tile[(i / BK_F) * BK_PITCH + i % BK_F];
    }
}

void gs_launch_scene_bake(const float* xyz_in, const float* feat_in, int64_t n, const GsBakeTransform& A, float* xyz_out, float* feat_out,
                          int64_t row_offset, hipStream_t s)
{
    const dim3 grid((unsigned)((n + BK_ROWS - 1) / BK_ROWS));
    const int vec = ((((uintptr_t)feat_in | (uintptr_t)feat_out) & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(k_scene_bake, grid, dim3(BK_ROWS), 0, s, xyz_in, feat_in, n, A, xyz_out, feat_out, row_offset, vec);
}
