// k_vq.hip -- the two halves of a k-means iteration (include/gs_vq.h, which states every chain to the parenthesis).
//
//   gs_vq_assign   k_vq_norms    one thread per centroid: cc_k, the fmaf chain over its Dp columns, into the scratch
//                  k_vq_assign   128 rows per block, 32 per wave, on the matrix cores: v_mfma_f32_32x32x2_f32 adds a_k0 b_k0 and
//                                then a_k1 b_k1 to C, each fused and rounded once -- the chain s = fmaf(x_j, -2 c_j, s) in ascending
//                                j when step t feeds it the columns 2t and 2t + 1.  Rows of x sit on the accumulator's column
//                                (lane & 31), centroids on its 16 registers x 2 lane halves; C starts as cc_k.  A tile of 64
//                                centroids (-2 c, zero padded) is staged in LDS per round and used by two accumulators.  Each lane
//                                keeps (best, label) over its registers in ascending k; the two lane halves of a column are merged
//                                once at the end, by (s, k).
//   gs_vq_update   k_vq_update   one wave per 1 or VU_CODES consecutive codes, one lane per column: all labels in ascending order, the
//                                matching rows added one after the other into float64 registers
//
// No float atomics, no atomics at all: every output has one writer.
#include "gs_common.h"
#include "../../include/gs_vq.h"

#define VQ_BLOCK 256
#define VQ_ROWS 128                      // rows of x per block: 32 per wave
#define VQ_TILE 64                       // centroids per round: two 32-row accumulators
#define VU_CHUNK 8                       // 64-label loads in flight per wave of the update
#define VU_GATHER 4                      // rows of x in flight per wave of the update
#ifndef VU_CODES
#define VU_CODES 4                       // codes per wave of the update past 1024 codes (changes no bit of the result)
#endif

typedef float vq_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ bool vq_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }      // false for NaN and +-inf
__host__ __device__ static inline int vq_dp(int dim) { return (dim + 3) & ~3; }

size_t gs_vq_scratch_size(int64_t n_rows, int n_codes, int dim) { (void)n_rows; (void)dim; return (size_t)(4 * (((int64_t)n_codes + 15) & ~15ll) + 64); }
static size_t vq_assign_lds(int Dp) { return sizeof(float) * ((size_t)(VQ_ROWS + VQ_TILE) * (Dp + 1) + VQ_TILE); }

__global__ __launch_bounds__(VQ_BLOCK) void k_vq_norms(const float* __restrict__ cb, int64_t ldc, int K, int dim, int Dp, float* __restrict__ cc)
{
    const int k = blockIdx.x * VQ_BLOCK + threadIdx.x;
    if (k >= K) return;
    const float* row = cb + (size_t)k * ldc;
    float acc = 0.0f;
    for (int j = 0; j < Dp; ++j) {
        const float v = j < dim ? row[j] : 0.0f;
        acc = fmaf(v, v, acc);
    }
    cc[k] = acc;
}

// `rows` rows of src (leading dimension ld, the first at row0, n_total in all) into dst[rows][Dp + 1], times `scale`; rows past
// the end and columns past dim as scale * +0.  16-byte loads: ld is a multiple of 4 and >= Dp.
__device__ __forceinline__ void vq_stage(float* __restrict__ dst, const float* __restrict__ src, int64_t ld, int64_t row0, int64_t n_total,
                                         int rows, int dim, int Dp, float scale)
{
    const int Dq = Dp >> 2, stride = Dp + 1;
    for (int idx = threadIdx.x; idx < rows * Dq; idx += VQ_BLOCK) {
        const int r = idx / Dq, q = idx - r * Dq;
        const int64_t n = row0 + r;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (n < n_total) v = *reinterpret_cast<const float4*>(src + (size_t)n * ld + 4 * q);
        const int j = 4 * q;
        float* d = dst + r * stride + j;
        d[0] = scale * v.x;                                        // j < dim always: Dp - dim < 4
        d[1] = scale * (j + 1 < dim ? v.y : 0.0f);
        d[2] = scale * (j + 2 < dim ? v.z : 0.0f);
        d[3] = scale * (j + 3 < dim ? v.w : 0.0f);
    }
}

// the centroid a lane's accumulator register i holds, within a 32-row accumulator (the C/D map of the 32x32 matrix instructions)
__device__ __forceinline__ int vq_acc_row(int i, int half) { return (i & 3) + 8 * (i >> 2) + 4 * half; }

__global__ __launch_bounds__(VQ_BLOCK) void k_vq_assign(const float* __restrict__ x, int64_t ldx, int64_t N, int dim, int Dp,
                                                        const float* __restrict__ cb, int64_t ldc, int K, const float* __restrict__ cc,
                                                        int32_t* __restrict__ labels, float* __restrict__ dist)
{
    extern __shared__ float vq_lds[];
    const int stride = Dp + 1;                                      // odd: the 32 rows a half-wave reads fall on 32 banks
    float* sx = vq_lds;                                             // [VQ_ROWS][stride]   x
    float* sc = sx + VQ_ROWS * stride;                              // [VQ_TILE][stride]   -2 c of the round's centroids
    float* scc = sc + VQ_TILE * stride;                             // [VQ_TILE]           their cc
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, half = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * VQ_ROWS;
    vq_stage(sx, x, ldx, row0, N, VQ_ROWS, dim, Dp, 1.0f);
    float best = __builtin_inff();
    int label = -1;
    for (int k0 = 0; k0 < K; k0 += VQ_TILE) {
        __syncthreads();                                            // the last round's readers are done (and sx is written)
        vq_stage(sc, cb, ldc, k0, K, VQ_TILE, dim, Dp, -2.0f);
        if (threadIdx.x < VQ_TILE) scc[threadIdx.x] = k0 + (int)threadIdx.x < K ? cc[k0 + threadIdx.x] : 0.0f;
        __syncthreads();
        vq_f32x16 acc0, acc1;
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc0[i] = scc[vq_acc_row(i, half)]; acc1[i] = scc[32 + vq_acc_row(i, half)]; }
#if defined(__HIP_DEVICE_COMPILE__)                                 // (the host pass does not know the instruction)
        const float* my_x = sx + (wave * 32 + col) * stride + half; // column 2t + half at step t
        const float* my_c = sc + col * stride + half;
        for (int t = 0; t < (Dp >> 1); ++t) {
            const float b = my_x[2 * t];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(my_c[2 * t], b, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(my_c[32 * stride + 2 * t], b, acc1, 0, 0, 0);
        }
#endif
#pragma unroll
        for (int i = 0; i < 16; ++i) {                              // ascending k within the lane: a tie keeps the earlier
            const int r = vq_acc_row(i, half), k = k0 + r;
            if (k < K && vq_finite(scc[r]) && acc0[i] < best) { best = acc0[i]; label = k; }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = 32 + vq_acc_row(i, half), k = k0 + r;
            if (k < K && vq_finite(scc[r]) && acc1[i] < best) { best = acc1[i]; label = k; }
        }
    }
    // the other half of the column: the smaller s, and on a tie the smaller k
    const float o_best = __shfl_xor(best, 32);
    const int o_label = __shfl_xor(label, 32);
    if (o_label >= 0 && (label < 0 || o_best < best || (o_best == best && o_label < label))) { best = o_best; label = o_label; }
    const int64_t n = row0 + wave * 32 + col;
    if (half != 0 || n >= N) return;
    float xx = 0.0f;
    const float* xr = sx + (wave * 32 + col) * stride;
    for (int j = 0; j < Dp; ++j) xx = fmaf(xr[j], xr[j], xx);
    if (!vq_finite(xx)) label = -1;
    labels[n] = label;
    if (dist) dist[n] = label < 0 ? __builtin_nanf("") : fmaxf(0.0f, xx + best);
}

// One wave per CODES consecutive codes, lane j = column j.
template <int CODES>
__global__ __launch_bounds__(64) void k_vq_update(const float* __restrict__ x, int64_t ldx, int64_t N, int dim, const float* __restrict__ weights,
                                                  const int32_t* __restrict__ labels, float* __restrict__ cb, int64_t ldc, int K,
                                                  int32_t* __restrict__ counts, double* __restrict__ weight_sums)
{
    const int lane = threadIdx.x;
    const int k0 = blockIdx.x * CODES;
    double S[CODES], W[CODES];
    int cnt[CODES];
#pragma unroll
    for (int c = 0; c < CODES; ++c) { S[c] = 0.0; W[c] = 0.0; cnt[c] = 0; }
    const bool column = lane < dim;
    for (int64_t base = 0; base < N; base += 64 * VU_CHUNK) {
        int local[VU_CHUNK];
        float w[VU_CHUNK];
#pragma unroll
        for (int u = 0; u < VU_CHUNK; ++u) {                        // the loads of a round go out together
            const int64_t n = base + 64 * u + lane;
            const int lb = n < N ? labels[n] : -1;
            local[u] = (lb >= k0 && lb < k0 + CODES && lb < K) ? lb - k0 : -1;
            w[u] = (n < N && weights) ? weights[n] : 1.0f;
        }
#pragma unroll
        for (int u = 0; u < VU_CHUNK; ++u) {
            const bool member = local[u] >= 0 && w[u] > 0.0f && vq_finite(w[u]);
            unsigned long long m = gs_ballot(member);
            while (m) {                                             // ascending rows; m is wave-uniform
                int bit[VU_GATHER], n_bits = 0;
                float v[VU_GATHER];
#pragma unroll
                for (int g = 0; g < VU_GATHER; ++g) {
                    bit[g] = 0;
                    v[g] = 0.0f;
                    if (m) {
                        bit[g] = __builtin_ctzll(m);
                        m &= m - 1;
                        n_bits = g + 1;
                        if (column) v[g] = x[(size_t)(base + 64 * u + bit[g]) * ldx + lane];
                    }
                }
#pragma unroll
                for (int g = 0; g < VU_GATHER; ++g) {
                    if (g < n_bits) {
                        const int cl = __builtin_amdgcn_readfirstlane(__shfl(local[u], bit[g]));
                        const double wd = (double)__shfl(w[u], bit[g]);
                        const double p = wd * (double)v[g];
#pragma unroll
                        for (int c = 0; c < CODES; ++c)
                            if (cl == c) { W[c] = W[c] + wd; S[c] = S[c] + p; cnt[c] += 1; }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < CODES; ++c) {
        const int k = k0 + c;
        if (k >= K) break;
        if (lane == 0) { counts[k] = cnt[c]; if (weight_sums) weight_sums[k] = W[c]; }
        if (cnt[c] > 0 && column) cb[(size_t)k * ldc + lane] = (float)(S[c] / W[c]);
    }
}

// ---- launchers: they trust what the entry points checked ---------------------------------------------------------------------
void gs_launch_vq_assign(const float* x, int64_t ldx, int64_t N, int dim, const float* cb, int64_t ldc, int K, int32_t* labels, float* dist,
                         void* scratch, hipStream_t s)
{
    if (N <= 0) return;
    const int Dp = vq_dp(dim);
    float* cc = static_cast<float*>(scratch);
    k_vq_norms<<<(K + VQ_BLOCK - 1) / VQ_BLOCK, VQ_BLOCK, 0, s>>>(cb, ldc, K, dim, Dp, cc);
    const unsigned grid = (unsigned)((N + VQ_ROWS - 1) / VQ_ROWS);
    k_vq_assign<<<grid, VQ_BLOCK, vq_assign_lds(Dp), s>>>(x, ldx, N, dim, Dp, cb, ldc, K, cc, labels, dist);
}

void gs_launch_vq_update(const float* x, int64_t ldx, int64_t N, int dim, const float* weights, const int32_t* labels, float* cb, int64_t ldc,
                         int K, int32_t* counts, double* weight_sums, hipStream_t s)
{
    // few codes: a wave each, so that there are waves enough; many: VU_CODES share a pass over the labels
    if (K <= 1024) k_vq_update<1><<<K, 64, 0, s>>>(x, ldx, N, dim, weights, labels, cb, ldc, K, counts, weight_sums);
    else k_vq_update<VU_CODES><<<(K + VU_CODES - 1) / VU_CODES, 64, 0, s>>>(x, ldx, N, dim, weights, labels, cb, ldc, K, counts, weight_sums);
}
