// k_sparse.hip -- include/gs_sparse.h: the rows a backward touched as an ordered list on the device (k_rows_count,
// k_rows_scatter) and Adam over such a list (k_adam_rows).  Nothing here waits on another workgroup and no atomic decides a
// position: the list is the same on every run.
#include "gs_common.h"

#include <cstdlib>

// ---- ordered compaction -------------------------------------------------------------------------------------------
// Input: the M tag bytes of the last backward (touched[m] == gen where some pixel took a contribution from in-camera point m;
// k_blend_bwd_tile writes them, k_sum_rows reads them the same way), NOT column 10 of the per-point sums: the bytes are a
// twelfth of the traffic and exist for gs_backward_projected too, whose sums live in the caller's memory.  ids_in[m] ascends
// with m (k_project compacts in order), so keeping m order keeps the output ascending.
//
// A block owns GS_ROWS_BLOCK consecutive points: a lane loads four tag bytes as one word, its hits are a 4-bit mask, its
// count a popcount, and the positions come from gs_wave_scan_incl / gs_block_scan_*.  Across blocks: k_rows_count leaves
// one total per block, and every k_rows_scatter block adds up the totals before it (the pattern of k_keygen), so the list
// needs two launches and no block waits for another.  With one block (M <= GS_ROWS_BLOCK) the count launch is skipped.
// The re-summing is O(nb^2) words from L2, nb = ceil(M / 1024): 122 blocks * 61 words on average at M = 1.25e5, nothing;
// at N = 1e7 with every point in camera nb = 9766 and the blocks read 4.8e7 words = 191 MB from a 39 KB L2-resident array
// in all, against 50 MB of compulsory HBM traffic (10 MB of tags, 40 MB of ids) -- a few tens of microseconds beside a
// dense step that streams 16 GB there.  Blocks of 4096 points would make it 12 MB.
#define GS_ROWS_BLOCK 1024

int gs_rows_blocks(int M) { return M > 0 ? (M + GS_ROWS_BLOCK - 1) / GS_ROWS_BLOCK : 0; }

// the hits among points first .. first + 3 as a 4-bit mask (first is a multiple of 4)
__device__ __forceinline__ uint32_t gs_tag_mask4(const uint8_t* __restrict__ touched, int first, int M, uint32_t gen)
{
    if (first >= M) return 0u;
    const uint32_t w = *reinterpret_cast<const uint32_t*>(touched + first);
    uint32_t mask = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (((w >> (8 * k)) & 255u) == gen && first + k < M) mask |= 1u << k;
    return mask;
}

__global__ __launch_bounds__(256) void k_rows_count(const uint8_t* __restrict__ touched, uint32_t gen, int M, uint32_t* __restrict__ block_totals)
{
    __shared__ int ws[4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int first = (int)blockIdx.x * GS_ROWS_BLOCK + 4 * (int)threadIdx.x;
    gs_block_put(ws, wave, lane, gs_wave_sum_i(__popc(gs_tag_mask4(touched, first, M, gen))));
    __syncthreads();
    if (threadIdx.x == 0) block_totals[blockIdx.x] = (uint32_t)gs_block_sum<4>(ws);
}

__global__ __launch_bounds__(256) void k_rows_scatter(const uint8_t* __restrict__ touched, uint32_t gen, const int32_t* __restrict__ ids_in, int M,
                                                      const uint32_t* __restrict__ block_totals, int32_t* __restrict__ ids_out,
                                                      int64_t capacity, int32_t* __restrict__ count_out)
{
    __shared__ uint32_t ws[4], wpre[4];
    __shared__ int32_t sOut[GS_ROWS_BLOCK];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int first = (int)blockIdx.x * GS_ROWS_BLOCK + 4 * (int)threadIdx.x;
    uint32_t mask = gs_tag_mask4(touched, first, M, gen);
    const uint32_t n = (uint32_t)__popc(mask);
    const uint32_t incl = gs_wave_scan_incl(n, lane);
    gs_block_scan_put(ws, wave, lane, incl);
    // first entry of this block = the hits of all blocks before it (block 0 reads nothing: block_totals may be NULL then)
    gs_block_put(wpre, wave, lane, gs_sum_of_blocks_before<256>(block_totals, (int)blockIdx.x));
    __syncthreads();
    const uint32_t base = gs_block_sum<4>(wpre), total = gs_block_sum<4>(ws);
    uint32_t at = gs_block_scan_excl(ws, wave, incl, n);
    // the block's rows go through LDS so that the list is stored in whole, coalesced runs
    while (mask) {
        const int k = __builtin_ctz(mask);
        mask &= mask - 1u;
        sOut[at++] = ids_in ? ids_in[first + k] : first + k;    // (NULL: the identity, the tags are indexed by row -- gs_merge_rows)
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *count_out = (int32_t)(base + total);      // the block that owns the end
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < total; i += 256u)
        if ((int64_t)(base + i) < capacity) ids_out[base + i] = sOut[i];
}

void gs_launch_touched_rows(const uint8_t* touched, uint8_t gen, const int32_t* ids_in, int M, uint32_t* block_totals,
                            int32_t* ids_out, int64_t capacity, int32_t* count_out, hipStream_t s)
{
    const int nb = gs_rows_blocks(M);
    if (nb == 0) { (void)hipMemsetAsync(count_out, 0, sizeof(int32_t), s); return; }
    if (nb > 1) k_rows_count<<<nb, 256, 0, s>>>(touched, gen, M, block_totals);
    k_rows_scatter<<<nb, 256, 0, s>>>(touched, gen, ids_in, M, block_totals, ids_out, capacity, count_out);
}

// ---- Adam over a list of rows ----------------------------------------------------------------------------------------
// gs_adam_update on rows ids[0 .. *count) of four (n_rows, row_len) tensors.  V = 4: consecutive lanes take consecutive
// float4s of a row (a 56-float row is 224 contiguous bytes, 14 lanes), flat index over count * row_len / 4, every stream
// 16-byte coalesced inside a row.  V = 1: one float per lane over count * row_len (row_len not a multiple of 4 -- the (N,3)
// positions -- or a tensor that is not 16-byte aligned).  The grid covers max_count rows, the host's bound; *count is read on
// the device and the threads beyond it leave at once (nine in ten blocks at the headline workload, where max_count is the
// frame's M).  An id outside [0, n_rows) is skipped: a stale list cannot write out of bounds.
template <int V>
__global__ __launch_bounds__(256) void k_adam_rows(float* __restrict__ param, const float* __restrict__ grad, float* __restrict__ exp_avg,
                                                   float* __restrict__ exp_avg_sq, int64_t n_rows, int row_len, const int32_t* __restrict__ ids,
                                                   const int32_t* __restrict__ count, int64_t max_count, float lr, float beta1, float beta2,
                                                   float eps, float bias1, float bias2_sqrt)
{
    const int per_row = row_len / V;
    int64_t rows = (int64_t)count[0];
    rows = rows < max_count ? rows : max_count;
    const int64_t total = rows * per_row;
    // (one pass when the grid covers max_count rows; a smaller grid strides)
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        int64_t r;
        int c;
        if (total <= 0xffffffffll) {                            // (uniform; a 64-bit division is a subroutine on this part)
            const uint32_t r32 = (uint32_t)e / (uint32_t)per_row;
            r = r32; c = (int)((uint32_t)e - r32 * (uint32_t)per_row);
        } else { r = e / per_row; c = (int)(e - r * per_row); }
        const int64_t id = (int64_t)ids[r];
        if (id < 0 || id >= n_rows) continue;
        const int64_t at = id * row_len + (int64_t)V * c;
        if constexpr (V == 4) {
            float4 p = *reinterpret_cast<const float4*>(param + at), m = *reinterpret_cast<const float4*>(exp_avg + at);
            float4 v = *reinterpret_cast<const float4*>(exp_avg_sq + at);
            const float4 g = *reinterpret_cast<const float4*>(grad + at);
            gs_adam_update(p.x, g.x, m.x, v.x, lr, beta1, beta2, eps, bias1, bias2_sqrt);
            gs_adam_update(p.y, g.y, m.y, v.y, lr, beta1, beta2, eps, bias1, bias2_sqrt);
            gs_adam_update(p.z, g.z, m.z, v.z, lr, beta1, beta2, eps, bias1, bias2_sqrt);
            gs_adam_update(p.w, g.w, m.w, v.w, lr, beta1, beta2, eps, bias1, bias2_sqrt);
            *reinterpret_cast<float4*>(exp_avg + at) = m; *reinterpret_cast<float4*>(exp_avg_sq + at) = v;
            *reinterpret_cast<float4*>(param + at) = p;
        } else {
            float p = param[at], m = exp_avg[at], v = exp_avg_sq[at];
            gs_adam_update(p, grad[at], m, v, lr, beta1, beta2, eps, bias1, bias2_sqrt);
            exp_avg[at] = m; exp_avg_sq[at] = v;
            param[at] = p;
        }
    }
}

void gs_launch_adam_rows(float* param, const float* grad, float* m, float* v, int64_t n_rows, int row_len, const int32_t* ids,
                         const int32_t* count, int64_t max_count, float lr, float beta1, float beta2, float eps, int64_t step, hipStream_t s)
{
    if (n_rows <= 0 || max_count <= 0) return;
    if (max_count > n_rows) max_count = n_rows;                 // ids are unique: no list is longer than the tensor
    float bias1, bias2_sqrt;
    gs_adam_bias(beta1, beta2, step, &bias1, &bias2_sqrt);
    const bool vec = row_len % 4 == 0 && (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v) & 15u) == 0;
    const int64_t work = max_count * (vec ? row_len / 4 : row_len);
    int64_t nb = (work + 255) / 256;
    // GS_ADAM_ROWS_GRID=<blocks>: a fixed grid that strides to *count instead, read at every call so that
    // tools/bench_sparse_step.py can alternate the two shapes in one process (DESIGN.md section 5 has the comparison)
    const char* env = getenv("GS_ADAM_ROWS_GRID");
    const int64_t fixed = env ? (int64_t)atoll(env) : (int64_t)0;
    if (fixed > 0 && fixed < nb) nb = fixed;
    if (nb > 0x7fffffff) nb = 0x7fffffff;                       // (the loop strides over the rest)
    if (vec) k_adam_rows<4><<<(unsigned)nb, 256, 0, s>>>(param, grad, m, v, n_rows, row_len, ids, count, max_count, lr, beta1, beta2, eps, bias1, bias2_sqrt);
    else k_adam_rows<1><<<(unsigned)nb, 256, 0, s>>>(param, grad, m, v, n_rows, row_len, ids, count, max_count, lr, beta1, beta2, eps, bias1, bias2_sqrt);
}
