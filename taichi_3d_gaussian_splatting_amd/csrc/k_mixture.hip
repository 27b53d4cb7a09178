// k_mixture.hip -- the scene as a Gaussian mixture (include/gs_mixture.h): log-density at points, closed-form Fourier transform
// at frequencies.  Brute force by definition -- every row that takes part enters every output -- so the work is P x N pairs of
// about twenty f32 operations and one exponential (the transform: a sine and cosine by polynomial besides), and nearly no
// memory traffic.  The arithmetic of a row and of a pair is gs_mixture_math.h.
//
//   k_mix_sigma_blocks   sum of sigmoid(opacity logit) over the rows that take part, per block of 256 rows (float64, LDS tree)
//   k_mix_sigma_total    those block sums in ascending order (one workgroup)
//   k_mix_records        one 64-byte record per row, the rows padded to a multiple of GS_MIX_CHUNK with records of no effect
//   k_mix_density / k_mix_fourier
//                        grid (query blocks) x (component chunks).  A lane owns GS_MIX_LANE_POINTS queries (independent
//                        chains); the records are read at wave-uniform addresses, four at a time, so they arrive by scalar
//                        loads and sit in scalar registers as operands of the vector arithmetic.  Four records that all take
//                        no part are skipped by a wave-uniform branch.  The density keeps a running maximum m and
//                        s = sum 2^(t - m) per query, m moved once per four records (five exponentials per four pairs).
//   k_mix_merge_density / k_mix_merge_fourier
//                        the chunk partials of a query in ascending chunk order, in float64, rounded once.
//
// The split into chunks (gs_mix_chunks) reads (n_points, n_x) only.  Nothing here uses an atomic.
#include "gs_common.h"
#include "gs_mixture_math.h"

#include <cfloat>

#define GS_MIX_CHUNK 256                // records per unit of the component loop: a chunk is a whole number of units
#define GS_MIX_LANE_POINTS 2            // queries per lane
#define GS_MIX_POINTS_PER_WG 512        // queries per workgroup: 256 lanes x GS_MIX_LANE_POINTS
#define GS_MIX_TARGET_WGS 2048          // workgroups the grid aims at when few query blocks exist (256 CUs x 8)
#define GS_MIX_MAX_CHUNKS 1024
static_assert(GS_MIX_POINTS_PER_WG == 256 * GS_MIX_LANE_POINTS, "a workgroup is 256 lanes");
static_assert(GS_MIX_CHUNK % GS_MIX_BATCH == 0, "a unit is a whole number of steps");

static int64_t gs_mix_units(int64_t n) { return (n + GS_MIX_CHUNK - 1) / GS_MIX_CHUNK; }
static int64_t gs_mix_sigma_blocks(int64_t n) { return (n + 255) / 256; }

// How the component loop of a call is split: -> number of chunks, *units_per_chunk units of GS_MIX_CHUNK records in each (the
// last may hold fewer).  A function of (n_points, n_x) alone.
int gs_mix_chunks(int64_t n_points, int64_t n_x, int64_t* units_per_chunk)
{
    const int64_t units = gs_mix_units(n_points), qblocks = (n_x + GS_MIX_POINTS_PER_WG - 1) / GS_MIX_POINTS_PER_WG;
    int64_t want = (GS_MIX_TARGET_WGS + qblocks - 1) / qblocks;
    want = want > GS_MIX_MAX_CHUNKS ? GS_MIX_MAX_CHUNKS : want;
    want = want > units ? units : want;
    want = want < 1 ? 1 : want;
    const int64_t upc = (units + want - 1) / want;
    *units_per_chunk = upc;
    return (int)((units + upc - 1) / upc);
}

size_t gs_mix_record_bytes(int64_t n_points) { return (size_t)gs_mix_units(n_points) * GS_MIX_CHUNK * GS_MIX_REC_FLOATS * sizeof(float); }
size_t gs_mix_sum_bytes(int64_t n_points) { return (size_t)(gs_mix_sigma_blocks(n_points) + 1) * sizeof(double); }
size_t gs_mix_partial_bytes(int64_t n_points, int64_t n_x)
{
    int64_t upc;
    return (size_t)gs_mix_chunks(n_points, n_x, &upc) * (size_t)n_x * sizeof(float2);
}

// ---- the weights' sum ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_mix_sigma_blocks(const float* __restrict__ mu, const float* __restrict__ feat,
                                                          const int8_t* __restrict__ mask, int64_t n, double* __restrict__ block_sums)
{
    __shared__ double lds[256];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v = 0.0;
    if (i < n && gs_mix_takes_part(mu + 3 * i, feat + GS_MIX_NFEAT * i, mask, i)) v = gs_mix_sigmoid((double)feat[GS_MIX_NFEAT * i + 7]);
    const double sum = gs_mix_block_sum(v, lds);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = sum;
}

// block_sums[n_blocks] = their sum: lane t takes blocks t, t + 256, ... in ascending order, then the tree
__global__ void __launch_bounds__(256) k_mix_sigma_total(double* __restrict__ block_sums, int64_t n_blocks)
{
    __shared__ double lds[256];
    double v = 0.0;
    for (int64_t b = threadIdx.x; b < n_blocks; b += 256) v += block_sums[b];
    const double sum = gs_mix_block_sum(v, lds);
    if (threadIdx.x == 0) block_sums[n_blocks] = sum;
}

__global__ void __launch_bounds__(256) k_mix_records(const float* __restrict__ mu, const float* __restrict__ feat,
                                                     const int8_t* __restrict__ mask, int64_t n, int64_t n_pad,
                                                     const double* __restrict__ total, int fourier, const float* __restrict__ centre,
                                                     float4* __restrict__ rec_out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pad) return;
    float rec[GS_MIX_REC_FLOATS];
    const bool inside = i < n;
    const int64_t row = inside ? i : 0;                        // a padding record reads row 0 and takes no part
    const bool part = inside && gs_mix_takes_part(mu + 3 * row, feat + GS_MIX_NFEAT * row, mask, row);
    gs_mix_record(mu + 3 * row, feat + GS_MIX_NFEAT * row, part, total[0], fourier != 0, centre, rec);
#pragma unroll
    for (int j = 0; j < 4; ++j) rec_out[4 * i + j] = make_float4(rec[4 * j], rec[4 * j + 1], rec[4 * j + 2], rec[4 * j + 3]);
}

// ---- the pair loops --------------------------------------------------------------------------------------------------------------
// the queries of this lane: row p of xyz, the last row where p is past the end (computed, never written)
__device__ __forceinline__ void gs_mix_load_queries(const float* __restrict__ xyz, int64_t n_x, int64_t (&p)[GS_MIX_LANE_POINTS],
                                                    float (&v)[GS_MIX_LANE_POINTS][3], bool (&finite)[GS_MIX_LANE_POINTS])
{
#pragma unroll
    for (int q = 0; q < GS_MIX_LANE_POINTS; ++q) {
        p[q] = (int64_t)blockIdx.x * GS_MIX_POINTS_PER_WG + q * 256 + threadIdx.x;
        const int64_t row = p[q] < n_x ? p[q] : n_x - 1;
        v[q][0] = xyz[3 * row]; v[q][1] = xyz[3 * row + 1]; v[q][2] = xyz[3 * row + 2];
        finite[q] = gs_mix_finite(v[q][0]) && gs_mix_finite(v[q][1]) && gs_mix_finite(v[q][2]);
    }
}

// partial[chunk][p] = (m, s): the running maximum of the base-2 exponents of the chunk's records and sum 2^(t - m); s is NaN for
// a non-finite query.  n_pad = records in all (a multiple of GS_MIX_CHUNK).
__global__ void __launch_bounds__(256) k_mix_density(const float4* __restrict__ rec, int64_t n_pad, int64_t units_per_chunk,
                                                     const float* __restrict__ x, int64_t n_x, float2* __restrict__ partial)
{
    int64_t p[GS_MIX_LANE_POINTS];
    float v[GS_MIX_LANE_POINTS][3], m[GS_MIX_LANE_POINTS], s[GS_MIX_LANE_POINTS];
    bool finite[GS_MIX_LANE_POINTS];
    gs_mix_load_queries(x, n_x, p, v, finite);
#pragma unroll
    for (int q = 0; q < GS_MIX_LANE_POINTS; ++q) { m[q] = -FLT_MAX; s[q] = 0.0f; }
    const int64_t r0 = (int64_t)blockIdx.y * units_per_chunk * GS_MIX_CHUNK;
    const int64_t r1 = r0 + units_per_chunk * GS_MIX_CHUNK < n_pad ? r0 + units_per_chunk * GS_MIX_CHUNK : n_pad;
    for (int64_t i = r0; i < r1; i += GS_MIX_BATCH) {
        float r[GS_MIX_BATCH][GS_MIX_REC_FLOATS];
        gs_mix_load_batch(rec, i, r);
        bool any = false;
#pragma unroll
        for (int u = 0; u < GS_MIX_BATCH; ++u) any = any || r[u][3] > -INFINITY;
        if (!any) continue;                                    // wave-uniform: none of the four takes part
#pragma unroll
        for (int q = 0; q < GS_MIX_LANE_POINTS; ++q) {
            float t[GS_MIX_BATCH];
#pragma unroll
            for (int u = 0; u < GS_MIX_BATCH; ++u) t[u] = gs_mix_density_term(r[u], v[q][0], v[q][1], v[q][2]);
            float top = m[q];                                  // fmaxf keeps the number where a term is NaN; the sum then becomes NaN
#pragma unroll
            for (int u = 0; u < GS_MIX_BATCH; ++u) top = fmaxf(top, t[u]);
            float acc = s[q] * gs_mix_exp2(m[q] - top);
#pragma unroll
            for (int u = 0; u < GS_MIX_BATCH; ++u) acc += gs_mix_exp2(t[u] - top);
            m[q] = top; s[q] = acc;
        }
    }
#pragma unroll
    for (int q = 0; q < GS_MIX_LANE_POINTS; ++q)
        if (p[q] < n_x) partial[(size_t)blockIdx.y * (size_t)n_x + (size_t)p[q]] = make_float2(m[q], finite[q] ? s[q] : NAN);
}

// out[p] = ln 2 (M + log2 sum_c s_c 2^(m_c - M)), M = max_c m_c; -inf where the sum is zero (no row takes part, or every term
// underflowed against a maximum no term reached)
__global__ void __launch_bounds__(256) k_mix_merge_density(const float2* __restrict__ partial, int n_chunks, int64_t n_x, float* __restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_x) return;
    float top = -FLT_MAX;
    for (int c = 0; c < n_chunks; ++c) top = fmaxf(top, partial[(size_t)c * (size_t)n_x + (size_t)p].x);
    double sum = 0.0;
    for (int c = 0; c < n_chunks; ++c) {
        const float2 ms = partial[(size_t)c * (size_t)n_x + (size_t)p];
        sum += (double)ms.y * exp2((double)ms.x - (double)top);
    }
    float result = NAN;
    if (sum > 0.0) result = gs_mix_round(((double)top + log2(sum)) * 0.69314718055994530942);
    else if (sum == 0.0) result = -INFINITY;
    out[p] = result;
}

// partial[chunk][k] = (re, im) of the chunk's records; NaN for a non-finite frequency
__global__ void __launch_bounds__(256) k_mix_fourier(const float4* __restrict__ rec, int64_t n_pad, int64_t units_per_chunk,
                                                     const float* __restrict__ k, int64_t n_k, float2* __restrict__ partial)
{
    int64_t p[GS_MIX_LANE_POINTS];
    float v[GS_MIX_LANE_POINTS][3], re[GS_MIX_LANE_POINTS], im[GS_MIX_LANE_POINTS];
    bool finite[GS_MIX_LANE_POINTS];
    gs_mix_load_queries(k, n_k, p, v, finite);
#pragma unroll
    for (int q = 0; q < GS_MIX_LANE_POINTS; ++q) { re[q] = 0.0f; im[q] = 0.0f; }
    const int64_t r0 = (int64_t)blockIdx.y * units_per_chunk * GS_MIX_CHUNK;
    const int64_t r1 = r0 + units_per_chunk * GS_MIX_CHUNK < n_pad ? r0 + units_per_chunk * GS_MIX_CHUNK : n_pad;
    for (int64_t i = r0; i < r1; i += GS_MIX_BATCH) {
        float r[GS_MIX_BATCH][GS_MIX_REC_FLOATS];
        gs_mix_load_batch(rec, i, r);
        bool any = false;
#pragma unroll
        for (int u = 0; u < GS_MIX_BATCH; ++u) any = any || r[u][3] > 0.0f;
        if (!any) continue;                                    // wave-uniform: none of the four has a weight
#pragma unroll
        for (int u = 0; u < GS_MIX_BATCH; ++u)
#pragma unroll
            for (int q = 0; q < GS_MIX_LANE_POINTS; ++q) gs_mix_fourier_term(r[u], v[q][0], v[q][1], v[q][2], &re[q], &im[q]);
    }
#pragma unroll
    for (int q = 0; q < GS_MIX_LANE_POINTS; ++q)
        if (p[q] < n_k) partial[(size_t)blockIdx.y * (size_t)n_k + (size_t)p[q]] = finite[q] ? make_float2(re[q], im[q]) : make_float2(NAN, NAN);
}

__global__ void __launch_bounds__(256) k_mix_merge_fourier(const float2* __restrict__ partial, int n_chunks, int64_t n_k, float2* __restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_k) return;
    double re = 0.0, im = 0.0;
    for (int c = 0; c < n_chunks; ++c) {
        const float2 v = partial[(size_t)c * (size_t)n_k + (size_t)p];
        re += (double)v.x; im += (double)v.y;
    }
    out[p] = make_float2((float)re, (float)im);
}

// ---- launch --------------------------------------------------------------------------------------------------------------------
// fourier == 0: out = n_q log-densities, centre unused; else out = n_q (re, im) pairs.  n_points and n_q are > 0; the three work
// buffers hold gs_mix_record_bytes / gs_mix_sum_bytes / gs_mix_partial_bytes.
// block_sums[n_blocks] = the sum of block_sums[0 .. n_blocks) in the fixed order of k_mix_sigma_total
void gs_launch_mix_total(double* block_sums, int64_t n_blocks, hipStream_t s)
{
    k_mix_sigma_total<<<1, 256, 0, s>>>(block_sums, n_blocks);
}

// The weights' sum and the records of a call (the first three launches of gs_launch_mixture; the backward calls read the same
// records).  -> where the sum lies in sum_ws; *n_pad_out = records written, a multiple of GS_MIX_CHUNK.
const double* gs_launch_mixture_records(const float* point_cloud, const float* features, const int8_t* invalid, int64_t n_points,
                                        int fourier, const float* centre, void* record_ws, void* sum_ws, int64_t* n_pad_out, hipStream_t s)
{
    const int64_t n_pad = gs_mix_units(n_points) * GS_MIX_CHUNK, blocks = gs_mix_sigma_blocks(n_points);
    double* sums = reinterpret_cast<double*>(sum_ws);
    k_mix_sigma_blocks<<<(unsigned)blocks, 256, 0, s>>>(point_cloud, features, invalid, n_points, sums);
    gs_launch_mix_total(sums, blocks, s);
    k_mix_records<<<(unsigned)(n_pad / 256), 256, 0, s>>>(point_cloud, features, invalid, n_points, n_pad, sums + blocks, fourier, centre,
                                                          reinterpret_cast<float4*>(record_ws));
    *n_pad_out = n_pad;
    return sums + blocks;
}

void gs_launch_mixture(const float* point_cloud, const float* features, const int8_t* invalid, int64_t n_points, const float* queries,
                       int64_t n_q, int fourier, const float* centre, float* out, void* record_ws, void* sum_ws, void* partial_ws, hipStream_t s)
{
    int64_t n_pad;
    gs_launch_mixture_records(point_cloud, features, invalid, n_points, fourier, centre, record_ws, sum_ws, &n_pad, s);
    float4* rec = reinterpret_cast<float4*>(record_ws);
    float2* partial = reinterpret_cast<float2*>(partial_ws);
    int64_t upc;
    const int n_chunks = gs_mix_chunks(n_points, n_q, &upc);
    const dim3 grid((unsigned)((n_q + GS_MIX_POINTS_PER_WG - 1) / GS_MIX_POINTS_PER_WG), (unsigned)n_chunks);
    const unsigned merge_blocks = (unsigned)((n_q + 255) / 256);
    if (fourier) {
        k_mix_fourier<<<grid, 256, 0, s>>>(rec, n_pad, upc, queries, n_q, partial);
        k_mix_merge_fourier<<<merge_blocks, 256, 0, s>>>(partial, n_chunks, n_q, reinterpret_cast<float2*>(out));
    } else {
        k_mix_density<<<grid, 256, 0, s>>>(rec, n_pad, upc, queries, n_q, partial);
        k_mix_merge_density<<<merge_blocks, 256, 0, s>>>(partial, n_chunks, n_q, out);
    }
}
