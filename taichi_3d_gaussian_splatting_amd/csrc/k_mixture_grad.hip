// k_mixture_grad.hip -- the gradients of the scene-as-mixture evaluations (include/gs_mixture_grad.h): of the log-density at
// points and of the Fourier transform at frequencies, to mu, q, log s and the opacity logit of every row, and of the log-density
// to the points.  The transpose of k_mixture.hip's pair loop: the same P x N pairs, each adding its weight times (1, y, y y^T)
// to ten sums of its ROW, so here the lanes own the rows and the queries arrive wave-uniform.  The arithmetic of a pair and of a
// row is gs_mixture_math.h; the records are the forward's (gs_launch_mixture_records).
//
//   k_mixg_log2p         (density) log2 p of every query again, from the same base-2 exponents t the shares are formed with, every
//                        2^(t - m) added in float64.  The caller's log p has been rounded to f32 in another base (2^-24 |log p| in
//                        every share) and its sum is an f32 sum as long as a chunk; neither matters to log p, both would to
//                        2^(t - log2 p).  Grid (query blocks) x (component chunks) like k_mixg_density_x; the chunks' (m, s) are
//                        merged in ascending order inside k_mixg_queries.
//   k_mixg_queries       one 32-byte record per query: x | g | log2 p as hi + lo (density), k | g_re | g_im (transform); all zero
//                        for a query that contributes nothing.  Density: the sum of g over the others per block of 256 (float64 tree).
//   k_mixg_rows          grid (row blocks) x (query chunks).  A lane owns GS_MIXG_LANE_COMPONENTS rows: their records and 2 x 10
//                        f32 sums sit in VGPRs, the query records are read at wave-uniform addresses (scalar loads).  After every
//                        GS_MIXG_RUN queries the f32 sums are added into float64 ones and cleared, so no f32 sum is longer than
//                        GS_MIXG_RUN terms.  A query whose record is zero is skipped by a wave-uniform branch.
//   k_mixg_merge         the chunk partials of a row in ascending chunk order (float64); transform: the block sums of sum A.
//   k_mixg_tail          gs_mix_grad_row per row: columns 0..7 of the feature gradient and the position gradient, zero for a row
//                        that takes no part.
//   k_mixg_density_x / k_mixg_merge_x
//                        d log p / dx, a pass of the forward's shape (queries in lanes, records wave-uniform, the component loop
//                        split by the forward's rule), f32 runs of GS_MIXG_RUN records flushed into float64, chunks merged in order.
//
// Both splits read (n_points, n_q) only.  Nothing here uses an atomic.
#include "gs_common.h"
#include "gs_mixture_math.h"

#include <cfloat>

#define GS_MIXG_LANE_COMPONENTS 2       // rows per lane: two independent chains
#define GS_MIXG_LANES 128               // lanes of a workgroup of k_mixg_rows
#define GS_MIXG_COMPONENTS_PER_WG 256   // rows per workgroup: GS_MIXG_LANES x GS_MIXG_LANE_COMPONENTS
#define GS_MIXG_QUERY_CHUNK 256         // queries per unit of the query loop: a chunk of it is a whole number of these
#define GS_MIXG_RUN 32                  // queries (k_mixg_rows) or records (k_mixg_density_x) per f32 run
#define GS_MIXG_TARGET_WGS 2048         // workgroups the grid aims at when few row blocks exist
#define GS_MIXG_MAX_QUERY_CHUNKS 64
#define GS_MIXG_MAX_COMPONENT_CHUNKS 1024
#define GS_MIXG_QREC_FLOATS 8
#define GS_MIXG_X_POINTS_PER_WG 512     // queries per workgroup of k_mixg_density_x: 256 lanes x 2 (the forward's blocking)
static_assert(GS_MIXG_COMPONENTS_PER_WG == GS_MIXG_LANES * GS_MIXG_LANE_COMPONENTS, "a workgroup is GS_MIXG_LANES lanes");
static_assert(GS_MIXG_QUERY_CHUNK % GS_MIXG_RUN == 0 && GS_MIXG_RUN % GS_MIX_BATCH == 0, "a unit is a whole number of runs");

static int64_t gs_mixg_row_blocks(int64_t n_pad) { return (n_pad + GS_MIXG_COMPONENTS_PER_WG - 1) / GS_MIXG_COMPONENTS_PER_WG; }
static int64_t gs_mixg_pad(int64_t n_points) { return (int64_t)(gs_mix_record_bytes(n_points) / (GS_MIX_REC_FLOATS * sizeof(float))); }
static int64_t gs_mixg_blocks256(int64_t n) { return (n + 255) / 256; }

// How the query loop of k_mixg_rows is split: -> number of chunks, *units_per_chunk units of GS_MIXG_QUERY_CHUNK queries in each
// (the last may hold fewer).  A function of (n_points, n_q) alone.
static int gs_mixg_query_chunks(int64_t n_points, int64_t n_q, int64_t* units_per_chunk)
{
    const int64_t row_blocks = gs_mixg_row_blocks(gs_mixg_pad(n_points));
    const int64_t units = (n_q + GS_MIXG_QUERY_CHUNK - 1) / GS_MIXG_QUERY_CHUNK;
    int64_t want = GS_MIXG_TARGET_WGS / row_blocks;
    want = want > GS_MIXG_MAX_QUERY_CHUNKS ? GS_MIXG_MAX_QUERY_CHUNKS : want;
    want = want > units ? units : want;
    want = want < 1 ? 1 : want;
    const int64_t upc = (units + want - 1) / want;
    *units_per_chunk = upc;
    return (int)((units + upc - 1) / upc);
}

// How the component loop of k_mixg_density_x is split (the rule of the forward's gs_mix_chunks, in units of
// GS_MIXG_COMPONENTS_PER_WG records): a function of (n_points, n_x) alone.
static int gs_mixg_component_chunks(int64_t n_points, int64_t n_x, int64_t* units_per_chunk)
{
    const int64_t units = gs_mixg_row_blocks(gs_mixg_pad(n_points)), qblocks = (n_x + GS_MIXG_X_POINTS_PER_WG - 1) / GS_MIXG_X_POINTS_PER_WG;
    int64_t want = (GS_MIXG_TARGET_WGS + qblocks - 1) / qblocks;
    want = want > GS_MIXG_MAX_COMPONENT_CHUNKS ? GS_MIXG_MAX_COMPONENT_CHUNKS : want;
    want = want > units ? units : want;
    want = want < 1 ? 1 : want;
    const int64_t upc = (units + want - 1) / want;
    *units_per_chunk = upc;
    return (int)((units + upc - 1) / upc);
}

size_t gs_mixg_query_bytes(int64_t n_q) { return (size_t)n_q * GS_MIXG_QREC_FLOATS * sizeof(float); }
size_t gs_mixg_partial_bytes(int64_t n_points, int64_t n_q)
{
    int64_t upc;
    return (size_t)gs_mixg_query_chunks(n_points, n_q, &upc) * GS_MIX_GRAD_SUMS * (size_t)gs_mixg_pad(n_points) * sizeof(double);
}
size_t gs_mixg_sum_bytes(int64_t n_points, int64_t n_q)
{
    const int64_t a = gs_mixg_blocks256(n_q), b = gs_mixg_blocks256(gs_mixg_pad(n_points));
    return (size_t)((a > b ? a : b) + 1) * sizeof(double);
}
size_t gs_mixg_x_partial_bytes(int64_t n_points, int64_t n_x)
{
    int64_t upc;
    return (size_t)gs_mixg_component_chunks(n_points, n_x, &upc) * 3 * (size_t)n_x * sizeof(double);
}

// ---- log2 p again ------------------------------------------------------------------------------------------------------------------
// the queries of this lane of the two kernels that keep queries in lanes: row p of x, the last row where p is past the end
__device__ __forceinline__ void gs_mixg_lane_queries(const float* __restrict__ x, int64_t n_x, int64_t (&p)[2], float (&v)[2][3])
{
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        p[q] = (int64_t)blockIdx.x * GS_MIXG_X_POINTS_PER_WG + q * 256 + threadIdx.x;
        const int64_t i = p[q] < n_x ? p[q] : n_x - 1;
        v[q][0] = x[3 * i]; v[q][1] = x[3 * i + 1]; v[q][2] = x[3 * i + 2];
    }
}

// partial[chunk][0][p] = m, the largest base-2 exponent of the chunk's records, partial[chunk][1][p] = s = sum 2^(t - m): the terms
// are f32 (gs_mix_density_term and gs_mix_exp2, the forward's), their sum is float64.  m moves once per GS_MIX_BATCH records.
__global__ void __launch_bounds__(256) k_mixg_log2p(const float4* __restrict__ rec, int64_t n_pad, int64_t units_per_chunk,
                                                    const float* __restrict__ x, int64_t n_x, double* __restrict__ partial)
{
    int64_t p[2];
    float v[2][3], m[2];
    double s[2];
    gs_mixg_lane_queries(x, n_x, p, v);
#pragma unroll
    for (int q = 0; q < 2; ++q) { m[q] = -FLT_MAX; s[q] = 0.0; }
    const int64_t r0 = (int64_t)blockIdx.y * units_per_chunk * GS_MIXG_COMPONENTS_PER_WG;
    const int64_t r1 = r0 + units_per_chunk * GS_MIXG_COMPONENTS_PER_WG < n_pad ? r0 + units_per_chunk * GS_MIXG_COMPONENTS_PER_WG : n_pad;
    for (int64_t i = r0; i < r1; i += GS_MIX_BATCH) {
        float r[GS_MIX_BATCH][GS_MIX_REC_FLOATS];
        gs_mix_load_batch(rec, i, r);
        bool any = false;
#pragma unroll
        for (int u = 0; u < GS_MIX_BATCH; ++u) any = any || r[u][3] > -INFINITY;
        if (!any) continue;                                    // wave-uniform: none of the four takes part
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float t[GS_MIX_BATCH];
#pragma unroll
            for (int u = 0; u < GS_MIX_BATCH; ++u) t[u] = gs_mix_density_term(r[u], v[q][0], v[q][1], v[q][2]);
            float top = m[q];                                  // fmaxf keeps the number where a term is NaN; the sum then becomes NaN
#pragma unroll
            for (int u = 0; u < GS_MIX_BATCH; ++u) top = fmaxf(top, t[u]);
            double acc = s[q] * (double)gs_mix_exp2(m[q] - top);          // exactly s while the maximum stays
#pragma unroll
            for (int u = 0; u < GS_MIX_BATCH; ++u) acc += (double)gs_mix_exp2(t[u] - top);
            m[q] = top; s[q] = acc;
        }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
        if (p[q] < n_x) {
            partial[((size_t)blockIdx.y * 2) * (size_t)n_x + (size_t)p[q]] = (double)m[q];
            partial[((size_t)blockIdx.y * 2 + 1) * (size_t)n_x + (size_t)p[q]] = s[q];
        }
}

// log2 p of query p from the chunks' (m, s) in ascending order: M + log2 sum_c s_c 2^(m_c - M); -inf where the sum is zero, NaN
// where a term was
__device__ __forceinline__ double gs_mixg_merged_log2p(const double* __restrict__ partial, int n_chunks, int64_t n_x, int64_t p)
{
    double top = -(double)FLT_MAX;
    for (int c = 0; c < n_chunks; ++c) top = fmax(top, partial[((size_t)c * 2) * (size_t)n_x + (size_t)p]);
    double sum = 0.0;
    for (int c = 0; c < n_chunks; ++c)
        sum += partial[((size_t)c * 2 + 1) * (size_t)n_x + (size_t)p] * exp2(partial[((size_t)c * 2) * (size_t)n_x + (size_t)p] - top);
    if (sum > 0.0) return top + log2(sum);
    return sum == 0.0 ? -(double)INFINITY : (double)NAN;
}

// ---- the queries' records ----------------------------------------------------------------------------------------------------------
// A query contributes if its coordinates are finite, its upstream gradient is not exactly zero and (density) its forward value
// is finite (log_p: what the caller holds; log2_partial: the chunks of k_mixg_log2p).  block_sums (density only): the sum of g over the block's contributing queries.
__global__ void __launch_bounds__(256) k_mixg_queries(const float* __restrict__ q, int64_t n_q, int fourier, const float* __restrict__ log_p,
                                                      const double* __restrict__ log2_partial, int log2_chunks, const float* __restrict__ grad, float4* __restrict__ qrec, double* __restrict__ block_sums)
{
    __shared__ double lds[256];
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double g_sum = 0.0;
    if (p < n_q) {
        const float x = q[3 * p], y = q[3 * p + 1], z = q[3 * p + 2];
        bool ok = gs_mix_finite(x) && gs_mix_finite(y) && gs_mix_finite(z);
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
        if (fourier) {
            const float g_re = grad[2 * p], g_im = grad[2 * p + 1];
            ok = ok && (g_re != 0.0f || g_im != 0.0f);
            if (ok) { a = make_float4(x, y, z, g_re); b.x = g_im; }
        } else {
            const float g = grad[p];
            const double l2 = gs_mixg_merged_log2p(log2_partial, log2_chunks, n_q, p);
            ok = ok && g != 0.0f && gs_mix_finite(log_p[p]) && fabs(l2) <= (double)FLT_MAX;
            if (ok) {
                const float hi = (float)l2, lo = (float)(l2 - (double)hi);
                a = make_float4(x, y, z, g);
                b.x = hi; b.y = lo;
                g_sum = (double)g;
            }
        }
        qrec[2 * p] = a; qrec[2 * p + 1] = b;
    }
    if (!fourier) {
        const double sum = gs_mix_block_sum(g_sum, lds);
        if (threadIdx.x == 0) block_sums[blockIdx.x] = sum;
    }
}

// ---- the rows' sums ------------------------------------------------------------------------------------------------------------------
// partial[chunk][j][row], j < GS_MIX_GRAD_SUMS: the chunk's queries, in ascending order, in f32 runs of GS_MIXG_RUN
template <int FOURIER>
__global__ void __launch_bounds__(GS_MIXG_LANES) k_mixg_rows(const float4* __restrict__ rec, int64_t n_pad, const float4* __restrict__ qrec,
                                                             int64_t n_q, int64_t units_per_chunk, double* __restrict__ partial)
{
    float r[GS_MIXG_LANE_COMPONENTS][GS_MIX_REC_FLOATS];
    double total[GS_MIXG_LANE_COMPONENTS][GS_MIX_GRAD_SUMS];
    int64_t row[GS_MIXG_LANE_COMPONENTS];
#pragma unroll
    for (int u = 0; u < GS_MIXG_LANE_COMPONENTS; ++u) {
        row[u] = (int64_t)blockIdx.x * GS_MIXG_COMPONENTS_PER_WG + u * GS_MIXG_LANES + threadIdx.x;
        const int64_t i = row[u] < n_pad ? row[u] : n_pad - 1;              // past the end: computed, never written
        const float4 a = rec[4 * i], b = rec[4 * i + 1], c = rec[4 * i + 2], d = rec[4 * i + 3];
        r[u][0] = a.x; r[u][1] = a.y; r[u][2] = a.z; r[u][3] = a.w;
        r[u][4] = b.x; r[u][5] = b.y; r[u][6] = b.z; r[u][7] = b.w;
        r[u][8] = c.x; r[u][9] = c.y; r[u][10] = c.z; r[u][11] = c.w;
        r[u][12] = d.x; r[u][13] = 0.0f; r[u][14] = 0.0f; r[u][15] = 0.0f;
#pragma unroll
        for (int j = 0; j < GS_MIX_GRAD_SUMS; ++j) total[u][j] = 0.0;
    }
    const int64_t q0 = (int64_t)blockIdx.y * units_per_chunk * GS_MIXG_QUERY_CHUNK;
    const int64_t q1 = q0 + units_per_chunk * GS_MIXG_QUERY_CHUNK < n_q ? q0 + units_per_chunk * GS_MIXG_QUERY_CHUNK : n_q;
    for (int64_t run = q0; run < q1; run += GS_MIXG_RUN) {
        float acc[GS_MIXG_LANE_COMPONENTS][GS_MIX_GRAD_SUMS];
#pragma unroll
        for (int u = 0; u < GS_MIXG_LANE_COMPONENTS; ++u)
#pragma unroll
            for (int j = 0; j < GS_MIX_GRAD_SUMS; ++j) acc[u][j] = 0.0f;
        const int64_t end = run + GS_MIXG_RUN < q1 ? run + GS_MIXG_RUN : q1;
        for (int64_t q = run; q < end; ++q) {
            const float4 a = qrec[2 * q], b = qrec[2 * q + 1];              // wave-uniform
            if (a.w == 0.0f && (!FOURIER || b.x == 0.0f)) continue;         // contributes nothing
#pragma unroll
            for (int u = 0; u < GS_MIXG_LANE_COMPONENTS; ++u) {
                if (FOURIER) gs_mix_fourier_grad_term(r[u], a.x, a.y, a.z, a.w, b.x, acc[u]);
                else gs_mix_density_grad_term(r[u], a.x, a.y, a.z, a.w, b.x, b.y, acc[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < GS_MIXG_LANE_COMPONENTS; ++u)
#pragma unroll
            for (int j = 0; j < GS_MIX_GRAD_SUMS; ++j) total[u][j] += (double)acc[u][j];
    }
#pragma unroll
    for (int u = 0; u < GS_MIXG_LANE_COMPONENTS; ++u)
        if (row[u] < n_pad)
#pragma unroll
            for (int j = 0; j < GS_MIX_GRAD_SUMS; ++j)
                partial[((size_t)blockIdx.y * GS_MIX_GRAD_SUMS + j) * (size_t)n_pad + (size_t)row[u]] = total[u][j];
}

// partial[0][j][row] = the sum over the chunks in ascending order; transform: block_sums[block] = the block's sum of sums[0]
__global__ void __launch_bounds__(256) k_mixg_merge(double* __restrict__ partial, int n_chunks, int64_t n_pad, int fourier,
                                                    double* __restrict__ block_sums)
{
    __shared__ double lds[256];
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double first = 0.0;
    if (row < n_pad) {
        for (int j = 0; j < GS_MIX_GRAD_SUMS; ++j) {
            double sum = 0.0;
            for (int c = 0; c < n_chunks; ++c) sum += partial[((size_t)c * GS_MIX_GRAD_SUMS + j) * (size_t)n_pad + (size_t)row];
            partial[(size_t)j * (size_t)n_pad + (size_t)row] = sum;
            if (j == 0) first = sum;
        }
    }
    if (fourier) {
        const double sum = gs_mix_block_sum(first, lds);
        if (threadIdx.x == 0) block_sums[blockIdx.x] = sum;
    }
}

__global__ void __launch_bounds__(256) k_mixg_tail(const float* __restrict__ mu, const float* __restrict__ feat, const int8_t* __restrict__ mask,
                                                   int64_t n, int64_t n_pad, const double* __restrict__ sigma_total, int fourier,
                                                   const double* __restrict__ sums, const double* __restrict__ scalar,
                                                   float* __restrict__ grad_mu, float* __restrict__ grad_feat)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double row_sums[GS_MIX_GRAD_SUMS];
#pragma unroll
    for (int j = 0; j < GS_MIX_GRAD_SUMS; ++j) row_sums[j] = sums[(size_t)j * (size_t)n_pad + (size_t)i];
    float g_mu[3], g_head[8];
    gs_mix_grad_row(feat + GS_MIX_NFEAT * i, gs_mix_takes_part(mu + 3 * i, feat + GS_MIX_NFEAT * i, mask, i), sigma_total[0], fourier != 0,
                    row_sums, scalar[0], g_mu, g_head);
#pragma unroll
    for (int j = 0; j < 3; ++j) grad_mu[3 * i + j] = g_mu[j];
#pragma unroll
    for (int j = 0; j < 8; ++j) grad_feat[GS_MIX_NFEAT * i + j] = g_head[j];
}

// ---- d log p / dx ----------------------------------------------------------------------------------------------------------------------
// partial[chunk][c][p], c < 3: sum over the chunk's records of (pi N / p) A'^T y'
__global__ void __launch_bounds__(256) k_mixg_density_x(const float4* __restrict__ rec, int64_t n_pad, int64_t units_per_chunk,
                                                        const float4* __restrict__ qrec, int64_t n_x, double* __restrict__ partial)
{
    int64_t p[2];
    float v[2][3], hi[2], lo[2];
    double total[2][3];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        p[q] = (int64_t)blockIdx.x * GS_MIXG_X_POINTS_PER_WG + q * 256 + threadIdx.x;
        const int64_t i = p[q] < n_x ? p[q] : n_x - 1;
        const float4 a = qrec[2 * i], b = qrec[2 * i + 1];
        v[q][0] = a.x; v[q][1] = a.y; v[q][2] = a.z; hi[q] = b.x; lo[q] = b.y;
        total[q][0] = total[q][1] = total[q][2] = 0.0;
    }
    const int64_t r0 = (int64_t)blockIdx.y * units_per_chunk * GS_MIXG_COMPONENTS_PER_WG;
    const int64_t r1 = r0 + units_per_chunk * GS_MIXG_COMPONENTS_PER_WG < n_pad ? r0 + units_per_chunk * GS_MIXG_COMPONENTS_PER_WG : n_pad;
    for (int64_t run = r0; run < r1; run += GS_MIXG_RUN) {
        float acc[2][3] = { { 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f } };
        const int64_t end = run + GS_MIXG_RUN < r1 ? run + GS_MIXG_RUN : r1;
        for (int64_t i = run; i < end; i += GS_MIX_BATCH) {
            float r[GS_MIX_BATCH][GS_MIX_REC_FLOATS];
            gs_mix_load_batch(rec, i, r);
            bool any = false;
#pragma unroll
            for (int u = 0; u < GS_MIX_BATCH; ++u) any = any || r[u][3] > -INFINITY;
            if (!any) continue;                                    // wave-uniform: none of the four takes part
#pragma unroll
            for (int u = 0; u < GS_MIX_BATCH; ++u)
#pragma unroll
                for (int q = 0; q < 2; ++q) gs_mix_density_grad_x_term(r[u], v[q][0], v[q][1], v[q][2], hi[q], lo[q], acc[q]);
        }
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) total[q][c] += (double)acc[q][c];
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
        if (p[q] < n_x)
#pragma unroll
            for (int c = 0; c < 3; ++c) partial[((size_t)blockIdx.y * 3 + c) * (size_t)n_x + (size_t)p[q]] = total[q][c];
}

// grad_x[p] = -2 ln 2 g_p (the chunks in ascending order); 0 for a query that contributes nothing
__global__ void __launch_bounds__(256) k_mixg_merge_x(const double* __restrict__ partial, int n_chunks, const float4* __restrict__ qrec,
                                                      int64_t n_x, float* __restrict__ grad_x)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_x) return;
    const float g = qrec[2 * p].w;
    for (int c = 0; c < 3; ++c) {
        double sum = 0.0;
        for (int k = 0; k < n_chunks; ++k) sum += partial[((size_t)k * 3 + c) * (size_t)n_x + (size_t)p];
        grad_x[3 * p + c] = g != 0.0f ? gs_mix_round(-1.38629436111989061883 * (double)g * sum) : 0.0f;
    }
}

// ---- launch --------------------------------------------------------------------------------------------------------------------------
// n_points and n_q are > 0.  fourier == 0: grad_out = n_q floats, log_density the forward's output, grad_x (n_q,3) or NULL;
// else grad_out = n_q (re, im) pairs, log_density and grad_x unused.
void gs_launch_mixture_grad(const float* point_cloud, const float* features, const int8_t* invalid, int64_t n_points, const float* queries,
                            int64_t n_q, int fourier, const float* centre, const float* log_density, const float* grad_out,
                            float* grad_point_cloud, float* grad_features, float* grad_x, void* record_ws, void* sum_ws, void* query_ws,
                            void* partial_ws, void* gsum_ws, void* x_partial_ws, hipStream_t s)
{
    int64_t n_pad;
    const double* sigma_total = gs_launch_mixture_records(point_cloud, features, invalid, n_points, fourier, centre, record_ws, sum_ws, &n_pad, s);
    const float4* rec = reinterpret_cast<const float4*>(record_ws);
    float4* qrec = reinterpret_cast<float4*>(query_ws);
    double* partial = reinterpret_cast<double*>(partial_ws);
    double* gsums = reinterpret_cast<double*>(gsum_ws);
    const int64_t q_blocks = gs_mixg_blocks256(n_q), row_blocks256 = gs_mixg_blocks256(n_pad);
    // the density's two passes with queries in lanes share one split of the component loop and one buffer: log2 p's (m, s) are
    // consumed by k_mixg_queries before k_mixg_density_x writes its partials there
    double* x_partial = reinterpret_cast<double*>(x_partial_ws);
    int64_t x_upc = 0;
    const int x_chunks = fourier ? 0 : gs_mixg_component_chunks(n_points, n_q, &x_upc);
    const dim3 x_grid((unsigned)((n_q + GS_MIXG_X_POINTS_PER_WG - 1) / GS_MIXG_X_POINTS_PER_WG), (unsigned)(x_chunks > 0 ? x_chunks : 1));
    if (!fourier) k_mixg_log2p<<<x_grid, 256, 0, s>>>(rec, n_pad, x_upc, queries, n_q, x_partial);
    k_mixg_queries<<<(unsigned)q_blocks, 256, 0, s>>>(queries, n_q, fourier, log_density, x_partial, x_chunks, grad_out, qrec, gsums);
    int64_t upc;
    const int n_chunks = gs_mixg_query_chunks(n_points, n_q, &upc);
    const dim3 grid((unsigned)gs_mixg_row_blocks(n_pad), (unsigned)n_chunks);
    int64_t scalar_blocks = q_blocks;
    if (fourier) {
        k_mixg_rows<1><<<grid, GS_MIXG_LANES, 0, s>>>(rec, n_pad, qrec, n_q, upc, partial);
        scalar_blocks = row_blocks256;
    } else {
        gs_launch_mix_total(gsums, q_blocks, s);                 // sum g over the queries that contribute
        k_mixg_rows<0><<<grid, GS_MIXG_LANES, 0, s>>>(rec, n_pad, qrec, n_q, upc, partial);
    }
    k_mixg_merge<<<(unsigned)row_blocks256, 256, 0, s>>>(partial, n_chunks, n_pad, fourier, gsums);
    if (fourier) gs_launch_mix_total(gsums, row_blocks256, s);
    k_mixg_tail<<<(unsigned)gs_mixg_blocks256(n_points), 256, 0, s>>>(point_cloud, features, invalid, n_points, n_pad, sigma_total, fourier,
                                                                      partial, gsums + scalar_blocks, grad_point_cloud, grad_features);
    if (!fourier && grad_x) {
        k_mixg_density_x<<<x_grid, 256, 0, s>>>(rec, n_pad, x_upc, qrec, n_q, x_partial);
        k_mixg_merge_x<<<(unsigned)q_blocks, 256, 0, s>>>(x_partial, x_chunks, qrec, n_q, grad_x);
    }
}
