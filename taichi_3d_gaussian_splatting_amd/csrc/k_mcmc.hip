// k_mcmc.hip -- fixed-budget densification (include/gs_mcmc.h, which states every rule to the parenthesis).
//
//   gs_mcmc_noise        k_mcmc_noise         N-pass, one thread per row: gate, one Philox draw, Sigma z, x += delta
//   gs_mcmc_regulariser  k_mcmc_reg_partial   N-pass: float64 sums of opacity and scale per block, fixed tree
//                        k_mcmc_reg_total     one block over the partials: the totals, value_and_count
//                        k_mcmc_reg_grad      N-pass: the four columns of every valid row, +=
//   gs_mcmc_relocate     k_mcmc_classify      N-pass: class and weight per row, in-block prefix of the weights, per-block sums
//                        k_mcmc_scan          one block: prefixes over the blocks, W, the budget, counts[]
//                        k_mcmc_destinations  N-pass: the dead rows, then the first n_new free rows, ascending
//                        k_mcmc_sample        one thread per destination: draw, two binary searches, multiplicity
//                        k_mcmc_apply_dest    one thread per destination: the source's row with the new opacity and scale
//                        k_mcmc_apply_src     N-pass: the sources themselves, after every destination has read them
//
// No float atomics, no host waits: the counts a host would read (D, n_new, V) are read on the device by the next kernel.
#include "gs_point_math.h"
#include "gs_random.h"
#include "../../include/gs_mcmc.h"

#include <algorithm>

#define MC_BLOCK GS_MCMC_BLOCK
#define MC_WAVES (MC_BLOCK / 64)
#define MC_SCAN_THREADS 1024
#define MC_NBLK(N) (((N) + MC_BLOCK - 1) / MC_BLOCK)
#define MC_F4_PER_ROW (GS_NFEAT / 4)
static_assert(256ull * (GS_MCMC_WEIGHT_ONE - 1) < (1ull << 32), "a block's weights must fit uint32");

enum { MC_OTHER = 0, MC_ALIVE = 1, MC_DEAD = 2, MC_FREE = 3 };

// What the relocation keeps between its launches, at the head of plan->scratch.
struct McHeader { unsigned long long W; long long dead, n_new, D; };
// scratch: [McHeader, padded to 64 B][uint64 nb: weight prefix][int32 4 nb: dead, free, valid, alive][uint32 N: in-block prefix][uint8 N: class]
struct McScratch { McHeader* hdr; unsigned long long* wpre; int32_t* cnt; uint32_t* excl; uint8_t* cls; };
__host__ __device__ static inline McScratch mc_scratch(void* p, int64_t N)
{
    const int64_t nb = MC_NBLK(N);
    char* c = static_cast<char*>(p);
    McScratch s;
    s.hdr = reinterpret_cast<McHeader*>(c);
    s.wpre = reinterpret_cast<unsigned long long*>(c + 64);
    s.cnt = reinterpret_cast<int32_t*>(c + 64 + 8 * nb);
    s.excl = reinterpret_cast<uint32_t*>(c + 64 + 24 * nb);
    s.cls = reinterpret_cast<uint8_t*>(c + 64 + 24 * nb + 4 * N);
    return s;
}
size_t gs_mcmc_scratch_size(int64_t N) { return (size_t)(64 + 24 * MC_NBLK(N) + 5 * N + 16); }
size_t gs_mcmc_reg_ws_size(int64_t N) { return (size_t)(64 + 24 * MC_NBLK(N)); }

// in-block exclusive prefix sum of v in row order (uint32: see the static_assert) and the block's total, from gs_common.h's scan halves
__device__ __forceinline__ uint32_t mc_block_prefix(uint32_t v, uint32_t* s_wave, unsigned long long* total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t incl = gs_wave_scan_incl(v, lane);
    gs_block_scan_put(s_wave, w, lane, incl);
    __syncthreads();
    const uint32_t before = gs_block_scan_excl(s_wave, w, incl, v);
    *total = gs_block_sum<MC_WAVES>(s_wave);
    __syncthreads();
    return before;
}

__device__ __forceinline__ bool mc_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }      // false for NaN and +-inf

// ---- noise ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_BLOCK) void k_mcmc_noise(float* __restrict__ pc, const float4* __restrict__ feat4,
                                                         const int8_t* __restrict__ mask, int64_t N, float noise_scale, float gate_k,
                                                         float gate_x0, uint32_t key0, uint32_t key1, uint32_t step_index)
{
    const int64_t n = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (n >= N || mask[n] != 0) return;
    const float4 a = feat4[(size_t)n * MC_F4_PER_ROW], b = feat4[(size_t)n * MC_F4_PER_ROW + 1];
    const float row[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
    const float o = gs_sigmoid(row[7]);
    const float g = 1.0f / (1.0f + gs_expf(-(gate_k * ((1.0f - o) - gate_x0))));
    const float s = g * noise_scale;
    float z[3];
    gs_normal3(gs_philox4x32_10(make_uint4((uint32_t)n, step_index, GS_MCMC_STREAM_NOISE, 0u), key0, key1), z);
    float Sigma[9];
    gs_sigma_from_row(row, Sigma);
    const float v[3] = { z[0] * s, z[1] * s, z[2] * s };
    float delta[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) delta[i] = (Sigma[3 * i] * v[0] + Sigma[3 * i + 1] * v[1]) + Sigma[3 * i + 2] * v[2];
    if (!(mc_finite(delta[0]) && mc_finite(delta[1]) && mc_finite(delta[2]))) return;
#pragma unroll
    for (int i = 0; i < 3; ++i) pc[3 * n + i] = pc[3 * n + i] + delta[i];
}

// ---- regulariser ------------------------------------------------------------------------------------------------------
struct McRegTotals { double So, Ss; long long V; };

__global__ __launch_bounds__(MC_BLOCK) void k_mcmc_reg_partial(const float* __restrict__ feat, const int8_t* __restrict__ mask, int64_t N,
                                                               double* __restrict__ po, double* __restrict__ ps, long long* __restrict__ pv)
{
    __shared__ double s_o[MC_BLOCK], s_s[MC_BLOCK];
    __shared__ int s_wave[MC_WAVES];
    const int64_t n = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    const bool valid = n < N && mask[n] == 0;
    double o = 0.0, e = 0.0;
    if (valid) {
        const float4 b = reinterpret_cast<const float4*>(feat)[(size_t)n * MC_F4_PER_ROW + 1];
        o = (double)gs_sigmoid(b.w);
        e = ((double)gs_expf(b.x) + (double)gs_expf(b.y)) + (double)gs_expf(b.z);
    }
    s_o[threadIdx.x] = o;
    s_s[threadIdx.x] = e;
    int total;
    (void)gs_block_rank<MC_WAVES>(valid, s_wave, &total);                 // (its barriers order the stores above too)
    for (int d = MC_BLOCK / 2; d > 0; d >>= 1) {                // a fixed tree: the same bits on every run
        if ((int)threadIdx.x < d) { s_o[threadIdx.x] += s_o[threadIdx.x + d]; s_s[threadIdx.x] += s_s[threadIdx.x + d]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { po[blockIdx.x] = s_o[0]; ps[blockIdx.x] = s_s[0]; pv[blockIdx.x] = total; }
}

__global__ __launch_bounds__(MC_SCAN_THREADS) void k_mcmc_reg_total(const double* __restrict__ po, const double* __restrict__ ps,
                                                                    const long long* __restrict__ pv, int nb, float lambda_opacity,
                                                                    float lambda_scale, McRegTotals* __restrict__ totals,
                                                                    float* __restrict__ value_and_count)
{
    __shared__ double s_o[MC_SCAN_THREADS], s_s[MC_SCAN_THREADS];
    __shared__ long long s_v[MC_SCAN_THREADS];
    const int t = threadIdx.x;
    const int per = (nb + MC_SCAN_THREADS - 1) / MC_SCAN_THREADS;
    const int lo = min(nb, t * per), hi = min(nb, lo + per);
    double o = 0.0, e = 0.0;
    long long v = 0;
    for (int i = lo; i < hi; ++i) { o += po[i]; e += ps[i]; v += pv[i]; }
    s_o[t] = o; s_s[t] = e; s_v[t] = v;
    __syncthreads();
    for (int d = MC_SCAN_THREADS / 2; d > 0; d >>= 1) {
        if (t < d) { s_o[t] += s_o[t + d]; s_s[t] += s_s[t + d]; s_v[t] += s_v[t + d]; }
        __syncthreads();
    }
    if (t != 0) return;
    const long long V = s_v[0];
    totals->So = s_o[0]; totals->Ss = s_s[0]; totals->V = V;
    if (value_and_count) {
        value_and_count[0] = V > 0 ? (float)((double)lambda_opacity * s_o[0] / (double)V) : 0.0f;
        value_and_count[1] = V > 0 ? (float)((double)lambda_scale * s_s[0] / (3.0 * (double)V)) : 0.0f;
        value_and_count[2] = (float)V;
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_mcmc_reg_grad(const float* __restrict__ feat, const int8_t* __restrict__ mask, int64_t N,
                                                            float lambda_opacity, float lambda_scale, const float* __restrict__ upstream,
                                                            const McRegTotals* __restrict__ totals, float* __restrict__ grad)
{
    const long long V = totals->V;
    const int64_t n = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (V <= 0 || n >= N || mask[n] != 0) return;
    const float up = upstream ? *upstream : 1.0f;
    const float Vf = (float)V;
    const float co = (up * lambda_opacity) / Vf, cs = (up * lambda_scale) / (3.0f * Vf);
    const float4 b = reinterpret_cast<const float4*>(feat)[(size_t)n * MC_F4_PER_ROW + 1];
    float4* g4 = reinterpret_cast<float4*>(grad) + (size_t)n * MC_F4_PER_ROW + 1;
    const float o = gs_sigmoid(b.w);
    float4 g = *g4;
    g.x = g.x + cs * gs_expf(b.x);
    g.y = g.y + cs * gs_expf(b.y);
    g.z = g.z + cs * gs_expf(b.z);
    g.w = g.w + co * (o * (1.0f - o));
    *g4 = g;
}

// ---- relocation -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_BLOCK) void k_mcmc_classify(const float* __restrict__ feat, const int8_t* __restrict__ mask, int64_t N,
                                                            float min_opacity_logit, McScratch ws)
{
    __shared__ int s_wave[MC_WAVES];
    __shared__ uint32_t s_sum[MC_WAVES];
    const int64_t n = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    int cls = MC_OTHER;
    uint32_t w = 0;
    if (n < N) {
        const int8_t m = mask[n];
        if (m == 1) cls = MC_FREE;
        else if (m == 0) {
            const float logit = feat[(size_t)n * GS_NFEAT + 7];
            if (logit > min_opacity_logit) {
                cls = MC_ALIVE;
                const int wi = (int)floorf(gs_sigmoid(logit) * (float)GS_MCMC_WEIGHT_ONE);
                w = (uint32_t)min(max(wi, 1), GS_MCMC_WEIGHT_ONE - 1);
            } else cls = MC_DEAD;                                   // a NaN logit too
        }
    }
    unsigned long long wsum;
    const uint32_t before = mc_block_prefix(w, s_sum, &wsum);
    if (n < N) { ws.excl[n] = before; ws.cls[n] = (uint8_t)cls; }
    const int nb = gridDim.x;
    const bool preds[4] = { cls == MC_DEAD, cls == MC_FREE, cls == MC_ALIVE || cls == MC_DEAD, cls == MC_ALIVE };
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        int total;
        (void)gs_block_rank<MC_WAVES>(preds[a], s_wave, &total);
        if (threadIdx.x == 0) ws.cnt[a * nb + blockIdx.x] = total;
    }
    if (threadIdx.x == 0) ws.wpre[blockIdx.x] = wsum;
}

// One block.  Sums 0 (weights), 1 (dead), 2 (free) become exclusive prefixes in place; 3 (valid) and 4 (alive) are totals only.
__global__ __launch_bounds__(MC_SCAN_THREADS) void k_mcmc_scan(McScratch ws, int nb, gs_mcmc_config cfg, int32_t* __restrict__ counts)
{
    __shared__ unsigned long long s[MC_SCAN_THREADS];
    __shared__ unsigned long long s_tot[5];
    const int t = threadIdx.x;
    const int per = (nb + MC_SCAN_THREADS - 1) / MC_SCAN_THREADS;
    const int lo = min(nb, t * per), hi = min(nb, lo + per);
    for (int a = 0; a < 5; ++a) {
        int32_t* c32 = a == 0 ? nullptr : ws.cnt + (size_t)(a - 1) * nb;
        unsigned long long local = 0;
        for (int i = lo; i < hi; ++i) local += a == 0 ? ws.wpre[i] : (unsigned long long)c32[i];
        s[t] = local;
        __syncthreads();
        for (int d = 1; d < MC_SCAN_THREADS; d <<= 1) {            // inclusive Hillis-Steele scan of the per-thread sums
            const unsigned long long v = t >= d ? s[t - d] : 0ull;
            __syncthreads();
            s[t] += v;
            __syncthreads();
        }
        if (a < 3) {                                               // exclusive prefix written back in place
            unsigned long long run = s[t] - local;
            for (int i = lo; i < hi; ++i) {
                if (a == 0) { const unsigned long long c = ws.wpre[i]; ws.wpre[i] = run; run += c; }
                else { const int32_t c = c32[i]; c32[i] = (int32_t)run; run += (unsigned long long)c; }
            }
        }
        if (t == 0) s_tot[a] = s[MC_SCAN_THREADS - 1];
        __syncthreads();
    }
    if (t != 0) return;
    const long long dead = (long long)s_tot[1], n_free = (long long)s_tot[2], valid = (long long)s_tot[3], alive = (long long)s_tot[4];
    const long long target = min((long long)cfg.cap_max, valid + valid * (long long)cfg.grow_permille / 1000);
    long long n_new = min(n_free, max(0ll, target - valid));
    if (alive == 0) n_new = 0;
    const long long D = alive == 0 ? 0 : dead + n_new;
    ws.hdr->W = s_tot[0]; ws.hdr->dead = dead; ws.hdr->n_new = n_new; ws.hdr->D = D;
    counts[GS_MC_VALID_BEFORE] = (int32_t)valid; counts[GS_MC_DEAD] = (int32_t)dead; counts[GS_MC_ALIVE] = (int32_t)alive;
    counts[GS_MC_FREE] = (int32_t)n_free; counts[GS_MC_NEW] = (int32_t)n_new; counts[GS_MC_DESTINATIONS] = (int32_t)D;
    counts[GS_MC_SOURCES] = 0;                                      // tallied by k_mcmc_apply_src
    counts[GS_MC_VALID_AFTER] = (int32_t)(valid + n_new);
}

__global__ __launch_bounds__(MC_BLOCK) void k_mcmc_destinations(McScratch ws, int64_t N, int32_t* __restrict__ dest_row,
                                                                int32_t* __restrict__ multiplicity)
{
    __shared__ int s_wave[MC_WAVES];
    const long long D = ws.hdr->D, dead = ws.hdr->dead, n_new = ws.hdr->n_new;
    if (D == 0) return;                                             // block-uniform: nothing is written
    const int nb = gridDim.x;
    const int64_t n = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    const int cls = n < N ? ws.cls[n] : MC_OTHER;
    if (n < N) multiplicity[n] = 0;
    int total;
    const int rd = gs_block_rank<MC_WAVES>(cls == MC_DEAD, s_wave, &total);
    if (cls == MC_DEAD) dest_row[ws.cnt[blockIdx.x] + rd] = (int32_t)n;
    const int rf = gs_block_rank<MC_WAVES>(cls == MC_FREE, s_wave, &total);
    const long long jf = (long long)ws.cnt[nb + blockIdx.x] + rf;
    if (cls == MC_FREE && jf < n_new) dest_row[dead + jf] = (int32_t)n;
}

__global__ __launch_bounds__(MC_BLOCK) void k_mcmc_sample(McScratch ws, int64_t N, int nb, uint32_t key0, uint32_t key1, uint32_t call_index,
                                                          int32_t* __restrict__ source_of, int32_t* __restrict__ multiplicity)
{
    const long long D = ws.hdr->D;
    const unsigned long long W = ws.hdr->W;
    for (long long j = (long long)blockIdx.x * MC_BLOCK + threadIdx.x; j < D; j += (long long)gridDim.x * MC_BLOCK) {
        const uint4 u = gs_philox4x32_10(make_uint4((uint32_t)j, call_index, GS_MCMC_STREAM_RELOCATE, 0u), key0, key1);
        const unsigned long long r = (unsigned long long)u.x | ((unsigned long long)u.y << 32);
        const unsigned long long t = __umul64hi(r, W);              // < W
        int lo = 0, hi = nb - 1;                                    // the last block whose prefix is <= t
        while (lo < hi) {
            const int mid = lo + (hi - lo + 1) / 2;
            if (ws.wpre[mid] <= t) lo = mid; else hi = mid - 1;
        }
        const uint32_t local = (uint32_t)(t - ws.wpre[lo]);         // < the block's sum: the row found has w > 0
        const int64_t first = (int64_t)lo * MC_BLOCK;
        int a = 0, b = (int)min((int64_t)MC_BLOCK, N - first) - 1;  // the last row of the block whose prefix is <= local
        while (a < b) {
            const int mid = a + (b - a + 1) / 2;
            if (ws.excl[first + mid] <= local) a = mid; else b = mid - 1;
        }
        const int32_t src = (int32_t)(first + a);
        source_of[j] = src;
        atomicAdd(&multiplicity[src], 1);
    }
}

// gs_mcmc.h, step 5: the logit and the three log-scales of a group whose source was drawn m times
__device__ __forceinline__ void mc_relocated(float logit, const float ls[3], int m, int n_max, float* logit_out, float ls_out[3])
{
    const int M = min(m + 1, n_max);
    const double o = (double)gs_sigmoid(logit);
    double p = 1.0 - pow(1.0 - o, 1.0 / (double)M);
    p = p < 0.005 ? 0.005 : (p > 1.0 - 5.9604644775390625e-8 ? 1.0 - 5.9604644775390625e-8 : p);
    double d = 0.0;
    for (int i = 1; i <= M; ++i) {
        double c = 1.0, pk = p;                                     // C(i-1, 0), p^1
        for (int k = 0; k < i; ++k) {
            const double term = (c * pk) / sqrt((double)(k + 1));
            d = (k & 1) ? d - term : d + term;
            c = (c * (double)(i - 1 - k)) / (double)(k + 1);        // C(i-1, k+1): exact, every product is below 2^53
            pk = pk * p;
        }
    }
    *logit_out = (float)log(p / (1.0 - p));
    const double shift = log(o / d);
#pragma unroll
    for (int j = 0; j < 3; ++j) ls_out[j] = (float)((double)ls[j] + shift);
}

struct McMoments { float4* feat[2]; float* pos[2]; };

__device__ __forceinline__ void mc_zero_moments(const McMoments& mo, int64_t n)
{
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        if (mo.feat[a])
            for (int k = 0; k < MC_F4_PER_ROW; ++k) mo.feat[a][(size_t)n * MC_F4_PER_ROW + k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (mo.pos[a]) { mo.pos[a][3 * n] = 0.0f; mo.pos[a][3 * n + 1] = 0.0f; mo.pos[a][3 * n + 2] = 0.0f; }
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_mcmc_apply_dest(McScratch ws, float* __restrict__ pc, float4* __restrict__ feat4,
                                                              int8_t* __restrict__ mask, int32_t* __restrict__ obj, McMoments mo, int n_max,
                                                              const int32_t* __restrict__ source_of, const int32_t* __restrict__ dest_row,
                                                              const int32_t* __restrict__ multiplicity)
{
    const long long D = ws.hdr->D;
    for (long long j = (long long)blockIdx.x * MC_BLOCK + threadIdx.x; j < D; j += (long long)gridDim.x * MC_BLOCK) {
        const int64_t src = source_of[j], dst = dest_row[j];
        const float4* rs = feat4 + (size_t)src * MC_F4_PER_ROW;     // an alive row: no thread of this launch writes it
        float4* rd = feat4 + (size_t)dst * MC_F4_PER_ROW;
        const float4 b = rs[1];
        const float ls[3] = { b.x, b.y, b.z };
        float logit, ls_new[3];
        mc_relocated(b.w, ls, multiplicity[src], n_max, &logit, ls_new);
        rd[0] = rs[0];
        rd[1] = make_float4(ls_new[0], ls_new[1], ls_new[2], logit);
        for (int k = 2; k < MC_F4_PER_ROW; ++k) rd[k] = rs[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) pc[3 * dst + k] = pc[3 * src + k];
        obj[dst] = obj[src];
        mask[dst] = 0;
        mc_zero_moments(mo, dst);
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_mcmc_apply_src(McScratch ws, int64_t N, float4* __restrict__ feat4, McMoments mo, int n_max,
                                                             const int32_t* __restrict__ multiplicity, int32_t* __restrict__ counts)
{
    if (ws.hdr->D == 0) return;                                     // block-uniform (multiplicity was not written)
    const int64_t n = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    const int m = n < N ? multiplicity[n] : 0;
    if (m > 0) {
        float4* row = feat4 + (size_t)n * MC_F4_PER_ROW;
        const float4 b = row[1];
        const float ls[3] = { b.x, b.y, b.z };
        float logit, ls_new[3];
        mc_relocated(b.w, ls, m, n_max, &logit, ls_new);
        row[1] = make_float4(ls_new[0], ls_new[1], ls_new[2], logit);
        mc_zero_moments(mo, n);
    }
    const unsigned long long sources = gs_ballot(m > 0);
    if ((threadIdx.x & 63) == 0 && sources) atomicAdd(&counts[GS_MC_SOURCES], (int)__popcll(sources));
}

// ---- launchers ------------------------------------------------------------------------------------------------------
void gs_launch_mcmc_noise(float* pc, const float* feat, const int8_t* mask, int64_t N, float noise_scale, float gate_k, float gate_x0,
                          uint64_t seed, uint32_t step_index, hipStream_t s)
{
    if (N <= 0) return;
    k_mcmc_noise<<<(unsigned)MC_NBLK(N), MC_BLOCK, 0, s>>>(pc, reinterpret_cast<const float4*>(feat), mask, N, noise_scale, gate_k, gate_x0,
                                                           (uint32_t)seed, (uint32_t)(seed >> 32), step_index);
}

void gs_launch_mcmc_regulariser(const float* feat, const int8_t* mask, int64_t N, float lambda_opacity, float lambda_scale,
                                const float* upstream, float* grad, float* value_and_count, void* ws, hipStream_t s)
{
    const int nb = (int)MC_NBLK(N);
    char* c = static_cast<char*>(ws);
    McRegTotals* totals = reinterpret_cast<McRegTotals*>(c);
    double* po = reinterpret_cast<double*>(c + 64);
    double* ps = po + nb;
    long long* pv = reinterpret_cast<long long*>(ps + nb);
    if (N > 0) k_mcmc_reg_partial<<<nb, MC_BLOCK, 0, s>>>(feat, mask, N, po, ps, pv);
    k_mcmc_reg_total<<<1, MC_SCAN_THREADS, 0, s>>>(po, ps, pv, nb, lambda_opacity, lambda_scale, totals, value_and_count);
    if (N > 0 && grad) k_mcmc_reg_grad<<<nb, MC_BLOCK, 0, s>>>(feat, mask, N, lambda_opacity, lambda_scale, upstream, totals, grad);
}

void gs_launch_mcmc_relocate(const gs_density_scene& scene, float* const moments[4], const gs_mcmc_config& cfg, const gs_mcmc_plan& plan,
                             uint64_t seed, uint32_t call_index, hipStream_t s)
{
    const int64_t N = scene.n_points;
    if (N <= 0) {                                                   // no row, no scratch: the counts are all zero
        (void)hipMemsetAsync(plan.counts, 0, GS_MC_COUNT_ * sizeof(int32_t), s);
        return;
    }
    const int nb = (int)MC_NBLK(N);
    const McScratch ws = mc_scratch(plan.scratch, N);
    k_mcmc_classify<<<nb, MC_BLOCK, 0, s>>>(scene.point_cloud_features, scene.point_invalid_mask, N, cfg.min_opacity_logit, ws);
    k_mcmc_scan<<<1, MC_SCAN_THREADS, 0, s>>>(ws, nb, cfg, plan.counts);
    const McMoments mo{ { reinterpret_cast<float4*>(moments[0]), reinterpret_cast<float4*>(moments[1]) }, { moments[2], moments[3] } };
    float4* feat4 = reinterpret_cast<float4*>(scene.point_cloud_features);
    k_mcmc_destinations<<<nb, MC_BLOCK, 0, s>>>(ws, N, plan.dest_row, plan.multiplicity);
    // D <= N destinations; the grid walks them, the count is read on the device
    const int grid = std::min(nb, 1024);
    k_mcmc_sample<<<grid, MC_BLOCK, 0, s>>>(ws, N, nb, (uint32_t)seed, (uint32_t)(seed >> 32), call_index, plan.source_of, plan.multiplicity);
    k_mcmc_apply_dest<<<grid, MC_BLOCK, 0, s>>>(ws, scene.point_cloud, feat4, scene.point_invalid_mask, scene.point_object_id, mo, cfg.n_max,
                                                plan.source_of, plan.dest_row, plan.multiplicity);
    k_mcmc_apply_src<<<nb, MC_BLOCK, 0, s>>>(ws, N, feat4, mo, cfg.n_max, plan.multiplicity, plan.counts);
}
