// k_knn.hip -- include/gs_knn.h: exact k nearest neighbours over the point cloud (DESIGN.md "Scene initialisation").
//
//   k_knn_box      bounding box of the participating rows (integer min / max atomics on order-preserving float bits: the result
//                  does not depend on the order of the updates)
//   k_knn_codes    63-bit Morton code per row, 21 bits per axis inside that box; a row that does not take part gets bit 63 and
//                  sorts behind every participating row
//   k_knn_sort_*   stable LSD radix sort of (code, row), eight 8-bit passes, in this file: the rasteriser's sort is not touched
//   k_knn_gather   the rows in sorted order as (x, y, z, row) records, padded to whole leaves
//   k_knn_leaves   one f32 AABB per leaf = run of GS_KNN_LEAF consecutive sorted points (one wave's worth)
//   k_knn_level    AABBs of a complete implicit binary tree over the leaves, heap order, one launch per level, bottom-up
//   k_knn_query    one wave per leaf, one lane per point: the k best of every lane in registers
//
// Exactness does not depend on the order: the sort and the tree only decide which pairs are looked at.  A pair is skipped only
// below a box whose f32 lower bound is strictly greater than the lane's k-th best f32 distance, and every operation of the
// bound (subtract, max, square, add) is monotonic under round-to-nearest, so the bound never exceeds the f32 distance of a
// point inside the box.  Candidates are compared as (d2, row) pairs, so the order of arrival does not matter either.
#include "gs_common.h"

#include <cfloat>
#include <climits>

#define GS_KNN_LEAF 64
#define GS_KNN_SORT_TILE 1024           // keys per block of the sort: 256 threads, four rounds of 256
#define GS_KNN_INVALID 0x80000000u      // flag on the row of a record that does not take part
#define GS_KNN_PAD 0xffffffffu          // row of a record behind the last point (pads the last leaf)

// ---- sizes ----------------------------------------------------------------------------------------------------------
int64_t gs_knn_leaves(int64_t n) { return (n + GS_KNN_LEAF - 1) / GS_KNN_LEAF; }
// leaves of the complete tree: the next power of two
int64_t gs_knn_tree_leaves(int64_t n)
{
    int64_t p = 1;
    while (p < gs_knn_leaves(n)) p <<= 1;
    return p;
}
int64_t gs_knn_sort_blocks(int64_t n) { return (n + GS_KNN_SORT_TILE - 1) / GS_KNN_SORT_TILE; }
size_t gs_knn_sort_bytes(int64_t n) { return (size_t)n * 2 * (sizeof(uint64_t) + sizeof(uint32_t)); }
size_t gs_knn_hist_bytes(int64_t n) { return (size_t)gs_knn_sort_blocks(n) * 256 * sizeof(uint32_t) + 32; }
size_t gs_knn_points_bytes(int64_t n) { return (size_t)gs_knn_leaves(n) * GS_KNN_LEAF * sizeof(float4); }
size_t gs_knn_tree_bytes(int64_t n) { return (size_t)(2 * gs_knn_tree_leaves(n) - 1) * 2 * sizeof(float4); }

// ---- bounding box -----------------------------------------------------------------------------------------------------
// order-preserving map of a finite float onto uint32
__device__ __forceinline__ uint32_t gs_knn_ordered(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float gs_knn_unordered(uint32_t o)
{
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__device__ __forceinline__ bool gs_knn_takes_part(const float* __restrict__ xyz, const int8_t* __restrict__ invalid, int64_t i,
                                                  float& x, float& y, float& z)
{
    x = xyz[3 * i]; y = xyz[3 * i + 1]; z = xyz[3 * i + 2];
    const bool finite = fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX;          // (false for NaN)
    return finite && (!invalid || invalid[i] == 0);
}

// box[0..2] = min, box[3..5] = max as ordered bits; the launcher presets them to 0xffffffff / 0
__global__ __launch_bounds__(256) void k_knn_box(const float* __restrict__ xyz, const int8_t* __restrict__ invalid, int64_t n,
                                                 uint32_t* __restrict__ box)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t lo[3] = { 0xffffffffu, 0xffffffffu, 0xffffffffu }, hi[3] = { 0u, 0u, 0u };
    float p[3];
    if (i < n && gs_knn_takes_part(xyz, invalid, i, p[0], p[1], p[2]))
        for (int a = 0; a < 3; ++a) lo[a] = hi[a] = gs_knn_ordered(p[a]);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], o, 64));
            hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], o, 64));
        }
    }
    if ((threadIdx.x & 63) == 0 && lo[0] != 0xffffffffu)
        for (int a = 0; a < 3; ++a) { atomicMin(&box[a], lo[a]); atomicMax(&box[3 + a], hi[a]); }
}

// ---- Morton codes -----------------------------------------------------------------------------------------------------
// the low 21 bits of v, two zero bits between neighbours
__device__ __forceinline__ uint64_t gs_knn_spread(uint64_t v)
{
    v &= 0x1fffffull;
    v = (v | (v << 32)) & 0x1f00000000ffffull;
    v = (v | (v << 16)) & 0x1f0000ff0000ffull;
    v = (v | (v << 8)) & 0x100f00f00f00f00full;
    v = (v | (v << 4)) & 0x10c30c30c30c30c3ull;
    v = (v | (v << 2)) & 0x1249249249249249ull;
    return v;
}

__global__ __launch_bounds__(256) void k_knn_codes(const float* __restrict__ xyz, const int8_t* __restrict__ invalid, int64_t n,
                                                   const uint32_t* __restrict__ box, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float p[3];
    uint64_t code = 1ull << 63;
    if (gs_knn_takes_part(xyz, invalid, i, p[0], p[1], p[2])) {
        code = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            // the cell only orders the points: double keeps 21 bits honest over an extent of many orders of magnitude
            const double lo = (double)gs_knn_unordered(box[a]), hi = (double)gs_knn_unordered(box[3 + a]);
            const double ext = hi - lo;
            double q = ext > 0.0 ? ((double)p[a] - lo) / ext * 2097152.0 : 0.0;
            q = q < 0.0 ? 0.0 : (q > 2097151.0 ? 2097151.0 : q);
            code |= gs_knn_spread((uint64_t)q) << a;
        }
    }
    keys[i] = code;
    vals[i] = (uint32_t)i;
}

// ---- radix sort: (code, row), stable, 8 bits per pass ---------------------------------------------------------------------
// A block owns GS_KNN_SORT_TILE consecutive keys.  k_knn_sort_hist leaves counts[digit * nb + block]; k_knn_sort_scan turns the
// table into exclusive offsets in that (digit-major) order, one block, the carry in a register; k_knn_sort_scatter ranks every
// key among the keys of its digit before it in the block -- by wave ballots, no atomic decides a position -- and writes it.
__global__ __launch_bounds__(256) void k_knn_sort_hist(const uint64_t* __restrict__ keys, int64_t n, int shift, uint32_t nb,
                                                       uint32_t* __restrict__ counts)
{
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * GS_KNN_SORT_TILE;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t i = first + r * 256 + threadIdx.x;
        if (i < n) atomicAdd(&h[(uint32_t)(keys[i] >> shift) & 255u], 1u);          // (a count: the order of the adds is nothing)
    }
    __syncthreads();
    counts[(size_t)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(1024) void k_knn_sort_scan(uint32_t* __restrict__ counts, int64_t total)
{
    __shared__ uint32_t ws[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (int64_t base = 0; base < total; base += 1024) {
        const int64_t i = base + threadIdx.x;
        const uint32_t v = i < total ? counts[i] : 0u;
        const uint32_t incl = gs_wave_scan_incl(v, lane);
        gs_block_scan_put(ws, wave, lane, incl);
        __syncthreads();
        if (i < total) counts[i] = carry + gs_block_scan_excl(ws, wave, incl, v);
        carry += gs_block_sum<16>(ws);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_knn_sort_scatter(const uint64_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in, int64_t n,
                                                          int shift, uint32_t nb, const uint32_t* __restrict__ offsets,
                                                          uint64_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out)
{
    __shared__ uint32_t cnt[16][256];           // [round * 4 + wave][digit]: keys of the digit in that run of 64, then their first position
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = 0; c < 16; ++c) cnt[c][threadIdx.x] = 0;
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * GS_KNN_SORT_TILE;
    uint64_t key[4];
    uint32_t val[4], rank[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t i = first + r * 256 + threadIdx.x;
        const bool live = i < n;
        key[r] = live ? keys_in[i] : 0ull;
        val[r] = live ? vals_in[i] : 0u;
        const uint32_t digit = (uint32_t)(key[r] >> shift) & 255u;
        uint64_t same = __ballot(live);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (digit >> b) & 1u;
            const uint64_t bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        rank[r] = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (live && rank[r] == 0) cnt[r * 4 + wave][digit] = (uint32_t)__popcll(same);
    }
    __syncthreads();
    {
        uint32_t run = offsets[(size_t)threadIdx.x * nb + blockIdx.x];
        for (int c = 0; c < 16; ++c) { const uint32_t t = cnt[c][threadIdx.x]; cnt[c][threadIdx.x] = run; run += t; }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t i = first + r * 256 + threadIdx.x;
        if (i < n) {
            const uint32_t at = cnt[r * 4 + wave][(uint32_t)(key[r] >> shift) & 255u] + rank[r];
            if ((int64_t)at < n) { keys_out[at] = key[r]; vals_out[at] = val[r]; }
        }
    }
}

// ---- sorted records, leaves, tree -------------------------------------------------------------------------------------
// pts[i] = (x, y, z, row bits) of the i-th sorted row; n_pad = whole leaves
__global__ __launch_bounds__(256) void k_knn_gather(const float* __restrict__ xyz, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                    int64_t n, int64_t n_pad, float4* __restrict__ pts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pad) return;
    float4 p = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(GS_KNN_PAD));
    const uint32_t row = i < n ? vals[i] : GS_KNN_PAD;
    if ((int64_t)row < n) {                                 // (always, for a sorted permutation: no row from here on is out of range)
        if (keys[i] >> 63) p.w = __uint_as_float(row | GS_KNN_INVALID);
        else p = make_float4(xyz[3 * (int64_t)row], xyz[3 * (int64_t)row + 1], xyz[3 * (int64_t)row + 2], __uint_as_float(row));
    }
    pts[i] = p;
}

// node i of the heap: lo = nodes[2 i], hi = nodes[2 i + 1]; an empty box has lo = +inf, hi = -inf
__global__ __launch_bounds__(256) void k_knn_leaves(const float4* __restrict__ pts, int64_t n_leaves, int64_t tree_leaves, float4* __restrict__ nodes)
{
    const int64_t leaf = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (leaf >= tree_leaves) return;
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    if (leaf < n_leaves) {
        const float4 p = pts[leaf * GS_KNN_LEAF + (threadIdx.x & 63)];
        if (!(__float_as_uint(p.w) & GS_KNN_INVALID)) { lo[0] = hi[0] = p.x; lo[1] = hi[1] = p.y; lo[2] = hi[2] = p.z; }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64)); }
    }
    if ((threadIdx.x & 63) == 0) {
        const int64_t node = tree_leaves - 1 + leaf;
        nodes[2 * node] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        nodes[2 * node + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
}

// the `count` nodes first .. first + count of one level from their children
__global__ __launch_bounds__(256) void k_knn_level(float4* __restrict__ nodes, int64_t first, int64_t count)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= count) return;
    const int64_t node = first + j, l = 2 * node + 1, r = l + 1;
    const float4 a = nodes[2 * l], b = nodes[2 * r], c = nodes[2 * l + 1], d = nodes[2 * r + 1];
    nodes[2 * node] = make_float4(fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z), 0.0f);
    nodes[2 * node + 1] = make_float4(fmaxf(c.x, d.x), fmaxf(c.y, d.y), fmaxf(c.z, d.z), 0.0f);
}

// ---- query ------------------------------------------------------------------------------------------------------------
// The k best (d2, row) pairs of a lane, ascending, in registers: every index below is a constant after unrolling.
template <int K> struct GsKnnBest {
    float d[K];
    uint32_t r[K];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int j = 0; j < K; ++j) { d[j] = INFINITY; r[j] = 0x7fffffffu; }
    }
    static __device__ __forceinline__ bool before(float d0, uint32_t r0, float d1, uint32_t r1) { return d0 < d1 || (d0 == d1 && r0 < r1); }
    __device__ __forceinline__ void insert(float dd, uint32_t rr)
    {
        if (!before(dd, rr, d[K - 1], r[K - 1])) return;
#pragma unroll
        for (int j = K - 1; j >= 0; --j) {
            const bool here = before(dd, rr, d[j], r[j]);
            if (j < K - 1 && here) { d[j + 1] = d[j]; r[j + 1] = r[j]; }
            bool above = false;                                                      // ... and not before slot j - 1: slot j is its place
            if (j > 0) above = before(dd, rr, d[j - 1], r[j - 1]);
            if (here && !above) { d[j] = dd; r[j] = rr; }
        }
    }
};

// the f32 squared distance of include/gs_knn.h: (dx dx + dy dy) + dz dz, every operation rounded once (-ffp-contract=off)
__device__ __forceinline__ float gs_knn_d2(float x, float y, float z, float px, float py, float pz)
{
    const float dx = x - px, dy = y - py, dz = z - pz;
    return (dx * dx + dy * dy) + dz * dz;
}

// One wave per leaf, four leaves per block.  The wave walks the tree as ONE walker (the node is uniform, in scalar registers):
// a node is entered when ANY lane's bound test passes, a leaf entered is staged in LDS once (a coalesced 1 KB load) and read
// by all lanes at the same address (a broadcast, no bank conflict).  Looking at more pairs than a lane alone would is harmless:
// a pair only enters a lane's list by the (d2, row) comparison.  Stackless: from a node the walk goes down to the left child,
// or to the right sibling, or up while the node is a right child (heap order: children of i are 2i+1 and 2i+2).
template <int K>
__global__ __launch_bounds__(256) void k_knn_query(const float4* __restrict__ pts, const float4* __restrict__ nodes, int64_t n_leaves,
                                                   int64_t tree_leaves, int k_out, float* __restrict__ d2_out, int32_t* __restrict__ idx_out)
{
    __shared__ float4 sLeaf[4][GS_KNN_LEAF];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t leaf = (int64_t)blockIdx.x * 4 + wave;
    if (leaf >= n_leaves) return;                      // (whole waves leave; the block has no barrier)
    float4* stage = sLeaf[wave];
    const float4 me = pts[leaf * GS_KNN_LEAF + lane];
    const uint32_t my_row = __float_as_uint(me.w);
    const bool asks = !(my_row & GS_KNN_INVALID);
    GsKnnBest<K> best;
    best.clear();
    // the lane's own leaf first: its points are the wave's own records
    stage[lane] = me;
    __builtin_amdgcn_wave_barrier();
    for (int j = 0; j < GS_KNN_LEAF; ++j) {
        const float4 p = stage[j];
        const uint32_t row = __float_as_uint(p.w);
        if (asks && !(row & GS_KNN_INVALID) && row != my_row) best.insert(gs_knn_d2(me.x, me.y, me.z, p.x, p.y, p.z), row);
    }
    const int64_t own = tree_leaves - 1 + leaf;
    int64_t node = 0;
    while (true) {
        bool enter = false;
        if (node != own) {
            const float4 lo = nodes[2 * node], hi = nodes[2 * node + 1];
            if (lo.x <= hi.x) {                        // (not an empty box)
                const float bx = fmaxf(fmaxf(lo.x - me.x, 0.0f), me.x - hi.x), by = fmaxf(fmaxf(lo.y - me.y, 0.0f), me.y - hi.y);
                const float bz = fmaxf(fmaxf(lo.z - me.z, 0.0f), me.z - hi.z);
                const float bound = (bx * bx + by * by) + bz * bz;
                // skipped only when strictly greater than the k-th best: an equal distance may still win on the row
                enter = __ballot(asks && !(bound > best.d[K - 1])) != 0ull;
            }
        }
        if (enter && node < tree_leaves - 1) { node = 2 * node + 1; continue; }
        if (enter) {
            __builtin_amdgcn_wave_barrier();
            stage[lane] = pts[(node - (tree_leaves - 1)) * GS_KNN_LEAF + lane];
            __builtin_amdgcn_wave_barrier();
            for (int j = 0; j < GS_KNN_LEAF; ++j) {
                const float4 p = stage[j];
                const uint32_t row = __float_as_uint(p.w);
                if (asks && !(row & GS_KNN_INVALID)) best.insert(gs_knn_d2(me.x, me.y, me.z, p.x, p.y, p.z), row);
            }
        }
        while (node != 0 && (node & 1) == 0) node = (node - 1) >> 1;
        if (node == 0) break;
        node += 1;
    }
    if (my_row == GS_KNN_PAD) return;
    const int64_t out = (int64_t)(my_row & ~GS_KNN_INVALID) * k_out;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j < k_out) {
            d2_out[out + j] = best.d[j];
            if (idx_out) idx_out[out + j] = best.r[j] == 0x7fffffffu ? -1 : (int32_t)best.r[j];
        }
    }
}

// ---- launcher -----------------------------------------------------------------------------------------------------------
// sort_ws: gs_knn_sort_bytes, hist_ws: gs_knn_hist_bytes (the last 32 bytes are the box), pts_ws: gs_knn_points_bytes,
// tree_ws: gs_knn_tree_bytes.  Everything is queued on s; nothing is read back.
void gs_launch_knn(const float* xyz, const int8_t* invalid, int64_t n, int k, float* d2_out, int32_t* idx_out,
                   void* sort_ws, void* hist_ws, void* pts_ws, void* tree_ws, hipStream_t s)
{
    if (n <= 0) return;
    uint64_t* keys[2] = { reinterpret_cast<uint64_t*>(sort_ws), reinterpret_cast<uint64_t*>(sort_ws) + n };
    uint32_t* vals[2] = { reinterpret_cast<uint32_t*>(keys[1] + n), reinterpret_cast<uint32_t*>(keys[1] + n) + n };
    const int64_t nb = gs_knn_sort_blocks(n), n_leaves = gs_knn_leaves(n), tree_leaves = gs_knn_tree_leaves(n);
    uint32_t* counts = reinterpret_cast<uint32_t*>(hist_ws);
    uint32_t* box = counts + nb * 256;
    float4* pts = reinterpret_cast<float4*>(pts_ws);
    float4* nodes = reinterpret_cast<float4*>(tree_ws);
    const unsigned g256 = (unsigned)((n + 255) / 256);

    (void)hipMemsetAsync(box, 0xff, 3 * sizeof(uint32_t), s);
    (void)hipMemsetAsync(box + 3, 0, 3 * sizeof(uint32_t), s);
    k_knn_box<<<g256, 256, 0, s>>>(xyz, invalid, n, box);
    k_knn_codes<<<g256, 256, 0, s>>>(xyz, invalid, n, box, keys[0], vals[0]);
    for (int pass = 0; pass < 8; ++pass) {
        const int a = pass & 1, b = a ^ 1;
        k_knn_sort_hist<<<(unsigned)nb, 256, 0, s>>>(keys[a], n, 8 * pass, (uint32_t)nb, counts);
        k_knn_sort_scan<<<1, 1024, 0, s>>>(counts, nb * 256);
        k_knn_sort_scatter<<<(unsigned)nb, 256, 0, s>>>(keys[a], vals[a], n, 8 * pass, (uint32_t)nb, counts, keys[b], vals[b]);
    }
    // (eight passes: the sorted pairs are back in the first half)
    k_knn_gather<<<(unsigned)((n_leaves * GS_KNN_LEAF + 255) / 256), 256, 0, s>>>(xyz, keys[0], vals[0], n, n_leaves * GS_KNN_LEAF, pts);
    k_knn_leaves<<<(unsigned)((tree_leaves + 3) / 4), 256, 0, s>>>(pts, n_leaves, tree_leaves, nodes);
    for (int64_t width = tree_leaves / 2; width >= 1; width /= 2)
        k_knn_level<<<(unsigned)((width + 255) / 256), 256, 0, s>>>(nodes, width - 1, width);
    const unsigned gq = (unsigned)((n_leaves + 3) / 4);
    if (k <= 1) k_knn_query<1><<<gq, 256, 0, s>>>(pts, nodes, n_leaves, tree_leaves, k, d2_out, idx_out);
    else if (k <= 3) k_knn_query<3><<<gq, 256, 0, s>>>(pts, nodes, n_leaves, tree_leaves, k, d2_out, idx_out);
    else if (k <= 4) k_knn_query<4><<<gq, 256, 0, s>>>(pts, nodes, n_leaves, tree_leaves, k, d2_out, idx_out);
    else k_knn_query<8><<<gq, 256, 0, s>>>(pts, nodes, n_leaves, tree_leaves, k, d2_out, idx_out);
}
