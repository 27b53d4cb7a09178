// k_exchange.hip -- include/gs_exchange.h: the touched rows of the two point gradients gathered into packed rows (k_pack_rows)
// and several packed lists merged into one union list and one summed gradient (k_merge_tag, the ordered compaction of
// k_sparse.hip, k_merge_sum).  Nothing here waits on another workgroup, no atomic is used and every sum has a fixed order: the
// result is the same on every run.
//
// A packed row is 60 words = fifteen 16-byte quads: quads 0..13 the 56 feature gradients, quad 14 the three position gradients
// and the row id.  One lane moves one quad, so consecutive lanes store (pack) or load (merge) consecutive 16 bytes of the packed
// buffer, and the fourteen feature quads of a row are 224 contiguous bytes of the dense gradient as well.
#include "gs_common.h"

#define GS_XROW_WORDS 60        // GS_PACKED_ROW_WORDS
#define GS_XROW_QUADS 15
#define GS_XROW_ID 59

// e -> (e / d, e % d); 32-bit when the whole range fits (uniform: a 64-bit division is a subroutine on this part)
__device__ __forceinline__ void gs_divmod(int64_t e, int64_t total, int64_t d, int64_t* quot, int64_t* rem)
{
    if (total <= 0xffffffffll && d <= 0xffffffffll) {
        const uint32_t q = (uint32_t)e / (uint32_t)d;
        *quot = q; *rem = (int64_t)((uint32_t)e - q * (uint32_t)d);
    } else { *quot = e / d; *rem = e - *quot * d; }
}

__device__ __forceinline__ int64_t gs_clamped_count(const int32_t* __restrict__ count, int64_t bound)
{
    const int64_t n = (int64_t)count[0];
    return n < 0 ? 0 : (n < bound ? n : bound);
}

// ---- pack ---------------------------------------------------------------------------------------------------------------
// The grid covers max_count rows, the host's bound; *count is read on the device and the lanes beyond it leave at once.
// vec_in: grad_features is 16-byte aligned (every 224-byte row is, then).  Values travel as bits.
__global__ __launch_bounds__(256) void k_pack_rows(const float* __restrict__ grad_features, const float* __restrict__ grad_pointcloud, int64_t n_rows,
                                                   const int32_t* __restrict__ ids, const int32_t* __restrict__ count, int64_t max_count,
                                                   uint4* __restrict__ packed, int vec_in)
{
    const int64_t total = gs_clamped_count(count, max_count) * GS_XROW_QUADS;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        int64_t r, c;
        gs_divmod(e, total, GS_XROW_QUADS, &r, &c);
        const int64_t id = (int64_t)ids[r];
        const bool ok = id >= 0 && id < n_rows;
        uint4 q = make_uint4(0u, 0u, 0u, 0u);
        if (c < GS_XROW_QUADS - 1) {
            if (ok) {
                const float* src = grad_features + id * 56 + 4 * c;
                float4 v;
                if (vec_in) v = *reinterpret_cast<const float4*>(src);
                else v = make_float4(src[0], src[1], src[2], src[3]);
                q = make_uint4(__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w));
            }
        } else {
            if (ok) {
                const float* src = grad_pointcloud + id * 3;
                q.x = __float_as_uint(src[0]); q.y = __float_as_uint(src[1]); q.z = __float_as_uint(src[2]);
            }
            q.w = ok ? (uint32_t)id : 0xffffffffu;              // an id outside the tensor: the merge skips the row
        }
        packed[e] = q;                                          // e == r * 15 + c
    }
}

void gs_launch_pack_rows(const float* grad_features, const float* grad_pointcloud, int64_t n_rows, const int32_t* ids, const int32_t* count,
                         int64_t max_count, float* packed_out, hipStream_t s)
{
    if (n_rows <= 0 || max_count <= 0) return;
    int64_t nb = (max_count * GS_XROW_QUADS + 255) / 256;
    if (nb > 0x7fffffff) nb = 0x7fffffff;                       // (the loop strides over the rest)
    k_pack_rows<<<(unsigned)nb, 256, 0, s>>>(grad_features, grad_pointcloud, n_rows, ids, count, max_count, reinterpret_cast<uint4*>(packed_out),
                                             ((uintptr_t)grad_features & 15u) == 0 ? 1 : 0);
}

// ---- merge --------------------------------------------------------------------------------------------------------------
// 1. k_merge_tag, one lane per (list, position) inside the list's count: tag[id] = 1 -- every writer of a byte stores the same
//    value, so the race is benign, needs no atomic and decides no position -- and ids_all[list][position] = id, a compact copy
//    of the id words (4 bytes apart instead of 240) for the searches of step 3.  A skipped row (id word outside [0, n_rows),
//    what k_pack_rows leaves for a bad id) takes the id of the nearest kept row before it (-1 without one): the copy stays
//    non-decreasing, and the FIRST entry that is >= a searched id is then always a kept row.
// 2. the ordered compaction of k_sparse.hip over the n_rows tag bytes with the identity as its ids_in: the union, ascending.
// 3. k_merge_sum, fifteen lanes per union row: a binary search of every list's ids (lower bound), the hit rows' quads added to
//    the lane's accumulator in list order (the first hit seeds it: a row of one list is copied bit for bit), one 16-byte store
//    into the dense feature row; the last lane of a row owns the three position floats.  One search after the other is a chain
//    of n_lists * log2(count) dependent loads per lane; the searches of 2, 4 or 8 lists (the smallest chunk that covers
//    n_lists, 8 beyond) advance together instead, so that a round's loads are in flight at once.
//    A slot whose search has ended, or that lies past the last list, still loads entry 0 and row 0 of its list -- inside the
//    buffers, possibly behind the count -- and the value is discarded.
// Cost of skipped rows: the backward walk of step 1 is one strided load per skipped row in a run, so a list that is mostly
// skipped rows costs count^2 / 2 loads.  Lists from k_pack_rows hold such rows only for ids that were already bad.
__global__ __launch_bounds__(256) void k_merge_tag(const uint32_t* __restrict__ packed, const int32_t* __restrict__ counts, int n_lists,
                                                   int64_t list_stride, int64_t n_rows, uint8_t* __restrict__ tag, int32_t* __restrict__ ids_all)
{
    const int64_t total = (int64_t)n_lists * list_stride;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        int64_t l, p;
        gs_divmod(e, total, list_stride, &l, &p);
        if (p >= gs_clamped_count(counts + l, list_stride)) continue;      // behind the count: never read, here or in k_merge_sum
        const uint32_t* id_words = packed + l * list_stride * GS_XROW_WORDS + GS_XROW_ID;
        int32_t id = (int32_t)id_words[p * GS_XROW_WORDS];
        if (id >= 0 && (int64_t)id < n_rows) tag[id] = 1;
        else {
            id = -1;
            for (int64_t b = p - 1; b >= 0; --b) {
                const int32_t x = (int32_t)id_words[b * GS_XROW_WORDS];
                if (x >= 0 && (int64_t)x < n_rows) { id = x; break; }
            }
        }
        ids_all[e] = id;
    }
}

template <int GS_MERGE_CHUNK>      // lists whose searches run side by side: 2, 4 or 8, the smallest that covers n_lists (8 beyond)
__global__ __launch_bounds__(256) void k_merge_sum(const float* __restrict__ packed, const int32_t* __restrict__ counts, int n_lists, int64_t list_stride,
                                                   const int32_t* __restrict__ ids_all, const int32_t* __restrict__ union_ids,
                                                   const int32_t* __restrict__ union_count, int64_t max_union, int64_t n_rows,
                                                   float* __restrict__ grad_features, float* __restrict__ grad_pointcloud, int vec_out)
{
    const int64_t total = gs_clamped_count(union_count, max_union) * GS_XROW_QUADS;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        int64_t u, c;
        gs_divmod(e, total, GS_XROW_QUADS, &u, &c);
        const int32_t id = union_ids[u];
        if (id < 0 || (int64_t)id >= n_rows) continue;          // (the compaction lists rows of the tag array only)
        bool have = false;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        // GS_MERGE_CHUNK lists at a time, their searches in lockstep: every round loads one entry of each list at once (an
        // index inside the list whether or not that search still runs, so the loads need no branch and are all in flight
        // together), and the hit rows' quads are loaded the same way before they are added, in list order
        for (int l0 = 0; l0 < n_lists; l0 += GS_MERGE_CHUNK) {
            uint32_t lo[GS_MERGE_CHUNK], hi[GS_MERGE_CHUNK], cnt[GS_MERGE_CHUNK];
            int64_t base[GS_MERGE_CHUNK];
#pragma unroll
            for (int j = 0; j < GS_MERGE_CHUNK; ++j) {
                const int l = l0 + j < n_lists ? l0 + j : l0;                                  // (past the last list: a copy of list l0 that counts for nothing)
                cnt[j] = l0 + j < n_lists ? (uint32_t)gs_clamped_count(counts + l, list_stride < 0x7fffffffll ? list_stride : 0x7fffffffll) : 0u;
                base[j] = (int64_t)l * list_stride;
                lo[j] = 0u; hi[j] = cnt[j];                                                   // the first entry >= id
            }
            for (;;) {
                bool more = false;
                int32_t at[GS_MERGE_CHUNK];
#pragma unroll
                for (int j = 0; j < GS_MERGE_CHUNK; ++j) at[j] = ids_all[base[j] + (lo[j] < hi[j] ? (lo[j] + hi[j]) >> 1 : 0u)];
#pragma unroll
                for (int j = 0; j < GS_MERGE_CHUNK; ++j)
                    if (lo[j] < hi[j]) {
                        const uint32_t mid = (lo[j] + hi[j]) >> 1;
                        if (at[j] < id) lo[j] = mid + 1; else hi[j] = mid;
                        more |= lo[j] < hi[j];
                    }
                if (!more) break;
            }
            int32_t found[GS_MERGE_CHUNK];
            float4 v[GS_MERGE_CHUNK];
#pragma unroll
            for (int j = 0; j < GS_MERGE_CHUNK; ++j) found[j] = ids_all[base[j] + (lo[j] < cnt[j] ? lo[j] : 0u)];
#pragma unroll
            for (int j = 0; j < GS_MERGE_CHUNK; ++j) {
                const bool hit = lo[j] < cnt[j] && found[j] == id;
                v[j] = *reinterpret_cast<const float4*>(packed + (base[j] + (hit ? lo[j] : 0u)) * GS_XROW_WORDS + 4 * c);
                if (!hit) continue;
                if (!have) { acc = v[j]; have = true; }
                else { acc.x += v[j].x; acc.y += v[j].y; acc.z += v[j].z; acc.w += v[j].w; }   // (.w of the last quad is the id word: never stored)
            }
        }
        if (!have) continue;                                    // (only a list that does not ascend can tag a row no search finds)
        if (c < GS_XROW_QUADS - 1) {
            float* dst = grad_features + (int64_t)id * 56 + 4 * c;
            if (vec_out) *reinterpret_cast<float4*>(dst) = acc;
            else { dst[0] = acc.x; dst[1] = acc.y; dst[2] = acc.z; dst[3] = acc.w; }
        } else {
            float* dst = grad_pointcloud + (int64_t)id * 3;
            dst[0] = acc.x; dst[1] = acc.y; dst[2] = acc.z;
        }
    }
}

size_t gs_merge_tag_bytes(int64_t n_rows) { return (size_t)((n_rows + 3) & ~(int64_t)3) + 16; }

void gs_launch_merge_rows(const float* packed, const int32_t* counts, int n_lists, int64_t list_stride, int64_t n_rows, float* grad_features_out,
                          float* grad_pointcloud_out, int32_t* union_ids_out, int64_t union_capacity, int32_t* union_count_out, uint8_t* tag,
                          int32_t* ids_all, uint32_t* block_totals, hipStream_t s)
{
    const int64_t entries = (int64_t)n_lists * list_stride;
    (void)hipMemsetAsync(tag, 0, gs_merge_tag_bytes(n_rows), s);
    int64_t nb = (entries + 255) / 256;
    if (nb > 0x7fffffff) nb = 0x7fffffff;
    k_merge_tag<<<(unsigned)nb, 256, 0, s>>>(reinterpret_cast<const uint32_t*>(packed), counts, n_lists, list_stride, n_rows, tag, ids_all);
    gs_launch_touched_rows(tag, 1, nullptr, (int)n_rows, block_totals, union_ids_out, union_capacity, union_count_out, s);
    const int64_t max_union = n_rows < entries ? n_rows : entries;
    nb = (max_union * GS_XROW_QUADS + 255) / 256;
    if (nb > 0x7fffffff) nb = 0x7fffffff;
    const int vec_out = ((uintptr_t)grad_features_out & 15u) == 0 ? 1 : 0;
#define GS_MERGE_SUM(CHUNK)                                                                                                              \
    k_merge_sum<CHUNK><<<(unsigned)nb, 256, 0, s>>>(packed, counts, n_lists, list_stride, ids_all, union_ids_out, union_count_out, max_union, \
                                                    n_rows, grad_features_out, grad_pointcloud_out, vec_out)
    if (n_lists <= 2) GS_MERGE_SUM(2);
    else if (n_lists <= 4) GS_MERGE_SUM(4);
    else GS_MERGE_SUM(8);
#undef GS_MERGE_SUM
}
