// k_fusion.hip -- depth frames fused into a truncated signed distance volume, and an indexed triangle mesh out of any device
// volume by marching tetrahedra (include/gs_fusion.h, where the per-voxel rule and the mesh's orders are stated).
//
// Both halves give a thread one voxel, by linear index: z is the fastest axis, so the lanes of a wave run along z, volume
// traffic is coalesced and neighbouring lanes gather neighbouring pixels.
//  k_tsdf_integrate    the volume struct and up to GS_TSDF_VIEWS_PER_LAUNCH view structs are the kernel's argument: the view loop
//                      is wave-uniform and reads the views with scalar loads; a voxel is read once, walked through the views in
//                      registers and written once (only if a view changed it); a view that a voxel does not see costs it no gather.
//                      No atomics, no reductions.  (Issuing the gathers of four views together, branch-free, before their updates
//                      measured slower: 30.3 against 16.5 ms for 16 views of 1920 x 1088 into 512^3 with colour.)
//  k_iso_plan          27 corners around the voxel as two bit masks (valid, inside) -> which of the 8 cells around it are
//                      processed, the 7-bit mask of the crossings it owns, its own cell's triangle count; one 16-bit word per
//                      voxel, and the block's two sums.
//  k_iso_scan_blocks   one block walks the block sums 256 at a time (gs_common.h's block scan, a 64-bit carry between rounds):
//                      exclusive offsets in place, the totals to the caller's word pair.
//  k_iso_vertices      block scan of the crossing counts -> every voxel's first vertex (kept for the faces), the vertices.
//  k_iso_faces         block scan of the triangle counts -> the cell's first triangle; a corner of a triangle is found as its
//                      owner's first vertex + the owner's crossings of lower edge type.
// Every store is guarded by the sizes the caller gave; every gather index is checked as a float before it becomes an integer.
#include "gs_common.h"
#include "../../include/gs_fusion.h"

#define FU_THREADS GS_ISO_BLOCK
#define FU_WAVES (FU_THREADS / 64)

struct GsTsdfLaunch {
    gs_tsdf_volume vol;
    int32_t n_views;
    gs_tsdf_view views[GS_TSDF_VIEWS_PER_LAUNCH];
};
static_assert(sizeof(GsTsdfLaunch) <= 4096, "the launch argument must fit the kernel argument segment");

__device__ __forceinline__ bool fu_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

template <bool COLOUR>
__global__ __launch_bounds__(FU_THREADS) void k_tsdf_integrate(const GsTsdfLaunch a)
{
    const int64_t n = (int64_t)a.vol.nx * a.vol.ny * a.vol.nz;
    const int64_t idx = (int64_t)blockIdx.x * FU_THREADS + threadIdx.x;
    if (idx >= n) return;
    const int k = (int)(idx % a.vol.nz);
    const int64_t ij = idx / a.vol.nz;
    const int j = (int)(ij % a.vol.ny), i = (int)(ij / a.vol.ny);
    const float px = a.vol.origin[0] + (float)i * a.vol.voxel[0];
    const float py = a.vol.origin[1] + (float)j * a.vol.voxel[1];
    const float pz = a.vol.origin[2] + (float)k * a.vol.voxel[2];
    const float trunc = a.vol.trunc, max_weight = a.vol.max_weight, min_alpha = a.vol.min_alpha, near = a.vol.near;
    float tsdf = a.vol.tsdf[idx], weight = a.vol.weight[idx];
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    if constexpr (COLOUR) { c0 = a.vol.colour[3 * idx]; c1 = a.vol.colour[3 * idx + 1]; c2 = a.vol.colour[3 * idx + 2]; }
    bool changed = false;
    for (int v = 0; v < a.n_views; ++v) {                   // wave-uniform
        const gs_tsdf_view& V = a.views[v];
        const float x = ((V.m[0][0] * px + V.m[0][1] * py) + V.m[0][2] * pz) + V.m[0][3];
        const float y = ((V.m[1][0] * px + V.m[1][1] * py) + V.m[1][2] * pz) + V.m[1][3];
        const float z = ((V.m[2][0] * px + V.m[2][1] * py) + V.m[2][2] * pz) + V.m[2][3];
        if (!(z > near)) continue;
        const float pu_f = V.fx * (x / z) + V.cx, pv_f = V.fy * (y / z) + V.cy;
        if (!(pu_f >= 0.0f && pu_f < (float)V.w && pv_f >= 0.0f && pv_f < (float)V.h)) continue;     // NaN fails
        const int pu = (int)floorf(pu_f), pv = (int)floorf(pv_f);
        const int64_t pixel = (int64_t)pv * V.w + pu;
        const float d = V.depth[pixel];
        if (!(d > 0.0f) || !fu_finite(d)) continue;
        if (V.alpha && !(V.alpha[pixel] >= min_alpha)) continue;
        const float sdf = d - z;
        if (sdf < -trunc) continue;
        const float s = fminf(1.0f, sdf / trunc);
        const float W = weight, Wn = W + 1.0f;
        tsdf = (W * tsdf + s) / Wn;
        if constexpr (COLOUR) {
            if (V.image) {
                c0 = (W * c0 + V.image[3 * pixel]) / Wn;
                c1 = (W * c1 + V.image[3 * pixel + 1]) / Wn;
                c2 = (W * c2 + V.image[3 * pixel + 2]) / Wn;
            }
        }
        weight = fminf(Wn, max_weight);
        changed = true;
    }
    if (!changed) return;
    a.vol.tsdf[idx] = tsdf;
    a.vol.weight[idx] = weight;
    if constexpr (COLOUR) { a.vol.colour[3 * idx] = c0; a.vol.colour[3 * idx + 1] = c1; a.vol.colour[3 * idx + 2] = c2; }
}

void gs_launch_tsdf_integrate(const gs_tsdf_volume& vol, const gs_tsdf_view* views, int n_views, hipStream_t s)
{
    const int64_t n = (int64_t)vol.nx * vol.ny * vol.nz;
    const dim3 grid((unsigned)((n + FU_THREADS - 1) / FU_THREADS));
    for (int first = 0; first < n_views; first += GS_TSDF_VIEWS_PER_LAUNCH) {
        GsTsdfLaunch a;
        a.vol = vol;
        a.n_views = n_views - first < GS_TSDF_VIEWS_PER_LAUNCH ? n_views - first : GS_TSDF_VIEWS_PER_LAUNCH;
        for (int v = 0; v < GS_TSDF_VIEWS_PER_LAUNCH; ++v) a.views[v] = views[first + (v < a.n_views ? v : 0)];
        if (vol.colour) hipLaunchKernelGGL(k_tsdf_integrate<true>, grid, dim3(FU_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_tsdf_integrate<false>, grid, dim3(FU_THREADS), 0, s, a);
    }
}

// ---- the isosurface ----------------------------------------------------------------------------------------------------
// Corners of a cell as codes 4 dx + 2 dy + dz.  Tetrahedron t of the Kuhn split, permutations in lexicographic order:
// v0 = 0, v1 = the first axis, v2 = the first two, v3 = 7.
__device__ static const uint8_t ISO_TET_CORNER[6][4] = { { 0, 4, 6, 7 }, { 0, 4, 5, 7 }, { 0, 2, 6, 7 }, { 0, 2, 3, 7 }, { 0, 1, 5, 7 }, { 0, 1, 3, 7 } };
#define ISO_NEGATIVE_TETS 0x26u                          // bit t: tetrahedron t (an odd permutation: 1, 2, 5) has determinant -1
__device__ static const uint8_t ISO_EDGE_ENDS[6][2] = { { 0, 1 }, { 0, 2 }, { 0, 3 }, { 1, 2 }, { 1, 3 }, { 2, 3 } };
// edge type of the corner-code difference: +x 0, +y 1, +z 2, +x+y 3, +x+z 4, +y+z 5, +x+y+z 6
__device__ static const uint8_t ISO_TYPE_OF_DELTA[8] = { 0, 2, 1, 5, 0, 4, 3, 6 };
#define ISO_DELTA_OF_TYPE(e) ((e) == 0 ? 4 : (e) == 1 ? 2 : (e) == 2 ? 1 : (e) == 3 ? 6 : (e) == 4 ? 5 : (e) == 5 ? 3 : 7)
// By the set of inside corners (bit v: corner v): the triangles as tetrahedron edges (ISO_EDGE_ENDS), three bits each, triangle 0
// in bits 0..8 and triangle 1 in bits 9..17, wound for a tetrahedron of determinant +1 (gs_fusion.h); the count in bits 18..19.
#define ISO_TRI(a, b, c) ((uint32_t)(a) | (uint32_t)(b) << 3 | (uint32_t)(c) << 6)
#define ISO_ONE(a, b, c) (ISO_TRI(a, b, c) | 1u << 18)
#define ISO_TWO(a, b, c, d, e, f) (ISO_TRI(a, b, c) | ISO_TRI(d, e, f) << 9 | 2u << 18)
__device__ static const uint32_t ISO_CASE[16] = {
    0u, ISO_ONE(0, 1, 2), ISO_ONE(0, 4, 3), ISO_TWO(1, 2, 4, 1, 4, 3), ISO_ONE(1, 3, 5), ISO_TWO(2, 0, 3, 2, 3, 5), ISO_TWO(0, 4, 5, 0, 5, 1),
    ISO_ONE(2, 4, 5), ISO_ONE(2, 5, 4), ISO_TWO(0, 1, 5, 0, 5, 4), ISO_TWO(3, 0, 2, 3, 2, 5), ISO_ONE(1, 5, 3), ISO_TWO(1, 3, 4, 1, 4, 2),
    ISO_ONE(0, 3, 4), ISO_ONE(0, 2, 1), 0u };

// the 8 corners of the cell (a,b,c), a,b,c in {0,1}, of the 3x3x3 neighbourhood whose corner (p,q,r) is bit 9p + 3q + r
#define ISO_CELL_BITS(a, b, c) (0x361Bu << (9 * (a) + 3 * (b) + (c)))
#define ISO_CENTRE_BIT 13

__device__ __forceinline__ void iso_ijk(int64_t idx, int ny, int nz, int& i, int& j, int& k)
{
    k = (int)(idx % nz);
    const int64_t ij = idx / nz;
    j = (int)(ij % ny);
    i = (int)(ij / ny);
}

__global__ __launch_bounds__(FU_THREADS) void k_iso_plan(const gs_iso_volume vol, uint16_t* __restrict__ cell_ws, int64_t* __restrict__ block_ws)
{
    __shared__ int ws_v[FU_WAVES], ws_t[FU_WAVES];
    const int64_t n = (int64_t)vol.nx * vol.ny * vol.nz;
    const int64_t idx = (int64_t)blockIdx.x * FU_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t mask = 0, ntri = 0;
    if (idx < n) {
        int i, j, k;
        iso_ijk(idx, vol.ny, vol.nz, i, j, k);
        uint32_t ok = 0, in = 0;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const int ii = i + p - 1, jj = j + q - 1, kk = k + r - 1;
                    if (ii < 0 || jj < 0 || kk < 0 || ii >= vol.nx || jj >= vol.ny || kk >= vol.nz) continue;
                    const int64_t at = ((int64_t)ii * vol.ny + jj) * vol.nz + kk;
                    const float value = vol.values[at];
                    const uint32_t bit = 1u << (9 * p + 3 * q + r);
                    if (fu_finite(value) && (!vol.valid || vol.valid[at] > 0.0f)) ok |= bit;
                    if (value < vol.level) in |= bit;
                }
        uint32_t cells = 0;                                  // bit 4a + 2b + c: the cell (a,b,c) around the voxel is processed
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int c = 0; c < 2; ++c)
                    if ((ok & ISO_CELL_BITS(a, b, c)) == ISO_CELL_BITS(a, b, c)) cells |= 1u << (4 * a + 2 * b + c);
        const uint32_t centre = in >> ISO_CENTRE_BIT & 1u;
#pragma unroll
        for (int e = 0; e < 7; ++e) {
            const int delta = ISO_DELTA_OF_TYPE(e), dx = delta >> 2 & 1, dy = delta >> 1 & 1, dz = delta & 1;
            const uint32_t other = in >> (ISO_CENTRE_BIT + 9 * dx + 3 * dy + dz) & 1u;
            // the cells (a,b,c) that hold both ends: a = 1 where the edge steps along the axis, a in {0,1} where it does not
            uint32_t holders = 0;
#pragma unroll
            for (int a = dx; a < 2; ++a)
#pragma unroll
                for (int b = dy; b < 2; ++b)
#pragma unroll
                    for (int c = dz; c < 2; ++c) holders |= 1u << (4 * a + 2 * b + c);
            if (centre != other && (cells & holders)) mask |= 1u << e;
        }
        if (cells & 0x80u) {                                 // the voxel's own cell (1,1,1)
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                uint32_t inside = 0;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int code = ISO_TET_CORNER[t][v];
                    inside += in >> (ISO_CENTRE_BIT + 9 * (code >> 2 & 1) + 3 * (code >> 1 & 1) + (code & 1)) & 1u;
                }
                ntri += inside == 2 ? 2u : (inside == 1 || inside == 3 ? 1u : 0u);
            }
        }
        cell_ws[idx] = (uint16_t)(mask | ntri << 8);
    }
    const int sum_v = gs_wave_sum_i(__popc(mask)), sum_t = gs_wave_sum_i((int)ntri);
    gs_block_put(ws_v, wave, lane, sum_v);
    gs_block_put(ws_t, wave, lane, sum_t);
    __syncthreads();
    if (threadIdx.x == 0) {
        block_ws[2 * (int64_t)blockIdx.x] = gs_block_sum<FU_WAVES>(ws_v);
        block_ws[2 * (int64_t)blockIdx.x + 1] = gs_block_sum<FU_WAVES>(ws_t);
    }
}

// exclusive prefix sums of the (crossings, triangles) block sums in place; a block sum is at most 12 * 256, a round's total below 2^20
__global__ __launch_bounds__(FU_THREADS) void k_iso_scan_blocks(int64_t* __restrict__ block_ws, int64_t n_blocks, int64_t* __restrict__ totals)
{
    __shared__ uint32_t ws_v[FU_WAVES], ws_t[FU_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t carry_v = 0, carry_t = 0;
    for (int64_t base = 0; base < n_blocks; base += FU_THREADS) {
        const int64_t at = base + threadIdx.x;
        const uint32_t v = at < n_blocks ? (uint32_t)block_ws[2 * at] : 0u, t = at < n_blocks ? (uint32_t)block_ws[2 * at + 1] : 0u;
        const uint32_t incl_v = gs_wave_scan_incl(v, lane), incl_t = gs_wave_scan_incl(t, lane);
        gs_block_scan_put(ws_v, wave, lane, incl_v);
        gs_block_scan_put(ws_t, wave, lane, incl_t);
        __syncthreads();
        if (at < n_blocks) {
            block_ws[2 * at] = carry_v + gs_block_scan_excl(ws_v, wave, incl_v, v);
            block_ws[2 * at + 1] = carry_t + gs_block_scan_excl(ws_t, wave, incl_t, t);
        }
        carry_v += gs_block_sum<FU_WAVES>(ws_v);
        carry_t += gs_block_sum<FU_WAVES>(ws_t);
        __syncthreads();                                     // the next round's deposits
    }
    if (threadIdx.x == 0) { totals[0] = carry_v; totals[1] = carry_t; }
}

__global__ __launch_bounds__(FU_THREADS) void k_iso_vertices(const gs_iso_volume vol, const uint16_t* __restrict__ cell_ws,
                                                            const int64_t* __restrict__ block_ws, uint32_t* __restrict__ voxel_ws,
                                                            int64_t n_vertices, float* __restrict__ vertices, float* __restrict__ colours)
{
    __shared__ uint32_t ws[FU_WAVES];
    const int64_t n = (int64_t)vol.nx * vol.ny * vol.nz;
    const int64_t idx = (int64_t)blockIdx.x * FU_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t mask = idx < n ? cell_ws[idx] & 0x7fu : 0u;
    const uint32_t count = __popc(mask);
    const uint32_t incl = gs_wave_scan_incl(count, lane);
    gs_block_scan_put(ws, wave, lane, incl);
    __syncthreads();
    if (idx >= n) return;
    const int64_t first = block_ws[2 * (int64_t)blockIdx.x] + gs_block_scan_excl(ws, wave, incl, count);
    voxel_ws[idx] = (uint32_t)first;
    if (!mask) return;
    int i, j, k;
    iso_ijk(idx, vol.ny, vol.nz, i, j, k);
    const float a = vol.values[idx];
    const float ax = vol.origin[0] + (float)i * vol.spacing[0], ay = vol.origin[1] + (float)j * vol.spacing[1], az = vol.origin[2] + (float)k * vol.spacing[2];
    int64_t vertex = first;
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        if (!(mask >> e & 1u)) continue;
        const int delta = ISO_DELTA_OF_TYPE(e), dx = delta >> 2 & 1, dy = delta >> 1 & 1, dz = delta & 1;
        const int64_t out = vertex++;
        // a crossing the plan recorded has its other end inside the volume; the test keeps a foreign work buffer from steering a read
        if (out >= n_vertices || i + dx >= vol.nx || j + dy >= vol.ny || k + dz >= vol.nz) continue;
        const int64_t other = idx + ((int64_t)dx * vol.ny + dy) * vol.nz + dz;
        const float b = vol.values[other];
        const float t = (vol.level - a) / (b - a);
        const float bx = vol.origin[0] + (float)(i + dx) * vol.spacing[0], by = vol.origin[1] + (float)(j + dy) * vol.spacing[1],
                    bz = vol.origin[2] + (float)(k + dz) * vol.spacing[2];
        vertices[3 * out] = ax + t * (bx - ax);
        vertices[3 * out + 1] = ay + t * (by - ay);
        vertices[3 * out + 2] = az + t * (bz - az);
        if (colours && vol.colour) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float ca = vol.colour[3 * idx + c], cb = vol.colour[3 * other + c];
                colours[3 * out + c] = ca + t * (cb - ca);
            }
        }
    }
}

__global__ __launch_bounds__(FU_THREADS) void k_iso_faces(const gs_iso_volume vol, const uint16_t* __restrict__ cell_ws,
                                                         const int64_t* __restrict__ block_ws, const uint32_t* __restrict__ voxel_ws,
                                                         int64_t n_vertices, int64_t n_faces, int32_t* __restrict__ faces)
{
    __shared__ uint32_t ws[FU_WAVES];
    const int64_t n = (int64_t)vol.nx * vol.ny * vol.nz;
    const int64_t idx = (int64_t)blockIdx.x * FU_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t count = idx < n ? (uint32_t)(cell_ws[idx] >> 8) : 0u;
    const uint32_t incl = gs_wave_scan_incl(count, lane);
    gs_block_scan_put(ws, wave, lane, incl);
    __syncthreads();
    if (idx >= n || !count) return;
    int i, j, k;
    iso_ijk(idx, vol.ny, vol.nz, i, j, k);
    if (i + 1 >= vol.nx || j + 1 >= vol.ny || k + 1 >= vol.nz) return;      // a triangle count the plan wrote belongs to a whole cell
    int64_t face = block_ws[2 * (int64_t)blockIdx.x + 1] + gs_block_scan_excl(ws, wave, incl, count);
    int64_t corner_at[8];
    uint32_t in = 0;
#pragma unroll
    for (int code = 0; code < 8; ++code) {
        corner_at[code] = idx + ((int64_t)(code >> 2 & 1) * vol.ny + (code >> 1 & 1)) * vol.nz + (code & 1);
        if (vol.values[corner_at[code]] < vol.level) in |= 1u << code;
    }
    for (int t = 0; t < 6; ++t) {
        uint32_t inside = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) inside |= (in >> ISO_TET_CORNER[t][v] & 1u) << v;
        const uint32_t entry = ISO_CASE[inside];
        const bool exchange = ((ISO_NEGATIVE_TETS >> t & 1u) != 0) != (vol.flip != 0);
        for (uint32_t tri = 0; tri < (entry >> 18); ++tri) {
            int32_t corner[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t edge = entry >> (9 * tri + 3 * c) & 7u;
                const int lower = ISO_TET_CORNER[t][ISO_EDGE_ENDS[edge][0]], upper = ISO_TET_CORNER[t][ISO_EDGE_ENDS[edge][1]];
                const int type = ISO_TYPE_OF_DELTA[upper - lower];
                const int64_t owner = corner_at[lower];
                corner[c] = (int32_t)(voxel_ws[owner] + (uint32_t)__popc(cell_ws[owner] & 0x7fu & ((1u << type) - 1u)));
            }
            const int64_t out = face++;
            if (out >= n_faces) continue;
            faces[3 * out] = corner[0];
            faces[3 * out + 1] = exchange ? corner[2] : corner[1];
            faces[3 * out + 2] = exchange ? corner[1] : corner[2];
        }
    }
}

void gs_launch_iso_plan(const gs_iso_volume& vol, void* cell_ws, void* block_ws, int64_t* totals, hipStream_t s)
{
    const int64_t n = (int64_t)vol.nx * vol.ny * vol.nz, n_blocks = (n + FU_THREADS - 1) / FU_THREADS;
    hipLaunchKernelGGL(k_iso_plan, dim3((unsigned)n_blocks), dim3(FU_THREADS), 0, s, vol, reinterpret_cast<uint16_t*>(cell_ws),
                       reinterpret_cast<int64_t*>(block_ws));
    hipLaunchKernelGGL(k_iso_scan_blocks, dim3(1), dim3(FU_THREADS), 0, s, reinterpret_cast<int64_t*>(block_ws), n_blocks, totals);
}

void gs_launch_iso_emit(const gs_iso_volume& vol, const void* cell_ws, const void* block_ws, void* voxel_ws, int64_t n_vertices,
                        int64_t n_faces, float* vertices, float* colours, int32_t* faces, hipStream_t s)
{
    const int64_t n = (int64_t)vol.nx * vol.ny * vol.nz, n_blocks = (n + FU_THREADS - 1) / FU_THREADS;
    hipLaunchKernelGGL(k_iso_vertices, dim3((unsigned)n_blocks), dim3(FU_THREADS), 0, s, vol, reinterpret_cast<const uint16_t*>(cell_ws),
                       reinterpret_cast<const int64_t*>(block_ws), reinterpret_cast<uint32_t*>(voxel_ws), n_vertices, vertices, colours);
    if (n_faces > 0)
        hipLaunchKernelGGL(k_iso_faces, dim3((unsigned)n_blocks), dim3(FU_THREADS), 0, s, vol, reinterpret_cast<const uint16_t*>(cell_ws),
                           reinterpret_cast<const int64_t*>(block_ws), reinterpret_cast<const uint32_t*>(voxel_ws), n_vertices, n_faces, faces);
}
