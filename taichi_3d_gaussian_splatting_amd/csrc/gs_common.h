// gs_common.h -- shared declarations of libgsrast (HIP, gfx950 only).
//
// Arithmetic contract: every expression that decides an INDEX (frustum test, tile
// box, depth code, the 1/255 and 1e-4 blend thresholds) is evaluated with the same
// IEEE f32 operation sequence on every build of this library: the sources are
// compiled with -ffp-contract=off, division and sqrt are correctly rounded (hipcc
// default), and exp is gs_expf below (add/mul/fma only).  See DESIGN.md "Numerics".
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GS_TILE_SZ 16

// Wave-wide vote.  The intrinsic folds into the v_cmp that produced the predicate (an SGPR-pair mask); HIP's __ballot()
// goes through v_cndmask + v_cmp_ne, two half-rate VALU instructions per vote.
#define gs_ballot(pred) __builtin_amdgcn_ballot_w64(pred)

// Diagnostic builds only, never loaded by the product:
//   `make stats` (-DGS_STATS=2) -> libgsrast_stats.so: event counters of the two blend kernels (tools/blend_stats.py) + wave times;
//   `make times` (-DGS_STATS=1) -> libgsrast_times.so: start / end time of every blend wave ONLY (tools/*_wave_timeline.py).
// The counters are global atomics in the inner loops (~100 ns each on this part): a build that counts runs tens of times
// slower and its wave times say nothing about the real launch, hence the separate timing-only build.
#ifdef GS_STATS
extern __device__ unsigned long long gs_stats_counters[32];
extern __device__ unsigned long long gs_stats_wave_times[2 * 65536];   // start, end (wall clock ticks) of each blend wave
#endif
#if defined(GS_STATS) && GS_STATS >= 2
#define GS_STAT(i, n) do { const unsigned long long gs_stat_n = (unsigned long long)(n); if (threadIdx.x % 64 == 0) atomicAdd(&gs_stats_counters[i], gs_stat_n); } while (0)
#else
#define GS_STAT(i, n) do { } while (0)
#endif
// Projected splat records: four float4 per in-camera point -- A {u, v, conic a, conic b}, B {conic c, rescale, opacity, depth},
// C {r, g, b, log-domain alpha cut}, D {x, y, z in camera, radius} -- kept as ONE 64-byte row per point (the pointers PA..PD
// are rec, rec+1, rec+2, rec+3), so that the blend kernels' gather by sorted index touches one 64-byte segment per splat
// instead of three cache lines, and so that a shard's records are one contiguous (M,16) float array for the Gaussian-parallel
// exchange.  (Four separate planes measured no faster: DESIGN.md, row f-3.)
#define GS_REC(ptr, i) (ptr)[(size_t)(i) * 4]
#define GS_BOUNDARY_TILES 3          // reference RAST:26
#define GS_ALPHA_EPS 0.00392156862745098f   // 1./255. (RAST:451, RAST:634)
#define GS_ALPHA_MAX 0.99f           // RAST:453
#define GS_T_STOP 0.0001f            // RAST:458
#define GS_NFEAT 56
// Cuts of long tile lists (k_blend_fwd writes them, the backward blend of a HEAVY tile starts its segments from them): every
// GS_SEG entries of a list longer than GS_CUT_MIN_LEN the forward stores each pixel's transmittance and accumulated colour.
// Every list longer than one segment is cut: a dense list of 600 - 1000 entries, left whole, is twice the longest segment and was
// what the backward of the clustered 976x544 workload waited for (0.224 -> 0.179 ms; 1024 was the threshold while cutting cost
// an atomic claim and a barrier at the head of the list -- k_blend_fwd.hip).  Segments of 256 entries: no further gain (0.183).
#ifndef GS_SEG
#define GS_SEG 512
#endif
#ifndef GS_CUT_MIN_LEN
#define GS_CUT_MIN_LEN 512
#endif
#define GS_HEAVY_CAP 1024            // most tiles a backward treats as heavy
// tile arrays of a frame, cleared by its first kernel: tile_start | tile_end | tile_work | tile_cut (first cut record + 1, 0 = none) | four spare ints
#define GS_TILE_INTS(T) (4 * (size_t)(T) + 4)
// the four trailing ints: one spare (the cut records' claim counter until their positions became a closed form), then the largest tile count of one point of the frame (k_project -> k_sum_rows), two spare
#define GS_TILE_SPARE_MAX_TILES 3          // index from the END of the tile arrays
// tile_order buffer: order (T) | n_heavy | n_items | pad pad | item_base (GS_HEAVY_CAP + 1)
#define GS_ORDER_INTS(T) ((size_t)(T) + 4 + GS_HEAVY_CAP + 4 + GS_HEAVY_CAP)
#define GS_ORDER_REDO_OFFSET (4 + GS_HEAVY_CAP + 4)      // from n_heavy: one flag per heavy tile, "walk this tile again in one piece" (k_backward.hip)
// the two pad words, from n_heavy: the frame's slots of the context's view table (below), written by block 0 of k_filter
#define GS_ORDER_READ_SLOT 2
#define GS_ORDER_WRITE_SLOT 3

// ---- the view table: dispatch orders of the forward blend, per view (scheduling only) -------------------------------------
// A context keeps the tile order (heaviest first) of the last backward of each of S views and dispatches the next forward blend of a
// view in the order its own last visit left: a trainer revisits a fixed set of cameras in shuffled order, so the LAST backward's order
// belongs to an unrelated view, the same view's order of an epoch ago nearly fits.  The poses are device memory, so the table lives on
// the device and is consulted there: block 0 of k_filter (the first kernel to read the pose) looks the pose of object 0 up among the keys
// and leaves two words in the frame's tile-order buffer; k_blend_fwd reads the order of the frame's read slot, k_tile_order writes its
// order, then the key, into the frame's write slot.  Any permutation of the tiles gives the same bits.
// A forward only reads the table: a frame that is never back-propagated changes nothing in it (the cursor too moves in k_tile_order).
// Words: cursor (the slot the next eviction takes) | last slot written + 1 (0: none) | two spare | S keys of 8 words (q xyzw, t xyz of object 0 as
// given, then the tag: the tile count T once the slot's order is complete, 0 = unfilled) | S + 1 orders of T tiles.  Order S belongs to the
// frames that did not come through k_filter (records-built ones: no pose to key them by); they read whichever slot was written last.
#define GS_VIEW_HDR_INTS 4
#define GS_VIEW_KEY_INTS 8
#define GS_VIEW_MAX_SLOTS 1024
#define GS_VIEW_INTS(S, T) (GS_VIEW_HDR_INTS + (size_t)GS_VIEW_KEY_INTS * (size_t)(S) + ((size_t)(S) + 1) * (size_t)(T))
// Two poses are the same view while d = |q - q'|^2 + |t - t'|^2 / (1 + |t|^2) stays below this (q and -q being one rotation, the
// nearer sign counts).  A rotation by a about any axis moves a unit quaternion by 2 sin(a / 4): d = 1.9e-5 is a rotation of 0.5 degrees, or a
// camera moved by 0.44 % of sqrt(1 + |t|^2).  It separates the drift of pose optimisation (a few hundredths of a degree per epoch: d below
// 1e-6, and the key follows the pose at every backward) from the benchmark's neighbouring views, 2 degrees apart: d = 3.05e-4.
#define GS_VIEW_SAME_D 1.9e-5f
struct GsViewTable {
    int32_t* base;      // NULL: no table (GS_VIEW_HINTS=0, or no tile)
    int S, T;
    __host__ __device__ int32_t* key(int slot) const { return base + GS_VIEW_HDR_INTS + GS_VIEW_KEY_INTS * slot; }
    __host__ __device__ int32_t* order(int slot) const { return base + GS_VIEW_HDR_INTS + GS_VIEW_KEY_INTS * S + (size_t)slot * (size_t)T; }
    // S = 1: one slot for everything, the behaviour before the table -- every pose matches it, so no frame looks its pose up: all are keyless
    __host__ __device__ int keyless_slot() const { return S > 1 ? S : 0; }
};

// Per-object pose record built once per frame (every k_filter block derives it, block 0 stores it).
struct GsPose {
    float R[9];          // rotation_matrix_from_quaternion(conj(q_pointcloud_camera)), GP3D:30-48
    float t[3];          // t_camera_pointcloud, UTIL:426-432
    float origin_fwd[3]; // camera centre as forward computes it: taichi_inverse_SE3, RAST:280-282
    float origin_bwd[3]; // camera centre as backward reads it: t_pointcloud_camera, RAST:731-732
    float q_cp[4];
    float pad[2];
};

// ---- pose gradient (k_pose.hip; the per-point part of its math is in gs_point_math.h) -----------------------------------
// The per-object end of the pose gradient: from g = (dL/dW (9, row-major), dL/dt_cp (3), dL/do (3)) summed over the object's
// points to dL/dq_pointcloud_camera (4) and dL/dt_pointcloud_camera (3), through what make_pose (k_project.hip) computes:
//   q' = (-qx, -qy, -qz, qw);  W = R(q') by the un-normalised formula (GP3D:30-48);
//   t_cp = -(n t_pc n*) with n = q' / |q'| (UTIL:426-432);  o = -W^T t_cp (origin_fwd, UTIL:495-510).
// P is the frame's pose record: P.q_cp = q', P.origin_bwd = t_pc, P.R = W, P.t = t_cp.
__device__ __forceinline__ void gs_pose_grad_chain(const GsPose& P, const float g[15], float gq[4], float gt[3])
{
    float dW[9], dt[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) dW[k] = g[k];
    const float* dO = g + 12;
    // o_i = -sum_j W_ji t_j
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int i = 0; i < 3; ++i) dW[3 * j + i] -= P.t[j] * dO[i];
        dt[j] = g[9 + j] - ((P.R[3 * j] * dO[0] + P.R[3 * j + 1] * dO[1]) + P.R[3 * j + 2] * dO[2]);
    }
    // W = R(q'), q' = (x, y, z, w) not normalised
    const float x = P.q_cp[0], y = P.q_cp[1], z = P.q_cp[2], w = P.q_cp[3];
    float gx = 2.0f * (y * (dW[1] + dW[3]) + z * (dW[2] + dW[6]) + w * (dW[7] - dW[5])) - 4.0f * x * (dW[4] + dW[8]);
    float gy = 2.0f * (x * (dW[1] + dW[3]) + w * (dW[2] - dW[6]) + z * (dW[5] + dW[7])) - 4.0f * y * (dW[0] + dW[8]);
    float gz = 2.0f * (w * (dW[3] - dW[1]) + x * (dW[2] + dW[6]) + y * (dW[5] + dW[7])) - 4.0f * z * (dW[0] + dW[4]);
    float gw = 2.0f * (z * (dW[3] - dW[1]) + y * (dW[2] - dW[6]) + x * (dW[7] - dW[5]));
    // t_cp = -rot, rot = n v n* = (nw^2 - u.u) v + 2 (u.v) u + 2 nw (u x v), u = n.xyz, v = t_pc; h = dL/drot
    const float nrm = sqrtf(x * x + y * y + z * z + w * w);
    const float ux = x / nrm, uy = y / nrm, uz = z / nrm, nw = w / nrm;
    const float vx = P.origin_bwd[0], vy = P.origin_bwd[1], vz = P.origin_bwd[2];
    const float hx = -dt[0], hy = -dt[1], hz = -dt[2];
    const float hv = hx * vx + hy * vy + hz * vz, uh = ux * hx + uy * hy + uz * hz, uv = ux * vx + uy * vy + uz * vz;
    const float uu = ux * ux + uy * uy + uz * uz, ww = nw * nw;
    // d(h . rot)/du = -2 (h.v) u + 2 (u.h) v + 2 (u.v) h + 2 nw (v x h);  d/dnw = 2 nw (h.v) + 2 h.(u x v)
    const float gnx = -2.0f * hv * ux + 2.0f * uh * vx + 2.0f * uv * hx + 2.0f * nw * (vy * hz - vz * hy);
    const float gny = -2.0f * hv * uy + 2.0f * uh * vy + 2.0f * uv * hy + 2.0f * nw * (vz * hx - vx * hz);
    const float gnz = -2.0f * hv * uz + 2.0f * uh * vz + 2.0f * uv * hz + 2.0f * nw * (vx * hy - vy * hx);
    const float gnw = 2.0f * nw * hv + 2.0f * (hx * (uy * vz - uz * vy) + hy * (uz * vx - ux * vz) + hz * (ux * vy - uy * vx));
    // n = q' / |q'|: the tangential part, divided by |q'|
    const float ng = ux * gnx + uy * gny + uz * gnz + nw * gnw;
    gx += (gnx - ux * ng) / nrm; gy += (gny - uy * ng) / nrm; gz += (gnz - uz * ng) / nrm; gw += (gnw - nw * ng) / nrm;
    gq[0] = -gx; gq[1] = -gy; gq[2] = -gz; gq[3] = gw;
    // d(h . rot)/dv = (nw^2 - u.u) h + 2 (u.h) u + 2 nw (h x u)
    gt[0] = (ww - uu) * hx + 2.0f * uh * ux + 2.0f * nw * (hy * uz - hz * uy);
    gt[1] = (ww - uu) * hy + 2.0f * uh * uy + 2.0f * nw * (hz * ux - hx * uz);
    gt[2] = (ww - uu) * hz + 2.0f * uh * uz + 2.0f * nw * (hx * uy - hy * ux);
}

// Device-side frame counters, mirrored to pinned host memory once per forward.
struct GsCounters {
    int32_t M;               // points in camera
    uint32_t K;              // sort pairs
    int32_t max_depth_code;  // max over visible points of i32(depth * scale)
    int32_t reserved;        // host mirror only: ticket of the forward that published these values
    int32_t bad_object_ids;  // valid rows whose point_object_id is outside [0, n_objects): treated as not in camera, reported
    int32_t pad[3];
};

// One thread hands the frame counters to the host (see k_project.hip: k_scan_tiles_publish, k_binning.hip: k_keygen).
__device__ __forceinline__ void gs_publish_counters(GsCounters* __restrict__ counters, uint32_t K, volatile GsCounters* host_mirror, int32_t ticket)
{
    counters->K = K;
    host_mirror->M = counters->M;
    host_mirror->K = K;
    host_mirror->max_depth_code = counters->max_depth_code;
    host_mirror->bad_object_ids = counters->bad_object_ids;
    __threadfence_system();
    host_mirror->reserved = ticket;              // the host waits for this value
    __threadfence_system();
    // the accumulating counters start the next frame at zero (zero at gs_create for the first one): no clearing
    // launch, and no block of the next k_filter / k_project can run ahead of a clear
    counters->max_depth_code = 0;
    counters->bad_object_ids = 0;
}

// ---- device math -------------------------------------------------------------
__device__ __forceinline__ float gs_expf(float x)
{
    x = x < -86.0f ? -86.0f : x;                     // the oracle's two compares, so that a NaN parameter stays a NaN as in the reference
    x = x > 88.0f ? 88.0f : x;                       // (v_med3_f32 / v_min / v_max would return the finite operand)
    float fx = x * 1.44269504088896341f;
    float n = (fx + 12582912.0f) - 12582912.0f;      // round to nearest even
    float r = __builtin_fmaf(n, -0.693359375f, x);
    r = __builtin_fmaf(n, 2.12194440e-4f, r);
    float z = r * r;
    float p = 1.9875691500E-4f;
    p = __builtin_fmaf(p, r, 1.3981999507E-3f);
    p = __builtin_fmaf(p, r, 8.3334519073E-3f);
    p = __builtin_fmaf(p, r, 4.1665795894E-2f);
    p = __builtin_fmaf(p, r, 1.6666665459E-1f);
    p = __builtin_fmaf(p, r, 5.0000001201E-1f);
    float y = __builtin_fmaf(p, z, r);
    y = y + 1.0f;
    int32_t bits = __float_as_int(y) + (((int32_t)n) << 23);
    return __int_as_float(bits);
}

// exp of the Gaussian falloff in the blend kernels (oracle: gso_exp_blend, same sequence bit for bit): eleven VALU
// instructions where gs_expf takes seventeen.  2^(x log2 e): integer part through the 1.5*2^23 constant, fraction with one
// fused multiply-add (the rounding of x*log2(e) does not enter), degree-5 polynomial for 2^f on [-0.5, 0.5], the integer
// added to the exponent field (v_lshl_add_u32).  Within 3e-7 of exp for x in [-10, 0].
__device__ __forceinline__ float gs_exp_blend(float x)
{
    x = __builtin_amdgcn_fmed3f(x, -86.0f, 88.0f);   // (a NaN exponent -- NaN position, rotation or scale -- becomes -86: such a splat has no
                                                     // defined tile box in the reference either; NaN colour and opacity do propagate)
    const float L = 1.44269504088896341f;
    const float t = x * L;
    const float m = t + 12582912.0f;
    const float n = m - 12582912.0f;
    const float f = __builtin_fmaf(x, L, -n);
    float q = 0.0013264712179079652f;
    q = __builtin_fmaf(q, f, 0.009671511128544807f);
    q = __builtin_fmaf(q, f, 0.05550733581185341f);
    q = __builtin_fmaf(q, f, 0.24022242426872253f);
    q = __builtin_fmaf(q, f, 0.6931470036506653f);
    const float p = __builtin_fmaf(q, f, 1.0f);
    return __uint_as_float(__float_as_uint(p) + (__float_as_uint(m) << 23));
}

__device__ __forceinline__ float gs_sigmoid(float x) { return 1.0f / (1.0f + gs_expf(-x)); }

// C[r x c] = A[r x k] @ B[k x c]; terms summed k = 0,1,2,... like the Python matmul chain.
template <int R, int K, int C>
__device__ __forceinline__ void gs_mm(const float* A, const float* B, float* Cout)
{
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < C; ++j) {
            float acc = A[i * K] * B[j];
#pragma unroll
            for (int t = 1; t < K; ++t) acc = acc + A[i * K + t] * B[t * C + j];
            Cout[i * C + j] = acc;
        }
}

// Tile box of a splat, RAST:81-103.  box = {min_tile_u, max_tile_u, min_tile_v, max_tile_v}
__device__ __forceinline__ void gs_tile_box(float u, float v, float radii, int tiles_u, int tiles_v, int box[4])
{
    radii = radii > 1.0f ? radii : 1.0f;
    float min_u = u - radii; min_u = min_u > 0.0f ? min_u : 0.0f;
    float max_u = u + radii;
    float min_v = v - radii; min_v = min_v > 0.0f ? min_v : 0.0f;
    float max_v = v + radii;
    int a = (int)floorf(min_u / 16.0f); a = a < tiles_u ? a : tiles_u;
    int b = (int)floorf(max_u / 16.0f) + 1; b = b > a + 1 ? b : a + 1; b = b < tiles_u ? b : tiles_u;
    int c = (int)floorf(min_v / 16.0f); c = c < tiles_v ? c : tiles_v;
    int d = (int)floorf(max_v / 16.0f) + 1; d = d > c + 1 ? d : c + 1; d = d < tiles_v ? d : tiles_v;
    box[0] = a; box[1] = b; box[2] = c; box[3] = d;
}

// wave64 helpers -----------------------------------------------------------------
template <int CTRL, int ROW_MASK = 0xf, int BANK_MASK = 0xf, bool BOUND = true>
__device__ __forceinline__ float gs_dpp(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, BANK_MASK, BOUND));
}

// Sum of eleven values over the 64 lanes (totals valid in lanes 48..63, all of row 3): six DPP steps
// (quad_perm x2, row_half_mirror, row_mirror, row_bcast:15, row_bcast:31), written as v_add_f32_dpp so that every step is ONE
// instruction per value (hipcc lowers the builtin form to v_mov_dpp + add, and to three
// instructions for the row_bcast steps).  A DPP source written by the previous VALU instruction
// needs two wait states: each step starts with s_nop 1; inside a step the eleven registers
// are independent and eleven instructions apart from their next use.
#define GS_DPP11(ctrl)                                                                              \
    asm volatile("s_nop 1\n\t"                                                                      \
                 "v_add_f32_dpp %0, %0, %0 " ctrl "\n\t"                                            \
                 "v_add_f32_dpp %1, %1, %1 " ctrl "\n\t"                                            \
                 "v_add_f32_dpp %2, %2, %2 " ctrl "\n\t"                                            \
                 "v_add_f32_dpp %3, %3, %3 " ctrl "\n\t"                                            \
                 "v_add_f32_dpp %4, %4, %4 " ctrl "\n\t"                                            \
                 "v_add_f32_dpp %5, %5, %5 " ctrl "\n\t"                                            \
                 "v_add_f32_dpp %6, %6, %6 " ctrl "\n\t"                                            \
                 "v_add_f32_dpp %7, %7, %7 " ctrl "\n\t"                                            \
                 "v_add_f32_dpp %8, %8, %8 " ctrl "\n\t"                                            \
                 "v_add_f32_dpp %9, %9, %9 " ctrl "\n\t"                                            \
                 "v_add_f32_dpp %10, %10, %10 " ctrl "\n\t"                                         \
                 : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), \
                   "+v"(v[7]), "+v"(v[8]), "+v"(v[9]), "+v"(v[10]))

__device__ __forceinline__ void gs_wave_sum11_row3(float (&v)[11])
{
    GS_DPP11("quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf");
    GS_DPP11("quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf");
    GS_DPP11("row_half_mirror row_mask:0xf bank_mask:0xf");
    GS_DPP11("row_mirror row_mask:0xf bank_mask:0xf");
    GS_DPP11("row_bcast:15 row_mask:0xa bank_mask:0xf");     // rows 1,3 += lane 15 of rows 0,2; rows 0,2 untouched
    GS_DPP11("row_bcast:31 row_mask:0xc bank_mask:0xf");     // rows 2,3 += lane 31
    asm volatile("s_nop 1");
}

__device__ __forceinline__ int gs_wave_sum_i(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// a float over the 64 lanes, every lane the total: butterfly from distance 1 up (the order is part of the pose gradient's bits)
__device__ __forceinline__ float gs_wave_sum_f(float v)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int gs_wave_max_i(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { int w = __shfl_xor(v, o, 64); v = v > w ? v : w; }
    return v;
}

// inclusive scan over the 64 lanes (lane 63 holds the wave's total)
__device__ __forceinline__ uint32_t gs_wave_scan_incl(uint32_t v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(v, o, 64); if (lane >= o) v += t; }
    return v;
}
// Block reductions and scans over NW waves go through an NW-word LDS array in two halves, a deposit and a combine; the __syncthreads()
// between them stays in the KERNEL, where one barrier often serves several of these (and other LDS) at once.
//   reduction:  gs_block_put(ws, wave, lane, <the wave's total, in every lane>);  barrier;  gs_block_sum<NW>(ws) / gs_block_max<NW>(ws)
//   scan:       incl = gs_wave_scan_incl(v, lane);  gs_block_scan_put(ws, wave, lane, incl);  barrier;
//               gs_block_scan_excl(ws, wave, incl, v) = the waves before mine + the lanes before me;  total = gs_block_sum<NW>(ws)
template <typename T> __device__ __forceinline__ void gs_block_put(T* ws, int wave, int lane, T v) { if (lane == 0) ws[wave] = v; }
__device__ __forceinline__ void gs_block_scan_put(uint32_t* ws, int wave, int lane, uint32_t incl) { if (lane == 63) ws[wave] = incl; }
template <int NW, typename T> __device__ __forceinline__ T gs_block_sum(const T* ws) { if constexpr (NW == 1) return ws[0]; else return gs_block_sum<NW - 1>(ws) + ws[NW - 1]; }
template <int NW> __device__ __forceinline__ int gs_block_max(const int* ws) { if constexpr (NW == 1) return ws[0]; else return max(gs_block_max<NW / 2>(ws), gs_block_max<NW / 2>(ws + NW / 2)); }
__device__ __forceinline__ uint32_t gs_block_scan_excl(const uint32_t* ws, int wave, uint32_t incl, uint32_t v)
{
    uint32_t woff = 0;
    for (int w = 0; w < wave; ++w) woff += ws[w];
    return woff + incl - v;
}
// in-block exclusive rank of `pred` in thread order and the block's total, for a block of NW waves (every thread of the block must call
// it; s_wave: NW words of LDS, free for the next call when this one returns)
template <int NW>
__device__ __forceinline__ int gs_block_rank(bool pred, int* s_wave, int* total)
{
    const unsigned long long b = gs_ballot(pred);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) s_wave[w] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) { const int c = s_wave[i]; before += i < w ? c : 0; all += c; }
    __syncthreads();
    *total = all;
    return before + __popcll(b & ((1ull << lane) - 1ull));
}
// counts[0 .. block) summed by a block of NT threads (a few thousand L2-resident words read by every block, instead of a scan launch in
// between): every lane gets its WAVE's share, the caller folds the shares with a block sum
template <int NT, typename T> __device__ __forceinline__ T gs_sum_of_blocks_before(const T* __restrict__ counts, int block)
{
    T pre = 0;
    for (int j = threadIdx.x; j < block; j += NT) pre += counts[j];
    return (T)gs_wave_sum_i((int)pre);
}

// ---- optional per-kernel timing with HIP events on the launch stream -------------
// Kernel ids index the comma-separated list returned by gs_kernel_names().
enum GsKernelId { KID_FILTER = 0, KID_PUBLISH, KID_PROJECT, KID_KEYGEN,
                  KID_SORT_HIST, KID_SORT_ROWSCAN, KID_SORT_SCATTER, KID_BLEND_FWD,
                  KID_BLEND_BWD, KID_BWD_POINTS, KID_SUM_ROWS, KID_TILE_ORDER, KID_BLEND_BWD_REPAIR, KID_COUNT_ };
struct GsProf;
int gs_prof_begin(GsProf* p, int kid, hipStream_t s);     // returns a record index or -1
void gs_prof_end(GsProf* p, int rec, hipStream_t s);
#define GS_TIMED(prof, kid, stream, ...)                     \
    do {                                                     \
        int rec__ = gs_prof_begin((prof), (kid), (stream));  \
        __VA_ARGS__;                                         \
        gs_prof_end((prof), rec__, (stream));                \
    } while (0)

// ---- host-side launch wrappers (implemented in the k_*.hip files) --------------
// A frame's device buffers, sliced into what its kernels read and write (gs_api.hip: frame_view, the one place that knows how
// they are laid out).
struct GsFrameView {
    float4 *PA, *PB, *PC, *PD;                  // record rows A..D of each point (GS_REC)
    ushort4* box; int32_t* ntiles;
    int32_t* depth_codes;                       // (M) i32(depth * scale) per in-camera point, for the key build
    uint32_t* offsets;                          // (M) exclusive scan of ntiles, written by keygen
    int32_t* ids; int32_t* cam_index; int8_t* mask; GsPose* pose;
    int T;
    // the tile arrays, cleared together by the frame's first kernel (tile_ints ints from tile_start on)
    int32_t *tile_start, *tile_end;             // written by the forward blend (each tile's block finds its range in the sorted keys)
    int32_t* tile_work;                         // (T) max over the tile's pixels of last - start (k_blend_fwd)
    int32_t* tile_cut;                          // (T) first cut record of each tile + 1, 0 = none
    int32_t* max_tiles;                         // the frame's largest tile count of one point (k_project -> k_sum_rows)
    int tile_ints;
    int32_t* tile_order;                        // (T) scheduling: heaviest tiles first (k_tile_order)
    int32_t* n_heavy;                           // number of heavy tiles at the head of tile_order (k_tile_order -> k_blend_bwd_tile); n_items and item_base follow it
    const void* keys_sorted; const int32_t* vals_sorted;   // the sorted pairs: whichever of the ping-pong buffers holds them
    float4* cuts; float2* cut_mag;              // list cuts of the forward (NULL: none), per-segment |d uv| partial sums
};

struct GsProjectArgs {
    GsProf* prof;
    const float* point_cloud; float* features; const int8_t* invalid; const int32_t* object_id;
    int64_t N; const float* q_pc; const float* t_pc; int n_objects; const float* Kmat;
    int H, W; float near_plane, far_plane, depth_scale;
    GsFrameView v;                              // written: pose, mask, ids, cam_index, records, box, ntiles, depth codes; tile arrays cleared before the binning
    int32_t* block_counts; int32_t* block_offsets; uint32_t* tile_block_sums;
    // (256, blocks) pair counts per low byte of the depth code and block of this stage, with room for the scanned table behind it
    // (gs_first_hist_elems), or NULL: the sort's first radix pass as k_keygen does it (k_binning.hip)
    uint32_t* first_hist;
    GsCounters* counters;
    GsCounters* host_mirror; int32_t ticket;    // pinned host copy of the counters; .reserved = ticket once they are valid
    GsViewTable views;                          // base != NULL: block 0 of k_filter looks the pose up and writes the frame's two slot words
};
void gs_launch_project(const GsProjectArgs& a, hipStream_t s, bool publish);
void gs_launch_publish(const GsProjectArgs& a, int n_blocks, hipStream_t s);    // the hand-over of the counters as a launch of its own
// the per-pixel half started from records (gs_forward_projected): tile boxes, counts, block sums and the depth-code range
// from the records, then the same scan + publication as gs_launch_project
void gs_launch_boxes_from_records(const GsProjectArgs& a, int M, hipStream_t s, bool publish);

struct GsBinArgs {
    GsProf* prof;
    // M and K are BOUNDS here: the per-pixel half may be queued before the host has read the frame's counters (gs_api.hip,
    // "predicted sizing").  M bounds the in-camera offsets (N rows when unknown); K is the pair capacity the launch geometry and
    // the buffers were sized for -- every kernel works on min(counters->K, K) pairs, read on the device.
    int64_t N; int M; uint32_t K; const GsCounters* counters; int tiles_x; int depth_bits; int key_bits;
    GsFrameView v;                              // read: box, ntiles, depth codes; written: offsets
    const uint32_t* tile_block_sums;
    GsCounters* counters_rw; GsCounters* host_mirror; int32_t ticket;   // host_mirror != NULL: the last k_keygen block publishes the frame counters
    const int32_t *block_offsets, *block_counts;   // k_project's blocks (first in-camera offset, count); NULL: 256 consecutive records per block
    void *keys_a, *keys_b; int32_t *vals_a, *vals_b;       // ping-pong (K); keys of key_bytes bytes
    int key_bytes;                                         // 2, 4 or 8: the frame's key class (gs_sort_key.h: gs_key_bytes)
    uint32_t* hist;                             // (256 * sort_blocks) + scratch
    // the per-point stage's digit table (GsProjectArgs::first_hist) when k_keygen is to do the first radix pass itself, or NULL: the
    // host's decision (gs_api.hip: run_raster_stage); taken only where depth_bits >= 8
    uint32_t* first_hist;
    uint32_t* scan_tmp;                         // GS_SORT_DIGITS digit totals of the current pass
    void** keys_sorted; int32_t** vals_sorted;       // out: which of a/b holds the result
};
void gs_launch_binning(const GsBinArgs& a, hipStream_t s);
size_t gs_sort_hist_elems(uint32_t K);
size_t gs_first_hist_elems(int64_t rows);        // words of first_hist for a per-point stage over `rows` rows: raw + scanned
#define GS_SORT_DIGITS 256          // words of scan_tmp: one row total per digit (k_binning.hip: k_sort_rowscan)

struct GsBlendFwdArgs {
    GsProf* prof;
    int H, W, tiles_x; int rgb_only;
    GsFrameView v;                 // read: sorted pairs, records; written: tile ranges, tile_work, list cuts for the backward (v.cuts NULL: none wanted)
    int key_bytes, depth_bits; uint32_t K; const GsCounters* counters;   // min(counters->K, K) pairs (see GsBinArgs)
    float* image; float* depth; float* acc_alpha; int32_t* last; int32_t* count;
    int cut_cap;
    // the dispatch order (scheduling only): order *view_slot - view_slot_bias of the view table, a permutation of the tiles, heaviest first,
    // from an earlier frame of this ctx; a negative slot, or views.base NULL, is the natural order
    GsViewTable views; const int32_t* view_slot; int view_slot_bias;
};
void gs_launch_blend_fwd(const GsBlendFwdArgs& a, hipStream_t s);

struct GsBackwardArgs {
    GsProf* prof;
    int64_t N; int M; uint32_t K; int H, W, tiles_x;
    GsFrameView v;                                   // the frame's records, pairs, tile arrays, tile order and cuts
    // base != NULL: k_tile_order leaves a second copy of the order, which outlives the frame, in slot *view_slot of the view table (view_slot
    // NULL: in the keyless slot) and then keys the slot with the frame's pose of object 0
    GsViewTable views; const int32_t* view_slot;
    const float* grad_image; const float* acc_alpha; const int32_t* last;
    // gs_backward_ex: upstream gradients of rasterized_depth (with the forward's depth) and of pixel_accumulated_alpha, (H,W) or
    // NULL; aux = 1 selects the AUX kernels (k_blend_bwd_tile, k_sum_rows, k_bwd_points, k_pose_points) and requires v.cuts = NULL
    const float* grad_depth; const float* depth; const float* grad_alpha; int aux;
    int G;                         // waves per tile in k_blend_bwd_tile (1, 2 or 4) = rows of `partial` per (point, tile) pair
    int item_cap;                   // work items of heavy tiles the launch has room for when there are cuts
    int heavy_factor_x2;            // a tile is heavy from this many half-means of work on; 0: no tile is (GS_BWD_SPLIT_HEAVY=0)
    int strict;                     // gs_config.bwd_reference_order: loop 1's UTIL:331-348 in the reference's own operation order
    float* partial;                 // (K*G,12) per (point,tile[,quadrant group]) sums in slot order
    uint8_t* visited;               // (K*G) == gen where the row of `partial` was written by this backward
    uint8_t gen;                    // this backward's tag (1..255): flags are never cleared per backward, a stale one just does not match
    uint8_t* touched;               // (M) == gen where some pixel took a contribution from the point
    const float4* zero_row;         // that row
    const int32_t* max_tiles_hint;  // device: v.max_tiles when k_project computed it, or NULL
    float4* sums;                   // (M,3) per-point sums of the visited rows (count as int32 bits in [10])
    const float* point_cloud; const float* features; const int32_t* object_id; const float* Kmat;
    int sh_band; float f_color, f_high, f_s, f_q, f_alpha;
    float* grad_pc; float* grad_feat; float* grad_uv; float* mag; float* mag_image; int32_t* n_affected;
    // 1: gs_launch_backward_blend writes what an untouched point receives into every per-point output, the hook's copies of forward data
    // and the controller's in-camera count (fill blocks of k_blend_bwd_tile's launch), and gs_launch_backward_points visits the touched
    // points only.  The host decides once per call (gs_api.hip: backward_impl); 0 wherever the two halves do not
    // run in one call or the blend is not launched.
    int prefill;
    // 1: k_sum_rows in its mapping over compacted live points, 0: four lanes per point over all M (the same sums, bit for bit).
    // Set with the blend half of the arguments (gs_api.hip: prepare_backward_blend); GS_BWD_PREFILL=0 selects 0.
    int live_sums;
    float* hook_gpc; float* hook_gfeat; float* hook_guv; float* hook_mag;
    int32_t* hook_ids; int32_t* hook_ntiles; float* hook_depth; float* hook_uv;
    // adaptive-controller accumulators (CTRL:114-141), all nullable together
    int32_t* c_num_in_camera; int32_t* c_num_pixels; float* c_vs_grad; float* c_vs_grad_avg; float* c_pos_grad; float* c_pos_grad_norm;
};
void gs_launch_backward_blend(const GsBackwardArgs& a, hipStream_t s);     // tile order, blend backward, per-splat sums -> a.sums
void gs_launch_backward_points(const GsBackwardArgs& a, hipStream_t s);    // a.sums -> every gradient / hook array
// a.sums -> dL/dq_pointcloud_camera (n_objects,4) and dL/dt_pointcloud_camera (n_objects,3) (k_pose.hip); scratch: gs_pose_scratch_size bytes
size_t gs_pose_scratch_size(int M, int n_objects);
void gs_launch_pose_grad(const GsBackwardArgs& a, int n_objects, void* scratch, float* grad_q, float* grad_t, hipStream_t s);

// per-Gaussian feature channels over a frame (k_channels.hip; include/gs_channels.h).  Forward: values (N,C) -> out (H,W,C);
// backward: grad_out (H,W,C) -> grad_values (N,C), whose rows outside the camera the caller has zeroed.
struct GsChannelsArgs {
    GsFrameView v;                              // read: sorted pairs, records, ids, tile ranges; the backward also box, offsets, ntiles
    int M; uint32_t K; int H, W, tiles_x; int C;
    const int32_t* last;                        // the forward's pixel_offset_of_last_effective_point
    const float* values; float* out;
    const float* grad_out; float* grad_values;
    // backward scratch of one channel chunk: (4K, chunk) partial rows, one per (point, tile, quadrant) in slot order; 4K row flags
    // with the M per-point `touched` bytes behind them (flag_bytes in all, cleared before every chunk)
    float* partial; uint8_t* flags; uint8_t* touched; size_t flag_bytes;
};
int gs_channels_chunk(int C);                   // channels per pass: 4, 16 or 32
void gs_launch_channels_fwd(const GsChannelsArgs& a, hipStream_t s);
hipError_t gs_launch_channels_bwd(const GsChannelsArgs& a, hipStream_t s);

// the argument of k_export, passed by value
struct GsExportArgs { int what; int64_t N; int M; uint32_t K; int T; int depth_bits; int key_bytes;
    const int32_t* depth_codes;     // (M) per point: the low byte a narrow key left out (gs_sort_key.h)
    const int32_t* ids; const float4 *PA, *PB, *PC, *PD; const int32_t* ntiles; const uint32_t* offsets;
    const void* keys_sorted; const int32_t* vals_sorted; const int32_t *tile_start, *tile_end; const int8_t* mask; void* dst; };
void gs_launch_export(const GsExportArgs& a, hipStream_t s);

// a (3,H,W) f32 image as the loss kernels see it: element (c, y, x) at p[c * sc + y * sy + x * sx] (strides in floats), optionally
// passed through torch.clamp(., 0, 1) on the fly
struct GsLossImage { const float* p; long long sc, sy, sx; int clamp; };
size_t gs_loss_maps_size(int H, int W);          // the three padded derivative maps the forward leaves for the backward
size_t gs_loss_partials_floats(int H, int W);      // per-block partial sums of the forward
void gs_launch_loss_forward(const GsLossImage& X, const GsLossImage& Y, int H, int W, float lambda, float* maps, float* partials, float* terms,
                            hipStream_t s);
void gs_launch_loss_backward(const GsLossImage& X, const GsLossImage& Y, int H, int W, float lambda, const float* maps, const float* upstream,
                             const GsLossImage& G, hipStream_t s);
// the same with per-pixel weights (include/gs_loss_weighted.h): weight is a contiguous (H,W) plane; terms has five floats
size_t gs_loss_weighted_partials_floats(int H, int W);
void gs_launch_loss_weighted_forward(const GsLossImage& X, const GsLossImage& Y, const float* weight, int H, int W, float lambda, float* maps,
                                     float* partials, float* terms, hipStream_t s);
void gs_launch_loss_weighted_backward(const GsLossImage& X, const GsLossImage& Y, const float* weight, int H, int W, float lambda,
                                      const float* maps, const float* terms, const float* upstream, const GsLossImage& G, hipStream_t s);
void gs_launch_adam(float* param, const float* grad, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                    int64_t step, hipStream_t s);
// torch.optim.Adam's update of ONE element (no weight decay, no amsgrad): the arithmetic of k_adam (k_loss.hip) and of
// k_adam_rows (k_sparse.hip), stated once.  bias1 = 1 - beta1^t, bias2_sqrt = sqrt(1 - beta2^t), rounded to f32 by the launcher.
__device__ __forceinline__ void gs_adam_update(float& p, const float g, float& m_io, float& v_io, const float lr, const float beta1,
                                               const float beta2, const float eps, const float bias1, const float bias2_sqrt)
{
    const float m = beta1 * m_io + (1.0f - beta1) * g;                // exp_avg.lerp_(grad, 1 - beta1)
    // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2); g * g first, as torch's GPU addcmul: a gradient whose square
    // overflows f32 makes v infinite (and the step zero) there too, rather than finite through (1 - beta2) g first
    const float v = beta2 * v_io + (1.0f - beta2) * (g * g);
    m_io = m; v_io = v;
    const float denom = sqrtf(v) / bias2_sqrt + eps;
    p = p - (lr / bias1) * (m / denom);
}
// the two bias corrections of step t as the kernels take them
void gs_adam_bias(float beta1, float beta2, int64_t step, float* bias1, float* bias2_sqrt);
// k_sparse.hip (include/gs_sparse.h).  Compaction: ids_in[m] of the M in-camera points whose tag is `gen`, in m order ->
// ids_out[0 .. *count_out); block_totals: gs_rows_blocks(M) words of scratch.  touched must be 4-byte aligned with M rounded
// up to 4 readable bytes.
int gs_rows_blocks(int M);
void gs_launch_touched_rows(const uint8_t* touched, uint8_t gen, const int32_t* ids_in, int M, uint32_t* block_totals,
                            int32_t* ids_out, int64_t capacity, int32_t* count_out, hipStream_t s);
void gs_launch_adam_rows(float* param, const float* grad, float* m, float* v, int64_t n_rows, int row_len, const int32_t* ids,
                         const int32_t* count, int64_t max_count, float lr, float beta1, float beta2, float eps, int64_t step, hipStream_t s);
// k_exchange.hip (include/gs_exchange.h): rows ids[0 .. *count) of the two dense gradients as packed rows of 60 words, and the merge of
// n_lists packed lists (list l at packed + l * list_stride rows) into the union list and the summed dense rows.  tag:
// gs_merge_tag_bytes(n_rows) bytes, ids_all: n_lists * list_stride words, block_totals: gs_rows_blocks(n_rows) words of scratch.
// gs_launch_touched_rows with ids_in == NULL lists the tagged positions themselves.
void gs_launch_pack_rows(const float* grad_features, const float* grad_pointcloud, int64_t n_rows, const int32_t* ids, const int32_t* count,
                         int64_t max_count, float* packed_out, hipStream_t s);
size_t gs_merge_tag_bytes(int64_t n_rows);
void gs_launch_merge_rows(const float* packed, const int32_t* counts, int n_lists, int64_t list_stride, int64_t n_rows, float* grad_features_out,
                          float* grad_pointcloud_out, int32_t* union_ids_out, int64_t union_capacity, int32_t* union_count_out, uint8_t* tag,
                          int32_t* ids_all, uint32_t* block_totals, hipStream_t s);
// k_knn.hip (include/gs_knn.h): exact k nearest neighbours of the n rows of xyz; the four work buffers hold gs_knn_*_bytes(n)
size_t gs_knn_sort_bytes(int64_t n);
size_t gs_knn_hist_bytes(int64_t n);
size_t gs_knn_points_bytes(int64_t n);
size_t gs_knn_tree_bytes(int64_t n);
void gs_launch_knn(const float* xyz, const int8_t* invalid, int64_t n, int k, float* d2_out, int32_t* idx_out,
                   void* sort_ws, void* hist_ws, void* pts_ws, void* tree_ws, hipStream_t s);
// k_mixture.hip (include/gs_mixture.h): log-density (fourier == 0, out n_q floats) or Fourier transform (out n_q (re, im) pairs) of the
// scene read as a mixture; the three work buffers hold gs_mix_*_bytes
size_t gs_mix_record_bytes(int64_t n_points);
size_t gs_mix_sum_bytes(int64_t n_points);
size_t gs_mix_partial_bytes(int64_t n_points, int64_t n_q);
void gs_launch_mixture(const float* point_cloud, const float* features, const int8_t* invalid, int64_t n_points, const float* queries,
                       int64_t n_q, int fourier, const float* centre, float* out, void* record_ws, void* sum_ws, void* partial_ws, hipStream_t s);
// the pieces of it the backward calls share: the weights' sum and the records (-> where the sum
// lies in sum_ws, *n_pad_out records written), and the fixed-order total block_sums[n_blocks] of block_sums[0 .. n_blocks)
const double* gs_launch_mixture_records(const float* point_cloud, const float* features, const int8_t* invalid, int64_t n_points,
                                        int fourier, const float* centre, void* record_ws, void* sum_ws, int64_t* n_pad_out, hipStream_t s);
void gs_launch_mix_total(double* block_sums, int64_t n_blocks, hipStream_t s);
// k_mixture_grad.hip (include/gs_mixture_grad.h): the gradients of the two evaluations above to the scene (and to x, if grad_x is
// given), from the upstream gradient `grad_out` (n_q floats, or n_q (re, im) pairs); log_density = the forward's output (density
// only).  record_ws / sum_ws as above; the four others hold gs_mixg_*_bytes (x_partial_ws: the density only, with or without grad_x).
size_t gs_mixg_query_bytes(int64_t n_q);
size_t gs_mixg_partial_bytes(int64_t n_points, int64_t n_q);
size_t gs_mixg_sum_bytes(int64_t n_points, int64_t n_q);
size_t gs_mixg_x_partial_bytes(int64_t n_points, int64_t n_x);
void gs_launch_mixture_grad(const float* point_cloud, const float* features, const int8_t* invalid, int64_t n_points, const float* queries,
                            int64_t n_q, int fourier, const float* centre, const float* log_density, const float* grad_out,
                            float* grad_point_cloud, float* grad_features, float* grad_x, void* record_ws, void* sum_ws, void* query_ws,
                            void* partial_ws, void* gsum_ws, void* x_partial_ws, hipStream_t s);
// k_targets.hip (include/gs_targets.h): the (h_out, w_out) crop of the antialiased resize of a resident image.  One axis of the
// resize as the host made it (gs_api_calls.hip: float64, rounded once): output i reads `count[i]` inputs from `start[i]` on with the
// weights weight[i * taps .. + count[i]); taps <= GS_RS_MAX_TAPS.  The launcher trusts what gs_image_resample checked: the
// window of GS_RESAMPLE_TILE_W consecutive outputs spans at most GS_RS_MAX_SPAN input pixels.
#define GS_RS_MAX_TAPS 18
#define GS_RS_MAX_SPAN 524
struct GsResampleAxis { const int32_t* start; const int32_t* count; const float* weight; int taps; };
// dst_channels 3, or 4 (include/gs_targets_rgba.h; channels must be 4 then): channel 3 through the same filter into plane 3
void gs_launch_image_resample(const void* src, int src_format, int channels, int H_in, int W_in, int64_t pitch_bytes, GsResampleAxis ax,
                              GsResampleAxis ay, int h_out, int w_out, float* dst, int dst_channels, hipStream_t s);
// k_compose.hip (include/gs_compose.h): rows [0, n) of the inputs under the transform A into rows [row_offset, row_offset + n)
// of the outputs.  A as gs_scene_bake made it on the host (float64, rounded once): m = s R_A row-major, t = t_A, q = q_A / |q_A|
// (xyzw), log_scale = log(s), sh = M_0 | M_1 | M_2 | M_3 row-major (1 + 9 + 25 + 49 floats).  Passed by value: wave-uniform.
struct GsBakeTransform { float m[9]; float t[3]; float q[4]; float log_scale; float sh[84]; };
void gs_launch_scene_bake(const float* xyz_in, const float* feat_in, int64_t n, const GsBakeTransform& A, float* xyz_out, float* feat_out,
                          int64_t row_offset, hipStream_t s);
// k_frames.hip (include/gs_frames.h): the uint8 (h,w,3) form of an f32 frame, and with gt the sum of squared byte differences
// added to *sse.  The launcher trusts what gs_frame_to_u8 checked.
void gs_launch_frame_to_u8(const float* src, int mode, int h, int w, uint8_t* dst, int64_t pitch, const uint8_t* gt, int gt_channels,
                           int64_t gt_pitch, int64_t* sse, hipStream_t s);
void gs_launch_reg_value(const float* feat, const int8_t* invalid, int64_t N, float* workspace, float* out, hipStream_t s);
void gs_launch_reg_grad(const float* feat, const int8_t* invalid, int64_t N, const float* value_and_count, const float* upstream,
                        float* grad, hipStream_t s);

// ---- adaptive density controller (k_density.hip; GaussianPointAdaptiveController.py, CTRL) --------------------------------
// The six accumulator updates of GaussianPointAdaptiveController.update() (CTRL:133-141) for one in-camera point n, in the
// one operation order both k_bwd_points (from its per-splat sums) and k_controller_accumulate (from the hook payload) use,
// so that the two wirings give the same bits.  npix / mag / g: the point's num_affected_pixels, magnitude_grad_viewspace
// and grad_point_in_camera row.
// IN_CAMERA = false: without num_in_camera -- in a gs_backward whose fill blocks count it (k_backward.hip: GsZeroFill).
template <bool IN_CAMERA = true>
__device__ __forceinline__ void gs_controller_add(int64_t n, int32_t npix, float mag, float g0, float g1, float g2,
                                                  int32_t* num_in_camera, int32_t* num_pixels, float* vs_grad, float* vs_grad_avg,
                                                  float* pos_grad, float* pos_grad_norm)
{
    if constexpr (IN_CAMERA) num_in_camera[n] += 1;
    num_pixels[n] += npix;
    vs_grad[n] += mag;
    const float avg = mag / (float)npix;                            // 0/0 -> NaN -> 0 (CTRL:138-139); x/0 -> inf is kept
    vs_grad_avg[n] += (avg != avg) ? 0.0f : avg;
    pos_grad[3 * n] += g0; pos_grad[3 * n + 1] += g1; pos_grad[3 * n + 2] += g2;
    pos_grad_norm[n] += sqrtf(g0 * g0 + g1 * g1 + g2 * g2);
}

#include "../../include/gs_rasterizer.h"
// select (CTRL:170-265), apply (CTRL:290-353) and the hook-side accumulation (CTRL:133-141); argument checks are gs_api_calls.hip's
void gs_launch_density_select(const gs_scene& scene, const gs_controller_accumulators& acc, const int32_t* ids, const int32_t* npix,
                              const float* depth, const float* mag, int64_t M, int remove_floaters, const gs_density_config& cfg,
                              const gs_density_plan& plan, hipStream_t s);
void gs_launch_density_apply(const gs_density_scene& scene, const gs_density_config& cfg, const gs_density_plan& plan, uint64_t seed,
                             uint32_t call_index, hipStream_t s);
void gs_launch_controller_accumulate(const int32_t* ids, const int32_t* npix, const float* mag, const float* gpc, int64_t M, int64_t N,
                                     const gs_controller_accumulators& acc, hipStream_t s);
size_t gs_density_scratch_size(int64_t N);

// k_mcmc.hip (include/gs_mcmc.h): fixed-budget densification.  The launchers trust what the entry points checked.  ws of the
// regulariser: gs_mcmc_reg_ws_size(N) bytes of the context's; moments: exp_avg, exp_avg_sq of the features, then of the positions.
struct gs_mcmc_config;
struct gs_mcmc_plan;
void gs_launch_mcmc_noise(float* pc, const float* feat, const int8_t* mask, int64_t N, float noise_scale, float gate_k, float gate_x0,
                          uint64_t seed, uint32_t step_index, hipStream_t s);
void gs_launch_mcmc_regulariser(const float* feat, const int8_t* mask, int64_t N, float lambda_opacity, float lambda_scale,
                                const float* upstream, float* grad, float* value_and_count, void* ws, hipStream_t s);
void gs_launch_mcmc_relocate(const gs_density_scene& scene, float* const moments[4], const gs_mcmc_config& cfg, const gs_mcmc_plan& plan,
                             uint64_t seed, uint32_t call_index, hipStream_t s);
size_t gs_mcmc_scratch_size(int64_t N);
size_t gs_mcmc_reg_ws_size(int64_t N);

// k_vq.hip (include/gs_vq.h): nearest centroid per row and weighted mean per centroid.  The launchers trust what the entry
// points checked.  scratch of the assignment: gs_vq_scratch_size() bytes of the caller's.
void gs_launch_vq_assign(const float* x, int64_t ldx, int64_t N, int dim, const float* cb, int64_t ldc, int K, int32_t* labels, float* dist,
                         void* scratch, hipStream_t s);
void gs_launch_vq_update(const float* x, int64_t ldx, int64_t N, int dim, const float* weights, const int32_t* labels, float* cb, int64_t ldc,
                         int K, int32_t* counts, double* weight_sums, hipStream_t s);
size_t gs_vq_scratch_size(int64_t n_rows, int n_codes, int dim);

// k_appearance.hip (include/gs_appearance.h): the affine colour transform of an image.  The launchers trust what the entry
// points checked.  ws: gs_appearance_ws_size(H, W) bytes of the context's, 8-byte aligned (the per-block sums).  GI.p NULL:
// no image gradient; grad_transform NULL: no sums.
size_t gs_appearance_ws_size(int H, int W);
void gs_launch_appearance_apply(const GsLossImage& X, const float* M, int H, int W, const GsLossImage& C, hipStream_t s);
void gs_launch_appearance_backward(const GsLossImage& X, const GsLossImage& G, const float* M, int H, int W, const GsLossImage& GI,
                                   float* grad_transform, void* ws, hipStream_t s);
void gs_launch_appearance_moments(const GsLossImage& X, const GsLossImage& Y, const float* weight, int H, int W, double* moments, void* ws,
                                  hipStream_t s);
// k_posetable.hip (include/gs_pose_table.h): a view's six floats composed onto its K base poses, and the way back.  The
// launchers trust what the entry points checked; V, K > 0.
void gs_launch_pose_compose(const float* delta, const float* q_base, const float* t_base, int V, int K, float* q_out, float* t_out, hipStream_t s);
void gs_launch_pose_compose_backward(const float* delta, const float* q_base, const float* grad_q, const float* grad_t, int V, int K, float reg,
                                     float* grad_delta, hipStream_t s);
// k_background.hip (include/gs_background.h): a colour or a spherical-harmonics sky behind an image.  The launchers trust what
// the entry points checked.  ws: gs_background_ws_size(H, W) bytes of the context's (the per-block sums), unused when grad_coef
// is NULL.  X.p NULL: colours only.
size_t gs_background_ws_size(int H, int W);
void gs_launch_background_composite(const GsLossImage& X, const float* alpha, const float* coef, int bands, const float* q, const float* Km,
                                    int H, int W, int flags, const GsLossImage& O, hipStream_t s);
void gs_launch_background_backward(const GsLossImage& G, const float* alpha, const float* coef, int bands, const float* q, const float* Km,
                                   int H, int W, float* grad_alpha, float* grad_coef, void* ws, hipStream_t s);
// k_bilateral.hip (include/gs_bilateral.h): the bilateral grid of colour transforms of an image.  The launchers trust what the
// entry points checked.  ws: gs_bilateral_ws_size(Gx, Gy, L) bytes of the context's (the block sums of a split footprint; 0
// where no footprint is split).  GI.p NULL: no image gradient; grad_grid NULL: no gather.
size_t gs_bilateral_ws_size(int Gx, int Gy, int L);
void gs_launch_bilateral_slice(const GsLossImage& X, const float* grid, int Gx, int Gy, int L, int H, int W, const GsLossImage& C, hipStream_t s);
void gs_launch_bilateral_backward(const GsLossImage& X, const GsLossImage& G, const float* grid, int Gx, int Gy, int L, int H, int W,
                                  const GsLossImage& GI, float* grad_grid, void* ws, hipStream_t s);
void gs_launch_bilateral_tv(const float* grid, int Gx, int Gy, int L, float weight, float* grad_grid, float* value, hipStream_t s);
// k_filter3d.hip (include/gs_filter3d.h): the 3D smoothing filter.  The launchers trust what the entry points checked; n > 0.
// ws: gs_filter3d_ws_size() bytes of the context's (the bits of the smallest seen rate).  grad_in == grad_out: in place.
size_t gs_filter3d_ws_size();
void gs_launch_filter3d_rate(const float* point_cloud, const int8_t* mask, int64_t n, const float* views, int n_views, int W, int H, float near,
                             float margin, float* rate, void* ws, hipStream_t s);
void gs_launch_filter3d_apply(float* features, const float* rate, int64_t n, float k, float* features_out, hipStream_t s);
void gs_launch_filter3d_backward(const float* grad_out, const float* features, const float* rate, int64_t n, float k, float* grad_in,
                                 hipStream_t s);
// k_depth.hip (include/gs_depth.h): the depth target with its weight plane, and the depth loss.  The launchers trust what the
// entry points checked.  ws: gs_depth_ws_size(H, W) bytes of the context's, 8-byte aligned (finished moments, per-block sums).
void gs_launch_depth_resample(const void* src, int src_format, int H_in, int W_in, int64_t pitch_bytes, float depth_scale, GsResampleAxis ax,
                              GsResampleAxis ay, int h_out, int w_out, float min_coverage, float* dst, hipStream_t s);
size_t gs_depth_ws_size(int H, int W);
void gs_launch_depth_loss_forward(const float* D, const float* Z, const float* wt, const float* wp, int H, int W, int flags, float* terms, void* ws,
                                  hipStream_t s);
void gs_launch_depth_loss_backward(const float* D, const float* Z, const float* wt, const float* wp, int H, int W, int flags, const float* terms,
                                   const float* upstream, float* G, hipStream_t s);

// k_geometry.hip (include/gs_geometry.h): the depth-derived normal, the normal loss and the depth smoothness.  The launchers trust
// what the entry points checked.  ws: gs_geometry_ws_size(H, W) bytes of the context's, 8-byte aligned (per-tile sums).
size_t gs_geometry_ws_size(int H, int W);
void gs_launch_depth_normals(const float* D, int H, int W, float fx, float fy, float cx, float cy, float jump, float* normals, hipStream_t s);
void gs_launch_normal_loss_forward(const float* D, const float* N, const float* wn, const float* wp, int H, int W, float fx, float fy, float cx,
                                   float cy, float jump, int flags, float* terms, void* ws, hipStream_t s);
void gs_launch_normal_loss_backward(const float* D, const float* N, const float* wn, const float* wp, int H, int W, float fx, float fy, float cx,
                                    float cy, float jump, int flags, const float* terms, const float* upstream, float* G, hipStream_t s);
void gs_launch_depth_smooth_forward(const float* D, const float* I, const float* wp, int H, int W, float lambda, int flags, float* terms, void* ws,
                                    hipStream_t s);
void gs_launch_depth_smooth_backward(const float* D, const float* I, const float* wp, int H, int W, float lambda, int flags, const float* terms,
                                     const float* upstream, float* G, hipStream_t s);

// k_normals.hip (include/gs_normals.h): the per-Gaussian normals (N >= 1 rows) and the consistency of their render with the depth
// normal.  ws: gs_geometry_ws_size(H, W) bytes, as above.
void gs_launch_gaussian_normals_forward(const float* pc, const float* feat, const int32_t* obj, const float* q_pc, const float* t_pc, int64_t N,
                                        int K, float* normals, hipStream_t s);
void gs_launch_gaussian_normals_backward(const float* pc, const float* feat, const int32_t* obj, const float* q_pc, const float* t_pc, int64_t N,
                                         int K, const float* grad_normals, float* grad_feat, hipStream_t s);
void gs_launch_normal_consistency_forward(const float* D, const float* R, const float* wp, int H, int W, float fx, float fy, float cx, float cy,
                                          float jump, float min_length, float* terms, void* ws, hipStream_t s);
void gs_launch_normal_consistency_backward(const float* D, const float* R, const float* wp, int H, int W, float fx, float fy, float cx, float cy,
                                           float jump, float min_length, const float* terms, const float* upstream, float* G, float* GR,
                                           hipStream_t s);

// k_fusion.hip (include/gs_fusion.h): depth frames into a TSDF volume (n_views cut into launches of GS_TSDF_VIEWS_PER_LAUNCH, in
// order), and the two halves of the isosurface around the caller's read of the totals.  The launchers trust what the entry
// points checked: a non-empty volume, non-NULL arrays and work buffers, counts below 2^31.
struct gs_tsdf_volume;
struct gs_tsdf_view;
struct gs_iso_volume;
void gs_launch_tsdf_integrate(const gs_tsdf_volume& vol, const gs_tsdf_view* views, int n_views, hipStream_t s);
void gs_launch_iso_plan(const gs_iso_volume& vol, void* cell_ws, void* block_ws, int64_t* totals, hipStream_t s);
void gs_launch_iso_emit(const gs_iso_volume& vol, const void* cell_ws, const void* block_ws, void* voxel_ws, int64_t n_vertices,
                        int64_t n_faces, float* vertices, float* colours, int32_t* faces, hipStream_t s);
