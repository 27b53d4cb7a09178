// k_density.hip -- adaptive density control of the reference's GaussianPointAdaptiveController (CTRL =
// taichi_3d_gaussian_splatting/GaussianPointAdaptiveController.py, GP3D = .../GaussianPoint3D.py) on the device.
//
//   select (CTRL:170-265, before the optimiser step)
//     k_density_mark      M-pass over the hook arrays: per-frame floater / single-frame marks, one byte store per id
//     k_density_rows      N-pass: floater, transparent (alpha or any NaN feature), multi-frame criteria -> final flags,
//                         per-block counts
//     k_density_scan      one block: exclusive prefix of the per-block densify counts, totals -> counts[]
//     k_density_scatter   N-pass: ascending-id compaction of the densify set + the snapshots CTRL:256-263 keeps
//   apply (CTRL:290-353, after the optimiser step)
//     k_density_prune     N-pass: invalid mask on floaters and transparent rows, per-block valid / free counts
//     k_density_scan      one block: prefix of the free counts, fillable = min(densify, free)
//     k_density_free_rows N-pass: the first `densify` free rows, ascending
//     k_density_fill      one thread per (densify row, fill row) pair: copy, size reduction, foci offset, samples / move
//   k_controller_accumulate   CTRL:133-141 from the hook payload (gs_controller_add, shared with k_bwd_points)
//
// No float atomics, no host waits: the counts the host would learn with .item() (CTRL:220,223,244,301,318) are read
// on the device by the next kernel.  Integer atomics only for the over / under tallies of the fill pass.
#include "gs_point_math.h"
#include "gs_random.h"

#include <algorithm>

#define DEN_BLOCK 256                       // rows per block of every N-pass (one row per thread)
#define DEN_SCAN_THREADS 1024
#define DEN_NBLK(N) (((N) + DEN_BLOCK - 1) / DEN_BLOCK)
// scratch: five int32 arrays of one entry per N-pass block (select: densify, floater, transparent, single, single by
// viewspace; apply reuses the first two for free and valid)
#define DEN_ARRAYS 5

size_t gs_density_scratch_size(int64_t N)
{
    return (size_t)(DEN_ARRAYS * DEN_NBLK(N) + 16) * sizeof(int32_t);
}

// GP3D:391-406 GaussianPoint3D.sample(): centre + R S (z1, z2, z3), z from Box-Muller on the four uniforms of one draw (gs_random.h)
__device__ __forceinline__ void gs_sample_point(const float* centre, const float* feat, uint4 ctr, uint32_t k0, uint32_t k1, float out[3])
{
    float z[3];
    gs_normal3(gs_philox4x32_10(ctr, k0, k1), z);
    float R[3][3];
    rotation_from_quaternion(feat, &R[0][0]);
    const float s[3] = { gs_expf(feat[4]), gs_expf(feat[5]), gs_expf(feat[6]) };
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float v = (R[i][0] * s[0]) * z[0] + (R[i][1] * s[1]) * z[1] + (R[i][2] * s[2]) * z[2];   // (R @ S) @ base
        out[i] = centre[i] + v;
    }
}

// GP3D:376-388 get_ellipsoid_foci_vector(), base-axis choice included as written
__device__ __forceinline__ void gs_foci_vector(const float* feat, float out[3])
{
    const float sx = feat[4], sy = feat[5], sz = feat[6];
    int axis = 0;
    if (sx < sy && sy > sz) axis = 1;
    else if (sx < sz && sy < sz) axis = 2;
    float R[3][3];
    rotation_from_quaternion(feat, &R[0][0]);
    const float ex = gs_expf(sx), ey = gs_expf(sy), ez = gs_expf(sz);
    const float rc = fmaxf(fmaxf(ex, ey), ez), ra = fminf(fminf(ex, ey), ez);
    const float len = sqrtf(rc * rc - ra * ra);
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = len * R[i][axis];
}

// ---- select ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DEN_BLOCK) void k_density_mark(
    const int32_t* __restrict__ ids, const int32_t* __restrict__ npix, const float* __restrict__ depth, const float* __restrict__ mag,
    int64_t M, int64_t N, int remove_floaters, gs_density_config cfg, int8_t* __restrict__ flags)
{
    const int64_t m = (int64_t)blockIdx.x * DEN_BLOCK + threadIdx.x;
    if (m >= M) return;
    const int32_t n = ids[m];
    if (n < 0 || n >= N) return;
    const float g = mag[m];
    const int32_t np = npix[m];
    int bits = 0;
    if (remove_floaters && np > cfg.floater_near_camrea_num_pixels_threshold && depth[m] < cfg.floater_depth_threshold)   // CTRL:192-193
        bits |= GS_DENSITY_CAM_FLOATER;
    const bool by_vs = g > cfg.densification_view_space_position_gradients_threshold;                                    // CTRL:217
    const bool by_avg = g / (float)np > cfg.densification_view_avg_space_position_gradients_threshold;                   // CTRL:221
    if (by_vs) bits |= GS_DENSITY_CAM_VIEWSPACE;
    if (by_vs || by_avg) bits |= GS_DENSITY_CAM_SINGLE;
    flags[n] = (int8_t)bits;                        // ids are unique within a frame: a plain store
}

__global__ __launch_bounds__(DEN_BLOCK) void k_density_rows(
    const float* __restrict__ feat, const int8_t* __restrict__ mask, gs_controller_accumulators acc, int64_t N,
    gs_density_config cfg, int8_t* __restrict__ flags, int32_t* __restrict__ bc)
{
    __shared__ int s_wave[DEN_BLOCK / 64];
    const int64_t n = (int64_t)blockIdx.x * DEN_BLOCK + threadIdx.x;
    bool floater = false, transparent = false, densify = false, single = false, single_vs = false;
    if (n < N) {
        const int marks = flags[n];
        const bool valid = mask[n] == 0;
        floater = (marks & GS_DENSITY_CAM_FLOATER) && valid;                                     // CTRL:196-198
        if (valid && !floater) {                                                                 // CTRL:202-207
            const float* row = feat + (size_t)n * GS_NFEAT;
            bool nan = false;
#pragma unroll 8
            for (int k = 0; k < GS_NFEAT; ++k) nan |= row[k] != row[k];
            transparent = row[7] < cfg.transparent_alpha_threshold || nan;
        }
        // single-frame (CTRL:217-228): the in-camera removal mask is floater_mask_in_camera | transparent
        single = (marks & GS_DENSITY_CAM_SINGLE) && !(marks & GS_DENSITY_CAM_FLOATER) && !transparent;
        single_vs = single && (marks & GS_DENSITY_CAM_VIEWSPACE);
        // multi-frame (CTRL:230-242), torch's true division: both int32 operands to f32, then divide
        const float nic = (float)acc.accumulated_num_in_camera[n];
        float avg_npix = (float)acc.accumulated_num_pixels[n] / nic;                             // CTRL:181-182
        avg_npix = avg_npix != avg_npix ? 0.0f : avg_npix;
        float mf1 = acc.accumulated_view_space_position_gradients[n] / nic;                      // CTRL:230-233
        mf1 = mf1 != mf1 ? 0.0f : mf1;
        float mf2 = acc.accumulated_view_space_position_gradients_avg[n] / nic;                  // CTRL:235-238
        mf2 = mf2 != mf2 ? 0.0f : mf2;
        const float mf3 = acc.accumulated_position_gradients_norm[n] / nic;                      // CTRL:239-240, no NaN fill
        const bool multi = mf1 > cfg.densification_multi_frame_view_space_position_gradients_threshold ||
                           mf2 / avg_npix > cfg.densification_multi_frame_view_pixel_avg_space_position_gradients_threshold ||
                           mf3 > cfg.densification_multi_frame_position_gradients_threshold;
        // CTRL:243, restricted to valid rows: a free row never enters the densify set, so densify rows and the free rows
        // apply fills are disjoint (the reference's own wiring never selects one: hook ids are valid rows and a free row's
        // statistics are zero, which no threshold >= 0 passes)
        densify = valid && (single || multi) && !floater && !transparent;
        const bool over = densify && acc.accumulated_num_pixels[n] > cfg.under_reconstructed_num_pixels_threshold;   // CTRL:253
        flags[n] = (int8_t)((marks & (GS_DENSITY_CAM_FLOATER | GS_DENSITY_CAM_SINGLE | GS_DENSITY_CAM_VIEWSPACE)) |
                            (floater ? GS_DENSITY_FLOATER : 0) | (transparent ? GS_DENSITY_TRANSPARENT : 0) |
                            (densify ? GS_DENSITY_DENSIFY : 0) | (over ? GS_DENSITY_OVER : 0));
    }
    const int nb = gridDim.x;
    const bool preds[DEN_ARRAYS] = { densify, floater, transparent, single, single_vs };
#pragma unroll
    for (int a = 0; a < DEN_ARRAYS; ++a) {
        int total;
        (void)gs_block_rank<DEN_BLOCK / 64>(preds[a], s_wave, &total);
        if (threadIdx.x == 0) bc[a * nb + blockIdx.x] = total;
    }
}

// mode 0 (select): bc[0..nb) densify counts -> exclusive prefix; counts of floaters, transparent, densify, single-frame.
// mode 1 (apply):  bc[0..nb) free counts -> exclusive prefix, bc[nb..2nb) valid-before counts; fillable and the valid totals.
__global__ __launch_bounds__(DEN_SCAN_THREADS) void k_density_scan(int32_t* __restrict__ bc, int nb, int mode, int64_t N,
                                                                   int32_t* __restrict__ counts)
{
    __shared__ int s[DEN_SCAN_THREADS];
    __shared__ int s_tot[DEN_ARRAYS];
    const int t = threadIdx.x;
    const int per = (nb + DEN_SCAN_THREADS - 1) / DEN_SCAN_THREADS;
    const int lo = min(nb, t * per), hi = min(nb, lo + per);
    const int n_sums = mode == 0 ? DEN_ARRAYS : 2;
    for (int a = 0; a < n_sums; ++a) {
        int local = 0;
        for (int i = lo; i < hi; ++i) local += bc[a * nb + i];
        s[t] = local;
        __syncthreads();
        for (int d = 1; d < DEN_SCAN_THREADS; d <<= 1) {          // inclusive Hillis-Steele scan of the per-thread sums
            const int v = t >= d ? s[t - d] : 0;
            __syncthreads();
            s[t] += v;
            __syncthreads();
        }
        if (a == 0) {                                              // exclusive prefix written back in place
            int run = s[t] - local;
            for (int i = lo; i < hi; ++i) { const int c = bc[i]; bc[i] = run; run += c; }
        }
        if (t == 0) s_tot[a] = s[DEN_SCAN_THREADS - 1];
        __syncthreads();
    }
    if (t != 0) return;
    if (mode == 0) {
        counts[GS_DC_DENSIFY] = s_tot[0]; counts[GS_DC_FLOATERS] = s_tot[1]; counts[GS_DC_TRANSPARENT] = s_tot[2];
        counts[GS_DC_SINGLE_FRAME] = s_tot[3]; counts[GS_DC_SINGLE_FRAME_VIEWSPACE] = s_tot[4];
    } else {
        const int n_free = s_tot[0], fill = min(counts[GS_DC_DENSIFY], n_free);
        counts[GS_DC_FILLABLE] = fill;
        counts[GS_DC_OVER] = 0; counts[GS_DC_UNDER] = 0;                           // tallied by k_density_fill
        counts[GS_DC_VALID_BEFORE] = s_tot[1];
        counts[GS_DC_VALID_AFTER] = (int32_t)(N - n_free) + fill;
    }
}

__global__ __launch_bounds__(DEN_BLOCK) void k_density_scatter(
    const int8_t* __restrict__ flags, const float* __restrict__ pc, gs_controller_accumulators acc, int64_t N, float log_phi,
    const int32_t* __restrict__ offsets, int32_t* __restrict__ ids_out, float* __restrict__ pos_out, float* __restrict__ grad_out,
    float* __restrict__ factor_out)
{
    __shared__ int s_wave[DEN_BLOCK / 64];
    const int64_t n = (int64_t)blockIdx.x * DEN_BLOCK + threadIdx.x;
    const int f = n < N ? flags[n] : 0;
    int total;
    const int r = gs_block_rank<DEN_BLOCK / 64>(f & GS_DENSITY_DENSIFY, s_wave, &total);
    if (!(f & GS_DENSITY_DENSIFY)) return;
    const size_t d = (size_t)offsets[blockIdx.x] + r;
    ids_out[d] = (int32_t)n;
    const float nic = (float)acc.accumulated_num_in_camera[n];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        pos_out[3 * d + k] = pc[3 * n + k];                                                  // CTRL:248
        const float g = acc.accumulated_position_gradients[3 * n + k] / nic;                 // CTRL:249-251
        grad_out[3 * d + k] = g != g ? 0.0f : g;
    }
    factor_out[d] = (f & GS_DENSITY_OVER) ? log_phi : 0.0f;                                 // CTRL:252-255
}

// ---- apply ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DEN_BLOCK) void k_density_prune(const int8_t* __restrict__ flags, int8_t* __restrict__ mask, int64_t N,
                                                             int32_t* __restrict__ bc)
{
    __shared__ int s_wave[DEN_BLOCK / 64];
    const int64_t n = (int64_t)blockIdx.x * DEN_BLOCK + threadIdx.x;
    bool valid = false, free_row = false;
    if (n < N) {
        const int8_t m = mask[n];
        valid = m == 0;
        const bool prune = (flags[n] & (GS_DENSITY_FLOATER | GS_DENSITY_TRANSPARENT)) != 0;    // CTRL:294-297 (valid rows only)
        if (prune) mask[n] = 1;
        free_row = prune || m == 1;
    }
    int total;
    (void)gs_block_rank<DEN_BLOCK / 64>(free_row, s_wave, &total);
    if (threadIdx.x == 0) bc[blockIdx.x] = total;
    (void)gs_block_rank<DEN_BLOCK / 64>(valid, s_wave, &total);
    if (threadIdx.x == 0) bc[gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(DEN_BLOCK) void k_density_free_rows(const int8_t* __restrict__ mask, int64_t N, const int32_t* __restrict__ offsets,
                                                                 const int32_t* __restrict__ counts, int32_t* __restrict__ fill_out)
{
    __shared__ int s_wave[DEN_BLOCK / 64];
    const int want = counts[GS_DC_DENSIFY];                        // CTRL:299 torch.where(mask == 1)[0][:num_of_densify_points]
    const int base = offsets[blockIdx.x];
    if (base >= want) return;                                      // block-uniform
    const int64_t n = (int64_t)blockIdx.x * DEN_BLOCK + threadIdx.x;
    const bool free_row = n < N && mask[n] == 1;
    int total;
    const int r = gs_block_rank<DEN_BLOCK / 64>(free_row, s_wave, &total);
    if (free_row && base + r < want) fill_out[base + r] = (int32_t)n;
}

__global__ __launch_bounds__(DEN_BLOCK) void k_density_fill(
    float* __restrict__ pc, float* __restrict__ feat, int8_t* __restrict__ mask, int32_t* __restrict__ obj,
    const int32_t* __restrict__ densify_ids, const int32_t* __restrict__ fill_ids, const float* __restrict__ pos_before,
    const float* __restrict__ grad_pos, const float* __restrict__ factor, int32_t* __restrict__ counts,
    gs_density_config cfg, uint32_t key0, uint32_t key1, uint32_t call_index)
{
    const int n_fill = counts[GS_DC_FILLABLE];
    for (int64_t base = (int64_t)blockIdx.x * DEN_BLOCK; base < n_fill; base += (int64_t)gridDim.x * DEN_BLOCK) {   // wave-uniform
        const int64_t p = base + threadIdx.x;
        const bool live = p < n_fill;
        bool over = false;
        if (live) {
            const int64_t d = densify_ids[p], f = fill_ids[p];
            float* rd = feat + (size_t)d * GS_NFEAT;
            float* rf = feat + (size_t)f * GS_NFEAT;
            for (int k = 0; k < GS_NFEAT; ++k) rf[k] = rd[k];                            // CTRL:309-310
            obj[f] = obj[d];                                                             // CTRL:311-312
            float pf[3], pd[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { pf[k] = pos_before[3 * p + k]; pd[k] = pc[3 * d + k]; }   // CTRL:307-308
            const float red = factor[p];
#pragma unroll
            for (int k = 4; k < 7; ++k) { rf[k] = rf[k] - red; rd[k] = rd[k] - red; }    // CTRL:313-314, 320-321
            over = red > 1e-6f;                                                          // CTRL:315
            if (cfg.enable_ellipsoid_offset) {                                           // CTRL:322-328, from the reduced scale
                float off[3];
                gs_foci_vector(rd, off);
#pragma unroll
                for (int k = 0; k < 3; ++k) { pf[k] = pf[k] + off[k]; pd[k] = pd[k] - off[k]; }
            }
            if (cfg.enable_sample_from_point) {                                          // CTRL:329-344
                if (over) {
                    const float centre[3] = { pd[0], pd[1], pd[2] };                      // both samples around the original's position
                    gs_sample_point(centre, rd, make_uint4((uint32_t)f, call_index, 0u, 0u), key0, key1, pf);
                    gs_sample_point(centre, rd, make_uint4((uint32_t)d, call_index, 1u, 0u), key0, key1, pd);
                } else {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const float step = grad_pos[3 * p + k] * cfg.under_reconstructed_move_factor;   // two roundings, no fma
                        pf[k] = pf[k] + step;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) { pc[3 * f + k] = pf[k]; pc[3 * d + k] = pd[k]; }
            mask[f] = 0;                                                                 // CTRL:345
        }
        const unsigned long long b_over = gs_ballot(live && over), b_under = gs_ballot(live && !over);
        if ((threadIdx.x & 63) == 0 && (b_over | b_under)) {
            atomicAdd(&counts[GS_DC_OVER], (int)__popcll(b_over));
            atomicAdd(&counts[GS_DC_UNDER], (int)__popcll(b_under));
        }
    }
}

// ---- hook-side accumulation -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(DEN_BLOCK) void k_controller_accumulate(
    const int32_t* __restrict__ ids, const int32_t* __restrict__ npix, const float* __restrict__ mag, const float* __restrict__ gpc,
    int64_t M, int64_t N, gs_controller_accumulators acc)
{
    const int64_t m = (int64_t)blockIdx.x * DEN_BLOCK + threadIdx.x;
    if (m >= M) return;
    const int64_t n = ids[m];
    if (n < 0 || n >= N) return;
    gs_controller_add(n, npix[m], mag[m], gpc[3 * m], gpc[3 * m + 1], gpc[3 * m + 2],
                      acc.accumulated_num_in_camera, acc.accumulated_num_pixels, acc.accumulated_view_space_position_gradients,
                      acc.accumulated_view_space_position_gradients_avg, acc.accumulated_position_gradients,
                      acc.accumulated_position_gradients_norm);
}

// ---- launchers ------------------------------------------------------------------------------------------------------
void gs_launch_density_select(const gs_scene& scene, const gs_controller_accumulators& acc, const int32_t* ids, const int32_t* npix,
                              const float* depth, const float* mag, int64_t M, int remove_floaters, const gs_density_config& cfg,
                              const gs_density_plan& plan, hipStream_t s)
{
    const int64_t N = scene.n_points;
    const int nb = (int)DEN_NBLK(N);
    int32_t* bc = reinterpret_cast<int32_t*>(plan.scratch);
    if (N > 0) (void)hipMemsetAsync(plan.flags, 0, (size_t)N, s);
    if (N > 0 && M > 0)
        k_density_mark<<<(unsigned)DEN_NBLK(M), DEN_BLOCK, 0, s>>>(ids, npix, depth, mag, M, N, remove_floaters, cfg, plan.flags);
    if (N > 0)
        k_density_rows<<<nb, DEN_BLOCK, 0, s>>>(scene.point_cloud_features, scene.point_invalid_mask, acc, N, cfg, plan.flags, bc);
    k_density_scan<<<1, DEN_SCAN_THREADS, 0, s>>>(bc, nb, 0, N, plan.counts);
    if (N > 0)
        k_density_scatter<<<nb, DEN_BLOCK, 0, s>>>(plan.flags, scene.point_cloud, acc, N, cfg.log_gaussian_split_factor_phi, bc,
                                                   plan.densify_point_id, plan.densify_point_position_before_optimization,
                                                   plan.densify_point_grad_position, plan.densify_size_reduction_factor);
}

void gs_launch_density_apply(const gs_density_scene& scene, const gs_density_config& cfg, const gs_density_plan& plan, uint64_t seed,
                             uint32_t call_index, hipStream_t s)
{
    const int64_t N = scene.n_points;
    const int nb = (int)DEN_NBLK(N);
    int32_t* bc = reinterpret_cast<int32_t*>(plan.scratch);
    if (N > 0) k_density_prune<<<nb, DEN_BLOCK, 0, s>>>(plan.flags, scene.point_invalid_mask, N, bc);
    k_density_scan<<<1, DEN_SCAN_THREADS, 0, s>>>(bc, nb, 1, N, plan.counts);
    if (N == 0) return;
    k_density_free_rows<<<nb, DEN_BLOCK, 0, s>>>(scene.point_invalid_mask, N, bc, plan.counts, plan.fill_point_id);
    // pairs <= N / 2 (a densify row is valid, a fill row free); the grid walks them, the count is read on the device
    const int grid = std::min(nb, 1024);
    k_density_fill<<<grid, DEN_BLOCK, 0, s>>>(scene.point_cloud, scene.point_cloud_features, scene.point_invalid_mask, scene.point_object_id,
                                              plan.densify_point_id, plan.fill_point_id, plan.densify_point_position_before_optimization,
                                              plan.densify_point_grad_position, plan.densify_size_reduction_factor, plan.counts, cfg,
                                              (uint32_t)seed, (uint32_t)(seed >> 32), call_index);
}

void gs_launch_controller_accumulate(const int32_t* ids, const int32_t* npix, const float* mag, const float* gpc, int64_t M, int64_t N,
                                     const gs_controller_accumulators& acc, hipStream_t s)
{
    if (M <= 0 || N <= 0) return;
    k_controller_accumulate<<<(unsigned)DEN_NBLK(M), DEN_BLOCK, 0, s>>>(ids, npix, mag, gpc, M, N, acc);
}
