// k_pose.hip -- gradient with respect to the object poses (q_pointcloud_camera, t_pointcloud_camera), from the per-splat sums
// loop 1 leaves (k_backward.hip: k_sum_rows).  The reference reserves the two slots and returns None in them (RAST:1158-1163);
// here the pose gradient is the derivative of the forward as k_project computes it, including the J(p) and view-direction paths
// that the point gradient leaves out (DESIGN.md "Pose gradient").  Two kernels, no float atomics, bitwise reproducible:
//   k_pose_points  one thread per in-camera entry m: 15 floats per touched point -- dL/dW (9), dL/dt_cp (3), dL/do (3) -- summed
//                  per object in fixed order: over the lanes of a wave (butterfly), then over the block's four waves in wave
//                  order, and stored as (object, 15 floats) records, at most min(n_objects, 256) per block;
//   k_pose_reduce  one workgroup per object: every block's record of that object in block order, the workgroup's sum in fixed
//                  order, then the object's chain to dL/dq (4) and dL/dt (3) (gs_pose_grad_chain).  No touched point: exact zeros.
// The forward's expressions come from where k_project takes them (gs_point_math.h: feature row, Sigma, J, gs_sh16_grad_dir beside
// gs_sh16), the sums' columns from GsRow, the wave sum from gs_common.h (gs_wave_sum_f).
#include "gs_point_math.h"

#define POSE_G 15          // floats of a point's contribution
#define POSE_REC 16        // object id (int bits) + POSE_G
#define POSE_BLOCK 256
#define POSE_REDUCE_THREADS 1024

static inline int pose_block_cap(int n_objects) { return n_objects < POSE_BLOCK ? n_objects : POSE_BLOCK; }

// AUX: the sums carry d depth in column 11 (gs_backward_ex): it joins dL/dp_cam z
template <bool AUX>
__global__ __launch_bounds__(POSE_BLOCK) void k_pose_points(int M, int n_objects, int cap,
    const int32_t* __restrict__ ids, const float4* __restrict__ sums,
    const float4* __restrict__ PB, const float4* __restrict__ PC, const float4* __restrict__ PD,
    const float* __restrict__ pc, const float* __restrict__ feat, const int32_t* __restrict__ obj,
    const float* __restrict__ Kmat, const GsPose* __restrict__ pose,
    float* __restrict__ rec, int32_t* __restrict__ n_rec)
{
    __shared__ float sWave[4][64][POSE_REC];
    __shared__ float sBlock[POSE_BLOCK][POSE_REC];
    __shared__ int sWaveN[4];
    __shared__ int sBlockN;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m = blockIdx.x * POSE_BLOCK + threadIdx.x;
    float g[POSE_G];
#pragma unroll
    for (int k = 0; k < POSE_G; ++k) g[k] = 0.0f;
    int o = -1;
    const float4 r2 = m < M ? sums[3 * (size_t)m + 2] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int n = m < M ? ids[m] : 0;
    const int oid = m < M ? obj[n] : -1;
    // touched points only, as k_bwd_points (an untouched point's sums are all zero)
    if (m < M && gs_row_count(r2) != 0 && oid >= 0 && oid < n_objects) {
        o = oid;
        const GsRow s = gs_row(sums[3 * (size_t)m], sums[3 * (size_t)m + 1], r2);
        // the per-splat factors k_blend_bwd_tile left out: opacity, 0.5 opacity (k_bwd_points)
        const float apt = GS_REC(PB, m).z;
        const float a0 = s.vs0 * apt, a1 = s.vs1 * apt;
        const float hf = 0.5f * apt;
        const float G00 = s.cov00 * hf, G01 = s.cov01 * hf, G11 = s.cov11 * hf;
        const GsPose& P = pose[o];
        float Km[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Km[k] = Kmat[k];
        const float x = pc[3 * (size_t)n], y = pc[3 * (size_t)n + 1], z = pc[3 * (size_t)n + 2];
        const float4 pd = GS_REC(PD, m);                                  // p = W x + t_cp, as the forward computed it
        const float px = pd.x, py = pd.y, pz = pd.z, pz2 = pz * pz;
        // ---- uv = (K p)_01 / p_z ----
        const float d[6] = { Km[0] / pz, Km[1] / pz, (-Km[0] * px - Km[1] * py) / pz2,
                             Km[3] / pz, Km[4] / pz, (-Km[3] * px - Km[4] * py) / pz2 };
        float gp[3] = { a0 * d[0] + a1 * d[3], a0 * d[1] + a1 * d[4], a0 * d[2] + a1 * d[5] };
        // ---- Sigma' = J W Sigma W^T J^T: H = G J W Sigma; dL/dW += 2 J^T H; dL/dJ = 2 G J V = 2 H W^T ----
        const float4* row4 = reinterpret_cast<const float4*>(feat + (size_t)GS_NFEAT * n);
        float row[GS_NFEAT];
        gs_load_feat_row(row4, row);
        const float fx = Km[0], fy = Km[4];
        float J[6], Sigma[9];
        gs_projection_jacobian(fx, fy, px, py, pz, J);
        gs_sigma_from_row(row, Sigma);
        float JW[6], JWS[6], H[6];
        gs_mm<2, 3, 3>(J, P.R, JW);
        gs_mm<2, 3, 3>(JW, Sigma, JWS);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            H[j] = G00 * JWS[j] + G01 * JWS[3 + j];
            H[3 + j] = G01 * JWS[j] + G11 * JWS[3 + j];
        }
        float B[6];                                                       // dL/dJ
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int i = 0; i < 3; ++i)
                B[3 * r + i] = 2.0f * ((H[3 * r] * P.R[3 * i] + H[3 * r + 1] * P.R[3 * i + 1]) + H[3 * r + 2] * P.R[3 * i + 2]);
        // J(p): dJ00/dpz = -fx/pz^2, dJ02/dpx = -fx/pz^2, dJ02/dpz = 2 fx px/pz^3, and the same for row 1 with fy, py
        const float fx2 = fx / pz2, fy2 = fy / pz2;
        gp[0] += B[2] * -fx2;
        gp[1] += B[5] * -fy2;
        gp[2] += (B[0] * -fx2 + B[2] * (2.0f * fx2 * px / pz)) + (B[4] * -fy2 + B[5] * (2.0f * fy2 * py / pz));
        if constexpr (AUX) gp[2] += s.depth;                                 // the splat's depth is p_z
        // ---- p = W x + t_cp ----
        const float xv[3] = { x, y, z };
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) g[3 * i + j] = gp[i] * xv[j] + 2.0f * (J[i] * H[j] + J[3 + i] * H[3 + j]);
        g[9] = gp[0]; g[10] = gp[1]; g[11] = gp[2];
        // ---- colour = sigmoid(sum_k f_k Y_k(d / |d|)), d = x - o ----
        const float dx = x - P.origin_fwd[0], dy = y - P.origin_fwd[1], dz = z - P.origin_fwd[2];
        const float dn = sqrtf(dx * dx + dy * dy + dz * dz);
        const float ux = dx / dn, uy = dy / dn, uz = dz / dn;
        const float4 col = GS_REC(PC, m);                                  // the forward's sigmoid values
        const float ga[3] = { s.col[0] * (col.x * (1.0f - col.x)), s.col[1] * (col.y * (1.0f - col.y)), s.col[2] * (col.z * (1.0f - col.z)) };
        float gY[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) gY[k] = (ga[0] * row[8 + k] + ga[1] * row[24 + k]) + ga[2] * row[40 + k];
        float gu[3];
        gs_sh16_grad_dir(ux, uy, uz, gY, gu);
        const float ug = ux * gu[0] + uy * gu[1] + uz * gu[2];
        g[12] = -(gu[0] - ux * ug) / dn;                                   // dL/do = -dL/dd
        g[13] = -(gu[1] - uy * ug) / dn;
        g[14] = -(gu[2] - uz * ug) / dn;
    }
    // ---- per object: the wave's lanes (butterfly, the same order for every object), then the block's waves in order ----
    unsigned long long live = gs_ballot(o >= 0);
    int k = 0;
    while (live) {
        const int cur = __builtin_amdgcn_readlane(o, __builtin_ctzll(live));
        const bool mine = o == cur;
        float v[POSE_G];
#pragma unroll
        for (int j = 0; j < POSE_G; ++j) v[j] = gs_wave_sum_f(mine ? g[j] : 0.0f);
        if (lane == 0) {
            sWave[wave][k][0] = __int_as_float(cur);
#pragma unroll
            for (int j = 0; j < POSE_G; ++j) sWave[wave][k][1 + j] = v[j];
        }
        live &= ~gs_ballot(mine);
        ++k;
    }
    if (lane == 0) sWaveN[wave] = k;
    __syncthreads();
    if (threadIdx.x == 0) {
        int nb = 0;
        for (int w = 0; w < 4; ++w)
            for (int r = 0; r < sWaveN[w]; ++r) {
                const int id = __float_as_int(sWave[w][r][0]);
                int b = 0;
                while (b < nb && __float_as_int(sBlock[b][0]) != id) ++b;
                if (b == nb) {
                    if (nb == cap) continue;           // cannot happen: a block holds at most min(n_objects, 256) distinct ids
                    for (int j = 0; j < POSE_REC; ++j) sBlock[b][j] = sWave[w][r][j];
                    ++nb;
                } else {
                    for (int j = 1; j < POSE_REC; ++j) sBlock[b][j] += sWave[w][r][j];
                }
            }
        sBlockN = nb;
        n_rec[blockIdx.x] = nb;
    }
    __syncthreads();
    const int nb = sBlockN;
    float* dst = rec + (size_t)blockIdx.x * cap * POSE_REC;
    for (int e = threadIdx.x; e < nb * POSE_REC; e += POSE_BLOCK) dst[e] = (&sBlock[0][0])[e];
}

__global__ __launch_bounds__(POSE_REDUCE_THREADS) void k_pose_reduce(int n_blocks, int cap, const float* __restrict__ rec,
                                                                     const int32_t* __restrict__ n_rec, const GsPose* __restrict__ pose,
                                                                     float* __restrict__ grad_q, float* __restrict__ grad_t)
{
    __shared__ float sW[POSE_REDUCE_THREADS / 64][POSE_REC];
    const int o = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float acc[POSE_G];
#pragma unroll
    for (int j = 0; j < POSE_G; ++j) acc[j] = 0.0f;
    int hits = 0;
    for (int b = threadIdx.x; b < n_blocks; b += POSE_REDUCE_THREADS) {
        const int nr = n_rec[b];
        const float4* r = reinterpret_cast<const float4*>(rec + (size_t)b * cap * POSE_REC);
        for (int k = 0; k < nr; ++k, r += POSE_REC / 4) {
            const float4 r0 = r[0];
            if (__float_as_int(r0.x) != o) continue;
            const float4 r1 = r[1], r2 = r[2], r3 = r[3];
            acc[0] += r0.y; acc[1] += r0.z; acc[2] += r0.w;
            acc[3] += r1.x; acc[4] += r1.y; acc[5] += r1.z; acc[6] += r1.w;
            acc[7] += r2.x; acc[8] += r2.y; acc[9] += r2.z; acc[10] += r2.w;
            acc[11] += r3.x; acc[12] += r3.y; acc[13] += r3.z; acc[14] += r3.w;
            ++hits;
            break;                                     // an object has at most one record per block
        }
    }
#pragma unroll
    for (int j = 0; j < POSE_G; ++j) acc[j] = gs_wave_sum_f(acc[j]);
    hits = gs_wave_sum_i(hits);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < POSE_G; ++j) sW[wave][j] = acc[j];
        sW[wave][POSE_G] = __int_as_float(hits);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float g[POSE_G];
        int total = 0;
#pragma unroll
        for (int j = 0; j < POSE_G; ++j) g[j] = sW[0][j];
        total += __float_as_int(sW[0][POSE_G]);
        for (int w = 1; w < POSE_REDUCE_THREADS / 64; ++w) {
#pragma unroll
            for (int j = 0; j < POSE_G; ++j) g[j] += sW[w][j];
            total += __float_as_int(sW[w][POSE_G]);
        }
        float gq[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, gt[3] = { 0.0f, 0.0f, 0.0f };
        if (total > 0) gs_pose_grad_chain(pose[o], g, gq, gt);      // a pose no touched point depends on: exact zeros
        grad_q[4 * o] = gq[0]; grad_q[4 * o + 1] = gq[1]; grad_q[4 * o + 2] = gq[2]; grad_q[4 * o + 3] = gq[3];
        grad_t[3 * o] = gt[0]; grad_t[3 * o + 1] = gt[1]; grad_t[3 * o + 2] = gt[2];
    }
}

size_t gs_pose_scratch_size(int M, int n_objects)
{
    const size_t nb = (size_t)((M + POSE_BLOCK - 1) / POSE_BLOCK);
    return nb * (size_t)pose_block_cap(n_objects) * POSE_REC * sizeof(float) + nb * sizeof(int32_t) + 16;
}

void gs_launch_pose_grad(const GsBackwardArgs& a, int n_objects, void* scratch, float* grad_q, float* grad_t, hipStream_t s)
{
    if (n_objects <= 0) return;
    const int nb = (a.M + POSE_BLOCK - 1) / POSE_BLOCK;
    const int cap = pose_block_cap(n_objects);
    float* rec = static_cast<float*>(scratch);
    int32_t* n_rec = reinterpret_cast<int32_t*>(rec + (size_t)nb * cap * POSE_REC);
    if (nb > 0 && a.aux)
        k_pose_points<true><<<nb, POSE_BLOCK, 0, s>>>(a.M, n_objects, cap, a.v.ids, a.sums, a.v.PB, a.v.PC, a.v.PD, a.point_cloud, a.features,
                                                      a.object_id, a.Kmat, a.v.pose, rec, n_rec);
    else if (nb > 0)
        k_pose_points<false><<<nb, POSE_BLOCK, 0, s>>>(a.M, n_objects, cap, a.v.ids, a.sums, a.v.PB, a.v.PC, a.v.PD, a.point_cloud, a.features,
                                                       a.object_id, a.Kmat, a.v.pose, rec, n_rec);
    k_pose_reduce<<<n_objects, POSE_REDUCE_THREADS, 0, s>>>(nb, cap, rec, n_rec, a.v.pose, grad_q, grad_t);
}
