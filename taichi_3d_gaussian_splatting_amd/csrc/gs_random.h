// gs_random.h -- the counter-based random numbers the density controller (k_density.hip) and the fixed-budget strategy
// (k_mcmc.hip) draw from, each piece stated once: a draw is a pure function of its counter and key, so a result never depends
// on the launch shape.  The third counter word names the stream: 0 / 1 the two split samples of gs_density_apply, 2 the
// position noise of gs_mcmc_noise, 3 the source draw of gs_mcmc_relocate.
#pragma once
#include "gs_common.h"

// ---- Philox4x32-10 (Salmon et al., SC'11; constants of Random123) -----------------------------------------------
__device__ __forceinline__ uint4 gs_philox4x32_10(uint4 c, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    }
    return c;
}

// 24 random bits -> (0, 1]: log never sees 0
__device__ __forceinline__ float gs_unit(uint32_t x) { return (float)((x >> 8) + 1u) * 5.9604644775390625e-8f; }

// three standard normals from the four words of one draw: Box-Muller (GP3D:91-94), z = (r1 cos, r1 sin, r3 cos)
__device__ __forceinline__ void gs_normal3(const uint4 u, float z[3])
{
    const float u1 = gs_unit(u.x), u2 = gs_unit(u.y), u3 = gs_unit(u.z), u4 = gs_unit(u.w);
    const float two_pi = (float)(2.0 * 3.141592653589);                 // the reference's constant
    const float r1 = sqrtf(-2.0f * logf(u1)), r3 = sqrtf(-2.0f * logf(u3));
    z[0] = r1 * cosf(two_pi * u2);
    z[1] = r1 * sinf(two_pi * u2);
    z[2] = r3 * cosf(two_pi * u4);
}
