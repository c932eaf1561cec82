// philox.h -- the counter-based noise the device-resident samplers share (csrc/ode_sde.hip, csrc/surfel_densify.hip): one block of
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the words -> normal transform
// written out in include/ga_dit.h ("noise of ga_sde_step").  Both includers are built with -ffp-contract=off: every operation of the
// transform is rounded on its own, in the order written.
#ifndef GA_PHILOX_H
#define GA_PHILOX_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace gaphilox {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4])
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// One normal of the Box-Muller pair of the words (wa, wb): the cosine branch (odd = 0) or the sine branch (odd = 1).  24-bit uniforms,
// u1 in (0, 1], u2 in [0, 1).
__device__ __forceinline__ float box_muller(uint32_t wa, uint32_t wb, int odd)
{
    const float u1 = (float)((wa >> 8) + 1u) * 5.9604644775390625e-08f;      // (0, 1], exact in fp32
    const float u2 = (float)(wb >> 8) * 5.9604644775390625e-08f;             // [0, 1)
    const float radius = sqrtf(-2.0f * logf(u1));
    const float theta = 6.283185307179586f * u2;
    return radius * (odd ? sinf(theta) : cosf(theta));
}

}  // namespace gaphilox

#endif  // GA_PHILOX_H
