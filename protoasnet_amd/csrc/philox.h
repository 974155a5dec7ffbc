// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants), usable on
// the host and on the device: a counter-based generator, so draw d of replicate b is a function of (seed, b, d) and of nothing else.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PASN_HD __host__ __device__ __forceinline__
#else
#define PASN_HD inline
#endif

namespace pasn {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

PASN_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

// the resampling unit of draw word r among G: multiply-shift (bias <= G / 2^32)
PASN_HD uint32_t philox_unit(uint32_t r, uint32_t G) { return (uint32_t)(((uint64_t)r * G) >> 32); }

}  // namespace pasn
