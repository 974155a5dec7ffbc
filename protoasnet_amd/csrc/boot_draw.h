// boot_draw.h -- the grouped-bootstrap draws inside a block: the ONE copy bootstrap.hip and ordinal.hip share, so that replicate b of either
// is the same multiset of rows.  Draw d of replicate b is output word d & 3 of Philox4x32-10 at counter (d >> 2, b, 0, 0); the unit is
// (r * G) >> 32 (include/protoasnet_amd.h, "Draws").  G <= BOOT_LDS_MAX_G: uint16 pairs in LDS (integer LDS atomics); above, an int32
// slice of global memory that the block owns (global integer atomics).
#pragma once
#include <algorithm>

#include "common.h"
#include "philox.h"

namespace pasn {

constexpr int BOOT_LDS_MAX_G = PASN_BOOTSTRAP_LDS_MAX_G;  // uint16 counts: 32 KiB of LDS, four blocks per CU
constexpr int BOOT_NT = 256;
constexpr size_t BOOT_SLOT_BYTES = 256ull << 20;  // the count slices of the global path together
constexpr int BOOT_MAX_SLOTS = 512;

// counts of replicate b as uint16 pairs in s_cnt[(G + 1) / 2]; ones: the point estimate.  Ends with a barrier.
__device__ __forceinline__ void boot_draw_lds(uint32_t* s_cnt, int G, uint32_t b, uint32_t k0, uint32_t k1, bool ones) {
    const int tid = threadIdx.x;
    for (int w = tid; w < (G + 1) / 2; w += BOOT_NT) s_cnt[w] = ones ? 0x00010001u : 0u;
    __syncthreads();
    if (!ones)
        for (int q = tid; q < (G + 3) / 4; q += BOOT_NT) {
            uint32_t r[4];
            philox4x32_10((uint32_t)q, b, 0u, 0u, k0, k1, r);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * q + j < G) {
                    const uint32_t g = philox_unit(r[j], (uint32_t)G);  // a count never exceeds G < 2^16: no carry into the neighbour
                    atomicAdd(&s_cnt[g >> 1], 1u << (16 * (g & 1)));
                }
        }
    __syncthreads();
}

__device__ __forceinline__ uint32_t boot_count_lds(const uint32_t* s_cnt, uint32_t g) { return (s_cnt[g >> 1] >> (16 * (g & 1))) & 0xFFFFu; }

// the same into an int32 slice of global memory that this block owns.  The adds happen in L2; boot_count_global reads there too.
__device__ __forceinline__ void boot_draw_global(int32_t* cg, long G, uint32_t b, uint32_t k0, uint32_t k1, bool ones) {
    const int tid = threadIdx.x;
    for (long g = tid; g < G; g += BOOT_NT) cg[g] = ones ? 1 : 0;
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stores have reached L2 before another wave's atomic finds the word
    __syncthreads();
    if (!ones)
        for (long q = tid; q < (G + 3) / 4; q += BOOT_NT) {
            uint32_t r[4];
            philox4x32_10((uint32_t)q, b, 0u, 0u, k0, k1, r);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * q + j < G) atomicAdd(&cg[philox_unit(r[j], (uint32_t)G)], 1);
        }
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

__device__ __forceinline__ uint32_t boot_count_global(const int32_t* cg, uint32_t g) {
    return (uint32_t)__hip_atomic_load(cg + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// blocks of the global path (each owns a slice of G counts and loops over the replicates); 0: the counts fit LDS
static inline int boot_slots(long G, int B) {
    if (G <= BOOT_LDS_MAX_G) return 0;
    const long fit = std::max(1L, (long)(BOOT_SLOT_BYTES / ((size_t)G * sizeof(int32_t))));
    return (int)std::min({(long)B + 1, (long)BOOT_MAX_SLOTS, fit});
}

}  // namespace pasn
