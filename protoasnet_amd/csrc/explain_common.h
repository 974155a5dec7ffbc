// explain_common.h -- what the explanation kernels (explain.hip, perturb.hip, corrupt.hip) share: the prediction rule, the rank of a
// prototype inside its class block, the add of a batch onto a sweep's accumulators, and the raw-element helpers of the 16-byte store
// passes.  "The predicted class" and "the k best prototypes" are reported by pasn_explain_rank (and through it by the faithfulness
// curves) and by pasn_stability_stats: both call the SAME function here, which is why there is one copy of each ("Explanation
// kernels: one selection rule").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pasn {

// The predicted class (torch.argmax): the first maximum of l[0 .. K_real), NaN counts as the largest value.
__device__ __forceinline__ int explain_pred(const float* l, int K_real) {
    int best = 0;
    float bv = l[0];
    for (int c = 1; c < K_real; ++c) {
        const float v = l[c];
        if (!(bv != bv) && (v > bv || v != v)) {
            bv = v;
            best = c;
        }
    }
    return best;
}

// The rank of prototype p inside its class block [base, base + G): the number of members that beat it, by similarity descending and the
// HIGHER index first on ties (reversing a stable ascending argsort).  A NaN beats nothing and is beaten by nothing.  `sim` may point into
// LDS or global memory: the caller's address space survives the inlining.
__device__ __forceinline__ int explain_block_rank(const float* sim, int base, int G, int p) {
    const float v = sim[p];
    int r = 0;
    for (int q = base; q < base + G; ++q) {
        const float o = sim[q];
        r += (o > v || (o == v && q > p)) ? 1 : 0;
    }
    return r;
}

// acc[e] += sum over the clips of term(n, e), n ascending, one thread of the block of NT per entry; the last entry += N.  The order is
// part of the contract: the accumulators of two runs are compared bitwise.
template <int NT, typename F>
__device__ __forceinline__ void sweep_acc_add(double* acc, int total, int N, F term) {
    for (int e = threadIdx.x; e < total; e += NT) {
        double t = acc[e];
        if (e == total - 1) {
            t += (double)N;
        } else {
            for (long n = 0; n < N; ++n) t += term(n, e);
        }
        acc[e] = t;
    }
}

// ---- raw elements: a clip's element as its bits (uint32_t: fp32, uint16_t: bf16) ------------------------------------------------------
// fp32 bits -> bf16 bits, to nearest even.  No NaN case: a caller that can meet one handles it first.
__host__ __device__ __forceinline__ uint32_t bf16_round_bits(uint32_t u) { return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16; }

__device__ __forceinline__ float raw_widen(uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ float raw_widen(uint16_t u) { return __uint_as_float((uint32_t)u << 16); }
// one rounding to the dtype
template <typename U>
__device__ __forceinline__ U raw_narrow(float f) {
    const uint32_t u = __float_as_uint(f);
    if constexpr (sizeof(U) == 4) return u;
    else return (U)bf16_round_bits(u);
}

// elements from p up to the next 16-byte boundary (0 when p lies on one)
template <typename U>
__device__ __forceinline__ int lead_to_16(const U* p) {
    return (int)(((16 - ((uintptr_t)p & 15)) & 15) / sizeof(U));
}

}  // namespace pasn
