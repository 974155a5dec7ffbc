// block_reduce.h -- the fixed-order block reduce behind every two-stage sum of the training path (train.hip's row passes, the depthwise
// weight-gradient kernels of dw_wgrad.hip) and behind every block sum of the evaluation kernels (eval_metrics, selective, bootstrap,
// calibration).  DESIGN.md promises bitwise reproducible gradients and statistics; the summation order of the loops below keeps that
// promise, which is why there is ONE copy of it.
#pragma once
#include <hip/hip_runtime.h>

namespace pasn {

// lanes per position of a 256-thread block: the channel groups padded to a power of two, so that they divide the block
static inline int pow2_at_least(int v) {
    int b = 1;
    while (b < v) b <<= 1;
    return b;
}

// A 256-thread block = PL position lanes x LPR lanes per position; lane g < CG of a position owns channels g CH .. g CH + CH - 1 and holds
// W partial rows of them, get(p, j) = channel j of row p.  Row p < nlive of the block's sum goes to out[p * Cp + g * CH + j]: the position
// lanes q = 0 .. PL - 1 added in ascending order, one row after the other through red[256 * CH].  PADDED = false: the caller's LPR is CG
// (no lane g >= CG exists), and the guard is compiled out.
template <int W, int CH, bool PADDED, typename Get>
__device__ __forceinline__ void block_reduce_rows(Get get, float* red, float* out, int Cp, int CG, int LPR, int PL, int nlive = W) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int p = 0; p < W; ++p) {
        if (p < nlive) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < CH; ++j) red[tid * CH + j] = get(p, j);
            __syncthreads();
            for (int t = tid; t < LPR * CH; t += 256) {
                const int g = t / CH, j = t % CH;
                if (!PADDED || g < CG) {
                    float s = 0.0f;
                    for (int q = 0; q < PL; ++q) s += red[(q * LPR + g) * CH + j];
                    out[(size_t)p * Cp + g * CH + j] = s;
                }
            }
        }
    }
}
// the same for accumulators held as float[W][CH] with all 256 threads in use (PL = 256 / LPR)
template <int W, int CH>
__device__ __forceinline__ void block_reduce_rows(const float (&acc)[W][CH], float* red, float* out, int Cp, int CG, int LPR, int nlive = W) {
    block_reduce_rows<W, CH, true>([&](int p, int j) { return acc[p][j]; }, red, out, Cp, CG, LPR, 256 / LPR, nlive);
}

// The sum of one fp64 value per thread of a 256-thread block, the same in every thread and in every run: a butterfly within each wave
// (a + b == b + a, so every lane holds the same bits), then the four waves as (0 + 1) + (2 + 3) through red[4].  Two barriers: the first
// frees red from whoever read it before, the second publishes it -- LDS traffic issued before the call is complete after it.
__device__ __forceinline__ double block_sum_fixed(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// its int64 twin, with the same two barriers (integers: any order gives the same sum)
__device__ __forceinline__ long long block_sum_i64(long long v, long long* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

}  // namespace pasn
