// eval_common.h -- what the evaluation kernels (eval_metrics.hip, selective.hip, bootstrap.hip, calibration.hip) share beyond the block
// sums of block_reduce.h and the rank pass of order_key.h: the limits, the fp32 softmax sequence, the first-largest rule, the confusion
// counts -> metrics arithmetic, the packed wave scan and the workspace cursor.  Several of them carry a bitwise promise (DESIGN.md,
// "Evaluation metrics"): two kernels that must agree call the SAME function, which is why there is one copy of each.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_reduce.h"
#include "order_key.h"

namespace pasn {

constexpr int EVAL_MAX_K = 16;           // real classes
constexpr long EVAL_MAX_ROWS = 1L << 20;  // of a rank by counting, a bootstrap or a reliability table
constexpr int EVAL_MAX_REPLICATES = 65536;

// The (label, prediction) of a row, four bits each, inside a workspace word: the label at bit `lbit`, the prediction at bit `pbit`.
struct ClassCell {
    int lbit, pbit;
    __device__ __forceinline__ int pack(int L, int P) const { return (L << lbit) | (P << pbit); }
    __device__ __forceinline__ int label(int c) const { return (c >> lbit) & (EVAL_MAX_K - 1); }
    __device__ __forceinline__ int pred(int c) const { return (c >> pbit) & (EVAL_MAX_K - 1); }
};

// The softmax of lg[0 .. n) in fp32 is __fdiv_rn(expf(lg[k] - *m), s) with the s returned here: the largest logit through an fmaxf chain,
// the sum in column order.  The stored probs of eval_batch_stats_kernel and the uncertainty scores are bitwise equal through it.
__device__ __forceinline__ float softmax_max_sum_f32(const float* lg, int n, float* m) {
    float mx = lg[0];
    for (int k = 1; k < n; ++k) mx = fmaxf(mx, lg[k]);
    float s = 0.0f;
    for (int k = 0; k < n; ++k) s += expf(lg[k] - mx);
    *m = mx;
    return s;
}

// The predicted class of a row: the FIRST largest of p[0 .. K) (strict >, from column 0; a row of NaNs gives 0).  *best: that entry.
__device__ __forceinline__ int first_largest(const float* p, int K, float* best) {
    int pred = 0;
    float b = p[0];
    for (int k = 1; k < K; ++k)
        if (p[k] > b) {
            b = p[k];
            pred = k;
        }
    *best = b;
    return pred;
}

// Confusion counts -> accuracy, balanced accuracy, mean F1 (confusion_to_metrics of trainer.py): add() once per class in class order, then
// the three readings.  fp64, every operation rounded on its own.
struct ClassTally {
    long long trace = 0;
    int present = 0;
    double rsum = 0.0, fsum = 0.0;
    __device__ __forceinline__ void add(long long tp, long long sup, long long prd) {
#pragma clang fp contract(off)
        trace += tp;
        if (sup > 0) {
            rsum += (double)tp / (double)sup;
            ++present;
        }
        if (sup + prd > 0) fsum += 2.0 * (double)tp / (double)(sup + prd);
    }
    __device__ __forceinline__ double accuracy(long long W) const { return W > 0 ? (double)trace / (double)W : 0.0; }
    __device__ __forceinline__ double balanced_accuracy() const { return present > 0 ? rsum / (double)present : 0.0; }
    __device__ __forceinline__ double f1_mean(int K) const { return fsum / (double)K; }
};

// inclusive scan over the wave (T: uint32_t counts, or a packed 64-bit word)
template <typename T>
__device__ __forceinline__ T wave_scan_incl(T inc) {
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) {
        const T v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    return inc;
}

// A cursor over a workspace: take() hands out the next n elements (the offset rounded up to `align` first).  On a null base nothing is
// addressed and `used` ends as the bytes the layout needs.
struct Carve {
    char* base;
    size_t used = 0;
    template <typename T>
    T* take(size_t n, size_t align = alignof(T)) {
        used = (used + align - 1) / align * align;
        T* r = reinterpret_cast<T*>(base + used);
        used += n * sizeof(T);
        return r;
    }
};

}  // namespace pasn
