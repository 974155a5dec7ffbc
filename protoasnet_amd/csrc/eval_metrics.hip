// eval_metrics.hip -- the evaluation statistics of the reference's epoch loop (Video_XProtoNet_e2e.py:112-173 per batch, :240-319 per
// epoch; XProtoNet_Base.py:499-567) on the device.
//
// pasn_eval_batch_stats: one launch per batch.  Blocks 0 .. N-1 own one row each: the softmax over the real-class logits, the label, the
// SparsityMetric index (src/utils/metrics.py:16-25) and the diversity top-k (Video_XProtoNet_e2e.py:159-171).  A row's sort is a rank
// count out of LDS: the rank of p is the number of q with v[q] > v[p], or v[q] == v[p] and q < p (a stable descending sort), O(P^2 / 256)
// comparisons per thread, no sort network.  The prefix sums run serially in fp64 on one lane -- the order torch's CPU cumsum adds in.
// Blocks N .. hold one thread per prototype column that adds the N rows in order into the fp64 similarity sums (no float atomics: the
// sums are bitwise reproducible).  Integer epoch counters use integer atomics, which do not depend on the order of arrival.
//
// pasn_roc_auc_ovr: the exact Mann-Whitney form of sklearn's roc_auc_score(average="weighted", multi_class="ovr").  Every valid row i is
// the positive of exactly one class (its label L), so one pass over the row pairs counts all classes: thread i compares s_j = p_j[L] of
// every row j with another label against s_i = p_i[L].  Launch 1 tiles the pairs: blockIdx.x = 256 rows i (one per thread), blockIdx.y =
// a chunk of rows j staged through LDS 256 at a time; each block writes its per-class int32 sums to its own workspace slot (no
// atomics, no zeroing), the y = 0 blocks also count the positives, NaN rows and bad labels of their rows i.  Launch 2 (one block) sums the
// slots in int64 and writes the per-class and weighted AUC in fp64.
#include "common.h"
#include "eval_common.h"  // block_sum_fixed / block_sum_i64, rank_geom, softmax_max_sum_f32

namespace pasn {

constexpr int EV_MAX_P = 4096;  // 3 x P floats of LDS per row block
constexpr int AUC_TILE = RANK_TILE;

// rank of element p among x[lo, hi) under a stable descending sort
__device__ __forceinline__ int ev_rank_desc(const float* x, int lo, int hi, int p) {
    const float v = x[p];
    int r = 0;
    for (int q = lo; q < hi; ++q) {
        const float u = x[q];
        r += (u > v) || (u == v && q < p);
    }
    return r;
}

__global__ __launch_bounds__(256) void eval_batch_stats_kernel(const float* __restrict__ logits, const float* __restrict__ sim,
                                                               const int64_t* __restrict__ target, int N, int K, int K_real, int P,
                                                               int P_cls, int kc, int ka, float level, long row_offset,
                                                               float* __restrict__ probs, int32_t* __restrict__ labels,
                                                               float* __restrict__ logits_out, unsigned long long* __restrict__ sparsity,
                                                               unsigned long long* __restrict__ div_counts, double* __restrict__ sim_sums) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= N) {  // column blocks: the similarity sums, rows in order
        const int p = ((int)blockIdx.x - N) * 256 + tid;
        if (sim_sums && p < P) {
            double s = sim_sums[p];
            for (int n = 0; n < N; ++n) s += (double)sim[(long)n * P + p];
            sim_sums[p] = s;
        }
        return;
    }
    const int n = blockIdx.x;
    const long row = row_offset + n;
    const float* lg = logits + (long)n * K;
    if (tid == 0) {
        if (probs) {  // softmax over the real-class logits (Video_XProtoNet_e2e.py:114-117)
            float m;
            const float s = softmax_max_sum_f32(lg, K_real, &m);
            for (int k = 0; k < K_real; ++k) probs[row * K_real + k] = __fdiv_rn(expf(lg[k] - m), s);
        }
        if (labels) labels[row] = (int32_t)target[n];
    }
    if (logits_out)
        for (int k = tid; k < K; k += 256) logits_out[row * K + k] = lg[k];
    if (!sparsity && !div_counts) return;
    extern __shared__ float ev_lds[];  // v [P], norm [P], sorted norm [P]
    __shared__ double red[4];
    __shared__ int has_nan;
    float* v = ev_lds;
    float* nrm = ev_lds + P;
    float* srt = ev_lds + 2 * P;
    const float* src = sim + (long)n * P;
    double part = 0.0;
    for (int p = tid; p < P; p += 256) {
        v[p] = src[p];
        part += (double)v[p];
    }
    if (tid == 0) has_nan = 0;
    const float rs = (float)block_sum_fixed(part, red);  // includes a __syncthreads: v and has_nan are visible
    if (div_counts) {  // top-k of each prototype group by similarity, ties to the lower index
        for (int p = tid; p < P; p += 256) {
            const bool cls = p < P_cls;
            const int r = cls ? ev_rank_desc(v, 0, P_cls, p) : ev_rank_desc(v, P_cls, P, p);
            if (r < (cls ? kc : ka)) atomicAdd(&div_counts[p], 1ull);
        }
    }
    if (!sparsity) return;
    for (int p = tid; p < P; p += 256) {
        const float x = __fdiv_rn(v[p], rs);
        nrm[p] = x;
        if (x != x) has_nan = 1;
    }
    __syncthreads();
    if (has_nan) {  // torch.sort puts NaN first: every prefix is NaN, the mask all false, argmax 0
        if (tid == 0) atomicAdd(&sparsity[1], 1ull);
        return;
    }
    for (int p = tid; p < P; p += 256) srt[ev_rank_desc(nrm, 0, P, p)] = nrm[p];
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        int res = 0;
        for (int i = 0; i < P; ++i) {
            acc += (double)srt[i];
            if ((float)acc >= level) {
                res = i;
                break;
            }
        }
        atomicAdd(&sparsity[0], (unsigned long long)res);
        atomicAdd(&sparsity[1], 1ull);
    }
}

// The pairs are tiled by rank_geom (order_key.h).  The AUC takes up to 2^24 rows: a block's per-class sum stays below
// 256 * 2 * chunk <= 2^31 (chunk <= 2^22 for M <= 2^24).
// workspace: int32 pair sums [gy][gx][K] | int32 row stats [gx][K + 2] (positives per class, NaN rows, labels >= K)
__global__ __launch_bounds__(256) void roc_auc_count_kernel(const float* __restrict__ probs, const int32_t* __restrict__ labels, long M,
                                                            int K, RankGeom g, int32_t* __restrict__ pair, int32_t* __restrict__ rstat) {
    __shared__ float s_tile[EVAL_MAX_K * AUC_TILE];  // [k][t]: a wave reads one t at up to K addresses
    __shared__ int32_t l_tile[AUC_TILE];
    __shared__ int32_t acc[EVAL_MAX_K + 2];  // row stats of this block's rows i
    __shared__ int32_t pk[EVAL_MAX_K];       // pair sums per class
    const int tid = threadIdx.x;
    const long i = (long)blockIdx.x * AUC_TILE + tid;
    int L = -1;
    bool bad = false;
    float si = 0.0f;
    if (i < M) {
        L = labels[i];
        if (L >= K) {  // counted below; compares nothing
            bad = true;
            L = -1;
        }
        if (L >= 0) si = probs[i * K + L];
    }
    if (tid < K + 2) acc[tid] = 0;
    if (tid < K) pk[tid] = 0;
    __syncthreads();
    if (blockIdx.y == 0 && i < M) {
        if (L >= 0) {
            atomicAdd(&acc[L], 1);
            bool nan = false;
            for (int k = 0; k < K; ++k) nan |= probs[i * K + k] != probs[i * K + k];
            if (nan) atomicAdd(&acc[K], 1);
        } else if (bad) {
            atomicAdd(&acc[K + 1], 1);
        }
    }
    int cnt = 0;
    const long j0 = (long)blockIdx.y * g.chunk, j1 = min(M, j0 + g.chunk);
    for (long jt = j0; jt < j1; jt += AUC_TILE) {
        const int nt = (int)min((long)AUC_TILE, j1 - jt);
        __syncthreads();
        if (tid < nt) {
            const long j = jt + tid;
            const int lj = labels[j];
            l_tile[tid] = lj;
            for (int k = 0; k < K; ++k) s_tile[k * AUC_TILE + tid] = lj >= 0 && lj < K ? probs[j * K + k] : 0.0f;
        }
        __syncthreads();
        if (L >= 0) {
            const float* col = s_tile + L * AUC_TILE;
            for (int t = 0; t < nt; ++t) {
                const int lj = l_tile[t];
                const float sj = col[t];
                const bool neg = lj >= 0 && lj < K && lj != L;
                cnt += neg ? 2 * (sj < si) + (sj == si) : 0;
            }
        }
    }
    if (L >= 0 && cnt) atomicAdd(&pk[L], cnt);
    __syncthreads();
    if (tid < K) pair[((long)blockIdx.y * g.gx + blockIdx.x) * K + tid] = pk[tid];
    if (blockIdx.y == 0 && tid < K + 2) rstat[(long)blockIdx.x * (K + 2) + tid] = acc[tid];
}

// a / b correctly rounded (what numpy's division gives): the quotient of the division sequence, checked against its exact residual
// fma(-q, b, a) and moved by one ulp when the neighbour is nearer.  Finite non-negative a, positive b (counts) only.
__device__ __forceinline__ double auc_div_rn(double a, double b) {
    const double q = a / b;
    const double r = __fma_rn(-q, b, a);
    if (r == 0.0) return q;
    const double q2 = __longlong_as_double(__double_as_longlong(q) + (r > 0.0 ? 1 : -1));  // the neighbour towards a / b (q >= 0)
    const double r2 = __fma_rn(-q2, b, a);
    return fabs(r2) < fabs(r) ? q2 : q;
}

__global__ __launch_bounds__(256) void roc_auc_finish_kernel(const int32_t* __restrict__ pair, const int32_t* __restrict__ rstat, int K,
                                                             RankGeom g, double* __restrict__ auc, double* __restrict__ auc_k) {
#pragma clang fp contract(off)  // every product rounded on its own, as numpy computes the weighted mean (the HIP default contracts)
    __shared__ long long red[4];
    __shared__ long long tot[2 * EVAL_MAX_K + 2];  // U2 per class | positives per class | NaN rows | bad labels
    const int tid = threadIdx.x;
    const long slots = (long)g.gx * g.gy;
    for (int e = 0; e < 2 * K + 2; ++e) {
        long long s = 0;
        if (e < K) {
            for (long b = tid; b < slots; b += 256) s += pair[b * K + e];
        } else {
            const int c = e - K;  // column of the row stats
            for (long b = tid; b < g.gx; b += 256) s += rstat[b * (K + 2) + c];
        }
        s = block_sum_i64(s, red);
        if (tid == 0) tot[e] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    long long nvalid = 0;
    for (int k = 0; k < K; ++k) nvalid += tot[K + k];
    const bool poisoned = tot[2 * K] > 0 || tot[2 * K + 1] > 0;
    bool defined = !poisoned;
    double num = 0.0, den = 0.0;
    for (int k = 0; k < K; ++k) {
        const long long npos = tot[K + k], nneg = nvalid - npos;
        double a = __builtin_nan("");
        if (!poisoned && npos > 0 && nneg > 0) a = auc_div_rn((double)tot[k], 2.0 * (double)npos * (double)nneg);
        else defined = false;
        auc_k[k] = a;
        num += (double)npos * a;
        den += (double)npos;
    }
    auc[0] = defined ? auc_div_rn(num, den) : 0.0;
}

}  // namespace pasn

using namespace pasn;

extern "C" int pasn_eval_batch_stats(const float* logits, const float* sim, const int64_t* target, int N, int K, int K_real, int P, int P_cls,
                                     int k_cls, int k_abs, float level, long row_offset, long capacity, float* probs, int32_t* labels,
                                     float* logits_out, int64_t* sparsity, int64_t* div_counts, double* sim_sums, void* stream) {
    PASN_REQUIRE(N > 0 && K > 0 && P > 0, "N, K and P must be positive");
    PASN_REQUIRE(K_real >= 1 && K_real <= K, "K_real must lie in [1, K]");
    PASN_REQUIRE(P_cls >= 0 && P_cls <= P, "P_cls must lie in [0, P]");
    PASN_REQUIRE(k_cls >= 0 && k_abs >= 0, "k_cls and k_abs must not be negative");
    PASN_REQUIRE(!(probs || logits_out) || logits, "probs and logits_out need the logits");
    PASN_REQUIRE(!labels || target, "labels need the target");
    PASN_REQUIRE(!(sparsity || div_counts || sim_sums) || sim, "the similarity statistics need sim");
    PASN_REQUIRE(probs || labels || logits_out || sparsity || div_counts || sim_sums, "nothing to write");
    PASN_REQUIRE(!(probs || labels || logits_out) || (row_offset >= 0 && row_offset + N <= capacity), "rows past the epoch buffers' capacity");
    if (P > EV_MAX_P) {
        set_error("pasn_eval_batch_stats: P > 4096 prototypes is not supported (LDS)");
        return PASN_ERR_UNSUPPORTED;
    }
    const int col_blocks = sim_sums ? ceil_div(P, 256) : 0;
    const size_t lds = (sparsity || div_counts) ? (size_t)3 * P * sizeof(float) : 0;
    hipLaunchKernelGGL(eval_batch_stats_kernel, dim3(N + col_blocks), dim3(256), lds, (hipStream_t)stream, logits, sim, target, N, K, K_real,
                       P, P_cls, std::min(k_cls, P_cls), std::min(k_abs, P - P_cls), level, row_offset, probs, labels, logits_out,
                       reinterpret_cast<unsigned long long*>(sparsity), reinterpret_cast<unsigned long long*>(div_counts), sim_sums);
    return check_launch("eval_batch_stats");
}

extern "C" size_t pasn_roc_auc_workspace_bytes(long M, int K_real) {
    if (M <= 0 || K_real <= 0) return 0;
    const RankGeom g = rank_geom(M);
    return ((size_t)g.gy * g.gx * K_real + (size_t)g.gx * (K_real + 2)) * sizeof(int32_t);
}

extern "C" int pasn_roc_auc_ovr(const float* probs, const int32_t* labels, long M, int K_real, double* auc, double* auc_per_class,
                                void* workspace, void* stream) {
    PASN_REQUIRE(probs && labels && auc && auc_per_class && workspace, "probs, labels, auc, auc_per_class and workspace are required");
    PASN_REQUIRE(K_real >= 2 && K_real <= EVAL_MAX_K, "K_real must lie in [2, 16]");
    PASN_REQUIRE(M >= 1 && M <= (1L << 24), "M must lie in [1, 2^24]");
    PASN_REQUIRE(((uintptr_t)workspace & 3) == 0, "misaligned workspace");
    const RankGeom g = rank_geom(M);
    int32_t* pair = static_cast<int32_t*>(workspace);
    int32_t* rstat = pair + (size_t)g.gy * g.gx * K_real;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(roc_auc_count_kernel, dim3(g.gx, g.gy), dim3(256), 0, s, probs, labels, M, K_real, g, pair, rstat);
    hipLaunchKernelGGL(roc_auc_finish_kernel, dim3(1), dim3(256), 0, s, pair, rstat, K_real, g, auc, auc_per_class);
    return check_launch("roc_auc_ovr");
}
