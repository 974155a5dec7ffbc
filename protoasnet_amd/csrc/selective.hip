// selective.hip -- what the abstention output is for: an uncertainty score per clip, one prediction per cine, and the risk-coverage
// curve (accuracy, balanced accuracy and mean F1 of the rows kept when the most uncertain ones are set aside).  The reference trains the
// abstention class (src/loss/loss.py:323-371) and has no code that evaluates it; include/protoasnet_amd.h holds the definitions.
//
// pasn_uncertainty_scores: one thread per row, through softmax_max_sum_f32 (eval_common.h) as eval_batch_stats_kernel (eval_metrics.hip),
// so mode 0 is bitwise 1.0f - the largest entry of the probs row that kernel stores.
//
// pasn_group_predictions: groups as CSR.  One launch, four groups per block.  A group of up to GP_WAVE_ROWS rows belongs to one wave:
// lane k < K_real carries column k's two fp64 sums, every lane the two sums over u, and the wave walks the rows in the listed order.
// A larger group gets the whole block: 256 threads stage 256 rows at a time in LDS, wave 0 adds them -- still in the listed order, so a
// group's sums do not depend on which path it took.  Every add and multiply is __dadd_rn / __dmul_rn (nothing contracts into an FMA).
//
// pasn_risk_coverage: five launches.
//   1. rank: the position of valid row i under (u ascending, NaN last, lower index first) is the number of valid rows j before it,
//      counted out of LDS tiles of 256 keys (rank_count_chunk of order_key.h, which bootstrap.hip calls too).  u maps to a uint32 key
//      that orders as the floats do (-0 = +0, NaN above +inf, padding above NaN).  Integer atomics add the chunks' counts to rank[i];
//      the y = 0 blocks count the valid and the NaN rows.
//   2. scatter: order[rank] = i, threshold[rank] = u_i, cell[rank] = (label, first largest probability).
//   3. histogram: per scan block of 1024 positions, the count of tp_k, support_k and predicted_k for every class.
//   4. curve: a block's base is the sum of the histograms before it; a packed 3 x 20 bit scan per class gives every position its prefix
//      counts, from which the three metrics follow in fp64 (confusion_to_metrics of trainer.py on a prefix).  All counts are integers:
//      the order of arrival cannot matter.  The block also adds its (1 - acc) terms in a fixed tree (block_sum_fixed).
//   5. aurc: the blocks' partial sums in the same tree, over Mv.
#include "common.h"
#include "eval_common.h"

namespace pasn {

constexpr int SEL_TILE = RANK_TILE;
constexpr int GP_WAVE_ROWS = 64;  // larger groups get the block
constexpr int RC_SCAN = 1024;     // positions per scan block: 4 per thread
constexpr ClassCell RC_CELL = {4, 0};  // cell = label * 16 + prediction

// ---- uncertainty scores ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void uncertainty_scores_kernel(const float* __restrict__ logits, long M, int K, int K_real, int mode,
                                                                 float* __restrict__ u) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const float* lg = logits + i * K;
    if (mode == 2) {  // sigmoid of the abstention logit (loss.py:358), never exponentiating a positive number
        const float x = lg[K - 1];
        const float e = expf(-fabsf(x));
        u[i] = __fdiv_rn(x >= 0.0f ? 1.0f : e, 1.0f + e);
        return;
    }
    const int n = mode == 0 ? K_real : K;
    float m;
    const float s = softmax_max_sum_f32(lg, n, &m);
    if (mode == 1) {  // the abstention column of the joined softmax (loss.py:356)
        u[i] = __fdiv_rn(expf(lg[K - 1] - m), s);
        return;
    }
    float best = __fdiv_rn(expf(lg[0] - m), s);
    for (int k = 1; k < n; ++k) {
        const float p = __fdiv_rn(expf(lg[k] - m), s);
        best = p > best ? p : best;  // what max() over the stored row gives; a NaN row is NaN in every entry
    }
    u[i] = 1.0f - best;
}

// ---- one prediction per group ------------------------------------------------------------------------------------------------------------
struct GpAcc {
    double sp, spc, sw, su;  // sum p_k, sum (1 - u) p_k (this lane's column), sum (1 - u), sum u
    int conflict, nan;       // rows whose label differs from the first row's; rows holding a NaN
};

__device__ __forceinline__ void gp_add(GpAcc& a, float ui, float pk, bool col, int lab, int lab0) {
    const double w = __dsub_rn(1.0, (double)ui);
    const double p = (double)pk;
    a.sp = __dadd_rn(a.sp, p);
    a.spc = __dadd_rn(a.spc, __dmul_rn(w, p));
    a.sw = __dadd_rn(a.sw, w);
    a.su = __dadd_rn(a.su, (double)ui);
    a.conflict += lab != lab0;
    a.nan += (__ballot(col && pk != pk) != 0ull) || ui != ui;
}

__device__ __forceinline__ void gp_store(const GpAcc& a, int g, int n, int lab0, int K, int lane, double* __restrict__ p_mean,
                                         double* __restrict__ p_conf, double* __restrict__ u_mean, int32_t* __restrict__ g_label,
                                         int32_t* __restrict__ g_count, int32_t* __restrict__ status) {
    const double dn = (double)n;
    if (lane < K) {
        const double mean = __ddiv_rn(a.sp, dn);
        p_mean[(long)g * K + lane] = mean;
        p_conf[(long)g * K + lane] = a.sw == 0.0 ? mean : __ddiv_rn(a.spc, a.sw);
    }
    if (lane == 0) {
        u_mean[g] = __ddiv_rn(a.su, dn);
        g_label[g] = lab0;
        g_count[g] = n;
        if (a.conflict) atomicAdd(&status[0], 1);
        if (a.nan) atomicAdd(&status[1], a.nan);
    }
}

__global__ __launch_bounds__(256) void group_predictions_kernel(const float* __restrict__ probs, const float* __restrict__ u,
                                                                const int32_t* __restrict__ labels, const int64_t* __restrict__ offs,
                                                                const int32_t* __restrict__ rows, int G, int K, double* __restrict__ p_mean,
                                                                double* __restrict__ p_conf, double* __restrict__ u_mean,
                                                                int32_t* __restrict__ g_label, int32_t* __restrict__ g_count,
                                                                int32_t* __restrict__ status) {
    __shared__ float s_p[SEL_TILE * EVAL_MAX_K];
    __shared__ float s_u[SEL_TILE];
    __shared__ int32_t s_lab[SEL_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool col = lane < K;
    const int kk = col ? lane : 0;
    {  // a wave's own group
        const int g = (int)blockIdx.x * 4 + wave;
        if (g < G) {
            const int64_t lo = offs[g];
            const int n = (int)(offs[g + 1] - lo);
            if (n <= GP_WAVE_ROWS) {
                GpAcc a = {0.0, 0.0, 0.0, 0.0, 0, 0};
                const int lab0 = n > 0 ? labels[rows[lo]] : -1;
                for (int r = 0; r < n; ++r) {
                    const long i = rows[lo + r];
                    gp_add(a, u[i], probs[i * K + kk], col, labels[i], lab0);
                }
                gp_store(a, g, n, lab0, K, lane, p_mean, p_conf, u_mean, g_label, g_count, status);
            }
        }
    }
    for (int w = 0; w < 4; ++w) {  // the block's large groups, one after the other (every condition below is uniform over the block)
        const int g = (int)blockIdx.x * 4 + w;
        if (g >= G) break;
        const int64_t lo = offs[g];
        const int n = (int)(offs[g + 1] - lo);
        if (n <= GP_WAVE_ROWS) continue;
        GpAcc a = {0.0, 0.0, 0.0, 0.0, 0, 0};
        const int lab0 = labels[rows[lo]];
        for (int t0 = 0; t0 < n; t0 += SEL_TILE) {
            const int nt = min(SEL_TILE, n - t0);
            __syncthreads();
            if (tid < nt) {
                const long i = rows[lo + t0 + tid];
                s_u[tid] = u[i];
                s_lab[tid] = labels[i];
                for (int k = 0; k < K; ++k) s_p[tid * EVAL_MAX_K + k] = probs[i * K + k];
            }
            __syncthreads();
            if (wave == 0)
                for (int r = 0; r < nt; ++r) gp_add(a, s_u[r], s_p[r * EVAL_MAX_K + kk], col, s_lab[r], lab0);
        }
        if (wave == 0) gp_store(a, g, n, lab0, K, lane, p_mean, p_conf, u_mean, g_label, g_count, status);
    }
}

// ---- risk-coverage -----------------------------------------------------------------------------------------------------------------------
static int rc_scan_blocks(long M) { return ceil_div(M, RC_SCAN); }

__global__ __launch_bounds__(256) void rc_rank_kernel(const float* __restrict__ u, const int32_t* __restrict__ labels, long M, int K,
                                                      RankGeom g, int32_t* __restrict__ rank, unsigned long long* __restrict__ counts) {
    __shared__ int s_cnt[2];
    const int tid = threadIdx.x;
    const long i = (long)blockIdx.x * RANK_TILE + tid;
    const auto key = [&](long j) {  // a row with a label outside [0, K) never enters
        const int L = labels[j];
        return L >= 0 && L < K ? rc_key(u[j]) : RC_KEY_PAD;
    };
    const uint32_t ki = i < M ? key(i) : RC_KEY_PAD;
    const bool valid = ki != RC_KEY_PAD;
    if (blockIdx.y == 0) {
        if (tid < 2) s_cnt[tid] = 0;
        __syncthreads();
        const unsigned long long bv = __ballot(valid), bn = __ballot(ki == RC_KEY_NAN);
        if ((tid & 63) == 0) {
            if (bv) atomicAdd(&s_cnt[0], __popcll(bv));
            if (bn) atomicAdd(&s_cnt[1], __popcll(bn));
        }
        __syncthreads();
        if (tid < 2 && s_cnt[tid]) atomicAdd(&counts[tid], (unsigned long long)s_cnt[tid]);
    }
    const int cnt = rank_count_chunk(key, ki, M, g.chunk);
    if (valid && cnt) atomicAdd(&rank[i], cnt);
}

__global__ __launch_bounds__(256) void rc_scatter_kernel(const float* __restrict__ probs, const int32_t* __restrict__ labels,
                                                         const float* __restrict__ u, long M, int K, const int32_t* __restrict__ rank,
                                                         int32_t* __restrict__ order, float* __restrict__ threshold,
                                                         int32_t* __restrict__ cell) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const int L = labels[i];
    if (L < 0 || L >= K) return;
    float best;
    const int pred = first_largest(probs + i * K, K, &best);
    const int r = rank[i];  // < Mv <= M: the number of valid rows before this one
    order[r] = (int32_t)i;
    threshold[r] = u[i];
    cell[r] = RC_CELL.pack(L, pred);
}

// hist [nb][3][K] int32: per scan block, tp_k | support_k | predicted_k
__global__ __launch_bounds__(256) void rc_hist_kernel(const int32_t* __restrict__ cell, const unsigned long long* __restrict__ counts, int K,
                                                      int32_t* __restrict__ hist) {
    __shared__ int32_t h[3 * EVAL_MAX_K];
    const int tid = threadIdx.x;
    const long Mv = (long)counts[0];
    if (tid < 3 * K) h[tid] = 0;
    __syncthreads();
    for (int q = 0; q < RC_SCAN / 256; ++q) {
        const long pos = (long)blockIdx.x * RC_SCAN + q * 256 + tid;
        if (pos < Mv) {
            const int c = cell[pos], L = RC_CELL.label(c), P = RC_CELL.pred(c);
            if (L == P) atomicAdd(&h[L], 1);
            atomicAdd(&h[K + L], 1);
            atomicAdd(&h[2 * K + P], 1);
        }
    }
    __syncthreads();
    if (tid < 3 * K) hist[(long)blockIdx.x * 3 * K + tid] = h[tid];
}

__global__ __launch_bounds__(256) void rc_curve_kernel(const int32_t* __restrict__ cell, const unsigned long long* __restrict__ counts,
                                                       int K, const int32_t* __restrict__ hist, double* __restrict__ acc,
                                                       double* __restrict__ bal_acc, double* __restrict__ f1_mean,
                                                       double* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ int32_t base[3 * EVAL_MAX_K];
    __shared__ unsigned long long wsum[4];
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long Mv = (long)counts[0];
    const long p0 = (long)blockIdx.x * RC_SCAN + tid * 4;  // this thread's four positions
    if ((long)blockIdx.x * RC_SCAN >= Mv) {
        if (tid == 0) partial[blockIdx.x] = 0.0;
        return;
    }
    if (tid < 3 * K) {
        int32_t s = 0;
        for (int b = 0; b < (int)blockIdx.x; ++b) s += hist[(long)b * 3 * K + tid];
        base[tid] = s;
    }
    int L[4], P[4];
    for (int q = 0; q < 4; ++q) {
        const bool in = p0 + q < Mv;
        const int c = in ? cell[p0 + q] : 0;
        L[q] = in ? RC_CELL.label(c) : -1;
        P[q] = in ? RC_CELL.pred(c) : -1;
    }
    ClassTally tally[4];
    for (int k = 0; k < K; ++k) {
        // inclusive prefix of (tp_k, support_k, predicted_k) packed 20 bits each: a block holds 1024 positions
        unsigned long long loc[4], run = 0ull;
        for (int q = 0; q < 4; ++q) {
            run += (unsigned long long)(L[q] == k && P[q] == k) | ((unsigned long long)(L[q] == k) << 20) | ((unsigned long long)(P[q] == k) << 40);
            loc[q] = run;
        }
        const unsigned long long inc = wave_scan_incl(run);
        __syncthreads();  // wsum of the class before has been read; base is visible (k = 0)
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        unsigned long long ex = inc - run;
        for (int w = 0; w < wave; ++w) ex += wsum[w];
        for (int q = 0; q < 4; ++q) {
            const unsigned long long v = ex + loc[q];
            const long tp = base[k] + (long)(v & 0xFFFFFull), sup = base[K + k] + (long)((v >> 20) & 0xFFFFFull),
                       prd = base[2 * K + k] + (long)((v >> 40) & 0xFFFFFull);
            tally[q].add(tp, sup, prd);
        }
    }
    double e = 0.0;
    for (int q = 0; q < 4; ++q) {
        const long m = p0 + q + 1;  // the rows kept: >= 1
        if (m > Mv) break;
        const double a = tally[q].accuracy(m);
        acc[m - 1] = a;
        bal_acc[m - 1] = tally[q].balanced_accuracy();
        f1_mean[m - 1] = tally[q].f1_mean(K);
        e += 1.0 - a;
    }
    e = block_sum_fixed(e, red);
    if (tid == 0) partial[blockIdx.x] = e;
}

__global__ __launch_bounds__(256) void rc_aurc_kernel(const double* __restrict__ partial, int nb,
                                                      const unsigned long long* __restrict__ counts, double* __restrict__ aurc) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int b = tid; b < nb; b += 256) s += partial[b];
    s = block_sum_fixed(s, red);
    if (tid == 0) {
        const long Mv = (long)counts[0];
        aurc[0] = Mv > 0 ? s / (double)Mv : __builtin_nan("");
    }
}

struct RcWorkspace {
    double* partial;
    int32_t *rank, *cell, *hist;
    size_t bytes;
};

static RcWorkspace rc_workspace(void* ws, long M, int K) {
    RcWorkspace w;
    Carve c{static_cast<char*>(ws)};
    const size_t nb = (size_t)rc_scan_blocks(M);
    w.partial = c.take<double>(nb);
    w.rank = c.take<int32_t>((size_t)M);
    w.cell = c.take<int32_t>((size_t)M);
    w.hist = c.take<int32_t>(nb * 3 * K);
    w.bytes = c.used;
    return w;
}

}  // namespace pasn

using namespace pasn;

extern "C" int pasn_uncertainty_scores(const float* logits, long M, int K, int K_real, int mode, float* u, void* stream) {
    PASN_REQUIRE(logits && u, "logits and u are required");
    PASN_REQUIRE(M >= 1, "M must be positive");
    PASN_REQUIRE(K_real >= 2 && K_real <= EVAL_MAX_K, "K_real must lie in [2, 16]");
    PASN_REQUIRE(K >= K_real && K <= EVAL_MAX_K + 1, "K must lie in [K_real, 17]");
    PASN_REQUIRE(mode >= 0 && mode <= 2, "mode must be 0 (maxprob), 1 (alpha, joined) or 2 (alpha, separate)");
    PASN_REQUIRE(mode != 1 || K == K_real + 1, "mode 1 (alpha, joined) needs K == K_real + 1");
    PASN_REQUIRE(mode != 2 || K > K_real, "mode 2 (alpha, separate) needs an abstention column: K > K_real");
    hipLaunchKernelGGL(uncertainty_scores_kernel, dim3(ceil_div(M, 256)), dim3(256), 0, (hipStream_t)stream, logits, M, K, K_real, mode, u);
    return check_launch("uncertainty_scores");
}

extern "C" int pasn_group_predictions(const float* probs, const float* u, const int32_t* labels, const int64_t* group_offsets,
                                      const int32_t* group_rows, int G, int K_real, double* p_mean, double* p_conf, double* u_mean,
                                      int32_t* g_label, int32_t* g_count, int32_t* status, void* stream) {
    PASN_REQUIRE(probs && u && labels && group_offsets && group_rows, "probs, u, labels, group_offsets and group_rows are required");
    PASN_REQUIRE(p_mean && p_conf && u_mean && g_label && g_count && status, "every output is required");
    PASN_REQUIRE(G >= 1, "G must be positive");
    PASN_REQUIRE(K_real >= 2 && K_real <= EVAL_MAX_K, "K_real must lie in [2, 16]");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, 2 * sizeof(int32_t), s) != hipSuccess) return check_launch("group_predictions (status)");
    hipLaunchKernelGGL(group_predictions_kernel, dim3(ceil_div(G, 4)), dim3(256), 0, s, probs, u, labels, group_offsets, group_rows, G, K_real,
                       p_mean, p_conf, u_mean, g_label, g_count, status);
    return check_launch("group_predictions");
}

extern "C" size_t pasn_risk_coverage_workspace_bytes(long M, int K_real) {
    if (M <= 0 || M > EVAL_MAX_ROWS || K_real < 2 || K_real > EVAL_MAX_K) return 0;
    return rc_workspace(nullptr, M, K_real).bytes;
}

extern "C" int pasn_risk_coverage(const float* probs, const int32_t* labels, const float* u, long M, int K_real, int32_t* order, double* acc,
                                  double* bal_acc, double* f1_mean, float* threshold, double* aurc, int64_t* counts, void* workspace,
                                  void* stream) {
    PASN_REQUIRE(probs && labels && u, "probs, labels and u are required");
    PASN_REQUIRE(order && acc && bal_acc && f1_mean && threshold && aurc && counts, "every output is required");
    PASN_REQUIRE(workspace, "workspace is required");
    PASN_REQUIRE(K_real >= 2 && K_real <= EVAL_MAX_K, "K_real must lie in [2, 16]");
    PASN_REQUIRE(M >= 1 && M <= EVAL_MAX_ROWS, "M must lie in [1, 2^20]");
    PASN_REQUIRE(((uintptr_t)workspace & 7) == 0, "misaligned workspace");
    const RankGeom g = rank_geom(M);
    const int nb = rc_scan_blocks(M);
    const RcWorkspace w = rc_workspace(workspace, M, K_real);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
    if (hipMemsetAsync(w.rank, 0, (size_t)M * sizeof(int32_t), s) != hipSuccess || hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s) != hipSuccess)
        return check_launch("risk_coverage (zeroing)");
    hipLaunchKernelGGL(rc_rank_kernel, dim3(g.gx, g.gy), dim3(256), 0, s, u, labels, M, K_real, g, w.rank, cnt);
    hipLaunchKernelGGL(rc_scatter_kernel, dim3(g.gx), dim3(256), 0, s, probs, labels, u, M, K_real, w.rank, order, threshold, w.cell);
    hipLaunchKernelGGL(rc_hist_kernel, dim3(nb), dim3(256), 0, s, w.cell, cnt, K_real, w.hist);
    hipLaunchKernelGGL(rc_curve_kernel, dim3(nb), dim3(256), 0, s, w.cell, cnt, K_real, w.hist, acc, bal_acc, f1_mean, w.partial);
    hipLaunchKernelGGL(rc_aurc_kernel, dim3(1), dim3(256), 0, s, w.partial, nb, cnt, aurc);
    return check_launch("risk_coverage");
}
