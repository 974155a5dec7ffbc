// calibration.hip -- are the model's numbers probabilities?  Reliability bins, ECE / MCE / class-wise ECE / Brier / NLL / confidence gap of
// the sample and of its grouped-bootstrap replicates, and temperature scaling (one scalar fitted on a split, applied on another).
// include/protoasnet_amd.h holds the definitions, tests/calibration_cases.py their float64 / int64 restatement.
//
// pasn_calibration_bins: what all replicates share is computed once (calib_rows_kernel): per row its unit (-1: the row never enters), a
// 64-bit word (q | bin << 40 | hit << 46 | skipped << 47 | label << 48) for the top label and one (q | bin << 40 | unbinned << 47) per
// class, and the row's fp64 Brier and NLL terms; the top label is first_largest of eval_common.h, the rule of the confusion matrix and of
// the risk-coverage curve.  Then a block owns an output row (replicate b < B, or the point estimate B: every weight
// 1), the blocks looping when B + 1 exceeds the grid: per row it gathers one count and adds into ONE LDS histogram of (K_real + 1) x n_bins x
// {n, hit, qsum} with 64-bit integer LDS atomics -- integers, so the histogram does not depend on the order --, the Brier / NLL sums go
// through block_sum_fixed, and thread 0 writes the statistics.
//
// pasn_temperature_fit: safeguarded Newton on the convex g(beta) across LAUNCH boundaries: no block ever waits for another.  Launch s
// re-adds the (g, g', g'', rows) partials of launch s - 1 in index order -- every block redundantly and identically --, advances the
// state (bracket, beta, status) from them, and reduces its slice of the rows at the new beta into its slot of a double-buffered partial
// array.  Launches 0 .. 2 evaluate 1/64, 64 and 1; launches 3 .. 50 take the PASN_TEMPERATURE_STEPS steps; a one-block finish writes `fit`.
#include <cfloat>

#include "common.h"
#include "eval_common.h"

namespace pasn {

constexpr int CAL_MAX_BINS = 64, CAL_NT = 256, CAL_MAX_GRID = 2048;
constexpr unsigned long long CAL_Q_MASK = (1ull << 40) - 1, CAL_HIT = 1ull << 46, CAL_SKIP = 1ull << 47;
constexpr int TEMP_MAX_BLOCKS = 256, TEMP_LAUNCHES = 3 + PASN_TEMPERATURE_STEPS;
constexpr double TEMP_LO = 1.0 / 64.0, TEMP_HI = 64.0;

// ---- the reliability bins ----------------------------------------------------------------------------------------------------------------
// (q | bin << 40) of a confidence in [0, 1]; CAL_SKIP for anything else (NaN included)
__device__ __forceinline__ unsigned long long cal_word(float c, int n_bins) {
    if (!(c >= 0.0f && c <= 1.0f)) return CAL_SKIP;
    const double d = (double)c;
    const int bin = min(n_bins - 1, (int)(d * (double)n_bins));
    return (unsigned long long)(d * 4294967296.0) | ((unsigned long long)bin << 40);
}

struct CalWorkspace {
    unsigned long long *top, *cls;  // [M], [M][K]
    double* terms;                  // [M][2]: Brier, NLL
    int32_t* unit;                  // [M]
    size_t bytes;
};

static CalWorkspace cal_workspace(void* ws, long M, int K) {
    CalWorkspace w;
    Carve c{static_cast<char*>(ws)};
    w.top = c.take<unsigned long long>((size_t)M);
    w.cls = c.take<unsigned long long>((size_t)M * K);
    w.terms = c.take<double>((size_t)M * 2);
    w.unit = c.take<int32_t>(((size_t)M + 3) / 4 * 4);  // rounded up to 16 bytes
    w.bytes = c.used;
    return w;
}

__global__ __launch_bounds__(CAL_NT) void calib_rows_kernel(const float* __restrict__ probs, const int32_t* __restrict__ labels,
                                                            const float* __restrict__ conf, const int32_t* __restrict__ row_unit, long M,
                                                            long G, int K, int n_bins, CalWorkspace w) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * CAL_NT + threadIdx.x;
    if (i >= M) return;
    const int L = labels[i];
    const long g = row_unit ? (long)row_unit[i] : i;
    if (L < 0 || L >= K || g < 0 || g >= G) {  // padding, or a row no group lists (a unit past G would read past `counts`)
        w.unit[i] = -1;
        return;
    }
    const float* p = probs + i * K;
    float best;
    const int pred = first_largest(p, K, &best);
    double brier = 0.0, pl = 0.0;
    for (int k = 0; k < K; ++k) {
        const float v = p[k];
        const double d = (double)v - (k == L ? 1.0 : 0.0);
        brier += d * d;
        if (k == L) pl = (double)v;
        w.cls[i * K + k] = cal_word(v, n_bins);
    }
    w.top[i] = cal_word(conf ? conf[i] : best, n_bins) | (pred == L ? CAL_HIT : 0ull) | ((unsigned long long)L << 48);
    w.terms[2 * i] = brier;
    w.terms[2 * i + 1] = -log(fmax(pl, (double)FLT_MIN));
    w.unit[i] = (int32_t)g;
}

struct CalArgs {
    CalWorkspace w;
    const int32_t* counts;
    long M, G;
    int K, n_bins, B;
    int64_t *n, *hit, *cn, *cpos, *skipped;
    uint64_t *qsum, *cq;
    double* stats;
};

__global__ __launch_bounds__(CAL_NT) void calib_bins_kernel(CalArgs a) {
#pragma clang fp contract(off)
    __shared__ unsigned long long s_h[(EVAL_MAX_K + 1) * CAL_MAX_BINS * 3];  // [K + 1][n_bins][n, hit, qsum]; table K is the top label's
    __shared__ unsigned long long s_skip;
    __shared__ double s_red[CAL_NT / 64];
    const int tid = threadIdx.x, K = a.K, nb = a.n_bins, cells = (K + 1) * nb * 3;
    unsigned long long* s_top = s_h + K * nb * 3;
    for (int r = blockIdx.x; r <= a.B; r += gridDim.x) {
        __syncthreads();  // the row before has been written out
        for (int e = tid; e < cells; e += CAL_NT) s_h[e] = 0ull;
        if (tid == 0) s_skip = 0ull;
        __syncthreads();
        const int32_t* cnt = r < a.B ? a.counts + (long)r * a.G : nullptr;
        double brier = 0.0, nll = 0.0;
        for (long i = tid; i < a.M; i += CAL_NT) {
            const int g = a.w.unit[i];
            if (g < 0) continue;
            const unsigned long long wt = cnt ? (unsigned long long)(uint32_t)cnt[g] : 1ull;
            if (wt == 0ull) continue;
            const unsigned long long t = a.w.top[i];
            const int L = (int)(t >> 48);
            if (t & CAL_SKIP) {
                atomicAdd(&s_skip, wt);
            } else {
                unsigned long long* h = s_top + (int)((t >> 40) & 63) * 3;
                atomicAdd(h, wt);
                if (t & CAL_HIT) atomicAdd(h + 1, wt);
                atomicAdd(h + 2, wt * (t & CAL_Q_MASK));
            }
            for (int k = 0; k < K; ++k) {
                const unsigned long long c = a.w.cls[i * K + k];
                if (c & CAL_SKIP) continue;
                unsigned long long* h = s_h + (k * nb + (int)((c >> 40) & 63)) * 3;
                atomicAdd(h, wt);
                if (k == L) atomicAdd(h + 1, wt);
                atomicAdd(h + 2, wt * (c & CAL_Q_MASK));
            }
            const double wd = (double)wt;
            brier += wd * a.w.terms[2 * i];
            nll += wd * a.w.terms[2 * i + 1];
        }
        brier = block_sum_fixed(brier, s_red);  // (its barriers also close the histogram)
        nll = block_sum_fixed(nll, s_red);
        for (int e = tid; e < nb * 3; e += CAL_NT) {
            const int j = e / 3, f = e % 3;
            const unsigned long long v = s_top[e];
            if (f == 0) a.n[(long)r * nb + j] = (int64_t)v;
            else if (f == 1) a.hit[(long)r * nb + j] = (int64_t)v;
            else a.qsum[(long)r * nb + j] = v;
        }
        for (int e = tid; e < K * nb * 3; e += CAL_NT) {
            const int j = e / 3, f = e % 3;  // j = k * n_bins + bin
            const unsigned long long v = s_h[e];
            if (f == 0) a.cn[(long)r * K * nb + j] = (int64_t)v;
            else if (f == 1) a.cpos[(long)r * K * nb + j] = (int64_t)v;
            else a.cq[(long)r * K * nb + j] = v;
        }
        if (tid != 0) continue;
        a.skipped[r] = (int64_t)s_skip;
        double gap_abs = 0.0, gap = 0.0, worst = 0.0;
        unsigned long long W = 0ull;
        for (int j = 0; j < nb; ++j) {
            const unsigned long long nj = s_top[3 * j];
            const double d = (double)s_top[3 * j + 2] * 0x1p-32 - (double)s_top[3 * j + 1];  // conf_j - hit_j
            W += nj;
            gap += d;
            gap_abs += fabs(d);
            if (nj > 0ull) worst = fmax(worst, fabs(d) / (double)nj);
        }
        double cw = 0.0;
        for (int e = 0; e < K * nb; ++e) cw += fabs((double)s_h[3 * e + 1] - (double)s_h[3 * e + 2] * 0x1p-32);
        const double nan = __builtin_nan(""), Wd = (double)W, Wv = (double)(W + s_skip);
        double* st = a.stats + (long)r * 6;
        st[0] = W > 0ull ? gap_abs / Wd : nan;
        st[1] = W > 0ull ? worst : nan;
        st[2] = Wv > 0.0 ? cw / Wv / (double)K : nan;
        st[3] = Wv > 0.0 ? brier / Wv : nan;
        st[4] = Wv > 0.0 ? nll / Wv : nan;
        st[5] = W > 0ull ? gap / Wd : nan;
    }
}

static bool cal_sizes_ok(long M, long G, int K, int n_bins, int B) {
    return K >= 2 && K <= EVAL_MAX_K && M >= 1 && M <= EVAL_MAX_ROWS && G >= 1 && G <= M && n_bins >= 1 && n_bins <= CAL_MAX_BINS && B >= 0 &&
           B <= EVAL_MAX_REPLICATES;
}

// ---- temperature scaling -----------------------------------------------------------------------------------------------------------------
struct TempState {
    double lo, hi, beta, status, g1, d_lo, d_hi, pad;
};

struct TempSums {
    double g, d1, d2, rows;
};

struct TempWorkspace {
    TempState* state;  // [2]
    TempSums* part;    // [2][TEMP_MAX_BLOCKS]
};

static TempWorkspace temp_workspace(void* ws) {
    TempWorkspace w;
    w.state = static_cast<TempState*>(ws);
    w.part = reinterpret_cast<TempSums*>(w.state + 2);
    return w;
}

static int temp_blocks(long M) { return std::min(ceil_div(M, CAL_NT), TEMP_MAX_BLOCKS); }

// The softmax moments of one row at beta, every value fp64, d_k = z_k - z_max: returns S = sum_k exp(beta d_k); *mean = E_beta[d],
// *var = Var_beta[d], *dl = d_label (L < 0: unused).  Fully unrolled with guards: no indexed private array, no scratch.
__device__ __forceinline__ double temp_row(const float* __restrict__ z, int K, int L, double beta, double* e, double* mean, double* var,
                                           double* dl) {
#pragma clang fp contract(off)
    double d[EVAL_MAX_K];
    float zmax = z[0];
#pragma unroll
    for (int k = 1; k < EVAL_MAX_K; ++k)
        if (k < K) zmax = fmaxf(zmax, z[k]);
    double S = 0.0, m = 0.0, v = 0.0, lab = 0.0;
#pragma unroll
    for (int k = 0; k < EVAL_MAX_K; ++k) {
        d[k] = k < K ? (double)z[k] - (double)zmax : 0.0;
        e[k] = k < K ? exp(beta * d[k]) : 0.0;
        S += e[k];
        m += e[k] * d[k];
        if (k == L) lab = d[k];
    }
    m = m / S;
#pragma unroll
    for (int k = 0; k < EVAL_MAX_K; ++k) v += e[k] * ((d[k] - m) * (d[k] - m));
    *mean = m;
    *var = v / S;
    *dl = lab;
    return S;
}

__device__ __forceinline__ TempSums temp_total(const TempSums* __restrict__ part, int nblocks) {
#pragma clang fp contract(off)
    TempSums t = {0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < nblocks; ++b) {  // index order
        t.g += part[b].g;
        t.d1 += part[b].d1;
        t.d2 += part[b].d2;
        t.rows += part[b].rows;
    }
    return t;
}

// the state after launch s - 1's sums: which beta launch s evaluates
__device__ __forceinline__ TempState temp_advance(int s, TempState st, const TempSums& t) {
#pragma clang fp contract(off)
    if (s == 0) {
        st = TempState{TEMP_LO, TEMP_HI, TEMP_LO, 0.0, 0.0, 0.0, 0.0, 0.0};
    } else if (s == 1) {
        st.d_lo = t.d1;
        st.beta = TEMP_HI;
    } else if (s == 2) {
        st.d_hi = t.d1;
        st.beta = 1.0;
    } else {
        if (s == 3) {
            st.g1 = t.g;
            if (t.rows == 0.0) {
                st.status = 3.0;
            } else if (st.d_lo >= 0.0) {
                st.status = 1.0;
                st.beta = TEMP_LO;
            } else if (st.d_hi <= 0.0) {
                st.status = 2.0;
                st.beta = TEMP_HI;
            }
        }
        if (st.status == 0.0) {  // one safeguarded Newton step; at a bound or without rows beta stays where it is
            if (t.d1 > 0.0) st.hi = st.beta;
            else if (t.d1 < 0.0) st.lo = st.beta;
            else st.lo = st.hi = st.beta;
            const double nt = st.beta - t.d1 / t.d2;
            st.beta = (t.d2 > 0.0 && nt > st.lo && nt < st.hi) ? nt : 0.5 * (st.lo + st.hi);
        }
    }
    return st;
}

__global__ __launch_bounds__(CAL_NT) void temp_step_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels, long M, int K,
                                                           int K_real, int s, TempWorkspace w) {
#pragma clang fp contract(off)
    __shared__ double s_red[CAL_NT / 64];
    __shared__ double s_beta;
    const int tid = threadIdx.x, nblocks = gridDim.x;
    if (tid == 0) {
        TempSums t = {0.0, 0.0, 0.0, 0.0};
        if (s > 0) t = temp_total(w.part + (s & 1) * TEMP_MAX_BLOCKS, nblocks);
        const TempState st = temp_advance(s, w.state[s & 1], t);  // (s == 0 reads nothing of it)
        if (blockIdx.x == 0) w.state[(s + 1) & 1] = st;
        s_beta = st.beta;
    }
    __syncthreads();
    const double beta = s_beta;
    TempSums acc = {0.0, 0.0, 0.0, 0.0};
    for (long i = (long)blockIdx.x * CAL_NT + tid; i < M; i += (long)nblocks * CAL_NT) {
        const int L = labels[i];
        if (L < 0 || L >= K_real) continue;
        double e[EVAL_MAX_K], mean, var, dl;
        const double S = temp_row(logits + i * K, K_real, L, beta, e, &mean, &var, &dl);
        acc.g += log(S) - beta * dl;
        acc.d1 += mean - dl;
        acc.d2 += var;
        acc.rows += 1.0;
    }
    acc.g = block_sum_fixed(acc.g, s_red);
    acc.d1 = block_sum_fixed(acc.d1, s_red);
    acc.d2 = block_sum_fixed(acc.d2, s_red);
    acc.rows = block_sum_fixed(acc.rows, s_red);
    if (tid == 0) w.part[((s + 1) & 1) * TEMP_MAX_BLOCKS + blockIdx.x] = acc;
}

__global__ void temp_finish_kernel(TempWorkspace w, int nblocks, double* __restrict__ fit) {
    if (threadIdx.x != 0) return;
    const TempSums t = temp_total(w.part + (TEMP_LAUNCHES & 1) * TEMP_MAX_BLOCKS, nblocks);  // g at the last beta
    const TempState st = w.state[TEMP_LAUNCHES & 1];
    fit[0] = st.beta;
    fit[1] = st.g1 / t.rows;  // no valid row: 0 / 0
    fit[2] = t.g / t.rows;
    fit[3] = st.status;
}

__global__ __launch_bounds__(CAL_NT) void temp_probs_kernel(const float* __restrict__ logits, long M, int K, int K_real,
                                                            const double* __restrict__ beta, float* __restrict__ probs, float* __restrict__ u) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * CAL_NT + threadIdx.x;
    if (i >= M) return;
    double e[EVAL_MAX_K], mean, var, dl;
    const double S = temp_row(logits + i * K, K_real, -1, beta[0], e, &mean, &var, &dl);
    float best = 0.0f;
#pragma unroll
    for (int k = 0; k < EVAL_MAX_K; ++k)
        if (k < K_real) {
            const float p = (float)(e[k] / S);
            probs[i * K_real + k] = p;
            best = fmaxf(best, p);
        }
    if (u) u[i] = 1.0f - best;
}

static bool temp_sizes_ok(long M, int K, int K_real) { return K_real >= 2 && K_real <= EVAL_MAX_K && K >= K_real && K <= 17 && M >= 1 && M <= EVAL_MAX_ROWS; }

}  // namespace pasn

using namespace pasn;

extern "C" size_t pasn_calibration_workspace_bytes(long M, long G, int K_real, int n_bins, int B) {
    if (!cal_sizes_ok(M, G, K_real, n_bins, B)) return 0;
    return cal_workspace(nullptr, M, K_real).bytes;
}

extern "C" int pasn_calibration_bins(const float* probs, const int32_t* labels, const float* conf, const int32_t* row_unit,
                                     const int32_t* counts, long M, long G, int K_real, int n_bins, int B, int64_t* n, int64_t* hit,
                                     uint64_t* qsum, int64_t* cn, int64_t* cpos, uint64_t* cq, int64_t* skipped, double* stats,
                                     void* workspace, void* stream) {
    PASN_REQUIRE(probs && labels, "probs and labels are required");
    PASN_REQUIRE(n && hit && qsum && cn && cpos && cq && skipped && stats, "every output is required");
    PASN_REQUIRE(workspace, "workspace is required");
    PASN_REQUIRE(K_real >= 2 && K_real <= EVAL_MAX_K, "K_real must lie in [2, 16]");
    PASN_REQUIRE(M >= 1 && M <= EVAL_MAX_ROWS, "M must lie in [1, 2^20]");
    PASN_REQUIRE(G >= 1 && G <= M, "G must lie in [1, M]");
    PASN_REQUIRE(row_unit || G == M, "without row_unit every row is its own unit: G must equal M");
    PASN_REQUIRE(n_bins >= 1 && n_bins <= CAL_MAX_BINS, "n_bins must lie in [1, 64]");
    PASN_REQUIRE(B >= 0 && B <= EVAL_MAX_REPLICATES, "B must lie in [0, 65536]");
    PASN_REQUIRE((counts == nullptr) == (B == 0), "counts is NULL exactly when B == 0");
    PASN_REQUIRE(((uintptr_t)workspace & 15) == 0, "misaligned workspace");
    hipStream_t s = (hipStream_t)stream;
    CalArgs a;
    a.w = cal_workspace(workspace, M, K_real);
    hipLaunchKernelGGL(calib_rows_kernel, dim3(ceil_div(M, CAL_NT)), dim3(CAL_NT), 0, s, probs, labels, conf, row_unit, M, G, K_real, n_bins, a.w);
    a.counts = counts;
    a.M = M;
    a.G = G;
    a.K = K_real;
    a.n_bins = n_bins;
    a.B = B;
    a.n = n;
    a.hit = hit;
    a.qsum = qsum;
    a.cn = cn;
    a.cpos = cpos;
    a.cq = cq;
    a.skipped = skipped;
    a.stats = stats;
    hipLaunchKernelGGL(calib_bins_kernel, dim3(std::min(B + 1, CAL_MAX_GRID)), dim3(CAL_NT), 0, s, a);
    return check_launch("calibration_bins");
}

extern "C" size_t pasn_temperature_workspace_bytes(long M, int K_real) {
    if (!temp_sizes_ok(M, K_real, K_real)) return 0;
    return 2 * sizeof(TempState) + 2 * TEMP_MAX_BLOCKS * sizeof(TempSums);
}

extern "C" int pasn_temperature_fit(const float* logits, const int32_t* labels, long M, int K, int K_real, double* fit, void* workspace,
                                    void* stream) {
    PASN_REQUIRE(logits && labels && fit, "logits, labels and fit are required");
    PASN_REQUIRE(workspace, "workspace is required");
    PASN_REQUIRE(K_real >= 2 && K_real <= EVAL_MAX_K, "K_real must lie in [2, 16]");
    PASN_REQUIRE(K >= K_real && K <= 17, "K must lie in [K_real, 17]");
    PASN_REQUIRE(M >= 1 && M <= EVAL_MAX_ROWS, "M must lie in [1, 2^20]");
    PASN_REQUIRE(((uintptr_t)workspace & 15) == 0, "misaligned workspace");
    hipStream_t s = (hipStream_t)stream;
    const TempWorkspace w = temp_workspace(workspace);
    const int nblocks = temp_blocks(M);
    for (int step = 0; step < TEMP_LAUNCHES; ++step)
        hipLaunchKernelGGL(temp_step_kernel, dim3(nblocks), dim3(CAL_NT), 0, s, logits, labels, M, K, K_real, step, w);
    hipLaunchKernelGGL(temp_finish_kernel, dim3(1), dim3(64), 0, s, w, nblocks, fit);
    return check_launch("temperature_fit");
}

extern "C" int pasn_temperature_probs(const float* logits, long M, int K, int K_real, const double* beta, float* probs, float* u, void* stream) {
    PASN_REQUIRE(logits && beta && probs, "logits, beta and probs are required");
    PASN_REQUIRE(K_real >= 2 && K_real <= EVAL_MAX_K, "K_real must lie in [2, 16]");
    PASN_REQUIRE(K >= K_real && K <= 17, "K must lie in [K_real, 17]");
    PASN_REQUIRE(M >= 1 && M <= EVAL_MAX_ROWS, "M must lie in [1, 2^20]");
    hipLaunchKernelGGL(temp_probs_kernel, dim3(ceil_div(M, CAL_NT)), dim3(CAL_NT), 0, (hipStream_t)stream, logits, M, K, K_real, beta, probs, u);
    return check_launch("temperature_probs");
}
