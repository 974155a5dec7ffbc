// bootstrap.hip -- grouped bootstrap replicates of the evaluation statistics (accuracy, balanced accuracy, mean F1, weighted one-vs-rest
// AUC, risk-coverage area, error-detection AUROC).  The resampling unit is a group of rows (a cine's clips); include/protoasnet_amd.h holds
// the definitions, tests/bootstrap_cases.py their float64 / int64 restatement.
//
// pasn_bootstrap_counts: the draws alone.  Draw d of replicate b is output word d & 3 of Philox4x32-10 at counter (d >> 2, b, 0, 0); the
// unit is (r * G) >> 32.  G <= BOOT_LDS_MAX_G: a block per replicate histograms into uint16 pairs in LDS (integer LDS atomics) and writes the
// row out; above, the threads add straight into the zeroed output (global integer atomics).
//
// pasn_bootstrap_metrics: what all replicates share is computed once, in five launches:
//   1. gid: the group of every listed row (a wave per group), -1 for the others
//   2. info: per row (group | label << 20 | first largest probability << 24), negative for a row that never enters
//   3. rank: rank_count_chunk of order_key.h for every class column (ascending probability) and for u (ascending, NaN last)
//   4. scatter: per order and position the word (group | POS | NAN) and the key; POS marks the positives of the order (label == k for
//      column k, a wrong prediction for u)
//   5. ties: TIE marks the first position of every run of equal keys
// and one launch does the replicates, a block each (replicate B is the point estimate: every count 1).  The block draws its counts (LDS
// uint16 for G <= BOOT_LDS_MAX_G; above, an int32 slice of the workspace owned by the block, blocks looping over the replicates), adds the
// confusion matrix with integer LDS atomics, and sweeps every order in chunks of 2048 positions, eight per thread: a block-wide scan of
// the (negative, positive) weight packed in 64 bits gives each position the weights before it, a second scan carries the prefix AT THE
// START OF ITS TIE RUN forward, and
//   U2 = Wp Wn + sum_{i pos} w_i Nlt_i - sum_{j neg} w_j Plt_j        (Nlt / Plt: negative / positive weight with a strictly smaller key)
// which is sum w_i w_j (2 [s_j < s_i] + [s_j == s_i]) over the pairs, in integers.  The u order also adds the risk terms 1 - acc[m] of
// every copy of a row, each thread its positions in order, the threads in the tree of block_sum_fixed.  One barrier per chunk (wave
// summaries in a double-buffered LDS table).  Thread 0 turns the confusion matrix into accuracy, balanced accuracy and mean F1 with the
// ClassTally of eval_common.h, the arithmetic of rc_curve_kernel (selective.hip).
#include "boot_draw.h"
#include "common.h"
#include "eval_common.h"

namespace pasn {

constexpr int BOOT_E = 8, BOOT_CHUNK = BOOT_NT * BOOT_E;
constexpr uint32_t BOOT_EMPTY = 0xFFFFFFFFu, BOOT_TIE = 1u << 31, BOOT_POS = 1u << 30, BOOT_NAN = 1u << 29, BOOT_GID = 0xFFFFFu;
constexpr ClassCell BOOT_CELL = {20, 24};  // info = group | label << 20 | prediction << 24

// ---- draws (the per-block draws themselves: boot_draw.h) -------------------------------------------------------------------------------
__global__ __launch_bounds__(BOOT_NT) void boot_counts_lds_kernel(int32_t* __restrict__ counts, int G, int B, uint32_t k0, uint32_t k1, int b0) {
    extern __shared__ uint32_t boot_lds[];
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        __syncthreads();  // the row before has been read
        boot_draw_lds(boot_lds, G, (uint32_t)(b0 + b), k0, k1, false);
        for (int g = threadIdx.x; g < G; g += BOOT_NT) counts[(long)b * G + g] = (int32_t)boot_count_lds(boot_lds, g);
    }
}

// grid (blocks of 256 Philox calls, replicates); counts is zero
__global__ __launch_bounds__(BOOT_NT) void boot_counts_global_kernel(int32_t* __restrict__ counts, long G, int B, uint32_t k0, uint32_t k1, int b0) {
    const long q = (long)blockIdx.x * BOOT_NT + threadIdx.x;
    if (q >= (G + 3) / 4) return;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        uint32_t r[4];
        philox4x32_10((uint32_t)q, (uint32_t)(b0 + b), 0u, 0u, k0, k1, r);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * q + j < G) atomicAdd(&counts[(long)b * G + philox_unit(r[j], (uint32_t)G)], 1);
    }
}

// ---- what the replicates share -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void boot_gid_kernel(const int64_t* __restrict__ offs, const int32_t* __restrict__ rows, long G, long M,
                                                       int32_t* __restrict__ gid) {
    const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= G) return;
    const int64_t lo = offs[g], hi = offs[g + 1];
    for (int64_t r = lo + (threadIdx.x & 63); r < hi; r += 64) {
        const long i = rows[r];
        if (i >= 0 && i < M) gid[i] = (int32_t)g;
    }
}

__global__ __launch_bounds__(256) void boot_info_kernel(const float* __restrict__ probs, const int32_t* __restrict__ labels,
                                                        const int32_t* __restrict__ gid, long M, int K, int32_t* __restrict__ info) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const int L = labels[i];
    const int g = gid ? gid[i] : (int)i;
    int v = -1;
    if (L >= 0 && L < K && g >= 0) {
        float best;
        v = g | BOOT_CELL.pack(L, first_largest(probs + i * K, K, &best));
    }
    info[i] = v;
}

// positions of an order, padded to whole sweep chunks
static long boot_padded(long M) { return (long)ceil_div(M, BOOT_CHUNK) * BOOT_CHUNK; }

// key of row j in order c: column c of probs, or u for c == K; a row that never enters is padding
__device__ __forceinline__ uint32_t boot_key(const float* __restrict__ probs, const float* __restrict__ u, const int32_t* __restrict__ info,
                                             long j, int K, int c) {
    if (info[j] < 0) return RC_KEY_PAD;
    return rc_key(c < K ? probs[j * K + c] : u[j]);
}

// grid (gx, gy, orders); rank [orders][M] is zero
__global__ __launch_bounds__(256) void boot_rank_kernel(const float* __restrict__ probs, const float* __restrict__ u,
                                                        const int32_t* __restrict__ info, long M, int K, RankGeom g,
                                                        int32_t* __restrict__ rank) {
    const int c = blockIdx.z;
    const long i = (long)blockIdx.x * RANK_TILE + threadIdx.x;
    const auto key = [&](long j) { return boot_key(probs, u, info, j, K, c); };
    const uint32_t ki = i < M ? key(i) : RC_KEY_PAD;
    const int cnt = rank_count_chunk(key, ki, M, g.chunk);
    if (ki != RC_KEY_PAD && cnt) atomicAdd(&rank[(long)c * M + i], cnt);
}

// grid (gx, orders); og [orders][Mp] is BOOT_EMPTY everywhere
__global__ __launch_bounds__(256) void boot_scatter_kernel(const float* __restrict__ probs, const float* __restrict__ u,
                                                           const int32_t* __restrict__ info, long M, int K, long Mp,
                                                           const int32_t* __restrict__ rank, uint32_t* __restrict__ og,
                                                           uint32_t* __restrict__ skey) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    if (i >= M) return;
    const int v = info[i];
    if (v < 0) return;
    const uint32_t key = boot_key(probs, u, info, i, K, c);
    const int L = BOOT_CELL.label(v), P = BOOT_CELL.pred(v);
    const bool pos = c < K ? L == c : L != P;
    const long r = rank[(long)c * M + i];  // < the number of rows that enter <= M
    og[(long)c * Mp + r] = ((uint32_t)v & BOOT_GID) | (pos ? BOOT_POS : 0u) | (c == K && key == RC_KEY_NAN ? BOOT_NAN : 0u);
    skey[(long)c * Mp + r] = key;
}

__global__ __launch_bounds__(256) void boot_ties_kernel(long M, long Mp, uint32_t* __restrict__ og, const uint32_t* __restrict__ skey) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    const long at = (long)blockIdx.y * Mp + p;
    if (p >= M || og[at] == BOOT_EMPTY) return;
    if (p == 0 || skey[at] != skey[at - 1]) og[at] |= BOOT_TIE;
}

// ---- the replicates ----------------------------------------------------------------------------------------------------------------------
struct BootArgs {
    const int32_t* info;
    const uint32_t* og;
    int32_t* slots;
    long M, Mp, G;
    int K, orders, B;
    uint32_t k0, k1;
    double* stats;
    int64_t *cm, *u2, *n_pos, *n_neg;
};

struct BootWave {  // a wave's summary of one chunk
    unsigned long long tot, snap;
    int flag;
};

// One order of one replicate.  Returns (block-wide) sum_{pos} w Nlt - sum_{neg} w Plt; AURC: *risk = the sum of 1 - acc[m] over the
// expanded rows (negatives are the right predictions), *nan_seen set when a row with weight has the NAN mark.
template <bool LDSC, bool AURC>
__device__ __forceinline__ long long boot_sweep(const uint32_t* __restrict__ og, long Mp, const uint32_t* s_cnt, const int32_t* cg,
                                                BootWave (*s_ws)[4], long long* s_red, double* s_redd, double* risk, int* nan_seen) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long carry = 0ull, carry_snap = 0ull;  // (negative | positive << 32) weight before the chunk / before its open tie run
    long long S = 0;
    double dsum = 0.0;
    int par = 0;
    for (long c0 = 0; c0 < Mp; c0 += BOOT_CHUNK, par ^= 1) {
        const uint4* src = reinterpret_cast<const uint4*>(og + c0 + (long)tid * BOOT_E);
        const uint4 a = src[0], b = src[1];
        const uint32_t word[BOOT_E] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint32_t w[BOOT_E];
        unsigned long long tot = 0ull, rel_snap = 0ull;
        int hf = 0;
#pragma unroll
        for (int e = 0; e < BOOT_E; ++e) {
            w[e] = word[e] == BOOT_EMPTY ? 0u : (LDSC ? boot_count_lds(s_cnt, word[e] & BOOT_GID) : boot_count_global(cg, word[e] & BOOT_GID));
            if (word[e] & BOOT_TIE) {
                hf = 1;
                rel_snap = tot;
            }
            tot += (word[e] & BOOT_POS) ? (unsigned long long)w[e] << 32 : (unsigned long long)w[e];
        }
        const unsigned long long inc = wave_scan_incl(tot);
        const unsigned long long ex_w = inc - tot;
        unsigned long long ps = ex_w + rel_snap;  // the latest tie start at or before this thread's last position, relative to the wave
        int pf = hf;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long s = __shfl_up(ps, o);
            const int f = __shfl_up(pf, o);
            if (lane >= o && !pf) {
                ps = s;
                pf = f;
            }
        }
        unsigned long long in_s = __shfl_up(ps, 1);
        int in_f = __shfl_up(pf, 1);
        if (lane == 0) in_f = 0;
        if (lane == 63) {
            s_ws[par][wave].tot = inc;
            s_ws[par][wave].snap = ps;
            s_ws[par][wave].flag = pf;
        }
        __syncthreads();  // (the table of the chunk before is free again once every wave has passed this barrier)
        unsigned long long off = carry, snap = carry_snap, woff = carry, wsnap = carry_snap;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const BootWave t = s_ws[par][v];
            if (t.flag) snap = off + t.snap;
            off += t.tot;
            if (v + 1 == wave) {
                woff = off;
                wsnap = snap;
            }
        }
        if (wave == 0) {
            woff = carry;
            wsnap = carry_snap;
        }
        carry = off;
        carry_snap = snap;
        unsigned long long run = woff + ex_w, cur = in_f ? woff + in_s : wsnap;
#pragma unroll
        for (int e = 0; e < BOOT_E; ++e) {
            if (word[e] & BOOT_TIE) cur = run;
            const bool pos = (word[e] & BOOT_POS) != 0u;
            if (w[e]) {
                if (pos) S += (long long)w[e] * (long long)(cur & 0xFFFFFFFFull);
                else S -= (long long)w[e] * (long long)(cur >> 32);
                if (AURC) {
                    if (word[e] & BOOT_NAN) *nan_seen = 1;
                    const long long C = (long long)(run & 0xFFFFFFFFull), T = C + (long long)(run >> 32);
                    for (uint32_t t = 1; t <= w[e]; ++t) dsum += 1.0 - (double)(C + (pos ? 0 : (long long)t)) / (double)(T + t);
                }
            }
            run += pos ? (unsigned long long)w[e] << 32 : (unsigned long long)w[e];
        }
    }
    if (AURC) {  // the tree of block_sum_fixed, written out: the call costs boot_metrics_kernel<true> five VGPRs (profiles/README.md)
        for (int o = 32; o > 0; o >>= 1) dsum += __shfl_xor(dsum, o);
        __syncthreads();
        if (lane == 0) s_redd[wave] = dsum;
        __syncthreads();
        *risk = (s_redd[0] + s_redd[1]) + (s_redd[2] + s_redd[3]);
    }
    return block_sum_i64(S, s_red);
}

template <bool LDSC>
__global__ __launch_bounds__(BOOT_NT) void boot_metrics_kernel(BootArgs a) {
#pragma clang fp contract(off)
    extern __shared__ uint32_t boot_lds[];
    __shared__ uint32_t s_cm[EVAL_MAX_K * EVAL_MAX_K];
    __shared__ BootWave s_ws[2][4];
    __shared__ long long s_red[4];
    __shared__ double s_redd[4];
    __shared__ long long s_s[EVAL_MAX_K + 1];
    __shared__ int s_nan;
    const int tid = threadIdx.x, K = a.K;
    int32_t* cg = LDSC ? nullptr : a.slots + (long)blockIdx.x * a.G;
    for (int b = blockIdx.x; b <= a.B; b += gridDim.x) {
        __syncthreads();  // the replicate before is finished with the counts and the tables
        if (LDSC) boot_draw_lds(boot_lds, (int)a.G, (uint32_t)b, a.k0, a.k1, b == a.B);
        else boot_draw_global(cg, a.G, (uint32_t)b, a.k0, a.k1, b == a.B);
        if (tid < K * K) s_cm[tid] = 0u;
        if (tid == 0) s_nan = 0;
        __syncthreads();
        for (long i = tid; i < a.M; i += BOOT_NT) {
            const int v = a.info[i];
            if (v < 0) continue;
            const uint32_t w = LDSC ? boot_count_lds(boot_lds, v & BOOT_GID) : boot_count_global(cg, v & BOOT_GID);
            if (w) atomicAdd(&s_cm[BOOT_CELL.label(v) * K + BOOT_CELL.pred(v)], w);
        }
        __syncthreads();
        double risk = 0.0;
        for (int c = 0; c < a.orders; ++c) {
            const uint32_t* og = a.og + (long)c * a.Mp;
            const long long s = c < K ? boot_sweep<LDSC, false>(og, a.Mp, boot_lds, cg, s_ws, s_red, s_redd, nullptr, nullptr)
                                      : boot_sweep<LDSC, true>(og, a.Mp, boot_lds, cg, s_ws, s_red, s_redd, &risk, &s_nan);
            if (tid == 0) s_s[c] = s;
        }
        __syncthreads();
        if (tid != 0) continue;
        long long W = 0;
        for (int e = 0; e < K * K; ++e) {
            W += s_cm[e];
            a.cm[(long)b * K * K + e] = s_cm[e];
        }
        ClassTally tally;
        double num = 0.0, den = 0.0;
        bool defined = true;
        for (int k = 0; k < K; ++k) {
            long long sup = 0, prd = 0;
            for (int j = 0; j < K; ++j) {
                sup += s_cm[k * K + j];
                prd += s_cm[j * K + k];
            }
            const long long tp = s_cm[k * K + k], nneg = W - sup, u2 = sup * nneg + s_s[k];
            tally.add(tp, sup, prd);
            a.u2[(long)b * K + k] = u2;
            a.n_pos[(long)b * K + k] = sup;
            a.n_neg[(long)b * K + k] = nneg;
            if (sup > 0 && nneg > 0) {
                num += (double)sup * ((double)u2 / (2.0 * (double)sup * (double)nneg));
                den += (double)sup;
            } else {
                defined = false;  // a class the replicate lost: no AUC, and a 0 would poison the interval
            }
        }
        const double nan = __builtin_nan("");
        double* st = a.stats + (long)b * 6;
        st[0] = tally.accuracy(W);
        st[1] = tally.balanced_accuracy();
        st[2] = tally.f1_mean(K);
        st[3] = defined ? num / den : nan;
        st[4] = nan;
        st[5] = nan;
        if (a.orders > K) {
            const long long trace = tally.trace, wrong = W - trace;
            st[4] = W > 0 ? risk / (double)W : nan;
            if (!s_nan && wrong > 0 && trace > 0) st[5] = (double)(wrong * trace + s_s[K]) / (2.0 * (double)wrong * (double)trace);
        }
    }
}

struct BootWorkspace {
    uint32_t *og, *skey;
    int32_t *rank, *gid, *info, *slots;
    int nslots;
    size_t bytes;
};

static BootWorkspace boot_workspace(void* ws, long M, long G, int K, int B) {
    BootWorkspace w;
    Carve c{static_cast<char*>(ws)};
    const size_t orders = (size_t)K + 1, Mp = (size_t)boot_padded(M);
    w.og = c.take<uint32_t>(orders * Mp);
    w.skey = c.take<uint32_t>(orders * Mp);
    w.rank = c.take<int32_t>(orders * M);
    w.gid = c.take<int32_t>((size_t)M);
    w.info = c.take<int32_t>((size_t)M);
    w.nslots = boot_slots(G, B);
    w.slots = c.take<int32_t>((size_t)w.nslots * G);
    w.bytes = c.used;
    return w;
}

static bool boot_sizes_ok(long M, long G, int K, int B) {
    return K >= 2 && K <= EVAL_MAX_K && M >= 1 && M <= EVAL_MAX_ROWS && G >= 1 && G <= M && B >= 1 && B <= EVAL_MAX_REPLICATES;
}

}  // namespace pasn

using namespace pasn;

extern "C" int pasn_bootstrap_lds_max_groups(void) { return BOOT_LDS_MAX_G; }

extern "C" int pasn_bootstrap_counts(int32_t* counts, long G, int B, uint64_t seed, int b0, void* stream) {
    PASN_REQUIRE(counts, "counts is required");
    PASN_REQUIRE(G >= 1 && G <= EVAL_MAX_ROWS, "G must lie in [1, 2^20]");
    PASN_REQUIRE(B >= 1 && B <= EVAL_MAX_REPLICATES, "B must lie in [1, 65536]");
    PASN_REQUIRE(b0 >= 0 && (long)b0 + B <= (1L << 31) - 1, "b0 must not be negative, and b0 + B must fit an int32");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
    if (G <= BOOT_LDS_MAX_G) {
        hipLaunchKernelGGL(boot_counts_lds_kernel, dim3(B), dim3(BOOT_NT), (size_t)((G + 1) / 2) * sizeof(uint32_t), s, counts, (int)G, B, k0, k1, b0);
    } else {
        if (hipMemsetAsync(counts, 0, (size_t)B * G * sizeof(int32_t), s) != hipSuccess) return check_launch("bootstrap_counts (zeroing)");
        hipLaunchKernelGGL(boot_counts_global_kernel, dim3(ceil_div((G + 3) / 4, BOOT_NT), std::min(B, 4096)), dim3(BOOT_NT), 0, s, counts, G, B, k0,
                           k1, b0);
    }
    return check_launch("bootstrap_counts");
}

extern "C" size_t pasn_bootstrap_workspace_bytes(long M, long G, int K_real, int B) {
    if (!boot_sizes_ok(M, G, K_real, B)) return 0;
    return boot_workspace(nullptr, M, G, K_real, B).bytes;
}

extern "C" int pasn_bootstrap_metrics(const float* probs, const int32_t* labels, const float* u, const int64_t* group_offsets,
                                      const int32_t* group_rows, long M, long G, int K_real, int B, uint64_t seed, double* stats, int64_t* cm,
                                      int64_t* u2, int64_t* n_pos, int64_t* n_neg, void* workspace, void* stream) {
    PASN_REQUIRE(probs && labels, "probs and labels are required");
    PASN_REQUIRE(stats && cm && u2 && n_pos && n_neg, "every output is required");
    PASN_REQUIRE(workspace, "workspace is required");
    PASN_REQUIRE((group_offsets == nullptr) == (group_rows == nullptr), "group_offsets and group_rows come together");
    PASN_REQUIRE(K_real >= 2 && K_real <= EVAL_MAX_K, "K_real must lie in [2, 16]");
    PASN_REQUIRE(M >= 1 && M <= EVAL_MAX_ROWS, "M must lie in [1, 2^20]");
    PASN_REQUIRE(G >= 1 && G <= M, "G must lie in [1, M]");
    PASN_REQUIRE(group_offsets || G == M, "without groups every row is its own group: G must equal M");
    PASN_REQUIRE(B >= 1 && B <= EVAL_MAX_REPLICATES, "B must lie in [1, 65536]");
    PASN_REQUIRE(((uintptr_t)workspace & 15) == 0, "misaligned workspace");
    const RankGeom g = rank_geom(M);
    const long Mp = boot_padded(M);
    const BootWorkspace w = boot_workspace(workspace, M, G, K_real, B);
    const int orders = u ? K_real + 1 : K_real;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(w.og, 0xFF, (size_t)orders * Mp * sizeof(uint32_t), s) != hipSuccess ||
        hipMemsetAsync(w.rank, 0, (size_t)orders * M * sizeof(int32_t), s) != hipSuccess ||
        (group_offsets && hipMemsetAsync(w.gid, 0xFF, (size_t)M * sizeof(int32_t), s) != hipSuccess))
        return check_launch("bootstrap_metrics (zeroing)");
    if (group_offsets) hipLaunchKernelGGL(boot_gid_kernel, dim3(ceil_div(G, 4)), dim3(256), 0, s, group_offsets, group_rows, G, M, w.gid);
    hipLaunchKernelGGL(boot_info_kernel, dim3(g.gx), dim3(256), 0, s, probs, labels, group_offsets ? w.gid : nullptr, M, K_real, w.info);
    hipLaunchKernelGGL(boot_rank_kernel, dim3(g.gx, g.gy, orders), dim3(256), 0, s, probs, u, w.info, M, K_real, g, w.rank);
    hipLaunchKernelGGL(boot_scatter_kernel, dim3(g.gx, orders), dim3(256), 0, s, probs, u, w.info, M, K_real, Mp, w.rank, w.og, w.skey);
    hipLaunchKernelGGL(boot_ties_kernel, dim3(g.gx, orders), dim3(256), 0, s, M, Mp, w.og, w.skey);
    BootArgs a;
    a.info = w.info;
    a.og = w.og;
    a.slots = w.slots;
    a.M = M;
    a.Mp = Mp;
    a.G = G;
    a.K = K_real;
    a.orders = orders;
    a.B = B;
    a.k0 = (uint32_t)(seed & 0xffffffffull);
    a.k1 = (uint32_t)(seed >> 32);
    a.stats = stats;
    a.cm = cm;
    a.u2 = u2;
    a.n_pos = n_pos;
    a.n_neg = n_neg;
    if (w.nslots == 0)
        hipLaunchKernelGGL(boot_metrics_kernel<true>, dim3(B + 1), dim3(BOOT_NT), (size_t)((G + 1) / 2) * sizeof(uint32_t), s, a);
    else
        hipLaunchKernelGGL(boot_metrics_kernel<false>, dim3(w.nslots), dim3(BOOT_NT), 0, s, a);
    return check_launch("bootstrap_metrics");
}
