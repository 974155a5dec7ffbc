// ordinal.hip -- the evaluation that uses the ORDER of the classes (class index = grade): the agreement statistics of a confusion matrix
// (mean absolute grade error, within-one accuracy, under- / over-grading, linear and quadratic weighted kappa) and, for every cut
// "grade >= c" of the scale, its ROC and precision-recall areas and operating points, for the sample and for grouped-bootstrap replicates
// of it.  include/protoasnet_amd.h holds the definitions, tests/ordinal_cases.py their float64 / int64 restatement.
//
// pasn_ordinal_agreement: a thread per confusion matrix; every statistic one fp64 expression of integer sums.
// pasn_ordinal_confusion: the confusion matrix of the rows (LDS histogram per block, 64-bit global integer atomics into the zeroed output).
//
// pasn_ordinal_screen has the shape of pasn_bootstrap_metrics.  What all replicates share is computed once, in five launches:
//   1. gid: the group of every listed row (a wave per group), -1 for the others
//   2. info: per row (group | label << 20), negative for a row that never enters; and the K - 1 cut scores of the row
//   3. rank: rank_count_chunk of order_key.h for every cut (ASCENDING score)
//   4. scatter: per cut and position the word (group | POS) and the key of the score; POS marks label >= c
//   5. marks: TIE on the first position of every run of equal keys and on the position behind the last row (the END: an empty position
//      that closes the last run); FIX on every position at which a caller-given threshold is crossed (key(theta) lies above the key
//      before and not above the key here)
// and one launch does the replicates, a block each (replicate B is the point estimate: every count 1), with the draws of boot_draw.h.
// The block adds the label histogram (P and N of every cut), and sweeps every cut in chunks of 2048 positions, eight per thread.  A
// block-wide scan of the (negative, positive) weight packed in 64 bits gives each position the weights BELOW it (`run`), a second scan
// carries the prefix AT THE START OF ITS TIE RUN forward (`cur`): the weights with a strictly smaller score, so TP = P - cur.pos and
// FP = N - cur.neg are the tallies of the threshold "this row's score".  From that single pass:
//   U2      P N + sum_{i pos} w_i Nlt_i - sum_{j neg} w_j Plt_j, as in bootstrap.hip
//   ap      at every TIE mark the run before it is closed: its positive weight is run.pos - cur.pos; a run with positive weight adds its
//           term.  Each thread adds its terms in position order, the threads in the tree of block_sum_fixed
//   sens    the closed run is the answer when its TP meets the target and the TP behind it (P - run.pos: that of the next candidate,
//           or 0 for +inf) does not: exactly one run per target, a plain LDS store
//   spec    a row with weight whose Nlt meets the target offers (position << 32 | Plt) and (position << 32 | Nlt) to two 64-bit LDS
//           atomicMin; a thread offers once per target (its later rows lie higher)
//   youden  every row with weight is a candidate; thread-local best, then a block reduce on (J, position)
//   fixed   the thread that meets a FIX mark finds which thresholds cross there and stores `run`
// The targets are turned into integer needs first (the smallest x with (double)x / (double)N >= tau), so the sweep compares integers.
#include "boot_draw.h"
#include "common.h"
#include "eval_common.h"

namespace pasn {

constexpr int ORD_NT = BOOT_NT, ORD_E = 8, ORD_CHUNK = ORD_NT * ORD_E;
constexpr int ORD_MAX_T = PASN_ORDINAL_MAX_TARGETS, ORD_MAX_F = PASN_ORDINAL_MAX_FIXED;
constexpr uint32_t ORD_TIE = 1u << 31, ORD_POS = 1u << 30, ORD_FIX = 1u << 29, ORD_EMPTY = 1u << 28, ORD_GID = 0xFFFFFu;
constexpr int ORD_EMPTY_BYTE = 0x10;  // memset value: ORD_EMPTY and no mark
constexpr uint32_t ORD_INF_POS = 0xFFFFFFFFu;  // the position of the candidate +inf
constexpr int ORD_LBIT = 20;

// the float whose key this is (-0 comes back as +0)
__device__ __forceinline__ float ord_key_score(uint32_t key) { return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key); }

// s_c = p[c] + p[c + 1] + ... + p[K - 1], fp32, added in that order
__device__ __forceinline__ float ord_cut_score(const float* __restrict__ p, int K, int c) {
    float s = p[c];
    for (int k = c + 1; k < K; ++k) s += p[k];
    return s;
}

// ---- agreement ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void ord_agreement_kernel(const int64_t* __restrict__ cm, long R, int K, double* __restrict__ out) {
#pragma clang fp contract(off)
    const long r = (long)blockIdx.x * 64 + threadIdx.x;
    if (r >= R) return;
    const int64_t* m = cm + r * K * K;
    long long row[EVAL_MAX_K], col[EVAL_MAX_K];
#pragma unroll
    for (int i = 0; i < EVAL_MAX_K; ++i) row[i] = col[i] = 0;
    long long n = 0, s_abs = 0, s_w1 = 0, s_under = 0, s_over = 0, s_sq = 0;
#pragma unroll
    for (int i = 0; i < EVAL_MAX_K; ++i)
#pragma unroll
        for (int j = 0; j < EVAL_MAX_K; ++j)
            if (i < K && j < K) {
                const long long v = m[i * K + j];
                const int d = i > j ? i - j : j - i;
                row[i] += v;
                col[j] += v;
                n += v;
                s_abs += d * v;
                s_sq += d * d * v;
                if (d <= 1) s_w1 += v;
                if (j < i) s_under += v;
                if (j > i) s_over += v;
            }
    long long e_abs = 0, e_sq = 0;
#pragma unroll
    for (int i = 0; i < EVAL_MAX_K; ++i)
#pragma unroll
        for (int j = 0; j < EVAL_MAX_K; ++j)
            if (i < K && j < K) {
                const int d = i > j ? i - j : j - i;
                const long long rc = row[i] * col[j];
                e_abs += d * rc;
                e_sq += d * d * rc;
            }
    const double nan = __builtin_nan(""), dn = (double)n;
    double* o = out + r * 6;
    if (n <= 0) {
        for (int q = 0; q < 6; ++q) o[q] = nan;
        return;
    }
    o[0] = (double)s_abs / dn;
    o[1] = (double)s_w1 / dn;
    o[2] = (double)s_under / dn;
    o[3] = (double)s_over / dn;
    o[4] = e_abs != 0 ? 1.0 - (dn * (double)s_abs) / (double)e_abs : nan;
    o[5] = e_sq != 0 ? 1.0 - (dn * (double)s_sq) / (double)e_sq : nan;
}

// cm [K][K] is zero
__global__ __launch_bounds__(256) void ord_confusion_kernel(const float* __restrict__ probs, const int32_t* __restrict__ labels, long M, int K,
                                                            unsigned long long* __restrict__ cm) {
    __shared__ uint32_t s_cm[EVAL_MAX_K * EVAL_MAX_K];
    const int tid = threadIdx.x;
    s_cm[tid] = 0u;
    __syncthreads();
    for (long i = (long)blockIdx.x * 256 + tid; i < M; i += (long)gridDim.x * 256) {
        const int L = labels[i];
        if (L < 0 || L >= K) continue;
        float best;
        atomicAdd(&s_cm[L * K + first_largest(probs + i * K, K, &best)], 1u);
    }
    __syncthreads();
    if (tid < K * K && s_cm[tid]) atomicAdd(&cm[tid], (unsigned long long)s_cm[tid]);
}

__global__ __launch_bounds__(256) void ord_cut_scores_kernel(const float* __restrict__ probs, long M, int K, float* __restrict__ scores) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    for (int c = 1; c < K; ++c) scores[(long)(c - 1) * M + i] = ord_cut_score(probs + i * K, K, c);
}

// ---- what the replicates share -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ord_gid_kernel(const int64_t* __restrict__ offs, const int32_t* __restrict__ rows, long G, long M,
                                                      int32_t* __restrict__ gid) {
    const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= G) return;
    const int64_t lo = offs[g], hi = offs[g + 1];
    for (int64_t r = lo + (threadIdx.x & 63); r < hi; r += 64) {
        const long i = rows[r];
        if (i >= 0 && i < M) gid[i] = (int32_t)g;
    }
}

__global__ __launch_bounds__(256) void ord_info_kernel(const float* __restrict__ probs, const int32_t* __restrict__ labels,
                                                       const int32_t* __restrict__ gid, long M, int K, int32_t* __restrict__ info,
                                                       float* __restrict__ scores) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const int L = labels[i];
    const int g = gid ? gid[i] : (int)i;
    const bool in = L >= 0 && L < K && g >= 0;
    info[i] = in ? (g | (L << ORD_LBIT)) : -1;
    for (int c = 1; c < K; ++c) scores[(long)(c - 1) * M + i] = ord_cut_score(probs + i * K, K, c);
}

static long ord_padded(long M) { return (long)ceil_div(M + 1, ORD_CHUNK) * ORD_CHUNK; }  // + 1: the END position

// grid (gx, gy, cuts); rank [cuts][M] is zero
__global__ __launch_bounds__(256) void ord_rank_kernel(const float* __restrict__ scores, const int32_t* __restrict__ info, long M, RankGeom g,
                                                       int32_t* __restrict__ rank) {
    const int c = blockIdx.z;
    const long i = (long)blockIdx.x * RANK_TILE + threadIdx.x;
    const auto key = [&](long j) { return info[j] < 0 ? RC_KEY_PAD : rc_key(scores[(long)c * M + j]); };
    const uint32_t ki = i < M ? key(i) : RC_KEY_PAD;
    const int cnt = rank_count_chunk(key, ki, M, g.chunk);
    if (ki != RC_KEY_PAD && cnt) atomicAdd(&rank[(long)c * M + i], cnt);
}

// grid (gx, cuts); og [cuts][Mp] is ORD_EMPTY everywhere, skey RC_KEY_PAD
__global__ __launch_bounds__(256) void ord_scatter_kernel(const float* __restrict__ scores, const int32_t* __restrict__ info, long M, long Mp,
                                                          const int32_t* __restrict__ rank, uint32_t* __restrict__ og,
                                                          uint32_t* __restrict__ skey) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    if (i >= M) return;
    const int v = info[i];
    if (v < 0) return;
    const long r = rank[(long)c * M + i];  // < the number of rows that enter <= M
    og[(long)c * Mp + r] = ((uint32_t)v & ORD_GID) | ((v >> ORD_LBIT) > c ? ORD_POS : 0u);
    skey[(long)c * Mp + r] = rc_key(scores[(long)c * M + i]);
}

// does the threshold with key kt cross at a position with key kp whose predecessor has key kprev (first: no predecessor)?
__device__ __forceinline__ bool ord_crosses(uint32_t kt, uint32_t kprev, uint32_t kp, bool first) { return (first || kt > kprev) && kt <= kp; }

// grid (blocks over M + 1 positions, cuts); fixed [cuts][F] fp32
__global__ __launch_bounds__(256) void ord_marks_kernel(long M, long Mp, uint32_t* __restrict__ og, const uint32_t* __restrict__ skey,
                                                        const float* __restrict__ fixed, int F) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    const long at = (long)c * Mp + p;
    if (p > M) return;
    const uint32_t kp = skey[at], kprev = p > 0 ? skey[at - 1] : 0u;
    if (kp == RC_KEY_PAD && p > 0 && kprev == RC_KEY_PAD) return;  // behind the END
    uint32_t mark = (p == 0 || kp != kprev) ? ORD_TIE : 0u;
    if (mark)
        for (int f = 0; f < F; ++f)
            if (ord_crosses(rc_key(fixed[c * F + f]), kprev, kp, p == 0)) mark |= ORD_FIX;
    if (mark) og[at] |= mark;
}

// ---- the replicates ----------------------------------------------------------------------------------------------------------------------
struct OrdArgs {
    const int32_t* info;
    const uint32_t *og, *skey;
    const float* fixed;
    int32_t* slots;
    long M, Mp, G;
    int K, B, n_spec, n_sens, F;
    uint32_t k0, k1;
    double target[2 * ORD_MAX_T];  // specificities, then sensitivities
    int64_t *pn, *u2, *op_tally, *fix_tally;
    double* stats;
    float* op_theta;
};

struct OrdWave {  // a wave's summary of one chunk
    unsigned long long tot, snap;
    int flag;
};

struct OrdCut {  // one cut of one replicate, in LDS
    uint32_t P, N, ok;
    uint32_t need[2 * ORD_MAX_T];               // integer needs of the targets
    uint32_t need_spec_lo, need_sens_lo, need_sens_hi;
    uint32_t kfix[ORD_MAX_F];                   // keys of the fixed thresholds
    unsigned long long spec_p[ORD_MAX_T], spec_n[ORD_MAX_T];  // position << 32 | Plt, position << 32 | Nlt (atomicMin)
    unsigned long long sens_cur[ORD_MAX_T], fix_run[ORD_MAX_F];
    uint32_t sens_pos[ORD_MAX_T];
    long long yj[4];  // Youden: a wave's best
    unsigned long long ycur[4];
    uint32_t ypos[4];
};

// the smallest x in [1, n] with (double)x / (double)n >= tau (0 < tau < 1, n >= 1): the quotient is monotone in x
__device__ __forceinline__ uint32_t ord_need(double tau, uint32_t n) {
#pragma clang fp contract(off)
    const double dn = (double)n;
    long long x = (long long)(tau * dn);
    if (x < 1) x = 1;
    if (x > (long long)n) x = n;
    while (x > 1 && (double)(x - 1) / dn >= tau) --x;
    while (x < (long long)n && (double)x / dn < tau) ++x;
    return (uint32_t)x;
}

// One cut of one replicate.  s_cut holds P, N, the needs and the keys of the fixed thresholds on entry, and the answers on return.
template <bool LDSC>
__device__ __forceinline__ void ord_sweep(const uint32_t* __restrict__ og, const uint32_t* __restrict__ skey, long Mp, const uint32_t* s_cnt,
                                          const int32_t* cg, OrdWave (*s_ws)[4], long long* s_red, double* s_redd, OrdCut* s_cut, int n_spec,
                                          int n_sens, int F, long long* u2_rest, double* ap) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long P = s_cut->P, N = s_cut->N;
    const bool ok = s_cut->ok != 0u;
    const double dP = (double)P;
    uint32_t spec_lo = ok && n_spec ? s_cut->need_spec_lo : 0xFFFFFFFFu, spec_done = 0u;
    const uint32_t sens_lo = s_cut->need_sens_lo, sens_hi = ok && n_sens ? s_cut->need_sens_hi : 0u;
    unsigned long long carry = 0ull, carry_snap = 0ull;  // (negative | positive << 32) weight before the chunk / before its open tie run
    long long S = 0, yj = 0;
    unsigned long long ycur = ((unsigned long long)P << 32) | (unsigned long long)N;  // +inf: nobody positive
    uint32_t ypos = ORD_INF_POS;
    double dsum = 0.0;
    int par = 0;
    for (long c0 = 0; c0 < Mp; c0 += ORD_CHUNK, par ^= 1) {
        const long base = c0 + (long)tid * ORD_E;
        const uint4* src = reinterpret_cast<const uint4*>(og + base);
        const uint4 a = src[0], b = src[1];
        const uint32_t word[ORD_E] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint32_t w[ORD_E];
        unsigned long long tot = 0ull, rel_snap = 0ull;
        int hf = 0;
#pragma unroll
        for (int e = 0; e < ORD_E; ++e) {
            w[e] = (word[e] & ORD_EMPTY) ? 0u : (LDSC ? boot_count_lds(s_cnt, word[e] & ORD_GID) : boot_count_global(cg, word[e] & ORD_GID));
            if (word[e] & ORD_TIE) {
                hf = 1;
                rel_snap = tot;
            }
            tot += (word[e] & ORD_POS) ? (unsigned long long)w[e] << 32 : (unsigned long long)w[e];
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
            const OrdWave t = s_ws[par][v];
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
        for (int e = 0; e < ORD_E; ++e) {
            const uint32_t wd = word[e];
            if (wd & ORD_TIE) {
                if (run != cur) {  // close the run [cur, run): it has weight
                    const long long tpv = (long long)(run >> 32) - (long long)(cur >> 32);
                    const long long TP = P - (long long)(cur >> 32), FP = N - (long long)(cur & 0xFFFFFFFFull);
                    const long long TPn = P - (long long)(run >> 32);
                    if (ok && tpv > 0) dsum += ((double)tpv / dP) * ((double)TP / (double)(TP + FP));
                    if (TPn < (long long)sens_hi && TP >= (long long)sens_lo)
                        for (int t = 0; t < n_sens; ++t) {
                            const long long need = s_cut->need[ORD_MAX_T + t];
                            if (TP >= need && TPn < need) {
                                s_cut->sens_pos[t] = (uint32_t)(base + e - 1);  // the last position of the closed run
                                s_cut->sens_cur[t] = cur;
                            }
                        }
                }
                cur = run;
                if (wd & ORD_FIX) {
                    const long p = base + e;
                    const uint32_t kp = skey[p], kprev = p > 0 ? skey[p - 1] : 0u;
                    for (int f = 0; f < F; ++f)
                        if (ord_crosses(s_cut->kfix[f], kprev, kp, p == 0)) s_cut->fix_run[f] = run;
                }
            }
            const bool pos = (wd & ORD_POS) != 0u;
            if (w[e]) {
                const long long plt = (long long)(cur >> 32), nlt = (long long)(cur & 0xFFFFFFFFull);
                if (pos) S += (long long)w[e] * nlt;
                else S -= (long long)w[e] * plt;
                if (ok) {
                    const long long J = (P - plt) * N - (N - nlt) * P;
                    if (J >= yj) {  // a later position has the larger score; +inf (J = 0) gives way to a positive J only
                        if (J > yj || ypos != ORD_INF_POS) {
                            yj = J;
                            ycur = cur;
                            ypos = (uint32_t)(base + e);
                        }
                    }
                    if ((uint32_t)nlt >= spec_lo) {
                        uint32_t lo = 0xFFFFFFFFu;
                        for (int t = 0; t < n_spec; ++t) {
                            if ((spec_done >> t) & 1u) continue;
                            const uint32_t need = s_cut->need[t];
                            if ((uint32_t)nlt >= need) {
                                const unsigned long long hi = (unsigned long long)(uint32_t)(base + e) << 32;
                                atomicMin(&s_cut->spec_p[t], hi | (unsigned long long)plt);
                                atomicMin(&s_cut->spec_n[t], hi | (unsigned long long)nlt);
                                spec_done |= 1u << t;
                            } else if (need < lo) {
                                lo = need;
                            }
                        }
                        spec_lo = lo;
                    }
                }
            }
            run += pos ? (unsigned long long)w[e] << 32 : (unsigned long long)w[e];
        }
    }
    // Youden: the best (J, position) of the block; equal J: the larger position (ORD_INF_POS is the largest)
    for (int o = 32; o > 0; o >>= 1) {
        const long long oj = __shfl_xor(yj, o);
        const unsigned long long oc = __shfl_xor(ycur, o);
        const uint32_t op = __shfl_xor(ypos, o);
        if (oj > yj || (oj == yj && op > ypos)) {
            yj = oj;
            ycur = oc;
            ypos = op;
        }
    }
    *ap = block_sum_fixed(dsum, s_redd);
    if (lane == 0) {
        s_cut->yj[wave] = yj;
        s_cut->ycur[wave] = ycur;
        s_cut->ypos[wave] = ypos;
    }
    *u2_rest = block_sum_i64(S, s_red);  // (its barriers publish the Youden table and every LDS answer of the sweep)
}

template <bool LDSC>
__global__ __launch_bounds__(ORD_NT) void ord_screen_kernel(OrdArgs a) {
#pragma clang fp contract(off)
    extern __shared__ uint32_t ord_lds[];
    __shared__ uint32_t s_hist[EVAL_MAX_K];
    __shared__ OrdWave s_ws[2][4];
    __shared__ long long s_red[4];
    __shared__ double s_redd[4];
    __shared__ OrdCut s_cut;
    const int tid = threadIdx.x, K = a.K, C = K - 1, T = a.n_spec + a.n_sens + 1, F = a.F;
    int32_t* cg = LDSC ? nullptr : a.slots + (long)blockIdx.x * a.G;
    const float nanf_ = __builtin_nanf("");
    for (int b = blockIdx.x; b <= a.B; b += gridDim.x) {
        __syncthreads();  // the replicate before is finished with the counts and the tables
        if (LDSC) boot_draw_lds(ord_lds, (int)a.G, (uint32_t)b, a.k0, a.k1, b == a.B);
        else boot_draw_global(cg, a.G, (uint32_t)b, a.k0, a.k1, b == a.B);
        if (tid < EVAL_MAX_K) s_hist[tid] = 0u;
        __syncthreads();
        for (long i = tid; i < a.M; i += ORD_NT) {
            const int v = a.info[i];
            if (v < 0) continue;
            const uint32_t w = LDSC ? boot_count_lds(ord_lds, v & ORD_GID) : boot_count_global(cg, v & ORD_GID);
            if (w) atomicAdd(&s_hist[(v >> ORD_LBIT) & (EVAL_MAX_K - 1)], w);
        }
        __syncthreads();
        for (int c = 0; c < C; ++c) {
            // ---- the cut's totals, needs and empty answers
            uint32_t P = 0u, N = 0u;
            for (int k = 0; k < K; ++k) {
                if (k > c) P += s_hist[k];
                else N += s_hist[k];
            }
            const bool ok = P > 0u && N > 0u;
            __syncthreads();  // the cut before has been written out
            if (tid == 0) {
                s_cut.P = P;
                s_cut.N = N;
                s_cut.ok = ok ? 1u : 0u;
            }
            if (tid < a.n_spec) {
                s_cut.need[tid] = ok ? ord_need(a.target[tid], N) : 0u;
                s_cut.spec_p[tid] = ((unsigned long long)ORD_INF_POS << 32) | P;  // +inf: Plt = P, Nlt = N
                s_cut.spec_n[tid] = ((unsigned long long)ORD_INF_POS << 32) | N;
            }
            if (tid < a.n_sens) {
                s_cut.need[ORD_MAX_T + tid] = ok ? ord_need(a.target[ORD_MAX_T + tid], P) : 0u;
                s_cut.sens_pos[tid] = ORD_INF_POS;
                s_cut.sens_cur[tid] = ((unsigned long long)P << 32) | N;
            }
            if (tid < F) {
                s_cut.kfix[tid] = rc_key(a.fixed[c * F + tid]);
                s_cut.fix_run[tid] = ((unsigned long long)P << 32) | N;
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t lo = 0xFFFFFFFFu, slo = 0xFFFFFFFFu, shi = 0u;
                for (int t = 0; t < a.n_spec; ++t) lo = min(lo, s_cut.need[t]);
                for (int t = 0; t < a.n_sens; ++t) {
                    slo = min(slo, s_cut.need[ORD_MAX_T + t]);
                    shi = max(shi, s_cut.need[ORD_MAX_T + t]);
                }
                s_cut.need_spec_lo = lo;
                s_cut.need_sens_lo = slo;
                s_cut.need_sens_hi = shi;
            }
            __syncthreads();
            long long rest;
            double ap;
            ord_sweep<LDSC>(a.og + (long)c * a.Mp, a.skey + (long)c * a.Mp, a.Mp, ord_lds, cg, s_ws, s_red, s_redd, &s_cut, a.n_spec, a.n_sens, F,
                            &rest, &ap);
            // ---- write the cut out
            const long rc = (long)b * C + c;
            const uint32_t* skey = a.skey + (long)c * a.Mp;
            if (tid == 0) {
                const long long u2 = (long long)P * (long long)N + rest;
                a.pn[rc * 2 + 0] = P;
                a.pn[rc * 2 + 1] = N;
                a.u2[rc] = u2;
                const double nan = __builtin_nan("");
                a.stats[rc * 2 + 0] = ok ? (double)u2 / (2.0 * (double)P * (double)N) : nan;
                a.stats[rc * 2 + 1] = ok ? ap : nan;
            }
            if (tid < T) {
                uint32_t pos = ORD_INF_POS;
                unsigned long long cur = ((unsigned long long)P << 32) | N;
                if (tid < a.n_spec) {
                    pos = (uint32_t)(s_cut.spec_p[tid] >> 32);
                    cur = ((s_cut.spec_p[tid] & 0xFFFFFFFFull) << 32) | (s_cut.spec_n[tid] & 0xFFFFFFFFull);
                } else if (tid < a.n_spec + a.n_sens) {
                    pos = s_cut.sens_pos[tid - a.n_spec];
                    cur = s_cut.sens_cur[tid - a.n_spec];
                } else {
                    long long yj = s_cut.yj[0];
                    pos = s_cut.ypos[0];
                    cur = s_cut.ycur[0];
                    for (int v = 1; v < 4; ++v)
                        if (s_cut.yj[v] > yj || (s_cut.yj[v] == yj && s_cut.ypos[v] > pos)) {
                            yj = s_cut.yj[v];
                            pos = s_cut.ypos[v];
                            cur = s_cut.ycur[v];
                        }
                }
                const long o = rc * T + tid;
                a.op_theta[o] = !ok ? nanf_ : pos == ORD_INF_POS ? __builtin_inff() : ord_key_score(skey[pos]);
                a.op_tally[o * 2 + 0] = ok ? (long long)P - (long long)(cur >> 32) : 0;
                a.op_tally[o * 2 + 1] = ok ? (long long)N - (long long)(cur & 0xFFFFFFFFull) : 0;
            }
            if (tid < F) {
                const unsigned long long run = s_cut.fix_run[tid];
                const long o = rc * F + tid;
                a.fix_tally[o * 2 + 0] = (long long)P - (long long)(run >> 32);
                a.fix_tally[o * 2 + 1] = (long long)N - (long long)(run & 0xFFFFFFFFull);
            }
        }
    }
}

struct OrdWorkspace {
    uint32_t *og, *skey;
    float* scores;
    int32_t *rank, *gid, *info, *slots;
    int nslots;
    size_t bytes;
};

static OrdWorkspace ord_workspace(void* ws, long M, long G, int K, int B) {
    OrdWorkspace w;
    Carve c{static_cast<char*>(ws)};
    const size_t cuts = (size_t)K - 1, Mp = (size_t)ord_padded(M);
    w.og = c.take<uint32_t>(cuts * Mp, 16);
    w.skey = c.take<uint32_t>(cuts * Mp, 16);
    w.scores = c.take<float>(cuts * M);
    w.rank = c.take<int32_t>(cuts * M);
    w.gid = c.take<int32_t>((size_t)M);
    w.info = c.take<int32_t>((size_t)M);
    w.nslots = boot_slots(G, B);
    w.slots = c.take<int32_t>((size_t)w.nslots * G);
    w.bytes = c.used;
    return w;
}

static bool ord_sizes_ok(long M, long G, int K, int B) {
    return K >= 2 && K <= EVAL_MAX_K && M >= 1 && M <= EVAL_MAX_ROWS && G >= 1 && G <= M && B >= 0 && B <= EVAL_MAX_REPLICATES;
}

}  // namespace pasn

using namespace pasn;

extern "C" int pasn_ordinal_agreement(const int64_t* cm, long R, int K_real, double* out, void* stream) {
    PASN_REQUIRE(cm && out, "cm and out are required");
    PASN_REQUIRE(K_real >= 2 && K_real <= EVAL_MAX_K, "K_real must lie in [2, 16]");
    PASN_REQUIRE(R >= 1 && R <= EVAL_MAX_REPLICATES + 1, "R must lie in [1, 65537]");
    hipLaunchKernelGGL(ord_agreement_kernel, dim3(ceil_div(R, 64)), dim3(64), 0, (hipStream_t)stream, cm, R, K_real, out);
    return check_launch("ordinal_agreement");
}

extern "C" int pasn_ordinal_confusion(const float* probs, const int32_t* labels, long M, int K_real, int64_t* cm, void* stream) {
    PASN_REQUIRE(probs && labels && cm, "probs, labels and cm are required");
    PASN_REQUIRE(K_real >= 2 && K_real <= EVAL_MAX_K, "K_real must lie in [2, 16]");
    PASN_REQUIRE(M >= 1 && M <= EVAL_MAX_ROWS, "M must lie in [1, 2^20]");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(cm, 0, (size_t)K_real * K_real * sizeof(int64_t), s) != hipSuccess) return check_launch("ordinal_confusion (zeroing)");
    hipLaunchKernelGGL(ord_confusion_kernel, dim3(std::min(ceil_div(M, 256), 1024)), dim3(256), 0, s, probs, labels, M, K_real,
                       reinterpret_cast<unsigned long long*>(cm));
    return check_launch("ordinal_confusion");
}

extern "C" int pasn_ordinal_cut_scores(const float* probs, long M, int K_real, float* scores, void* stream) {
    PASN_REQUIRE(probs && scores, "probs and scores are required");
    PASN_REQUIRE(K_real >= 2 && K_real <= EVAL_MAX_K, "K_real must lie in [2, 16]");
    PASN_REQUIRE(M >= 1 && M <= EVAL_MAX_ROWS, "M must lie in [1, 2^20]");
    hipLaunchKernelGGL(ord_cut_scores_kernel, dim3(ceil_div(M, 256)), dim3(256), 0, (hipStream_t)stream, probs, M, K_real, scores);
    return check_launch("ordinal_cut_scores");
}

extern "C" size_t pasn_ordinal_workspace_bytes(long M, long G, int K_real, int B) {
    if (!ord_sizes_ok(M, G, K_real, B)) return 0;
    return ord_workspace(nullptr, M, G, K_real, B).bytes;
}

extern "C" int pasn_ordinal_screen(const float* probs, const int32_t* labels, const int64_t* group_offsets, const int32_t* group_rows, long M,
                                   long G, int K_real, int B, uint64_t seed, const double* specificities, int n_spec,
                                   const double* sensitivities, int n_sens, const float* fixed, int n_fixed, int64_t* pn, int64_t* u2,
                                   double* stats, float* op_theta, int64_t* op_tally, int64_t* fix_tally, void* workspace, void* stream) {
    PASN_REQUIRE(probs && labels, "probs and labels are required");
    PASN_REQUIRE(pn && u2 && stats && op_theta && op_tally, "every output is required");
    PASN_REQUIRE(workspace, "workspace is required");
    PASN_REQUIRE((group_offsets == nullptr) == (group_rows == nullptr), "group_offsets and group_rows come together");
    PASN_REQUIRE(K_real >= 2 && K_real <= EVAL_MAX_K, "K_real must lie in [2, 16]");
    PASN_REQUIRE(M >= 1 && M <= EVAL_MAX_ROWS, "M must lie in [1, 2^20]");
    PASN_REQUIRE(G >= 1 && G <= M, "G must lie in [1, M]");
    PASN_REQUIRE(group_offsets || G == M, "without groups every row is its own group: G must equal M");
    PASN_REQUIRE(B >= 0 && B <= EVAL_MAX_REPLICATES, "B must lie in [0, 65536]");
    PASN_REQUIRE(n_spec >= 0 && n_spec <= ORD_MAX_T && (n_spec == 0 || specificities), "n_spec must lie in [0, 8], with its targets");
    PASN_REQUIRE(n_sens >= 0 && n_sens <= ORD_MAX_T && (n_sens == 0 || sensitivities), "n_sens must lie in [0, 8], with its targets");
    PASN_REQUIRE(n_fixed >= 0 && n_fixed <= ORD_MAX_F && (n_fixed == 0 || (fixed && fix_tally)),
                 "n_fixed must lie in [0, 32], with its thresholds and tallies");
    for (int t = 0; t < n_spec; ++t) PASN_REQUIRE(specificities[t] > 0.0 && specificities[t] < 1.0, "every specificity must lie in (0, 1)");
    for (int t = 0; t < n_sens; ++t) PASN_REQUIRE(sensitivities[t] > 0.0 && sensitivities[t] < 1.0, "every sensitivity must lie in (0, 1)");
    PASN_REQUIRE(((uintptr_t)workspace & 15) == 0, "misaligned workspace");
    const RankGeom g = rank_geom(M);
    const long Mp = ord_padded(M);
    const int cuts = K_real - 1;
    const OrdWorkspace w = ord_workspace(workspace, M, G, K_real, B);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(w.og, ORD_EMPTY_BYTE, (size_t)cuts * Mp * sizeof(uint32_t), s) != hipSuccess ||
        hipMemsetAsync(w.skey, 0xFF, (size_t)cuts * Mp * sizeof(uint32_t), s) != hipSuccess ||
        hipMemsetAsync(w.rank, 0, (size_t)cuts * M * sizeof(int32_t), s) != hipSuccess ||
        (group_offsets && hipMemsetAsync(w.gid, 0xFF, (size_t)M * sizeof(int32_t), s) != hipSuccess))
        return check_launch("ordinal_screen (zeroing)");
    if (group_offsets) hipLaunchKernelGGL(ord_gid_kernel, dim3(ceil_div(G, 4)), dim3(256), 0, s, group_offsets, group_rows, G, M, w.gid);
    hipLaunchKernelGGL(ord_info_kernel, dim3(g.gx), dim3(256), 0, s, probs, labels, group_offsets ? w.gid : nullptr, M, K_real, w.info, w.scores);
    hipLaunchKernelGGL(ord_rank_kernel, dim3(g.gx, g.gy, cuts), dim3(256), 0, s, w.scores, w.info, M, g, w.rank);
    hipLaunchKernelGGL(ord_scatter_kernel, dim3(g.gx, cuts), dim3(256), 0, s, w.scores, w.info, M, Mp, w.rank, w.og, w.skey);
    hipLaunchKernelGGL(ord_marks_kernel, dim3(ceil_div(M + 1, 256), cuts), dim3(256), 0, s, M, Mp, w.og, w.skey, fixed, n_fixed);
    OrdArgs a;
    a.info = w.info;
    a.og = w.og;
    a.skey = w.skey;
    a.fixed = fixed;
    a.slots = w.slots;
    a.M = M;
    a.Mp = Mp;
    a.G = G;
    a.K = K_real;
    a.B = B;
    a.n_spec = n_spec;
    a.n_sens = n_sens;
    a.F = n_fixed;
    a.k0 = (uint32_t)(seed & 0xffffffffull);
    a.k1 = (uint32_t)(seed >> 32);
    for (int t = 0; t < ORD_MAX_T; ++t) {
        a.target[t] = t < n_spec ? specificities[t] : 0.5;
        a.target[ORD_MAX_T + t] = t < n_sens ? sensitivities[t] : 0.5;
    }
    a.pn = pn;
    a.u2 = u2;
    a.op_tally = op_tally;
    a.fix_tally = fix_tally;
    a.stats = stats;
    a.op_theta = op_theta;
    if (w.nslots == 0)
        hipLaunchKernelGGL(ord_screen_kernel<true>, dim3(B + 1), dim3(ORD_NT), (size_t)((G + 1) / 2) * sizeof(uint32_t), s, a);
    else
        hipLaunchKernelGGL(ord_screen_kernel<false>, dim3(w.nslots), dim3(ORD_NT), 0, s, a);
    return check_launch("ordinal_screen");
}
