// conformal.hip -- split conformal prediction sets: which classes can NOT be ruled out for a row, at a stated error rate?  Scores of
// every (row, class), the calibrated thresholds (one order statistic per stratum and miscoverage level) and the sets with their tallies.
// include/protoasnet_amd.h holds the definitions, tests/conformal_cases.py their float64 / int64 restatement.
//
// pasn_conformal_scores: one thread per row, the row in registers.  The ranking (descending probability, the lower class first on ties) is
// an odd-even transposition network over (probability, class) pairs -- adjacent exchanges on STRICT disorder only, so it is stable and
// the tie rule needs no second comparison; every index is a compile-time constant after unrolling: no private array, no scratch.  Scores
// are fp64 without contraction and rounded once to fp32.
//
// pasn_conformal_quantiles: a byte-wise radix select on rc_key(score), most significant byte first.  Launch p counts, per stratum
// (blockIdx.y) and target, the 256 values of byte 3 - p among the rows that still match the target's prefix: LDS counters, then integer
// atomics into the workspace.  The narrowing between two passes is done by EVERY block of the next launch, redundantly and identically,
// from the histogram the launch before completed (a wave scan over 256 bins): no block waits for another.  A one-block-per-stratum
// finish narrows the last byte and turns the key back into the float.  5 launches and one memset whatever M is; work linear in M.
//
// pasn_conformal_sets: one thread per row, its scores in registers; a mask per level, the tallies in 64-bit LDS counters per block, then
// integer atomics to global memory.
#include <cmath>

#include "common.h"
#include "eval_common.h"
#include "philox.h"

namespace pasn {

constexpr int CONF_NT = 256, CONF_MAX_A = PASN_CONFORMAL_MAX_ALPHAS, CONF_MAX_CHUNKS = 64, CONF_ROWS_PER_BLOCK = 2048, CONF_PASSES = 4;
constexpr int CONF_PAD = -1, CONF_NAN = -2;  // `stratum` of a row that is not valid

// ---- scores ------------------------------------------------------------------------------------------------------------------------------
struct ScoreArgs {
    const float* probs;
    const int32_t* labels;
    long M;
    int K, kind, randomized, k_reg;
    uint32_t seed_lo, seed_hi, salt;
    double lam;
    float *scores, *own;
    int32_t* stratum;
};

__global__ __launch_bounds__(CONF_NT) void conformal_scores_kernel(ScoreArgs a) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * CONF_NT + threadIdx.x;
    if (i >= a.M) return;
    const int K = a.K;
    const float* p = a.probs + i * K;
    float v[EVAL_MAX_K];
    int c[EVAL_MAX_K];
    bool nan = false;
#pragma unroll
    for (int k = 0; k < EVAL_MAX_K; ++k) {
        v[k] = k < K ? p[k] : -INFINITY;  // the tail stays behind every class: exchanges are strict
        c[k] = k;
        nan |= v[k] != v[k];
    }
    const int L = a.labels ? a.labels[i] : 0;
    const bool in_range = L >= 0 && L < K;
    float* out = a.scores + i * K;
    float mine = __builtin_nanf("");
    if (nan) {
#pragma unroll
        for (int k = 0; k < EVAL_MAX_K; ++k)
            if (k < K) out[k] = mine;
    } else if (a.kind == PASN_CONFORMAL_LAC) {
#pragma unroll
        for (int k = 0; k < EVAL_MAX_K; ++k)
            if (k < K) {
                const float s = (float)(1.0 - (double)v[k]);
                out[k] = s;
                if (k == L) mine = s;
            }
    } else {
#pragma unroll
        for (int round = 0; round < EVAL_MAX_K; ++round)
#pragma unroll
            for (int j = round & 1; j + 1 < EVAL_MAX_K; j += 2)
                if (v[j + 1] > v[j]) {
                    const float tv = v[j];
                    v[j] = v[j + 1];
                    v[j + 1] = tv;
                    const int tc = c[j];
                    c[j] = c[j + 1];
                    c[j + 1] = tc;
                }
        double U = 1.0;
        if (a.randomized) {
            uint32_t w[4];
            philox4x32_10((uint32_t)i, (uint32_t)((uint64_t)i >> 32), a.salt, 0u, a.seed_lo, a.seed_hi, w);
            U = (double)w[0] * 0x1p-32;
        }
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < EVAL_MAX_K; ++r)
            if (r < K) {
                const double pk = (double)v[r];
                double s = acc + U * pk;
                if (a.kind == PASN_CONFORMAL_RAPS) s = s + a.lam * (double)max(0, r + 1 - a.k_reg);
                const float sf = (float)s;
                out[c[r]] = sf;
                if (c[r] == L) mine = sf;
                acc = acc + pk;
            }
    }
    if (a.own) {
        const bool valid = in_range && !nan;
        a.own[i] = valid ? mine : __builtin_nanf("");
        a.stratum[i] = valid ? L : (nan ? CONF_NAN : CONF_PAD);
    }
}

// ---- thresholds --------------------------------------------------------------------------------------------------------------------------
struct ConfTarget {
    uint32_t prefix, k;  // the bytes fixed so far; the rank (1-based) among the rows that share them, 0: r > n, the threshold is +inf
};

struct ConfWorkspace {
    uint32_t* hist;     // [CONF_PASSES][S][A][256]; pass 0 counts once for all targets, in slot a = 0
    ConfTarget* state;  // [2][S][A]
    size_t hist_bytes, bytes;
};

static ConfWorkspace conf_workspace(void* ws, int K, int A) {
    ConfWorkspace w;
    Carve c{static_cast<char*>(ws)};
    const size_t S = (size_t)K + 1;
    w.hist = c.take<uint32_t>((size_t)CONF_PASSES * S * A * 256, 16);
    w.hist_bytes = c.used;
    w.state = c.take<ConfTarget>(2 * S * A, 16);
    w.bytes = (c.used + 15) / 16 * 16;
    return w;
}

struct QuantArgs {
    const float* own;
    const int32_t* stratum;
    long M;
    int K, A, pass;  // pass p counts byte 3 - p; pass CONF_PASSES is the finish
    double alphas[CONF_MAX_A];
    ConfWorkspace w;
    float* qhat;
    int64_t *n, *r;
};

// The byte at which target `t` stands after the 256-bin histogram `h` of its current rows: the smallest b whose inclusive count reaches
// t.k.  One wave, every lane in it; lane l holds bins 4l .. 4l + 3.  Returns the narrowed target in every lane.
__device__ __forceinline__ ConfTarget conf_narrow(const uint32_t* __restrict__ h, ConfTarget t) {
    const int lane = threadIdx.x & 63;
    const uint4 c4 = reinterpret_cast<const uint4*>(h)[lane];
    const uint32_t tot = c4.x + c4.y + c4.z + c4.w;
    const uint32_t incl = wave_scan_incl<uint32_t>(tot), excl = incl - tot;
    const bool hit = t.k != 0u && excl < t.k && t.k <= incl;
    const unsigned long long m = __ballot(hit);
    uint32_t b = 0u, k = 0u;
    if (hit) {
        uint32_t run = excl;
        b = 4u * lane;
        k = t.k - run;
        if (k > c4.x) {
            k -= c4.x;
            ++b;
            if (k > c4.y) {
                k -= c4.y;
                ++b;
                if (k > c4.z) {
                    k -= c4.z;
                    ++b;
                }
            }
        }
    }
    if (m == 0ull) return ConfTarget{t.prefix, 0u};  // (t.k == 0, or past the rows: +inf)
    const int src = __ffsll((long long)m) - 1;
    return ConfTarget{(t.prefix << 8) | (uint32_t)__shfl((int)b, src), (uint32_t)__shfl((int)k, src)};
}

// The targets of stratum s as launch `pass` needs them (into s_t[A]): launch 1 forms n and r from the first histogram, the later ones
// advance the state the launch before left.  Block x == 0 keeps the new state (and, in launch 1, n and r) for its successor.
__device__ __forceinline__ void conf_advance(const QuantArgs& a, int s, ConfTarget* s_t) {
#pragma clang fp contract(off)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, S = a.K + 1, A = a.A, pass = a.pass;
    const uint32_t* hist = a.w.hist + (size_t)(pass - 1) * S * A * 256 + (size_t)s * A * 256;
    for (int t = wave; t < A; t += CONF_NT / 64) {
        ConfTarget cur;
        if (pass == 1) {
            const uint4 c4 = reinterpret_cast<const uint4*>(hist)[lane];
            uint32_t n = c4.x + c4.y + c4.z + c4.w;
            for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
            const double rd = ceil((double)((long long)n + 1) * (1.0 - a.alphas[t]));
            const long long r = (long long)rd;
            cur = ConfTarget{0u, r > (long long)n ? 0u : (uint32_t)r};
            if (blockIdx.x == 0 && lane == 0) {
                a.r[(long)s * A + t] = r;
                if (t == 0) a.n[s] = (long long)n;
            }
            cur = conf_narrow(hist, cur);  // every target reads slot 0
        } else {
            cur = a.w.state[((size_t)(pass & 1) * S + s) * A + t];
            cur = conf_narrow(hist + (size_t)t * 256, cur);
        }
        if (lane == 0) {
            s_t[t] = cur;
            if (blockIdx.x == 0 && pass < CONF_PASSES) a.w.state[((size_t)((pass + 1) & 1) * S + s) * A + t] = cur;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(CONF_NT) void conformal_count_kernel(QuantArgs a) {
    __shared__ uint32_t s_cnt[CONF_MAX_A * 256];
    __shared__ ConfTarget s_t[CONF_MAX_A];
    const int tid = threadIdx.x, s = blockIdx.y, A = a.A, pass = a.pass, S = a.K + 1;
    const int slots = pass == 0 ? 1 : A;
    for (int e = tid; e < slots * 256; e += CONF_NT) s_cnt[e] = 0u;
    if (pass > 0) conf_advance(a, s, s_t);  // (ends on a barrier)
    else __syncthreads();
    const int shift = 8 * (3 - pass);
    const long per = (a.M + gridDim.x - 1) / gridDim.x, i0 = (long)blockIdx.x * per, i1 = min(a.M, i0 + per);
    for (long i = i0 + tid; i < i1; i += CONF_NT) {
        const int st = a.stratum[i];
        if (st < 0 || (s > 0 && st != s - 1)) continue;
        const uint32_t key = rc_key(a.own[i]);
        const uint32_t byte = (key >> shift) & 255u;
        if (pass == 0) {
            atomicAdd(&s_cnt[byte], 1u);
        } else {
            const uint32_t head = key >> (shift + 8);
            for (int t = 0; t < A; ++t)
                if (s_t[t].k != 0u && s_t[t].prefix == head) atomicAdd(&s_cnt[t * 256 + byte], 1u);
        }
    }
    __syncthreads();
    uint32_t* hist = a.w.hist + (size_t)pass * S * A * 256 + (size_t)s * A * 256;
    for (int e = tid; e < slots * 256; e += CONF_NT)
        if (s_cnt[e] != 0u) atomicAdd(&hist[e], s_cnt[e]);
}

__global__ __launch_bounds__(CONF_NT) void conformal_finish_kernel(QuantArgs a) {
    __shared__ ConfTarget s_t[CONF_MAX_A];
    const int s = blockIdx.x;  // (one block per stratum: conf_advance's blockIdx.x == 0 writes are guarded by pass < CONF_PASSES)
    conf_advance(a, s, s_t);
    if (threadIdx.x < a.A) {
        const ConfTarget t = s_t[threadIdx.x];
        const uint32_t key = t.prefix;  // all four bytes
        a.qhat[(long)s * a.A + threadIdx.x] = t.k == 0u ? INFINITY : __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
    }
}

// ---- sets --------------------------------------------------------------------------------------------------------------------------------
struct SetsArgs {
    const float *scores, *qhat, *u;
    const int32_t* labels;
    long M;
    int K, A, mondrian;
    uint16_t* masks;
    unsigned long long* tallies;
};

// the tallies of one level: [rows, covered, nan_rows, size_hist, covered_by_size, u_by_size, u_rows_by_size (K + 1 each), class_n, class_covered (K each)]
__host__ __device__ static inline int conf_tally_words(int K) { return 3 + 4 * (K + 1) + 2 * K; }

__global__ __launch_bounds__(CONF_NT) void conformal_sets_kernel(SetsArgs a) {
    __shared__ unsigned long long s_t[CONF_MAX_A * (3 + 4 * (EVAL_MAX_K + 1) + 2 * EVAL_MAX_K)];
    __shared__ float s_q[(EVAL_MAX_K + 1) * CONF_MAX_A];
    const int tid = threadIdx.x, K = a.K, A = a.A, T = conf_tally_words(K);
    for (int e = tid; e < A * T; e += CONF_NT) s_t[e] = 0ull;
    for (int e = tid; e < (K + 1) * A; e += CONF_NT) s_q[e] = a.qhat[e];
    __syncthreads();
    const long i = (long)blockIdx.x * CONF_NT + tid;
    if (i < a.M) {
        float sc[EVAL_MAX_K];
        bool nan = false;
#pragma unroll
        for (int k = 0; k < EVAL_MAX_K; ++k) {
            sc[k] = k < K ? a.scores[i * K + k] : 0.0f;
            nan |= sc[k] != sc[k];
        }
        const int L = a.labels ? a.labels[i] : -1;
        const bool labelled = L >= 0 && L < K, enters = !nan && (labelled || !a.labels);
        bool has_u = false;
        unsigned long long uq = 0ull;
        if (a.u) {
            const float uv = a.u[i];
            has_u = uv >= 0.0f && uv <= 1.0f;
            if (has_u) uq = (unsigned long long)((double)uv * 4294967296.0);
        }
        for (int t = 0; t < A; ++t) {
            unsigned mask = 0u;
#pragma unroll
            for (int k = 0; k < EVAL_MAX_K; ++k)
                if (k < K && sc[k] <= s_q[(a.mondrian ? 1 + k : 0) * A + t]) mask |= 1u << k;  // (a NaN score compares false)
            a.masks[(long)t * a.M + i] = (uint16_t)mask;
            unsigned long long* h = s_t + t * T;
            if (nan) atomicAdd(h + 2, 1ull);
            if (!enters) continue;
            const int size = __popc(mask);
            atomicAdd(h, 1ull);
            atomicAdd(h + 3 + size, 1ull);
            if (has_u) {
                atomicAdd(h + 3 + 2 * (K + 1) + size, uq);
                atomicAdd(h + 3 + 3 * (K + 1) + size, 1ull);
            }
            if (labelled) {
                const bool cov = (mask >> L) & 1u;
                atomicAdd(h + 3 + 4 * (K + 1) + L, 1ull);
                if (cov) {
                    atomicAdd(h + 1, 1ull);
                    atomicAdd(h + 3 + (K + 1) + size, 1ull);
                    atomicAdd(h + 3 + 4 * (K + 1) + K + L, 1ull);
                }
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < A * T; e += CONF_NT)
        if (s_t[e] != 0ull) atomicAdd(&a.tallies[e], s_t[e]);
}

static bool conf_sizes_ok(long M, int K, int A) { return K >= 2 && K <= EVAL_MAX_K && M >= 1 && M <= EVAL_MAX_ROWS && A >= 1 && A <= CONF_MAX_A; }

}  // namespace pasn

using namespace pasn;

extern "C" int pasn_conformal_scores(const float* probs, const int32_t* labels, long M, int K_real, int kind, int randomized, uint64_t seed,
                                     uint32_t salt, double lam, int k_reg, float* scores, float* own, int32_t* stratum, void* stream) {
    PASN_REQUIRE(probs && scores, "probs and scores are required");
    PASN_REQUIRE((labels != nullptr) == (own != nullptr) && (own != nullptr) == (stratum != nullptr),
                 "labels, own and stratum are given together or not at all");
    PASN_REQUIRE(K_real >= 2 && K_real <= EVAL_MAX_K, "K_real must lie in [2, 16]");
    PASN_REQUIRE(M >= 1 && M <= EVAL_MAX_ROWS, "M must lie in [1, 2^20]");
    PASN_REQUIRE(kind >= PASN_CONFORMAL_LAC && kind <= PASN_CONFORMAL_RAPS, "kind must be PASN_CONFORMAL_LAC, _APS or _RAPS");
    PASN_REQUIRE(randomized == 0 || randomized == 1, "randomized must be 0 or 1");
    PASN_REQUIRE(lam >= 0.0 && std::isfinite(lam), "lam must be a finite number >= 0");
    PASN_REQUIRE(k_reg >= 0, "k_reg must be >= 0");
    ScoreArgs a{probs, labels, M, K_real, kind, randomized, k_reg, (uint32_t)seed, (uint32_t)(seed >> 32), salt, lam, scores, own, stratum};
    hipLaunchKernelGGL(conformal_scores_kernel, dim3(ceil_div(M, CONF_NT)), dim3(CONF_NT), 0, (hipStream_t)stream, a);
    return check_launch("conformal_scores");
}

extern "C" size_t pasn_conformal_workspace_bytes(long M, int K_real, int A) {
    if (!conf_sizes_ok(M, K_real, A)) return 0;
    return conf_workspace(nullptr, K_real, A).bytes;
}

extern "C" int pasn_conformal_quantiles(const float* own, const int32_t* stratum, long M, int K_real, int A, const double* alphas, float* qhat,
                                        int64_t* n, int64_t* r, void* workspace, void* stream) {
    PASN_REQUIRE(own && stratum, "own and stratum are required");
    PASN_REQUIRE(alphas, "alphas is required");
    PASN_REQUIRE(qhat && n && r, "every output is required");
    PASN_REQUIRE(workspace, "workspace is required");
    PASN_REQUIRE(K_real >= 2 && K_real <= EVAL_MAX_K, "K_real must lie in [2, 16]");
    PASN_REQUIRE(M >= 1 && M <= EVAL_MAX_ROWS, "M must lie in [1, 2^20]");
    PASN_REQUIRE(A >= 1 && A <= CONF_MAX_A, "A must lie in [1, 8]");
    for (int t = 0; t < A; ++t) PASN_REQUIRE(alphas[t] > 0.0 && alphas[t] < 1.0, "every alpha must lie strictly between 0 and 1");
    PASN_REQUIRE(((uintptr_t)workspace & 15) == 0, "misaligned workspace");
    hipStream_t s = (hipStream_t)stream;
    QuantArgs a;
    a.own = own;
    a.stratum = stratum;
    a.M = M;
    a.K = K_real;
    a.A = A;
    for (int t = 0; t < CONF_MAX_A; ++t) a.alphas[t] = t < A ? alphas[t] : 0.5;
    a.w = conf_workspace(workspace, K_real, A);
    a.qhat = qhat;
    a.n = n;
    a.r = r;
    if (hipMemsetAsync(a.w.hist, 0, a.w.hist_bytes, s) != hipSuccess) return check_launch("conformal_quantiles");
    const int chunks = std::min(ceil_div(M, CONF_ROWS_PER_BLOCK), CONF_MAX_CHUNKS);
    for (a.pass = 0; a.pass < CONF_PASSES; ++a.pass)
        hipLaunchKernelGGL(conformal_count_kernel, dim3(chunks, K_real + 1), dim3(CONF_NT), 0, s, a);
    hipLaunchKernelGGL(conformal_finish_kernel, dim3(K_real + 1), dim3(CONF_NT), 0, s, a);
    return check_launch("conformal_quantiles");
}

extern "C" int pasn_conformal_sets(const float* scores, const float* qhat, const int32_t* labels, const float* u, long M, int K_real, int A,
                                   int mondrian, uint16_t* masks, int64_t* tallies, void* stream) {
    PASN_REQUIRE(scores && qhat, "scores and qhat are required");
    PASN_REQUIRE(masks && tallies, "masks and tallies are required");
    PASN_REQUIRE(K_real >= 2 && K_real <= EVAL_MAX_K, "K_real must lie in [2, 16]");
    PASN_REQUIRE(M >= 1 && M <= EVAL_MAX_ROWS, "M must lie in [1, 2^20]");
    PASN_REQUIRE(A >= 1 && A <= CONF_MAX_A, "A must lie in [1, 8]");
    PASN_REQUIRE(mondrian == 0 || mondrian == 1, "mondrian must be 0 or 1");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(tallies, 0, (size_t)A * conf_tally_words(K_real) * sizeof(int64_t), s) != hipSuccess) return check_launch("conformal_sets");
    SetsArgs a{scores, qhat, u, labels, M, K_real, A, mondrian, masks, reinterpret_cast<unsigned long long*>(tallies)};
    hipLaunchKernelGGL(conformal_sets_kernel, dim3(ceil_div(M, CONF_NT)), dim3(CONF_NT), 0, s, a);
    return check_launch("conformal_sets");
}

extern "C" int pasn_conformal_tally_words(int K_real) { return K_real >= 2 && K_real <= EVAL_MAX_K ? conf_tally_words(K_real) : 0; }
