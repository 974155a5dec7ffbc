// prune.hip -- prototype pruning: the tallies of "the model without prototype p" for every p from ONE sweep's similarities, and a greedy
// elimination loop that never reads back.  include/protoasnet_amd.h holds the definitions, tests/prune_cases.py their float64 / int64
// restatement.
//
// prune_pass_kernel: one wave per chunk of PRUNE_CHUNK consecutive rows, lanes over candidates (lane l owns prototypes l, l + 64, ...), the
// rows walked in order -- which is the fixed order of the margin sums, whatever the grid.  A row's K_real logits live in lanes 0 .. K_real - 1
// (those lanes load z, subtract the prototype the round before removed and store it back: every row is owned by one wave, so the pass that
// tallies round r also applies removal r - 1) and are broadcast by lane reads.  The last layer sits in LDS as it is ([k][p]: lanes read
// consecutive words), the per-class error counts in LDS words that only their candidate's lane touches (dynamic LDS, sized by P and K_real).  A chunk ends with one fp64
// partial per candidate to the workspace and integer atomics for the counts.  The building launch first forms z: a lane per row, j
// ascending, fp64 without contraction.
//
// prune_select_kernel: one block.  Thread p adds candidate p's chunk partials in ascending chunk order (eight loads in flight), thread 0
// scans the P keys in index order (strict improvement: equal keys keep the lower index), applies the acceptance test, records the round
// and clears the counts for the next pass.  A refused round sets a flag in the workspace; the launches after it return at once.
#include <cmath>

#include "common.h"
#include "eval_common.h"

namespace pasn {

constexpr int PRUNE_CHUNK = 128, PRUNE_MAX_P = PASN_PRUNE_MAX_P, PRUNE_SLOTS = PRUNE_MAX_P / 64, PRUNE_SEL_NT = 256;
enum { PRUNE_BUILD = 0, PRUNE_ROUND = 1, PRUNE_APPLY = 2 };

struct PruneState {
    int stop, pad;
    long long wrong0;
    double margin0;
};

struct PruneWorkspace {
    unsigned long long* acc;  // [P + 1][2 + K_real]: wrong, flips, wrong per class; row P: the model as it stands
    PruneState* st;
    double* part;             // [chunks][P + 1]
    size_t zero_bytes, bytes;
};

static PruneWorkspace prune_workspace(void* ws, long M, int P, int Kr) {
    PruneWorkspace w;
    Carve c{static_cast<char*>(ws)};
    w.acc = c.take<unsigned long long>((size_t)(P + 1) * (2 + Kr), 16);
    w.st = c.take<PruneState>(1, 16);
    w.zero_bytes = (c.used + 15) / 16 * 16;
    c.used = w.zero_bytes;
    w.part = c.take<double>((size_t)ceil_div(M, PRUNE_CHUNK) * (P + 1), 16);
    w.bytes = (c.used + 15) / 16 * 16;
    return w;
}

struct PruneArgs {
    const float *sim, *w;
    const int32_t *labels, *proto_class, *floor;
    long M;
    int P, Kr, mode, round;  // pass `round` applies removed[round - 1]; select `round` fills removed[round] (-1: the table only)
    int accept, use_margin;
    long long max_extra;
    double margin_fraction;
    double* z;
    long long* table_i;
    double* table_m;
    int32_t* removed;
    long long* trace_i;
    double* trace_m;
    int32_t* kept;
    PruneWorkspace ws;
};

// The tallies of one row for one logit vector: zb[k] - wp[k * P] * sv (sv = 0: the model as it stands; the product is exact, the
// difference one rounding).  Returns the prediction -- the first largest --, *margin = v[y] - max_{k != y} v[k].
__device__ __forceinline__ int prune_row(const double (&zb)[EVAL_MAX_K], const float* wp, int P, double sv, int Kr, int y, double* margin) {
#pragma clang fp contract(off)
    double best = 0.0, zy = 0.0, other = -INFINITY;
    int pred = 0;
#pragma unroll
    for (int k = 0; k < EVAL_MAX_K; ++k)
        if (k < Kr) {
            const double prod = (double)wp[k * P] * sv;
            const double v = zb[k] - prod;
            if (k == 0 || v > best) {
                best = v;
                pred = k;
            }
            if (k == y) zy = v;
            else other = v > other ? v : other;
        }
    *margin = zy - other;
    return pred;
}

static size_t prune_pass_lds(int P, int Kr) { return ((size_t)Kr * P + (size_t)(P + 1) * Kr) * 4; }  // at most 32 832 B

__global__ __launch_bounds__(64) void prune_pass_kernel(PruneArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];  // prune_pass_lds(P, K_real) bytes: sized by the call, not by the limits
    const int lane = threadIdx.x, P = a.P, Kr = a.Kr, mode = a.mode, W = 2 + Kr;
    float* s_w = reinterpret_cast<float*>(s_dyn);                 // [K_real][P]
    uint32_t* s_cls = reinterpret_cast<uint32_t*>(s_w + Kr * P);  // [P + 1][K_real]
    int rm = -1;
    if (mode != PRUNE_BUILD) {
        if (a.ws.st->stop) return;
        rm = a.removed[a.round - 1];
        if (rm < 0) return;
    }
    const long n0 = (long)blockIdx.x * PRUNE_CHUNK, n1 = min(a.M, n0 + PRUNE_CHUNK);
    for (int e = lane; e < Kr * P; e += 64) s_w[e] = a.w[e];  // rows 0 .. K_real - 1 of fc_w [K][P]
    for (int e = lane; e < (P + 1) * Kr; e += 64) s_cls[e] = 0u;
    if (mode == PRUNE_BUILD && blockIdx.x == 0)
        for (int p = lane; p < P; p += 64) a.kept[p] = 1;
    __syncthreads();

    if (mode == PRUNE_BUILD) {
        for (long n = n0 + lane; n < n1; n += 64) {
            const float* s = a.sim + n * P;
            double acc[EVAL_MAX_K];
#pragma unroll
            for (int k = 0; k < EVAL_MAX_K; ++k) acc[k] = 0.0;
            for (int j = 0; j < P; ++j) {
                const double sv = (double)s[j];
#pragma unroll
                for (int k = 0; k < EVAL_MAX_K; ++k)
                    if (k < Kr) {
                        const double prod = (double)s_w[k * P + j] * sv;
                        acc[k] = acc[k] + prod;
                    }
            }
#pragma unroll
            for (int k = 0; k < EVAL_MAX_K; ++k)
                if (k < Kr) a.z[n * Kr + k] = acc[k];
        }
        __syncthreads();  // (with its fence: the rows below are read by other lanes of this wave)
    }

    bool kp[PRUNE_SLOTS];
#pragma unroll
    for (int c = 0; c < PRUNE_SLOTS; ++c) {
        const int p = lane + 64 * c;
        kp[c] = p < P && mode != PRUNE_APPLY && (mode == PRUNE_BUILD || a.kept[p] != 0);
    }
    double ms[PRUNE_SLOTS], bms = 0.0;
    int fl[PRUNE_SLOTS];
#pragma unroll
    for (int c = 0; c < PRUNE_SLOTS; ++c) {
        ms[c] = 0.0;
        fl[c] = 0;
    }
    const double wrm = (rm >= 0 && lane < Kr) ? (double)s_w[lane * P + rm] : 0.0;
    for (long n = n0; n < n1; ++n) {
        const float* s = a.sim + n * P;
        double zk = 0.0;
        if (lane < Kr) {
            zk = a.z[n * Kr + lane];
            if (rm >= 0) {
                const double prod = wrm * (double)s[rm];
                zk = zk - prod;
                a.z[n * Kr + lane] = zk;
            }
        }
        if (mode == PRUNE_APPLY) continue;
        const int y = a.labels[n];
        if (y < 0 || y >= Kr) continue;
        double zb[EVAL_MAX_K];
#pragma unroll
        for (int k = 0; k < EVAL_MAX_K; ++k) zb[k] = k < Kr ? __shfl(zk, k) : 0.0;
        double mg;
        const int bpred = prune_row(zb, s_w, P, 0.0, Kr, y, &mg);
        bms = bms + mg;
        if (lane == 0 && bpred != y) ++s_cls[P * Kr + y];
#pragma unroll
        for (int c = 0; c < PRUNE_SLOTS; ++c)
            if (kp[c]) {
                const int p = lane + 64 * c;
                const int pred = prune_row(zb, s_w + p, P, (double)s[p], Kr, y, &mg);
                ms[c] = ms[c] + mg;
                if (pred != y) ++s_cls[p * Kr + y];
                if (pred != bpred) ++fl[c];
            }
    }
    if (mode == PRUNE_APPLY) return;

    double* part = a.ws.part + (size_t)blockIdx.x * (P + 1);
#pragma unroll
    for (int c = 0; c < PRUNE_SLOTS; ++c) {
        const int p = lane + 64 * c;
        if (p < P) part[p] = kp[c] ? ms[c] : 0.0;
        if (kp[c]) {
            unsigned long long wrong = 0ull;
            for (int k = 0; k < Kr; ++k) {
                const unsigned long long cnt = s_cls[p * Kr + k];
                if (cnt) atomicAdd(&a.ws.acc[(size_t)p * W + 2 + k], cnt);
                wrong += cnt;
            }
            if (wrong) atomicAdd(&a.ws.acc[(size_t)p * W], wrong);
            if (fl[c]) atomicAdd(&a.ws.acc[(size_t)p * W + 1], (unsigned long long)fl[c]);
        }
    }
    if (lane == 0) {
        part[P] = bms;
        unsigned long long wrong = 0ull;
        for (int k = 0; k < Kr; ++k) {
            const unsigned long long cnt = s_cls[P * Kr + k];
            if (cnt) atomicAdd(&a.ws.acc[(size_t)P * W + 2 + k], cnt);
            wrong += cnt;
        }
        if (wrong) atomicAdd(&a.ws.acc[(size_t)P * W], wrong);
    }
}

// Sum of pp[b * stride], b = 0 .. rows - 1, from 0.0 IN INDEX ORDER, eight loads in flight.
__device__ __forceinline__ double prune_sum_chunks(const double* pp, int rows, long stride) {
#pragma clang fp contract(off)
    double sum = 0.0;
    for (int b = 0; b < rows; b += 8) {
        double t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] = pp[(long)min(b + e, rows - 1) * stride];
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (b + e < rows) sum = sum + t[e];
    }
    return sum;
}

__global__ __launch_bounds__(PRUNE_SEL_NT) void prune_select_kernel(PruneArgs a) {
#pragma clang fp contract(off)
    __shared__ double s_m[PRUNE_MAX_P + 1];
    __shared__ int s_cnt[EVAL_MAX_K];
    const int tid = threadIdx.x, P = a.P, Kr = a.Kr, W = 2 + Kr, r = a.round;
    const int chunks = (int)((a.M + PRUNE_CHUNK - 1) / PRUNE_CHUNK);
    PruneState* st = a.ws.st;
    long long* acc = reinterpret_cast<long long*>(a.ws.acc);
    if (r > 0 && st->stop) {  // a no-op round: the model as it stood
        if (tid == 0) {
            a.removed[r] = -1;
            a.trace_m[r] = a.trace_m[r - 1];
        }
        if (tid <= Kr) a.trace_i[(long)r * (1 + Kr) + tid] = a.trace_i[(long)(r - 1) * (1 + Kr) + tid];
        return;
    }
    for (int p = tid; p <= P; p += PRUNE_SEL_NT) {
        // after round 0 only the rows a round can read: the kept prototypes of a real class, and the model as it stands
        const bool dead = r > 0 && p < P && (a.kept[p] == 0 || a.proto_class[p] < 0 || a.proto_class[p] >= Kr);
        const double m = dead ? 0.0 : prune_sum_chunks(a.ws.part + p, chunks, P + 1);
        s_m[p] = m;
        if (r <= 0) {
            a.table_m[p] = m;
            for (int e = 0; e < W; ++e) a.table_i[(long)p * W + e] = acc[(long)p * W + e];
        }
    }
    if (tid < EVAL_MAX_K) s_cnt[tid] = 0;
    __syncthreads();
    if (r < 0) return;
    if (tid < P && a.kept[tid] != 0) {
        const int c = a.proto_class[tid];
        if (c >= 0 && c < Kr) atomicAdd(&s_cnt[c], 1);
    }
    __syncthreads();
    if (tid == 0) {
        if (r == 0) {
            st->wrong0 = acc[(long)P * W];
            st->margin0 = s_m[P];
        }
        int best = -1;
        long long bw = 0;
        double bm = 0.0;
        for (int p = 0; p < P; ++p) {
            if (a.kept[p] == 0) continue;
            const int c = a.proto_class[p];
            if (c < 0 || c >= Kr || s_cnt[c] <= a.floor[c]) continue;
            const long long w = acc[(long)p * W];
            const double m = s_m[p];
            if (best < 0 || w < bw || (w == bw && m > bm)) {
                best = p;
                bw = w;
                bm = m;
            }
        }
        bool ok = best >= 0;
        if (ok && a.accept) {
            ok = bw <= st->wrong0 + a.max_extra;
            if (ok && a.use_margin) {
                const double need = a.margin_fraction * st->margin0;
                ok = bm >= need;
            }
        }
        const int src = ok ? best : P;
        a.removed[r] = ok ? best : -1;
        a.trace_m[r] = s_m[src];
        a.trace_i[(long)r * (1 + Kr)] = acc[(long)src * W];
        for (int k = 0; k < Kr; ++k) a.trace_i[(long)r * (1 + Kr) + 1 + k] = acc[(long)src * W + 2 + k];
        if (ok) a.kept[best] = 0;
        else st->stop = 1;
    }
    __syncthreads();
    for (int e = tid; e < (P + 1) * W; e += PRUNE_SEL_NT) acc[e] = 0;  // for the next pass
}

static bool prune_sizes_ok(long M, int P, int Kr) {
    return M >= 1 && M <= PASN_PRUNE_MAX_ROWS && P >= 1 && P <= PRUNE_MAX_P && Kr >= 2 && Kr <= EVAL_MAX_K;
}

}  // namespace pasn

using namespace pasn;

extern "C" int pasn_prune_chunk(void) { return PRUNE_CHUNK; }

extern "C" size_t pasn_prune_workspace_bytes(long M, int P, int K_real) {
    if (!prune_sizes_ok(M, P, K_real)) return 0;
    return prune_workspace(nullptr, M, P, K_real).bytes;
}

extern "C" int pasn_prune_eliminate(const float* sim, const float* fc_w, const int32_t* labels, const int32_t* proto_class, const int32_t* floor,
                                    long M, int P, int K, int K_real, int rounds, int accept, int64_t max_extra_errors, int use_margin,
                                    double margin_fraction, double* z, int64_t* table_i, double* table_m, int32_t* removed, int64_t* trace_i,
                                    double* trace_m, int32_t* kept, void* workspace, void* stream) {
    PASN_REQUIRE(sim && fc_w && labels && proto_class, "sim, fc_w, labels and proto_class are required");
    PASN_REQUIRE(z && table_i && table_m && kept, "z, table_i, table_m and kept are required");
    PASN_REQUIRE(workspace, "workspace is required");
    PASN_REQUIRE(M >= 1 && M <= PASN_PRUNE_MAX_ROWS, "M must lie in [1, 2^24]");
    PASN_REQUIRE(P >= 1 && P <= PRUNE_MAX_P, "P must lie in [1, 256]");
    PASN_REQUIRE(K_real >= 2 && K_real <= K && K <= EVAL_MAX_K, "2 <= K_real <= K <= 16 is required");
    PASN_REQUIRE(rounds >= 0 && rounds <= P, "rounds must lie in [0, P]");
    PASN_REQUIRE(rounds == 0 || (floor && removed && trace_i && trace_m), "floor, removed, trace_i and trace_m are required when rounds > 0");
    PASN_REQUIRE(accept == 0 || accept == 1, "accept must be 0 or 1");
    PASN_REQUIRE(use_margin == 0 || use_margin == 1, "use_margin must be 0 or 1");
    PASN_REQUIRE(max_extra_errors >= 0, "max_extra_errors must be >= 0");
    PASN_REQUIRE(!use_margin || std::isfinite(margin_fraction), "margin_fraction must be finite");
    PASN_REQUIRE(((uintptr_t)workspace & 15) == 0, "misaligned workspace");
    hipStream_t s = (hipStream_t)stream;
    PruneArgs a;
    a.sim = sim;
    a.w = fc_w;
    a.labels = labels;
    a.proto_class = proto_class;
    a.floor = floor;
    a.M = M;
    a.P = P;
    a.Kr = K_real;
    a.accept = accept;
    a.use_margin = use_margin;
    a.max_extra = max_extra_errors;
    a.margin_fraction = margin_fraction;
    a.z = z;
    a.table_i = reinterpret_cast<long long*>(table_i);
    a.table_m = table_m;
    a.removed = removed;
    a.trace_i = reinterpret_cast<long long*>(trace_i);
    a.trace_m = trace_m;
    a.kept = kept;
    a.ws = prune_workspace(workspace, M, P, K_real);
    if (hipMemsetAsync(workspace, 0, a.ws.zero_bytes, s) != hipSuccess) return check_launch("prune_eliminate");
    const int chunks = ceil_div(M, PRUNE_CHUNK);
    a.mode = PRUNE_BUILD;
    a.round = 0;
    hipLaunchKernelGGL(prune_pass_kernel, dim3(chunks), dim3(64), prune_pass_lds(P, K_real), s, a);
    if (rounds == 0) {
        a.round = -1;
        hipLaunchKernelGGL(prune_select_kernel, dim3(1), dim3(PRUNE_SEL_NT), 0, s, a);
    }
    for (int r = 0; r < rounds; ++r) {
        a.round = r;
        hipLaunchKernelGGL(prune_select_kernel, dim3(1), dim3(PRUNE_SEL_NT), 0, s, a);
        a.round = r + 1;
        a.mode = r + 1 < rounds ? PRUNE_ROUND : PRUNE_APPLY;
        hipLaunchKernelGGL(prune_pass_kernel, dim3(chunks), dim3(64), prune_pass_lds(P, K_real), s, a);
    }
    return check_launch("prune_eliminate");
}
