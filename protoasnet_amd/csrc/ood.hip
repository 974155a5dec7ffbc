// ood.hip -- out-of-distribution detection: does a clip look like anything the model was trained on?  Scores that need no fit (1 - the
// largest prototype similarity, the free energy of the logits), the exact k nearest rows of a bank of training embeddings, the moments
// and scores of class-conditional Gaussians (Mahalanobis), and the flags and tallies of calibrated thresholds.  A HIGHER score means MORE
// out-of-distribution.  include/protoasnet_amd.h holds the definitions, tests/ood_cases.py their numpy restatement.
//
// pasn_ood_knn: d(i, m) = sum_j (q[i][j] - bank[m][j])^2 in fp32, j ascending, every operation rounded on its own -- a function of the two
// rows only, so the tiling below can not show in a bit.  Grid (bank chunks, query tiles).  A 256-thread block holds KNN_QT = 32 queries
// (resident in LDS, transposed, when E <= KNN_QE_MAX; else slab by slab) and streams its chunk of the bank through LDS in tiles of
// KNN_BT = 128 rows, KNN_EJ = 32 coordinates at a time, transposed ([j][row]: one ds_read_b128 gives a lane its four rows), the next
// slab fetched into registers while the current one is used.  A lane owns a
// 4 x 4 query x bank micro-tile and walks j in order.  After the last slab the 32 x 128 distances go to LDS and each wave merges them into
// its eight queries' sorted lists: a list lives one entry per lane, an insert is a ballot, a popcount and a lane shift.  The order is
// total ((d, bank index), NaN never enters), so the k best are the same whatever order the candidates arrive in.  Every block leaves its
// lists in the workspace; knn_finish_kernel (one wave per query) merges the chunks in bank order.  One memset and two launches whatever
// the sizes; no block waits for another; no floating-point atomics anywhere in this file.
//
// pasn_ood_moments: every term of n, sum and scatter is exact in fp64 (an fp32 converts exactly, a product of two has 48 bits), so only the
// order of the additions is free, and it is fixed: chunks of OOD_MOMENT_CHUNK rows summed from 0.0 in row order, the chunk partials added
// in chunk order.  A thread owns one output and walks ALL rows in that order, so there are no partials to store.
#include <cmath>

#include "common.h"
#include "eval_common.h"

#pragma clang fp contract(off)

namespace pasn {

constexpr int OOD_NT = 256;
constexpr int OOD_MAX_E = 1024, OOD_MAX_K = 64, OOD_MAX_P = 4096, OOD_MAX_A = 8, OOD_MAX_ME = 256, OOD_MOMENT_CHUNK = 256;
constexpr long OOD_MAX_Q = 1L << 20, OOD_MAX_B = 1L << 24;
constexpr int KNN_QT = 32, KNN_BT = 128, KNN_EJ = 32, KNN_QE_MAX = 256, KNN_BS = KNN_BT + 4, KNN_MAX_CHUNKS = 64, KNN_TARGET_BLOCKS = 512;
constexpr int KNN_FILL = 0x7fffffff;  // the index of an empty list entry while it is being built: behind every bank row at d = +inf

// ---- scores that need no fit -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OOD_NT) void ood_head_scores_kernel(const float* __restrict__ sim, const float* __restrict__ logits, long M, int P,
                                                                 int K, int K_real, float* maxsim, float* energy) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * OOD_NT + threadIdx.x;
    if (i >= M) return;
    if (maxsim) {
        const float* s = sim + i * P;
        float mx = s[0];
        bool nan = mx != mx;
        for (int p = 1; p < P; ++p) {
            const float v = s[p];
            nan |= v != v;
            if (v > mx) mx = v;
        }
        maxsim[i] = nan ? __builtin_nanf("") : 1.0f - mx;
    }
    if (energy) {
        const float* l = logits + i * K;
        double m = (double)l[0];
        bool nan = m != m;
        for (int k = 1; k < K_real; ++k) {
            const double v = (double)l[k];
            nan |= v != v;
            if (v > m) m = v;
        }
        double s = 0.0;
        for (int k = 0; k < K_real; ++k) s = s + exp((double)l[k] - m);
        energy[i] = nan ? __builtin_nanf("") : (float)(-(m + log(s)));
    }
}

__global__ __launch_bounds__(OOD_NT) void ood_rows_normalize_kernel(const float* x, long M, int E, float* y) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * OOD_NT + threadIdx.x;
    if (i >= M) return;
    const float* r = x + i * E;
    float n2 = 0.0f;
    for (int j = 0; j < E; ++j) {
        const float v = r[j];
        const float sq = v * v;
        n2 = n2 + sq;
    }
    const float nrm = sqrtf(n2);  // (correctly rounded: hipcc's default; __fsqrt_rn is the NATIVE square root here)
    float* o = y + i * E;
    if (n2 == 0.0f) {
        for (int j = 0; j < E; ++j) o[j] = r[j];
    } else {
        for (int j = 0; j < E; ++j) o[j] = __fdiv_rn(r[j], nrm);
    }
}

// ---- k nearest bank rows -----------------------------------------------------------------------------------------------------------------
struct KnnPlan {
    int qtiles, chunks;
    long chunk_rows;  // a multiple of KNN_BT
};

static KnnPlan knn_plan(long Mq, long Mb) {
    KnnPlan p;
    p.qtiles = (int)((Mq + KNN_QT - 1) / KNN_QT);
    const long tiles = (Mb + KNN_BT - 1) / KNN_BT;
    long want = std::max(1L, (long)KNN_TARGET_BLOCKS / p.qtiles);
    want = std::min(std::min(want, tiles), (long)KNN_MAX_CHUNKS);
    const long per = (tiles + want - 1) / want;
    p.chunk_rows = per * KNN_BT;
    p.chunks = (int)((tiles + per - 1) / per);
    return p;
}

struct KnnArgs {
    const float *q, *bank;
    long Mq, Mb, self_base, chunk_rows;
    int E, k, chunks;
    float* ws_d;     // [chunks][Mq][k]
    int32_t* ws_i;   // [chunks][Mq][k]
    float* dist;     // [Mq][k]
    int32_t* index;  // [Mq][k]
    unsigned long long* status;
};

// (d, i) before (e, j) in the list order: ascending distance, the lower bank index first.  A NaN d is before nothing.
__device__ __forceinline__ bool knn_before(float d, int i, float e, int j) { return d < e || (d == e && i < j); }

// One sorted list per wave, entry l in lane l (lanes >= k hold fill and are never read).  Inserts (nd, ni) if it goes before entry k - 1.
__device__ __forceinline__ void knn_insert(float& ed, int& ei, float nd, int ni, int k) {
    const int lane = threadIdx.x & 63;
    const float td = __shfl(ed, k - 1);
    const int ti = __shfl(ei, k - 1);
    if (!knn_before(nd, ni, td, ti)) return;  // (wave-uniform)
    const int pos = __popcll(__ballot(knn_before(ed, ei, nd, ni)));  // the entries before the new one are a prefix
    const float ud = __shfl_up(ed, 1);
    const int ui = __shfl_up(ei, 1);
    if (lane > pos) {
        ed = ud;
        ei = ui;
    } else if (lane == pos) {
        ed = nd;
        ei = ni;
    }
}

// The candidates cd (one per lane, bank index base + lane) into the list, in lane order.
__device__ __forceinline__ void knn_offer(float& ed, int& ei, float cd, int base, int k) {
    const int lane = threadIdx.x & 63;
    const float td = __shfl(ed, k - 1);
    const int ti = __shfl(ei, k - 1);
    unsigned long long m = __ballot(knn_before(cd, base + lane, td, ti));
    while (m != 0ull) {
        const int b = __ffsll((long long)m) - 1;
        m &= m - 1ull;
        knn_insert(ed, ei, __shfl(cd, b), base + b, k);
    }
}

__global__ __launch_bounds__(OOD_NT) void ood_knn_kernel(KnnArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float s_q[KNN_QE_MAX * KNN_QT];  // [j][query]: resident (E <= KNN_QE_MAX), or slab 0 only
    __shared__ __attribute__((aligned(16))) float s_b[KNN_EJ * KNN_BS];      // [j][bank row] of one slab; then the tile's distances [query][row]
    __shared__ float s_ld[KNN_QT * OOD_MAX_K];
    __shared__ int s_li[KNN_QT * OOD_MAX_K];
    __shared__ int s_bnan[KNN_BT];
    __shared__ int s_count;
    static_assert(KNN_EJ * KNN_BS >= KNN_QT * KNN_BT, "the distances of a tile reuse the slab");
    static_assert(KNN_EJ == 32 && OOD_NT == 8 * KNN_EJ && KNN_BT % 8 == 0 && KNN_QT % 8 == 0, "a thread stages coordinate tx of rows ty + 8 it");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tx = tid & 31, ty = tid >> 5;
    const int E = a.E, k = a.k;
    const bool resident = E <= KNN_QE_MAX;
    const long i0 = (long)blockIdx.y * KNN_QT;
    const long c0 = (long)blockIdx.x * a.chunk_rows, c1 = min(a.Mb, c0 + a.chunk_rows);

    auto stage_q = [&](int j0, float* dst) {  // q[i0 ..][j0 .. j0 + KNN_EJ) -> dst[j][query]; rows past Mq and coordinates past E are 0
        for (int e = tid; e < KNN_QT * KNN_EJ; e += OOD_NT) {
            const int r = e / KNN_EJ, j = e % KNN_EJ;
            const long i = i0 + r;
            dst[j * KNN_QT + r] = (i < a.Mq && j0 + j < E) ? a.q[i * E + j0 + j] : 0.0f;
        }
    };
    for (int e = tid; e < KNN_QT * OOD_MAX_K; e += OOD_NT) {
        s_ld[e] = INFINITY;
        s_li[e] = KNN_FILL;
    }
    if (tid < KNN_BT) s_bnan[tid] = 0;
    if (tid == 0) s_count = 0;
    if (resident)
        for (int j0 = 0; j0 < E; j0 += KNN_EJ) stage_q(j0, s_q + j0 * KNN_QT);
    int nan_rows = 0;  // (threads < KNN_BT: the bank rows holding a NaN among the rows this thread watched)

    // The bank slab (and, when the queries are not resident, the query slab) of the NEXT step is fetched into registers while this
    // step's is being used: thread (tx, ty) owns coordinate tx of rows ty + 8 it.
    float pb[KNN_BT * KNN_EJ / OOD_NT], pq[KNN_QT * KNN_EJ / OOD_NT];
    auto fetch = [&](long m0, int j0) {
        const bool live = j0 + tx < E;
#pragma unroll
        for (int it = 0; it < KNN_BT * KNN_EJ / OOD_NT; ++it) {
            const long m = m0 + ty + 8 * it;
            pb[it] = (live && m < c1) ? a.bank[m * E + j0 + tx] : 0.0f;
        }
        if (!resident) {
#pragma unroll
            for (int it = 0; it < KNN_QT * KNN_EJ / OOD_NT; ++it) {
                const long i = i0 + ty + 8 * it;
                pq[it] = (live && i < a.Mq) ? a.q[i * E + j0 + tx] : 0.0f;
            }
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int it = 0; it < KNN_BT * KNN_EJ / OOD_NT; ++it) {
            s_b[tx * KNN_BS + ty + 8 * it] = pb[it];
            if (pb[it] != pb[it]) s_bnan[ty + 8 * it] = 1;
        }
        if (!resident) {
#pragma unroll
            for (int it = 0; it < KNN_QT * KNN_EJ / OOD_NT; ++it) s_q[tx * KNN_QT + ty + 8 * it] = pq[it];
        }
    };
    fetch(c0, 0);
    for (long m0 = c0; m0 < c1; m0 += KNN_BT) {
        float acc[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[u][v] = 0.0f;
        for (int j0 = 0; j0 < E; j0 += KNN_EJ) {
            __syncthreads();  // the slab (or the distances) of the step before has been read
            commit();
            __syncthreads();
            if (j0 + KNN_EJ < E) fetch(m0, j0 + KNN_EJ);
            else if (m0 + KNN_BT < c1) fetch(m0 + KNN_BT, 0);
            const float* sq = s_q + (resident ? j0 * KNN_QT : 0) + 4 * ty;
            const float* sb = s_b + 4 * tx;
            const int jn = min(KNN_EJ, E - j0);
#pragma unroll 4
            for (int j = 0; j < jn; ++j) {
                const float4 qv = *reinterpret_cast<const float4*>(sq + j * KNN_QT);
                const float4 bv = *reinterpret_cast<const float4*>(sb + j * KNN_BS);
                const float qa[4] = {qv.x, qv.y, qv.z, qv.w}, ba[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const float t = qa[u] - ba[v];
                        const float p = t * t;
                        acc[u][v] = acc[u][v] + p;
                    }
            }
        }
        __syncthreads();  // every lane is done with the last slab
        {
            const float nanv = __builtin_nanf("");
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long i = i0 + 4 * ty + u;
                float o[4];
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const long m = m0 + 4 * tx + v;
                    const bool out = m >= c1 || (a.self_base >= 0 && m == a.self_base + i);
                    o[v] = out ? nanv : acc[u][v];  // a NaN is offered to no list
                }
                *reinterpret_cast<float4*>(s_b + (4 * ty + u) * KNN_BT + 4 * tx) = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
        __syncthreads();
        if (tid < KNN_BT) {
            nan_rows += s_bnan[tid];
            s_bnan[tid] = 0;  // (the next write to it comes behind the barrier at the top of the slab loop)
        }
        for (int r = wave * (KNN_QT / 4); r < (wave + 1) * (KNN_QT / 4); ++r) {
            float ed = s_ld[r * OOD_MAX_K + lane];
            int ei = s_li[r * OOD_MAX_K + lane];
            knn_offer(ed, ei, s_b[r * KNN_BT + lane], (int)m0, k);
            knn_offer(ed, ei, s_b[r * KNN_BT + 64 + lane], (int)m0 + 64, k);
            s_ld[r * OOD_MAX_K + lane] = ed;
            s_li[r * OOD_MAX_K + lane] = ei;
        }
    }
    // the block's lists (a wave wrote the ones it reads here)
    for (int r = wave * (KNN_QT / 4); r < (wave + 1) * (KNN_QT / 4); ++r) {
        const long i = i0 + r;
        if (i < a.Mq && lane < k) {
            const size_t o = ((size_t)blockIdx.x * a.Mq + i) * k + lane;
            a.ws_d[o] = s_ld[r * OOD_MAX_K + lane];
            a.ws_i[o] = s_li[r * OOD_MAX_K + lane];
        }
    }
    if (blockIdx.y == 0) {  // the bank rows holding a NaN are counted once: by the blocks of the first query tile
        if (nan_rows) atomicAdd(&s_count, nan_rows);
        __syncthreads();
        if (tid == 0 && s_count) atomicAdd(a.status, (unsigned long long)s_count);
    }
}

// One wave per query: its lists of all chunks, in bank order, into one; then the outputs.
__global__ __launch_bounds__(OOD_NT) void ood_knn_finish_kernel(KnnArgs a) {
    const int lane = threadIdx.x & 63, k = a.k;
    const long i = (long)blockIdx.x * (OOD_NT / 64) + (threadIdx.x >> 6);
    if (i >= a.Mq) return;  // (a whole wave)
    bool nan = false;
    for (int j = lane; j < a.E; j += 64) {
        const float v = a.q[i * a.E + j];
        nan |= v != v;
    }
    nan = __ballot(nan) != 0ull;
    float ed = INFINITY;
    int ei = KNN_FILL;
    if (!nan)
        for (int c = 0; c < a.chunks; ++c) {
            const size_t o = ((size_t)c * a.Mq + i) * k;
            const float cd = lane < k ? a.ws_d[o + lane] : INFINITY;
            const int ci = lane < k ? a.ws_i[o + lane] : KNN_FILL;
            const float td = __shfl(ed, k - 1);
            const int ti = __shfl(ei, k - 1);
            unsigned long long m = __ballot(ci != KNN_FILL && knn_before(cd, ci, td, ti));
            while (m != 0ull) {
                const int b = __ffsll((long long)m) - 1;
                m &= m - 1ull;
                knn_insert(ed, ei, __shfl(cd, b), __shfl(ci, b), k);
            }
        }
    if (lane < k) {
        a.dist[i * k + lane] = nan ? __builtin_nanf("") : ed;
        a.index[i * k + lane] = (nan || ei == KNN_FILL) ? -1 : ei;
    }
    if (nan && lane == 0) atomicAdd(a.status + 1, 1ull);
}

// ---- class-conditional Gaussians -----------------------------------------------------------------------------------------------------------
struct MomentArgs {
    const float* x;
    const int32_t* labels;
    long M;
    int E, K, accumulate;
    long long *n, *skipped;
    double *sum, *scatter;
    unsigned long long* cnt;  // workspace [K + 2]: valid rows per class, rows with a label out of range, labelled rows holding a NaN
    int32_t* cls;             // workspace [M]: the label of a valid row, -1
};

__global__ __launch_bounds__(OOD_NT) void ood_moment_rows_kernel(MomentArgs a) {
    __shared__ unsigned long long s_c[EVAL_MAX_K + 2];
    const int tid = threadIdx.x;
    if (tid < a.K + 2) s_c[tid] = 0ull;
    __syncthreads();
    const long i = (long)blockIdx.x * OOD_NT + tid;
    if (i < a.M) {
        const int L = a.labels[i];
        int c = -1;
        if (L < 0 || L >= a.K) {
            atomicAdd(&s_c[a.K], 1ull);
        } else {
            bool nan = false;
            for (int j = 0; j < a.E; ++j) {
                const float v = a.x[i * a.E + j];
                nan |= v != v;
            }
            if (nan) atomicAdd(&s_c[a.K + 1], 1ull);
            else {
                c = L;
                atomicAdd(&s_c[L], 1ull);
            }
        }
        a.cls[i] = c;
    }
    __syncthreads();
    if (tid < a.K + 2 && s_c[tid]) atomicAdd(&a.cnt[tid], s_c[tid]);
}

// blocks [0, T * T), T = ceil(E / 16): a 16 x 16 tile of scatter, one entry per thread.  blocks past them: sum, one (class, column) per
// thread, and (the first of them) n and skipped.  Every thread walks the rows in the one defined order.
__global__ __launch_bounds__(OOD_NT) void ood_moments_kernel(MomentArgs a) {
#pragma clang fp contract(off)
    constexpr int R = 64;  // rows staged at a time; divides OOD_MOMENT_CHUNK
    static_assert(OOD_MOMENT_CHUNK % R == 0, "a stage never straddles a chunk");
    __shared__ float s_a[R][16], s_b[R][16];
    __shared__ int s_cls[R];
    const int tid = threadIdx.x, E = a.E, T = (E + 15) / 16;
    if ((int)blockIdx.x < T * T) {
        const int a0 = ((int)blockIdx.x / T) * 16, b0 = ((int)blockIdx.x % T) * 16, ta = tid >> 4, tb = tid & 15;
        double total = 0.0, part = 0.0;
        for (long r0 = 0; r0 < a.M; r0 += R) {
            __syncthreads();
            for (int e = tid; e < R * 16; e += OOD_NT) {
                const int r = e >> 4, j = e & 15;
                const long i = r0 + r;
                s_a[r][j] = (i < a.M && a0 + j < E) ? a.x[i * E + a0 + j] : 0.0f;
                s_b[r][j] = (i < a.M && b0 + j < E) ? a.x[i * E + b0 + j] : 0.0f;
            }
            if (tid < R) s_cls[tid] = r0 + tid < a.M ? a.cls[r0 + tid] : -1;
            __syncthreads();
#pragma unroll 8
            for (int r = 0; r < R; ++r)  // (+ 0.0 for a skipped row changes nothing: part is never -0.0)
                part = part + (s_cls[r] >= 0 ? (double)s_a[r][ta] * (double)s_b[r][tb] : 0.0);
            if ((r0 + R) % OOD_MOMENT_CHUNK == 0 || r0 + R >= a.M) {
                total = total + part;
                part = 0.0;
            }
        }
        if (a0 + ta < E && b0 + tb < E) {
            double* o = a.scatter + (size_t)(a0 + ta) * E + b0 + tb;
            *o = a.accumulate ? *o + total : total;
        }
        return;
    }
    const int e = ((int)blockIdx.x - T * T) * OOD_NT + tid;
    if (e < a.K + 2) {
        long long* o = e < a.K ? a.n + e : a.skipped + (e - a.K);
        *o = (a.accumulate ? *o : 0ll) + (long long)a.cnt[e];
    }
    if (e >= a.K * E) return;
    const int c = e / E, j = e % E;
    double total = 0.0, part = 0.0;
    for (long r0 = 0; r0 < a.M; r0 += OOD_MOMENT_CHUNK) {
        const long r1 = min(a.M, r0 + OOD_MOMENT_CHUNK);
#pragma unroll 8
        for (long i = r0; i < r1; ++i) part = part + (a.cls[i] == c ? (double)a.x[i * E + j] : 0.0);  // (+ 0.0 changes nothing: part is never -0.0)
        total = total + part;
        part = 0.0;
    }
    a.sum[e] = a.accumulate ? a.sum[e] + total : total;
}

// A block scores MAHA_ROWS rows: per class the differences x - mu_c in LDS, thread i the i-th entry of W (x - mu_c) for each row, a fixed
// block sum of the squares.
constexpr int MAHA_ROWS = 4;

__global__ __launch_bounds__(OOD_NT) void ood_mahalanobis_kernel(const float* __restrict__ x, const double* __restrict__ mu,
                                                                 const double* __restrict__ W, long M, int E, int K, double* m_out, float* score,
                                                                 int32_t* argclass) {
#pragma clang fp contract(off)
    __shared__ double s_d[MAHA_ROWS][OOD_MAX_ME];
    __shared__ double s_red[4];
    __shared__ double s_m[MAHA_ROWS][EVAL_MAX_K];
    const int tid = threadIdx.x;
    const long i0 = (long)blockIdx.x * MAHA_ROWS;
    for (int c = 0; c < K; ++c) {
        __syncthreads();
        for (int e = tid; e < MAHA_ROWS * E; e += OOD_NT) {
            const int r = e / E, j = e % E;
            s_d[r][j] = i0 + r < M ? (double)x[(i0 + r) * E + j] - mu[(size_t)c * E + j] : 0.0;
        }
        __syncthreads();
        double y[MAHA_ROWS];
#pragma unroll
        for (int r = 0; r < MAHA_ROWS; ++r) y[r] = 0.0;
        if (tid < E) {
            const double* w = W + (size_t)tid * E;
            for (int j = 0; j <= tid; ++j) {
                const double wv = w[j];
#pragma unroll
                for (int r = 0; r < MAHA_ROWS; ++r) y[r] = y[r] + wv * s_d[r][j];
            }
        }
#pragma unroll
        for (int r = 0; r < MAHA_ROWS; ++r) {
            const double v = block_sum_fixed(y[r] * y[r], s_red);
            if (tid == 0) s_m[r][c] = v;
        }
    }
    __syncthreads();
    if (tid < MAHA_ROWS && i0 + tid < M) {
        const long i = i0 + tid;
        double best = 0.0;
        int arg = -1;
        for (int c = 0; c < K; ++c) {
            const double v = s_m[tid][c];
            m_out[i * K + c] = v;
            const double m0 = mu[(size_t)c * E];
            const bool fitted = m0 - m0 == 0.0;  // a class without rows has a NaN mean
            if (fitted && (arg < 0 ? v == v : v < best)) {
                best = v;
                arg = c;
            }
        }
        score[i] = arg < 0 ? __builtin_nanf("") : (float)best;
        argclass[i] = arg;
    }
}

// ---- flags and tallies ---------------------------------------------------------------------------------------------------------------------
constexpr int OOD_TALLY_WORDS = 8;  // id_rows, id_flagged, ood_rows, ood_flagged, nan_rows, id_correct_kept, id_kept, id_correct_flagged

__global__ __launch_bounds__(OOD_NT) void ood_tally_kernel(const float* __restrict__ scores, const int32_t* __restrict__ kind,
                                                           const int32_t* __restrict__ correct, const float* __restrict__ tau, long M, int A,
                                                           uint8_t* flags, unsigned long long* tallies) {
    __shared__ unsigned long long s_t[OOD_MAX_A * OOD_TALLY_WORDS];
    const int tid = threadIdx.x;
    if (tid < A * OOD_TALLY_WORDS) s_t[tid] = 0ull;
    __syncthreads();
    const long i = (long)blockIdx.x * OOD_NT + tid;
    if (i < M) {
        const float s = scores[i];
        const int kd = kind[i];
        const bool nan = s != s, row = kd == 0 || kd == 1;
        const bool ok = correct && correct[i] != 0;
        for (int t = 0; t < A; ++t) {
            const bool flag = nan || s > tau[t];
            flags[(long)t * M + i] = flag ? 1 : 0;
            if (!row) continue;
            unsigned long long* h = s_t + t * OOD_TALLY_WORDS;
            atomicAdd(h + (kd == 0 ? 0 : 2), 1ull);
            if (flag) atomicAdd(h + (kd == 0 ? 1 : 3), 1ull);
            if (nan) atomicAdd(h + 4, 1ull);
            if (kd == 0 && correct) {
                if (!flag) atomicAdd(h + 6, 1ull);
                if (ok) atomicAdd(h + (flag ? 7 : 5), 1ull);
            }
        }
    }
    __syncthreads();
    if (tid < A * OOD_TALLY_WORDS && s_t[tid]) atomicAdd(&tallies[tid], s_t[tid]);
}

static bool knn_sizes_ok(long Mq, long Mb, int E, int k) {
    return Mq >= 1 && Mq <= OOD_MAX_Q && Mb >= 1 && Mb <= OOD_MAX_B && E >= 1 && E <= OOD_MAX_E && k >= 1 && k <= OOD_MAX_K;
}

static bool moment_sizes_ok(long M, int E, int K) { return M >= 1 && M <= OOD_MAX_B && E >= 1 && E <= OOD_MAX_ME && K >= 1 && K <= EVAL_MAX_K; }

struct MomentWorkspace {
    unsigned long long* cnt;
    int32_t* cls;
    size_t cnt_bytes, bytes;
};

static MomentWorkspace moment_workspace(void* ws, long M, int K) {
    MomentWorkspace w;
    Carve c{static_cast<char*>(ws)};
    w.cnt = c.take<unsigned long long>((size_t)K + 2, 16);
    w.cnt_bytes = c.used;
    w.cls = c.take<int32_t>((size_t)M, 16);
    w.bytes = (c.used + 15) / 16 * 16;
    return w;
}

}  // namespace pasn

using namespace pasn;

extern "C" int pasn_ood_head_scores(const float* sim, const float* logits, long M, int P, int K, int K_real, float* maxsim, float* energy,
                                    void* stream) {
    PASN_REQUIRE(maxsim || energy, "at least one of maxsim and energy is required");
    PASN_REQUIRE(!maxsim || sim, "maxsim needs sim");
    PASN_REQUIRE(!energy || logits, "energy needs logits");
    PASN_REQUIRE(M >= 1 && M <= OOD_MAX_Q, "M must lie in [1, 2^20]");
    PASN_REQUIRE(!maxsim || (P >= 1 && P <= OOD_MAX_P), "P must lie in [1, 4096]");
    PASN_REQUIRE(!energy || (K_real >= 1 && K_real <= K && K <= OOD_MAX_P), "K_real must lie in [1, K], K in [1, 4096]");
    hipLaunchKernelGGL(ood_head_scores_kernel, dim3(ceil_div(M, OOD_NT)), dim3(OOD_NT), 0, (hipStream_t)stream, sim, logits, M, P, K, K_real,
                       maxsim, energy);
    return check_launch("ood_head_scores");
}

extern "C" int pasn_ood_rows_normalize(const float* x, long M, int E, float* y, void* stream) {
    PASN_REQUIRE(x && y, "x and y are required");
    PASN_REQUIRE(M >= 1 && M <= OOD_MAX_B, "M must lie in [1, 2^24]");
    PASN_REQUIRE(E >= 1 && E <= OOD_MAX_E, "E must lie in [1, 1024]");
    hipLaunchKernelGGL(ood_rows_normalize_kernel, dim3(ceil_div(M, OOD_NT)), dim3(OOD_NT), 0, (hipStream_t)stream, x, M, E, y);
    return check_launch("ood_rows_normalize");
}

extern "C" size_t pasn_ood_knn_workspace_bytes(long Mq, long Mb, int E, int k) {
    if (!knn_sizes_ok(Mq, Mb, E, k)) return 0;
    return ((size_t)knn_plan(Mq, Mb).chunks * Mq * k * 8 + 15) / 16 * 16;
}

extern "C" int pasn_ood_knn(const float* q, const float* bank, long Mq, long Mb, int E, int k, long self_base, float* dist, int32_t* index,
                            int64_t* status, void* workspace, void* stream) {
    PASN_REQUIRE(q && bank, "q and bank are required");
    PASN_REQUIRE(dist && index && status, "every output is required");
    PASN_REQUIRE(workspace, "workspace is required");
    PASN_REQUIRE(Mq >= 1 && Mq <= OOD_MAX_Q, "Mq must lie in [1, 2^20]");
    PASN_REQUIRE(Mb >= 1 && Mb <= OOD_MAX_B, "Mb must lie in [1, 2^24]");
    PASN_REQUIRE(E >= 1 && E <= OOD_MAX_E, "E must lie in [1, 1024]");
    PASN_REQUIRE(k >= 1 && k <= OOD_MAX_K, "k must lie in [1, 64]");
    PASN_REQUIRE(self_base >= -1 && self_base <= Mb, "self_base must be -1 (no leave-one-out) or a bank row");
    PASN_REQUIRE(((uintptr_t)workspace & 15) == 0, "misaligned workspace");
    hipStream_t s = (hipStream_t)stream;
    const KnnPlan p = knn_plan(Mq, Mb);
    KnnArgs a;
    a.q = q;
    a.bank = bank;
    a.Mq = Mq;
    a.Mb = Mb;
    a.self_base = self_base;
    a.chunk_rows = p.chunk_rows;
    a.E = E;
    a.k = k;
    a.chunks = p.chunks;
    a.ws_d = static_cast<float*>(workspace);
    a.ws_i = reinterpret_cast<int32_t*>(a.ws_d + (size_t)p.chunks * Mq * k);
    a.dist = dist;
    a.index = index;
    a.status = reinterpret_cast<unsigned long long*>(status);
    if (hipMemsetAsync(status, 0, 2 * sizeof(int64_t), s) != hipSuccess) return check_launch("ood_knn");
    hipLaunchKernelGGL(ood_knn_kernel, dim3(p.chunks, p.qtiles), dim3(OOD_NT), 0, s, a);
    hipLaunchKernelGGL(ood_knn_finish_kernel, dim3(ceil_div(Mq, OOD_NT / 64)), dim3(OOD_NT), 0, s, a);
    return check_launch("ood_knn");
}

extern "C" int pasn_ood_moment_chunk(void) { return OOD_MOMENT_CHUNK; }

extern "C" size_t pasn_ood_moments_workspace_bytes(long M, int E, int K) {
    if (!moment_sizes_ok(M, E, K)) return 0;
    return moment_workspace(nullptr, M, K).bytes;
}

extern "C" int pasn_ood_moments(const float* x, const int32_t* labels, long M, int E, int K, int accumulate, int64_t* n, double* sum,
                                double* scatter, int64_t* skipped, void* workspace, void* stream) {
    PASN_REQUIRE(x && labels, "x and labels are required");
    PASN_REQUIRE(n && sum && scatter && skipped, "every output is required");
    PASN_REQUIRE(workspace, "workspace is required");
    PASN_REQUIRE(M >= 1 && M <= OOD_MAX_B, "M must lie in [1, 2^24]");
    PASN_REQUIRE(E >= 1 && E <= OOD_MAX_ME, "E must lie in [1, 256]");
    PASN_REQUIRE(K >= 1 && K <= EVAL_MAX_K, "K must lie in [1, 16]");
    PASN_REQUIRE(accumulate == 0 || accumulate == 1, "accumulate must be 0 or 1");
    PASN_REQUIRE(((uintptr_t)workspace & 15) == 0, "misaligned workspace");
    hipStream_t s = (hipStream_t)stream;
    const MomentWorkspace w = moment_workspace(workspace, M, K);
    MomentArgs a{x, labels, M, E, K, accumulate, reinterpret_cast<long long*>(n), reinterpret_cast<long long*>(skipped), sum, scatter, w.cnt, w.cls};
    if (hipMemsetAsync(w.cnt, 0, w.cnt_bytes, s) != hipSuccess) return check_launch("ood_moments");
    hipLaunchKernelGGL(ood_moment_rows_kernel, dim3(ceil_div(M, OOD_NT)), dim3(OOD_NT), 0, s, a);
    const int T = (E + 15) / 16;
    hipLaunchKernelGGL(ood_moments_kernel, dim3(T * T + ceil_div(std::max(K * E, K + 2), OOD_NT)), dim3(OOD_NT), 0, s, a);
    return check_launch("ood_moments");
}

extern "C" int pasn_ood_mahalanobis(const float* x, const double* mu, const double* W, long M, int E, int K, double* m, float* score,
                                    int32_t* argclass, void* stream) {
    PASN_REQUIRE(x && mu && W, "x, mu and W are required");
    PASN_REQUIRE(m && score && argclass, "every output is required");
    PASN_REQUIRE(M >= 1 && M <= OOD_MAX_Q, "M must lie in [1, 2^20]");
    PASN_REQUIRE(E >= 1 && E <= OOD_MAX_ME, "E must lie in [1, 256]");
    PASN_REQUIRE(K >= 1 && K <= EVAL_MAX_K, "K must lie in [1, 16]");
    hipLaunchKernelGGL(ood_mahalanobis_kernel, dim3(ceil_div(M, MAHA_ROWS)), dim3(OOD_NT), 0, (hipStream_t)stream, x, mu, W, M, E, K, m, score,
                       argclass);
    return check_launch("ood_mahalanobis");
}

extern "C" int pasn_ood_tally(const float* scores, const int32_t* kind, const int32_t* correct, const float* tau, long M, int A, uint8_t* flags,
                              int64_t* tallies, void* stream) {
    PASN_REQUIRE(scores && kind && tau, "scores, kind and tau are required");
    PASN_REQUIRE(flags && tallies, "flags and tallies are required");
    PASN_REQUIRE(M >= 1 && M <= OOD_MAX_Q, "M must lie in [1, 2^20]");
    PASN_REQUIRE(A >= 1 && A <= OOD_MAX_A, "A must lie in [1, 8]");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(tallies, 0, (size_t)A * OOD_TALLY_WORDS * sizeof(int64_t), s) != hipSuccess) return check_launch("ood_tally");
    hipLaunchKernelGGL(ood_tally_kernel, dim3(ceil_div(M, OOD_NT)), dim3(OOD_NT), 0, s, scores, kind, correct, tau, M, A, flags,
                       reinterpret_cast<unsigned long long*>(tallies));
    return check_launch("ood_tally");
}
