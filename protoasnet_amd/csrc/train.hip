// train.hip -- the elementwise / reduction half of the training path: batch-statistics norm, activation forward and
// backward, squeeze-excite backward, strided scatter.  All HBM-bound passes over channels-last rows [N][S][Cp];
// a thread owns 8 channels of a row, a block's threads tile (row lane, channel group) so that a wave reads whole rows
// back to back, and every reduction is two-stage with a fixed summation order (bitwise reproducible gradients).
//
// Reference semantics: torch.nn.BatchNorm{2,3}d in train mode (biased batch variance for normalisation, unbiased for
// the running estimate, momentum 0.1) as instantiated at resnet_features.py:140,180 and by every trunk the reference
// trains (agents call model.train(): Video_XProtoNet_e2e.py:118); autograd's derivative of the same expressions.
#include "block_reduce.h"
#include "common.h"

namespace pasn {

constexpr int PASN_MAX_GROUPS = 4;  // statistics groups of one pass (bn_finalize_kernel)

struct RowGeom {
    int CG, LPR, RL, chunks, rows_per_chunk;
};

// 256 threads = RL row lanes x LPR lanes per row; lane cg of a row owns channels 8 cg .. 8 cg + 7 (lanes cg >= CG and the threads beyond
// RL * LPR idle).  LPR = the next power of two >= CG.  PASN_TRAIN_ROWS_CONTIG=1: LPR = CG -- a block's live threads read RL whole rows as
// ONE contiguous span and 240-255 of 256 threads are live at the X3D widths instead of 75-88 %; measured +-0 on the step (the passes are
// not short of requests in flight), and it re-partitions every sum, so the default keeps the summation order of rounds 1-3.
static RowGeom row_geom(int N, int S, int Cp) {
    RowGeom g;
    g.CG = Cp / 8;
    g.LPR = tune_is("PASN_TRAIN_ROWS_CONTIG", '1') ? g.CG : pow2_at_least(g.CG);
    g.RL = 256 / g.LPR;
    int blocks = 1024;
    if (const char* e = tune("PASN_TRAIN_BLOCKS")) blocks = std::max(256, atoi(e));
    const int want = std::max(1, blocks / std::max(1, N));
    const int maxc = std::max(1, S / (g.RL * 16));  // small tensors: fewer partials, the finalize pass is pure latency
    g.chunks = std::min(want, maxc);
    g.rows_per_chunk = ceil_div(S, g.chunks);
    g.chunks = ceil_div(S, g.rows_per_chunk);
    return g;
}

// Rows in flight per thread: every pass below requests ROWS_U rows of each operand, then computes, then stores.  (A plain loop, even
// unrolled, waited for each row's loads before the next row's went out wherever the pass writes in place or branches on the activation:
// two or three 16-byte loads in flight per thread, 2.8-4 TB/s.)
constexpr int ROWS_U = 4;
template <typename T>
struct Raw8 {
    uint4 r[(8 * sizeof(T)) / 16];
};
template <typename T>
__device__ __forceinline__ Raw8<T> load_raw8(const T* p) {
    Raw8<T> q;
#pragma unroll
    for (int i = 0; i < (int)((8 * sizeof(T)) / 16); ++i) q.r[i] = reinterpret_cast<const uint4*>(p)[i];
    return q;
}

template <typename T>
__device__ __forceinline__ Raw8<T> load_raw8(__amdgpu_buffer_rsrc_t rs, unsigned off) {
    Raw8<T> q;
#pragma unroll
    for (int i = 0; i < (int)((8 * sizeof(T)) / 16); ++i) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(off + 16 * i), 0, 0);
        q.r[i] = uint4{v[0], v[1], v[2], v[3]};
    }
    return q;
}
__device__ __forceinline__ void store8(__amdgpu_buffer_rsrc_t rs, unsigned off, const float (&v)[8], const __bf16*) {
    bf16x8 a;
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = (__bf16)v[j];
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, a), rs, (int)off, 0, 0);
}
__device__ __forceinline__ void store8(__amdgpu_buffer_rsrc_t rs, unsigned off, const float (&v)[8], const float*) {
    __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])}, rs, (int)off, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(v[4]), __float_as_uint(v[5]), __float_as_uint(v[6]), __float_as_uint(v[7])}, rs, (int)off + 16, 0, 0);
}

// one batch of ROWS_U rows of a thread, as RowWalk::batches hands it to a pass
struct RowBatch {
    unsigned off[ROWS_U];  // byte offset of row u's 8 channels inside the clip (for the descriptors of RowWalk::rows)
    int first, step, r1;   // row 0 of the batch, rows between its rows, the end of the chunk
    __device__ __forceinline__ bool in(int u) const { return first + u * step < r1; }  // row u lies inside the chunk
};
// The walk of one thread of block (chunk blockIdx.x, clip blockIdx.y) over its rows, the same in every row pass below: which channels the
// thread owns, whether it has rows at all, and its rows in batches of ROWS_U.  The order in which a thread meets its rows is, with
// block_reduce_rows, the summation order DESIGN.md promises -- which is why there is ONE copy of it.
template <typename T>
struct RowWalk {
    int n, c0;  // the block's clip; the first of the thread's 8 channels
    bool live;  // false: a lane beyond the channel groups or the row lanes -- no rows (it still joins a block reduce with zeros)

    __device__ __forceinline__ RowWalk(int S, int Cp, int CG, int LPR, int rows_per_chunk) {
        const int cg = threadIdx.x % LPR, rl = threadIdx.x / LPR, r0 = blockIdx.x * rows_per_chunk;
        n = blockIdx.y;
        c0 = cg * 8;
        step = 256 / LPR;
        live = cg < CG && rl < step;
        first = r0 + rl;
        r1 = min(S, r0 + rows_per_chunk);
        cp = Cp;
        clip = (size_t)n * S * Cp;
    }
    // This clip of tensor p behind a buffer descriptor that ends where the block's chunk ends (num_records = r1 rows): a row past the chunk
    // reads as zeros and its store is dropped by the hardware -- no clamped row index, no 64-bit address per row, no select per element to
    // keep such a row out of the sums (these passes are bound by vector issue).  Offsets are 32-bit bytes inside ONE clip (the launchers
    // check S * Cp * sizeof(T) < 2^31).
    __device__ __forceinline__ __amdgpu_buffer_rsrc_t rows(const T* p) const {
        return buffer_rsrc(p + clip, (unsigned)r1 * (unsigned)cp * (unsigned)sizeof(T));
    }
    // body(b) per batch of ROWS_U rows.  A row past the chunk is out of range of rows(): zeros in, nothing out -- only a pass whose
    // arithmetic turns a zero row into something else (a shift, an added constant) needs b.in(u).
    template <typename Body>
    __device__ __forceinline__ void batches(Body body) const {
        const unsigned rowb = (unsigned)cp * (unsigned)sizeof(T), cgo = (unsigned)c0 * (unsigned)sizeof(T);
        for (int r = first; r < r1; r += ROWS_U * step) {
            RowBatch b;
            b.first = r, b.step = step, b.r1 = r1;
#pragma unroll
            for (int u = 0; u < ROWS_U; ++u) b.off[u] = (unsigned)(r + u * step) * rowb + cgo;
            body(b);
        }
    }

private:
    int first, step, r1, cp;  // the thread's first row, the row lanes of the block, the end of the chunk, the channel stride
    size_t clip;              // element offset of the clip
};

// ---- batch statistics ---------------------------------------------------------------------------------------------
// ws[n][chunk][2][Cp]: sum(y - k), sum((y - k)^2) with the shift k[c] = y[0][0][c] (keeps the variance free of
// cancellation when |mean| >> std).  The one row pass that is NOT on RowWalk: it reads through clamped pointers (one operand, no store) and
// needs a select per row (0 - k is not 0); on the walk, in either load form, hipcc sinks part of the last row's load under that select
// and branches per row -- 23.9 us per launch where this form takes 22.8 (profiles/README.md "Training row passes refactor").  Its split of
// the block, chunk bounds and row order are RowWalk's.
template <typename T>
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const T* __restrict__ y, float* __restrict__ ws, int S, int Cp,
                                                               int CG, int LPR, int rows_per_chunk, int chunks) {
    __shared__ float red[256 * 8];
    const int n = blockIdx.y, ch = blockIdx.x;
    const int cg = threadIdx.x % LPR, rl = threadIdx.x / LPR, RL = 256 / LPR;
    float acc[2][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[0][j] = acc[1][j] = 0.0f;
    if (cg < CG && rl < RL) {
        float k[8];
        load8(y + cg * 8, k);
        const int r0 = ch * rows_per_chunk, r1 = min(S, r0 + rows_per_chunk);
        const T* base = y + (size_t)n * S * Cp + cg * 8;
        for (int r = r0 + rl; r < r1; r += ROWS_U * RL) {
            Raw8<T> yv[ROWS_U];
#pragma unroll
            for (int u = 0; u < ROWS_U; ++u) yv[u] = load_raw8(base + (size_t)min(r + u * RL, r1 - 1) * Cp);
#pragma unroll
            for (int u = 0; u < ROWS_U; ++u) {
                float v[8];
                raw_to_f8<T>(yv[u].r, v);
                const bool ok = r + u * RL < r1;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float dlt = ok ? v[j] - k[j] : 0.0f;
                    acc[0][j] += dlt;
                    acc[1][j] = fmaf(dlt, dlt, acc[1][j]);
                }
            }
        }
    }
    block_reduce_rows<2>(acc, red, ws + ((size_t)n * chunks + ch) * 2 * Cp, Cp, CG, LPR);
}

// Totals of statistics group g (clips g gdiv .. (g + 1) gdiv - 1) of partials ws[clip * chunks + chunk][2][Cp], for the block's 16
// channels: each of the 16 "parts" sums every 16th partial (independent loads), then part 0 adds the parts in order through red.  Call it
// group after group, g = 0, 1, ..: t1 / t2 are the totals in the threads of part 0.
__device__ __forceinline__ void group_totals(const float* __restrict__ ws, int g, int gdiv, int chunks, int Cp, int c, bool live,
                                             float (&red)[2][16][16], float& t1, float& t2) {
    const int cl = threadIdx.x & 15, part = threadIdx.x >> 4;
    float a1 = 0.0f, a2 = 0.0f;
    if (live) {
        const int lo = g * gdiv * chunks, hi = lo + gdiv * chunks;
#pragma unroll 8
        for (int i = lo + part; i < hi; i += 16) {
            const float* p = ws + (size_t)i * 2 * Cp + c;
            a1 += p[0];
            a2 += p[Cp];
        }
    }
    if (g) __syncthreads();  // the previous group's totals have been read
    red[0][part][cl] = a1;
    red[1][part][cl] = a2;
    __syncthreads();
    t1 = t2 = 0.0f;
    if (part == 0)
        for (int q = 0; q < 16; ++q) {
            t1 += red[0][q][cl];
            t2 += red[1][q][cl];
        }
}

// One block per 16 channels.  Totals: group_totals.  Per-clip pool (squeeze-excite only): a part owns whole clips, no cross-thread
// combine at all.
template <typename T>
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ ws, const T* __restrict__ y, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float* rmean, float* rvar,  // (no restrict: `shift` may alias rmean)
                                                          float momentum, float eps, float* __restrict__ stat, float* __restrict__ pool_u,
                                                          int N, int S, int C, int Cp, int chunks, const float* shift, int gdiv) {
    // GROUPS (round 4): clips n / gdiv form one statistics group -- the two trunk passes of the reference's loss recipe (the clips and their
    // warped copies) run as ONE 2N-clip pass, each half with its own batch statistics: stat[g][4][Cp], the running estimates updated group by
    // group in order, exactly as two N-clip passes leave them.  gdiv = N: one group, the layout of rounds 1-3.
    __shared__ float red[2][16][16];
    __shared__ float scsh[2][PASN_MAX_GROUPS][16];
    const int cl = threadIdx.x & 15, part = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    const bool live = c < Cp;
    const int G = N / gdiv;
    // the shift the partials were taken with: y[0][0][c] (bn_stats_partial_kernel), or `shift` (the stencils' fused statistics: the running
    // mean as it stood BEFORE this update -- read here ahead of the barrier, written below behind it), or 0
    float k = !live ? 0.0f : y ? (float)y[c] : (shift && c < C) ? shift[c] : 0.0f;  // `shift` holds C floats (padded channels: 0)
    asm volatile("" : "+v"(k));  // the value is taken HERE: `shift` may be the running mean this kernel updates behind the barrier
    for (int g = 0; g < G; ++g) {
        float t1, t2;
        group_totals(ws, g, gdiv, chunks, Cp, c, live, red, t1, t2);
        if (part == 0) {
            float mean = 0.0f, invstd = 0.0f, sc = 0.0f, sh = 0.0f;
            if (live && c < C) {
                const float R = (float)gdiv * (float)S;
                const float m = t1 / R;
                const float var = fmaxf(t2 / R - m * m, 0.0f);
                mean = k + m;
                invstd = 1.0f / sqrtf(var + eps);
                const float gm = gamma ? gamma[c] : 1.0f, bt = beta ? beta[c] : 0.0f;
                sc = gm * invstd;
                sh = bt - mean * sc;
                if (rmean) {
                    rmean[c] = (1.0f - momentum) * rmean[c] + momentum * mean;
                    rvar[c] = (1.0f - momentum) * rvar[c] + momentum * var * (R / fmaxf(R - 1.0f, 1.0f));
                }
            }
            if (live) {
                float* st = stat + (size_t)g * 4 * Cp;
                st[c] = mean;
                st[Cp + c] = invstd;
                st[2 * Cp + c] = sc;
                st[3 * Cp + c] = sh;
            }
            scsh[0][g][cl] = sc;
            scsh[1][g][cl] = sh;
        }
    }
    if (pool_u == nullptr) return;
    __syncthreads();
    if (!live) return;
    for (int n = part; n < N; n += 16) {
        const float sc = scsh[0][n / gdiv][cl], sh = scsh[1][n / gdiv][cl];
        float b1 = 0.0f;
        const float* p = ws + (size_t)n * chunks * 2 * Cp + c;
#pragma unroll 4
        for (int ch = 0; ch < chunks; ++ch) b1 += p[(size_t)ch * 2 * Cp];
        pool_u[(size_t)n * Cp + c] = sc * (k + b1 / (float)S) + sh;
    }
}

// ---- a = act((y*sc + sh + residual) * gate) ------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void affine_act_fwd_kernel(const T* __restrict__ y, const float* __restrict__ stat, const T* __restrict__ res,
                                                             const float* __restrict__ gate, T* __restrict__ a, int S, int Cp, int CG,
                                                             int LPR, int rows_per_chunk, int act, int gdiv) {
    const RowWalk<T> w(S, Cp, CG, LPR, rows_per_chunk);
    if (!w.live) return;
    stat += (size_t)(w.n / gdiv) * 4 * Cp;  // this clip's statistics group
    float sc[8], sh[8], g[8];
    load8(stat + 2 * Cp + w.c0, sc);
    load8(stat + 3 * Cp + w.c0, sh);
    if (gate) load8(gate + (size_t)w.n * Cp + w.c0, g);
    const __amdgpu_buffer_rsrc_t yrs = w.rows(y), qrs = w.rows(res ? res : y), ars = w.rows(a);
    w.batches([&](const RowBatch& b) {
        Raw8<T> yv[ROWS_U], qv[ROWS_U];
#pragma unroll
        for (int u = 0; u < ROWS_U; ++u) yv[u] = load_raw8<T>(yrs, b.off[u]);
        if (res) {
#pragma unroll
            for (int u = 0; u < ROWS_U; ++u) qv[u] = load_raw8<T>(qrs, b.off[u]);
        }
#pragma unroll
        for (int u = 0; u < ROWS_U; ++u) {
            float v[8];
            raw_to_f8<T>(yv[u].r, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = fmaf(v[j], sc[j], sh[j]);
            if (res) {
                float q[8];
                raw_to_f8<T>(qv[u].r, q);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] += q[j];
            }
            if (gate) {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] *= g[j];
            }
            act_vec(v, act);
            store8(ars, b.off[u], v, (const T*)nullptr);
        }
    });
}

// ---- backward pass over one unit (in place on d) --------------------------------------------------------------------
// The `mode` of pasn_unit_bwd_reduce (yhat = (y - mean) * invstd):
enum GradMode : int {
    GRAD_ACT = 0,         // d' = d * act'(y*sc + sh + residual)     partials: sum d', sum d' * yhat
    GRAD_GATE = 1,        // d' = d * act'((y*sc + sh) * gate)       partials: sum d' * (y*sc + sh)       (per clip: grad of the gate)
    GRAD_GATE_ADD = 2,    // d' = d * gate + add[n][c]               partials: sum d', sum d' * yhat
    GRAD_ACT_SUMS = 3,    // GRAD_ACT without the write-back of d': the same kernel instance, write_back = 0
    GRAD_GATE_STATS = 4,  // GRAD_GATE with the per-clip sums of the analytic squeeze-excite backward: sum d', sum d' * yhat, sum yhat
};
template <typename T, GradMode MODE>
__global__ __launch_bounds__(256) void grad_pass_kernel(T* __restrict__ d, const T* __restrict__ y, const float* __restrict__ stat,
                                                        const T* __restrict__ res, const float* __restrict__ gate, const float* __restrict__ add,
                                                        float* __restrict__ ws, int S, int Cp, int CG, int LPR, int rows_per_chunk,
                                                        int chunks, int act, int write_back, int gdiv) {
    static_assert(MODE != GRAD_ACT_SUMS, "GRAD_ACT with write_back = 0");
    __shared__ float red[256 * 8];
    const RowWalk<T> w(S, Cp, CG, LPR, rows_per_chunk);
    stat += (size_t)(w.n / gdiv) * 4 * Cp;  // this clip's statistics group
    constexpr int W = MODE == GRAD_GATE_STATS ? 3 : 2;
    constexpr int U = ROWS_U;
    float acc[W][8];
#pragma unroll
    for (int p = 0; p < W; ++p)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[p][j] = 0.0f;
    if (w.live) {
        float mean[8], invstd[8], sc[8], sh[8], g[8], ad[8];
        load8(stat + w.c0, mean);
        load8(stat + Cp + w.c0, invstd);
        load8(stat + 2 * Cp + w.c0, sc);
        load8(stat + 3 * Cp + w.c0, sh);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            g[j] = 1.0f;
            ad[j] = 0.0f;
        }
        if (gate) load8(gate + (size_t)w.n * Cp + w.c0, g);
        if (add) load8(add + (size_t)w.n * Cp + w.c0, ad);
        const __amdgpu_buffer_rsrc_t yrs = w.rows(y), drs = w.rows(d), qrs = w.rows((MODE == GRAD_ACT && res) ? res : y);
        w.batches([&](const RowBatch& b) {
            Raw8<T> yv[U], dr[U], qv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                yv[u] = load_raw8<T>(yrs, b.off[u]);
                dr[u] = load_raw8<T>(drs, b.off[u]);
            }
            if (MODE == GRAD_ACT && res) {
#pragma unroll
                for (int u = 0; u < U; ++u) qv[u] = load_raw8<T>(qrs, b.off[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float v[8], dv[8];
                raw_to_f8<T>(yv[u].r, v);
                raw_to_f8<T>(dr[u].r, dv);
                if (MODE == GRAD_ACT) {
                    float uu[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) uu[j] = fmaf(v[j], sc[j], sh[j]);
                    if (res) {
                        float q[8];
                        raw_to_f8<T>(qv[u].r, q);
#pragma unroll
                        for (int j = 0; j < 8; ++j) uu[j] += q[j];
                    }
                    act_grad_mul(dv, uu, act);
                } else if (MODE == GRAD_GATE) {
                    float uu[8], ug[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        uu[j] = fmaf(v[j], sc[j], sh[j]);
                        ug[j] = uu[j] * g[j];
                    }
                    act_grad_mul(dv, ug, act);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[0][j] = fmaf(dv[j], uu[j], acc[0][j]);  // (a row past the chunk: d = 0)
                } else if (MODE == GRAD_GATE_STATS) {
                    // as GRAD_GATE, but the sums the squeeze-excite unit's norm needs are taken here, per clip: (sum d', sum d' yhat, sum yhat).
                    // d'' = d' gate + add[n] is affine in d' per clip, so sum d'' and sum d'' yhat follow without a second pass over (d, y)
                    // (pasn_se_gate_bwd_stat), and sum d' u = gamma sum d' yhat + beta sum d' (the gate's gradient) as well
                    float ug[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) ug[j] = fmaf(v[j], sc[j], sh[j]) * g[j];
                    act_grad_mul(dv, ug, act);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float yc = v[j] - mean[j];  // (x invstd once, behind the loop)
                        acc[0][j] += dv[j];               // (a row past the chunk: d = 0, so d' = 0)
                        acc[1][j] = fmaf(dv[j], yc, acc[1][j]);
                        acc[W - 1][j] += b.in(u) ? yc : 0.0f;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) dv[j] = b.in(u) ? fmaf(dv[j], g[j], ad[j]) : 0.0f;  // (add[n][c] != 0: a row past the chunk must stay out of the sums)
                }
                if (MODE != GRAD_GATE && MODE != GRAD_GATE_STATS) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        acc[0][j] += dv[j];  // (a row past the chunk: d' = 0)
                        acc[1][j] = fmaf(dv[j], v[j] - mean[j], acc[1][j]);  // sum d' (y - mean); x invstd once, behind the loop
                    }
                }
                if (write_back) store8(drs, b.off[u], dv, (const T*)nullptr);
            }
        });
        // yhat = (y - mean) invstd: the factor invstd[c] is common to a thread's whole sum (the kernels are bound by vector issue, not bytes: 70-78 %
        // of the SIMD cycles carry a vector instruction; one multiply per element and sum less)
        if (MODE != GRAD_GATE) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                acc[1][j] *= invstd[j];
                if (MODE == GRAD_GATE_STATS) acc[W - 1][j] *= invstd[j];
            }
        }
    }
    block_reduce_rows<W>(acc, red, ws + ((size_t)w.n * chunks + blockIdx.x) * W * Cp, Cp, CG, LPR);
}

// totals of the mode 0 / 2 partials -> coef[g][2][Cp] = (sum d'/R, sum d' yhat / R) per statistics group, dgamma, dbeta (either may be NULL)
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ ws, float* __restrict__ coef, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta, int N, int S, int C, int Cp, int chunks, int gdiv) {
    // per statistics group g (clips n / gdiv): coef[g][2][Cp]; dgamma / dbeta are the parameter's: summed over the groups in order
    __shared__ float red[2][16][16];
    const int cl = threadIdx.x & 15, part = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    const bool live = c < Cp;
    const int G = N / gdiv;
    float dg = 0.0f, db = 0.0f;
    for (int g = 0; g < G; ++g) {
        float b1, b2;
        group_totals(ws, g, gdiv, chunks, Cp, c, live, red, b1, b2);
        if (part == 0 && live) {
            const float R = (float)gdiv * (float)S;
            coef[(size_t)g * 2 * Cp + c] = b1 / R;
            coef[(size_t)g * 2 * Cp + Cp + c] = b2 / R;
            dg += b2;
            db += b1;
        }
    }
    if (part == 0 && live && c < C) {
        if (dgamma) dgamma[c] = dg;
        if (dbeta) dbeta[c] = db;
    }
}

// The rows of both apply kernels: dy = s d' + bq (y - mean) + cq -- one subtraction and two FMAs per element -- with per-channel
// coefficients the kernel prepared; first(v, dv) is what the kernel does to d (given y) before that line.
template <typename T, typename First>
__device__ __forceinline__ void bn_apply_rows(const RowWalk<T>& w, const T* d, const T* y, T* dy, const float (&mean)[8], const float (&s)[8],
                                              const float (&bq)[8], const float (&cq)[8], First first) {
    const __amdgpu_buffer_rsrc_t yrs = w.rows(y), drs = w.rows(d), ors = w.rows(dy);
    w.batches([&](const RowBatch& b) {
        Raw8<T> yv[ROWS_U], dr[ROWS_U];
#pragma unroll
        for (int u = 0; u < ROWS_U; ++u) {
            yv[u] = load_raw8<T>(yrs, b.off[u]);
            dr[u] = load_raw8<T>(drs, b.off[u]);
        }
#pragma unroll
        for (int u = 0; u < ROWS_U; ++u) {
            float v[8], dv[8];
            raw_to_f8<T>(yv[u].r, v);
            raw_to_f8<T>(dr[u].r, dv);
            first(v, dv);
#pragma unroll
            for (int j = 0; j < 8; ++j) dv[j] = fmaf(s[j], dv[j], fmaf(bq[j], v[j] - mean[j], cq[j]));
            store8(ors, b.off[u], dv, (const T*)nullptr);
        }
    });
}

// dy = sc * (d' - m1 - yhat * m2),  d' = d (act == NONE: already differentiated by the reduce pass) or d * act'(y*sc + sh)
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ d, const T* __restrict__ y, const float* __restrict__ stat,
                                                           const float* __restrict__ coef, T* __restrict__ dy, int S, int Cp, int CG, int LPR,
                                                           int rows_per_chunk, int act, int gdiv) {
    const RowWalk<T> w(S, Cp, CG, LPR, rows_per_chunk);
    if (!w.live) return;
    stat += (size_t)(w.n / gdiv) * 4 * Cp;  // this clip's statistics group
    coef += (size_t)(w.n / gdiv) * 2 * Cp;
    float mean[8], invstd[8], sc[8], sh[8], m1[8], m2[8];
    load8(stat + w.c0, mean);
    load8(stat + Cp + w.c0, invstd);
    load8(stat + 2 * Cp + w.c0, sc);
    load8(stat + 3 * Cp + w.c0, sh);
    load8(coef + w.c0, m1);
    load8(coef + Cp + w.c0, m2);
    // dy = sc (d' - m1 - (y - mean) invstd m2) = sc d' + bq (y - mean) + cq
    float bq[8], cq[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        bq[j] = -sc[j] * invstd[j] * m2[j];
        cq[j] = -sc[j] * m1[j];
    }
    bn_apply_rows(w, d, y, dy, mean, sc, bq, cq, [&](const float (&v)[8], float (&dv)[8]) {
        if (act != PASN_ACT_NONE) {
            float uu[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) uu[j] = fmaf(v[j], sc[j], sh[j]);
            act_grad_mul(dv, uu, act);
        }
    });
}

// dy = sc * (d'' - m1 - yhat * m2) with d'' = d' * gate[n][c] + add[n][c] formed on the fly (d' as left by GRAD_GATE_STATS); no activation
// path in this instance (78 VGPRs against 114 in bf16)
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_se_kernel(const T* __restrict__ d, const T* __restrict__ y, const float* __restrict__ stat,
                                                              const float* __restrict__ coef, const float* __restrict__ gate,
                                                              const float* __restrict__ add, T* __restrict__ dy, int S, int Cp, int CG, int LPR,
                                                              int rows_per_chunk, int gdiv) {
    const RowWalk<T> w(S, Cp, CG, LPR, rows_per_chunk);
    if (!w.live) return;
    stat += (size_t)(w.n / gdiv) * 4 * Cp;  // this clip's statistics group
    coef += (size_t)(w.n / gdiv) * 2 * Cp;
    float mean[8], invstd[8], sc[8], m1[8], m2[8], g[8], ad[8];
    load8(stat + w.c0, mean);
    load8(stat + Cp + w.c0, invstd);
    load8(stat + 2 * Cp + w.c0, sc);
    load8(coef + w.c0, m1);
    load8(coef + Cp + w.c0, m2);
    load8(gate + (size_t)w.n * Cp + w.c0, g);
    load8(add + (size_t)w.n * Cp + w.c0, ad);
    // dy = sc (d' gate + add - m1 - (y - mean) invstd m2) = sg d' + bq (y - mean) + cq
    float sg[8], bq[8], cq[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        sg[j] = sc[j] * g[j];
        bq[j] = -sc[j] * invstd[j] * m2[j];
        cq[j] = sc[j] * (ad[j] - m1[j]);
    }
    bn_apply_rows(w, d, y, dy, mean, sg, bq, cq, [](const float (&)[8], float (&)[8]) {});
}

// ---- squeeze-excite backward (one block per clip) ---------------------------------------------------------------------
// a[k] = the sum over a clip's chunks, IN CHUNK ORDER, of row k < USED of its partials p[chunk][W][Cp] (p at the thread's channel).
// Batches of 8 chunks: 8 USED independent loads in flight, then the adds (a rolled load -> add loop is one L2 round trip per chunk: ~1 us x
// 32 chunks per launch, 15 launches per step).  common.h's sum_rows_in_order is the one-row form the forward gates use.
template <int W, int USED>
__device__ __forceinline__ void sum_chunks_in_order(const float* __restrict__ p, int chunks, int Cp, float (&a)[USED]) {
#pragma unroll
    for (int k = 0; k < USED; ++k) a[k] = 0.0f;
    for (int ch0 = 0; ch0 < chunks; ch0 += 8) {
        float t[USED][8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float* q = p + (size_t)min(ch0 + u, chunks - 1) * W * Cp;
#pragma unroll
            for (int k = 0; k < USED; ++k) t[k][u] = q[k * Cp];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (ch0 + u < chunks) {
#pragma unroll
                for (int k = 0; k < USED; ++k) a[k] += t[k][u];
            }
    }
}

// gate = sigmoid(w2 . relu(w1 . pool + b1) + b2).  In: dgate partials (mode 1), pool_u.  Out: add[n][c] = dpool[c] / S and
// this clip's parameter-gradient contributions pn[n][...] = (dw1 [Cse][C], db1 [Cse], dw2 [C][Cse], db2 [C]).
__global__ __launch_bounds__(256) void se_mlp_bwd_kernel(const float* __restrict__ ws, int chunks, const float* __restrict__ pool_u,
                                                         const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                                         const float* __restrict__ b2, float* __restrict__ add, float* __restrict__ pn, int S, int C,
                                                         int Cp, int Cse, const float* __restrict__ stat, float* __restrict__ ws3, int gdiv) {
    extern __shared__ float sm[];
    if (stat) stat += (size_t)(blockIdx.x / gdiv) * 4 * Cp;  // this clip's statistics group
    float* pool = sm;             // [C]
    float* ds = pool + C;         // [C]
    float* h = ds + C;            // [Cse]
    float* dh = h + Cse;          // [Cse]
    const int n = blockIdx.x, tid = threadIdx.x;
    for (int c = tid; c < C; c += 256) pool[c] = pool_u[(size_t)n * Cp + c];
    __syncthreads();
    // hidden units: 8 lanes share one dot product over the channels (shuffle combine in a fixed order)
    for (int j0 = 0; j0 < Cse; j0 += 32) {
        const int j = j0 + (tid >> 3), sub = tid & 7;
        float a = 0.0f;
        if (j < Cse)
#pragma unroll 8
            for (int c = sub; c < C; c += 8) a = fmaf(w1[(size_t)j * C + c], pool[c], a);
        a += __shfl_xor(a, 1);
        a += __shfl_xor(a, 2);
        a += __shfl_xor(a, 4);
        if (j < Cse && sub == 0) h[j] = fmaxf(a + b1[j], 0.0f);
    }
    __syncthreads();
    float* p = pn + (size_t)n * (2 * (size_t)C * Cse + Cse + C);
    float* p_w1 = p;
    float* p_b1 = p_w1 + (size_t)Cse * C;
    float* p_w2 = p_b1 + Cse;
    float* p_b2 = p_w2 + (size_t)C * Cse;
    for (int c = tid; c < C; c += 256) {
        float dg = 0.0f;
        if (stat) {
            // mode-4 partials [n][chunk][3][Cp]: clip totals (fixed order), left in chunk 0 for se_bn_coef_kernel; the gate's gradient
            // sum d' u with u = gamma yhat + beta
            float* q0 = ws3 + (size_t)n * chunks * 3 * Cp + c;
            float a[3];
            sum_chunks_in_order<3>(q0, chunks, Cp, a);
            q0[0] = a[0];
            q0[Cp] = a[1];
            q0[2 * Cp] = a[2];
            const float scv = stat[2 * Cp + c], gamma = scv / stat[Cp + c], beta = fmaf(stat[c], scv, stat[3 * Cp + c]);
            dg = fmaf(gamma, a[1], beta * a[0]);
        } else {
            float a[1];  // of the GRAD_GATE partials [n][chunk][2][Cp] only the first row is in use
            sum_chunks_in_order<2>(ws + (size_t)n * chunks * 2 * Cp + c, chunks, Cp, a);
            dg = a[0];
        }
        float a = b2[c];
#pragma unroll 8
        for (int j = 0; j < Cse; ++j) a = fmaf(w2[(size_t)c * Cse + j], h[j], a);
        const float g = 1.0f / (1.0f + expf(-a));
        const float d = dg * g * (1.0f - g);
        ds[c] = d;
        p_b2[c] = d;
#pragma unroll 8
        for (int j = 0; j < Cse; ++j) p_w2[(size_t)c * Cse + j] = d * h[j];
    }
    __syncthreads();
    for (int j0 = 0; j0 < Cse; j0 += 32) {
        const int j = j0 + (tid >> 3), sub = tid & 7;
        float a = 0.0f;
        if (j < Cse)
#pragma unroll 8
            for (int c = sub; c < C; c += 8) a = fmaf(w2[(size_t)c * Cse + j], ds[c], a);
        a += __shfl_xor(a, 1);
        a += __shfl_xor(a, 2);
        a += __shfl_xor(a, 4);
        if (j < Cse && sub == 0) {
            a = h[j] > 0.0f ? a : 0.0f;
            dh[j] = a;
            p_b1[j] = a;
        }
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        float a = 0.0f;
#pragma unroll 8
        for (int j = 0; j < Cse; ++j) {
            a = fmaf(w1[(size_t)j * C + c], dh[j], a);
            p_w1[(size_t)j * C + c] = dh[j] * pool[c];
        }
        add[(size_t)n * Cp + c] = a / (float)S;
    }
    for (int c = C + tid; c < Cp; c += 256) add[(size_t)n * Cp + c] = 0.0f;
}

// The per-clip parameter-gradient contributions pn[n][dw1 | db1 | dw2 | db2] summed over the clips (fixed order), each
// segment into its own gradient tensor -- one launch for the four.
__global__ __launch_bounds__(256) void se_sum_over_clips_kernel(const float* __restrict__ pn, float* __restrict__ dw1, float* __restrict__ db1,
                                                                float* __restrict__ dw2, float* __restrict__ db2, int N, int C, int Cse) {
    const size_t o_b1 = (size_t)Cse * C, o_w2 = o_b1 + Cse, o_b2 = o_w2 + (size_t)C * Cse, len = o_b2 + C;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    float s = 0.0f;
#pragma unroll 8
    for (int n = 0; n < N; ++n) s += pn[(size_t)n * len + i];
    if (i < o_b1) dw1[i] = s;
    else if (i < o_w2) db1[i - o_b1] = s;
    else if (i < o_b2) dw2[i - o_w2] = s;
    else db2[i - o_b2] = s;
}

// coef / dgamma / dbeta of a squeeze-excite unit's norm from the per-clip totals (A1, A2, A3) = (sum d', sum d' yhat, sum yhat) that
// se_mlp_bwd_kernel left in chunk 0 of the mode-4 partials:  sum d'' = sum_n gate A1 + S add,  sum d'' yhat = sum_n gate A2 + add A3.
__global__ __launch_bounds__(256) void se_bn_coef_kernel(const float* __restrict__ ws3, int chunks, const float* __restrict__ gate,
                                                         const float* __restrict__ add, float* __restrict__ coef, float* __restrict__ dgamma,
                                                         float* __restrict__ dbeta, int N, int S, int C, int Cp, int gdiv) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= Cp) return;
    float dg = 0.0f, db = 0.0f;
    for (int lo = 0; lo < N; lo += gdiv) {  // one statistics group after the other
        const int hi = lo + gdiv;
        float b1 = 0.0f, b2 = 0.0f;
        for (int n0 = lo; n0 < hi; n0 += 8) {  // 8 clips' loads in flight, the sums in clip order
            float q0[8], q1[8], q2[8], g[8], a[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int n = min(n0 + u, hi - 1);
                const float* q = ws3 + (size_t)n * chunks * 3 * Cp + c;
                q0[u] = q[0];
                q1[u] = q[Cp];
                q2[u] = q[2 * Cp];
                g[u] = gate[(size_t)n * Cp + c];
                a[u] = add[(size_t)n * Cp + c];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (n0 + u < hi) {
                    b1 += fmaf(g[u], q0[u], (float)S * a[u]);
                    b2 += fmaf(g[u], q1[u], a[u] * q2[u]);
                }
        }
        const float R = (float)gdiv * (float)S;
        float* cf = coef + (size_t)(lo / gdiv) * 2 * Cp;
        cf[c] = b1 / R;
        cf[Cp + c] = b2 / R;
        dg += b2;
        db += b1;
    }
    if (c < C) {
        if (dgamma) dgamma[c] = dg;
        if (dbeta) dbeta[c] = db;
    }
}

// element i of a grid-stride pass over [N][T][H][W][CG] 8-channel groups: its channel group, position and row (n, t, h, w)
struct CgRow {
    int cg, w, h, t, n;
    size_t row;
};
__device__ __forceinline__ CgRow split_cg_row(size_t i, int CG, int W, int H, int T) {
    const size_t row = i / CG, q = row / W, p = q / H;
    return {(int)(i % CG), (int)(row % W), (int)(q % H), (int)(p % T), (int)(p / T), row};
}

// ---- strided scatter: dst[n][t*st][h*sh][w*sw][:] (+)= src[n][t][h][w][:], every other element 0 (or kept) -------------
template <typename T>
__global__ __launch_bounds__(256) void scatter_strided_kernel(const T* __restrict__ src, T* __restrict__ dst, int N, int To, int Ho, int Wo,
                                                              int Ti, int Hi, int Wi, int st, int sh, int sw, int Cp, int accumulate) {
    const int CG = Cp / 8;
    const size_t total = (size_t)N * Ti * Hi * Wi * CG;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const auto [cg, w, h, t, n, row] = split_cg_row(i, CG, Wi, Hi, Ti);
        const bool on = (t % st == 0) && (h % sh == 0) && (w % sw == 0) && (t / st < To) && (h / sh < Ho) && (w / sw < Wo);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 0.0f;
        T* o = dst + row * Cp + cg * 8;
        if (on) {
            load8(src + ((((size_t)n * To + t / st) * Ho + h / sh) * Wo + w / sw) * Cp + cg * 8, v);
            if (accumulate) {
                float e[8];
                load8(o, e);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] += e[j];
            }
            store8(o, v);
        } else if (!accumulate) {
            store8(o, v);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void add_inplace_kernel(T* __restrict__ a, const T* __restrict__ b, size_t groups) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < groups; i += (size_t)gridDim.x * 256) {
        float x[8], y[8];
        load8(a + i * 8, x);
        load8(b + i * 8, y);
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] += y[j];
        store8(a + i * 8, x);
    }
}

// ---- max-pool backward (gather form, no atomics): an input element receives dy of every window whose FIRST maximum (scan
// order t, h, w -- the index torch's forward records) it is ------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx, pasn_conv_desc d) {
    const int CG = d.Cin_p / 8;
    const size_t total = (size_t)d.N * d.Ti * d.Hi * d.Wi * CG;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const auto [cg, wi, hi, ti, n, row] = split_cg_row(i, CG, d.Wi, d.Hi, d.Ti);
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
        const T* xn = x + (size_t)n * d.Ti * d.Hi * d.Wi * d.Cin_p + cg * 8;
        for (int to = max(0, (ti + d.pt - d.kt + d.st) / d.st); to <= min(d.To - 1, (ti + d.pt) / d.st); ++to)
            for (int ho = max(0, (hi + d.ph - d.kh + d.sh) / d.sh); ho <= min(d.Ho - 1, (hi + d.ph) / d.sh); ++ho)
                for (int wo = max(0, (wi + d.pw - d.kw + d.sw) / d.sw); wo <= min(d.Wo - 1, (wi + d.pw) / d.sw); ++wo) {
                    float best[8];
                    int bidx[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        best[j] = -INFINITY;
                        bidx[j] = -1;
                    }
                    for (int a = 0; a < d.kt; ++a)
                        for (int b = 0; b < d.kh; ++b)
                            for (int c = 0; c < d.kw; ++c) {
                                const int t2 = to * d.st - d.pt + a, h2 = ho * d.sh - d.ph + b, w2 = wo * d.sw - d.pw + c;
                                if (t2 < 0 || t2 >= d.Ti || h2 < 0 || h2 >= d.Hi || w2 < 0 || w2 >= d.Wi) continue;
                                const int lin = (t2 * d.Hi + h2) * d.Wi + w2;
                                float v[8];
                                load8(xn + (size_t)lin * d.Cin_p, v);
#pragma unroll
                                for (int j = 0; j < 8; ++j)
                                    if (v[j] > best[j] || (v[j] != v[j] && bidx[j] < 0)) {
                                        best[j] = v[j];
                                        bidx[j] = lin;
                                    }
                            }
                    const int me = (ti * d.Hi + hi) * d.Wi + wi;
                    float g[8];
                    load8(dy + ((((size_t)n * d.To + to) * d.Ho + ho) * d.Wo + wo) * d.Cout_p + cg * 8, g);
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (bidx[j] == me) acc[j] += g[j];
                }
        store8(dx + row * d.Cin_p + cg * 8, acc);
    }
}

}  // namespace pasn

using namespace pasn;

#define GROUPS_OK(fn, N, groups) \
    PASN_REQUIRE_AS(fn, (groups) >= 1 && (groups) <= PASN_MAX_GROUPS && (N) % (groups) == 0, "statistics groups must divide the batch (1 .. 4)")

// What every entry of the row passes checks and works out before it launches: the extents, the statistics groups, then the geometry, the
// grid of a row pass (chunk, clip), the clips per group and the stream.
struct RowPlan {
    RowGeom g;
    dim3 grid;
    int gdiv;
    hipStream_t s;
};
static int row_plan(const char* fn, int N, int S, int C, int Cp, int groups, void* stream, RowPlan& p) {
    PASN_REQUIRE_AS(fn, N > 0 && S > 0 && C > 0 && Cp >= C && Cp % 8 == 0, "bad tensor extents");
    PASN_REQUIRE_AS(fn, Cp <= 2048, "channel stride above 2048 is not covered");
    PASN_REQUIRE_AS(fn, (long)S * Cp * 4 < 2147483648L, "one clip's rows must stay below 2 GiB (32-bit offsets inside a clip)");
    GROUPS_OK(fn, N, groups);
    p.g = row_geom(N, S, Cp);
    p.grid = dim3(p.g.chunks, N);
    p.gdiv = N / groups;
    p.s = (hipStream_t)stream;
    return PASN_OK;
}

extern "C" int pasn_train_chunks(int N, int S, int Cp) {
    if (N <= 0 || S <= 0 || Cp <= 0 || Cp % 8 || Cp > 2048) return 0;
    return row_geom(N, S, Cp).chunks;
}

extern "C" int pasn_bn_stats_fwd(const void* y, float* ws, const float* gamma, const float* beta, float* running_mean,
                                 float* running_var, float momentum, float eps, float* stat, float* pool_u, int N, int S, int C,
                                 int Cp, int dtype, void* stream) {
    return pasn_bn_stats_fwd_g(y, ws, gamma, beta, running_mean, running_var, momentum, eps, stat, pool_u, N, S, C, Cp, dtype, 1, stream);
}

// ... with `groups` statistics groups of N / groups consecutive clips each: stat[groups][4][Cp]; running estimates updated group by group
extern "C" int pasn_bn_stats_fwd_g(const void* y, float* ws, const float* gamma, const float* beta, float* running_mean,
                                   float* running_var, float momentum, float eps, float* stat, float* pool_u, int N, int S, int C,
                                   int Cp, int dtype, int groups, void* stream) {
    RowPlan p;
    if (const int rc = row_plan(__func__, N, S, C, Cp, groups, stream, p)) return rc;
    PASN_REQUIRE(y && ws && stat, "null pointer");
    PASN_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "running_mean / running_var go together");
    with_dtype(dtype, [&](auto tag) {
        using T = elem_t<decltype(tag)>;
        launch256(bn_stats_partial_kernel<T>, p.grid, 0, p.s, (const T*)y, ws, S, Cp, p.g.CG, p.g.LPR, p.g.rows_per_chunk, p.g.chunks);
        launch256(bn_finalize_kernel<T>, dim3(ceil_div(Cp, 16)), 0, p.s, ws, (const T*)y, gamma, beta, running_mean, running_var, momentum, eps,
                  stat, pool_u, N, S, C, Cp, p.g.chunks, (const float*)nullptr, p.gdiv);
    });
    return check_launch("bn_stats_fwd");
}

// Depthwise stencil + batch statistics in ONE pass over y (the X3D conv_b units): the T-marching stencil accumulates sum / sum of squares
// of its fp32 outputs per block, bn_finalize_kernel turns the [N][rows][2][Cp] partials into the unit's statistics table.  Saves the
// read of y by pasn_bn_stats_fwd (27 launches, ~1 ms of the X3D-S step).  Unshifted second moments: var = E[y^2] - mean^2 in fp32 over
// per-block fp32 partials -- a conv output without bias has |mean| ~ std.
extern "C" int pasn_dwconv3d_stats_rows(const pasn_conv_desc* d, int dtype) {
    if (!d || d->Cout_p <= 0 || d->Cout_p % 8 != 0 || d->Cout_p > 2048) return 0;
    if (const char* e = tune("PASN_NO_DW_STATS"))
        if (e[0] == '1') return 0;
    // stride-1 layers: the matrix-core stencil with the statistics epilogue (one partial row pair per (clip, chunk)); PASN_DW_STATS_MFMA=0: the
    // VALU stencil everywhere, as before round 3
    if (!(tune("PASN_DW_STATS_MFMA") && tune("PASN_DW_STATS_MFMA")[0] == '0'))
        if (const DwMfmaGeom mf = dw_mfma_geom(*d, dtype); mf.ok && !mf.abl) return mf.chunks;
    const DwMarchGeom m = dw_march_geom(*d, dtype);
    return m.WT ? m.bpc : 0;
}

extern "C" int pasn_dwconv3d_stats_fwd(const void* x, const float* w, const float* scale, const float* bias, void* y, float* ws, const float* gamma, const float* beta,
                                       float* running_mean, float* running_var, float momentum, float eps, float* stat, float* pool_u,
                                       const pasn_conv_desc* d, int dtype, void* stream) {
    return pasn_dwconv3d_stats_fwd_g(x, w, scale, bias, y, ws, gamma, beta, running_mean, running_var, momentum, eps, stat, pool_u, d, dtype, 1, stream);
}

extern "C" int pasn_dwconv3d_stats_fwd_g(const void* x, const float* w, const float* scale, const float* bias, void* y, float* ws, const float* gamma, const float* beta,
                                         float* running_mean, float* running_var, float momentum, float eps, float* stat, float* pool_u,
                                         const pasn_conv_desc* d, int dtype, int groups, void* stream) {
    PASN_REQUIRE(x && w && scale && bias && y && ws && stat && d, "null pointer");
    GROUPS_OK(__func__, d->N, groups);
    PASN_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "running_mean / running_var go together");
    PASN_REQUIRE(d->act == PASN_ACT_NONE, "the training stencil writes the raw conv output");
    const int rows = pasn_dwconv3d_stats_rows(d, dtype);
    PASN_REQUIRE(rows > 0, "layer not covered (pasn_dwconv3d_stats_rows returns 0)");
    hipStream_t s = (hipStream_t)stream;
    const int Cp = d->Cout_p, S = d->To * d->Ho * d->Wo;
    int rc;
    const DwMfmaGeom mf = dw_mfma_geom(*d, dtype);
    if (mf.ok && !mf.abl && mf.chunks == rows && !(tune("PASN_DW_STATS_MFMA") && tune("PASN_DW_STATS_MFMA")[0] == '0')) {
        rc = launch_dw_mfma(x, w, scale, bias, y, ws, *d, mf, s, 1, running_mean);  // moments shifted by the running mean (as it stands now:
    } else {                                                                           // the finalize kernel reads it before updating it)
        const DwMarchGeom m = dw_march_geom(*d, dtype);
        rc = launch_dw_march(x, w, scale, bias, y, ws, *d, m, s, DwSeArgs{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0}, 1, nullptr, running_mean);
    }
    if (rc) return rc;
    hipLaunchKernelGGL(bn_finalize_kernel<__bf16>, dim3(ceil_div(Cp, 16)), dim3(256), 0, s, ws, (const __bf16*)nullptr, gamma, beta, running_mean,
                       running_var, momentum, eps, stat, pool_u, d->N, S, d->Cout, Cp, rows, (const float*)running_mean, d->N / groups);
    return check_launch("dwconv3d_stats_fwd");
}

// Input gradient of a stride-1 "same" depthwise conv (the forward stencil with reversed taps) AND the backward sums of the unit that
// produced the conv's input, in one pass: replaces pasn_dwconv3d_fwd (as dgrad) + pasn_unit_bwd_reduce(mode 3) of the X3D conv_a units.
extern "C" int pasn_dwconv3d_dgrad_reduce_rows(const pasn_conv_desc* d, int dtype) {
    if (!d || d->sw != 1 || d->sh != 1) return 0;
    // OPT-IN (PASN_DW_DGRAD_REDUCE=1): measured, the fusion does not pay -- the stencil is bound by vector-instruction issue, and the ~25
    // extra instructions per output vector cost what the separate pass did (X3D-S: 22 launches 2.31 ms fused vs 1.37 + 0.87 ms)
    const char* on = tune("PASN_DW_DGRAD_REDUCE");
    if (!on || on[0] != '1') return 0;
    if (pasn_dwconv3d_stats_rows(d, dtype) == 0) return 0;
    const DwMarchGeom m = dw_march_geom(*d, dtype);
    return dw_march_red_ok(*d, m) ? m.bpc : 0;
}

extern "C" int pasn_dwconv3d_dgrad_reduce(const void* dy, const float* w_flipped, const float* scale, const float* bias, void* dx,
                                          const void* y_prev, const float* stat_prev, int act_prev, float* ws, float* coef, float* dgamma,
                                          float* dbeta, const pasn_conv_desc* d, int dtype, void* stream) {
    PASN_REQUIRE(dy && w_flipped && scale && bias && dx && y_prev && stat_prev && ws && coef && d, "null pointer");
    PASN_REQUIRE(d->act == PASN_ACT_NONE, "a gradient pass has no activation");
    const int rows = pasn_dwconv3d_dgrad_reduce_rows(d, dtype);
    PASN_REQUIRE(rows > 0, "layer not covered (pasn_dwconv3d_dgrad_reduce_rows returns 0)");
    hipStream_t s = (hipStream_t)stream;
    const int Cp = d->Cout_p, S = d->To * d->Ho * d->Wo;
    const DwMarchGeom m = dw_march_geom(*d, dtype);
    const DwRedArgs rd = {y_prev, stat_prev, act_prev};
    const int rc = launch_dw_march(dy, w_flipped, scale, bias, dx, ws, *d, m, s, DwSeArgs{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0}, 1, &rd);
    if (rc) return rc;
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(ceil_div(Cp, 16)), dim3(256), 0, s, ws, coef, dgamma, dbeta, d->N, S, d->Cout, Cp, rows, d->N);
    return check_launch("dwconv3d_dgrad_reduce");
}

extern "C" int pasn_affine_act_fwd(const void* y, const float* stat, const void* residual, const float* gate, void* a, int N, int S,
                                   int C, int Cp, int act, int dtype, void* stream) {
    return pasn_affine_act_fwd_g(y, stat, residual, gate, a, N, S, C, Cp, act, dtype, 1, stream);
}

extern "C" int pasn_affine_act_fwd_g(const void* y, const float* stat, const void* residual, const float* gate, void* a, int N, int S,
                                     int C, int Cp, int act, int dtype, int groups, void* stream) {
    RowPlan p;
    if (const int rc = row_plan(__func__, N, S, C, Cp, groups, stream, p)) return rc;
    PASN_REQUIRE(y && stat && a, "null pointer");
    with_dtype(dtype, [&](auto tag) {
        using T = elem_t<decltype(tag)>;
        launch256(affine_act_fwd_kernel<T>, p.grid, 0, p.s, (const T*)y, stat, (const T*)residual, gate, (T*)a, S, Cp, p.g.CG, p.g.LPR, p.g.rows_per_chunk,
                  act, p.gdiv);
    });
    return check_launch("affine_act_fwd");
}

extern "C" int pasn_unit_bwd_reduce(int mode, void* d, const void* y, const float* stat, const void* residual, const float* gate,
                                    const float* add, float* ws, float* coef, float* dgamma, float* dbeta, int N, int S, int C, int Cp,
                                    int act, int dtype, void* stream) {
    return pasn_unit_bwd_reduce_g(mode, d, y, stat, residual, gate, add, ws, coef, dgamma, dbeta, N, S, C, Cp, act, dtype, 1, stream);
}

extern "C" int pasn_unit_bwd_reduce_g(int mode, void* d, const void* y, const float* stat, const void* residual, const float* gate,
                                      const float* add, float* ws, float* coef, float* dgamma, float* dbeta, int N, int S, int C, int Cp,
                                      int act, int dtype, int groups, void* stream) {
    RowPlan p;
    if (const int rc = row_plan(__func__, N, S, C, Cp, groups, stream, p)) return rc;
    PASN_REQUIRE(mode >= 0 && mode <= 4, "mode must be 0 .. 4");
    PASN_REQUIRE(d && y && stat && ws, "null pointer");
    const bool gate_grad = mode == GRAD_GATE || mode == GRAD_GATE_STATS, act_only = mode == GRAD_ACT || mode == GRAD_ACT_SUMS;
    PASN_REQUIRE(gate_grad || coef, "coef is required for modes 0, 2 and 3");
    PASN_REQUIRE(act_only || gate, "modes 1, 2 and 4 need the gate");
    PASN_REQUIRE(mode != GRAD_ACT_SUMS || residual == nullptr, "mode 3 leaves d untouched: a residual branch needs the differentiated d of mode 0");
    with_dtype(dtype, [&](auto tag) {
        using T = elem_t<decltype(tag)>;
        launch256(act_only ? grad_pass_kernel<T, GRAD_ACT> : mode == GRAD_GATE ? grad_pass_kernel<T, GRAD_GATE>
                  : mode == GRAD_GATE_STATS ? grad_pass_kernel<T, GRAD_GATE_STATS> : grad_pass_kernel<T, GRAD_GATE_ADD>,
                  p.grid, 0, p.s, (T*)d, (const T*)y, stat, (const T*)residual, gate, add, ws, S, Cp, p.g.CG, p.g.LPR, p.g.rows_per_chunk, p.g.chunks, act,
                  (int)(mode != GRAD_ACT_SUMS), p.gdiv);
    });
    if (!gate_grad) launch256(bn_bwd_finalize_kernel, dim3(ceil_div(Cp, 16)), 0, p.s, ws, coef, dgamma, dbeta, N, S, C, Cp, p.g.chunks, p.gdiv);
    return check_launch("unit_bwd_reduce");
}

extern "C" int pasn_bn_bwd_apply(const void* d, const void* y, const float* stat, const float* coef, void* dy, int N, int S, int C, int Cp,
                                 int act, int dtype, void* stream) {
    return pasn_bn_bwd_apply_g(d, y, stat, coef, dy, N, S, C, Cp, act, dtype, 1, stream);
}

extern "C" int pasn_bn_bwd_apply_g(const void* d, const void* y, const float* stat, const float* coef, void* dy, int N, int S, int C, int Cp,
                                   int act, int dtype, int groups, void* stream) {
    RowPlan p;
    if (const int rc = row_plan(__func__, N, S, C, Cp, groups, stream, p)) return rc;
    PASN_REQUIRE(d && y && stat && coef && dy, "null pointer");
    with_dtype(dtype, [&](auto tag) {
        using T = elem_t<decltype(tag)>;
        launch256(bn_bwd_apply_kernel<T>, p.grid, 0, p.s, (const T*)d, (const T*)y, stat, coef, (T*)dy, S, Cp, p.g.CG, p.g.LPR, p.g.rows_per_chunk, act, p.gdiv);
    });
    return check_launch("bn_bwd_apply");
}

extern "C" size_t pasn_se_bwd_workspace_floats(int N, int C, int Cse) { return (size_t)N * (2 * (size_t)C * Cse + Cse + C); }

extern "C" int pasn_se_gate_bwd(const float* ws, const float* pool_u, const float* w1, const float* b1, const float* w2, const float* b2,
                                float* add, float* pn, float* dw1, float* db1, float* dw2, float* db2, int N, int S, int C, int Cp, int Cse,
                                void* stream) {
    const int groups = 1;  // (no statistics enter this form)
    RowPlan p;
    if (const int rc = row_plan(__func__, N, S, C, Cp, groups, stream, p)) return rc;
    PASN_REQUIRE(Cse > 0 && ws && pool_u && w1 && b1 && w2 && b2 && add && pn && dw1 && db1 && dw2 && db2, "null pointer");
    const size_t lds = (2 * (size_t)C + 2 * Cse) * sizeof(float);
    PASN_REQUIRE(lds <= 64 * 1024, "squeeze-excite width above the LDS budget");
    launch256(se_mlp_bwd_kernel, dim3(N), lds, p.s, ws, p.g.chunks, pool_u, w1, b1, w2, b2, add, pn, S, C, Cp, Cse, (const float*)nullptr, (float*)nullptr, N);
    const size_t len = 2 * (size_t)C * Cse + Cse + C;
    launch256(se_sum_over_clips_kernel, dim3(ceil_div((long)len, 256)), 0, p.s, pn, dw1, db1, dw2, db2, N, C, Cse);
    return check_launch("se_gate_bwd");
}

extern "C" int pasn_se_gate_bwd_stat(float* ws3, const float* pool_u, const float* stat, const float* gate, const float* w1, const float* b1,
                                     const float* w2, const float* b2, float* add, float* pn, float* dw1, float* db1, float* dw2, float* db2,
                                     float* coef, float* dgamma, float* dbeta, int N, int S, int C, int Cp, int Cse, void* stream) {
    return pasn_se_gate_bwd_stat_g(ws3, pool_u, stat, gate, w1, b1, w2, b2, add, pn, dw1, db1, dw2, db2, coef, dgamma, dbeta, N, S, C, Cp, Cse, 1, stream);
}

extern "C" int pasn_se_gate_bwd_stat_g(float* ws3, const float* pool_u, const float* stat, const float* gate, const float* w1, const float* b1,
                                       const float* w2, const float* b2, float* add, float* pn, float* dw1, float* db1, float* dw2, float* db2,
                                       float* coef, float* dgamma, float* dbeta, int N, int S, int C, int Cp, int Cse, int groups, void* stream) {
    RowPlan p;
    if (const int rc = row_plan(__func__, N, S, C, Cp, groups, stream, p)) return rc;
    PASN_REQUIRE(Cse > 0 && ws3 && pool_u && stat && gate && w1 && b1 && w2 && b2 && add && pn && dw1 && db1 && dw2 && db2 && coef, "null pointer");
    const size_t lds = (2 * (size_t)C + 2 * Cse) * sizeof(float);
    PASN_REQUIRE(lds <= 64 * 1024, "squeeze-excite width above the LDS budget");
    launch256(se_mlp_bwd_kernel, dim3(N), lds, p.s, (const float*)nullptr, p.g.chunks, pool_u, w1, b1, w2, b2, add, pn, S, C, Cp, Cse, stat, ws3, p.gdiv);
    const size_t len = 2 * (size_t)C * Cse + Cse + C;
    launch256(se_sum_over_clips_kernel, dim3(ceil_div((long)len, 256)), 0, p.s, pn, dw1, db1, dw2, db2, N, C, Cse);
    launch256(se_bn_coef_kernel, dim3(ceil_div(Cp, 256)), 0, p.s, ws3, p.g.chunks, gate, add, coef, dgamma, dbeta, N, S, C, Cp, p.gdiv);
    return check_launch("se_gate_bwd_stat");
}

extern "C" int pasn_bn_bwd_apply_se(const void* d, const void* y, const float* stat, const float* coef, const float* gate, const float* add,
                                    void* dy, int N, int S, int C, int Cp, int dtype, void* stream) {
    return pasn_bn_bwd_apply_se_g(d, y, stat, coef, gate, add, dy, N, S, C, Cp, dtype, 1, stream);
}

extern "C" int pasn_bn_bwd_apply_se_g(const void* d, const void* y, const float* stat, const float* coef, const float* gate, const float* add,
                                      void* dy, int N, int S, int C, int Cp, int dtype, int groups, void* stream) {
    RowPlan p;
    if (const int rc = row_plan(__func__, N, S, C, Cp, groups, stream, p)) return rc;
    PASN_REQUIRE(d && y && stat && coef && gate && add && dy, "null pointer");
    with_dtype(dtype, [&](auto tag) {
        using T = elem_t<decltype(tag)>;
        launch256(bn_bwd_apply_se_kernel<T>, p.grid, 0, p.s, (const T*)d, (const T*)y, stat, coef, gate, add, (T*)dy, S, Cp, p.g.CG, p.g.LPR, p.g.rows_per_chunk,
                  p.gdiv);
    });
    return check_launch("bn_bwd_apply_se");
}

extern "C" int pasn_scatter_strided(const void* src, void* dst, const pasn_conv_desc* d, int accumulate, int dtype, void* stream) {
    PASN_REQUIRE(src && dst && d, "null pointer");
    // src: [N][To][Ho][Wo][Cin_p] (compact), dst: [N][Ti][Hi][Wi][Cin_p]; element (t,h,w) of src lands on (t*st, h*sh, w*sw)
    PASN_REQUIRE(d->Cin_p % 8 == 0 && d->st > 0 && d->sh > 0 && d->sw > 0, "bad descriptor");
    PASN_REQUIRE((d->To - 1) * d->st < d->Ti && (d->Ho - 1) * d->sh < d->Hi && (d->Wo - 1) * d->sw < d->Wi, "source does not fit the target");
    const size_t total = (size_t)d->N * d->Ti * d->Hi * d->Wi * (d->Cin_p / 8);
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 65536);
    with_dtype(dtype, [&](auto tag) {
        using T = elem_t<decltype(tag)>;
        launch256(scatter_strided_kernel<T>, dim3(blocks), 0, (hipStream_t)stream, (const T*)src, (T*)dst, d->N, d->To, d->Ho, d->Wo, d->Ti, d->Hi, d->Wi, d->st,
                  d->sh, d->sw, d->Cin_p, accumulate);
    });
    return check_launch("scatter_strided");
}

extern "C" int pasn_add_inplace(void* a, const void* b, size_t elements, int dtype, void* stream) {
    PASN_REQUIRE(a && b && elements % 8 == 0, "element count must be a multiple of 8");
    const size_t groups = elements / 8;
    const int blocks = (int)std::min<size_t>((groups + 255) / 256, 65536);
    with_dtype(dtype, [&](auto tag) {
        using T = elem_t<decltype(tag)>;
        launch256(add_inplace_kernel<T>, dim3(blocks), 0, (hipStream_t)stream, (T*)a, (const T*)b, groups);
    });
    return check_launch("add_inplace");
}

extern "C" int pasn_maxpool3d_bwd(const void* x, const void* dy, void* dx, const pasn_conv_desc* d, int dtype, void* stream) {
    PASN_REQUIRE(x && dy && dx && d, "null pointer");
    PASN_REQUIRE(d->Cin_p == d->Cout_p && d->Cin_p % 8 == 0, "pooling keeps the channel stride");
    const size_t total = (size_t)d->N * d->Ti * d->Hi * d->Wi * (d->Cin_p / 8);
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 1 << 20);
    with_dtype(dtype, [&](auto tag) {
        using T = elem_t<decltype(tag)>;
        launch256(maxpool_bwd_kernel<T>, dim3(blocks), 0, (hipStream_t)stream, (const T*)x, (const T*)dy, (T*)dx, *d);
    });
    return check_launch("maxpool3d_bwd");
}
