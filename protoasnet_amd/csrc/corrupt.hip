// corrupt.hip -- robustness.py: echo-style corruptions of a normalised clip and the stability of a prediction and its explanation under
// them.  include/protoasnet_amd.h holds the definitions, tests/robustness_cases.py their numpy restatement.
//
// pasn_clip_corrupt: one launch.  A block owns a 32 x 64 tile of one (n, t) plane and walks the C channels.  Every fp32 operation of the
// definition is rounded on its own (no contraction in this file), so numpy reproduces the output bit for bit.
//   noise   z of the tile's voxels (Philox, shared by the channels) goes into LDS once, before the channel loop
//   blur    per channel: the tile with its R-wide halo, in the pixel domain, into LDS (edge replication = clamped source coordinates);
//           the row pass into a second LDS image; the column pass, photometric stage, noise, clamp and normalisation into the first one;
//           then the store pass below
//   plain   (R = 0) the store pass computes its own elements: 16-byte loads where the source address allows
//   store   a tile row is cut on the 16-byte grid of its OUTPUT address (rows are misaligned whenever W is no multiple of the vector):
//           slot 0 is the row's head, the last slot its tail, both element by element; every slot between is one 16-byte store
// pasn_stability_stats: clip kernel (one wave per clip: predictions, fp64 softmax statistics, the two top-k selections), pair kernel (one
// block per (n, j): both maps in LDS, fp64 moments in index order by one lane each, ranks by counting), then one block adds onto acc.
#include "common.h"
#include "eval_common.h"
#include "explain_common.h"
#include "philox.h"

#pragma clang fp contract(off)

namespace pasn {

constexpr int CR_NT = 256, CR_TH = 32, CR_TW = 64, CR_RMAX = 8, CR_VW = CR_TW + 2 * CR_RMAX, CR_VH = CR_TH + 2 * CR_RMAX;
constexpr float CR_ZC = (float)(1.7320508075688772 / 16777216.0);  // the fp32 nearest sqrt(3) 2^-24
constexpr int ST_NT = 256, ST_MAX_S = 4096, ST_MAX_P = 16384;

struct CorruptArgs {
    const void* x;
    void* y;
    const int32_t* src_t;
    const float *taps, *row_a, *row_b;
    int N, C, T, H, W, R, tilesH, tilesW;
    float sigma_add, sigma_mul, mean, stdv;
    uint32_t k0, k1;
    int copy, photo, noise;
};

// The Irwin-Hall(4) variate of output voxel q of clip n: integers and one conversion, then one product.  NOT a Gaussian.
__device__ __forceinline__ float cr_z(uint32_t k0, uint32_t k1, long q, int n) {
    uint32_t r[4];
    philox4x32_10((uint32_t)q, (uint32_t)((uint64_t)q >> 32), (uint32_t)n, 0u, k0, k1, r);
    const int32_t s = (int32_t)((r[0] >> 8) + (r[1] >> 8) + (r[2] >> 8) + (r[3] >> 8)) - 33554430;
    return (float)s * CR_ZC;
}

// steps 5 - 8 of the definition on a pixel-domain value; returns the normalised value before its rounding to the dtype (raw_narrow: no
// NaN can arrive there, the clamp removed it)
__device__ __forceinline__ float cr_finish(const CorruptArgs& a, float v, float ra, float rb, float z) {
    if (a.photo) v = ra * v + rb;
    if (a.sigma_add != 0.0f) v = v + a.sigma_add * z;
    if (a.sigma_mul != 0.0f) v = v + (a.sigma_mul * z) * v;
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    return __fdiv_rn(v - a.mean, a.stdv);
}

// BLUR: the separable blur instance (1 <= R <= 8); else R = 0.  U: the element as raw bits.
template <typename U, bool BLUR>
__global__ __launch_bounds__(CR_NT) void clip_corrupt_kernel(CorruptArgs a) {
    constexpr int EPV = 16 / (int)sizeof(U), NSLOT = CR_TW / EPV + 1;
    __shared__ float s_z[CR_TH * CR_TW];
    __shared__ float s_v[BLUR ? CR_VH * CR_VW : 1];  // the pixel-domain tile with its halo; after the row pass: the finished values
    __shared__ float s_g[BLUR ? CR_VH * CR_TW : 1];  // the row pass
    __shared__ float s_taps[2 * CR_RMAX + 1];
    const int tid = threadIdx.x;
    const int H = a.H, W = a.W, T = a.T, R = BLUR ? a.R : 0;
    long b = blockIdx.x;
    const int tw = (int)(b % a.tilesW);
    b /= a.tilesW;
    const int th = (int)(b % a.tilesH);
    b /= a.tilesH;
    const int t = (int)(b % T), n = (int)(b / T);
    const int h0 = th * CR_TH, w0 = tw * CR_TW;
    const int rows = min(CR_TH, H - h0), cols = min(CR_TW, W - w0);
    int ts = t;
    if (a.src_t) ts = min(max(a.src_t[(long)n * T + t], 0), T - 1);
    if (a.noise) {
        for (int i = tid; i < CR_TH * CR_TW; i += CR_NT) {
            const int r = i / CR_TW, w = i % CR_TW;
            if (r < rows && w < cols) s_z[i] = cr_z(a.k0, a.k1, ((long)t * H + (h0 + r)) * W + (w0 + w), n);
        }
    }
    if (BLUR && tid < 2 * R + 1) s_taps[tid] = a.taps[tid];
    __syncthreads();
    for (int c = 0; c < a.C; ++c) {
        const U* xp = static_cast<const U*>(a.x) + (((long)n * a.C + c) * T + ts) * H * W;  // the source plane
        U* yp = static_cast<U*>(a.y) + (((long)n * a.C + c) * T + t) * H * W;
        if constexpr (BLUR) {
            const int vw = CR_TW + 2 * R, vh = CR_TH + 2 * R;
            for (int i = tid; i < vh * vw; i += CR_NT) {
                const int hh = i / vw, ww = i % vw;
                const int gh = min(max(h0 - R + hh, 0), H - 1), gw = min(max(w0 - R + ww, 0), W - 1);
                s_v[hh * CR_VW + ww] = raw_widen(xp[(long)gh * W + gw]) * a.stdv + a.mean;
            }
            __syncthreads();
            for (int i = tid; i < vh * CR_TW; i += CR_NT) {
                const int hh = i / CR_TW, w = i % CR_TW;
                float acc = 0.0f;
                for (int k = 0; k <= 2 * R; ++k) acc = acc + s_taps[k] * s_v[hh * CR_VW + w + k];
                s_g[i] = acc;
            }
            __syncthreads();
            for (int i = tid; i < CR_TH * CR_TW; i += CR_NT) {
                const int r = i / CR_TW, w = i % CR_TW;
                if (r < rows && w < cols) {
                    float acc = 0.0f;
                    for (int k = 0; k <= 2 * R; ++k) acc = acc + s_taps[k] * s_g[(r + k) * CR_TW + w];
                    const float ra = a.row_a ? a.row_a[h0 + r] : 1.0f, rb = a.row_b ? a.row_b[h0 + r] : 0.0f;
                    s_v[i] = cr_finish(a, acc, ra, rb, a.noise ? s_z[i] : 0.0f);
                }
            }
            __syncthreads();
        }
        for (int s = tid; s < rows * NSLOT; s += CR_NT) {
            const int r = s / NSLOT, j = s % NSLOT;
            U* orow = yp + (long)(h0 + r) * W + w0;
            const U* xrow = xp + (long)(h0 + r) * W + w0;
            const int e0 = lead_to_16(orow) + (j - 1) * EPV, lo = max(e0, 0), hi = min(e0 + EPV, cols);
            if (lo >= hi) continue;
            const bool full = hi - lo == EPV;
            U o[EPV];
            if constexpr (BLUR) {
#pragma unroll
                for (int e = 0; e < EPV; ++e) o[e] = raw_narrow<U>(s_v[r * CR_TW + min(max(e0 + e, 0), CR_TW - 1)]);
            } else {
                if (full && (((uintptr_t)(xrow + e0)) & 15) == 0) {
                    const uint4 q = *reinterpret_cast<const uint4*>(xrow + e0);
                    memcpy(o, &q, 16);
                } else {
#pragma unroll
                    for (int e = 0; e < EPV; ++e) o[e] = xrow[min(max(e0 + e, lo), hi - 1)];
                }
                if (!a.copy) {
                    const float ra = a.row_a ? a.row_a[h0 + r] : 1.0f, rb = a.row_b ? a.row_b[h0 + r] : 0.0f;
#pragma unroll
                    for (int e = 0; e < EPV; ++e) {
                        const float z = a.noise ? s_z[r * CR_TW + min(max(e0 + e, 0), CR_TW - 1)] : 0.0f;
                        o[e] = raw_narrow<U>(cr_finish(a, raw_widen(o[e]) * a.stdv + a.mean, ra, rb, z));
                    }
                }
            }
            if (full) {
                uint4 q;
                memcpy(&q, o, 16);
                *reinterpret_cast<uint4*>(orow + e0) = q;
            } else {
#pragma unroll
                for (int e = 0; e < EPV; ++e)
                    if (e0 + e >= lo && e0 + e < hi) orow[e0 + e] = o[e];
            }
        }
        if (BLUR) __syncthreads();  // the next channel's tile overwrites s_v
    }
}

// ---- stability ---------------------------------------------------------------------------------------------------------------------------
struct StabArgs {
    const float *logits_a, *logits_b, *sim_a, *sim_b, *occ_a, *occ_b;
    const int32_t* labels;
    int N, K, K_real, P, Ti, Hi, Wi, k, m;
    double* clip;
    int32_t *correct, *sel;
    double *pair, *acc;
};

// the first k of class block `base .. base + G` in the order of explain_block_rank, which is pasn_explain_rank's
__device__ __forceinline__ void st_select(const float* sim, int base, int G, int k, int32_t* out) {
    for (int p = base + (int)threadIdx.x; p < base + G; p += 64) {
        const int r = explain_block_rank(sim, base, G, p);
        if (r < k) out[r] = p;
    }
}

__global__ __launch_bounds__(64) void stability_clip_kernel(StabArgs a) {
    extern __shared__ int32_t s_sel[];  // [2][k]: sel_a, sel_b
    __shared__ int s_hits;
    const int n = blockIdx.x, tid = threadIdx.x, K_real = a.K_real, k = a.k;
    const float *la = a.logits_a + (long)n * a.K, *lb = a.logits_b + (long)n * a.K;
    const int pa = explain_pred(la, K_real), pb = explain_pred(lb, K_real);  // (pasn_explain_rank's prediction)
    const int G = a.P / a.K;
    if (tid == 0) s_hits = 0;
    for (int r = tid; r < 2 * k; r += 64) s_sel[r] = pa * G;  // a rank that NaN similarities leave out stays inside the block
    __syncthreads();
    st_select(a.sim_a + (long)n * a.P, pa * G, G, k, s_sel);
    st_select(a.sim_b + (long)n * a.P, pa * G, G, k, s_sel + k);
    __syncthreads();
    int hits = 0;
    for (int r = tid; r < k; r += 64) {
        const int p = s_sel[r];
        a.sel[(long)n * k + r] = p;
        for (int q = 0; q < k; ++q) hits += s_sel[k + q] == p ? 1 : 0;
    }
    if (hits) atomicAdd(&s_hits, hits);  // (LDS, integers)
    __syncthreads();
    if (tid != 0) return;
    double ma = (double)la[0], mb = (double)lb[0];
    for (int c = 1; c < K_real; ++c) {
        ma = fmax(ma, (double)la[c]);
        mb = fmax(mb, (double)lb[c]);
    }
    double sa = 0.0, sb = 0.0;
    for (int c = 0; c < K_real; ++c) {
        sa += exp((double)la[c] - ma);
        sb += exp((double)lb[c] - mb);
    }
    double tv = 0.0, drop = 0.0;
    for (int c = 0; c < K_real; ++c) {
        const double qa = exp((double)la[c] - ma) / sa, qb = exp((double)lb[c] - mb) / sb;
        tv += fabs(qa - qb);
        if (c == pa) drop = qa - qb;
    }
    double* out = a.clip + (long)n * 4;
    out[0] = pa != pb ? 1.0 : 0.0;
    out[1] = 0.5 * tv;
    out[2] = drop;
    out[3] = (double)s_hits / (double)k;
    if (a.labels && a.correct) {
        const int y = a.labels[n];
        a.correct[(long)n * 2] = pa == y ? 1 : 0;
        a.correct[(long)n * 2 + 1] = pb == y ? 1 : 0;
    }
}

// sum_i f(i) over [0, S) in index order, fp64, by the calling lane alone
template <typename F>
__device__ __forceinline__ double st_sum(int S, F f) {
    double s = 0.0;
    for (int i = 0; i < S; ++i) s += f(i);
    return s;
}

__global__ __launch_bounds__(ST_NT) void stability_pair_kernel(StabArgs a) {
    __shared__ float4 s_map4[2][ST_MAX_S / 4];
    __shared__ double s_sum[5];
    __shared__ int s_arg[2], s_inter;
    float* s_a = reinterpret_cast<float*>(s_map4[0]);
    float* s_b = reinterpret_cast<float*>(s_map4[1]);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int S = a.Ti * a.Hi * a.Wi, S4 = (S + 3) / 4, m = a.m;
    const long nj = blockIdx.x, n = nj / a.k;
    const int p = a.sel[nj];  // (written by the clip kernel: inside [0, P))
    const float *ga = a.occ_a + ((long)n * a.P + p) * S, *gb = a.occ_b + ((long)n * a.P + p) * S;
    for (int i = tid; i < S4 * 4; i += ST_NT) {  // the padding never outranks a voxel: -inf at an index past every voxel's
        s_a[i] = i < S ? ga[i] : -__builtin_inff();
        s_b[i] = i < S ? gb[i] : -__builtin_inff();
    }
    if (tid == 0) s_inter = 0, s_arg[0] = 0, s_arg[1] = 0;
    __syncthreads();
    if (lane == 0 && wave < 2) {
        const float* v = wave ? s_b : s_a;
        s_sum[wave] = st_sum(S, [&](int i) { return (double)v[i]; }) / (double)S;
    }
    __syncthreads();
    if (lane == 0 && wave < 3) {
        const double mu_a = s_sum[0], mu_b = s_sum[1];
        s_sum[2 + wave] = wave == 0   ? st_sum(S, [&](int i) { const double d = (double)s_a[i] - mu_a; return d * d; })
                          : wave == 1 ? st_sum(S, [&](int i) { const double d = (double)s_b[i] - mu_b; return d * d; })
                                      : st_sum(S, [&](int i) { return ((double)s_a[i] - mu_a) * ((double)s_b[i] - mu_b); });
    }
    // ranks by counting: (value descending, index ascending); four voxels per thread share every read of the map
    int inter = 0;
    for (int i0 = tid; i0 < S; i0 += 4 * ST_NT) {
        int idx[4], ra[4] = {0, 0, 0, 0}, rb[4] = {0, 0, 0, 0};
        float va[4], vb[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            idx[e] = min(i0 + e * ST_NT, S - 1);
            va[e] = s_a[idx[e]];
            vb[e] = s_b[idx[e]];
        }
        for (int j4 = 0; j4 < S4; ++j4) {
            const float4 oa = s_map4[0][j4], ob = s_map4[1][j4];
            const float fa[4] = {oa.x, oa.y, oa.z, oa.w}, fb[4] = {ob.x, ob.y, ob.z, ob.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = 4 * j4 + u;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    ra[e] += (fa[u] > va[e] || (fa[u] == va[e] && j < idx[e])) ? 1 : 0;
                    rb[e] += (fb[u] > vb[e] || (fb[u] == vb[e] && j < idx[e])) ? 1 : 0;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (i0 + e * ST_NT >= S) continue;
            if (ra[e] == 0) s_arg[0] = idx[e];
            if (rb[e] == 0) s_arg[1] = idx[e];
            inter += (ra[e] < m && rb[e] < m) ? 1 : 0;
        }
    }
    if (inter) atomicAdd(&s_inter, inter);  // (LDS, integers)
    __syncthreads();
    if (tid != 0) return;
    const double saa = s_sum[2], sbb = s_sum[3], sab = s_sum[4];
    double corr;
    if (saa == 0.0 && sbb == 0.0) corr = 1.0;
    else if (saa == 0.0 || sbb == 0.0) corr = 0.0;
    else corr = sab / sqrt(saa * sbb);
    const int ia = s_arg[0], ib = s_arg[1], HW = a.Hi * a.Wi;
    const long dt = ia / HW - ib / HW, dh = (ia % HW) / a.Wi - (ib % HW) / a.Wi, dw = ia % a.Wi - ib % a.Wi;
    const long diag = (long)(a.Ti - 1) * (a.Ti - 1) + (long)(a.Hi - 1) * (a.Hi - 1) + (long)(a.Wi - 1) * (a.Wi - 1);
    double* out = a.pair + nj * 4;
    out[0] = (double)a.sim_b[(long)n * a.P + p] - (double)a.sim_a[(long)n * a.P + p];
    out[1] = corr;
    out[2] = (double)s_inter / (double)(2 * m - s_inter);
    out[3] = diag > 0 ? sqrt((double)(dt * dt + dh * dh + dw * dw)) / sqrt((double)diag) : 0.0;
}

// acc = [clip statistics (4), correct counts (2), pair statistics (k, 4), N]
__global__ __launch_bounds__(ST_NT) void stability_acc_kernel(StabArgs a) {
    sweep_acc_add<ST_NT>(a.acc, 6 + 4 * a.k + 1, a.N, [&](long n, int e) {
        if (e < 4) return a.clip[n * 4 + e];
        if (e < 6) return (a.labels && a.correct) ? (double)a.correct[n * 2 + (e - 4)] : 0.0;
        return a.pair[n * 4 * a.k + (e - 6)];
    });
}

}  // namespace pasn

using namespace pasn;

extern "C" int pasn_clip_corrupt(const void* x, void* y, int N, int C, int T, int H, int W, int dtype, const pasn_corrupt_desc* desc,
                                 void* stream) {
    PASN_REQUIRE(x && y && desc, "x, y and the descriptor are required");
    PASN_REQUIRE(dtype == PASN_F32 || dtype == PASN_BF16, "dtype must be PASN_F32 or PASN_BF16");
    PASN_REQUIRE(N >= 1 && T >= 1 && H >= 1 && W >= 1, "N, T, H and W must be positive");
    PASN_REQUIRE(C == 1 || C == 3, "C must be 1 or 3");
    PASN_REQUIRE(desc->R >= 0 && desc->R <= CR_RMAX, "R must lie in [0, 8]");
    PASN_REQUIRE(desc->R == 0 || desc->taps, "a blur (R > 0) needs its taps");
    const uintptr_t esz = dtype == PASN_BF16 ? 2 : 4;
    PASN_REQUIRE((((uintptr_t)x | (uintptr_t)y) & (esz - 1)) == 0, "x and y must be aligned to their element");
    const bool photo = desc->row_a || desc->row_b, noise = desc->sigma_add != 0.0f || desc->sigma_mul != 0.0f;
    const CorruptArgs a{x, y, desc->src_t, desc->taps, desc->row_a, desc->row_b, N, C, T, H, W, desc->R, (H + CR_TH - 1) / CR_TH,
                        (W + CR_TW - 1) / CR_TW, desc->sigma_add, desc->sigma_mul, desc->mean, desc->stdv, (uint32_t)desc->seed,
                        (uint32_t)(desc->seed >> 32), desc->R == 0 && !photo && !noise, photo, noise};  // (the struct's field order)
    const long blocks = (long)N * T * a.tilesH * a.tilesW;
    PASN_REQUIRE(blocks <= 0x7fffffffL, "more than 2^31 - 1 tiles");
    const dim3 grid((unsigned)blocks);
    hipStream_t s = (hipStream_t)stream;
    const bool blur = desc->R > 0;
    if (dtype == PASN_BF16) {
        if (blur) hipLaunchKernelGGL((clip_corrupt_kernel<uint16_t, true>), grid, dim3(CR_NT), 0, s, a);
        else hipLaunchKernelGGL((clip_corrupt_kernel<uint16_t, false>), grid, dim3(CR_NT), 0, s, a);
    } else {
        if (blur) hipLaunchKernelGGL((clip_corrupt_kernel<uint32_t, true>), grid, dim3(CR_NT), 0, s, a);
        else hipLaunchKernelGGL((clip_corrupt_kernel<uint32_t, false>), grid, dim3(CR_NT), 0, s, a);
    }
    return check_launch("clip_corrupt");
}

extern "C" int pasn_stability_stats(const float* logits_a, const float* logits_b, const float* sim_a, const float* sim_b, const float* occ_a,
                                    const float* occ_b, const int32_t* labels, int N, int K, int K_real, int P, int Ti, int Hi, int Wi, int k,
                                    int m, double* clip, int32_t* correct, int32_t* sel, double* pair, double* acc, void* stream) {
    PASN_REQUIRE(logits_a && logits_b && sim_a && sim_b && occ_a && occ_b, "logits, sim and occ of both forwards are required");
    PASN_REQUIRE(clip && sel && pair, "clip, sel and pair are required");
    PASN_REQUIRE(!labels || correct, "labels need correct");
    PASN_REQUIRE(N >= 1 && N <= 65535, "N must lie in [1, 65535]");
    PASN_REQUIRE(K >= 1 && K_real >= 1 && K_real <= K, "K_real must lie in [1, K]");
    PASN_REQUIRE(P >= 1 && P % K == 0 && P <= ST_MAX_P, "P must be a multiple of K in [K, 16384]");
    PASN_REQUIRE(k >= 1 && k <= P / K && k <= ST_MAX_S, "k must lie in [1, min(P / K, 4096)]");
    PASN_REQUIRE(Ti >= 1 && Hi >= 1 && Wi >= 1, "Ti, Hi and Wi must be positive");
    const long S = (long)Ti * Hi * Wi;
    if (S > ST_MAX_S) {
        set_error("pasn_stability_stats: S = Ti Hi Wi > 4096 is not supported (LDS)");
        return PASN_ERR_UNSUPPORTED;
    }
    PASN_REQUIRE(m >= 1 && m <= S, "m must lie in [1, S]");
    PASN_REQUIRE((long)N * k <= 0x7fffffffL, "more than 2^31 - 1 maps");
    const StabArgs a{logits_a, logits_b, sim_a, sim_b, occ_a, occ_b, labels, N, K, K_real, P, Ti, Hi, Wi, k, m, clip, correct, sel, pair, acc};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(stability_clip_kernel, dim3((unsigned)N), dim3(64), 2 * (size_t)k * sizeof(int32_t), s, a);
    hipLaunchKernelGGL(stability_pair_kernel, dim3((unsigned)((long)N * k)), dim3(ST_NT), 0, s, a);
    if (acc) hipLaunchKernelGGL(stability_acc_kernel, dim3(1), dim3(ST_NT), 0, s, a);
    return check_launch("stability_stats");
}
