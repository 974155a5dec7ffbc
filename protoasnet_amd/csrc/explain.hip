// explain.hip -- local explanations (src/utils/local_explainability.py:17-200 + explainability_utils.py:135-200) on the device.
//
// pasn_explain_rank: per clip, the class contributions W[k, p] * sim[p] and their sums sim @ W.T (local_explainability.py:91, :181-183),
// the prototypes of each class block ordered by descending similarity (:112-125), the argmax of the non-abstain logits and the top
// k_sel prototypes of the predicted class.  One workgroup per clip; the rank of prototype p inside its block is explain_block_rank of
// explain_common.h (the number of block members that beat it), O((P/K)^2) comparisons out of LDS, no sort network, deterministic.
//
// pasn_explain_maps: get_normalized_upsample_occurence_maps (explainability_utils.py:158-174) and the heat-map overlay (:177-200,
// local_explainability.py:76, :104).  Per map, torch.nn.Upsample(size, trilinear | bilinear), align_corners=False:
//     source coordinate  r = max(0, fma(in / out, o + 0.5, -0.5)),  i0 = (int)r,  i1 = i0 + (i0 < in - 1),  l1 = r - i0,  l0 = 1 - l1
//     u = fma(Y(t0), lt0, Y(t1) * lt1),  Y(t) = fma(X(t, h0), lh0, X(t, h1) * lh1),  X(t, h) = fma(S[t][h][w0], lw0, S[t][h][w1] * lw1)
// which is, bit for bit, what torch's CPU kernels (upsample_trilinear3d, and upsample_bilinear2d's generic kernel with T = 1) compute on
// an FMA host (the index is computed in double there and rounded once; the lerps contract into one fma each).  Then
//     d = (max - min) + 1e-7f,   v = (u - min) / d   (correctly rounded, as IEEE division: never fast-math here; uint8 parity needs it)
// with min / max over every output voxel of the map, and optionally uint8 (uint8)(255.0f * v) (numpy's truncation) and the overlay
//     (src * std + mean) + alpha * lut[uint8][c]
// Two launches: a stats pass that evaluates every voxel of a (map, frame, row band) slab and writes its min / max to the workspace, and
// a write pass that reduces the map's slab stats, evaluates the same voxels with the same code and streams the outputs (16-byte fp32 stores,
// 4-byte uint8 stores along W).  Both evaluate with the same code (explicit fma / mul, no contraction left to the compiler), so min / max are exactly those of the values written: the minimum maps to 0.0, nothing
// falls outside [0, 1].  A block keeps the x-interpolated rows X(t0 | t1, h) of its band in LDS (2 x rows x Wo floats), so a voxel costs
// four LDS reads and three fmas.
#include "common.h"
#include "explain_common.h"

namespace pasn {

struct ExAxis {
    int i0, i1;
    float l0, l1;
};

// area_pixel_compute_source_index (align_corners = False) + the lambdas of compute_indices_weights_linear
__device__ __forceinline__ ExAxis ex_axis(int o, int in, float scale) {
    const float r = fmaxf(__fmaf_rn(scale, (float)o + 0.5f, -0.5f), 0.0f);
    ExAxis a;
    a.i0 = min((int)r, in - 1);
    a.i1 = a.i0 + (a.i0 < in - 1 ? 1 : 0);
    a.l1 = fminf(fmaxf(__fsub_rn(r, (float)a.i0), 0.0f), 1.0f);
    a.l0 = __fsub_rn(1.0f, a.l1);
    return a;
}

__device__ __forceinline__ float ex_lerp(float a, float b, float w0, float w1) { return __fmaf_rn(a, w0, __fmul_rn(b, w1)); }

struct ExGeom {
    int N, P, k, Ti, Hi, Wi, To, Ho, Wo;
    int nb, hb;        // row bands per frame, rows per band
    int bdx;           // threads along W (column groups); the 256 threads of a block are (256 / bdx) rows of bdx, the rest idle
    float st, sh, sw;  // in / out per axis
};

// op (fminf / fmaxf) over the block's 256 values; every thread gets the result
template <typename Op>
__device__ __forceinline__ float ex_block_reduce(float v, float* red, Op op) {
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = op(op(red[0], red[1]), op(red[2], red[3]));
    return v;
}
__device__ __forceinline__ float ex_block_min(float v, float* red) { return ex_block_reduce(v, red, [](float a, float b) { return fminf(a, b); }); }
__device__ __forceinline__ float ex_block_max(float v, float* red) { return ex_block_reduce(v, red, [](float a, float b) { return fmaxf(a, b); }); }

template <typename TS>
__device__ __forceinline__ float ex_src(const TS* p) { return (float)*p; }

// WRITE = false: stats pass (slab min / max -> stats[m][slab][2]).  WRITE = true: outputs.  VEC consecutive voxels along W per thread.
template <int VEC, bool WRITE, typename TS>
__global__ __launch_bounds__(256) void explain_maps_kernel(const float* __restrict__ occ, const int32_t* __restrict__ sel,
                                                           float* __restrict__ stats, float* __restrict__ map_f, uint8_t* __restrict__ map_u8,
                                                           float* __restrict__ ovl, const TS* __restrict__ src, int src_c,
                                                           const float* __restrict__ lut, float mean, float stdv, float alpha, ExGeom g) {
    extern __shared__ __attribute__((aligned(16))) float xl[];  // [2][nh][Wo]: X(t0, h), X(t1, h) for the band's source rows h = hlo .. hlo + nh - 1
    __shared__ float red[8];
    __shared__ float lut_s[WRITE ? 768 : 1];
    const int tid = threadIdx.x, nt = 256;  // full waves: the block reductions shuffle across all 64 lanes
    const int tx = tid % g.bdx, ty = tid / g.bdx, nty = 256 / g.bdx;
    const int nslab = g.To * g.nb;
    const int m = blockIdx.x / nslab, s = blockIdx.x - m * nslab;
    const int t = s / g.nb, band = s - t * g.nb;
    const int n = m / g.k, j = m - n * g.k;
    int p = sel ? sel[m] : j;
    p = min(max(p, 0), g.P - 1);  // the host side validates the table; a bad entry must not read another clip's memory
    const float* S = occ + ((long)n * g.P + p) * ((long)g.Ti * g.Hi * g.Wi);
    const ExAxis at = ex_axis(t, g.Ti, g.st);
    const int ya = band * g.hb, yb = min(g.Ho, ya + g.hb);
    const int hlo = ex_axis(ya, g.Hi, g.sh).i0, nh = ex_axis(yb - 1, g.Hi, g.sh).i1 - hlo + 1;  // <= Hi (source index monotone in y)
    const int Wo = g.Wo;
    for (int x = tid; x < Wo; x += nt) {  // one output column per thread: its weights once, then every row of both frames
        const ExAxis ax = ex_axis(x, g.Wi, g.sw);
        for (int f = 0; f < 2; ++f) {
            const float* row = S + ((long)(f ? at.i1 : at.i0) * g.Hi + hlo) * g.Wi;
            for (int h = 0; h < nh; ++h, row += g.Wi) xl[(f * nh + h) * Wo + x] = ex_lerp(row[ax.i0], row[ax.i1], ax.l0, ax.l1);
        }
    }
    float lo = 0.0f, d = 1.0f, rd = 1.0f;
    bool markstein = false;
    if constexpr (WRITE) {
        if (lut)
            for (int e = tid; e < 768; e += nt) lut_s[e] = lut[e];
        const float* st = stats + (long)m * nslab * 2;
        float a = INFINITY, b = -INFINITY;
        for (int i = tid; i < nslab; i += nt) {
            a = fminf(a, st[2 * i]);
            b = fmaxf(b, st[2 * i + 1]);
        }
        lo = ex_block_min(a, red);
        const float hi = ex_block_max(b, red);
        d = __fadd_rn(__fsub_rn(hi, lo), 1e-7f);
        rd = __fdiv_rn(1.0f, d);
        markstein = d >= 0x1p-100f && d <= 0x1p100f;  // no underflow / overflow in the refinement below
    }
    __syncthreads();
    float mn = INFINITY, mx = -INFINITY;
    const int Gx = Wo / VEC;
    for (int y = ya + ty; ty < nty && y < yb; y += nty) {
        const ExAxis ay = ex_axis(y, g.Hi, g.sh);
        const float* r00 = xl + (ay.i0 - hlo) * Wo;
        const float* r01 = xl + (ay.i1 - hlo) * Wo;
        const float* r10 = r00 + nh * Wo;
        const float* r11 = r01 + nh * Wo;
        const long vox0 = (((long)m * g.To + t) * g.Ho + y) * Wo;  // flat voxel index of (m, t, y, 0)
        for (int xg = tx; xg < Gx; xg += g.bdx) {
            const int x0 = xg * VEC;
            float u[VEC];
            if constexpr (VEC % 4 == 0) {
#pragma unroll
                for (int q = 0; q < VEC; q += 4) {
                    const float4 a = *reinterpret_cast<const float4*>(r00 + x0 + q), b = *reinterpret_cast<const float4*>(r01 + x0 + q);
                    const float4 c = *reinterpret_cast<const float4*>(r10 + x0 + q), e = *reinterpret_cast<const float4*>(r11 + x0 + q);
                    u[q + 0] = ex_lerp(ex_lerp(a.x, b.x, ay.l0, ay.l1), ex_lerp(c.x, e.x, ay.l0, ay.l1), at.l0, at.l1);
                    u[q + 1] = ex_lerp(ex_lerp(a.y, b.y, ay.l0, ay.l1), ex_lerp(c.y, e.y, ay.l0, ay.l1), at.l0, at.l1);
                    u[q + 2] = ex_lerp(ex_lerp(a.z, b.z, ay.l0, ay.l1), ex_lerp(c.z, e.z, ay.l0, ay.l1), at.l0, at.l1);
                    u[q + 3] = ex_lerp(ex_lerp(a.w, b.w, ay.l0, ay.l1), ex_lerp(c.w, e.w, ay.l0, ay.l1), at.l0, at.l1);
                }
            } else {
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    const int x = x0 + q;
                    u[q] = ex_lerp(ex_lerp(r00[x], r01[x], ay.l0, ay.l1), ex_lerp(r10[x], r11[x], ay.l0, ay.l1), at.l0, at.l1);
                }
            }
            if constexpr (!WRITE) {
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    mn = fminf(mn, u[q]);
                    mx = fmaxf(mx, u[q]);
                }
            } else {
                const long vox = vox0 + x0;
                float v[VEC];
                uint8_t q8[VEC];
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    // (u - min) / d correctly rounded: q0 = a * RN(1/d), then one Markstein step q0 + fma(-q0, d, a) * RN(1/d), which is
                    // RN(a / d) (Markstein's theorem: RN(1/d) within half an ulp, q0 within one ulp, no underflow / overflow)
                    const float a = __fsub_rn(u[q], lo);
                    if (markstein) {
                        const float q0 = __fmul_rn(a, rd);
                        v[q] = __fmaf_rn(__fmaf_rn(-q0, d, a), rd, q0);
                    } else {
                        v[q] = __fdiv_rn(a, d);
                    }
                    q8[q] = (uint8_t)(int)__fmul_rn(255.0f, v[q]);
                }
                if (map_f) {
                    if constexpr (VEC % 4 == 0) {
#pragma unroll
                        for (int q = 0; q < VEC; q += 4)
                            *reinterpret_cast<float4*>(map_f + vox + q) = make_float4(v[q], v[q + 1], v[q + 2], v[q + 3]);
                    } else {
#pragma unroll
                        for (int q = 0; q < VEC; ++q) map_f[vox + q] = v[q];
                    }
                }
                if (map_u8) {
                    if constexpr (VEC == 4) {
                        *reinterpret_cast<uint32_t*>(map_u8 + vox) = q8[0] | (q8[1] << 8) | (q8[2] << 16) | ((uint32_t)q8[3] << 24);
                    } else {
#pragma unroll
                        for (int q = 0; q < VEC; ++q) map_u8[vox + q] = q8[q];
                    }
                }
                if (ovl) {
                    // source clip (n, c, t, y, x0 ..): one channel counts as three identical ones
                    const long plane = (long)g.To * g.Ho * Wo;
                    const TS* s0 = src + (long)n * src_c * plane + ((long)t * g.Ho + y) * Wo + x0;
                    float o[3 * VEC];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const TS* sc = s0 + (src_c == 3 ? c : 0) * plane;
#pragma unroll
                        for (int q = 0; q < VEC; ++q) {
                            const float img = __fadd_rn(__fmul_rn(ex_src(sc + q), stdv), mean);
                            o[3 * q + c] = __fadd_rn(img, __fmul_rn(alpha, lut_s[3 * q8[q] + c]));
                        }
                    }
                    float* dst = ovl + vox * 3;
                    if constexpr (VEC % 4 == 0) {
#pragma unroll
                        for (int q = 0; q < 3 * VEC; q += 4) *reinterpret_cast<float4*>(dst + q) = make_float4(o[q], o[q + 1], o[q + 2], o[q + 3]);
                    } else {
#pragma unroll
                        for (int q = 0; q < 3 * VEC; ++q) dst[q] = o[q];
                    }
                }
            }
        }
    }
    if constexpr (!WRITE) {
        mn = ex_block_min(mn, red);
        mx = ex_block_max(mx, red);
        if (tid == 0) {
            float2* st = reinterpret_cast<float2*>(stats) + (long)m * nslab + s;
            *st = make_float2(mn, mx);
        }
    }
}

// ---- rank ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void explain_rank_kernel(const float* __restrict__ sim, const float* __restrict__ fc_w,
                                                           const float* __restrict__ logits, int P, int K, int K_real, int k_sel,
                                                           float* __restrict__ contrib, float* __restrict__ totals, int32_t* __restrict__ order,
                                                           int32_t* __restrict__ rank, int32_t* __restrict__ pred, int32_t* __restrict__ sel) {
    extern __shared__ float s_sim[];  // [P]
    __shared__ double red[4];
    __shared__ int s_pred;
    const int n = blockIdx.x, tid = threadIdx.x;
    for (int p = tid; p < P; p += 256) s_sim[p] = sim[(long)n * P + p];
    if (tid == 0) pred[n] = s_pred = explain_pred(logits + (long)n * K, K_real);
    __syncthreads();
    for (int c = 0; c < K; ++c) {
        const float* w = fc_w + (long)c * P;
        double acc = 0.0;
        for (int p = tid; p < P; p += 256) {
            const float wv = w[p], sv = s_sim[p];
            if (contrib) contrib[((long)n * K + c) * P + p] = __fmul_rn(wv, sv);
            acc += (double)wv * (double)sv;  // exact products, fp64 sum: within one fp32 rounding of sim @ W.T
        }
        if (totals) {
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
            if ((tid & 63) == 0) red[tid >> 6] = acc;
            __syncthreads();
            if (tid == 0) totals[(long)n * K + c] = (float)(((red[0] + red[1]) + red[2]) + red[3]);
            __syncthreads();
        }
    }
    const int G = P / K, pc = s_pred;
    for (int p = tid; p < G * K; p += 256) {
        const int base = (p / G) * G;
        const int r = explain_block_rank(s_sim, base, G, p);
        order[(long)n * P + base + r] = p;
        if (rank) rank[(long)n * P + p] = r;
        if (sel && base == pc * G && r < k_sel) sel[(long)n * k_sel + r] = p;
    }
}

// geometry shared by the workspace query and the launch: enough (map, frame, band) slabs to fill the chip
static ExGeom ex_geom(int N, int P, int k, int Ti, int Hi, int Wi, int To, int Ho, int Wo) {
    ExGeom g{N, P, k, Ti, Hi, Wi, To, Ho, Wo, 1, Ho, 1, (float)Ti / (float)To, (float)Hi / (float)Ho, (float)Wi / (float)Wo};
    const long slabs = (long)N * k * To;
    int nb = (int)std::min<long>(std::max<long>((2048 + slabs - 1) / slabs, 1), Ho);
    g.hb = (Ho + nb - 1) / nb;
    g.nb = (Ho + g.hb - 1) / g.hb;
    return g;
}

}  // namespace pasn

using namespace pasn;

extern "C" int pasn_explain_rank(const float* sim, const float* fc_w, const float* logits, int N, int P, int K, int K_real, int k_sel,
                                 float* contrib, float* totals, int32_t* order, int32_t* rank, int32_t* pred, int32_t* sel, void* stream) {
    PASN_REQUIRE(sim && fc_w && logits && order && pred, "sim, fc_w, logits, order and pred are required");
    PASN_REQUIRE(N > 0 && P > 0 && K > 0 && P % K == 0, "P must be a positive multiple of K");
    PASN_REQUIRE(K_real >= 1 && K_real <= K, "K_real must lie in [1, K]");
    PASN_REQUIRE(P <= 16384, "P > 16384 prototypes per clip is not supported (LDS)");
    PASN_REQUIRE(!sel || (k_sel >= 1 && k_sel <= P / K), "k_sel must lie in [1, P / K]");
    hipLaunchKernelGGL(explain_rank_kernel, dim3(N), dim3(256), P * sizeof(float), (hipStream_t)stream, sim, fc_w, logits, P, K, K_real,
                       sel ? k_sel : 0, contrib, totals, order, rank, pred, sel);
    return check_launch("explain_rank");
}

extern "C" size_t pasn_explain_maps_workspace_bytes(int N, int P, int k, int Ti, int Hi, int Wi, int To, int Ho, int Wo) {
    if (N <= 0 || k <= 0 || To <= 0 || Ho <= 0) return 0;
    const ExGeom g = ex_geom(N, P, k, Ti, Hi, Wi, To, Ho, Wo);
    return (size_t)N * k * To * g.nb * 2 * sizeof(float);
}

extern "C" int pasn_explain_maps(const float* occ, const int32_t* sel, int N, int P, int k, int Ti, int Hi, int Wi, int To, int Ho, int Wo,
                                 void* maps, int maps_dtype, float* overlay, const void* src, int src_dtype, int src_channels, const float* lut,
                                 float mean, float stdv, float alpha, void* workspace, void* stream) {
    PASN_REQUIRE(occ && workspace, "occ and workspace are required");
    PASN_REQUIRE(N > 0 && P > 0 && k > 0 && Ti > 0 && Hi > 0 && Wi > 0 && To > 0 && Ho > 0 && Wo > 0, "bad extents");
    PASN_REQUIRE(sel || k == P, "without a selection table k must equal P");
    PASN_REQUIRE(maps || overlay, "nothing to write: pass maps and / or overlay");
    PASN_REQUIRE(!maps || maps_dtype == PASN_F32 || maps_dtype == PASN_U8, "maps are fp32 or uint8");
    PASN_REQUIRE(!overlay || (src && lut), "an overlay needs the source clip and the 256 x 3 colour table");
    PASN_REQUIRE(!overlay || src_dtype == PASN_F32 || src_dtype == PASN_BF16, "the source clip is fp32 or bf16");
    PASN_REQUIRE(!overlay || src_channels == 1 || src_channels == 3, "the source clip has 1 or 3 channels");
    PASN_REQUIRE(((uintptr_t)maps & 15) == 0 && ((uintptr_t)overlay & 15) == 0 && ((uintptr_t)workspace & 7) == 0, "misaligned output");
    const size_t lds = (size_t)2 * Hi * Wo * sizeof(float);
    if (lds > 65536) {
        set_error("pasn_explain_maps: source rows x output width too large for LDS (2 * Hi * Wo * 4 > 64 KiB)");
        return PASN_ERR_UNSUPPORTED;
    }
    ExGeom g = ex_geom(N, P, k, Ti, Hi, Wi, To, Ho, Wo);
    const int vec = Wo % 4 == 0 ? 4 : 1;  // 28 column groups at Wo = 112: 9 rows of a block at a time
    g.bdx = std::min(Wo / vec, 256);
    const long blocks = (long)N * k * To * g.nb;
    PASN_REQUIRE(blocks < (1L << 31), "too many slabs");
    hipStream_t s = (hipStream_t)stream;
    float* map_f = maps && maps_dtype == PASN_F32 ? static_cast<float*>(maps) : nullptr;
    uint8_t* map_u8 = maps && maps_dtype == PASN_U8 ? static_cast<uint8_t*>(maps) : nullptr;
    float* ws = static_cast<float*>(workspace);
#define EXM(V, W, TS)                                                                                                                     \
    hipLaunchKernelGGL((explain_maps_kernel<V, W, TS>), dim3((unsigned)blocks), dim3(256), lds, s, occ, sel, ws, map_f, map_u8, overlay, \
                       static_cast<const TS*>(src), src_channels, lut, mean, stdv, alpha, g)
#define EXM_PAIR(V, TS)   \
    do {                  \
        EXM(V, false, TS); \
        EXM(V, true, TS);  \
    } while (0)
    const bool bf = overlay && src_dtype == PASN_BF16;
    if (vec == 4) {
        if (bf) EXM_PAIR(4, __bf16);
        else EXM_PAIR(4, float);
    } else {
        if (bf) EXM_PAIR(1, __bf16);
        else EXM_PAIR(1, float);
    }
#undef EXM_PAIR
#undef EXM
    return check_launch("explain_maps");
}
