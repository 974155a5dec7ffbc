// dw_wgrad.hip -- the depthwise convs' backward: input gradient (any window / stride, and the 3x3x3 stride-(1,2,2) patch form) and the
// five weight-gradient kernels (row partials, strip, two T-marching cuts, temporal) with their host ladder.  Every weight-gradient kernel
// leaves one partial row per block through block_reduce_rows (block_reduce.h: the fixed summation order shared with train.hip), and
// dw_wgrad_reduce_kernel combines the rows in index order; the two marching kernels share their tap FMA against the gradient ring
// (march_row_fma).
#include <type_traits>

#include "block_reduce.h"
#include "common.h"

namespace pasn {

// ---- depthwise input gradient (any window / stride): dx[n,ti,hi,wi,c] = sum_taps dy[n,to,ho,wo,c] * w[tap][c] -----------
template <typename T>
__global__ __launch_bounds__(256) void dw_dgrad_kernel(const T* __restrict__ dy, const float* __restrict__ w, T* __restrict__ dx,
                                                       pasn_conv_desc d) {
    const int CG = d.Cin_p / 8;
    const size_t total = (size_t)d.N * d.Ti * d.Hi * d.Wi * CG;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int cg = (int)(i % CG);
        const size_t row = i / CG;
        const int wi = (int)(row % d.Wi);
        size_t q = row / d.Wi;
        const int hi = (int)(q % d.Hi);
        q /= d.Hi;
        const int ti = (int)(q % d.Ti), n = (int)(q / d.Ti);
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
        for (int a = 0; a < d.kt; ++a) {
            const int tn = ti + d.pt - a;
            if (tn < 0 || tn % d.st) continue;
            const int to = tn / d.st;
            if (to >= d.To) continue;
            for (int b = 0; b < d.kh; ++b) {
                const int hn = hi + d.ph - b;
                if (hn < 0 || hn % d.sh) continue;
                const int ho = hn / d.sh;
                if (ho >= d.Ho) continue;
                for (int c = 0; c < d.kw; ++c) {
                    const int wn = wi + d.pw - c;
                    if (wn < 0 || wn % d.sw) continue;
                    const int wo = wn / d.sw;
                    if (wo >= d.Wo) continue;
                    float g[8], wv[8];
                    load8(dy + ((((size_t)n * d.To + to) * d.Ho + ho) * d.Wo + wo) * d.Cout_p + cg * 8, g);
                    load8(w + (size_t)((a * d.kh + b) * d.kw + c) * d.Cout_p + cg * 8, wv);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = fmaf(g[j], wv[j], acc[j]);
                }
            }
        }
        store8(dx + row * d.Cin_p + cg * 8, acc);
    }
}

// ---- depthwise weight gradient: partial[chunk][tap][Cp] over output-row chunks, one temporal tap plane per blockIdx.z ----
template <typename T>
__global__ __launch_bounds__(256) void dw_wgrad_partial_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ partial,
                                                               pasn_conv_desc d, int CG, int CGb, long rows_per_chunk) {
    __shared__ float red[256 * 8];
    const int cg = threadIdx.x % CGb, rl = threadIdx.x / CGb, RL = 256 / CGb;
    const int a = blockIdx.z;  // temporal tap
    const int KP = d.kh * d.kw;  // <= 9
    float acc[9][8];
#pragma unroll
    for (int p = 0; p < 9; ++p)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[p][j] = 0.0f;
    const long R = (long)d.N * d.To * d.Ho * d.Wo;
    const long r0 = (long)blockIdx.x * rows_per_chunk, r1 = min(R, r0 + rows_per_chunk);
    if (cg < CG) {
        for (long r = r0 + rl; r < r1; r += RL) {
            const int wo = (int)(r % d.Wo);
            long q = r / d.Wo;
            const int ho = (int)(q % d.Ho);
            q /= d.Ho;
            const int to = (int)(q % d.To), n = (int)(q / d.To);
            const int ti = to * d.st - d.pt + a;
            if (ti < 0 || ti >= d.Ti) continue;
            float g[8];
            load8(dy + r * d.Cout_p + cg * 8, g);
#pragma unroll
            for (int p = 0; p < 9; ++p) {
                if (p < KP) {
                    const int hi = ho * d.sh - d.ph + p / d.kw, wi = wo * d.sw - d.pw + p % d.kw;
                    if (hi >= 0 && hi < d.Hi && wi >= 0 && wi < d.Wi) {
                        float v[8];
                        load8(x + ((((size_t)n * d.Ti + ti) * d.Hi + hi) * d.Wi + wi) * d.Cin_p + cg * 8, v);
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[p][j] = fmaf(g[j], v[j], acc[p][j]);
                    }
                }
            }
        }
    }
    const int taps = d.kt * KP;
    block_reduce_rows(acc, red, partial + ((size_t)blockIdx.x * taps + (size_t)a * KP) * d.Cout_p, d.Cout_p, CG, CGb, KP);
}

__global__ void dw_wgrad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw, int chunks, int taps, int C, int Cp);

static long dw_wgrad_rows_per_chunk(const pasn_conv_desc& d) {
    const long R = (long)d.N * d.To * d.Ho * d.Wo;
    const int RL = 256 / pow2_at_least(d.Cout_p / 8);
    const long chunks = std::max<long>(1, std::min<long>(2048, R / ((long)RL * 8)));
    return (R + chunks - 1) / chunks;
}

}  // namespace pasn

using namespace pasn;

// 3x3x3, stride (1,2,2), pad 1 (the first block of every X3D stage): a thread owns a 2x2 input patch.  Even rows / columns
// see only the centre tap, odd ones the two outer taps, so the four pixels need dy[to][i..i+1][j..j+1] for the three temporal
// taps -- 12 loads and 27 FMAs per channel for 4 outputs, no divergent tap loop.
template <typename T>
__global__ __launch_bounds__(256) void dw_dgrad_s2_kernel(const T* __restrict__ dy, const float* __restrict__ w, T* __restrict__ dx,
                                                          pasn_conv_desc d) {
    constexpr int CH = 4;  // channels per thread: 4 keeps the patch + taps + gradients at ~130 registers (8: 330, one wave per SIMD)
    // the 27 x Cp taps in LDS, staged once per block (the first version read its 27 weight vectors per patch from global memory: 864
    // bytes of weights for 192 bytes of gradients per thread)
    extern __shared__ __attribute__((aligned(16))) float wl[];  // [27][Cp]
    for (int i = threadIdx.x * 4; i < 27 * d.Cout_p; i += 256 * 4) *reinterpret_cast<f32x4*>(wl + i) = *reinterpret_cast<const f32x4*>(w + i);
    __syncthreads();
    const int CG = d.Cin_p / CH, Hh = (d.Hi + 1) / 2, Wh = (d.Wi + 1) / 2;
    const size_t total = (size_t)d.N * d.Ti * Hh * Wh * CG;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int cg = (int)(idx % CG);
        size_t q = idx / CG;
        const int j = (int)(q % Wh);
        q /= Wh;
        const int i = (int)(q % Hh);
        q /= Hh;
        const int ti = (int)(q % d.Ti), n = (int)(q / d.Ti);
        float o[2][2][CH];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int e = 0; e < CH; ++e) o[a][b][e] = 0.0f;
        // all twelve gradient loads first (clamped addresses), masks afterwards
        float g[3][2][2][CH];
        unsigned okbits = 0;
#pragma unroll
        for (int kt = 0; kt < 3; ++kt) {
            const int to = ti + 1 - kt;
            const bool tok = to >= 0 && to < d.To;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int ho = i + a, wo = j + b;
                    const bool ok = tok && ho < d.Ho && wo < d.Wo;
                    load4(dy + ((((size_t)n * d.To + (tok ? to : 0)) * d.Ho + (ok ? ho : 0)) * d.Wo + (ok ? wo : 0)) * d.Cout_p + cg * CH, g[kt][a][b]);
                    okbits |= (ok ? 1u : 0u) << (kt * 4 + a * 2 + b);
                }
        }
#pragma unroll
        for (int kt = 0; kt < 3; ++kt) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    if (!((okbits >> (kt * 4 + a * 2 + b)) & 1u)) {
#pragma unroll
                        for (int e = 0; e < CH; ++e) g[kt][a][b][e] = 0.0f;
                    }
            const float* wk = wl + kt * 9 * d.Cout_p + cg * CH;
            float wv[9][CH];
#pragma unroll
            for (int tp = 0; tp < 9; ++tp) load4(wk + tp * d.Cout_p, wv[tp]);
            // input (2i+a, 2j+b) <- output (ho, wo) through tap (kh, kw) with 2*ho - 1 + kh = 2i + a
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                o[0][0][e] = fmaf(g[kt][0][0][e], wv[4][e], o[0][0][e]);                                                      // (1,1)
                o[0][1][e] = fmaf(g[kt][0][0][e], wv[5][e], fmaf(g[kt][0][1][e], wv[3][e], o[0][1][e]));                      // (1,2) from j, (1,0) from j+1
                o[1][0][e] = fmaf(g[kt][0][0][e], wv[7][e], fmaf(g[kt][1][0][e], wv[1][e], o[1][0][e]));                      // (2,1) from i, (0,1) from i+1
                o[1][1][e] = fmaf(g[kt][0][0][e], wv[8][e], fmaf(g[kt][0][1][e], wv[6][e],
                             fmaf(g[kt][1][0][e], wv[2][e], fmaf(g[kt][1][1][e], wv[0][e], o[1][1][e]))));
            }
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int hi = 2 * i + a, wi = 2 * j + b;
                if (hi < d.Hi && wi < d.Wi) store4(dx + ((((size_t)n * d.Ti + ti) * d.Hi + hi) * d.Wi + wi) * d.Cin_p + cg * CH, o[a][b]);
            }
    }
}

extern "C" int pasn_dwconv3d_dgrad(const void* dy, const float* w, void* dx, const pasn_conv_desc* d, int dtype, void* stream) {
    PASN_REQUIRE(dy && w && dx && d, "null pointer");
    PASN_REQUIRE(d->Cin_p == d->Cout_p && d->Cin_p % 8 == 0, "depthwise conv keeps the channel stride");
    const bool s2 = d->kt == 3 && d->kh == 3 && d->kw == 3 && d->st == 1 && d->sh == 2 && d->sw == 2 && d->pt == 1 && d->ph == 1 && d->pw == 1 &&
                    d->Cout_p <= 512 && !tune("PASN_NO_DGRAD_S2");
    // the patch form is grid-stride (its weight staging amortises over many patches), 27 x Cp taps in LDS: <= 55 KB (Cout_p <= 512 checked above)
    const size_t items = s2 ? (size_t)d->N * d->Ti * ((d->Hi + 1) / 2) * ((d->Wi + 1) / 2) * (d->Cin_p / 4) : (size_t)d->N * d->Ti * d->Hi * d->Wi * (d->Cin_p / 8);
    const int blocks = (int)std::min<size_t>((items + 255) / 256, s2 ? 4096 : 1 << 20);
    const size_t lds = s2 ? (size_t)27 * d->Cout_p * sizeof(float) : 0;
    with_dtype(dtype, [&](auto tag) {
        using T = elem_t<decltype(tag)>;
        launch256(s2 ? dw_dgrad_s2_kernel<T> : dw_dgrad_kernel<T>, dim3(blocks), lds, (hipStream_t)stream, (const T*)dy, w, (T*)dx, *d);
    });
    return check_launch("dwconv3d_dgrad");
}

// ---- depthwise 3x3 (spatial) weight gradient, strip form -------------------------------------------------------------------
// item = (channel group, strip of WT outputs along w, HR consecutive output rows of one (n, to) plane); one temporal tap per
// blockIdx.z.  Per output row a thread loads the WT gradients and the three (WT-1)*SW+3 wide input rows once and feeds all nine
// spatial taps from registers (the row-per-thread kernel above re-loads every input pixel nine times and pays an integer
// division per row); the item decomposition is done once.  Partials per block, fixed-order combine by dw_wgrad_reduce_kernel.
namespace pasn {

// CH = 4 channels per thread (half the registers of 8, twice the resident waves -- the kernel is bound by load latency, not by
// bytes per load instruction); CGb = lanes per position (power of two >= Cp / CH)
// NA = temporal taps handled by one thread: 1 (one tap per blockIdx.z: x and dy stream from HBM once per tap) or 3 (all three in
// one pass: a third of the HBM traffic, three times the accumulators)
template <typename T, int SW, int WT, int NA>
__global__ __launch_bounds__(256) void dw_wgrad_strip_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ partial,
                                                             pasn_conv_desc d, int CG, int CGb, int strips, int HR, int hgroups, long items) {
    constexpr int CH = 4;
    __shared__ float red[256 * CH];
    constexpr int IW = (WT - 1) * SW + 3;
    const int cg = threadIdx.x % CGb, pl = threadIdx.x / CGb, PL = 256 / CGb;
    float acc[NA * 9][CH];
#pragma unroll
    for (int p = 0; p < NA * 9; ++p)
#pragma unroll
        for (int j = 0; j < CH; ++j) acc[p][j] = 0.0f;
    // over (n, to, hgroup, strip); a block keeps accumulating over several item groups before its one partial is written
    for (long item = (long)blockIdx.x * PL + pl; cg < CG && item < items; item += (long)gridDim.x * PL) {
        const int strip = (int)(item % strips);
        long q = item / strips;
        const int hg = (int)(q % hgroups);
        q /= hgroups;
        const int to = (int)(q % d.To), n = (int)(q / d.To);
        const int wo0 = strip * WT, wi0 = wo0 * SW - 1;
        const T* gp = dy + (((size_t)n * d.To + to) * d.Ho) * d.Wo * d.Cout_p + cg * CH;
        const int h1 = min(d.Ho, (hg + 1) * HR);
        {
            for (int ho = hg * HR; ho < h1; ++ho) {
                // every load of the row first (clamped addresses), the zeroing of out-of-image values afterwards: a select right after
                // a load makes hipcc wait for that load on the spot -- 18 dependent round trips per output row in the first version
                float g[WT][CH];
                unsigned gok = 0;
#pragma unroll
                for (int j = 0; j < WT; ++j) {
                    const int wo = wo0 + j;
                    const bool ok = wo < d.Wo;
                    load4(gp + ((size_t)ho * d.Wo + (ok ? wo : 0)) * d.Cout_p, g[j]);
                    gok |= (ok ? 1u : 0u) << j;
                }
#pragma unroll
                for (int ai = 0; ai < NA; ++ai) {
                const int a = NA == 1 ? (int)blockIdx.z : ai;
                const int ti = to * d.st - d.pt + a;
                const bool tok = ti >= 0 && ti < d.Ti;
                if (NA == 1 && !tok) continue;
                const T* xp = x + (((size_t)n * d.Ti + (tok ? ti : 0)) * d.Hi) * d.Wi * d.Cin_p + cg * CH;
                float xr[3][IW][CH];
                unsigned xok = 0;
#pragma unroll
                for (int dh = 0; dh < 3; ++dh) {
                    const int hi = ho * SW - 1 + dh;
                    const bool hok = tok && hi >= 0 && hi < d.Hi;
#pragma unroll
                    for (int i = 0; i < IW; ++i) {
                        const int wi = wi0 + i;
                        const bool ok = hok && wi >= 0 && wi < d.Wi;
                        load4(xp + ((size_t)(hok ? hi : 0) * d.Wi + (ok ? wi : 0)) * d.Cin_p, xr[dh][i]);
                        xok |= (ok ? 1u : 0u) << (dh * IW + i);
                    }
                }
                if (ai == 0) {
#pragma unroll
                    for (int j = 0; j < WT; ++j)
                        if (!((gok >> j) & 1u)) {
#pragma unroll
                            for (int e = 0; e < CH; ++e) g[j][e] = 0.0f;
                        }
                }
#pragma unroll
                for (int dh = 0; dh < 3; ++dh) {
#pragma unroll
                    for (int i = 0; i < IW; ++i)
                        if (!((xok >> (dh * IW + i)) & 1u)) {
#pragma unroll
                            for (int e = 0; e < CH; ++e) xr[dh][i][e] = 0.0f;
                        }
#pragma unroll
                    for (int dw_ = 0; dw_ < 3; ++dw_)
#pragma unroll
                        for (int j = 0; j < WT; ++j)
#pragma unroll
                            for (int e = 0; e < CH; ++e)
                                acc[ai * 9 + dh * 3 + dw_][e] = fmaf(g[j][e], xr[dh][j * SW + dw_][e], acc[ai * 9 + dh * 3 + dw_][e]);
                }
                }
            }
        }
    }
    const int taps = d.kt * 9;
    block_reduce_rows(acc, red, partial + ((size_t)blockIdx.x * taps + (size_t)(NA == 1 ? blockIdx.z : 0) * 9) * d.Cout_p, d.Cout_p, CG, CGb);
}

// ---- the core of the two T-marching kernels below: E = float, or f32x2 (packed FMAs) --------------------------------------------------
// Input row dh of frame ti (IW positions, converted) against the three-frame gradient ring -> the tap planes (a, dh, 0 .. 2) of acc.
// Temporal tap a pairs input frame ti with output frame ti - a + 1: a = 0 -> g2, 1 -> g1, 2 -> g0.
template <int SW, int WT, int IW, int N, typename E>
__device__ __forceinline__ void march_row_fma(E (&acc)[27][N], const E (&xr)[IW][N], const E (&g0)[WT][N], const E (&g1)[WT][N],
                                              const E (&g2)[WT][N], int dh) {
    static_assert(IW == (WT - 1) * SW + 3, "a strip of WT outputs reads (WT - 1) * SW + 3 input columns");
#pragma unroll
    for (int dw_ = 0; dw_ < 3; ++dw_)
#pragma unroll
        for (int j = 0; j < WT; ++j)
#pragma unroll
            for (int e = 0; e < N; ++e) {
                const E xv = xr[j * SW + dw_][e];
                acc[0 * 9 + dh * 3 + dw_][e] = __builtin_elementwise_fma(g2[j][e], xv, acc[0 * 9 + dh * 3 + dw_][e]);
                acc[1 * 9 + dh * 3 + dw_][e] = __builtin_elementwise_fma(g1[j][e], xv, acc[1 * 9 + dh * 3 + dw_][e]);
                acc[2 * 9 + dh * 3 + dw_][e] = __builtin_elementwise_fma(g0[j][e], xv, acc[2 * 9 + dh * 3 + dw_][e]);
            }
}
// (The ring shift g0 <- g1 <- g2 after it stays a loop in each kernel: behind a helper, over the whole ring or one strip column per call,
// the second marching kernel is scheduled differently -- 2-6 more VGPRs, or the same count and 0.4 % slower at 108 channels, 28 x 28.)

// ---- depthwise 3x3x3 weight gradient, T-marching form (stride (1,s,s), pad 1) -------------------------------------------------------
// The strip kernel above runs one temporal tap per blockIdx.z: every (frame, row) of x and dy is loaded and converted three times, 18
// loads for 108 FMAs.  It is VALU-issue bound at ~1 TB/s (the forward stencil, with the same 27 FMAs per element, runs at 2.4).  Here a
// thread owns (4 channels, a strip of WT outputs, one output row) and MARCHES ALONG T: the three rows of input frame ti are loaded and
// converted ONCE and meet the gradients of output frames ti+1, ti, ti-1 (temporal taps 0, 1, 2), which sit in a three-frame register
// ring -- 18 loads for 324 FMAs, 27 x 4 accumulators.
template <int SW, int WT>
__global__ __launch_bounds__(256, 2) void dw_wgrad_march_kernel(const __bf16* __restrict__ x, const __bf16* __restrict__ dy, float* __restrict__ partial,
                                                             pasn_conv_desc d, int CG, int CGb, int strips, long items) {
    typedef __bf16 T;
    constexpr int CH = 4;
    __shared__ float red[256 * CH];
    constexpr int IW = (WT - 1) * SW + 3;
    const int cg = threadIdx.x % CGb, pl = threadIdx.x / CGb, PL = 256 / CGb;
    float acc[27][CH];
#pragma unroll
    for (int p = 0; p < 27; ++p)
#pragma unroll
        for (int j = 0; j < CH; ++j) acc[p][j] = 0.0f;
    for (long item = (long)blockIdx.x * PL + pl; cg < CG && item < items; item += (long)gridDim.x * PL) {  // (n, ho, strip)
        const int strip = (int)(item % strips);
        const long q = item / strips;
        const int ho = (int)(q % d.Ho), n = (int)(q / d.Ho);
        const int wo0 = strip * WT, wi0 = wo0 * SW - 1;
        // gradients of this strip in frame `to` (clamped addresses; columns past the row are masked after the loads)
        const T* gp = dy + (((size_t)n * d.To) * d.Ho + ho) * d.Wo * d.Cout_p + cg * CH;
        const size_t gframe = (size_t)d.Ho * d.Wo * d.Cout_p;
        unsigned gmask = 0;
        int goff[WT];
#pragma unroll
        for (int j = 0; j < WT; ++j) {
            const bool ok = wo0 + j < d.Wo;
            goff[j] = (ok ? wo0 + j : 0) * d.Cout_p;
            gmask |= (ok ? 1u : 0u) << j;
        }
        // input rows hi = ho*SW - 1 + dh, columns wi0 .. wi0 + IW - 1 (clamped; masked after the loads)
        const T* xp = x + ((size_t)n * d.Ti) * d.Hi * d.Wi * d.Cin_p + cg * CH;
        const size_t xframe = (size_t)d.Hi * d.Wi * d.Cin_p;
        unsigned xmask = 0;
        int xoff[3][IW];
#pragma unroll
        for (int dh = 0; dh < 3; ++dh) {
            const int hi = ho * SW - 1 + dh;
            const bool hok = hi >= 0 && hi < d.Hi;
#pragma unroll
            for (int i = 0; i < IW; ++i) {
                const int wi = wi0 + i;
                const bool ok = hok && wi >= 0 && wi < d.Wi;
                xoff[dh][i] = ((hok ? hi : 0) * d.Wi + (ok ? wi : 0)) * d.Cin_p;
                xmask |= (ok ? 1u : 0u) << (dh * IW + i);
            }
        }
        float g0[WT][CH], g1[WT][CH], g2[WT][CH];  // gradients of output frames ti-1, ti, ti+1
#pragma unroll
        for (int j = 0; j < WT; ++j) {
            load4(gp + goff[j], g1[j]);
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                g0[j][e] = 0.0f;
                if (!((gmask >> j) & 1u)) g1[j][e] = 0.0f;
            }
        }
#pragma unroll 1
        for (int ti = 0; ti < d.Ti; ++ti) {
            // this frame's loads first (raw 8-byte words: 30 registers instead of 60 converted ones): the three input rows and the
            // gradients of frame ti + 1
            uint2 raw[3][IW];
#pragma unroll
            for (int dh = 0; dh < 3; ++dh)
#pragma unroll
                for (int i = 0; i < IW; ++i) raw[dh][i] = *reinterpret_cast<const uint2*>(xp + (size_t)ti * xframe + xoff[dh][i]);
            const bool next = ti + 1 < d.To;
#pragma unroll
            for (int j = 0; j < WT; ++j) load4(gp + (size_t)(next ? ti + 1 : ti) * gframe + goff[j], g2[j]);
#pragma unroll
            for (int j = 0; j < WT; ++j)
#pragma unroll
                for (int e = 0; e < CH; ++e)
                    if (!next || !((gmask >> j) & 1u)) g2[j][e] = 0.0f;
            // temporal tap a pairs input frame ti with output frame ti - a + 1: a = 0 -> g2, 1 -> g1, 2 -> g0
#pragma unroll
            for (int dh = 0; dh < 3; ++dh) {
                float xr[IW][CH];  // one row converted at a time
#pragma unroll
                for (int i = 0; i < IW; ++i) {
                    const bool ok = (xmask >> (dh * IW + i)) & 1u;
                    const unsigned lo = ok ? raw[dh][i].x : 0u, hi = ok ? raw[dh][i].y : 0u;
                    xr[i][0] = __uint_as_float(lo << 16);
                    xr[i][1] = __uint_as_float(lo & 0xffff0000u);
                    xr[i][2] = __uint_as_float(hi << 16);
                    xr[i][3] = __uint_as_float(hi & 0xffff0000u);
                }
                march_row_fma<SW>(acc, xr, g0, g1, g2, dh);
            }
#pragma unroll
            for (int j = 0; j < WT; ++j)
#pragma unroll
                for (int e = 0; e < CH; ++e) {
                    g0[j][e] = g1[j][e];
                    g1[j][e] = g2[j][e];
                }
        }
    }
    block_reduce_rows(acc, red, partial + (size_t)blockIdx.x * 27 * d.Cout_p, d.Cout_p, CG, CGb);
}

// ---- T-marching form, second cut (round 4) --------------------------------------------------------------------------------------------
// The kernel above asks for a step's 18 rows at the top of the step and waits for all of them (two resident waves per SIMD at 256 VGPRs
// cannot cover it): 1.1-1.7 TB/s, a quarter of its vector-issue bound.  Here
//  * a thread owns CH = 4 (or 2: 4-byte loads, half the accumulators, 4 waves per SIMD) channels of a strip of WT = 2 outputs,
//  * every row's registers are re-requested for the NEXT frame right after their conversion, ahead of the step's 27 x WT packed FMAs, and the
//    gradients one frame further ahead: a step never waits for a load it asked for in the same step,
//  * loads go through buffer descriptors: the frame offset is a scalar operand, positions outside the plane carry an out-of-range offset and
//    read as zero (no select per loaded value, no 64-bit address arithmetic per step),
//  * lanes map to (item, channel group) without padding the group count to a power of two.

template <int CW>
__device__ __forceinline__ void wg_load(unsigned (&r)[CW], __amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
    if constexpr (CW == 1) {
        r[0] = __builtin_amdgcn_raw_buffer_load_b32(rs, (int)voff, (int)soff, 0);
    } else {
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)voff, (int)soff, 0);
        r[0] = v[0];
        r[1] = v[1];
    }
}
template <int CW>
__device__ __forceinline__ void wg_cvt(const unsigned (&r)[CW], f32x2 (&v)[CW]) {
#pragma unroll
    for (int c = 0; c < CW; ++c) v[c] = f32x2{__uint_as_float(r[c] << 16), __uint_as_float(r[c] & 0xffff0000u)};
}

template <int SW, int WT, int CH>
__global__ __launch_bounds__(256) void dw_wgrad_march2_kernel(const __bf16* __restrict__ x, const __bf16* __restrict__ dy, float* __restrict__ partial,
                                                              pasn_conv_desc d, int CG, int PL, int strips, long items) {
    constexpr int IW = (WT - 1) * SW + 3, CW = CH / 2;
    __shared__ float red[256 * CH];
    const int cg = threadIdx.x % CG, pl = threadIdx.x / CG;
    const bool live = pl < PL;
    f32x2 acc[27][CW];
#pragma unroll
    for (int p = 0; p < 27; ++p)
#pragma unroll
        for (int c = 0; c < CW; ++c) acc[p][c] = f32x2{0.0f, 0.0f};
    const int Cp = d.Cout_p;
    const unsigned xframe = (unsigned)d.Hi * d.Wi * Cp * 2u, gframe = (unsigned)d.Ho * d.Wo * Cp * 2u;
    const __amdgpu_buffer_rsrc_t xrs = buffer_rsrc(x, (unsigned)d.N * d.Ti * xframe);
    const __amdgpu_buffer_rsrc_t grs = buffer_rsrc(dy, (unsigned)d.N * d.To * gframe);
    for (long item = (long)blockIdx.x * PL + pl; live && item < items; item += (long)gridDim.x * PL) {  // (n, ho, strip)
        const int strip = (int)(item % strips);
        const long q = item / strips;
        const int ho = (int)(q % d.Ho), n = (int)(q / d.Ho);
        const int wo0 = strip * WT, wi0 = wo0 * SW - 1;
        unsigned gv[WT], xv[3][IW];  // byte offsets inside frame 0 of clip n; outside the plane: out of range (reads as zero)
#pragma unroll
        for (int j = 0; j < WT; ++j)
            gv[j] = wo0 + j < d.Wo ? (unsigned)n * d.To * gframe + (unsigned)((ho * d.Wo + wo0 + j) * Cp + cg * CH) * 2u : BUF_OOB;
#pragma unroll
        for (int dh = 0; dh < 3; ++dh) {
            const int hi = ho * SW - 1 + dh;
            const bool hok = hi >= 0 && hi < d.Hi;
#pragma unroll
            for (int i = 0; i < IW; ++i) {
                const int wi = wi0 + i;
                xv[dh][i] = (hok && wi >= 0 && wi < d.Wi) ? (unsigned)n * d.Ti * xframe + (unsigned)((hi * d.Wi + wi) * Cp + cg * CH) * 2u : BUF_OOB;
            }
        }
        f32x2 g0[WT][CW], g1[WT][CW];  // gradients of output frames ti - 1, ti
        unsigned gn[WT][CW], raw[3][IW][CW];
#pragma unroll
        for (int j = 0; j < WT; ++j) wg_load<CW>(gn[j], grs, gv[j], 0u);
#pragma unroll
        for (int j = 0; j < WT; ++j) {
            wg_cvt<CW>(gn[j], g1[j]);
#pragma unroll
            for (int c = 0; c < CW; ++c) g0[j][c] = f32x2{0.0f, 0.0f};
        }
#pragma unroll
        for (int j = 0; j < WT; ++j) wg_load<CW>(gn[j], grs, d.To > 1 ? gv[j] : BUF_OOB, d.To > 1 ? gframe : 0u);
#pragma unroll
        for (int dh = 0; dh < 3; ++dh)
#pragma unroll
            for (int i = 0; i < IW; ++i) wg_load<CW>(raw[dh][i], xrs, xv[dh][i], 0u);
#pragma unroll 1
        for (int ti = 0; ti < d.Ti; ++ti) {
            f32x2 g2[WT][CW];  // gradient of output frame ti + 1 (zero past the clip)
#pragma unroll
            for (int j = 0; j < WT; ++j) wg_cvt<CW>(gn[j], g2[j]);
            {
                const bool more = ti + 2 < d.To;
                const unsigned so = (unsigned)min(ti + 2, d.To - 1) * gframe;
#pragma unroll
                for (int j = 0; j < WT; ++j) wg_load<CW>(gn[j], grs, more ? gv[j] : BUF_OOB, so);
            }
            f32x2 xc[3][IW][CW];
            const unsigned sx = (unsigned)min(ti + 1, d.Ti - 1) * xframe;  // (the last step's request is not used)
#pragma unroll
            for (int dh = 0; dh < 3; ++dh) {
#pragma unroll
                for (int i = 0; i < IW; ++i) wg_cvt<CW>(raw[dh][i], xc[dh][i]);
#pragma unroll
                for (int i = 0; i < IW; ++i) wg_load<CW>(raw[dh][i], xrs, xv[dh][i], sx);
            }
            // temporal tap a pairs input frame ti with output frame ti - a + 1: a = 0 -> g2, 1 -> g1, 2 -> g0
#pragma unroll
            for (int dh = 0; dh < 3; ++dh) march_row_fma<SW>(acc, xc[dh], g0, g1, g2, dh);
#pragma unroll
            for (int j = 0; j < WT; ++j)
#pragma unroll
                for (int c = 0; c < CW; ++c) {
                    g0[j][c] = g1[j][c];
                    g1[j][c] = g2[j][c];
                }
        }
    }
    // no padded lanes here (lanes per position = CG), so the reduce needs no lane guard
    block_reduce_rows<27, CH, false>([&](int p, int j) { return acc[p][j / 2][j % 2]; }, red, partial + (size_t)blockIdx.x * 27 * Cp, Cp, CG, CG, PL);
}

// dw[c][tap] = sum_chunks partial[chunk][tap*Cp + c]: 64 columns x 4 parts per block, parts combined in a fixed order
__global__ __launch_bounds__(256) void dw_wgrad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw, int chunks, int taps, int C,
                                                              int Cp) {
    __shared__ float red[4][64];
    const int col = blockIdx.x * 64 + (threadIdx.x & 63), part = threadIdx.x >> 6;
    const int L = taps * Cp;
    float s = 0.0f;
    if (col < L) {
#pragma unroll 8
        for (int ch = part; ch < chunks; ch += 4) s += partial[(size_t)ch * L + col];
    }
    red[part][threadIdx.x & 63] = s;
    __syncthreads();
    if (part == 0 && col < L) {
        const float tsum = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        const int tap = col / Cp, c = col % Cp;
        if (c < C) dw[(size_t)c * taps + tap] = tsum;
    }
}

// Temporal-only depthwise conv (kh = kw = 1, stride 1: the X3D stem's (5,1,1) conv): a thread owns 8 channels of one plane
// position and walks the frames; no divisions in the loop, the kt input frames of a step are the previous step's plus one.
template <typename T>
__global__ __launch_bounds__(256) void dw_wgrad_temporal_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ partial,
                                                                pasn_conv_desc d, int CG, int CGb, long items) {
    __shared__ float red[256 * 8];
    constexpr int KMAX = 5;
    const int cg = threadIdx.x % CGb, pl = threadIdx.x / CGb, PL = 256 / CGb;
    const long HW = (long)d.Hi * d.Wi;
    float acc[KMAX][8];
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k][j] = 0.0f;
    for (long item = (long)blockIdx.x * PL + pl; cg < CG && item < items; item += (long)gridDim.x * PL) {
        const long n = item / HW, pos = item % HW;
        const T* xp = x + ((size_t)n * d.Ti * HW + pos) * d.Cin_p + cg * 8;
        const T* gp = dy + ((size_t)n * d.To * HW + pos) * d.Cout_p + cg * 8;
        for (int t = 0; t < d.To; ++t) {
            float g[8];
            load8(gp + (size_t)t * HW * d.Cout_p, g);
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const int ti = t - d.pt + k;
                if (k < d.kt && ti >= 0 && ti < d.Ti) {
                    float v[8];
                    load8(xp + (size_t)ti * HW * d.Cin_p, v);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[k][j] = fmaf(g[j], v[j], acc[k][j]);
                }
            }
        }
    }
    block_reduce_rows(acc, red, partial + (size_t)blockIdx.x * d.kt * d.Cout_p, d.Cout_p, CG, CGb, d.kt);
}

static bool dw_temporal_ok(const pasn_conv_desc& d) {
    return d.kh == 1 && d.kw == 1 && d.kt <= 5 && d.st == 1 && d.sh == 1 && d.sw == 1 && d.ph == 0 && d.pw == 0 && d.Ti == d.To &&
           d.Cout_p % 8 == 0 && d.Cout_p <= 2048;
}
static long dw_temporal_blocks(const pasn_conv_desc& d) {
    const int b = pow2_at_least(d.Cout_p / 8);
    const long items = (long)d.N * d.Hi * d.Wi;
    return std::min<long>((items + 256 / b - 1) / (256 / b), 2048);
}

struct DwWgGeom {
    int ok, SW, WT, strips, HR, hgroups, CG, CGb, PL;
    long items, blocks;
};

static DwWgGeom dw_wgrad_strip_geom(const pasn_conv_desc& d) {
    DwWgGeom g{};
    if (d.kh != 3 || d.kw != 3 || d.ph != 1 || d.pw != 1 || d.sh != d.sw || (d.sh != 1 && d.sh != 2)) return g;
    if (d.Cout_p % 8 || d.Cout_p > 2048) return g;
    g.SW = d.sh;
    g.WT = g.SW == 1 ? 3 : 2;
    g.strips = ceil_div(d.Wo, g.WT);
    g.CG = d.Cout_p / 4;  // 4 channels per thread
    if (g.CG > 256) return g;
    g.CGb = pow2_at_least(g.CG);
    g.PL = 256 / g.CGb;
    // rows per item: enough items to fill the chip a few times over, few enough partial blocks to keep the combine small
    const long planes = (long)d.N * d.To;
    int HR = d.Ho;
    while (HR > 1 && planes * ceil_div(d.Ho, HR) * g.strips * g.CG < 400000) HR = (HR + 1) / 2;
    g.HR = HR;
    g.hgroups = ceil_div(d.Ho, HR);
    g.items = planes * g.hgroups * g.strips;
    // at most 768 blocks per temporal tap: each block loops over its item groups, so the partial buffer (and the combine
    // pass over it) stays small however many items there are
    g.blocks = std::min<long>((g.items + g.PL - 1) / g.PL, 768);
    g.ok = 1;
    return g;
}

// T-marching form: 3x3x3, temporal stride 1 and pad 1, frames kept (To == Ti)
static bool dw_wgrad_march_ok(const pasn_conv_desc& d) {
    if (tune_is("PASN_NO_DWWG_MARCH", '1')) return false;
    return d.kt == 3 && d.st == 1 && d.pt == 1 && d.To == d.Ti && d.kh == 3 && d.kw == 3 && d.ph == 1 && d.pw == 1;
}
static long dw_wgrad_march_blocks(const pasn_conv_desc& d, const DwWgGeom& g) {
    const long items = (long)d.N * d.Ho * g.strips;
    return std::min<long>((items + g.PL - 1) / g.PL, 1024);
}

struct DwWgMarch2 {
    int ok, SW, WT, CH, CG, PL, strips;
    long items, blocks;
};
// second cut of the marching kernel (PASN_DWWG_MARCH2=0: the first one).  Measured at the X3D-S shapes (tools/dwwg_bench.py,
// profiles/r04_dwwg_sweep.txt): 4 channels per thread and at most 512 blocks (= partial rows for the combine pass) is the best or within
// 2 % of the best arm at every shape; 2 channels / strips of 3 / 256-1024 blocks are switches
static DwWgMarch2 dw_wgrad_march2_geom(const pasn_conv_desc& d) {
    DwWgMarch2 g{};
    if (tune_is("PASN_DWWG_MARCH2", '0') || !dw_wgrad_march_ok(d) || d.sh != d.sw || (d.sh != 1 && d.sh != 2)) return g;
    g.CH = tune_is("PASN_DWWG_CH", '2') ? 2 : 4;
    if (d.Cout_p % g.CH || d.Cout_p / g.CH > 256) return g;
    // 32-bit byte offsets into either tensor
    if ((double)d.N * d.Ti * d.Hi * d.Wi * d.Cin_p * 2.0 >= 2147483648.0 || (double)d.N * d.To * d.Ho * d.Wo * d.Cout_p * 2.0 >= 2147483648.0) return g;
    g.SW = d.sh;
    g.WT = g.SW == 1 && tune_is("PASN_DWWG_WT", '3') ? 3 : 2;
    g.strips = ceil_div(d.Wo, g.WT);
    g.CG = d.Cout_p / g.CH;
    g.PL = 256 / g.CG;
    g.items = (long)d.N * d.Ho * g.strips;
    int cap = 512;
    if (const char* e = tune("PASN_DWWG_BLOCKS")) cap = std::max(64, atoi(e));
    g.blocks = std::min<long>((g.items + g.PL - 1) / g.PL, cap);
    g.ok = 1;
    return g;
}

// pasn_dwconv3d_wgrad: the kernel that takes the layer and the `blocks` partial rows of taps * Cout_p floats it writes into the workspace
// for dw_wgrad_reduce_kernel.  march2 = false: the ladder without the second marching kernel.
struct DwWgRoute {
    enum Arm { TEMPORAL, MARCH2, MARCH, STRIP, GENERIC } arm;
    DwWgGeom g;    // MARCH, STRIP
    DwWgMarch2 m;  // MARCH2
    long rpc;      // GENERIC: output rows per block
    long blocks;
    int taps;
};
static DwWgRoute dw_wgrad_route(const pasn_conv_desc& d, int dtype, bool march2 = true) {
    DwWgRoute r{};
    const bool fast = !tune("PASN_NO_DWWG_STRIP"), bf16 = dtype == PASN_BF16;
    if (fast && dw_temporal_ok(d)) r.arm = DwWgRoute::TEMPORAL, r.blocks = dw_temporal_blocks(d), r.taps = d.kt;
    else if (!fast || !(r.g = dw_wgrad_strip_geom(d)).ok) {
        r.arm = DwWgRoute::GENERIC, r.rpc = dw_wgrad_rows_per_chunk(d), r.taps = d.kt * d.kh * d.kw;
        r.blocks = ((long)d.N * d.To * d.Ho * d.Wo + r.rpc - 1) / r.rpc;
    } else if (bf16 && march2 && (r.m = dw_wgrad_march2_geom(d)).ok) r.arm = DwWgRoute::MARCH2, r.blocks = r.m.blocks, r.taps = 27;
    else if (bf16 && dw_wgrad_march_ok(d)) r.arm = DwWgRoute::MARCH, r.blocks = dw_wgrad_march_blocks(d, r.g), r.taps = 27;
    else r.arm = DwWgRoute::STRIP, r.blocks = r.g.blocks, r.taps = d.kt * 9;
    return r;
}

}  // namespace pasn

// The buffer is sized before the dtype is known: room for the arm of either dtype, and of either marching kernel.
extern "C" size_t pasn_dwconv3d_wgrad_workspace_floats(const pasn_conv_desc* d) {
    if (!d || d->Cout_p <= 0 || d->Cout_p % 8 || d->Cout_p > 2048) return 0;
    long rows = 0;
    for (int k = 0; k < 4; ++k) {
        const DwWgRoute r = dw_wgrad_route(*d, k & 1 ? PASN_BF16 : PASN_F32, k < 2);
        rows = std::max(rows, r.blocks * r.taps);
    }
    return (size_t)rows * d->Cout_p;
}

extern "C" int pasn_dwconv3d_wgrad(const void* x, const void* dy, float* ws, float* dw, const pasn_conv_desc* d, int dtype, void* stream) {
    PASN_REQUIRE(x && dy && ws && dw && d, "null pointer");
    PASN_REQUIRE(d->Cin_p == d->Cout_p && d->Cin_p % 8 == 0 && d->Cout_p <= 2048, "depthwise conv keeps the channel stride (<= 2048)");
    PASN_REQUIRE(d->kh * d->kw <= 9, "spatial window above 3x3 is not covered");
    hipStream_t s = (hipStream_t)stream;
    const DwWgRoute r = dw_wgrad_route(*d, dtype);
    const DwWgGeom& g = r.g;
    const DwWgMarch2& m = r.m;
    const bool na3 = d->kt == 3 && tune("PASN_DWWG_FUSED") && atoi(tune("PASN_DWWG_FUSED")) != 0;
    const int CG = d->Cout_p / 8, CGb = pow2_at_least(CG);  // TEMPORAL, GENERIC: 8 channels per thread
    const dim3 one((unsigned)r.blocks), per_tap((unsigned)r.blocks, 1, d->kt);
    const __bf16 *xb = (const __bf16*)x, *dyb = (const __bf16*)dy;  // the marching kernels are bf16 only
    auto march2 = [&](auto kernel) { launch256(kernel, one, 0, s, xb, dyb, ws, *d, m.CG, m.PL, m.strips, m.items); };
    auto march = [&](auto kernel) { launch256(kernel, one, 0, s, xb, dyb, ws, *d, g.CG, g.CGb, g.strips, (long)d->N * d->Ho * g.strips); };
    switch (r.arm) {
        case DwWgRoute::MARCH2:
            switch (m.SW * 100 + m.WT * 10 + m.CH) {
                case 222: march2(dw_wgrad_march2_kernel<2, 2, 2>); break;
                case 224: march2(dw_wgrad_march2_kernel<2, 2, 4>); break;
                case 132: march2(dw_wgrad_march2_kernel<1, 3, 2>); break;
                case 134: march2(dw_wgrad_march2_kernel<1, 3, 4>); break;
                case 122: march2(dw_wgrad_march2_kernel<1, 2, 2>); break;
                default: march2(dw_wgrad_march2_kernel<1, 2, 4>); break;
            }
            break;
        case DwWgRoute::MARCH:
            if (g.SW == 1) march(dw_wgrad_march_kernel<1, 3>);
            else march(dw_wgrad_march_kernel<2, 2>);
            break;
        default:
            with_dtype(dtype, [&](auto tag) {
                using T = elem_t<decltype(tag)>;
                const T *xt = (const T*)x, *dyt = (const T*)dy;
                auto strip = [&](auto fused, auto tap) { launch256(na3 ? fused : tap, na3 ? one : per_tap, 0, s, xt, dyt, ws, *d, g.CG, g.CGb, g.strips, g.HR, g.hgroups, g.items); };
                if (r.arm == DwWgRoute::TEMPORAL) launch256(dw_wgrad_temporal_kernel<T>, one, 0, s, xt, dyt, ws, *d, CG, CGb, (long)d->N * d->Hi * d->Wi);
                else if (r.arm == DwWgRoute::GENERIC) launch256(dw_wgrad_partial_kernel<T>, per_tap, 0, s, xt, dyt, ws, *d, CG, CGb, r.rpc);
                else if (g.SW == 1) strip(dw_wgrad_strip_kernel<T, 1, 3, 3>, dw_wgrad_strip_kernel<T, 1, 3, 1>);
                else strip(dw_wgrad_strip_kernel<T, 2, 2, 3>, dw_wgrad_strip_kernel<T, 2, 2, 1>);
            });
    }
    launch256(dw_wgrad_reduce_kernel, dim3(ceil_div((long)r.taps * d->Cout_p, 64)), 0, s, ws, dw, (int)r.blocks, r.taps, d->Cout, d->Cout_p);
    return check_launch("dwconv3d_wgrad");
}
