// Weight gradient of the stride-1 "same" windowed convs (bf16): (1,3,3) and (3,1,1) of R(2+1)D-18, 3x3 of ResNet-18
// (training path of resnet_features.py:49-66,307-327; `loss.backward()` in Video_XProtoNet_e2e.py:118-141).
//
//   dW[co][ci][tap] = sum_rows dy[row][co] * x[row + off(tap)][ci]        (zero where the tap leaves the image / the clip)
//
// pw_wgrad_bf16_kernel ran these as one pointwise gradient per tap (blockIdx.z): every tap re-read dy and x, every y-block staged all
// channels, every staged row paid three integer divisions for the window map, and the split-K atomics landed 36 bytes apart (tap is the
// fast index of dW).  R(2+1)D-18 at 8 x 32 x 112 x 112: 29.1 of the 41.3 ms training step, 139 GB/s; the 64 -> 144 (1,3,3) layer 2.5 ms
// (its forward: 0.2 ms).  Here:
//   * a block of 8 waves owns up to 3 output-channel tiles x 2 input-channel tiles x ALL taps (<= 54 32x32 tiles: a wave holds <= 3
//     (ci tile, tap) pairs x 3 co tiles in accumulators) and walks its row partition 128 rows at a time;
//   * per step dy is staged once (8 x 8 register transpose -> At[co][128 rows], as in the pointwise kernel) and x THREE times, each copy a
//     different row shift: MODE 0 (1,3,3): copy e holds x[row + e - 1] over the step's rows plus a halo of W rows either side, so tap (b, e)
//     is copy e read at the (even) offset (b - 1) W -- a 4-byte-aligned fragment read; rows whose column wraps over the image border are
//     zeroed while the copy is staged (copy 0: source column W - 1, copy 2: source column 0); the rows whose tap leaves the image
//     vertically (a few octets per frame) are masked in the fragment.  MODE 1 (3,1,1): copy a holds x[row + (a - 1) H W], tap a reads it
//     unshifted; frames that wrap over the clip are zeroed at staging;
//   * no atomics: a block stores its tiles to partial[partition][tap][co][ci] (contiguous 128-byte runs) and conv_wgrad_reduce_kernel sums
//     the partitions in index order into dW[co][ci][tap] -- deterministic, and the 36-byte scatter happens once on 83 k values instead of
//     once per partition.
#include "wgrad_tile.h"

namespace pasn {

template <int COT, int PW>
__global__ __launch_bounds__(512) void conv_wgrad_halo_kernel(const __bf16* __restrict__ x, const __bf16* __restrict__ dy, float* __restrict__ partial,
                                                              pasn_conv_desc d, WhGeom g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    unsigned char* const At = lds;                                            // [COT*32][pitchA]
    unsigned char* const Bt = lds + (size_t)COT * 32 * g.pitchA;              // [3][64][pitchB]
    unsigned char* const mb = Bt + (size_t)3 * 64 * g.pitchB;                 // [2][WH_KT/8] row-validity bytes (mode 0)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lane & 31, h = lane >> 5;
    const long M = (long)d.N * d.To * d.Ho * d.Wo;
    const int W = d.Wi, H = d.Hi, T = d.Ti, FR = d.Hi * d.Wi;
    const long r0 = (long)blockIdx.x * g.rows_per_block, r1 = min(M, r0 + g.rows_per_block);
    const int co0 = blockIdx.y * COT * 32, ci0 = blockIdx.z * 64;
    const int cit = min(2, g.ci_tiles - (int)blockIdx.z * 2);  // ci tiles of this block
    const int P = cit * g.taps;                                 // (ci tile, tap) pairs of this block

    // ---- this wave's pairs: p = wave + 8 i -> copy, LDS shift, row-mask selector ----
    int p_ci[PW], p_tap[PW], p_copy[PW], p_shift[PW], p_msel[PW];
    bool p_ok[PW];
#pragma unroll
    for (int i = 0; i < PW; ++i) {
        const int p = wave + 8 * i;
        p_ok[i] = p < P;
        const int pc = p_ok[i] ? p : 0;
        p_ci[i] = pc / g.taps;
        p_tap[i] = pc % g.taps;
        if (g.mode == 0) {
            const int b = p_tap[i] / 3, e = p_tap[i] % 3;
            p_copy[i] = e;
            p_shift[i] = g.HAL + (b - 1) * W;
            p_msel[i] = b == 0 ? 0 : (b == 2 ? 1 : -1);
        } else {
            p_copy[i] = p_tap[i];
            p_shift[i] = 0;
            p_msel[i] = -1;
        }
    }
    f32x16 acc[PW][COT];
#pragma unroll
    for (int i = 0; i < PW; ++i)
#pragma unroll
        for (int c = 0; c < COT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][c][r] = 0.0f;

    // ---- staging roles (the same every step): units = dy patches (octet, channel group), then the three x copies (copy, octet, group);
    // a thread owns units tid and tid + 512 ----
    const int dy_cgs = COT * 4, dy_units = (WH_KT / 8) * dy_cgs;
    const int x_oct = g.L / 8, x_units = 3 * x_oct * 8;
    const int units = dy_units + x_units;  // <= 1024 (host-checked)
    int u_dst[2];                 // LDS byte offset (wg_stage), -1 = no unit
    int u_pitch[2], u_cp[2];      // u_cp: -1 = dy patch, 0..2 = x copy
    int u_row[2];                 // source row of the patch's first row in the CURRENT step (32-bit: the host bounds rows * channels by 2^31)
    int u_ch[2];                  // first channel of the patch, -1 = zeros (channel group past the tensor / no unit)
    int u_rowlen[2];
    int u_coord[2], u_within[2];  // x copies: column (mode 0) / frame and in-frame position (mode 1) of that source row, kept incrementally
    const int Mi = (int)M, r0i = (int)r0, r1i = (int)r1;
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const int u = tid + v * 512;
        u_dst[v] = -1;
        u_ch[v] = -1;
        u_pitch[v] = 0;
        u_cp[v] = -1;
        u_row[v] = r0i;
        u_rowlen[v] = 0;
        u_coord[v] = u_within[v] = 0;
        if (u < dy_units) {
            const int cg = u % dy_cgs, oct = u / dy_cgs;
            const int ch = co0 + cg * 8;
            u_dst[v] = (cg * 8) * g.pitchA + oct * 16;
            u_pitch[v] = g.pitchA;
            u_row[v] = r0i + oct * 8;
            u_rowlen[v] = d.Cout_p;
            if (ch < d.Cout_p) u_ch[v] = ch;
        } else if (u < units) {
            const int q = u - dy_units;
            const int cg = q & 7, oct = (q >> 3) % x_oct, cp = (q >> 3) / x_oct;
            const int ch = ci0 + cg * 8;
            u_dst[v] = COT * 32 * g.pitchA + (cp * 64 + cg * 8) * g.pitchB + oct * 16;
            u_pitch[v] = g.pitchB;
            u_cp[v] = cp;
            u_row[v] = r0i + oct * 8 + (g.mode == 0 ? -g.HAL + (cp - 1) : (cp - 1) * FR);
            u_rowlen[v] = d.Cin_p;
            if (ch < d.Cin_p) u_ch[v] = ch;
            if (g.mode == 0) {
                u_coord[v] = ((u_row[v] % W) + W) % W;  // rows before the tensor are masked by their sign; the column arithmetic is modular
            } else {
                const int sp = u_row[v] + FR * T;        // one clip period up: non-negative, same frame index modulo T
                u_within[v] = sp % FR;
                u_coord[v] = (sp / FR) % T;
            }
        }
    }
    const int step_w = WH_KT % W, step_fr = WH_KT % FR, step_t = (WH_KT / FR) % T;  // coordinate advance per 128-row step

    for (long rb = r0; rb < r1; rb += WH_KT) {
#pragma unroll
        for (int v = 0; v < 2; ++v) {  // one unit at a time: both in flight (64 staging registers) spilled the 9-tile instance
            uint4 pre[8];
            unsigned okbits = 0;
            const bool chok = u_ch[v] >= 0;
            const __bf16* src = (u_cp[v] < 0 ? dy : x) + (chok ? u_ch[v] : 0);
            const int s0 = u_row[v];
            if (u_cp[v] < 0) {  // dy rows of this partition
                wg_load8<int>(src, s0, r1i, r0i, chok, u_rowlen[v], pre, okbits);
            } else {
                // x rows of copy cp; a row is zero when its column (mode 0) / frame (mode 1) is the one that only a wrapped tap would read
                const int period = g.mode == 0 ? W : T;
                const int bad = u_cp[v] == 0 ? period - 1 : (u_cp[v] == 2 ? 0 : -1);
                int coord = u_coord[v], within = u_within[v];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int sr = s0 + i;
                    const bool ok = chok && sr >= 0 && sr < Mi && coord != bad;
                    pre[i] = *reinterpret_cast<const uint4*>(src + (ok ? sr : 0) * u_rowlen[v]);
                    okbits |= (ok ? 1u : 0u) << i;
                    if (g.mode == 0) {
                        coord = coord + 1 == W ? 0 : coord + 1;
                    } else if (++within == FR) {
                        within = 0;
                        coord = coord + 1 == T ? 0 : coord + 1;
                    }
                }
                // advance to the next step
                if (g.mode == 0) {
                    u_coord[v] += step_w;
                    if (u_coord[v] >= W) u_coord[v] -= W;
                } else {
                    u_within[v] += step_fr;
                    int carry = step_t;
                    if (u_within[v] >= FR) {
                        u_within[v] -= FR;
                        ++carry;
                    }
                    u_coord[v] += carry;
                    while (u_coord[v] >= T) u_coord[v] -= T;
                }
            }
            u_row[v] += WH_KT;
            if (u_dst[v] >= 0) wg_stage(lds, u_dst[v], u_pitch[v], pre, okbits);
        }
        if (g.mode == 0 && tid < WH_KT / 8) {  // rows whose tap row b = 0 / b = 2 leaves the image: bit i of byte [sel][octet] = row valid
            unsigned m0 = 0, m2 = 0;
            const int rr = (int)rb + tid * 8;
            int hh = (rr / W) % H, ww = rr % W;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                m0 |= (hh != 0 ? 1u : 0u) << i;
                m2 |= (hh != H - 1 ? 1u : 0u) << i;
                if (++ww == W) {
                    ww = 0;
                    hh = hh + 1 == H ? 0 : hh + 1;
                }
            }
            mb[tid] = (unsigned char)m0;
            mb[WH_KT / 8 + tid] = (unsigned char)m2;
        }
        __syncthreads();
#pragma unroll 2
        for (int kk = 0; kk < WH_KT / 16; ++kk) {
            bf16x8 a[COT];
#pragma unroll
            for (int c = 0; c < COT; ++c) a[c] = *reinterpret_cast<const bf16x8*>(At + (size_t)(c * 32 + m) * g.pitchA + (kk * 2 + h) * 16);
#pragma unroll
            for (int i = 0; i < PW; ++i) {
                if (p_ok[i]) {  // wave-uniform
                    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                    const unsigned* p32 = reinterpret_cast<const unsigned*>(Bt + ((size_t)p_copy[i] * 64 + p_ci[i] * 32 + m) * g.pitchB +
                                                                            (size_t)(kk * 16 + 8 * h + p_shift[i]) * 2);  // 4-byte aligned
                    u32x4 v;
                    v.x = p32[0];
                    v.y = p32[1];
                    v.z = p32[2];
                    v.w = p32[3];
                    if (p_msel[i] >= 0) {
                        const unsigned mk = mb[p_msel[i] * (WH_KT / 8) + kk * 2 + h];
                        if (__builtin_amdgcn_ballot_w64(mk != 0xffu)) {  // rare: an octet with a row in the first / last image row
                            v.x &= ((mk & 1u) ? 0x0000ffffu : 0u) | ((mk & 2u) ? 0xffff0000u : 0u);
                            v.y &= ((mk & 4u) ? 0x0000ffffu : 0u) | ((mk & 8u) ? 0xffff0000u : 0u);
                            v.z &= ((mk & 16u) ? 0x0000ffffu : 0u) | ((mk & 32u) ? 0xffff0000u : 0u);
                            v.w &= ((mk & 64u) ? 0x0000ffffu : 0u) | ((mk & 128u) ? 0xffff0000u : 0u);
                        }
                    }
                    const bf16x8 b = __builtin_bit_cast(bf16x8, v);
#pragma unroll
                    for (int c = 0; c < COT; ++c) acc[i][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[c], b, acc[i][c], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    // ---- partial[part][tap][co][ci]: rows = co (accumulator row), lane = ci ----
#pragma unroll
    for (int i = 0; i < PW; ++i) {
        if (!p_ok[i]) continue;
#pragma unroll
        for (int c = 0; c < COT; ++c)
            if ((blockIdx.y * COT + c) < g.co_tiles)
                wg_tile_store(partial, acc[i][c], blockIdx.x, g.taps, p_tap[i], co0 + c * 32, ci0 + p_ci[i] * 32 + m, h, g.Cout_r, g.Cin_r);
    }
}

// dW[co][ci][tap] += sum over partitions (index order) of partial[part][tap][co][ci]
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw, int parts, int taps, int Cout,
                                                                int Cin, int Cout_r, int Cin_r) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;  // (tap, co, ci), ci fastest: coalesced reads
    const long total = (long)taps * Cout * Cin;
    if (idx >= total) return;
    const int ci = (int)(idx % Cin), co = (int)((idx / Cin) % Cout), tap = (int)(idx / ((long)Cin * Cout));
    const size_t stride = (size_t)taps * Cout_r * Cin_r;
    const float* p = partial + ((size_t)tap * Cout_r + co) * Cin_r + ci;
    float s = 0.0f;
    int q = 0;
    for (; q + 8 <= parts; q += 8) {
        float t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = p[(size_t)(q + k) * stride];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += t[k];
    }
    for (; q < parts; ++q) s += p[(size_t)q * stride];
    dw[((size_t)co * Cin + ci) * taps + tap] += s;
}

// ---- the other windowed / strided convs (bf16): (1,3,3) stride (1,2,2), (3,1,1) stride (2,1,1), strided 1x1x1 shortcuts ----------------
// One tap per blockIdx.z, as a pointwise gradient whose x rows are GATHERED through the window map -- but tile-local (a block owns a 2 x 2
// group of 32 x 32 tiles and stages only their 64 + 64 channels, 128 output rows per step, one 8 x 8 patch per thread), with the window
// map advanced incrementally (three integer divisions per thread and step instead of three per row), and into the partial buffer
// (deterministic) instead of atomics 36 bytes apart.  pw_wgrad_bf16_kernel took 1.08 ms for the 64 -> 230 (1,3,3) stride-2 layer.
__global__ __launch_bounds__(256) void conv_wgrad_gather_kernel(const __bf16* __restrict__ x, const __bf16* __restrict__ dy, float* __restrict__ partial,
                                                                pasn_conv_desc d, int ci_pairs, int rows_per_block, int Cout_r, int Cin_r) {
    constexpr int PITCH = WH_KT * 2 + 16, SLOTS = WH_KT / 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    unsigned char* const At = lds;                         // [64 co channels][PITCH]
    unsigned char* const Bt = lds + (size_t)64 * PITCH;    // [64 ci channels][PITCH]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lane & 31, h = lane >> 5;
    const int R = d.N * d.To * d.Ho * d.Wo;  // output rows (host: rows * channels < 2^31)
    const int r0 = blockIdx.x * rows_per_block, r1 = min(R, r0 + rows_per_block);
    const int cop = blockIdx.y / ci_pairs, cip = blockIdx.y % ci_pairs;
    const int co0 = cop * 64, ci0 = cip * 64;
    const int taps = d.kt * d.kh * d.kw, tap = blockIdx.z;
    const int ta = tap / (d.kh * d.kw), tb = (tap / d.kw) % d.kh, te = tap % d.kw;
    // staging role: one 8-row x 8-channel patch per thread and step -- 16 row octets x (8 co + 8 ci channel groups)
    const int gch = tid & 15, r8 = tid >> 4;
    const bool is_a = gch < 8;
    const int cg = is_a ? gch : gch - 8;
    const int cp = is_a ? d.Cout_p : d.Cin_p;
    const int ch = (is_a ? co0 : ci0) + cg * 8;
    const bool ch_ok = ch < cp;
    const __bf16* src = (is_a ? dy : x) + (ch_ok ? ch : 0);
    const int dst = (is_a ? 0 : 64 * PITCH) + (cg * 8) * PITCH + wg_slot(r8, cg, SLOTS) * 16;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    const int tco = wave >> 1, tci = wave & 1;
    for (int rb = r0; rb < r1; rb += WH_KT) {
        uint4 pre[8];
        unsigned okbits = 0;
        const int rr = rb + r8 * 8;
        if (is_a) {
            wg_load8<int>(src, rr, r1, r0, ch_ok, cp, pre, okbits);
        } else {
            // output position of the patch's first row, then one position per row
            const int rc = min(rr, R - 1);
            int wo = rc % d.Wo, q = rc / d.Wo;
            int ho = q % d.Ho;
            q /= d.Ho;
            int to = q % d.To, n = q / d.To;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int ti = to * d.st - d.pt + ta, hi = ho * d.sh - d.ph + tb, wi = wo * d.sw - d.pw + te;
                const bool ok = ch_ok && rr + i < r1 && (unsigned)ti < (unsigned)d.Ti && (unsigned)hi < (unsigned)d.Hi && (unsigned)wi < (unsigned)d.Wi;
                const int row = ((n * d.Ti + ti) * d.Hi + hi) * d.Wi + wi;
                pre[i] = *reinterpret_cast<const uint4*>(src + (ok ? row : 0) * cp);
                okbits |= (ok ? 1u : 0u) << i;
                if (++wo == d.Wo) {
                    wo = 0;
                    if (++ho == d.Ho) {
                        ho = 0;
                        if (++to == d.To) {
                            to = 0;
                            ++n;
                        }
                    }
                }
            }
        }
        wg_stage(lds, dst, PITCH, pre, okbits);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < WH_KT / 16; ++kk) {
            const bf16x8 a = wg_frag<SLOTS>(At, PITCH, tco, m, kk * 2 + h);
            const bf16x8 b = wg_frag<SLOTS>(Bt, PITCH, tci, m, kk * 2 + h);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    // partial[part][tap][co][ci]
    const int ci = ci0 + tci * 32 + m;
    if (ci < Cin_r && co0 + tco * 32 < Cout_r) wg_tile_store(partial, acc, blockIdx.x, taps, tap, co0 + tco * 32, ci, h, Cout_r, Cin_r);
}

// the route's HALO / GATHER arm into the partial buffer ws, then the partitions summed in index order into dw
void wgrad_partial_launch(const WgradRoute& r, const void* x, const void* dy, float* dw, void* ws, const pasn_conv_desc& d, hipStream_t s) {
    const __bf16 *xb = (const __bf16*)x, *dyb = (const __bf16*)dy;
    if (r.arm == WgradRoute::GATHER) {
        hipLaunchKernelGGL(conv_wgrad_gather_kernel, r.grid, dim3(256), r.lds, s, xb, dyb, (float*)ws, d, r.ci_split, r.rows_per_block, r.Cout_r, r.Cin_r);
    }
#define PASN_WH(COT_, PW_)                                                                                                \
    if (r.arm == WgradRoute::HALO && r.sel_a == COT_ && r.sel_b == PW_) {                                                 \
        PASN_MAX_LDS(160 * 1024, conv_wgrad_halo_kernel<COT_, PW_>);                                                      \
        hipLaunchKernelGGL((conv_wgrad_halo_kernel<COT_, PW_>), r.grid, dim3(512), r.lds, s, xb, dyb, (float*)ws, d, r.h); \
    }
    PASN_WH(1, 1) PASN_WH(2, 1) PASN_WH(3, 1) PASN_WH(1, 2) PASN_WH(2, 2) PASN_WH(3, 2) PASN_WH(1, 3) PASN_WH(2, 3) PASN_WH(3, 3)
#undef PASN_WH
    const long total = (long)r.taps * d.Cout * d.Cin;
    hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3((unsigned)ceil_div(total, 256L)), dim3(256), 0, s, (const float*)ws, dw, (int)r.parts, r.taps, d.Cout,
                       d.Cin, r.Cout_r, r.Cin_r);
}

}  // namespace pasn
