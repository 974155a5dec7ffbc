// The per-channel TOEPLITZ form of the depthwise 3x3x3 stencil (stride 1, pad 1) on a channel-planar LDS image, shared by its two staging
// front ends: x3d_expdw_tz.hip (the image is born from the expand conv's accumulators) and dw_tz.hip (the image arrives channels-last by
// LDS-DMA and a transposing read).  What lives here: the layout of the frame ring and the output image, the operands, one stencil step, the
// way out (output roles, the 16-byte stores) and the pool reduction.  What the kernels keep: staging, the T march with its barriers and
// waits, stamps, host geometry.
//
// The stencil of channel c is D[out column m][row n] += sum_k A_c[m][k] B[k][n] with K = two (frame, row) shifts x 16 input columns:
// A_c = 3-diagonal Toeplitz matrices of tap rows (dt, dh, :) of channel c, B = 16 B per lane of the planar image (8 consecutive columns of one
// input row); N = 2 output frames x 8 output rows.  The 9 (dt, dh) rows pair up into 5 MFMAs and 5 operand reads per 224 outputs of a
// channel, ONE accumulator of 4 registers: no T-marching accumulator sets.  A wave's persistent state is the Toeplitz operands of its 2
// channels (40 registers), so four waves fit a SIMD.  A block = 8 waves = 16 channels x two 16 x 14-output tiles, marching along T two
// output frames per step over a ring of 4 frame images; outputs leave through a planar LDS image and ds_read_b64_tr_b16 (gfx950's
// transposing read): lane = output column, 2 reads = the 8 channels of one position = one 16-byte channels-last store.
#pragma once
#include "common.h"

namespace pasn {

typedef __attribute__((address_space(3))) s16x4* tz_lds_s16x4_t;

constexpr int TZ_RT = 8;                       // output rows of a tile
constexpr int TZ_BW = 14;                      // output columns of a tile
constexpr int TZ_CT = 2;                       // tiles of a block (x3d_expdw_tz.hip: side by side, 28 output columns; dw_tz.hip: row bands of the plane)
constexpr int TZ_RH = TZ_RT + 2;               // staged rows of a tile
constexpr int TZ_TS = TZ_RH * 32;              // bytes per (channel, tile) of a frame image: 10 rows x 16 columns
constexpr int TZ_CHS = TZ_CT * TZ_TS + 16;     // bytes per channel of a frame image: a multiple of 16 -- the B operand reads are ds_read_b128, and a 16-byte LDS access
                                               // off its alignment is replayed at 64 cycles (the first version, at + 8, spent 78 % of its time in the LDS: SQ_LDS_IDX_ACTIVE
                                               // 21 per LDS instruction); 164 dwords: the 16 channels of a staging ds_write_b64 fall on 8 bank pairs, 2-way
constexpr int TZ_FS = 16 * TZ_CHS;             // bytes per frame image: 10496, a multiple of 256 (the two frames a B operand read spans stay bank-disjoint)
static_assert(TZ_FS % 256 == 0 && TZ_CHS % 16 == 0, "frame images: 16-byte aligned channel planes, 256-byte aligned frames");
constexpr int TZ_NF = 4;                       // frame images in the ring: pairs k, k + 1
constexpr int TZ_ORS = 40;                     // bytes per row of the output image (10 dwords: the 16 rows of a ds_write_b64 hit 32 distinct banks; 8-byte aligned for the transposing read)
constexpr int TZ_OTS = 16 * TZ_ORS;            // bytes per (channel, tile) of the output image
constexpr int TZ_OCS = TZ_CT * TZ_OTS + 16;    // bytes per channel of the output image

// The 9 (dt, dh) tap rows of a channel in 5 MFMAs: K half h of MFMA j carries tap row 2 j + h (row 9 = none)
__device__ __forceinline__ constexpr int tz_row(int j, int h) { return 2 * j + h; }

// ds_read_b64_tr_b16 as inline assembly, for a kernel with LDS-DMAs in flight: through the builtin the compiler cannot tell the read from the
// cells a pending `buffer_load ... lds` writes and puts s_waitcnt vmcnt(0) in front of EVERY transposing read -- the rows requested for the
// next step awaited on the spot (dw_tz.hip's first version: 60.7 us where the block-diagonal kernel takes 55.4).  The waits for the reads'
// own results are part of the statement.  (EXEC must be all ones at a transposing read.)
template <int O0, int O1>
__device__ __forceinline__ void tz_read_tr2(unsigned addr, u32x2& a, u32x2& b) {
    asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%3\n\tds_read_b64_tr_b16 %1, %2 offset:%4\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(a), "=&v"(b)
                 : "v"(addr), "n"(O0), "n"(O1)
                 : "memory");
}
template <int O0, int O1, int O2, int O3>
__device__ __forceinline__ void tz_read_tr4(unsigned addr, u32x2& a, u32x2& b, u32x2& c, u32x2& e) {
    asm volatile("ds_read_b64_tr_b16 %0, %4 offset:%5\n\tds_read_b64_tr_b16 %1, %4 offset:%6\n\tds_read_b64_tr_b16 %2, %4 offset:%7\n\t"
                 "ds_read_b64_tr_b16 %3, %4 offset:%8\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(e)
                 : "v"(addr), "n"(O0), "n"(O1), "n"(O2), "n"(O3)
                 : "memory");
}
__device__ __forceinline__ unsigned tz_lds_addr(const void* p) { return (unsigned)(unsigned long)(__attribute__((address_space(3))) const char*)p; }

// ---- operands: the Toeplitz matrices of channels cA, cA + 1 (this wave's two) in registers for the launch, lane (m, q) = lane & 15, lane >> 4.
// FOLDB (the instances without pool sums): norm's scale meets the stencil weights BEFORE their rounding to bf16 and its bias is the
// accumulator's initial value -- no scale / bias arithmetic in the epilogue.  The squeeze-excite instances keep the scale in fp32 behind the
// MFMAs: a weight rounded after scaling shifts a channel's outputs by up to one bf16 ulp of each tap SYSTEMATICALLY, which the pool sum over
// 50 k positions does not average away (and they have no Swish epilogue to make room for).
template <bool FOLDB>
__device__ __forceinline__ void tz_build_operands(const float* __restrict__ w, const float* __restrict__ scale, const float* __restrict__ bias, int cA, int Cout,
                                                  int Cp, int m, int q, u32x4 (&AT)[2][5], float (&bsv)[2], float (&scv)[2]) {
    // operand of lane (m, q), K group q: tap row (dt, dh) = 2 j + (q >> 1), input columns 8 (q & 1) .. + 7; output column m takes taps
    // (w0, w1, w2) at input columns m, m + 1, m + 2: the 48-bit string w0 | w1 | w2 shifted to slot m - 8 (q & 1) of the lane's eight
    // (all 54 weights requested before the first is used -- one load round trip, not one per operand -- and the 128-bit shift
    // branch-free: the first version waited for six scalar loads and took a divergent branch per operand, 9-12 k cycles per block)
    const int sh = 16 * (m - 8 * (q & 1));                // bit position of the string's first tap in the lane's 128 bits: -128 .. 240
    // (vector loads on purpose -- an opaque zero joins the wave-uniform index: as 54 scalar loads the weights sat in 160 spilled SGPRs)
    int vz = 0;
    asm volatile("" : "+v"(vz));
    float wv[2][27];
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
        const int cc = min(cA + c2, Cout - 1) + vz;
#pragma unroll
        for (int e = 0; e < 27; ++e) wv[c2][e] = w[e * Cp + cc];
    }
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
        const int c = cA + c2;
        const bool chok = c < Cout;                       // padded channels: zero operands and zero bias -> act(0) = 0 for none / Swish
        const int cc = min(c, Cout - 1);
        const float sc = chok ? scale[cc] : 0.0f;
        scv[c2] = sc;
        bsv[c2] = chok ? bias[cc] : 0.0f;
        const float sw = FOLDB ? sc : 1.0f;
        const bool on = chok && m < TZ_BW;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            unsigned long long T[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int row = min(tz_row(j, h), 8);
                const unsigned long long b0 = bf16_bits(wv[c2][row * 3 + 0] * sw), b1 = bf16_bits(wv[c2][row * 3 + 1] * sw),
                                         b2 = bf16_bits(wv[c2][row * 3 + 2] * sw);
                T[h] = tz_row(j, h) < 9 ? (b0 | (b1 << 16) | (b2 << 32)) : 0ull;
            }
            const unsigned long long Tl = on ? ((q >> 1) ? T[1] : T[0]) : 0ull;
            // (Tl << sh) as two 64-bit halves, shift amounts clamped into range and the out-of-range cases selected away
            const unsigned long long lo = (sh >= 0 && sh < 64) ? Tl << (sh & 63) : (sh < 0 && sh > -64) ? Tl >> ((-sh) & 63) : 0ull;
            const unsigned long long hi = (sh >= 64 && sh < 128) ? Tl << ((sh - 64) & 63) : (sh > 0 && sh < 64) ? Tl >> ((64 - sh) & 63) : 0ull;
            AT[c2][j] = u32x4{(unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32)};
        }
    }
}

// B operand of MFMA j for this lane: frame t + f2 + dt - 1 (f2 = m >> 3, the lane's output frame of the step), row r8 + dh, columns
// 8 (q & 1) ..  bpk[j] bits 0 .. 19: the offset inside the image, bits 20 ..: the frame's number relative to the step's first frame (dt + f2)
__device__ __forceinline__ void tz_operand_offsets(int wave, int m, int q, int (&bpk)[5]) {
    const int f2 = m >> 3;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int row = min(tz_row(j, q >> 1), 8);            // (the empty half of the last MFMA reads tap row 8's operand: finite values times zero)
        bpk[j] = ((row / 3 + f2) << 20) | ((2 * wave) * TZ_CHS + ((m & 7) + row % 3) * 32 + (q & 1) * 16);
    }
}

// ---- one step of the T march for a wave's two channels x two tiles: the stencil of output frames t, t + 1 (t = t0 + 2 k; t + 1 >= t1: the
// second does not exist) from frame pairs k, k + 1 of the ring -> epilogue -> output image; call it under `if (wave_live)`.
// Pool sums are taken from the ROUNDED outputs (v_dot2c_f32_bf16 of the packed pairs the store needs anyway with 1 / 0 pairs: 2 instructions
// per tile where fp32 masks cost 5 and 8 registers): the rounding errors are unbiased and the squeeze-excite mean runs over thousands of
// positions per clip and channel.  (Swish + pool, which no X3D block has, pools the pre-activation in fp32.)  The 1 / 0 weights of a lane's
// four outputs come from the kernel's table ptab[tile][pair][64 lanes] (columns 14, 15 of a tile, rows and columns beyond the plane), masked
// by the missing second frame of an odd chunk's last step.  ONESPW, the one kernel-specific hook: on a tile that lies inside the plane
// (!ragged, wave-uniform) the weights are ones except for columns 14, 15 (mk23: lanes q = 3, second pair) -- no table read.
template <int ACT, bool POOL, bool ONESPW>
__device__ __forceinline__ void tz_stencil_step(const char* ring, char* outi, const u32x4 (&AT)[2][5], const float (&bsv)[2], const float (&scv)[2],
                                                const int (&bpk)[5], int k, bool tailf, int wave, int lane, const unsigned* ptab, bool ragged,
                                                unsigned mk23, float (&psum)[2]) {
    constexpr bool FOLDB = !POOL;
    const int m = lane & 15, q = lane >> 4, f2 = m >> 3;
    int so[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) so[j] = ((2 * k + (bpk[j] >> 20)) & (TZ_NF - 1)) * TZ_FS + (bpk[j] & 0xfffff);
    const unsigned fm = (tailf && f2) ? 0u : 0xffffffffu;
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
        for (int ct = 0; ct < TZ_CT; ++ct) {
            const char* bp = ring + c2 * TZ_CHS + ct * TZ_TS;
            bf16x8 B[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) B[j] = *reinterpret_cast<const bf16x8*>(bp + so[j]);
            const float a0 = FOLDB ? bsv[c2] : 0.0f;
            f32x4 acc = {a0, a0, a0, a0};
#pragma unroll
            for (int j = 0; j < 5; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, AT[c2][j]), B[j], acc, 0, 0, 0);
            float v[4] = {acc[0], acc[1], acc[2], acc[3]};
            if (!FOLDB) {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = v[i] * scv[c2] + bsv[c2];
            }
            if constexpr (ACT == PASN_ACT_SWISH) {
                if (POOL) {
                    const unsigned w01 = ptab[(ct * 2) * 64 + lane] & fm, w23 = ptab[(ct * 2 + 1) * 64 + lane] & fm;
#pragma unroll
                    for (int i = 0; i < 4; ++i) psum[c2] += (((i < 2 ? w01 : w23) >> (16 * (i & 1))) & 0xffffu) ? v[i] : 0.0f;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = v[i] * sigmoidf_(v[i]);
            }
            const bf16x2 o0 = __builtin_convertvector(f32x2{v[0], v[1]}, bf16x2);
            const bf16x2 o1 = __builtin_convertvector(f32x2{v[2], v[3]}, bf16x2);
            if (POOL && ACT != PASN_ACT_SWISH) {
                unsigned w01 = 0x3f803f80u, w23 = mk23;
                if (!ONESPW || ragged || tailf) {  // wave-uniform
                    w01 = ptab[(ct * 2) * 64 + lane] & fm;
                    w23 = ptab[(ct * 2 + 1) * 64 + lane] & fm;
                }
                psum[c2] = __builtin_amdgcn_fdot2_f32_bf16(o0, __builtin_bit_cast(bf16x2, w01), psum[c2], false);
                psum[c2] = __builtin_amdgcn_fdot2_f32_bf16(o1, __builtin_bit_cast(bf16x2, w23), psum[c2], false);
            }
            *reinterpret_cast<u32x2*>(outi + (2 * wave + c2) * TZ_OCS + ct * TZ_OTS + m * TZ_ORS + q * 8) =
                u32x2{__builtin_bit_cast(unsigned, o0), __builtin_bit_cast(unsigned, o1)};
        }
}

// ---- the way out: 16-lane group G = tid >> 4 = (8 channels og = G & 1, tile ct = (G >> 1) & 1, output row n8 = G >> 2 of a tile), lane l16 =
// output column; the two frames of a step in turn.  tr_off: where this lane's transposing reads of the output image start (the second read of
// a frame + 4 TZ_OCS, the second frame + 8 TZ_ORS); ooff: byte offset of the lane's 8 channels inside an output frame, BUF_OOB where the
// tile leaves the plane.  Tile ct's origin in the plane is (h0 + ct cth, w0 + ct ctw); cut14: lanes 14, 15 hold no output column.
__device__ __forceinline__ void tz_output_roles(int tid, int cgi, const pasn_conv_desc& d, int h0, int w0, int cth, int ctw, bool cut14, int& tr_off,
                                                unsigned& ooff) {
    const int G = tid >> 4, l16 = tid & 15;
    const int og = G & 1, ct = (G >> 1) & 1, n8 = G >> 2;
    tr_off = (8 * og + (l16 >> 2)) * TZ_OCS + ct * TZ_OTS + n8 * TZ_ORS + (l16 & 3) * 8;
    const int ho = h0 + ct * cth + n8, wo = w0 + ct * ctw + l16;
    const bool ok = (!cut14 || l16 < TZ_BW) && wo < d.Wo && ho < d.Ho && cgi * 16 + 8 * og < d.Cout_p;
    ooff = ok ? (unsigned)(((ho * d.Wo + wo) * d.Cout_p + cgi * 16 + 8 * og) * 2) : BUF_OOB;
}

// One 16-byte channels-last store per output frame t, t + 1 of the step from the transposed registers (ua[ps]: channels 8 og .. + 3, ub[ps]:
// + 4 .. + 7 of this lane's column in frame ps).  The frame's offset rides in the VECTOR offset, soffset = 0: behind a 16-byte buffer store
// with an SGPR soffset the compiler puts no wait state before a VALU write to the store's data registers, and gfx950 needs one (dw_tz.hip met
// it: tools/store_hazard_scan.py, profiles/README.md).
__device__ __forceinline__ void tz_store_frames(const u32x2 (&ua)[2], const u32x2 (&ub)[2], __amdgpu_buffer_rsrc_t yrsrc, unsigned ooff, int t, int t1,
                                                unsigned oframe_bytes) {
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
        const int to = t + ps;
        const unsigned off = to < t1 ? ooff + (unsigned)to * oframe_bytes : BUF_OOB;
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{ua[ps].x, ua[ps].y, ub[ps].x, ub[ps].y}, yrsrc, (int)off, 0, 0);
    }
}

// Squeeze-excite partial row of this wave's two channels: the lanes' sums reduced across the wave, lane 0 writes pr[0], pr[1]
__device__ __forceinline__ void tz_pool_reduce(float (&psum)[2], float* pr, int lane) {
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
        float s = psum[c2];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
        psum[c2] = s;
    }
    if (lane == 0) {
        pr[0] = psum[0];
        pr[1] = psum[1];
    }
}

}  // namespace pasn
