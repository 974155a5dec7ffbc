// The BLOCK-DIAGONAL matrix-core form of the depthwise 3x3x3 stencil (pad 1, bf16), shared by its three kernels: dwmfma.hip (the frame image
// arrives by LDS-DMA), x3d_expdw.hip (the image is born from the expand conv's accumulators) and x3d_edp.hip (four whole frames of a 7 x 7
// plane).  What lives here: the weight operands, the tap offsets, the MFMA chains of one staged frame with their role rotation, the output
// epilogue and the pool partial row.  What the kernels keep: staging and DMA roles, the T march with its barriers and counted waits,
// x3d_expdw's pinned fused schedule, x3d_edp's in-place accumulation, stamps, ablation checks (none in here), host geometry.
//
//   v_mfma_f32_16x16x32_bf16:  D[16 channels][16 positions] += A[16 channels][K = 32] * B[K = 32][16 positions]
//   K = 2 taps x 16 channels;  B[(tap, c')][p] = x[p + tap][c0 + c'] -- for lane (p = lane & 15, g = lane >> 4) ONE 16-byte read:
//   8 consecutive channels c0 + 8 (g & 1) .. of the position shifted by tap (g >> 1) of the pair, no conversion;
//   A[c][(tap, c')] = w[tap][c0 + c] if c' == c else 0 -- 15 such operands (3 kt x 5 pairs of the 9 (kh, kw) taps), built once per
//   wave and kept in registers.
//
// 1/16 of every MFMA is useful work, which is still 27 useful MACs per 16 x 16 outputs per 15 MFMAs x 16 cycles -- what the packed fp32
// FMAs alone would take if nothing else had to be issued -- and the vector unit is left to the epilogue (scale, bias, Swish, SE partial
// sums, bf16 stores).  A wave MARCHES ALONG T with three accumulator sets per position tile (outputs t-1, t, t+1): every operand read
// feeds the three kt taps.  The sets have FIXED registers per role and the rotation is done by the MFMAs themselves (the first MFMA of a
// chain reads the previous role's set as C and writes its own): no register moves.  The kernels are bound by vector-instruction ISSUE next
// to the MFMAs, not by MFMA time: what is compiled in (activation), kept out of loop-invariant hoisting (operand addresses) or issued
// unconditionally (stores, so that the wave can count them) below is there for that reason.
//
// The frame image the chains read: [staged row][position][SLOTS 16-byte slots, 8 used = one 64-channel quad], ROWP slots per staged row;
// wave w of the block's four reads slots 2 w, 2 w + 1 (its 16 channels).  Weights are rounded to bf16 (round-to-nearest-even), accumulation
// is fp32.  A zero weight times a non-finite activation of ANOTHER channel of the tile would leak (0 x inf); the trunk's activations are finite.
#pragma once
#include "common.h"

namespace pasn {

// One bf16 tap (its 16 bits) in the operand of lane m = lane & 15: of the lane's eight k elements only (m & 7) can be nonzero
__device__ __forceinline__ u32x4 bd_place(unsigned bits16, int m) {
    const int dwsel = (m & 7) >> 1, sh = (m & 1) * 16;
    const unsigned bits = bits16 << sh;
    return u32x4{dwsel == 0 ? bits : 0u, dwsel == 1 ? bits : 0u, dwsel == 2 ? bits : 0u, dwsel == 3 ? bits : 0u};
}

// Weight operands A[kt][pair] of channels c0 .. c0 + 15 from the fp32 taps w[27][Cp]: lane (m, q) holds k = 8q .. 8q+7 = tap (q >> 1) of the
// pair, channels 8 (q & 1) ..; only when m's half matches is its element nonzero.  All 15 loads first, from clamped (always valid)
// addresses: predicated loads became 15 dependent round trips (~35 us per block).
__device__ __forceinline__ void bd_build_operands(const float* __restrict__ w, int Cp, int c0, int m, int q, u32x4 (&A)[3][5]) {
    const int c = c0 + m;
    const bool mine = ((m >> 3) == (q & 1)) && c < Cp;
    float wv[3][5];
    const int cc = min(c, Cp - 1);
#pragma unroll
    for (int kt = 0; kt < 3; ++kt)
#pragma unroll
        for (int j = 0; j < 5; ++j) wv[kt][j] = w[(kt * 9 + min(2 * j + (q >> 1), 8)) * Cp + cc];
#pragma unroll
    for (int kt = 0; kt < 3; ++kt)
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const bool live = mine && 2 * j + (q >> 1) < 9;
            A[kt][j] = bd_place(live ? bf16_bits(wv[kt][j]) : 0u, m);
        }
}

// Byte offsets of this lane's tap inside the staged region per pair j: tap 2j + (q >> 1); the absent 10th tap reads the 9th's cell (its
// weights are zero).  ROWP: slots per staged row, SLOTS: slots per position.
template <int ROWP, int SLOTS>
__device__ __forceinline__ void bd_tap_offsets(int q, int (&tapoff)[5]) {
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int tap9 = min(2 * j + (q >> 1), 8);
        tapoff[j] = ((tap9 / 3) * ROWP + (tap9 % 3) * SLOTS) * 16;
    }
}

// Per-frame operand addresses: fbo = the frame image's offset in `ring` + this lane's tile-0 offset.  Kept out of the loop-invariant
// hoisting: ring slots x five taps of them otherwise stay live across the whole march.
__device__ __forceinline__ void bd_tap_addrs(const char* ring, int fbo, const int (&tapoff)[5], const char* (&ta)[5]) {
    asm volatile("" : "+v"(fbo));
#pragma unroll
    for (int j = 0; j < 5; ++j) ta[j] = ring + fbo + tapoff[j];
}

// The MFMA chains of one staged frame over NT position tiles LSTEP bytes apart: P = output t-1 (kt = 2), C = output t (kt = 1), N = output
// t+1 (kt = 0); DOP / DOC / DON: which chains run (a chain whose output frame lies outside the T chunk need not; a skipped chain's set is
// never read before it is restarted from zero).  Explicit two-deep operand pipeline: the 5 reads of tile l + 1 are issued before the MFMAs
// of tile l (left to itself the scheduler serialises read -> lgkmcnt(0) -> 3 MFMAs, one LDS round trip per tap pair: ~2500 cycles per frame).
template <int NT, int LSTEP, bool DOP, bool DOC, bool DON>
__device__ __forceinline__ void bd_chains(const char* ring, int fbo, const int (&tapoff)[5], const u32x4 (&A)[3][5], f32x4 (&P)[NT], f32x4 (&C)[NT],
                                          f32x4 (&N)[NT]) {
    constexpr int NCH = (DOP ? 1 : 0) + (DOC ? 1 : 0) + (DON ? 1 : 0);
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    const char* ta[5];
    bd_tap_addrs(ring, fbo, tapoff, ta);
    bf16x8 Bq[2][5];
#pragma unroll
    for (int j = 0; j < 5; ++j) Bq[0][j] = *reinterpret_cast<const bf16x8*>(ta[j]);
    __builtin_amdgcn_sched_group_barrier(0x100, 5, 0);
#pragma unroll
    for (int l = 0; l < NT; ++l) {
        if (l + 1 < NT) {
#pragma unroll
            for (int j = 0; j < 5; ++j) Bq[(l + 1) & 1][j] = *reinterpret_cast<const bf16x8*>(ta[j] + (l + 1) * LSTEP);
            __builtin_amdgcn_sched_group_barrier(0x100, 5, 0);
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const bf16x8 B = Bq[l & 1][j];
            // The role rotation rides in the first MFMA of every chain (D and C are different registers there): the new P is
            // the old C plus this frame's kt = 2 taps, the new C the old N plus kt = 1, the new N starts from a constant zero.
            // No register moves (2 x NT x 4 per frame otherwise).  Order P, C, N: each reads a set before it is overwritten.
            if (DOP) P[l] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, A[2][j]), B, j == 0 ? C[l] : P[l], 0, 0, 0);
            if (DOC) C[l] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, A[1][j]), B, j == 0 ? N[l] : C[l], 0, 0, 0);
            if (DON) N[l] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, A[0][j]), B, j == 0 ? zero4 : N[l], 0, 0, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 5 * NCH, 0);
    }
}

// A frame outside the clip (zero padding in T), or an idle wave: only the roles move on
template <int NT>
__device__ __forceinline__ void bd_rotate(f32x4 (&P)[NT], f32x4 (&C)[NT], f32x4 (&N)[NT]) {
#pragma unroll
    for (int l = 0; l < NT; ++l) {
        P[l] = C[l];
        C[l] = N[l];
        N[l] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
}

// Output epilogue of one finished frame: scale * P + bias, pool sums, activation, bf16, one 8-byte store per tile -- straight to memory: a
// wave owns 32 bytes (16 channels) of each of its 16 positions per store.  ACT: the activation compiled in (none / Swish: what X3D uses),
// -1 = `act` at run time (a run-time switch per tile is ~10 scalar branches x NT per frame on a kernel bound by instruction issue).
// Tile l holds output rows l RPT .. of the region; mrow_lim = this lane's row inside its tile, or a value no row count reaches for a lane
// without an output (a caller with many tiles passes it through an opaque register: the per-tile sums are then not hoisted out of its march);
// rows_valid = output rows of the region.  pacc: this lane's pool sums of its 4 channels [+ STATS (training forward):
// sums of squares, both of (v - kshift)].  Stores go through the frame's buffer descriptor yrsrc (num_records = one output frame) at
// yvoff + l ystep2 bytes: rows below the plane fall out of range and are dropped by the hardware, lanes without an output carry
// BUF_OOB -- no per-tile predicate, exec juggling or 64-bit address arithmetic, and every tile's store is ISSUED, so the wave can count them.
// Straight-line over ALL tiles (the pool sums are formed whether or not the launch has a row to write them to; the padded channels carry
// zero scale and bias instead of a tail mask): with wave-uniform branches per tile every tile's epilogue was its own scheduling region.
template <int ACT, bool STATS, int RPT, int NT>
__device__ __forceinline__ void bd_epilogue(const f32x4 (&P)[NT], f32x4 sc, f32x4 bs, f32x4 kshift, float (&pacc)[STATS ? 8 : 4], int mrow_lim,
                                            int rows_valid, int act, int tail_valid, __amdgpu_buffer_rsrc_t yrsrc, unsigned yvoff, int ystep2) {
#pragma unroll
    for (int l = 0; l < NT; ++l) {
        float v[4];
        const bool ok = l * RPT + mrow_lim < rows_valid;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = P[l][i] * sc[i] + bs[i];
        if constexpr (STATS) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float dv = ok ? v[i] - kshift[i] : 0.0f;
                pacc[i] += dv;
                pacc[4 + i] = fmaf(dv, dv, pacc[4 + i]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) pacc[i] += ok ? v[i] : 0.0f;
        }
        if constexpr (ACT == PASN_ACT_SWISH) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = v[i] * sigmoidf_(v[i]);
        } else if constexpr (ACT != PASN_ACT_NONE) {
            act_vec(v, act);
        }
        if (ACT == -1) mask_tail(v, tail_valid);  // (run-time activation: sigmoid(0) is not 0; tail_valid >= 4: nothing to mask)
        bf16x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (__bf16)v[i];
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o), yrsrc, (int)yvoff, l * ystep2, 0);
    }
}

// Pool partial row: sum over the 16 positions of the tile (lanes sharing q) in a fixed butterfly order, then the `writer` lane (m == 0 of
// a live channel group) stores its 4 channels at pr [and, STATS, the sums of squares one row of Cp floats further]
template <bool STATS>
__device__ __forceinline__ void bd_pool_row(float (&pacc)[STATS ? 8 : 4], float* pr, int Cp, bool writer) {
#pragma unroll
    for (int i = 0; i < (STATS ? 8 : 4); ++i) {
        float s = pacc[i];
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        s += __shfl_xor(s, 8);
        pacc[i] = s;
    }
    if (writer) {
        *reinterpret_cast<f32x4*>(pr) = f32x4{pacc[0], pacc[1], pacc[2], pacc[3]};
        if constexpr (STATS) *reinterpret_cast<f32x4*>(pr + Cp) = f32x4{pacc[4], pacc[5], pacc[6], pacc[7]};
    }
}

}  // namespace pasn
