// wgrad_tile.h -- the 32 x 32 tile of the dense weight gradient, once: what wgrad.hip (conv_wgrad_kernel, pw_wgrad_bf16_kernel,
// pw_wgrad_tile_kernel) and wgrad_halo.hip (conv_wgrad_halo_kernel, conv_wgrad_gather_kernel) share, and the one route that picks among them.
//
//   dW[co][ci][tap] = sum_rows dy[row][co] * x[in(row, tap)][ci]
//
// is a GEMM whose contraction index (the activation ROW) is the slow index of both channels-last operands, while
// v_mfma_f32_32x32x16_bf16 wants 8 consecutive k per lane.  So every bf16 kernel moves 8-row x 8-channel PATCHES: a thread loads the 8 rows
// of a patch (wg_load8: eight 16-byte loads at clamped addresses; which rows were real is collected in a bit mask and applied only when the
// patch is staged, since a select right after a load makes hipcc wait for that load on the spot and serialises the batch), zeroes the
// unreal rows, transposes the patch in registers (wg_transpose8x8, 32 v_perm_b32) and writes, per channel, its 8 consecutive rows as ONE
// 16-byte LDS write (wg_stage).  LDS then holds At[channel][rows] / Bt[channel][rows], a fragment read is one ds_read_b128 (wg_frag), and an
// accumulator tile leaves through fp32 atomics into dW (wg_tile_atomic) or as a plain store into partial[part][tap][co][ci]
// (wg_tile_store).  What differs between the kernels -- which rows a patch holds, how the steps are pipelined, which tiles a wave owns --
// stays in the kernels.
#pragma once
#include "common.h"

namespace pasn {

// in[r] = 8 channels of row r (2 per dword); out[c] = 8 rows of channel c (2 per dword)
__device__ __forceinline__ void wg_transpose8x8(const uint4 (&in)[8], uint4 (&out)[8]) {
    const unsigned* I = reinterpret_cast<const unsigned*>(in);
    unsigned* O = reinterpret_cast<unsigned*>(out);
#pragma unroll
    for (int q = 0; q < 4; ++q)        // channel pair (2q, 2q+1)
#pragma unroll
        for (int p = 0; p < 4; ++p) {  // row pair (2p, 2p+1)
            const unsigned lo = I[(2 * p) * 4 + q], hi = I[(2 * p + 1) * 4 + q];
            O[(2 * q) * 4 + p] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);      // low halves  -> channel 2q
            O[(2 * q + 1) * 4 + p] = __builtin_amdgcn_perm(hi, lo, 0x07060302u);  // high halves -> channel 2q+1
        }
}

// Slot rotation.  A staging thread writes the 8 rows of channels 8 cg .. 8 cg + 7 as eight 16-byte LDS writes, and the 8 lanes a
// ds_write_b128 serves together hold 8 CONSECUTIVE channel groups of one row octet: 8 * pitch bytes apart = a multiple of 128 bytes whatever the
// pitch -- one bank group, 8-way conflicts on every staging write (SQ counters, tools/pmc_lds_audit.sh: 24 LDS cycles per LDS instruction, 78 %
// of them conflicts, in every pointwise weight-gradient kernel).  Rotating a channel row's slots by its channel group, slot' = (slot + cg) mod
// slots, spreads the 8 lanes over 8 slots; a fragment read (32 channel rows of one slot) adds the row's group the same way: 17 slots of pitch x
// channel row + rotation stays conflict-free except for one pair of lanes per group.  (slots is a power of two.)
__device__ __forceinline__ int wg_slot(int slot, int cg, int slots) { return (slot + cg) & (slots - 1); }

// lane m's fragment of 32-channel tile `tile` of a rotated operand T[channel][slots * 8 rows]: the 8 rows of slot `slot` (= kk * 2 + h)
template <int SLOTS>
__device__ __forceinline__ bf16x8 wg_frag(const unsigned char* T, int pitch, int tile, int m, int slot) {
    return *reinterpret_cast<const bf16x8*>(T + (size_t)(tile * 32 + m) * pitch + wg_slot(slot, tile * 4 + (m >> 3), SLOTS) * 16);
}

// Rows first .. first + 7 of a channels-last tensor (src: already at the patch's first channel; rowlen: its channel stride), every load
// issued whatever the row: a row at or past `end`, or any row of a patch that is not `live`, reads row `fallback` instead and gets no
// bit in okbits.  Row: int where the host bounds rows * channels by 2^31 (halo, gather), long in pw_wgrad_tile_kernel.
// (pw_wgrad_bf16_kernel keeps its own loop: its rows may go through the window map, row by row.)
template <typename Row>
__device__ __forceinline__ void wg_load8(const __bf16* src, Row first, Row end, Row fallback, bool live, int rowlen, uint4 (&pre)[8],
                                         unsigned& okbits) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const bool ok = live && first + i < end;
        pre[i] = *reinterpret_cast<const uint4*>(src + (ok ? first + i : fallback) * rowlen);
        okbits |= (ok ? 1u : 0u) << i;
    }
}

// The staging step: zero the rows whose bit in okbits is clear, transpose, eight 16-byte LDS writes one channel row (pitch bytes) apart.
// The destination is the BYTE OFFSET dst into the block's LDS: a pointer kept in a register array loses its address space, and every
// store through it becomes a flat_store.
__device__ __forceinline__ void wg_stage(unsigned char* lds, int dst, int pitch, uint4 (&pre)[8], unsigned okbits) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (!((okbits >> i) & 1u)) pre[i] = make_uint4(0, 0, 0, 0);
    uint4 out[8];
    wg_transpose8x8(pre, out);
#pragma unroll
    for (int c = 0; c < 8; ++c) *reinterpret_cast<uint4*>(lds + dst + c * pitch) = out[c];
}

// Output row -> input row of tap (tt, th, tw) through the conv's window map, by divisions; false (and row 0): the tap leaves the input.
__device__ __forceinline__ bool wg_window_row(const pasn_conv_desc& d, long row, int tt, int th, int tw, long& in_row) {
    const int wo = (int)(row % d.Wo);
    long q = row / d.Wo;
    const int ho = (int)(q % d.Ho);
    q /= d.Ho;
    const int to = (int)(q % d.To), n = (int)(q / d.To);
    const int ti = to * d.st - d.pt + tt, hi = ho * d.sh - d.ph + th, wi = wo * d.sw - d.pw + tw;
    const bool in = ti >= 0 && ti < d.Ti && hi >= 0 && hi < d.Hi && wi >= 0 && wi < d.Wi;
    in_row = in ? (((long)n * d.Ti + ti) * d.Hi + hi) * d.Wi + wi : 0;
    return in;
}

// An accumulator tile's way out.  Element `reg` of lane (m, h) is row (= co offset) acc_row(reg, h), column (= ci offset) m.
// dw[(co * Cin + ci) * taps + tap] += acc, channels past the layer's dropped (split-K over the grid: dw zeroed by the caller)
__device__ __forceinline__ void wg_tile_atomic(float* dw, const f32x16& acc, int co0, int ci, int h, int Cout, int Cin, int taps, int tap) {
    if (ci < Cin) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int co = co0 + acc_row(reg, h);
            if (co < Cout) unsafeAtomicAdd(dw + ((size_t)co * Cin + ci) * taps + tap, acc[reg]);
        }
    }
}
// partial[part][tap][co][ci] = acc (padded extents Cout_r x Cin_r: every element of a tile is stored)
__device__ __forceinline__ void wg_tile_store(float* partial, const f32x16& acc, int part, int taps, int tap, int co0, int ci, int h, int Cout_r,
                                              int Cin_r) {
    float* base = partial + (((size_t)part * taps + tap) * Cout_r) * Cin_r + ci;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) base[(size_t)(co0 + acc_row(reg, h)) * Cin_r] = acc[reg];
}

// ---- the route (DESIGN.md "Routes"): which kernel takes a dense weight gradient, with the taken arm's whole geometry.  wgrad_route()
// (wgrad.hip) is the only place that tests a switch, an LDS size or a launch limit; the workspace size, the probes and the launches read this.
constexpr int WH_KT = 128;  // rows per step of the halo and gather kernels

struct WhGeom {  // conv_wgrad_halo_kernel's argument
    int mode;        // 0: (1,3,3) spatial taps, 1: (3,1,1) temporal taps
    int taps;        // 9 | 3
    int HAL;         // mode 0: halo rows either side of a copy (multiple of 64, >= W); mode 1: 0
    int L;           // rows per copy (WH_KT + 2 HAL)
    int pitchA, pitchB;
    int co_tiles, ci_tiles, co_groups, ci_groups;
    int rows_per_block, parts;
    int Cout_r, Cin_r;  // padded extents of the partial buffer
};

struct WgradRoute {
    // HALO:    conv_wgrad_halo_kernel<COT = sel_a, PW = sel_b>, mode h.mode -> partial buffer (wgrad_halo.hip)
    // GATHER:  conv_wgrad_gather_kernel                                     -> partial buffer (wgrad_halo.hip)
    // TILE:    pw_wgrad_tile_kernel<COT = sel_a, CIT = sel_b>               -> atomics
    // LDS:     pw_wgrad_bf16_kernel<KT = sel_a, TPW = sel_b>                -> atomics
    // GENERIC: conv_wgrad_kernel<T = dtype, PW = sel_b>                     -> atomics
    enum Arm { GENERIC = 1, LDS, TILE, HALO, GATHER } arm;
    int sel_a, sel_b;
    dim3 grid;
    size_t lds;
    int rows_per_block;   // GENERIC: per wave
    long parts;           // row partitions: the fp32 adds a dw element receives (atomic arms) / the partitions of the partial buffer
    int co_split, ci_split;  // LDS: 32-channel tiles staged per block; TILE: tile groups; GATHER: (-, ci pairs); GENERIC: (-, ci tiles)
    int gy2;              // TILE: tile groups of the 1-D XCD block map, 0 = 2-D grid
    long tiles;           // GENERIC: (co, ci, tap) tiles = grid.y (checked against the launch limit where it is launched)
    int taps, Cout_r, Cin_r;  // partial-buffer arms: its padded extents ...
    size_t partial_bytes;     // ... and size, 0 in the atomic arms
    WhGeom h;             // HALO
};
WgradRoute wgrad_route(const pasn_conv_desc& d, int dtype, bool has_ws, bool lds_switch = true);
// wgrad_halo.hip: launches the HALO / GATHER arm into ws and reduces the partitions into dw
void wgrad_partial_launch(const WgradRoute& r, const void* x, const void* dy, float* dw, void* ws, const pasn_conv_desc& d, hipStream_t s);

}  // namespace pasn
