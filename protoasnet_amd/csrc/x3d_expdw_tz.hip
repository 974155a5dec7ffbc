// Front half of an X3D block in ONE launch, second formulation (round 5): 1x1x1 expand conv + BN + ReLU -> depthwise 3x3x3 conv, stride 1,
// pad 1, + BN (+ Swish, + squeeze-excite pool partial rows), with the stencil as PER-CHANNEL TOEPLITZ matrix products on a CHANNEL-PLANAR
// image of the expanded activation.  (pytorchvideo's BottleneckTransform conv_a / conv_b as the x3d trunks instantiate them; the reference
// itself ships no X3D -- SURVEY 8a row 5.)
//
// Why a second formulation.  x3d_expdw.hip runs the stencil as v_mfma_f32_16x16x32_bf16 with BLOCK-DIAGONAL weight operands (K = 2 taps x 16
// channels): 1/16 of every MFMA is useful, 15 MFMAs and 5 LDS operand reads per (16 channels x 16 positions) tile and frame, each 16-cycle
// MFMA holds the SIMD's vector issue for 8 cycles, and the three T-marching accumulator sets plus 60 registers of operands keep it at two
// waves per SIMD -- on a kernel whose waves are bound by vector issue and wait 60 % of the time (profiles/README.md entries 84, 123,
// r04_fwd_pmc_pipes.txt).  The stencil's operand never exists in HBM: it is born in LDS from the expand conv's accumulators, so its layout
// is free.  Here:
//   * the expand conv is v_mfma_f32_16x16x32_bf16 with A = a staged ROW of 16 x positions (8 channels per lane, loaded straight from global
//     memory one step ahead: no x tile in LDS, no DMA) and B = the block's 16 expand channels (whole K in registers): the accumulator holds,
//     per lane, 4 CONSECUTIVE COLUMNS of ONE channel -- bias as the initial value, ReLU + rounding on packed pairs, border zeroing as a
//     bitwise AND, one ds_write_b64 into the frame image [channel][column tile][staged row][16 columns] (no lane swap, no select per element);
//   * the stencil runs per channel as Toeplitz matrix products on that image and the outputs leave through a planar LDS image and gfx950's
//     transposing read -- toeplitz.h, shared with dw_tz.hip: 5 MFMAs and 5 operand reads per 224 outputs of a channel (block-diagonal: 15 + 15
//     per 224 when three frames are counted), ONE accumulator of 4 registers initialised with norm_b's bias: no T-marching accumulator sets,
//     no role rotation, no scale / bias arithmetic.  A wave's persistent state is the Toeplitz operands of its 2 channels (40 registers), so
//     16 waves fit a CU (4 per SIMD; x3d_expdw: 8).
// Block = 8 waves = 16 expanded channels x (8 x 28 outputs) of one clip, marching along T two output frames per step over a ring of 4 frame
// images (2 pairs); two barriers per step: [stencil of pairs k, k + 1 -> output image] | [store, expand pair k + 2 over pair k, request the x
// rows of pair k + 3].
// Rounding points: the expanded activation is rounded to bf16 (as by the two separate launches), norm_a's scale meets the expand weights and
// norm_b's scale the stencil weights before THEIR rounding to bf16 (the separate launches apply the scales in fp32 after the MFMAs), fp32
// accumulation in a different order from x3d_expdw.hip's: results agree with both to one bf16 ulp of the output, not bit for bit.
#include "toeplitz.h"

namespace pasn {

constexpr int TZ_ET = 2 * TZ_RH * TZ_CT;       // expand tiles (staged row x column tile) per pair of frames: 40
constexpr int TZ_EW = TZ_ET / 8;               // ... per wave: 5

#ifdef PASN_TUNING
// shader-clock stamps of block 0 / wave 0 (tuning builds, PASN_TZ_STAMPS=1; tools/tz_bench.py prints them): [0] start, [1] operands built, [2] prologue
// done, then per step 6: stencil done, barrier passed, stores issued, expand done, loads issued, barrier passed
__device__ long long tz_stamps[2 + 6 * 10];
#define TZ_STAMP(i) do { if (g.abl && (int)blockIdx.x == g.abl - 1 && threadIdx.x == 0 && (i) < 62) tz_stamps[i] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
#else
#define TZ_STAMP(i) do { } while (0)
#endif

// KS32: 32-wide k-steps of the expand conv (1: block width <= 32 channels); ACT: the stencil's epilogue (PASN_ACT_NONE / PASN_ACT_SWISH);
// POOL: squeeze-excite partial sums
template <int KS32, int ACT, bool POOL>
__global__ __launch_bounds__(512, 4) void x3d_expdw_tz_kernel(const __bf16* __restrict__ x, const __bf16* __restrict__ wa, const float* __restrict__ ba,
                                                              const float* __restrict__ w, const float* __restrict__ scale,
                                                              const float* __restrict__ bias, __bf16* __restrict__ y, float* __restrict__ pool,
                                                              pasn_conv_desc d, int Cin_p, int nks, XeGeom g) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    char* const ring = smem;                                  // [TZ_NF][TZ_FS]
    char* const outi = smem + TZ_NF * TZ_FS;                  // [16 channels][TZ_OCS]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lane & 15, q = lane >> 4;
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int cgi = lb % g.tzCG, r1 = lb / g.tzCG;
    const int regions = g.tzRTH * g.tzRTW, units = g.tznT * regions;
    const int u = r1 % units, n = r1 / units;
    const int tch = u / regions, reg = u - tch * regions;
    const int rth = reg / g.tzRTW, rtw = reg - rth * g.tzRTW;
    const int t0 = tch * g.tzTc, t1 = min(t0 + g.tzTc, d.To);
    const int h0 = rth * TZ_RT, w0 = rtw * (TZ_CT * TZ_BW);
    const int Cp = d.Cout_p, Ti = d.Ti, Hi = d.Hi, Wi = d.Wi;
    const int steps = (t1 - t0 + 1) >> 1;                     // output frames t0 + 2 k, t0 + 2 k + 1; input pairs 0 .. steps: frames (t0 - 1 + 2 p, t0 + 2 p)
    const int pieces = Cin_p >> 3;
    TZ_STAMP(0);

    // ---- expand roles: this lane = expand channel m of the block for 4 consecutive staged columns 4 q .. ----
    const int ce = cgi * 16 + m;
    bf16x8 WB[KS32];
    {
        const int ectiles = (Cp + 31) >> 5;
        const int ctile = min(ce >> 5, ectiles - 1), c32 = ce & 31;
#pragma unroll
        for (int k2 = 0; k2 < KS32; ++k2) {
            const int ks16 = 2 * k2 + (q >> 1);
            const bool ok = ks16 < nks && (ce >> 5) < ectiles;
            const bf16x8 v = load_frag<__bf16>(wa + (((long)ctile * nks + min(ks16, nks - 1)) * 64 + (q & 1) * 32 + c32) * 8);
            WB[k2] = ok ? v : zero_frag<__bf16>();
        }
    }
    const float biasE = ce < Cp ? ba[ce] : 0.0f;
    // border zeroing of the expanded activation (the stencil pads the EXPANDED tensor with zeros): columns as AND masks on packed pairs
    // (scalars, not arrays: the column tile of a wave's expand tile is wave-uniform but not a compile-time constant, and an array indexed by it goes to scratch)
    auto colmask = [&](int wb) -> unsigned { return ((unsigned)wb < (unsigned)Wi ? 0xffffu : 0u) | ((unsigned)(wb + 1) < (unsigned)Wi ? 0xffff0000u : 0u); };
    const unsigned cm00 = colmask(w0 - 1 + 4 * q), cm01 = colmask(w0 - 1 + 4 * q + 2);
    const unsigned cm10 = colmask(w0 - 1 + TZ_BW + 4 * q), cm11 = colmask(w0 - 1 + TZ_BW + 4 * q + 2);
    // this lane's x row piece for expand tile (row 0, column tile ct): staged column m, channels 8 q ..
    auto xo = [&](int wi) -> unsigned { return (unsigned)wi < (unsigned)Wi ? (unsigned)((wi * Cin_p + min(q, pieces - 1) * 8) * 2) : BUF_OOB; };
    const unsigned xoff0 = xo(w0 - 1 + m), xoff1 = xo(w0 - 1 + TZ_BW + m);
    const long fx = (long)Hi * Wi * Cin_p;
    const unsigned fx_bytes = (unsigned)(fx * 2), rx_bytes = (unsigned)(Wi * Cin_p * 2);
    const __amdgpu_buffer_rsrc_t xrsrc = buffer_rsrc(x + (long)n * Ti * fx, (unsigned)Ti * fx_bytes);
    // expand tile i of this wave in pair p: e = 5 wave + i of the pair's 40 (frame, staged row, column tile)
    u32x4 xq[TZ_EW];
#pragma unroll
    for (int i = 0; i < TZ_EW; ++i) xq[i] = u32x4{0u, 0u, 0u, 0u};
    auto load_tile = [&](int p, int i) {
        const int e = wave * TZ_EW + i;
        const int fs = e / (TZ_RH * TZ_CT), rem = e - fs * (TZ_RH * TZ_CT);
        const int rr = rem >> 1, ct = rem & 1;
        const int f = t0 - 1 + 2 * p + fs, hi = h0 - 1 + rr;
        if (f >= 0 && f < Ti && (unsigned)hi < (unsigned)Hi)  // wave-uniform (rows / frames outside: zeroed by the row mask whatever the registers hold)
            xq[i] = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, (int)(ct ? xoff1 : xoff0), (int)((unsigned)f * fx_bytes + (unsigned)hi * rx_bytes), 0);
    };
    auto expand_tile = [&](int p, int i) {
        const int e = wave * TZ_EW + i;
        const int fs = e / (TZ_RH * TZ_CT), rem = e - fs * (TZ_RH * TZ_CT);
        const int rr = rem >> 1, ct = rem & 1;
        const int f = t0 - 1 + 2 * p + fs;
        f32x4 acc = {biasE, biasE, biasE, biasE};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xq[i]), WB[0], acc, 0, 0, 0);
        const bool rowok = f >= 0 && f < Ti && (unsigned)(h0 - 1 + rr) < (unsigned)Hi;  // wave-uniform
        const unsigned rmask = rowok ? 0xffffffffu : 0u;
        s16x2 p0 = __builtin_bit_cast(s16x2, __builtin_convertvector(f32x2{acc[0], acc[1]}, bf16x2));
        s16x2 p1 = __builtin_bit_cast(s16x2, __builtin_convertvector(f32x2{acc[2], acc[3]}, bf16x2));
        p0 = __builtin_elementwise_max(p0, s16x2{0, 0});  // ReLU on the rounded pair (a bf16 is negative iff it is negative as an int16)
        p1 = __builtin_elementwise_max(p1, s16x2{0, 0});
        const unsigned c0m = ct ? cm10 : cm00, c1m = ct ? cm11 : cm01;
        const u32x2 o = {__builtin_bit_cast(unsigned, p0) & (c0m & rmask), __builtin_bit_cast(unsigned, p1) & (c1m & rmask)};
        const int slot = ((2 * p) & (TZ_NF - 1)) + fs;
        *reinterpret_cast<u32x2*>(ring + slot * TZ_FS + m * TZ_CHS + ct * TZ_TS + rr * 32 + q * 8) = o;
    };
    auto load_pair = [&](int p) {
#pragma unroll
        for (int i = 0; i < TZ_EW; ++i) load_tile(p, i);
    };
    auto expand_pair = [&](int p) {
#pragma unroll
        for (int i = 0; i < TZ_EW; ++i) expand_tile(p, i);
    };
    // the x rows of pairs 0 AND 1 are requested before the stencil operands are built (the second set of registers is free until they are)
    u32x4 xq1[TZ_EW];
#pragma unroll
    for (int i = 0; i < TZ_EW; ++i) xq1[i] = u32x4{0u, 0u, 0u, 0u};
    load_pair(0);
    {
#pragma unroll
        for (int i = 0; i < TZ_EW; ++i) {
            const int e = wave * TZ_EW + i;
            const int fs = e / (TZ_RH * TZ_CT), rem = e - fs * (TZ_RH * TZ_CT);
            const int rr = rem >> 1, ct = rem & 1;
            const int f = t0 + 1 + fs, hi = h0 - 1 + rr;
            if (f >= 0 && f < Ti && (unsigned)hi < (unsigned)Hi)
                xq1[i] = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, (int)(ct ? xoff1 : xoff0), (int)((unsigned)f * fx_bytes + (unsigned)hi * rx_bytes), 0);
        }
    }

    // ---- stencil roles: this wave's two channels; Toeplitz operands in registers for the launch (toeplitz.h) ----
    const int cA = cgi * 16 + 2 * wave;
    const bool wave_live = cA < Cp;
    u32x4 AT[2][5];
    float bsv[2], scv[2];
    int bpk[5];
    tz_build_operands<!POOL>(w, scale, bias, cA, d.Cout, Cp, m, q, AT, bsv, scv);
    tz_operand_offsets(wave, m, q, bpk);
    // Pool weights (toeplitz.h): on a region that lies inside the plane they are ones except for output columns 14, 15 of a tile (lanes q = 3,
    // second pair): ONE register; a region cut by the plane's border reads its column / row weights from a table.
    const bool ragged = w0 + TZ_CT * TZ_BW > d.Wo || h0 + TZ_RT > d.Ho;  // wave-uniform
    unsigned* const ptab = reinterpret_cast<unsigned*>(outi + 16 * TZ_OCS);  // [column tile][pair][64 lanes]: the weights of a cut region
    if (POOL && wave == 0) {
#pragma unroll
        for (int ct = 0; ct < TZ_CT; ++ct)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                unsigned v = 0;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int col = 4 * q + 2 * h + i;
                    if (col < TZ_BW && w0 + ct * TZ_BW + col < d.Wo && h0 + (m & 7) < d.Ho) v |= 0x3f80u << (16 * i);
                }
                ptab[(ct * 2 + h) * 64 + lane] = v;
            }
    }
    const unsigned mk23 = q < 3 ? 0x3f803f80u : 0u;
    float psum[2] = {0.0f, 0.0f};

    // ---- output roles (toeplitz.h): the region's origin is (h0, w0), its tiles lie side by side, 14 columns each ----
    const long oframe = (long)d.Ho * d.Wo * Cp;
    const __amdgpu_buffer_rsrc_t yrsrc = buffer_rsrc(y + (long)n * d.To * oframe, (unsigned)(d.To * oframe * 2));
    int tr_off;
    unsigned ooff;
    tz_output_roles(tid, cgi, d, h0, w0, 0, TZ_BW, true, tr_off, ooff);

    // ---- prologue: pairs 0 and 1 expanded, the x rows of pair 2 requested ----
    TZ_STAMP(1);
    expand_pair(0);
#pragma unroll
    for (int i = 0; i < TZ_EW; ++i) xq[i] = xq1[i];
    expand_pair(1);
    if (steps >= 2) load_pair(2);
    lds_barrier();
    TZ_STAMP(2);

#pragma unroll 1
    for (int k = 0; k < steps; ++k) {
        const int t = t0 + 2 * k;
        // ---- phase 1: the stencil of output frames t, t + 1 from pairs k, k + 1 -> output image ----
        if (wave_live) tz_stencil_step<ACT, POOL, true>(ring, outi, AT, bsv, scv, bpk, k, t + 1 >= t1, wave, lane, ptab, ragged, mk23, psum);
        TZ_STAMP(3 + 6 * k);
        lds_barrier();  // the output image is complete; nobody reads pair k's frame images any more
        TZ_STAMP(4 + 6 * k);
        // ---- phase 2: store (two transposing reads deliver channels 8 og .. + 3 and + 4 .. + 7 of this lane's column: one 16-byte
        // channels-last store; EXEC is all ones here, as the instruction needs), expand pair k + 2 over pair k, request pair k + 3 ----
        u32x2 ua[2], ub[2];
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            ua[ps] = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((tz_lds_s16x4_t)(outi + tr_off + ps * 8 * TZ_ORS)));
            ub[ps] = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((tz_lds_s16x4_t)(outi + tr_off + ps * 8 * TZ_ORS + 4 * TZ_OCS)));
        }
        tz_store_frames(ua, ub, yrsrc, ooff, t, t1, (unsigned)(oframe * 2));
        TZ_STAMP(5 + 6 * k);
        // (each tile's x row for the NEXT pair is requested as soon as the tile's registers are free)
        if (k + 2 <= steps) {
#pragma unroll
            for (int i = 0; i < TZ_EW; ++i) {
                expand_tile(k + 2, i);
                if (k + 3 <= steps) load_tile(k + 3, i);
            }
        }
        TZ_STAMP(6 + 6 * k);
        TZ_STAMP(7 + 6 * k);
        lds_barrier();  // pair k + 2's frame images are complete; everyone is done with the output image
        TZ_STAMP(8 + 6 * k);
    }

    if (POOL && pool && wave_live) tz_pool_reduce(psum, pool + ((long)n * g.tzChunks + u) * Cp + cA, lane);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// Fills the tz* fields of g (g.tz = 1) when the Toeplitz kernel covers the pair; called by xe_geom after its own checks passed.
void xe_geom_tz(XeGeom& g, const pasn_conv_desc& de, const pasn_conv_desc& d) {
    g.tz = 0;
    const char* mode = tune("PASN_EXPDW_TZ");
    if (mode && mode[0] == '0') return;
    const char* fold = tune("PASN_EXPDW_FOLD");
    if (fold && fold[0] == '0') return;                       // the kernel takes norm_a folded into the expand weights (scale_a == NULL)
    if (d.sh != 1 || d.sw != 1) return;                       // stride 1 only
    if (d.act != PASN_ACT_NONE && d.act != PASN_ACT_SWISH) return;
    const int nks = de.w_kc / 16;
    if (nks > 2) return;                                      // block width <= 32 channels in this round's instances (KS32 = 1)
    g.tzXS = 0;
    g.tzCG = ceil_div(d.Cout_p, 16);
    g.tzRTH = ceil_div(d.Ho, TZ_RT);
    g.tzRTW = ceil_div(d.Wo, TZ_CT * TZ_BW);
    const int force_tc = tune("PASN_EXPDW_TC") ? atoi(tune("PASN_EXPDW_TC")) : 0;
    g.tzTc = force_tc > 0 ? std::min(force_tc, (int)d.To) : d.To;
    g.tznT = ceil_div(d.To, g.tzTc);
    g.tzChunks = g.tznT * g.tzRTH * g.tzRTW;
    if (g.tzChunks > 64 && !force_tc) return;                 // SE partial rows per clip the consumers sum (see x3d_expdw.hip)
    g.tzLds = TZ_NF * TZ_FS + 16 * TZ_OCS + 1024;           // + the pool-weight table of a region cut by the plane's border
    g.abl = tune_dev("PASN_TZ_STAMPS") ? std::max(1, atoi(tune_dev("PASN_TZ_STAMPS"))) : 0;  // 1 + the block that leaves stamps
    g.tz = 1;
}

int launch_x3d_expdw_tz(const void* x, const void* wa, const float* ba, const float* w, const float* scale, const float* bias, void* y, float* pool,
                        const pasn_conv_desc& de, const pasn_conv_desc& d, const XeGeom& g, hipStream_t s) {
    const dim3 grid((unsigned)((long)d.N * g.tzCG * g.tznT * g.tzRTH * g.tzRTW)), block(512);
#define PASN_TZ(ACT_, POOL_)                                                                                                       \
    do {                                                                                                                         \
        PASN_MAX_LDS(80 * 1024, x3d_expdw_tz_kernel<1, ACT_, POOL_>);                                                            \
        hipLaunchKernelGGL((x3d_expdw_tz_kernel<1, ACT_, POOL_>), grid, block, (size_t)g.tzLds, s, (const __bf16*)x,            \
                           (const __bf16*)wa, ba, w, scale, bias, (__bf16*)y, pool, d, de.Cin_p, de.w_kc / 16, g);               \
    } while (0)
    if (d.act == PASN_ACT_SWISH) {
        if (pool) PASN_TZ(PASN_ACT_SWISH, true);
        else PASN_TZ(PASN_ACT_SWISH, false);
    } else {
        if (pool) PASN_TZ(PASN_ACT_NONE, true);
        else PASN_TZ(PASN_ACT_NONE, false);
    }
#undef PASN_TZ
    return check_launch("x3d_expdw_tz_kernel");
}

}  // namespace pasn

#ifdef PASN_TUNING
extern "C" int pasn_debug_tz_stamps(long long* host_out) { return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(pasn::tz_stamps), sizeof(long long) * 62); }
#endif
