// Depthwise 3x3x3 conv, stride 1, pad 1, + BN (+ Swish, + squeeze-excite pool partial rows) on planes at most 14 x 14 as PER-CHANNEL TOEPLITZ
// matrix products on a channel-planar LDS image (round 5): x3d_expdw_tz.hip's stencil for layers whose input arrives CHANNELS-LAST from HBM --
// the stride-1 blocks of the 14 x 14 stage, where the expand conv is a launch of its own (pytorchvideo's BottleneckTransform conv_b as the x3d
// trunks instantiate it).
//
// dwmfma.hip runs the same layers with block-diagonal operands at two waves per SIMD (15 MFMAs + 5 operand reads per 16-channel tile and frame,
// three T-marching accumulator sets, 226-253 registers).  The Toeplitz form needs 8 consecutive COLUMNS of one channel per lane; round 4 priced the
// transposition of a channels-last tensor at two passes per element and left it.  gfx950's ds_read_b64_tr_b16 does it in one: the rows of the
// plane arrive by LDS-DMA as they lie ([position][16 channels], 32 bytes per position), and a 16-lane group's transposing read of 4 positions x
// 16 channels hands lane i the 4 consecutive columns of channel i -- one ds_write_b64 into the planar frame image.  One read + one write per
// 4 positions x 16 channels, no vector arithmetic; zeros outside the image come from the DMA's range check.
//
// Block = 8 waves = 16 channels x one clip (a T chunk of it), the whole plane: the block's two 16 x 14-output tiles are ROW BANDS (tile ct =
// output rows 8 ct .. 8 ct + 7, every column).  It marches along T two output frames per step over a ring of 4 frame images, two barriers per
// step: [stencil of pairs k, k + 1 -> output image] | [store, transpose pair k + 2 over pair k, request the rows of pair k + 3].
// Stencil, operands, output path: toeplitz.h (5 MFMAs per 224 outputs of a channel, ONE accumulator of 4 registers, four waves per SIMD); tile ct of
// that header is the band ct here.  norm's scale is folded into the operands where no pool sums are taken (a weight rounded after scaling:
// results agree with dwmfma.hip to one bf16 ulp of the output, not bit for bit).
// Wider planes in regions of 8 x 28 outputs (two column tiles) were built and measured: 28 x 28 x 108 53 / 50 us against dwmfma.hip's 52 / 47,
// 56 x 56 x 54 117 / 114 against 103 / 86 -- a block's start-up (two memory round trips before its first MFMA) is a third of its time and
// 896 blocks on 512 slots run two rounds; that form is gone (profiles/README.md, round 5).
#include "toeplitz.h"

namespace pasn {

constexpr int TZ_PR = 16;                      // staged rows of the plane: -1 .. 14
constexpr int TZ_RAWROW = 16 * 32;             // bytes per raw row: 16 positions (columns -1 .. 14) x 16 channels; one LDS-DMA instruction = two rows
constexpr int TZ_RAW = 2 * TZ_PR * TZ_RAWROW;  // raw rows of one pair of frames
constexpr int TZ_NR = 2;                       // LDS-DMA instructions per wave and pair: rows 2 wave, 2 wave + 1 of either frame
static_assert(TZ_NF * TZ_FS + 16 * TZ_OCS + TZ_RAW + 1024 <= 80 * 1024, "two blocks per CU");

#ifdef PASN_TUNING
// shader-clock stamps of one block's wave 0 (tuning builds, PASN_TZ_STAMPS = 1 + block; tools/dwtz_bench.py prints them): [0] start, [1] operands
// built, [2] prologue done, then five per step: stencil done, rows landed, barrier passed + stores issued, pair transposed + next requested,
// barrier passed
__device__ long long dt_stamps[62];
#define TZ_STAMP(i) do { if (g.abl && (int)blockIdx.x == g.abl - 1 && threadIdx.x == 0 && (i) < 62) dt_stamps[i] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
#else
#define TZ_STAMP(i) do { } while (0)
#endif

// ACT: the epilogue (PASN_ACT_NONE / PASN_ACT_SWISH); POOL: squeeze-excite partial sums
template <int ACT, bool POOL>
__global__ __launch_bounds__(512, 4) void dwconv3d_tz_kernel(const __bf16* __restrict__ x, const float* __restrict__ w, const float* __restrict__ scale,
                                                             const float* __restrict__ bias, __bf16* __restrict__ y, float* __restrict__ pool,
                                                             pasn_conv_desc d, DtGeom g) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    char* const ring = smem;                                  // [TZ_NF][TZ_FS]
    char* const outi = smem + TZ_NF * TZ_FS;                  // [16 channels][TZ_OCS]
    char* const raw = outi + 16 * TZ_OCS;                     // the rows of ONE pair of frames as they lie in memory: [2 frames][TZ_PR][TZ_RAWROW]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lane & 15, q = lane >> 4;
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int cgi = lb % g.CG, r1 = lb / g.CG;
    const int u = r1 % g.nT, n = r1 / g.nT;                   // T chunk, clip
    const int t0 = u * g.Tc, t1 = min(t0 + g.Tc, d.To);
    const int Cp = d.Cout_p, Ti = d.Ti, Hi = d.Hi, Wi = d.Wi;
    TZ_STAMP(0);
    const int steps = (t1 - t0 + 1) >> 1;                     // output frames t0 + 2 k, t0 + 2 k + 1; input pairs 0 .. steps: frames (t0 - 1 + 2 p, t0 + 2 p)

    // ---- staging roles: two LDS-DMA instructions per wave and pair of frames, 1 KB each: instruction i = rows 2 wave, 2 wave + 1 of the plane's
    // 16 staged rows (-1 .. 14) of frame i, lane -> (row lane >> 5, staged column (lane & 31) >> 1, channel half lane & 1), 16 bytes each;
    // positions outside the image and channels beyond the tensor carry an out-of-range offset: the hardware writes zeros.  The wave that
    // requested a row transposes it.
    const long fx = (long)Hi * Wi * Cp;
    const unsigned fx_bytes = (unsigned)(fx * 2);
    const __amdgpu_buffer_rsrc_t xrsrc = buffer_rsrc(x + (long)n * Ti * fx, (unsigned)Ti * fx_bytes);
    unsigned xoff;
    {
        const int ch = cgi * 16 + (lane & 1) * 8;
        const int hi = 2 * wave + (lane >> 5) - 1, wi = ((lane & 31) >> 1) - 1;
        xoff = ((unsigned)hi < (unsigned)Hi && (unsigned)wi < (unsigned)Wi && ch < Cp) ? (unsigned)(((hi * Wi + wi) * Cp + ch) * 2) : BUF_OOB;
    }
    auto frame_ok = [&](int p, int fs) -> bool {  // wave-uniform: frame fs of pair p exists
        const int f = t0 - 1 + 2 * p + fs;
        return f >= 0 && f < Ti;
    };
    auto dma_rows = [&](int p, char* base) {
#pragma unroll
        for (int fs = 0; fs < TZ_NR; ++fs)
            if (frame_ok(p, fs))
                __builtin_amdgcn_raw_ptr_buffer_load_lds(xrsrc, (lds_ptr_t)(base + (fs * TZ_PR + 2 * wave) * TZ_RAWROW), 16, (int)xoff,
                                                         (int)((unsigned)(t0 - 1 + 2 * p + fs) * fx_bytes), 0, 0);
    };
    // transposing read of a raw row's 16 positions x 16 channels: lane 4 q' + p of a 16-lane group supplies the address of position 4 group + q',
    // channels 4 p ..; lane i receives channel i's values at the group's 4 positions = 4 consecutive columns of channel i -> one ds_write_b64
    // into the planar frame image.
    const int tr_in = (4 * q + (m >> 2)) * 32 + (m & 3) * 8;
    const unsigned raw_addr = tz_lds_addr(raw), outi_addr = tz_lds_addr(outi), tmp_addr = tz_lds_addr(ring + 2 * TZ_FS);
    // One pair of frames: the four transposing reads of this wave's rows (one statement, one wait: read by read, each with its own wait, the
    // pass was a chain of LDS round trips), the requests that refill the rows with pair pd (pd < 0: none) -- they are in registers -- and the
    // rows into the frame images: band 0 holds staged rows 0 .. 9 of the 16, band 1 rows 8 .. 17 as its rows 0 .. 9.  Frames outside the
    // clip: zeros whatever the raw rows hold.  (EXEC is all ones at every transposing read: the branches around them are wave-uniform.)
    auto stage_pair = [&](int p, unsigned base_addr, int pd) {
        u32x2 uv[TZ_NR][2];
        tz_read_tr4<0, TZ_RAWROW, TZ_PR * TZ_RAWROW, (TZ_PR + 1) * TZ_RAWROW>(base_addr + 2 * wave * TZ_RAWROW + tr_in, uv[0][0], uv[0][1], uv[1][0], uv[1][1]);
        if (pd >= 0) dma_rows(pd, raw);
#pragma unroll
        for (int fs = 0; fs < TZ_NR; ++fs) {
            const unsigned rmask = frame_ok(p, fs) ? 0xffffffffu : 0u;
            char* img = ring + (((2 * p) & (TZ_NF - 1)) + fs) * TZ_FS + m * TZ_CHS + q * 8;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int r = 2 * wave + j;  // staged row of the plane
                const u32x2 v = u32x2{uv[fs][j].x & rmask, uv[fs][j].y & rmask};
                if (r < TZ_RH) *reinterpret_cast<u32x2*>(img + r * 32) = v;
                if (r >= TZ_RT) *reinterpret_cast<u32x2*>(img + TZ_TS + (r - TZ_RT) * 32) = v;
            }
        }
    };
    // Both pairs of the prologue are requested at once: pair 1 into the raw rows, pair 0 into the (still empty) frame images 2, 3 of the ring
    dma_rows(0, ring + 2 * TZ_FS);
    dma_rows(1, raw);

    // ---- stencil roles: this wave's two channels; Toeplitz operands in registers for the launch (toeplitz.h) ----
    const int cA = cgi * 16 + 2 * wave;
    const bool wave_live = cA < Cp;
    u32x4 AT[2][5];
    float bsv[2], scv[2];
    int bpk[5];
    tz_build_operands<!POOL>(w, scale, bias, cA, d.Cout, Cp, m, q, AT, bsv, scv);
    tz_operand_offsets(wave, m, q, bpk);
    // The 1 / 0 pool weights of a lane's four outputs (columns 14, 15 of a band, rows below the plane) come from a 1 KB table.
    unsigned* const ptab = reinterpret_cast<unsigned*>(raw + TZ_RAW);  // [band][pair][64 lanes]
    if (POOL && wave == 0) {
#pragma unroll
        for (int ct = 0; ct < TZ_CT; ++ct)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                unsigned v = 0;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int col = 4 * q + 2 * h + i;
                    if (col < d.Wo && ct * TZ_RT + (m & 7) < d.Ho) v |= 0x3f80u << (16 * i);
                }
                ptab[(ct * 2 + h) * 64 + lane] = v;
            }
    }
    float psum[2] = {0.0f, 0.0f};

    // ---- output roles (toeplitz.h): a band's origin is row 8 ct of the plane, the lanes' columns are the plane's ----
    const long oframe = (long)d.Ho * d.Wo * Cp;
    const __amdgpu_buffer_rsrc_t yrsrc = buffer_rsrc(y + (long)n * d.To * oframe, (unsigned)(d.To * oframe * 2));
    int tr_off;
    unsigned ooff;
    tz_output_roles(tid, cgi, d, 0, 0, TZ_RT, 0, false, tr_off, ooff);

    // (the operands are built while the prologue's rows are in flight: without this the compiler sinks the build into the first step)
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
        for (int j = 0; j < 5; ++j) asm volatile("" : "+v"(AT[c2][j]));
    TZ_STAMP(1);
    // ---- prologue: pair 0 transposed out of the ring's far half, then pair 1 over it; the rows of pair 2 requested ----
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    auto zero_band_tail = [&](int sl0) {  // band 1's staged rows 8, 9 lie below every plane and are never staged: zeros once (finite values
                                          // under the pool sums' zero weights)
#pragma unroll
        for (int sl = sl0; sl < sl0 + 2; ++sl)
            if (tid < 16 * 8) *reinterpret_cast<u32x2*>(ring + sl * TZ_FS + (tid >> 3) * TZ_CHS + TZ_TS + TZ_RT * 32 + (tid & 7) * 8) = u32x2{0u, 0u};
    };
    zero_band_tail(0);
    lds_barrier();  // (the rows are read a barrier behind their wait, as in the loop)
    stage_pair(0, tmp_addr, -1);
    lds_barrier();  // everyone has read its rows of pair 0: frame images 2, 3 may be written
    zero_band_tail(2);
    stage_pair(1, raw_addr, steps >= 2 ? 2 : -1);
    lds_barrier();
    TZ_STAMP(2);

#pragma unroll 1
    for (int k = 0; k < steps; ++k) {
        const int t = t0 + 2 * k;
        // ---- phase 1: the stencil of output frames t, t + 1 from pairs k, k + 1 -> output image ----
        if (wave_live) tz_stencil_step<ACT, POOL, false>(ring, outi, AT, bsv, scv, bpk, k, t + 1 >= t1, wave, lane, ptab, false, 0u, psum);
        TZ_STAMP(3 + 5 * k);
        // The rows of pair k + 2 were requested one step ago.  The wait stands BEFORE the barrier and the rows are read behind it
        // (cdna_hip_programming.md: read a staged buffer one phase after the wait that retires it).
        if (k + 2 <= steps) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        TZ_STAMP(4 + 5 * k);
        lds_barrier();  // the output image is complete; nobody reads pair k's frame images any more
        // ---- phase 2: the store -- two transposing reads deliver channels 8 og .. + 3 and + 4 .. + 7 of this lane's column, one 16-byte
        // channels-last store per output frame -- then pair k + 2 transposed over pair k and the rows of pair k + 3 requested.  (Measured
        // both ways, 14 x 14 x 216, Swish / pool: stores first 29.5 / 26.9 us; requests first, then stores, then the writes of the frame
        // images 31.2 / 28.3 with vmcnt(0), 31.9 / 28.9 with a counted vmcnt(2).) ----
        u32x2 ua[2], ub[2];
        tz_read_tr4<0, 4 * TZ_OCS, 8 * TZ_ORS, 8 * TZ_ORS + 4 * TZ_OCS>(outi_addr + tr_off, ua[0], ub[0], ua[1], ub[1]);
        tz_store_frames(ua, ub, yrsrc, ooff, t, t1, (unsigned)(oframe * 2));
        TZ_STAMP(5 + 5 * k);
        if (k + 2 <= steps) stage_pair(k + 2, raw_addr, k + 3 <= steps ? k + 3 : -1);
        TZ_STAMP(6 + 5 * k);
        lds_barrier();  // pair k + 2's frame images are complete; everyone is done with the output image
        TZ_STAMP(7 + 5 * k);
    }

    if (POOL && pool && wave_live) tz_pool_reduce(psum, pool + ((long)n * g.nT + u) * Cp + cA, lane);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
DtGeom dw_tz_geom(const pasn_conv_desc& d, int dtype) {
    DtGeom g{};
    if (dtype != PASN_BF16) return g;
    // The stride-1 stencils of planes 9 .. 14 wide and at most 14 high (the 14 x 14 stage: one block = 16 channels of a whole clip; narrower
    // planes leave the 14-column tiles half empty and stay with dwmfma.hip).  PASN_DW_TZ=0: off.
    if (tune("PASN_DW_TZ") && tune("PASN_DW_TZ")[0] == '0') return g;
    if (tune("PASN_DWMFMA") && tune("PASN_DWMFMA")[0] == '0') return g;  // "no matrix-core stencil": the VALU stencil's tests and A/B runs
    const bool shape = d.kt == 3 && d.kh == 3 && d.kw == 3 && d.st == 1 && d.sh == 1 && d.sw == 1 && d.pt == 1 && d.ph == 1 && d.pw == 1 &&
                       d.To == d.Ti && d.Ho == d.Hi && d.Wo == d.Wi && d.Cin_p == d.Cout_p && d.Cin == d.Cout && d.Cout_p % 8 == 0;
    if (!shape || (d.act != PASN_ACT_NONE && d.act != PASN_ACT_SWISH)) return g;
    if (d.Wo > TZ_BW || d.Wo < 9 || d.Ho > TZ_BW) return g;   // (16 staged rows: plane rows -1 .. 14)
    if ((long)d.Ti * d.Hi * d.Wi * d.Cin_p * 2 >= (1L << 31)) return g;  // one clip per buffer descriptor
    g.CG = ceil_div(d.Cout_p, 16);
    const int force_tc = tune("PASN_DWMFMA_TC") ? atoi(tune("PASN_DWMFMA_TC")) : 0;
    g.Tc = force_tc > 0 ? std::min(force_tc, (int)d.To) : d.To;
    g.nT = ceil_div(d.To, g.Tc);                              // = SE partial rows per clip
    if (g.nT > 64 && !force_tc) return DtGeom{};
    // One round of blocks (two per CU, 256 CUs) or none: a block's first MFMA stands behind two memory round trips, and a second round pays
    // them again -- 64 clips of the 14 x 14 stage (the paired training pass: 896 blocks) take 58-64 us here against dwmfma.hip's 54-58, 32
    // clips (448 blocks) 29.6 / 26.2 against 33.5 / 29.6 (profiles/README.md entries 143, 149).  PASN_DW_TZ=1: whatever the block count.
    if ((long)d.N * g.CG * g.nT > 512 && !(tune("PASN_DW_TZ") && tune("PASN_DW_TZ")[0] == '1')) return DtGeom{};
    g.lds = TZ_NF * TZ_FS + 16 * TZ_OCS + TZ_RAW + 1024;      // + the pool-weight table
    g.abl = tune_dev("PASN_TZ_STAMPS") ? std::max(1, atoi(tune_dev("PASN_TZ_STAMPS"))) : 0;  // 1 + the block that leaves stamps
    g.ok = 1;
    return g;
}

int launch_dw_tz(const void* x, const float* w, const float* scale, const float* bias, void* y, float* pool, const pasn_conv_desc& d, const DtGeom& g,
                 hipStream_t s) {
    const dim3 grid((unsigned)((long)d.N * g.CG * g.nT)), block(512);
#define PASN_DT(ACT_, POOL_)                                                                                                          \
    do {                                                                                                                            \
        PASN_MAX_LDS(80 * 1024, dwconv3d_tz_kernel<ACT_, POOL_>);                                                                   \
        hipLaunchKernelGGL((dwconv3d_tz_kernel<ACT_, POOL_>), grid, block, (size_t)g.lds, s, (const __bf16*)x, w, scale, bias, (__bf16*)y, pool, d, g); \
    } while (0)
    if (d.act == PASN_ACT_SWISH) {
        if (pool) PASN_DT(PASN_ACT_SWISH, true);
        else PASN_DT(PASN_ACT_SWISH, false);
    } else {
        if (pool) PASN_DT(PASN_ACT_NONE, true);
        else PASN_DT(PASN_ACT_NONE, false);
    }
#undef PASN_DT
    return check_launch("dwconv3d_tz_kernel");
}

}  // namespace pasn

#ifdef PASN_TUNING
extern "C" int pasn_debug_dt_stamps(long long* host_out) { return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(pasn::dt_stamps), sizeof(long long) * 62); }
#endif
