// wgrad.hip -- weight gradients of the dense and first convs (depthwise: dw_wgrad.hip; partial-buffer kernels: wgrad_halo.hip; shared: wgrad_tile.h).
//
// Dense weight gradient dW[co][ci][tap] = sum_rows dy[row][co] * x[in(row, tap)][ci] is a GEMM whose contraction runs
// over the ROWS of two channels-last tensors.  v_mfma_f32_32x32x2_f32 wants, per lane, ONE A element (row m = lane & 31,
// k = lane >> 5) and ONE B element (column n = lane & 31, same k): with k = activation row and m / n = channel, a lane's
// operand is a single element of a channels-last row and a wave's load is two coalesced 128-byte row segments -- no
// transposition through LDS.  bf16 activations are widened on load; accumulation and the gradient are fp32.
// Row chunks are spread over the grid (split-K) and combined with fp32 atomics into the zero-initialised gradient.
//
// The input gradients of the dense convs need no kernel of their own: a 1x1x1 conv's dgrad is pasn_conv3d_fwd with the
// transposed weight (strided ones followed by pasn_scatter_strided).
#include "wgrad_tile.h"

namespace pasn {

constexpr int WG_U = 8;  // row pairs in flight per wave

// x: [N][Ti][Hi][Wi][Cin_p], dy: [N][To][Ho][Wo][Cout_p], dw: fp32 [Cout][Cin][taps]
template <typename T, bool PW>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ dw,
                                                         pasn_conv_desc d, int ci_tiles, int rows_per_wave) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 31, k = lane >> 5;
    const int taps = d.kt * d.kh * d.kw;
    int tile = blockIdx.y;
    const int tap = tile % taps;
    tile /= taps;
    const int ci_t = tile % ci_tiles, co_t = tile / ci_tiles;
    const int co = co_t * 32 + m, ci = ci_t * 32 + m;
    const bool a_ok = co < d.Cout_p, b_ok = ci < d.Cin_p;
    const int coc = a_ok ? co : 0, cic = b_ok ? ci : 0;
    const long R = (long)d.N * d.To * d.Ho * d.Wo;
    const long r0 = ((long)blockIdx.x * 4 + wave) * rows_per_wave;
    const long r1 = min(R, r0 + rows_per_wave);
    const int tt = tap / (d.kh * d.kw), th = (tap / d.kw) % d.kh, tw = tap % d.kw;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    for (long rb = r0; rb < r1; rb += 2 * WG_U) {
        T ra[WG_U], rx[WG_U];
        float ma[WG_U], mx[WG_U];
#pragma unroll
        for (int u = 0; u < WG_U; ++u) {
            const long r = rb + 2 * u + k;
            const bool rok = r < r1;
            const long rc = rok ? r : r0;
            long in_row = rc;
            bool vok = rok;
            if (!PW) vok = wg_window_row(d, rc, tt, th, tw, in_row) && rok;
            ra[u] = dy[rc * d.Cout_p + coc];
            rx[u] = x[in_row * d.Cin_p + cic];
            ma[u] = (rok && a_ok) ? 1.0f : 0.0f;
            mx[u] = (vok && b_ok) ? 1.0f : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < WG_U; ++u)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32((float)ra[u] * ma[u], (float)rx[u] * mx[u], acc, 0, 0, 0);
    }
    wg_tile_atomic(dw, acc, co_t * 32, ci_t * 32 + m, k, d.Cout, d.Cin, taps, tap);
}

// First conv (planar input x [N][3][T][Hi][Wi], window (1,kh,kw)): dw fp32 [Cout][3*kh*kw]
template <typename TIN, typename T>
__global__ __launch_bounds__(256) void first_conv_wgrad_kernel(const TIN* __restrict__ x, const T* __restrict__ dy, float* __restrict__ dw,
                                                               pasn_conv_desc d, int col_tiles, int rows_per_wave) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 31, k = lane >> 5;
    const int cols = d.Cin * d.kh * d.kw;
    const int col_t = blockIdx.y % col_tiles, co_t = blockIdx.y / col_tiles;
    const int co = co_t * 32 + m, col = col_t * 32 + m;
    const bool a_ok = co < d.Cout_p, b_ok = col < cols;
    const int coc = a_ok ? co : 0;
    const int ci = b_ok ? col / (d.kh * d.kw) : 0, th = b_ok ? (col / d.kw) % d.kh : 0, tw = b_ok ? col % d.kw : 0;
    const long R = (long)d.N * d.To * d.Ho * d.Wo;
    const long r0 = ((long)blockIdx.x * 4 + wave) * rows_per_wave;
    const long r1 = min(R, r0 + rows_per_wave);
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    for (long rb = r0; rb < r1; rb += 2 * WG_U) {
        T ra[WG_U];
        TIN rx[WG_U];
        float ma[WG_U], mx[WG_U];
#pragma unroll
        for (int u = 0; u < WG_U; ++u) {
            const long r = rb + 2 * u + k;
            const bool rok = r < r1;
            const long rc = rok ? r : r0;
            const int wo = (int)(rc % d.Wo);
            long q = rc / d.Wo;
            const int ho = (int)(q % d.Ho);
            q /= d.Ho;
            const int to = (int)(q % d.To), n = (int)(q / d.To);
            const int hi = ho * d.sh - d.ph + th, wi = wo * d.sw - d.pw + tw;
            const bool in = hi >= 0 && hi < d.Hi && wi >= 0 && wi < d.Wi;
            const long off = in ? ((((long)n * d.Cin + ci) * d.Ti + to) * d.Hi + hi) * d.Wi + wi : 0;
            ra[u] = dy[rc * d.Cout_p + coc];
            rx[u] = x[off];
            ma[u] = (rok && a_ok) ? 1.0f : 0.0f;
            mx[u] = (rok && in && b_ok) ? 1.0f : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < WG_U; ++u)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32((float)ra[u] * ma[u], (float)rx[u] * mx[u], acc, 0, 0, 0);
    }
    if (col < cols) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int cog = co_t * 32 + acc_row(reg, k);
            if (cog < d.Cout) unsafeAtomicAdd(dw + (size_t)cog * cols + col, acc[reg]);
        }
    }
}

bool pw_wgrad_bf16(const void* x, const void* dy, float* dw, const pasn_conv_desc& d, hipStream_t s);

static int wgrad_rows_per_wave(long R, int tiles) {
    long waves_per_tile = std::max<long>(1, std::min<long>(std::min(8192, 2048 + 65536 / std::max(1, tiles)) / std::max(1, tiles), R / 128));
    waves_per_tile = (waves_per_tile + 3) / 4 * 4;
    long rpw = (R + waves_per_tile - 1) / waves_per_tile;
    rpw = (rpw + 2 * WG_U - 1) / (2 * WG_U) * (2 * WG_U);
    return (int)rpw;
}

}  // namespace pasn

using namespace pasn;

// im2col of the planar clip for the first conv's weight gradient: X[row][col] (bf16, 32-column groups), col = (ci, r, s); then the
// gradient is the pointwise GEMM dW[co][col] = sum_rows dy[row][co] X[row][col] on the LDS-transposed bf16 MFMA kernel.  The
// gather costs one pass over the clip's windows instead of one scattered 2-byte load per MFMA operand element.
template <typename TIN>
__global__ __launch_bounds__(256) void first_conv_im2col_kernel(const TIN* __restrict__ x, __bf16* __restrict__ X, pasn_conv_desc d, int colp) {
    const int groups = colp / 8, cols = d.Cin * d.kh * d.kw;
    const long R = (long)d.N * d.To * d.Ho * d.Wo, total = R * groups;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int g = (int)(idx % groups);
        const long row = idx / groups;
        const int wo = (int)(row % d.Wo);
        long q = row / d.Wo;
        const int ho = (int)(q % d.Ho);
        q /= d.Ho;
        const int to = (int)(q % d.To), n = (int)(q / d.To);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int col = g * 8 + j;
            const int ci = col / (d.kh * d.kw), r = (col / d.kw) % d.kh, sx = col % d.kw;
            const int hi = ho * d.sh - d.ph + r, wi = wo * d.sw - d.pw + sx;
            const bool ok = col < cols && hi >= 0 && hi < d.Hi && wi >= 0 && wi < d.Wi;
            v[j] = ok ? (float)x[((((long)n * d.Cin + ci) * d.Ti + to) * d.Hi + hi) * d.Wi + wi] : 0.0f;
        }
        store8(X + row * colp + g * 8, v);
    }
}

// grey clip (Cin = 1): the three input-channel slices of conv.weight see the same sum dy * x, computed once into [Cout][kh*kw] scratch and
// written to all three slices here -- bitwise identical whatever order the atomics of the gradient kernel took
__global__ __launch_bounds__(256) void first_conv_grey_expand_kernel(const float* __restrict__ g, float* __restrict__ dw, int Cout, int K) {
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < Cout * K; idx += gridDim.x * 256) {
        const int co = idx / K, k = idx % K;
        const float v = g[idx];
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) dw[((long)co * 3 + ci) * K + k] += v;
    }
}

static size_t first_im2col_bytes(const pasn_conv_desc* d, int dtype) {
    if (dtype != PASN_BF16 || tune("PASN_NO_FIRST_IM2COL")) return 0;
    const int colp = (d->Cin * d->kh * d->kw + 7) / 8 * 8;
    if (colp > 512) return 0;
    return (size_t)d->N * d->To * d->Ho * d->Wo * colp * sizeof(__bf16);
}

// the grey clip's [Cout][kh*kw] gradient scratch, first in the workspace (256-byte aligned, so the im2col after it stays aligned)
static size_t first_grey_bytes(const pasn_conv_desc* d) {
    return d->Cin == 1 ? ((size_t)d->Cout * d->kh * d->kw * sizeof(float) + 255) / 256 * 256 : 0;
}

extern "C" size_t pasn_first_conv_wgrad_workspace_bytes(const pasn_conv_desc* d, int dtype) {
    if (!d) return 0;
    const size_t im2col = first_im2col_bytes(d, dtype);
    return im2col ? first_grey_bytes(d) + im2col : first_grey_bytes(d);
}

extern "C" int pasn_first_conv_wgrad(const void* x, const void* dy, float* dw, const pasn_conv_desc* d, int in_dtype, int dtype,
                                     void* ws, void* stream) {
    PASN_REQUIRE(x && dy && dw && d, "null pointer");
    PASN_REQUIRE(d->kt == 1 && d->st == 1 && d->pt == 0 && (d->Cin == 3 || d->Cin == 1),
                 "first conv is (1,kh,kw) over 3 planar channels (or the single channel of a grey clip)");
    PASN_REQUIRE(d->Cin == 3 || ws, "a grey clip (Cin = 1) needs pasn_first_conv_wgrad_workspace_bytes of workspace");
    const int cols = d->Cin * d->kh * d->kw;
    hipStream_t s = (hipStream_t)stream;
    // where the [Cout][cols] gradient goes: dw itself, or (grey) the scratch that is then written to the three channel slices of dw
    float* g = dw;
    const size_t gb = first_grey_bytes(d);
    if (gb) {
        g = static_cast<float*>(ws);
        if (hipMemsetAsync(g, 0, (size_t)d->Cout * cols * sizeof(float), s) != hipSuccess) return check_launch("first_conv_wgrad scratch");
    }
    auto finish = [&]() -> int {
        if (gb) {
            const int nb = std::max(1, std::min(1024, ceil_div((long)d->Cout * cols, 256)));
            hipLaunchKernelGGL(first_conv_grey_expand_kernel, dim3(nb), dim3(256), 0, s, g, dw, d->Cout, cols);
        }
        return check_launch("first_conv_wgrad");
    };
    if (ws && first_im2col_bytes(d, dtype)) {
        __bf16* X = reinterpret_cast<__bf16*>(static_cast<unsigned char*>(ws) + gb);
        const int colp = (cols + 7) / 8 * 8;
        const long R = (long)d->N * d->To * d->Ho * d->Wo, total = R * (colp / 8);
        const int nb = (int)std::min<long>((total + 255) / 256, 1 << 20);
        if (in_dtype == PASN_BF16)
            hipLaunchKernelGGL(first_conv_im2col_kernel<__bf16>, dim3(nb), dim3(256), 0, s, (const __bf16*)x, X, *d, colp);
        else
            hipLaunchKernelGGL(first_conv_im2col_kernel<float>, dim3(nb), dim3(256), 0, s, (const float*)x, X, *d, colp);
        pasn_conv_desc pw = *d;  // the equivalent pointwise problem over the im2col rows
        pw.Ti = d->To; pw.Hi = d->Ho; pw.Wi = d->Wo;
        pw.Cin = cols; pw.Cin_p = colp;
        pw.kt = pw.kh = pw.kw = 1; pw.st = pw.sh = pw.sw = 1; pw.pt = pw.ph = pw.pw = 0;
        if (pw_wgrad_bf16(X, dy, g, pw, s)) return finish();
    }
    const int co_tiles = ceil_div(d->Cout, 32), col_tiles = ceil_div(cols, 32);
    const long R = (long)d->N * d->To * d->Ho * d->Wo;
    const int rpw = wgrad_rows_per_wave(R, co_tiles * col_tiles);
    const dim3 grid(ceil_div(R, (long)rpw * 4), co_tiles * col_tiles);
#define FW(TI, T) hipLaunchKernelGGL((first_conv_wgrad_kernel<TI, T>), grid, dim3(256), 0, s, (const TI*)x, (const T*)dy, g, *d, col_tiles, rpw)
    if (in_dtype == PASN_BF16 && dtype == PASN_BF16) FW(__bf16, __bf16);
    else if (in_dtype == PASN_F32 && dtype == PASN_BF16) FW(float, __bf16);
    else if (in_dtype == PASN_BF16) FW(__bf16, float);
    else FW(float, float);
#undef FW
    return finish();
}

// =====================================================================================================================
// bf16 fast paths
// =====================================================================================================================
namespace pasn {

// ---- pointwise (1x1x1, any stride) weight gradient on v_mfma_f32_32x32x16_bf16 ------------------------------------------
// The patch staging of wgrad_tile.h: LDS holds At[channel][KT rows] / Bt[channel][KT rows] (row pitch KT*2 + 16 bytes, slots rotated).
// Four waves share the staged rows; each owns up to TPW 32x32 (co, ci) tiles.  Split-K over the grid, fp32 atomics into the zeroed gradient.
template <int KT, int TPW>
__global__ __launch_bounds__(256) void pw_wgrad_bf16_kernel(const __bf16* __restrict__ x, const __bf16* __restrict__ dy, float* __restrict__ dw,
                                                            pasn_conv_desc d, int co_tiles, int ci_tiles, int rows_per_block) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int PITCH = KT * 2 + 16, SLOTS = KT / 8;  // bytes / 16-byte slots (8 rows of a channel) per channel row
    static_assert((SLOTS & (SLOTS - 1)) == 0, "the slot rotation wraps with a mask");
    const int CGo = d.Cout_p / 8, CGi = d.Cin_p / 8;
    const int Bt_off = co_tiles * 32 * PITCH;
    unsigned char* At = lds;            // [co_tiles*32][PITCH]
    unsigned char* Bt = lds + Bt_off;   // [ci_tiles*32][PITCH]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = lane & 31, h = lane >> 5;
    const long R = (long)d.N * d.To * d.Ho * d.Wo;
    const long r0 = (long)blockIdx.x * rows_per_block, r1 = min(R, r0 + rows_per_block);
    // rows of x are gathered through the conv's window map when it is not the identity (strided 1x1x1 convs, windowed convs:
    // one tap per blockIdx.z, rows that fall into the padding read as zero)
    const int taps = d.kt * d.kh * d.kw, tap = blockIdx.z;
    const int tt = tap / (d.kh * d.kw), th = (tap / d.kw) % d.kh, tw = tap % d.kw;
    const bool strided = d.st != 1 || d.sh != 1 || d.sw != 1 || taps != 1 || d.pt || d.ph || d.pw;
    const int ntiles = co_tiles * ci_tiles;
    // this wave's tiles: (blockIdx.y * 4 + wave) * TPW + j; out-of-range ones alias tile 0 and are dropped at the end
    int t_co[TPW], t_ci[TPW];
    bool t_ok[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int t = (blockIdx.y * 4 + wave) * TPW + j;
        t_ok[j] = t < ntiles;
        const int tc = t_ok[j] ? t : 0;
        t_co[j] = tc / ci_tiles;
        t_ci[j] = tc % ci_tiles;
    }
    f32x16 acc[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.0f;
    // zero the LDS rows of padded channels once (channels >= C*_p of the last tile are never written by the staging)
    for (int i = tid * 16; i < (co_tiles + ci_tiles) * 32 * PITCH; i += 256 * 16) *reinterpret_cast<uint4*>(lds + i) = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const int units = (KT / 8) * (CGo + CGi);  // 8-row x 8-channel patches per staged K tile (at most 2 per thread, checked on the host)
    // the 16 row loads of a thread are issued as one batch (raw registers), transposed and staged afterwards
    uint4 pre[2][8];
    unsigned okbits = 0;  // validity of the 16 prefetched rows; applied when they are staged (a select right after a load would
                          // make hipcc wait for that load on the spot and serialise the batch)
    auto fetch = [&](long rb) {
        okbits = 0;
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int u = tid + v * 256;
            const bool live = u < units;
            const int uc = live ? u : 0;
            const int g = uc % (CGo + CGi), r8 = uc / (CGo + CGi);
            const bool is_a = g < CGo;
            const int cg = is_a ? g : g - CGo;
            const int cp = is_a ? d.Cout_p : d.Cin_p;
            const __bf16* src = (is_a ? dy : x) + cg * 8;
            // (not wg_load8: with the window map in a region of its own beside it the kernel ran 10 - 16 % slower, profiles/README.md)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const long r = rb + r8 * 8 + i;
                bool ok = live && r < r1;
                long row = ok ? r : r0;
                if (!is_a && strided) ok = wg_window_row(d, row, tt, th, tw, row) && ok;
                pre[v][i] = *reinterpret_cast<const uint4*>(src + row * cp);
                okbits |= (ok ? 1u : 0u) << (v * 8 + i);
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int u = tid + v * 256;
            if (u < units) {
                const int g = u % (CGo + CGi), r8 = u / (CGo + CGi);
                const bool is_a = g < CGo;
                const int cg = is_a ? g : g - CGo;
                wg_stage(lds, (is_a ? 0 : Bt_off) + (cg * 8) * PITCH + wg_slot(r8, cg, SLOTS) * 16, PITCH, pre[v], okbits >> (v * 8));
            }
        }
    };
    // (Issuing the next tile's loads before this tile's MFMAs -- a register software pipeline -- was measured 5 % SLOWER over the
    // 61 layers: the kernel is bound by HBM on the large layers and by its few blocks on the small ones, not by load latency.)
    for (long rb = r0; rb < r1; rb += KT) {
        fetch(rb);
        stage();
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < KT / 16; ++kk) {
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                const bf16x8 a = wg_frag<SLOTS>(At, PITCH, t_co[j], m, kk * 2 + h);
                const bf16x8 b = wg_frag<SLOTS>(Bt, PITCH, t_ci[j], m, kk * 2 + h);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[j], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < TPW; ++j)
        if (t_ok[j]) wg_tile_atomic(dw, acc[j], t_co[j] * 32, t_ci[j] * 32 + m, h, d.Cout, d.Cin, taps, tap);
}

// ---- the same for WIDE stride-1 pointwise layers (X3D stages 4-5: 216 <-> 96, 432 <-> 192 channels) -----------------------------
// pw_wgrad_bf16_kernel stages ALL channels of dy and x per 32-row step in every block and then lets blockIdx.y pick 16 of the (co, ci)
// tiles: on the 432 x 192 layers six y-blocks each load, transpose and store the same 624 channels for 8 MFMAs per wave and step, one
// exposed L2 round trip per step, 210 blocks for 256 CUs -- 71 us for 31 MB (0.44 TB/s), 69 us for 63 MB on the 216 x 96 layers; 34
// launches, 2.4 of the step's 32 ms.  Here a block owns a 2 x 2 group of tiles (one per wave) and stages ONLY the 64 + 64 channels those
// need, 128 rows per step: one 8 x 8 patch per thread and step, 8 MFMAs per wave between barriers, 35 KB of LDS (several blocks per CU,
// so one block's round trip hides under another's MFMAs), and 4 x 1024 atomics per block instead of 16 x 1024.
constexpr int WT_KT = 128, WT_PITCH = WT_KT * 2 + 16;

// COT x CIT tiles per WAVE (round 4): a block owns (2 COT) x (2 CIT) tiles.  (1, 1) stages 32 KB per 128-row step for 8 MFMAs per wave -- more than a
// CU takes from L2 in the time; (1, 2) / (2, 1) stage 48 KB for 16 (one shared fragment read per two MFMAs) and halve the groups along the wide side.
template <int COT, int CIT>
__global__ __launch_bounds__(256) void pw_wgrad_tile_kernel(const __bf16* __restrict__ x, const __bf16* __restrict__ dy, float* __restrict__ dw,
                                                            pasn_conv_desc d, int co_groups, int ci_groups, int rows_per_block, int gy2) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int CA = 64 * COT, CB = 64 * CIT;       // channels of dy / x a block stages
    constexpr int GA = CA / 8, GB = CB / 8, NG = GA + GB;  // 8-channel groups
    constexpr int NP = (16 * NG + 255) / 256;         // 8-row x 8-channel patches per thread and step
    constexpr int SLOTS = WT_KT / 8;
    unsigned char* At = lds;                  // [CA co channels][WT_PITCH]
    unsigned char* Bt = lds + CA * WT_PITCH;  // [CB ci channels][WT_PITCH]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = lane & 31, h = lane >> 5;
    const long R = (long)d.N * d.To * d.Ho * d.Wo;
    // Block -> (row range, tile group).  The gy tile groups of one row range read the same rows (each its own channels of them): as
    // blockIdx.y of a 2-D grid they ran a whole sweep over the rows apart, and every group fetched its rows from the fabric again -- 327 MB for
    // a 125 MB layer at 216 <-> 96 channels, 3.5 TB/s of fabric traffic for 1.3 TB/s of algorithmic bytes.  1-D grid (gy2 > 0): workgroups
    // b, b + 8, b + 16, ... share an XCD (round-robin dispatch), so the j-th block of XCD b % 8 takes tile group j % gy of row range
    // (j / gy) * 8 + b % 8: the groups of a row range run back to back on ONE L2.
    int bx = blockIdx.x, by = blockIdx.y;
    if (gy2 > 0) {
        const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        by = j % gy2;
        bx = (j / gy2) * 8 + xcd;
        if ((long)bx * rows_per_block >= R) return;  // (the grid is padded to whole groups of 8 row ranges)
    }
    const long r0 = (long)bx * rows_per_block, r1 = min(R, r0 + rows_per_block);
    const int cop = by / ci_groups, cip = by % ci_groups;
    const int co0 = cop * CA, ci0 = cip * CB;  // first channel of this block's co / ci tiles
    // staging roles: NP patches of 8 rows x 8 channels per thread and step; patch p = tid + 256 k -> channel group p % NG (fastest: a row's
    // groups are contiguous in memory), row octet p / NG
    const __bf16* src[NP];
    int dst[NP];  // LDS byte offset, -1 = no patch
    int cpp[NP], r8[NP];
    bool pok[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int p = tid + 256 * k;
        const int g = p % NG;
        r8[k] = min(p / NG, 15);
        const bool is_a = g < GA;
        const int cg = is_a ? g : g - GA;
        cpp[k] = is_a ? d.Cout_p : d.Cin_p;
        const int ch = (is_a ? co0 : ci0) + cg * 8;
        pok[k] = p < 16 * NG && ch < cpp[k];  // a group past the last tile, or no patch: zeros / nothing
        src[k] = (is_a ? dy : x) + (pok[k] ? ch : 0);
        dst[k] = p < 16 * NG ? (is_a ? 0 : CA * WT_PITCH) + (cg * 8) * WT_PITCH + wg_slot(r8[k], cg, SLOTS) * 16 : -1;
    }
    f32x16 acc[COT][CIT];
#pragma unroll
    for (int a = 0; a < COT; ++a)
#pragma unroll
        for (int b = 0; b < CIT; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.0f;
    const int tco = (wave >> 1) * COT, tci = (wave & 1) * CIT;  // this wave's first tile inside the block's group
    // The rows of step s + 1 are requested BEFORE the MFMAs of step s (register double buffer): a block's steps no longer each expose a
    // memory round trip, so fewer, longer blocks do the job -- and every block ends in fp32 atomics on the same small matrix.
    uint4 pre[NP][8];
    unsigned okbits[NP];  // applied after ALL loads are issued (a select next to a load serialises the batch)
    auto request = [&](long rb) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            okbits[k] = 0;
            wg_load8<long>(src[k], rb + r8[k] * 8, r1, r0, pok[k], cpp[k], pre[k], okbits[k]);
        }
    };
    if (r0 < r1) request(r0);
    for (long rb = r0; rb < r1; rb += WT_KT) {
#pragma unroll
        for (int k = 0; k < NP; ++k)
            if (dst[k] >= 0) wg_stage(lds, dst[k], WT_PITCH, pre[k], okbits[k]);
        if (rb + WT_KT < r1) request(rb + WT_KT);  // in flight under the barrier and the MFMAs below
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < WT_KT / 16; ++kk) {
            bf16x8 a[COT], b[CIT];
#pragma unroll
            for (int i = 0; i < COT; ++i) a[i] = wg_frag<SLOTS>(At, WT_PITCH, tco + i, m, kk * 2 + h);
#pragma unroll
            for (int j = 0; j < CIT; ++j) b[j] = wg_frag<SLOTS>(Bt, WT_PITCH, tci + j, m, kk * 2 + h);
#pragma unroll
            for (int i = 0; i < COT; ++i)
#pragma unroll
                for (int j = 0; j < CIT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < COT; ++i)
#pragma unroll
        for (int j = 0; j < CIT; ++j) {  // (not wg_tile_atomic: through it the <1, 2> instance ran 432 -> 192 2.7 % slower, profiles/README.md)
            const int cig = ci0 + (tci + j) * 32 + m;
            if (cig < d.Cin) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int cog = co0 + (tco + i) * 32 + acc_row(reg, h);
                    if (cog < d.Cout) unsafeAtomicAdd(dw + (size_t)cog * d.Cin + cig, acc[i][j][reg]);
                }
            }
        }
}

// ---- the route: one decision per launch (wgrad_tile.h), read by the workspace size, the probes and the launches -------------------------
// rows per block of a split over `parts` row partitions, in whole KT-row steps
static int wg_rows_per_block(long R, long parts, int KT) { return (ceil_div(R, parts) + KT - 1) / KT * KT; }

// HALO: stride-1 "same" (1,3,3) / (3,1,1) convs, bf16 (conv_wgrad_halo_kernel).  false: not this arm (a layer of these windows that misses
// the kernel's LDS / staging-unit limits takes no partial-buffer arm at all)
static bool route_halo(const pasn_conv_desc& d, int dtype, WgradRoute& r, bool& windows) {
    windows = false;
    if (tune_is("PASN_NO_WGRAD_HALO", '1') || dtype != PASN_BF16) return false;
    if (d.st != 1 || d.sh != 1 || d.sw != 1 || d.To != d.Ti || d.Ho != d.Hi || d.Wo != d.Wi) return false;
    WhGeom& g = r.h;
    if (d.kt == 1 && d.pt == 0 && d.kh == 3 && d.kw == 3 && d.ph == 1 && d.pw == 1 && d.Wi % 2 == 0) g.mode = 0;
    else if (d.kt == 3 && d.pt == 1 && d.kh == 1 && d.kw == 1 && d.ph == 0 && d.pw == 0) g.mode = 1;
    else return false;
    if (d.Cin_p % 8 || d.Cout_p % 8) return false;
    const long M = (long)d.N * d.To * d.Ho * d.Wo;
    if (M * d.Cin_p >= (1L << 31) || M * d.Cout_p >= (1L << 31)) return false;
    windows = true;
    g.taps = g.mode == 0 ? 9 : 3;
    g.HAL = g.mode == 0 ? (d.Wi + 63) / 64 * 64 : 0;  // L a multiple of 128: copy pitch = 4 dwords mod 64 banks
    g.L = WH_KT + 2 * g.HAL;
    g.pitchA = WH_KT * 2 + 16;
    g.pitchB = g.L * 2 + 16;
    g.co_tiles = ceil_div(d.Cout_p, 32);
    g.ci_tiles = ceil_div(d.Cin_p, 32);
    g.Cout_r = g.co_tiles * 32;
    g.Cin_r = g.ci_tiles * 32;
    const int cot = g.co_tiles >= 3 ? 3 : g.co_tiles;
    r.lds = (size_t)cot * 32 * g.pitchA + (size_t)3 * 64 * g.pitchB + 2 * (WH_KT / 8);
    // one block per CU (LDS); a thread stages at most two of the step's patches (dy, then the three x copies)
    if (r.lds > 160 * 1024 || (WH_KT / 8) * cot * 4 + 3 * (g.L / 8) * 8 > 1024) return false;
    g.co_groups = ceil_div(g.co_tiles, cot);
    g.ci_groups = ceil_div(g.ci_tiles, 2);
    // about two rounds of blocks, at least two 128-row steps each, at most 256 partitions (partial buffer)
    const long parts = std::max<long>(1, std::min<long>(std::min<long>(256, 512 / ((long)g.co_groups * g.ci_groups) + 1), M / (2 * WH_KT)));
    g.rows_per_block = wg_rows_per_block(M, parts, WH_KT);
    g.parts = ceil_div(M, g.rows_per_block);
    r.arm = WgradRoute::HALO;
    r.sel_a = cot;
    r.sel_b = ceil_div(std::min(2, g.ci_tiles) * g.taps, 8);  // (ci tile, tap) pairs per wave
    r.grid = dim3(g.parts, g.co_groups, g.ci_groups);
    r.rows_per_block = g.rows_per_block, r.parts = g.parts;
    r.taps = g.taps, r.Cout_r = g.Cout_r, r.Cin_r = g.Cin_r;
    return true;
}

// GATHER: the other windowed / strided convs, bf16 (conv_wgrad_gather_kernel)
static bool route_gather(const pasn_conv_desc& d, int dtype, WgradRoute& r) {
    if (tune_is("PASN_NO_WGRAD_GATHER", '1')) return false;
    if (dtype != PASN_BF16 || d.Cin_p % 8 || d.Cout_p % 8) return false;
    r.taps = d.kt * d.kh * d.kw;
    const bool strided = d.st != 1 || d.sh != 1 || d.sw != 1;
    const bool det = tune("PASN_WGRAD_DET") ? atoi(tune("PASN_WGRAD_DET")) != 0 : false;
    if (r.taps == 1 && !strided && !det) return false;  // plain pointwise layers keep their (atomic) kernels unless asked
    if (r.taps > 27) return false;
    const long R = (long)d.N * d.To * d.Ho * d.Wo, Rin = (long)d.N * d.Ti * d.Hi * d.Wi;
    if (R * d.Cout_p >= (1L << 31) || Rin * d.Cin_p >= (1L << 31)) return false;
    const int co_pairs = ceil_div(ceil_div(d.Cout_p, 32), 2);
    r.ci_split = ceil_div(ceil_div(d.Cin_p, 32), 2);
    r.Cout_r = co_pairs * 64;
    r.Cin_r = r.ci_split * 64;
    const long gy = (long)co_pairs * r.ci_split * r.taps;
    // about 2048 blocks, at least two 128-row steps each, at most 48 MB of partials
    const long per_part = (long)r.taps * r.Cout_r * r.Cin_r * 4;
    const long parts = std::max<long>(1, std::min<long>(std::min<long>((48L << 20) / per_part, 2048 / gy + 1), R / (2 * WH_KT)));
    r.rows_per_block = wg_rows_per_block(R, parts, WH_KT);
    r.parts = ceil_div(R, r.rows_per_block);
    r.arm = WgradRoute::GATHER;
    r.grid = dim3((unsigned)r.parts, co_pairs * r.ci_split, r.taps);
    r.lds = (size_t)128 * (WH_KT * 2 + 16);
    return true;
}

// TILE: wide stride-1 pointwise layers, bf16 (pw_wgrad_tile_kernel)
static bool route_tile(const pasn_conv_desc& d, WgradRoute& r) {
    const bool pointwise = d.kt * d.kh * d.kw == 1 && d.st == 1 && d.sh == 1 && d.sw == 1 && d.pt == 0 && d.ph == 0 && d.pw == 0;
    const int co_tiles = ceil_div(d.Cout_p, 32), ci_tiles = ceil_div(d.Cin_p, 32);
    if (tune_is("PASN_NO_WGRAD_TILE", '1') || !pointwise || co_tiles + ci_tiles <= 6) return false;  // narrow layers: every block stages all channels anyway
    // tiles per wave along the wide side (PASN_WGT_WIDE=0: one tile per wave everywhere, the kernel of rounds 2-3)
    const bool wide = !tune_is("PASN_WGT_WIDE", '0');
    const int cot = wide && co_tiles >= 2 * ci_tiles ? 2 : 1, cit = wide && cot == 1 && ci_tiles >= 2 * co_tiles ? 2 : 1;
    r.co_split = ceil_div(co_tiles, 2 * cot), r.ci_split = ceil_div(ci_tiles, 2 * cit);
    const long R = (long)d.N * d.To * d.Ho * d.Wo;
    const int gy = r.co_split * r.ci_split;
    // row partitions: about four blocks per CU in flight, at least two 128-row steps each
    // (two tiles per wave: the same ~13 steps per block, i.e. half the blocks -- 57-59 us at 216 <-> 96 against 64-69 with 1024: r04_pwwg_xcd.txt)
    const long target = tune_dev("PASN_WGT_BLOCKS") ? atol(tune_dev("PASN_WGT_BLOCKS")) : (cot * cit == 2 ? 512 : 1024);
    const long parts = std::max<long>(1, std::min<long>(target / gy + 1, R / (2 * WT_KT)));
    r.rows_per_block = wg_rows_per_block(R, parts, WT_KT);
    r.parts = ceil_div(R, r.rows_per_block);
    r.gy2 = tune_is("PASN_WGT_XCD", '0') ? 0 : gy;
    r.grid = r.gy2 ? dim3((unsigned)(ceil_div(r.parts, 8L) * 8 * gy)) : dim3((unsigned)r.parts, gy);
    r.lds = (size_t)64 * (cot + cit) * WT_PITCH;
    r.arm = WgradRoute::TILE;
    r.sel_a = cot, r.sel_b = cit;
    return true;
}

// LDS: every other layer whose channels fit the kernel's LDS and its two patches per thread, bf16 (pw_wgrad_bf16_kernel)
static bool route_lds(const pasn_conv_desc& d, WgradRoute& r) {
    const int co_tiles = ceil_div(d.Cout_p, 32), ci_tiles = ceil_div(d.Cin_p, 32);
    const int ntiles = co_tiles * ci_tiles, taps = d.kt * d.kh * d.kw;
    const int KT = co_tiles + ci_tiles <= 6 ? 128 : 32;  // few channels: stage more rows per step so every thread has a patch to move
    const size_t lds = (size_t)(co_tiles + ci_tiles) * 32 * (KT * 2 + 16);  // the kernel's PITCH per channel row
    if (lds > 64 * 1024) return false;
    if ((KT / 8) * (d.Cout_p / 8 + d.Cin_p / 8) > 512) return false;  // the kernel's register pipeline holds 2 patches per thread
    int tpw = ceil_div(ntiles, 4);
    tpw = tpw <= 1 ? 1 : tpw <= 2 ? 2 : tpw <= 4 ? 4 : 8;
    const int tpw_cap = tune_dev("PASN_WG_TPW") ? atoi(tune_dev("PASN_WG_TPW")) : 4;  // 8 tiles per wave (occupancy 1) measured 7 % slower
    tpw = std::min(tpw, std::max(1, tpw_cap));
    const int gy = ceil_div(ntiles, 4 * tpw);
    const long R = (long)d.N * d.To * d.Ho * d.Wo;
    // split-K partitions: enough blocks to fill the chip, but every partition ends in ntiles*1024 atomics on the same addresses
    const long want_blocks = std::max<long>(1, std::min<long>(2048 / ((long)gy * taps) + 1, std::max<long>(16, 3000 / ntiles)));
    r.rows_per_block = std::max(KT, wg_rows_per_block(R, want_blocks, KT));
    r.parts = ceil_div(R, r.rows_per_block);
    r.grid = dim3((unsigned)r.parts, gy, taps);
    r.lds = lds;
    r.co_split = co_tiles, r.ci_split = ci_tiles;
    r.arm = WgradRoute::LDS;
    r.sel_a = KT, r.sel_b = tpw;
    return true;
}

// GENERIC: conv_wgrad_kernel, any dtype and window
static void route_generic(const pasn_conv_desc& d, int dtype, WgradRoute& r) {
    const int taps = d.kt * d.kh * d.kw;
    r.ci_split = ceil_div(d.Cin, 32);
    r.tiles = (long)ceil_div(d.Cout, 32) * r.ci_split * taps;
    const long R = (long)d.N * d.To * d.Ho * d.Wo;
    r.rows_per_block = wgrad_rows_per_wave(R, (int)r.tiles);
    r.grid = dim3(ceil_div(R, (long)r.rows_per_block * 4), (unsigned)r.tiles);
    r.parts = (long)r.grid.x * 4;  // every wave of the grid adds its (possibly empty) sum
    r.arm = WgradRoute::GENERIC;
    r.sel_a = dtype == PASN_BF16 ? 1 : 0;
    r.sel_b = taps == 1 && d.st == 1 && d.sh == 1 && d.sw == 1 && d.pt == 0 && d.ph == 0 && d.pw == 0;
}

// has_ws: the caller brings pasn_conv3d_wgrad_workspace_bytes of workspace (without it a partial-buffer layer takes the atomic arms);
// lds_switch = false: the bf16 kernels whatever PASN_NO_WGRAD_LDS says (the first conv's im2col arm)
WgradRoute wgrad_route(const pasn_conv_desc& d, int dtype, bool has_ws, bool lds_switch) {
    WgradRoute r{};
    bool halo_windows = false;
    bool partial = has_ws && route_halo(d, dtype, r, halo_windows);
    if (has_ws && !partial && !halo_windows) partial = route_gather(d, dtype, r = WgradRoute{});
    if (partial) {
        r.partial_bytes = (size_t)r.parts * r.taps * r.Cout_r * r.Cin_r * sizeof(float);
        if (r.partial_bytes) return r;  // (no rows, no partition: the atomic arms)
    }
    r = WgradRoute{};
    const bool bf16_arms = dtype == PASN_BF16 && !(lds_switch && tune("PASN_NO_WGRAD_LDS")) && d.kt * d.kh * d.kw <= 64;
    if (!(bf16_arms && (route_tile(d, r) || route_lds(d, r)))) route_generic(d, dtype, r);
    return r;
}

// launches the atomic arms (dw zeroed by the caller; GENERIC: r.tiles within the grid limit, checked by the caller)
static void wgrad_atomic_launch(const WgradRoute& r, const void* x, const void* dy, float* dw, const pasn_conv_desc& d, hipStream_t s) {
    const __bf16 *xb = (const __bf16*)x, *dyb = (const __bf16*)dy;
#define WGT(A, B) hipLaunchKernelGGL((pw_wgrad_tile_kernel<A, B>), r.grid, dim3(256), r.lds, s, xb, dyb, dw, d, r.co_split, r.ci_split, r.rows_per_block, r.gy2)
#define PW(K, T) hipLaunchKernelGGL((pw_wgrad_bf16_kernel<K, T>), r.grid, dim3(256), r.lds, s, xb, dyb, dw, d, r.co_split, r.ci_split, r.rows_per_block)
#define WG(T, P) hipLaunchKernelGGL((conv_wgrad_kernel<T, P>), r.grid, dim3(256), 0, s, (const T*)x, (const T*)dy, dw, d, r.ci_split, r.rows_per_block)
    if (r.arm == WgradRoute::TILE) {
        if (r.sel_a == 2) WGT(2, 1);
        else if (r.sel_b == 2) WGT(1, 2);
        else WGT(1, 1);
    } else if (r.arm == WgradRoute::LDS && r.sel_a == 128) {
        if (r.sel_b == 1) PW(128, 1);
        else if (r.sel_b == 2) PW(128, 2);
        else PW(128, 4);
    } else if (r.arm == WgradRoute::LDS) {
        if (r.sel_b == 1) PW(32, 1);
        else if (r.sel_b == 2) PW(32, 2);
        else if (r.sel_b == 4) PW(32, 4);
        else PW(32, 8);
    } else {
        if (r.sel_a && r.sel_b) WG(__bf16, true);
        else if (r.sel_a) WG(__bf16, false);
        else if (r.sel_b) WG(float, true);
        else WG(float, false);
    }
#undef WG
#undef PW
#undef WGT
}

// the first conv's weight gradient over its im2col rows (above): the bf16 kernels whatever PASN_NO_WGRAD_LDS says; false: neither covers it
bool pw_wgrad_bf16(const void* x, const void* dy, float* dw, const pasn_conv_desc& d, hipStream_t s) {
    const WgradRoute r = wgrad_route(d, PASN_BF16, false, false);
    if (r.arm == WgradRoute::GENERIC) return false;
    wgrad_atomic_launch(r, x, dy, dw, d, s);
    return true;
}

}  // namespace pasn

extern "C" size_t pasn_conv3d_wgrad_workspace_bytes(const pasn_conv_desc* d, int dtype) {
    return d ? wgrad_route(*d, dtype, true).partial_bytes : 0;
}

extern "C" int pasn_conv3d_wgrad_variant(const pasn_conv_desc* d, int dtype, int has_ws) {
    if (!d) return 0;
    const WgradRoute r = wgrad_route(*d, dtype, has_ws != 0);  // (GATHER has no selectors, only HALO a mode: both fields are 0 elsewhere)
    return r.arm * 100000 + r.h.mode * 10000 + r.sel_a * 100 + r.sel_b;
}

extern "C" long pasn_conv3d_wgrad_row_parts(const pasn_conv_desc* d, int dtype, int has_ws) {
    if (!d) return 0;
    const WgradRoute r = wgrad_route(*d, dtype, has_ws != 0);
    return r.parts + (((long)r.grid.x * r.grid.y * r.grid.z) << 32);
}

extern "C" int pasn_conv3d_wgrad_ws(const void* x, const void* dy, float* dw, const pasn_conv_desc* d, int dtype, void* ws, void* stream) {
    PASN_REQUIRE(x && dy && dw && d, "null pointer");
    PASN_REQUIRE(d->Cin_p % 8 == 0 && d->Cout_p % 8 == 0 && d->Cin <= d->Cin_p && d->Cout <= d->Cout_p, "bad channel extents");
    hipStream_t s = (hipStream_t)stream;
    const WgradRoute r = wgrad_route(*d, dtype, ws != nullptr);
    if (r.partial_bytes) {
        wgrad_partial_launch(r, x, dy, dw, ws, *d, s);
        return check_launch("conv3d_wgrad_halo");
    }
    PASN_REQUIRE(r.arm != WgradRoute::GENERIC || r.tiles <= 65535, "too many weight tiles for one launch");
    wgrad_atomic_launch(r, x, dy, dw, *d, s);
    return check_launch("conv3d_wgrad");
}

extern "C" int pasn_conv3d_wgrad(const void* x, const void* dy, float* dw, const pasn_conv_desc* d, int dtype, void* stream) {
    return pasn_conv3d_wgrad_ws(x, dy, dw, d, dtype, nullptr, stream);
}
