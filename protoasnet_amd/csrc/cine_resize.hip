// cine_resize.hip -- the reference dataset's clip resize (as_dataloader.py:204-207: skimage.transform.resize(window, (T, H, W))) on the
// device, over a ragged batch of raw cine windows, in one launch.
//
// Numerical contract (scikit-image >= 0.19 defaults: order=1, mode='reflect', anti_aliasing when an axis shrinks, clip=True,
// preserve_range=False):
//   1. float conversion: uint8 / 255, fp32 as is;
//   2. f = n_in / n_out per axis, sigma = max(0, (f - 1) / 2);
//   3. if an axis shrinks: scipy.ndimage.gaussian_filter(x, sigma, mode='mirror', truncate=4.0) (radius int(4 sigma + 0.5));
//   4. scipy.ndimage.zoom(., 1 / f, order=1, mode='mirror', grid_mode=True): source coordinate (o + 0.5) f - 0.5;
//   5. clip to the input's range.
// The operator is separable, out = A_T (x) A_H (x) A_W x, each A_axis banded, non-negative, rows summing to 1 (step 5 is a no-op).
// The host builds the three band tables in float64 and rounds them to fp32 once (protoasnet_amd/resample.py); this kernel applies them
// with fp32 accumulation, the uint8 scale 1/255 applied to the accumulated value.
//
// One workgroup owns (clip n, a tile of output rows x columns, a chunk of TT output frames).  For every input frame of the chunk's T band:
//   stage the tile's input rows (the union of its H bands, only the columns of its W bands) into LDS with 16-byte loads, a chunk of rows
//   at a time, and run the W pass of each staged row into an LDS row buffer (fp32, one row per input row of the H band union);
//   then each thread takes its OPT output pixels through the H pass and accumulates acc[t] += A_T[t, f] * v in registers.
// The raw window is read from HBM once per tile (the H halo of neighbouring tiles comes from L2); the clip is written once, with the
// optional epilogue (v - mean) / std.  No intermediate in global memory.
//
// Safety: a clip whose descriptor or tables disagree with the launch (table lengths, source range, LDS geometry) is not read: its tile
// is written as NaN.
#include "common.h"

namespace pasn {

struct CineResizeArgs {
    const unsigned char* src;
    long src_bytes;
    const long long* desc;  // [N][8]: src byte offset, first frame, T_w, H0, W0, table offsets of T / H / W (int32 units)
    const int* bands;       // tables: n_in, n_out, S, start[n_out], weights[n_out][S] (fp32 bits)
    long bands_len;         // int32 entries of bands
    void* y;
    int N, T, H, W;
    int tile_h, tile_w, tmp_rows, raw_pitch, chunk_rows, band_floats;
    float scale, mean, stdev;
};

struct Band {
    const int* start;
    const float* w;
    int S;
};

__device__ __forceinline__ Band band_at(const int* bands, long bands_len, long long off, int n_in, int n_out, bool& ok) {
    ok = ok && off >= 0 && off + 3 <= bands_len;
    if (!ok) return Band{bands, reinterpret_cast<const float*>(bands), 1};
    const int* b = bands + off;
    ok = b[0] == n_in && b[1] == n_out && b[2] > 0 && b[2] <= n_in && off + 3 + (long long)n_out * (1 + b[2]) <= bands_len;
    return Band{b + 3, reinterpret_cast<const float*>(b + 3 + n_out), b[2]};
}

template <typename TI, typename TO, int TT, int OPT>
__global__ __launch_bounds__(256) void cine_resize_kernel(CineResizeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int ES = sizeof(TI);
    const int tid = threadIdx.x;
    const int tiles_w = (a.W + a.tile_w - 1) / a.tile_w;
    const int h0 = (blockIdx.x / tiles_w) * a.tile_h, w0 = (blockIdx.x % tiles_w) * a.tile_w;
    const int nh = min(a.tile_h, a.H - h0), nw = min(a.tile_w, a.W - w0);
    const int t0 = blockIdx.z * TT, nt = min(TT, a.T - t0);
    const int n = blockIdx.y;
    const long long* d = a.desc + (long)n * 8;
    const long long src_off = d[0], first = d[1];
    const int Tw = (int)d[2], H0 = (int)d[3], W0 = (int)d[4];
    bool ok = Tw > 0 && H0 > 0 && W0 > 0 && first >= 0 && src_off >= 0 && (src_off % ES) == 0 &&
              src_off + (first + Tw) * (long long)H0 * W0 * ES <= a.src_bytes;
    const Band bt = band_at(a.bands, a.bands_len, d[5], Tw, a.T, ok);
    const Band bh = band_at(a.bands, a.bands_len, d[6], H0, a.H, ok);
    const Band bw = band_at(a.bands, a.bands_len, d[7], W0, a.W, ok);
    // band unions of the tile (starts are non-decreasing): frames [f_lo, f_hi), rows [r_lo, r_hi), columns [c_lo, c_hi)
    int f_lo = 0, f_hi = 0, r_lo = 0, r_hi = 0, c_lo = 0, c_hi = 0;
    if (ok) {
        f_lo = bt.start[t0], f_hi = bt.start[t0 + nt - 1] + bt.S;
        r_lo = bh.start[h0], r_hi = bh.start[h0 + nh - 1] + bh.S;
        c_lo = bw.start[w0], c_hi = bw.start[w0 + nw - 1] + bw.S;
        ok = f_lo >= 0 && f_hi <= Tw && r_lo >= 0 && r_hi <= H0 && c_lo >= 0 && c_hi <= W0 && r_hi - r_lo <= a.tmp_rows &&
             (c_hi - c_lo) * ES + 15 <= a.raw_pitch && r_hi - r_lo >= bh.S && c_hi - c_lo >= bw.S &&
             nw * (bw.S + 1) + nh * (bh.S + 1) <= a.band_floats;
    }
    const long out_plane = (long)a.H * a.W;
    TO* y = static_cast<TO*>(a.y) + (long)n * a.T * out_plane;
    if (!ok) {  // block-uniform: no barrier is skipped by part of the block
        for (int i = tid; i < nt * nh * nw; i += 256) {
            const int t = i / (nh * nw), r = i % (nh * nw);
            y[(long)(t0 + t) * out_plane + (long)(h0 + r / nw) * a.W + w0 + r % nw] = (TO)__builtin_nanf("");
        }
        return;
    }
    const int R = r_hi - r_lo;
    float* tmp = reinterpret_cast<float*>(lds);  // [R][nw]
    unsigned char* raw = lds + (((long)a.tmp_rows * a.tile_w * 4 + 15) & ~15L);  // [chunk_rows][raw_pitch]
    // the tile's W and H bands, staged once: weights [nw][S_W], [nh][S_H], then the band starts relative to the tile unions
    float* wW = reinterpret_cast<float*>(raw + (long)a.chunk_rows * a.raw_pitch);
    float* wH = wW + nw * bw.S;
    int* sW = reinterpret_cast<int*>(wH + nh * bh.S);
    int* sH = sW + nw;
    for (int i = tid; i < nw * bw.S; i += 256) wW[i] = bw.w[(long)w0 * bw.S + i];
    for (int i = tid; i < nh * bh.S; i += 256) wH[i] = bh.w[(long)h0 * bh.S + i];
    for (int i = tid; i < nw; i += 256) sW[i] = min(max(bw.start[w0 + i] - c_lo, 0), c_hi - c_lo - bw.S);  // (clamps: a corrupt table)
    for (int i = tid; i < nh; i += 256) sH[i] = min(max(bh.start[h0 + i] - r_lo, 0), R - bh.S);
    // (the first staging barrier below orders these writes before their reads)
    const int nv = a.raw_pitch / 16;
    const long row_bytes = (long)W0 * ES;

    float acc[OPT][TT];
#pragma unroll
    for (int j = 0; j < OPT; ++j)
#pragma unroll
        for (int t = 0; t < TT; ++t) acc[j][t] = 0.0f;

    for (int f = f_lo; f < f_hi; ++f) {
        const long frame = src_off + (first + f) * (long)H0 * row_bytes;
        for (int rc0 = r_lo; rc0 < r_hi; rc0 += a.chunk_rows) {
            const int nr = min(a.chunk_rows, r_hi - rc0);
            // stage rows rc0 .. rc0 + nr - 1, columns [c_lo, c_hi), as whole 16-byte vectors from the aligned-down start
            for (int i = tid; i < nr * nv; i += 256) {
                const int r = i / nv, v = i - r * nv;
                const long addr = ((frame + (rc0 + r) * row_bytes + (long)c_lo * ES) & ~15L) + 16L * v;
                if (addr + 16 <= a.src_bytes)
                    *reinterpret_cast<uint4*>(raw + (long)r * a.raw_pitch + 16 * v) = *reinterpret_cast<const uint4*>(a.src + addr);
            }
            __syncthreads();
            // W pass of the staged rows -> tmp rows (rc0 - r_lo) ..: a thread takes one column of up to 4 rows, each weight read once
            const int groups = (nr + 3) / 4;
            for (int i = tid; i < groups * nw; i += 256) {
                const int g = i / nw, x = i - g * nw;
                const int s0 = sW[x];
                const float* wk = wW + x * bw.S;
                const TI* row[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int r = min(4 * g + q, nr - 1);  // a short last group repeats its last row (not stored)
                    const int head = (int)((frame + (rc0 + r) * row_bytes + (long)c_lo * ES) & 15L);
                    row[q] = reinterpret_cast<const TI*>(raw + (long)r * a.raw_pitch + head) + s0;
                }
                float acc_w[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                for (int k = 0; k < bw.S; ++k) {
                    const float w = wk[k];
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc_w[q] = fmaf(w, (float)row[q][k], acc_w[q]);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (4 * g + q < nr) tmp[(rc0 - r_lo + 4 * g + q) * nw + x] = acc_w[q];
            }
            __syncthreads();  // staging buffer and tmp rows: the next chunk overwrites the one, the H pass reads the other
        }
        // H pass + T accumulation of this thread's output pixels
#pragma unroll
        for (int j = 0; j < OPT; ++j) {
            const int o = tid + 256 * j;
            if (o < nh * nw) {
                const int hh = o / nw, x = o % nw;
                const int s0 = sH[hh];
                const float* wk = wH + hh * bh.S;
                float v = 0.0f;
                for (int k = 0; k < bh.S; ++k) v = fmaf(wk[k], tmp[(s0 + k) * nw + x], v);
#pragma unroll
                for (int t = 0; t < TT; ++t) {
                    if (t < nt) {
                        const int k = f - bt.start[t0 + t];
                        if (k >= 0 && k < bt.S) acc[j][t] = fmaf(bt.w[(long)(t0 + t) * bt.S + k], v, acc[j][t]);
                    }
                }
            }
        }
        // (no barrier here: the next frame's staging writes only the staging buffer; its barrier orders this H pass before the next
        // W pass writes tmp)
    }
    {
#pragma clang fp contract(off)  // v = acc * scale rounded on its own: the epilogue equals (v - mean) / std of the unnormalised clip
#pragma unroll
    for (int j = 0; j < OPT; ++j) {
        const int o = tid + 256 * j;
        if (o < nh * nw) {
            TO* dst = y + (long)(h0 + o / nw) * a.W + w0 + o % nw;
#pragma unroll
            for (int t = 0; t < TT; ++t)
                if (t < nt) {
                    const float v = acc[j][t] * a.scale;  // plain operators under contract(off): the inlined __fmul_rn / __fsub_rn
                    dst[(long)(t0 + t) * out_plane] = (TO)__fdiv_rn(v - a.mean, a.stdev);  // would still fuse into one FMA
                }
        }
    }
    }
}

// output frames per workgroup (TT) and output pixels per thread (OPT) of the instance a launch with T output frames takes
static void resize_instance(int T, int& tt, int& opt) {
    if (T == 1) tt = 1, opt = 8;
    else if (T == 16) tt = 16, opt = 4;
    else if (T == 32) tt = 32, opt = 2;
    else tt = 8, opt = 4;  // generic: chunks of 8 output frames (grid z)
}

template <typename TI, typename TO>
static void launch_resize(const CineResizeArgs& a, int tt, int opt, dim3 grid, size_t lds, hipStream_t s) {
#define RESIZE(TT_, OPT_)                                                                                  \
    do {                                                                                                   \
        if (lds > 65536) PASN_MAX_LDS((int)lds, cine_resize_kernel<TI, TO, TT_, OPT_>);                    \
        hipLaunchKernelGGL((cine_resize_kernel<TI, TO, TT_, OPT_>), grid, dim3(256), lds, s, a);           \
    } while (0)
    if (tt == 1) RESIZE(1, 8);
    else if (tt == 16) RESIZE(16, 4);
    else if (tt == 32) RESIZE(32, 2);
    else RESIZE(8, 4);
#undef RESIZE
}

}  // namespace pasn

using namespace pasn;

extern "C" int pasn_cine_resize_pixels_per_block(int T) {
    int tt, opt;
    resize_instance(T, tt, opt);
    return 256 * opt;
}

extern "C" int pasn_cine_resize(const void* src, long src_bytes, const long long* desc, const int* bands, long bands_len, void* y, int N,
                                int T, int H, int W, int tile_h, int tile_w, int tmp_rows, int raw_pitch, int chunk_rows, int band_floats, float mean,
                                float stdev, int in_dtype, int out_dtype, void* stream) {
    PASN_REQUIRE(src && desc && bands && y && src_bytes > 0 && bands_len > 0 && N > 0 && T > 0 && H > 0 && W > 0, "bad arguments");
    PASN_REQUIRE(((uintptr_t)src & 15) == 0 && (src_bytes & 15) == 0, "the source buffer must be 16-byte aligned and a multiple of 16 bytes");
    PASN_REQUIRE(in_dtype == PASN_U8 || in_dtype == PASN_F32, "source dtype is uint8 or fp32");
    PASN_REQUIRE(out_dtype == PASN_F32 || out_dtype == PASN_BF16, "output dtype is fp32 or bf16");
    PASN_REQUIRE(stdev != 0.0f, "std must be non-zero");
    int tt, opt;
    resize_instance(T, tt, opt);
    PASN_REQUIRE(tile_h > 0 && tile_w > 0 && tile_h <= H && tile_w <= W && tile_h * tile_w <= 256 * opt,
                 "tile must hold at most pasn_cine_resize_pixels_per_block(T) output pixels");
    PASN_REQUIRE(tmp_rows > 0 && chunk_rows > 0 && raw_pitch >= 32 && raw_pitch % 16 == 0 && band_floats > 0, "bad LDS geometry");
    const size_t lds = (((size_t)tmp_rows * tile_w * 4 + 15) & ~(size_t)15) + (size_t)chunk_rows * raw_pitch + (size_t)band_floats * 4;
    PASN_REQUIRE(lds <= 160 * 1024, "LDS geometry exceeds 160 KiB");
    CineResizeArgs a{static_cast<const unsigned char*>(src), src_bytes, desc, bands, bands_len, y, N, T, H, W, tile_h, tile_w, tmp_rows, raw_pitch,
                     chunk_rows, band_floats, in_dtype == PASN_U8 ? 1.0f / 255.0f : 1.0f, mean, stdev};
    const long tiles = (long)((H + tile_h - 1) / tile_h) * ((W + tile_w - 1) / tile_w);
    PASN_REQUIRE(tiles < (1L << 31) && N < 65536 && (T + tt - 1) / tt < 65536, "grid too large");
    const dim3 grid((unsigned)tiles, (unsigned)N, (unsigned)((T + tt - 1) / tt));
    hipStream_t s = (hipStream_t)stream;
    if (in_dtype == PASN_U8) {
        if (out_dtype == PASN_BF16) launch_resize<uint8_t, __bf16>(a, tt, opt, grid, lds, s);
        else launch_resize<uint8_t, float>(a, tt, opt, grid, lds, s);
    } else {
        if (out_dtype == PASN_BF16) launch_resize<float, __bf16>(a, tt, opt, grid, lds, s);
        else launch_resize<float, float>(a, tt, opt, grid, lds, s);
    }
    return check_launch("cine_resize");
}
