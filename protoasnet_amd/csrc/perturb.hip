// perturb.hip -- explanation faithfulness: the deletion / insertion curves of faithfulness.py.  include/protoasnet_amd.h holds the
// definitions, tests/faithfulness_cases.py their numpy restatement.
//
// pasn_perturb_steps: ordering the V voxels of a uint8 map by (level descending, index ascending) is a 256-bin counting problem.  A tile
// is 256 chunks of 16 bytes laid on the 16-byte grid of the ROW'S ADDRESS (rows are misaligned when V is odd): chunk g of a row that
// starts `off` bytes past a 16-byte boundary holds the voxels [16 g - off, 16 g - off + 16), so that every chunk inside the row is one
// aligned 16-byte word of the map and of the output; the row's first and last chunk go byte by byte.  A thread's chunk is consecutive
// voxels and the threads of a tile are in voxel order: rank inside a tile = (matches in the threads before) + (matches before in the chunk).
//   perturb_hist_kernel   per tile a 256-bin LDS histogram (runs of equal bytes are added once) -> workspace, uint16 (a tile has 4096 voxels)
//   perturb_plan_kernel   per map: level totals, the position of each level's first voxel, the step of a level whose voxels all share one,
//                         the levels that straddle a count (at most S1: a count lies inside one level) and, per tile, their prefixes
//                         across the tiles with a "present in this tile" bit
//   perturb_write_kernel  per tile: a 256-entry LDS table answers every non-straddling level; per straddling level present in the tile
//                         its voxels are ranked across the block (a ballot per byte position, plus the waves before).  Everything it
//                         needs from the plan is loaded once, beside the tile's own bytes: no global load inside the loop over the levels
// pasn_perturb_apply: one block per (4096 voxels, step, map): the steps become an LDS byte mask once, then the C channels are copied from
// x or the baseline by it, 16 bytes per store on the 16-byte grid of the OUTPUT row (the mask is read at any byte offset through
// v_alignbyte).  pasn_perturb_curves: one block gathers the curves, integrates them and adds them onto the sweep's accumulators.
#include <cstring>

#include "common.h"
#include "eval_common.h"
#include "explain_common.h"

namespace pasn {

constexpr int PT_NT = 256, PLAN_NT = 1024, PT_TILE = PT_NT * 16, PT_MAX_S1 = 64, PT_MAX_MAPS = 65535, PT_MAX_C = 64;
constexpr uint32_t PT_PRESENT = 1u << 31;  // (positions are below 2^31)
constexpr long PT_MAX_V = (1L << 31) - 1, PT_MAX_CURVE_ROWS = 1L << 20;

// 16 consecutive bytes of a row of V bytes from voxel vbeg on (vbeg may lie before the row or past it); bit i of `valid`: byte i exists
struct Chunk {
    uint32_t w[4];
    unsigned valid;
    __device__ __forceinline__ unsigned byte(int i) const { return (w[i >> 2] >> ((i & 3) * 8)) & 0xffu; }
    __device__ __forceinline__ bool has(int i) const { return (valid >> i) & 1u; }
    __device__ __forceinline__ void set(int i, unsigned b) {
        const int sh = (i & 3) * 8;
        w[i >> 2] = (w[i >> 2] & ~(0xffu << sh)) | (b << sh);
    }
};

// (row + vbeg is 16-byte aligned by the tile geometry whenever the whole chunk lies inside the row)
__device__ __forceinline__ Chunk load_chunk(const uint8_t* __restrict__ row, long vbeg, long V) {
    Chunk c;
    if (vbeg >= 0 && vbeg + 16 <= V) {
        const uint4 q = *reinterpret_cast<const uint4*>(row + vbeg);
        c.w[0] = q.x, c.w[1] = q.y, c.w[2] = q.z, c.w[3] = q.w;
        c.valid = 0xffffu;
    } else {
        c.w[0] = c.w[1] = c.w[2] = c.w[3] = 0u;
        c.valid = 0u;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long v = vbeg + i;
            if (v >= 0 && v < V) {
                c.set(i, row[v]);
                c.valid |= 1u << i;
            }
        }
    }
    return c;
}

__device__ __forceinline__ void store_chunk(uint8_t* __restrict__ row, long vbeg, long V, const Chunk& c) {
    if (c.valid == 0xffffu) {
        *reinterpret_cast<uint4*>(row + vbeg) = make_uint4(c.w[0], c.w[1], c.w[2], c.w[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (c.has(i)) row[vbeg + i] = (uint8_t)c.byte(i);
    }
}

// tiles that cover a row wherever it starts: off = 0 for every row when V is a multiple of 16 (the bases are aligned), else up to 15
static long perturb_tiles(long V) { return ((V % 16 ? (V + 30) / 16 : V / 16) + PT_NT - 1) / PT_NT; }

struct StepsPlan {  // of one map
    uint8_t table[256];  // level -> its step (< 128), or 128 + j: the j-th straddling level
    int32_t nstr, pad[3];
    int32_t level[PT_MAX_S1], step0[PT_MAX_S1];  // of straddling level j: the level, the step of its first voxel
    uint32_t start[PT_MAX_S1];                   // the position of its first voxel
};

struct StepsWorkspace {
    uint16_t* hist;    // [M][tiles][256]
    uint32_t* prefix;  // [M][tiles][PT_MAX_S1]: voxels of straddling level j in the tiles before | PT_PRESENT when the tile holds some
    StepsPlan* plan;   // [M]
    size_t bytes;
};

static StepsWorkspace steps_workspace(void* ws, long M, long tiles) {
    StepsWorkspace w;
    Carve c{static_cast<char*>(ws)};
    w.plan = c.take<StepsPlan>((size_t)M, 16);
    w.prefix = c.take<uint32_t>((size_t)M * PT_MAX_S1 * tiles, 16);
    w.hist = c.take<uint16_t>((size_t)M * tiles * 256, 16);
    w.bytes = (c.used + 15) / 16 * 16;
    return w;
}

__device__ __forceinline__ long chunk_begin(const uint8_t* row, int tile) {
    return ((long)tile * PT_NT + threadIdx.x) * 16 - (long)((uintptr_t)row & 15);
}

__global__ __launch_bounds__(PT_NT) void perturb_hist_kernel(const uint8_t* __restrict__ maps, long V, long tiles, uint16_t* __restrict__ hist) {
    __shared__ uint32_t s_h[256];
    const int tid = threadIdx.x;
    const long m = blockIdx.y;
    s_h[tid] = 0u;
    __syncthreads();
    const uint8_t* row = maps + m * V;
    const Chunk c = load_chunk(row, chunk_begin(row, blockIdx.x), V);
    unsigned cur = 0u, run = 0u;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (!c.has(i)) continue;
        const unsigned L = c.byte(i);
        if (run && L != cur) {
            atomicAdd(&s_h[cur], run);
            run = 0u;
        }
        cur = L;
        ++run;
    }
    if (run) atomicAdd(&s_h[cur], run);
    __syncthreads();
    hist[(m * tiles + blockIdx.x) * 256 + tid] = (uint16_t)s_h[tid];
}

// the number of s with counts[s] <= pos
__device__ __forceinline__ int steps_at(const int32_t* counts, int S1, long pos) {
    int n = 0;
    for (int s = 0; s < S1; ++s) n += (long)counts[s] <= pos ? 1 : 0;
    return n;
}

// One block of PLAN_NT threads per map.  Thread (g, L) adds the tiles g, g + 4, ... of level L (eight loads in flight); threads L < 256
// then own level L; at the end a wave per straddling level scans its counts over the tiles.
__global__ __launch_bounds__(PLAN_NT) void perturb_plan_kernel(const int32_t* __restrict__ counts, int S1, long tiles, StepsWorkspace w) {
    __shared__ uint32_t s_part[PLAN_NT], s_wave[4];
    __shared__ int32_t s_counts[PT_MAX_S1], s_level[PT_MAX_S1];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, L = tid & 255;
    const bool owner = tid < 256;
    const long m = blockIdx.x;
    const uint16_t* hist = w.hist + m * tiles * 256;
    StepsPlan* plan = w.plan + m;
    uint32_t tot = 0u;
    long t = tid >> 8;
    for (; t + 28 < tiles; t += 32) {
        uint32_t v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = hist[(t + 4 * e) * 256 + L];
#pragma unroll
        for (int e = 0; e < 8; ++e) tot += v[e];
    }
    for (; t < tiles; t += 4) tot += hist[t * 256 + L];
    s_part[tid] = tot;
    if (tid < S1) s_counts[tid] = counts[tid];
    __syncthreads();
    tot = owner ? s_part[L] + s_part[256 + L] + s_part[512 + L] + s_part[768 + L] : 0u;
    const uint32_t inc = wave_scan_incl(tot);
    if (owner && lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int lo = 0, hi = 0;
    long start = 0;
    if (owner) {
        uint32_t upto = inc, all = 0u;  // the voxels of the levels 0 .. L, of all levels
        for (int q = 0; q < 4; ++q) {
            upto += q < wave ? s_wave[q] : 0u;
            all += s_wave[q];
        }
        start = (long)all - (long)upto;  // the voxels of the levels above
        lo = steps_at(s_counts, S1, start);
        hi = tot ? steps_at(s_counts, S1, start + tot - 1) : lo;
    }
    const bool straddles = lo != hi;  // a count lies strictly inside the level's voxels, and inside no other level's: at most S1 levels
    const unsigned long long ballot = __ballot(straddles);
    __syncthreads();  // s_wave has been read
    if (owner && lane == 0) s_wave[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    int nstr = 0;
    for (int q = 0; q < 4; ++q) nstr += (int)s_wave[q];
    if (owner) {
        int j = __popcll(ballot & ((1ull << lane) - 1ull));
        for (int q = 0; q < wave; ++q) j += (int)s_wave[q];
        if (straddles) {
            plan->table[L] = (uint8_t)(128 + j);
            plan->level[j] = L;
            plan->step0[j] = lo;
            plan->start[j] = (uint32_t)start;
            s_level[j] = L;
        } else {
            plan->table[L] = (uint8_t)lo;
        }
        if (tid == 0) plan->nstr = nstr;
    }
    __syncthreads();
    for (int q = wave; q < nstr; q += PLAN_NT / 64) {  // exclusive prefix of level q's counts over the tiles; bit 31: the tile holds the level
        const int lv = s_level[q];
        uint32_t* prefix = w.prefix + m * tiles * PT_MAX_S1 + q;
        uint32_t before = 0u;
        for (long t0 = 0; t0 < tiles; t0 += 64) {
            const long tt = t0 + lane;
            const uint32_t h = tt < tiles ? hist[tt * 256 + lv] : 0u;
            const uint32_t in = wave_scan_incl(h);
            if (tt < tiles) prefix[tt * PT_MAX_S1] = (before + in - h) | (h ? PT_PRESENT : 0u);
            before += __shfl(in, 63);
        }
    }
}

__global__ __launch_bounds__(PT_NT) void perturb_write_kernel(const uint8_t* __restrict__ maps, const int32_t* __restrict__ counts, long V,
                                                              int S1, long tiles, StepsWorkspace w, uint8_t* __restrict__ steps) {
    __shared__ uint8_t s_table[256];
    __shared__ int32_t s_counts[PT_MAX_S1], s_level[PT_MAX_S1], s_step0[PT_MAX_S1];
    __shared__ uint32_t s_start[PT_MAX_S1], s_prefix[PT_MAX_S1], s_wave[2][PT_NT / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long m = blockIdx.y, tile = blockIdx.x;
    const uint8_t* row = maps + m * V;
    const long vbeg = chunk_begin(row, (int)tile);
    const Chunk c = load_chunk(row, vbeg, V);
    const StepsPlan* plan = w.plan + m;
    const int nstr = min(plan->nstr, PT_MAX_S1);
    s_table[tid] = plan->table[tid];
    if (tid < S1) s_counts[tid] = counts[tid];
    if (tid < nstr) {
        s_level[tid] = plan->level[tid];
        s_step0[tid] = plan->step0[tid];
        s_start[tid] = plan->start[tid];
        s_prefix[tid] = w.prefix[(m * tiles + tile) * PT_MAX_S1 + tid];
    }
    __syncthreads();
    Chunk o = c;
    bool mine = false;  // a voxel of a straddling level in this chunk
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const unsigned t = s_table[c.byte(i)];
        o.set(i, t);
        mine |= c.has(i) && t >= 128u;
    }
    const bool wave_has = __ballot(mine) != 0ull;
    int buf = 0;
    for (int j = 0; j < nstr; ++j) {
        const uint32_t prefix = s_prefix[j];
        if (!(prefix & PT_PRESENT)) continue;  // the same in every thread
        const unsigned L = (unsigned)s_level[j];
        // matches in the lanes below (a ballot per byte position, counted by v_mbcnt), in the wave, and this chunk's own as a bit mask
        unsigned before = 0u, in_wave = 0u, own = 0u;
        if (wave_has) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const bool hit = c.has(i) && c.byte(i) == L;
                const unsigned long long b = __ballot(hit);
                before = __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, before));
                in_wave += (unsigned)__popcll(b);
                own |= hit ? 1u << i : 0u;
            }
        }
        if (lane == 0) s_wave[buf][wave] = in_wave;
        __syncthreads();  // (one barrier per level: the next level writes the other buffer)
        for (int q = 0; q < wave; ++q) before += s_wave[buf][q];
        buf ^= 1;
        if (own) {
            // the level's first voxel has step st; the counts it straddles are counts[st], counts[st + 1], ...: nearly always one
            const int st = s_step0[j];
            const long c0 = st < S1 ? (long)s_counts[st] : PT_MAX_V + 1, c1 = st + 1 < S1 ? (long)s_counts[st + 1] : PT_MAX_V + 1;
            long pos = (long)s_start[j] + (prefix & ~PT_PRESENT) + before;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if ((own >> i) & 1u) {
                    int sv = st;
                    if (pos >= c0) {
                        sv = st + 1;
                        if (pos >= c1) {
                            sv = st + 2;
                            while (sv < S1 && (long)s_counts[sv] <= pos) ++sv;
                        }
                    }
                    o.set(i, (unsigned)sv);
                    ++pos;
                }
            }
        }
    }
    store_chunk(steps + m * V, vbeg, V, o);
}

// ---- the perturbed clips -----------------------------------------------------------------------------------------------------------------
struct ApplyArgs {
    const void *x, *baseline;
    const uint8_t* steps;
    const int32_t* step_ids;
    void* out;
    long V;
    int C, k, Sc, mode;
    uint32_t fill;  // the bit pattern of the scalar baseline in the clip's dtype
};

// eight mask bytes (0xff: the element comes from x) from LDS byte offset idx on
__device__ __forceinline__ void mask_words(const uint32_t* s_mask, long idx, uint32_t& m0, uint32_t& m1) {
    const int wd = (int)(idx >> 2);
    const unsigned r = (unsigned)(idx & 3);
    const uint32_t a = s_mask[wd], b = s_mask[wd + 1], c = s_mask[wd + 2];
    m0 = __builtin_amdgcn_alignbyte(b, a, r);
    m1 = __builtin_amdgcn_alignbyte(c, b, r);
}

// U: the element as raw bits (uint32_t: fp32, uint16_t: bf16): the copy is bitwise
template <typename U>
__global__ __launch_bounds__(PT_NT) void perturb_apply_kernel(ApplyArgs a) {
    constexpr int EPV = 16 / (int)sizeof(U);
    __shared__ uint4 s_mask4[PT_NT + 1];  // PT_TILE mask bytes + the words mask_words reads past the last one
    const uint32_t* s_mask = reinterpret_cast<const uint32_t*>(s_mask4);
    const int tid = threadIdx.x;
    const long nj = blockIdx.z, sc = blockIdx.y, n = nj / a.k, V = a.V;
    const uint8_t* srow = a.steps + nj * V;
    const long t0 = (long)blockIdx.x * PT_TILE - (long)((uintptr_t)srow & 15), t1 = min(t0 + PT_TILE, V), lo = max(t0, 0L);
    {
        const int s = a.step_ids[sc];
        const Chunk c = load_chunk(srow, t0 + 16L * tid, V);
        Chunk mk = c;
#pragma unroll
        for (int i = 0; i < 16; ++i) mk.set(i, (((int)c.byte(i) <= s) == (a.mode == 1)) ? 0xffu : 0u);
        s_mask4[tid] = make_uint4(mk.w[0], mk.w[1], mk.w[2], mk.w[3]);
        if (tid == 0) s_mask4[PT_NT] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    if (lo >= t1) return;  // a tile past the row (the grid covers the worst misalignment)
    const U fill = (U)a.fill;
    for (int ch = 0; ch < a.C; ++ch) {
        const U* xr = static_cast<const U*>(a.x) + (n * a.C + ch) * V;
        const U* br = a.baseline ? static_cast<const U*>(a.baseline) + (n * a.C + ch) * V : nullptr;
        U* orow = static_cast<U*>(a.out) + ((nj * a.Sc + sc) * a.C + ch) * V;
        const long va = min(lo + lead_to_16(orow + lo), t1), nvec = (t1 - va) / EPV, vt = va + nvec * EPV;
        const long nhead = va - lo, ntail = t1 - vt;  // fewer than EPV elements each
        if (tid < nhead + ntail) {
            const long v = tid < nhead ? lo + tid : vt + (tid - nhead);
            const bool from_x = reinterpret_cast<const uint8_t*>(s_mask)[v - t0] != 0;
            orow[v] = from_x ? xr[v] : (br ? br[v] : fill);
        }
        const bool aligned_in = ((((uintptr_t)(xr + va)) | (br ? (uintptr_t)(br + va) : (uintptr_t)0)) & 15) == 0;
        for (long i = tid; i < nvec; i += PT_NT) {
            const long v = va + i * EPV;
            uint32_t m0, m1;
            mask_words(s_mask, v - t0, m0, m1);
            uint4 xv, bv;
            if constexpr (sizeof(U) == 4) {
                const uint32_t f = a.fill;
                if (aligned_in) {
                    xv = *reinterpret_cast<const uint4*>(xr + v);
                    bv = br ? *reinterpret_cast<const uint4*>(br + v) : make_uint4(f, f, f, f);
                } else {
                    xv = make_uint4(xr[v], xr[v + 1], xr[v + 2], xr[v + 3]);
                    bv = br ? make_uint4(br[v], br[v + 1], br[v + 2], br[v + 3]) : make_uint4(f, f, f, f);
                }
                uint4 r;
                r.x = (m0 & 0xffu) ? xv.x : bv.x;
                r.y = (m0 & 0xff00u) ? xv.y : bv.y;
                r.z = (m0 & 0xff0000u) ? xv.z : bv.z;
                r.w = (m0 & 0xff000000u) ? xv.w : bv.w;
                *reinterpret_cast<uint4*>(orow + v) = r;
            } else {
                const uint32_t f = a.fill | (a.fill << 16);
                if (aligned_in) {
                    xv = *reinterpret_cast<const uint4*>(xr + v);
                    bv = br ? *reinterpret_cast<const uint4*>(br + v) : make_uint4(f, f, f, f);
                } else {
                    const auto pair = [](const U* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 16); };
                    xv = make_uint4(pair(xr + v), pair(xr + v + 2), pair(xr + v + 4), pair(xr + v + 6));
                    bv = br ? make_uint4(pair(br + v), pair(br + v + 2), pair(br + v + 4), pair(br + v + 6)) : make_uint4(f, f, f, f);
                }
                // two mask bytes (0xff / 0) -> the 32-bit select of an element pair
                const auto sel = [](uint32_t two) { return (two & 0xffu) * 0x0101u | ((two >> 8) & 0xffu) * 0x01010000u; };
                const uint32_t k0 = sel(m0), k1 = sel(m0 >> 16), k2 = sel(m1), k3 = sel(m1 >> 16);
                uint4 r;
                r.x = (xv.x & k0) | (bv.x & ~k0);
                r.y = (xv.y & k1) | (bv.y & ~k1);
                r.z = (xv.z & k2) | (bv.z & ~k2);
                r.w = (xv.w & k3) | (bv.w & ~k3);
                *reinterpret_cast<uint4*>(orow + v) = r;
            }
        }
    }
}

// ---- the curves --------------------------------------------------------------------------------------------------------------------------
struct CurveArgs {
    const float *sim, *logits;
    const int32_t *sel, *cls, *counts;
    int N, k, S1, P, K, K_real;
    long V;
    float *curve_sim, *curve_prob;
    double *auc, *acc;
};

__global__ __launch_bounds__(PT_NT) void perturb_curves_kernel(CurveArgs a) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, k = a.k, S1 = a.S1;
    const long B = (long)a.N * k * S1;
    for (long b = tid; b < B; b += PT_NT) {
        const long q = b / S1, n = q / k;  // q = n k + j
        const int p = a.sel[q], c = a.cls[n];
        float cs = __builtin_nanf(""), cp = cs;
        if (p >= 0 && p < a.P && c >= 0 && c < a.K_real) {
            const float* lg = a.logits + b * a.K;
            float mx;
            const float s = softmax_max_sum_f32(lg, a.K_real, &mx);
            cs = a.sim[b * a.P + p];
            cp = __fdiv_rn(expf(lg[c] - mx), s);
        }
        a.curve_sim[b] = cs;
        a.curve_prob[b] = cp;
    }
    __threadfence_block();
    __syncthreads();
    const double Vd = (double)a.V;
    for (long e = tid; e < (long)a.N * k * 2; e += PT_NT) {
        const float* y = ((e & 1) ? a.curve_prob : a.curve_sim) + (e >> 1) * S1;
        double area = 0.0;
        for (int s = 1; s < S1; ++s) {
            const double dx = (double)a.counts[s] / Vd - (double)a.counts[s - 1] / Vd;
            area += dx * ((double)y[s] + (double)y[s - 1]) / 2.0;
        }
        a.auc[e] = area;
    }
    if (!a.acc) return;
    __threadfence_block();
    __syncthreads();
    const int nc = k * S1;  // acc = [similarity curves (k, S1), probability curves (k, S1), areas (k, 2), N]
    sweep_acc_add<PT_NT>(a.acc, 2 * nc + 2 * k + 1, a.N, [&](long n, int e) {
        if (e < nc) return (double)a.curve_sim[n * nc + e];
        if (e < 2 * nc) return (double)a.curve_prob[n * nc + (e - nc)];
        return a.auc[n * 2 * k + (e - 2 * nc)];
    });
}

static bool steps_sizes_ok(long M, long V, int S1) { return M >= 1 && M <= PT_MAX_MAPS && V >= 1 && V <= PT_MAX_V && S1 >= 1 && S1 <= PT_MAX_S1; }

// fp32 -> bf16 bits, to nearest even (NaN stays a quiet NaN)
static uint32_t bf16_bits_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return bf16_round_bits(u);
}

}  // namespace pasn

using namespace pasn;

extern "C" size_t pasn_perturb_steps_workspace_bytes(long M, long V, int S1) {
    if (!steps_sizes_ok(M, V, S1)) return 0;
    return steps_workspace(nullptr, M, perturb_tiles(V)).bytes;
}

extern "C" int pasn_perturb_steps(const uint8_t* maps, const int32_t* counts, long M, long V, int S1, uint8_t* steps, void* workspace,
                                  void* stream) {
    PASN_REQUIRE(maps && counts && steps, "maps, counts and steps are required");
    PASN_REQUIRE(workspace, "workspace is required");
    PASN_REQUIRE(M >= 1 && M <= PT_MAX_MAPS, "M must lie in [1, 65535]");
    PASN_REQUIRE(V >= 1 && V <= PT_MAX_V, "V must lie in [1, 2^31)");
    PASN_REQUIRE(S1 >= 1 && S1 <= PT_MAX_S1, "S1 must lie in [1, 64]");
    PASN_REQUIRE((((uintptr_t)maps | (uintptr_t)steps | (uintptr_t)workspace) & 15) == 0, "misaligned maps, steps or workspace");
    hipStream_t s = (hipStream_t)stream;
    const long tiles = perturb_tiles(V);
    const StepsWorkspace w = steps_workspace(workspace, M, tiles);
    const dim3 grid((unsigned)tiles, (unsigned)M);
    hipLaunchKernelGGL(perturb_hist_kernel, grid, dim3(PT_NT), 0, s, maps, V, tiles, w.hist);
    hipLaunchKernelGGL(perturb_plan_kernel, dim3((unsigned)M), dim3(PLAN_NT), 0, s, counts, S1, tiles, w);
    hipLaunchKernelGGL(perturb_write_kernel, grid, dim3(PT_NT), 0, s, maps, counts, V, S1, tiles, w, steps);
    return check_launch("perturb_steps");
}

extern "C" int pasn_perturb_apply(const void* x, const uint8_t* steps, const int32_t* step_ids, const void* baseline, float fill, int N, int C,
                                  int k, long V, int Sc, int mode, int dtype, void* out, void* stream) {
    PASN_REQUIRE(x && steps && step_ids && out, "x, steps, step_ids and out are required");
    PASN_REQUIRE(dtype == PASN_F32 || dtype == PASN_BF16, "dtype must be PASN_F32 or PASN_BF16");
    PASN_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (deletion) or 1 (insertion)");
    PASN_REQUIRE(N >= 1 && k >= 1 && (long)N * k <= PT_MAX_MAPS, "N k must lie in [1, 65535]");
    PASN_REQUIRE(Sc >= 1 && Sc <= 65535, "Sc must lie in [1, 65535]");
    PASN_REQUIRE(C >= 1 && C <= PT_MAX_C, "C must lie in [1, 64]");
    PASN_REQUIRE(V >= 1 && V <= PT_MAX_V, "V must lie in [1, 2^31)");
    const uintptr_t esz = dtype == PASN_BF16 ? 2 : 4;
    PASN_REQUIRE((((uintptr_t)x | (uintptr_t)baseline | (uintptr_t)out) & (esz - 1)) == 0, "x, baseline and out must be aligned to their element");
    ApplyArgs a{x, baseline, steps, step_ids, out, V, C, k, Sc, mode, 0u};
    if (dtype == PASN_BF16) a.fill = bf16_bits_rne(fill);
    else memcpy(&a.fill, &fill, 4);
    const dim3 grid((unsigned)((V + 15 + PT_TILE - 1) / PT_TILE), (unsigned)Sc, (unsigned)(N * k));
    if (dtype == PASN_BF16) hipLaunchKernelGGL(perturb_apply_kernel<uint16_t>, grid, dim3(PT_NT), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(perturb_apply_kernel<uint32_t>, grid, dim3(PT_NT), 0, (hipStream_t)stream, a);
    return check_launch("perturb_apply");
}

extern "C" int pasn_perturb_curves(const float* sim, const float* logits, const int32_t* sel, const int32_t* cls, const int32_t* counts, int N,
                                   int k, int S1, int P, int K, int K_real, long V, float* curve_sim, float* curve_prob, double* auc,
                                   double* acc, void* stream) {
    PASN_REQUIRE(sim && logits && sel && cls && counts, "sim, logits, sel, cls and counts are required");
    PASN_REQUIRE(curve_sim && curve_prob && auc, "curve_sim, curve_prob and auc are required");
    PASN_REQUIRE(S1 >= 1 && S1 <= PT_MAX_S1, "S1 must lie in [1, 64]");
    PASN_REQUIRE(N >= 1 && k >= 1 && (long)N * k * S1 <= PT_MAX_CURVE_ROWS, "N k S1 must lie in [1, 2^20]");
    PASN_REQUIRE(K_real >= 1 && K_real <= EVAL_MAX_K, "K_real must lie in [1, 16]");
    PASN_REQUIRE(K >= K_real && K <= 17, "K must lie in [K_real, 17]");
    PASN_REQUIRE(P >= 1, "P must be positive");
    PASN_REQUIRE(V >= 1 && V <= PT_MAX_V, "V must lie in [1, 2^31)");
    const CurveArgs a{sim, logits, sel, cls, counts, N, k, S1, P, K, K_real, V, curve_sim, curve_prob, auc, acc};
    hipLaunchKernelGGL(perturb_curves_kernel, dim3(1), dim3(PT_NT), 0, (hipStream_t)stream, a);
    return check_launch("perturb_curves");
}
