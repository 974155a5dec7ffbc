// Rank by counting: the ONE copy selective.hip and bootstrap.hip share (eval_metrics.hip's AUC takes the geometry).  A float maps to a
// uint32 key that orders as the floats do; the rank of row i is the number of rows j whose key is smaller, or equal with j < i, counted
// out of LDS tiles of 256 keys.  Grid: blockIdx.x = 256 rows i (one per thread), blockIdx.y = a chunk of rows j.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pasn {

constexpr int RANK_TILE = 256;
constexpr uint32_t RC_KEY_NAN = 0xFFFFFFFEu, RC_KEY_PAD = 0xFFFFFFFFu;

// a uint32 that orders as the floats do: -0 and +0 share a key, NaN lies above +inf (0xFF800000) and padding above NaN
__device__ __forceinline__ uint32_t rc_key(float v) {
    if (v != v) return RC_KEY_NAN;
    const uint32_t b = v == 0.0f ? 0u : __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

struct RankGeom {
    int gx, gy, chunk;  // row blocks, row-j chunks and their length (a multiple of the tile)
};

static inline RankGeom rank_geom(long M) {
    RankGeom g;
    g.gx = (int)((M + RANK_TILE - 1) / RANK_TILE);
    const long per = (M + 63) / 64, c = per > 1024 ? per : 1024;  // at most 64 chunks of >= 1024 rows
    g.chunk = (int)(((c + RANK_TILE - 1) / RANK_TILE) * RANK_TILE);
    g.gy = (int)((M + g.chunk - 1) / g.chunk);
    return g;
}

// The rows of one staged tile (s_key, 16-byte aligned, RANK_TILE keys of the rows jt .. jt + 255) that come before row i0 + tid with key
// ki.  Tiles are aligned to the 256 rows of a block, so every tile but the block's own lies wholly before or behind its rows and needs
// ONE comparison per pair (<= or <).
__device__ __forceinline__ int rank_count_tile(const uint32_t* s_key, uint32_t ki, long jt, long i0, int tid) {
    const uint4* s4 = reinterpret_cast<const uint4*>(s_key);
    int cnt = 0;
    if (jt < i0) {  // every j of the tile lies before i: equal keys come first
#pragma unroll 8
        for (int t = 0; t < RANK_TILE / 4; ++t) {
            const uint4 k4 = s4[t];
            cnt += (k4.x <= ki) + (k4.y <= ki) + (k4.z <= ki) + (k4.w <= ki);
        }
    } else if (jt > i0) {
#pragma unroll 8
        for (int t = 0; t < RANK_TILE / 4; ++t) {
            const uint4 k4 = s4[t];
            cnt += (k4.x < ki) + (k4.y < ki) + (k4.z < ki) + (k4.w < ki);
        }
    } else {  // the block's own rows
        for (int t = 0; t < RANK_TILE; ++t) {
            const uint32_t kj = s_key[t];
            cnt += (kj < ki) || (kj == ki && t < tid);
        }
    }
    return cnt;
}

// The rank pass of one block: the rows of chunk blockIdx.y (of M rows) that come before row blockIdx.x * 256 + tid with key ki.  key(j)
// is row j's key, RC_KEY_PAD for a row that never enters; a thread whose own ki is RC_KEY_PAD counts nothing but still stages its key
// and reaches both barriers of every tile.  The tail of a short tile is padding: it counts for nobody.
template <typename Key>
__device__ __forceinline__ int rank_count_chunk(Key key, uint32_t ki, long M, int chunk) {
    __shared__ __attribute__((aligned(16))) uint32_t s_key[RANK_TILE];
    const int tid = threadIdx.x;
    const long i0 = (long)blockIdx.x * RANK_TILE, j0 = (long)blockIdx.y * chunk, j1 = min(M, j0 + (long)chunk);
    int cnt = 0;
    for (long jt = j0; jt < j1; jt += RANK_TILE) {
        __syncthreads();
        const long j = jt + tid;
        s_key[tid] = j < j1 ? key(j) : RC_KEY_PAD;
        __syncthreads();
        if (ki != RC_KEY_PAD) cnt += rank_count_tile(s_key, ki, jt, i0, tid);
    }
    return cnt;
}

}  // namespace pasn
