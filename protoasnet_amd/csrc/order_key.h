// Rank by counting: the pieces selective.hip and bootstrap.hip share.  A float maps to a uint32 key that orders as the floats do; the rank
// of row i is the number of rows j whose key is smaller, or equal with j < i, counted out of LDS tiles of 256 keys.
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

}  // namespace pasn
