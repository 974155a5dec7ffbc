// Global explanations: per prototype the k nearest clips of a split, their payload rows and the per-class similarity sums, all kept on
// the device while a loader is swept (the reference saves the whole (clips, P) similarity matrix for the host to rank,
// XProtoNet_Base.py:613-656; the per-batch selection rule is the push's, push_abs_revision.py:288-307).
#include "common.h"

namespace pasn {

// (distance, global index) ascending; the index compares UNSIGNED so that the empty entry (+inf, -1) sorts after a clip at +inf
__device__ __forceinline__ bool topk_less(float da, int64_t ia, float db, int64_t ib) {
    return da < db || (da == db && (uint64_t)ia < (uint64_t)ib);
}

// One wave per prototype, row entry e in lane e (lanes >= k idle).  The batch is walked 64 clips at a time; a ballot keeps the clips
// that beat the row's current k-th entry, and each survivor (ascending clip index) is inserted by compare + shift: the lanes behind its
// position take their left neighbour's entry, the evicted last entry's payload slot goes to the newcomer.
__global__ __launch_bounds__(64) void topk_xproto_kernel(const float* __restrict__ proto_dist, const int64_t* __restrict__ labels,
                                                         const int32_t* __restrict__ proto_class, const int32_t* __restrict__ class_mask,
                                                         float* __restrict__ top_dist, int64_t* __restrict__ top_index,
                                                         int32_t* __restrict__ top_slot, int B, int P, int k, int64_t index_base) {
    const int j = blockIdx.x;
    const int lane = threadIdx.x;
    const bool masked = class_mask[j] != 0;
    const int64_t cls = proto_class[j];
    const bool mine = lane < k;
    const long at = (long)j * k + lane;
    float rd = mine ? top_dist[at] : INFINITY;
    int64_t ri = mine ? top_index[at] : -1;
    int rs = mine ? top_slot[at] : 0;
    float kd = __shfl(rd, k - 1);
    int64_t ki = __shfl(ri, k - 1);
    bool dirty = false;
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int b = b0 + lane;
        float cd = INFINITY;
        const int64_t ci = index_base + b;
        bool pass = false;
        if (b < B && !(masked && labels[b] != cls)) {
            cd = proto_dist[(long)b * P + j];
            pass = topk_less(cd, ci, kd, ki);
        }
        unsigned long long todo = __ballot(pass);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const float nd = __shfl(cd, src);
            const int64_t ni = __shfl(ci, src);
            if (!topk_less(nd, ni, kd, ki)) continue;  // the k-th entry has tightened since the ballot
            const int pos = __popcll(__ballot(mine && topk_less(rd, ri, nd, ni)));  // entries that stay in front (the row is sorted)
            const int evicted = __shfl(rs, k - 1);
            const float ld = __shfl_up(rd, 1);
            const int64_t li = __shfl_up(ri, 1);
            const int ls = __shfl_up(rs, 1);
            if (mine && lane > pos) {
                rd = ld;
                ri = li;
                rs = ls;
            } else if (lane == pos) {  // pos < k: the newcomer beats entry k - 1
                rd = nd;
                ri = ni;
                rs = evicted;
            }
            kd = __shfl(rd, k - 1);
            ki = __shfl(ri, k - 1);
            dirty = true;
        }
    }
    if (dirty && mine) {
        top_dist[at] = rd;
        top_index[at] = ri;
        top_slot[at] = rs;
    }
}

// One wave per row entry (j, e), four per block; V = the widest word the row size and both base addresses allow.
template <typename V>
__global__ __launch_bounds__(256) void topk_gather_kernel(const int64_t* __restrict__ top_index, const int32_t* __restrict__ top_slot,
                                                          const V* __restrict__ payload, V* __restrict__ store, int B, int P, int k,
                                                          long row_words, int per_proto, int64_t index_base) {
    const long entry = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (entry >= (long)P * k) return;
    const int lane = threadIdx.x & 63;
    const int64_t g = top_index[entry];
    if (g < index_base || g >= index_base + B) return;
    const int slot = top_slot[entry];
    if (slot < 0 || slot >= k) return;  // a state the caller did not initialise: nothing is written out of the store
    const long j = entry / k;
    const long b = (long)(g - index_base);
    const V* src = payload + (per_proto ? b * P + j : b) * row_words;
    V* dst = store + (j * k + slot) * row_words;
    for (long w = lane; w < row_words; w += 64) dst[w] = src[w];
}

// One thread per prototype; per class the batch's rows are added in index order onto the running fp64 sum (bitwise reproducible).
// The first K threads of the grid also count the rows per label.
__global__ __launch_bounds__(64) void proto_class_stats_kernel(const float* __restrict__ proto_dist, const int64_t* __restrict__ labels,
                                                               int B, int P, int K, double* __restrict__ class_sim_sum,
                                                               int64_t* __restrict__ class_count) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p < K) {
        int64_t n = 0;
        for (int b = 0; b < B; ++b) n += labels[b] == (int64_t)p;
        class_count[p] += n;
    }
    if (p >= P) return;
    for (int c = 0; c < K; ++c) {
        double acc = class_sim_sum[(long)p * K + c];
        for (int b = 0; b < B; ++b)
            if (labels[b] == (int64_t)c) acc += (double)(1.0f - proto_dist[(long)b * P + p]);
        class_sim_sum[(long)p * K + c] = acc;
    }
}

}  // namespace pasn

using namespace pasn;

extern "C" int pasn_topk_xproto_update(const float* proto_dist, const int64_t* labels, const int32_t* proto_class,
                                       const int32_t* class_mask, float* top_dist, int64_t* top_index, int32_t* top_slot, int B, int P,
                                       int k, int64_t index_base, void* stream) {
    PASN_REQUIRE(proto_dist && labels && proto_class && class_mask, "null pointer");
    PASN_REQUIRE(top_dist && top_index && top_slot, "null state");
    PASN_REQUIRE(k >= 1 && k <= 64, "k must lie in [1, 64] (one row entry per lane; there is no slow path)");
    PASN_REQUIRE(P >= 1 && P <= 4096, "P must lie in [1, 4096]");
    PASN_REQUIRE(B >= 1 && index_base >= 0, "empty batch or negative index base");
    hipLaunchKernelGGL(topk_xproto_kernel, dim3(P), dim3(64), 0, (hipStream_t)stream, proto_dist, labels, proto_class, class_mask,
                       top_dist, top_index, top_slot, B, P, k, index_base);
    return check_launch("topk_xproto_kernel");
}

template <typename V>
static int launch_gather(const int64_t* top_index, const int32_t* top_slot, const void* payload, void* store, int B, int P, int k,
                         long row_bytes, int per_proto, int64_t index_base, hipStream_t s) {
    hipLaunchKernelGGL((topk_gather_kernel<V>), dim3(ceil_div((long)P * k, 4)), dim3(256), 0, s, top_index, top_slot, (const V*)payload,
                       (V*)store, B, P, k, row_bytes / (long)sizeof(V), per_proto, index_base);
    return check_launch("topk_gather_kernel");
}

extern "C" int pasn_topk_gather(const int64_t* top_index, const int32_t* top_slot, const void* payload, void* store, int B, int P,
                                int k, long row_elems, int elem_bytes, int per_proto, int64_t index_base, void* stream) {
    PASN_REQUIRE(top_index && top_slot, "null state");
    PASN_REQUIRE(payload && store, "null pointer");
    PASN_REQUIRE(k >= 1 && k <= 64, "k must lie in [1, 64]");
    PASN_REQUIRE(P >= 1 && P <= 4096, "P must lie in [1, 4096]");
    PASN_REQUIRE(B >= 1 && index_base >= 0, "empty batch or negative index base");
    PASN_REQUIRE(row_elems >= 1, "empty payload row");
    PASN_REQUIRE(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8, "elem_bytes must be 1, 2, 4 or 8");
    const long row_bytes = row_elems * elem_bytes;
    const uintptr_t bits = (uintptr_t)payload | (uintptr_t)store | (uintptr_t)row_bytes;
    PASN_REQUIRE(bits % elem_bytes == 0, "payload / store not aligned to their element size");
    hipStream_t s = (hipStream_t)stream;
    if (bits % 16 == 0) return launch_gather<uint4>(top_index, top_slot, payload, store, B, P, k, row_bytes, per_proto, index_base, s);
    if (bits % 8 == 0) return launch_gather<uint2>(top_index, top_slot, payload, store, B, P, k, row_bytes, per_proto, index_base, s);
    if (bits % 4 == 0) return launch_gather<uint32_t>(top_index, top_slot, payload, store, B, P, k, row_bytes, per_proto, index_base, s);
    if (bits % 2 == 0) return launch_gather<uint16_t>(top_index, top_slot, payload, store, B, P, k, row_bytes, per_proto, index_base, s);
    return launch_gather<uint8_t>(top_index, top_slot, payload, store, B, P, k, row_bytes, per_proto, index_base, s);
}

extern "C" int pasn_proto_class_stats(const float* proto_dist, const int64_t* labels, int B, int P, int K, double* class_sim_sum,
                                      int64_t* class_count, void* stream) {
    PASN_REQUIRE(proto_dist && labels, "null pointer");
    PASN_REQUIRE(class_sim_sum && class_count, "null state");
    PASN_REQUIRE(K >= 1 && K <= 64, "K must lie in [1, 64]");
    PASN_REQUIRE(P >= 1 && P <= 4096, "P must lie in [1, 4096]");
    PASN_REQUIRE(B >= 1, "empty batch");
    const int threads = P > K ? P : K;
    hipLaunchKernelGGL(proto_class_stats_kernel, dim3(ceil_div(threads, 64)), dim3(64), 0, (hipStream_t)stream, proto_dist, labels, B, P,
                       K, class_sim_sum, class_count);
    return check_launch("proto_class_stats_kernel");
}
