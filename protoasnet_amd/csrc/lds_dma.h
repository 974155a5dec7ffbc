// The vocabulary of the kernels that stage through LDS-DMA (`buffer_load ... lds`) and range-checked buffer accesses: one definition each of the
// LDS pointer type, the small vector types, the buffer descriptor, the out-of-range offset tag, the fence-free barrier, the counted wait and
// the bf16 bit pattern of a float.  Included by common.h.
#pragma once

namespace pasn {

typedef __attribute__((address_space(3))) void* lds_ptr_t;           // what `buffer_load ... lds` takes as its destination
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) short s16x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;
// (bf16x2, f32x2: common.h)

// Per-lane offset tag of a masked lane.  The range check of a raw buffer access compares offset (+ soffset) with num_records; every
// descriptor that is addressed with this tag describes fewer than 2^31 bytes (the launch code checks it), so the tag lies beyond every
// num_records whatever a soffset below 2^31 adds to it: a load returns zeros (an LDS-DMA writes zeros), a store is dropped.  Masked lanes
// issue the instruction all the same, which is what lets a wave COUNT its memory operations (wait_vmcnt_all_but).  (igemm.hip and
// igemm_halo.hip describe whole tensors of up to 2^32 - 32 bytes and tag with 0xfffffff0 instead.)
constexpr unsigned BUF_OOB = 0x80000000u;

// Raw buffer descriptor of `bytes` bytes at p: stride 0, num_records = bytes.  The flags word is gfx9's DATA_FORMAT = 4, the 32-bit format (bits 15 .. 18
// of dword 3: what raw untyped accesses expect), with everything else zero: no swizzle, no index stride, ADD_TID off -- the range check is the
// plain `offset >= num_records`.
template <typename T>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const T* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(p), 0, bytes, 0x00020000);
}

// Block barrier WITHOUT the fence of __syncthreads().  That fence is `s_waitcnt vmcnt(0) lgkmcnt(0)`: it would drain the LDS-DMA groups
// requested for the next steps and the output stores at every barrier and serialise the ring.  Here only LDS / scalar traffic is drained;
// what must have landed from memory is waited for by count (wait_vmcnt_all_but) or by an explicit vmcnt(0) just before.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Waits until all but this wave's n most recent vector-memory operations are done (n wave-uniform): `s_waitcnt vmcnt(n)` with the
// immediate picked by a scalar switch, exact for n = 0 .. MAXN, the caller's bound.  ONE rule beyond it: any other n waits for everything,
// vmcnt(0) -- stricter than any n asks for, never weaker, whatever the caller's arithmetic did.  (vmcnt is a 6-bit counter on gfx9.)
template <int MAXN>
__device__ __forceinline__ void wait_vmcnt_all_but(int n) {
    static_assert(MAXN >= 0 && MAXN <= 63, "s_waitcnt vmcnt: 6 bits");
#define PASN_VMW(k) case k: if (k <= MAXN) { asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); return; } break;
    switch (n) {
        PASN_VMW(0) PASN_VMW(1) PASN_VMW(2) PASN_VMW(3) PASN_VMW(4) PASN_VMW(5) PASN_VMW(6) PASN_VMW(7) PASN_VMW(8) PASN_VMW(9) PASN_VMW(10)
        PASN_VMW(11) PASN_VMW(12) PASN_VMW(13) PASN_VMW(14) PASN_VMW(15) PASN_VMW(16) PASN_VMW(17) PASN_VMW(18) PASN_VMW(19) PASN_VMW(20)
        PASN_VMW(21) PASN_VMW(22) PASN_VMW(23) PASN_VMW(24) PASN_VMW(25) PASN_VMW(26) PASN_VMW(27) PASN_VMW(28) PASN_VMW(29) PASN_VMW(30)
        PASN_VMW(31) PASN_VMW(32) PASN_VMW(33) PASN_VMW(34) PASN_VMW(35) PASN_VMW(36) PASN_VMW(37) PASN_VMW(38) PASN_VMW(39) PASN_VMW(40)
        PASN_VMW(41) PASN_VMW(42) PASN_VMW(43) PASN_VMW(44) PASN_VMW(45) PASN_VMW(46) PASN_VMW(47) PASN_VMW(48) PASN_VMW(49) PASN_VMW(50)
        PASN_VMW(51) PASN_VMW(52) PASN_VMW(53) PASN_VMW(54) PASN_VMW(55) PASN_VMW(56) PASN_VMW(57) PASN_VMW(58) PASN_VMW(59) PASN_VMW(60)
        PASN_VMW(61) PASN_VMW(62) PASN_VMW(63)
        default: break;
    }
#undef PASN_VMW
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// bf16 bit pattern of a float, rounded to nearest even
__device__ __forceinline__ unsigned bf16_bits(float f) {
    const __bf16 b = (__bf16)f;
    return (unsigned)__builtin_bit_cast(unsigned short, b);
}

}  // namespace pasn
