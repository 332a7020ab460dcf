// Device helpers shared by the BSR kernel files (kernels_bsr.hip, kernels_bsr_kron.hip): the
// vmcnt wait of an unrolled software pipeline, wave-uniform loads, LDS-DMA and the XCD-contiguous
// workgroup order.  Included by .hip files only.
#pragma once

#include <hip/hip_runtime.h>

namespace sbx {

/// The LDS address of a pointer into LDS (what m0 takes)
__device__ __forceinline__ unsigned lds_u32(const void *p) {
    return (unsigned)(size_t)(const __attribute__((address_space(3))) void *)p;
}

/// s_waitcnt vmcnt(n) for an n the unrolled caller knows at compile time (folds to one wait); a
/// count that is not listed waits for everything
__device__ __forceinline__ void wait_vmcnt(int n) {
    switch (n) {
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
    case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
    case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    case 15: asm volatile("s_waitcnt vmcnt(15)" ::: "memory"); break;
    case 18: asm volatile("s_waitcnt vmcnt(18)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
}

/// Wave-uniform element load through the constant address space (scalar loads into SGPRs)
template <typename R> using ConstPtr = const __attribute__((address_space(4))) R *;
template <typename E> struct Uniform {
    static __device__ __forceinline__ E load(const E *p, long i) {
        return ((ConstPtr<E>)p)[i];
    }
};
template <> struct Uniform<double2> {
    static __device__ __forceinline__ double2 load(const double2 *p, long i) {
        const ConstPtr<double> q = (ConstPtr<double>)p;
        return double2{q[2 * i], q[2 * i + 1]};
    }
};
template <> struct Uniform<float2> {
    static __device__ __forceinline__ float2 load(const float2 *p, long i) {
        const ConstPtr<float> q = (ConstPtr<float>)p;
        return float2{q[2 * i], q[2 * i + 1]};
    }
};

/// A binary16 element: scalar loads move whole dwords, and for a 2-byte element behind a pointer
/// that is only 2-byte aligned the compiler gives the scalar load up (global_load_ushort into a
/// VGPR per element).  Instead: the aligned dword that holds the element, then its low or high
/// half by the address's bit 1 -- right for an odd index and for a base that is 2 mod 4.  The
/// other half of that dword may lie just outside the array (its first element at 2 mod 4, or its
/// last at 0 mod 4); an aligned dword never crosses a page or an allocation granule, and that
/// half is dropped.  (A pair of binary16, 4-byte aligned, is one s_load_dword by the generic form.)
template <> struct Uniform<_Float16> {
    static __device__ __forceinline__ _Float16 load(const _Float16 *p, long i) {
        const size_t a = (size_t)(p + i);
        const unsigned w = *(ConstPtr<unsigned>)(a & ~(size_t)3);
        const unsigned short h = (unsigned short)((a & 2) ? w >> 16 : w);
        _Float16 r;
        __builtin_memcpy(&r, &h, 2);
        return r;
    }
};

// LDS-DMA: a lane's 16 (dma4: 4) bytes at buffer offset `off` of `rs` go to LDS address dst +
// 16 (4) * lane; dst is wave-uniform (m0), an offset past the buffer writes zeros.
// Inline asm: hipcc does not order its ds_reads against an LDS-DMA it cannot see; the kernel
// retires the DMA with an explicit vmcnt wait before its barrier or its reads.  nt (a uniform
// kernel argument, so a scalar branch): the streaming policy for data read once (the values).
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rs, unsigned off, unsigned dst, int nt = 0) {
    const unsigned m0 = __builtin_amdgcn_readfirstlane(dst);
    if (nt)
        asm volatile("s_mov_b32 m0, %1\n\t"
                     "s_nop 0\n\t"
                     "buffer_load_dwordx4 %0, %2, 0 offen nt lds"
                     :
                     : "v"(off), "s"(m0), "s"(rs)
                     : "memory", "m0");
    else
        asm volatile("s_mov_b32 m0, %1\n\t"
                     "s_nop 0\n\t"
                     "buffer_load_dwordx4 %0, %2, 0 offen lds"
                     :
                     : "v"(off), "s"(m0), "s"(rs)
                     : "memory", "m0");
}
__device__ __forceinline__ void dma4(__amdgpu_buffer_rsrc_t rs, unsigned off, unsigned dst) {
    asm volatile("s_mov_b32 m0, %1\n\t"
                 "s_nop 0\n\t"
                 "buffer_load_dword %0, %2, 0 offen lds"
                 :
                 : "v"(off), "s"(__builtin_amdgcn_readfirstlane(dst)), "s"(rs)
                 : "memory", "m0");
}
/// ... the lane's 16 bytes named by a 64-bit address (no buffer, so no bound: the caller's)
__device__ __forceinline__ void dma16_lane(const void *src, unsigned dst, bool nt) {
    const unsigned m0 = __builtin_amdgcn_readfirstlane(dst);
    if (nt)
        asm volatile("s_mov_b32 m0, %1\n\t"
                     "s_nop 0\n\t"
                     "global_load_lds_dwordx4 %0, off nt"
                     :
                     : "v"(src), "s"(m0)
                     : "memory", "m0");
    else
        asm volatile("s_mov_b32 m0, %1\n\t"
                     "s_nop 0\n\t"
                     "global_load_lds_dwordx4 %0, off"
                     :
                     : "v"(src), "s"(m0)
                     : "memory", "m0");
}

/// The hardware deals workgroups round robin over the 8 XCDs.  Workgroup `bid` of `nwg` -> its
/// position in the order that gives every XCD one contiguous range of positions, so that
/// neighbouring positions (chunks of block rows) share lines in that XCD's L2.  ilv > 1: the
/// XCD's range is visited as ilv interleaved parts (with 2: its two halves together; the
/// remainder of a range that ilv does not divide keeps its place).
__device__ __forceinline__ int xcd_chunk(int bid, int nwg, int ilv = 1) {
    const int xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
    const int cnt = xcd < r8 ? q8 + 1 : q8, q = bid >> 3, npart = cnt / ilv;
    const int loc = (ilv > 1 && q < npart * ilv) ? (q % ilv) * npart + q / ilv : q;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + loc;
}

} // namespace sbx
