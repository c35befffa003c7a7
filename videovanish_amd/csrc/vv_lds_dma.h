// LDS-DMA (global_load_lds_dwordx4) and the transposed LDS read: the one definition for every kernel that fills LDS tiles without staging registers
// (vv_gemm.hip, vv_gemm256.hip, the attention kernels through vv_attn_common.h, the slab-streaming fused kernels through vv_fused_common.h).
#pragma once
#include "vv_common.h"

// one 16-byte LDS-DMA per lane: 1 KB per wave from gptr (per lane) to lds_wave_base + 16 lane.  The compiler sees the LDS write: it keeps the ds_reads
// of the target ordered behind it by itself, with a conservative vmcnt(0) wherever it cannot tell the buffers apart (distinct __shared__ objects help)
__device__ __forceinline__ void glds16(const void* gptr, void* lds_wave_base) {
    typedef const void __attribute__((address_space(1))) * gp_t;
    typedef void __attribute__((address_space(3))) * lp_t;
    __builtin_amdgcn_global_load_lds((gp_t)gptr, (lp_t)lds_wave_base, 16, 0, 0);
}

// the same copy issued from inline asm: hipcc does not see the LDS write and inserts no wait of its own, every wait is the caller's hand-placed counted one.
// M0 = wave-uniform LDS destination, written in the same statement that reads it and restored behind it (cdna_hip_programming.md 5.7)
__device__ __forceinline__ void glds16_asm(const void* gptr, void* lds_wave_base) {
    typedef void __attribute__((address_space(3))) * lp_t;
    const unsigned dst = (unsigned)(size_t)(lp_t)lds_wave_base;
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gptr), "s"(dst) : "memory");
}

// ds_read_b64_tr_b16: the hardware-transposed read of a row-major h16 tile (the A operand V^T of the attention kernels)
__device__ __forceinline__ uint2 ds_read_tr16(const unsigned char* lds_ptr) {
    typedef s16x4 __attribute__((address_space(3))) * lds_s16x4_p;
    s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)lds_ptr);
    return __builtin_bit_cast(uint2, v);
}
