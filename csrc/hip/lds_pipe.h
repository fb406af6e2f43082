// LDS-DMA (global_load_lds_dwordx4) and the waits that order an LDS ring,
// shared by the GEMM and attention kernels.
#pragma once
#include "common.h"

namespace nos {

// LDS-DMA of 16 bytes per lane: lane L's 16 bytes at g land at
// lds_wave_base + 16 L (one 1 KiB piece per wave instruction).  Two forms,
// which do not compile to the same code:
//
//  * glds16 / glds16_s, inline asm -- for rings that keep a later stage in
//    flight while the current one is read.  The compiler does not know the
//    instruction writes LDS, so it inserts no wait of its own; with the
//    builtin, hipcc assumes every ds_read may alias an in-flight LDS-DMA and
//    puts s_waitcnt vmcnt(0) before the first LDS read after the issue, which
//    drains the NEXT stage's loads before the CURRENT stage's fragment reads
//    (seen in the ISA: a full L2 / HBM round trip per K step or key tile).
//    The kernel orders the ring itself: wait_stages or dma_wait_publish before
//    the barrier that publishes a stage, and anything the DMA must not
//    overtake (Q loaded to registers before the first issue) waited for
//    explicitly.  m0 (the LDS address) is an operand ("{m0}"), so the
//    compiler writes it and knows it is live -- a clobbered m0 is undefined
//    behaviour, m0 being a reserved register -- and the s_nop is the
//    SALU-write-m0 -> LDS-DMA wait state the compiler cannot see.
//  * glds16_builtin -- the compiler tracks the DMA and places the vmcnt(0)
//    itself: gemm.hip, gemm_f32.hip and attention.hip were written and
//    measured with it and keep it.
__device__ __forceinline__ void glds16(const void* g, unsigned char* lds_wave_base) {
  const unsigned lds = __builtin_amdgcn_readfirstlane(
      (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds_wave_base);
  asm volatile("s_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "{m0}"(lds) : "memory");
}

// the asm form from a wave-uniform tile base (SGPR pair) plus a per-lane 32-bit
// byte offset: the steady-state tiles need no 64-bit VALU address arithmetic
__device__ __forceinline__ void glds16_s(const void* sbase, unsigned voff, unsigned char* lds_wave_base) {
  const unsigned lds = __builtin_amdgcn_readfirstlane(
      (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds_wave_base);
  asm volatile("s_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "{m0}"(lds) : "memory");
}

__device__ __forceinline__ void glds16_builtin(const void* g, unsigned char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// every DMA this wave issued has landed, then the workgroup barrier publishes them
__device__ __forceinline__ void dma_wait_publish() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// s_waitcnt vmcnt(n * LPS) for a runtime n in [0, 3] (LPS DMAs per wave and
// stage: n later stages stay in flight); the immediate must be a constant
template <int LPS>
__device__ __forceinline__ void wait_stages(int n) {
  if (n <= 0)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if (n == 1)
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPS) : "memory");
  else if (n == 2)
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPS) : "memory");
  else
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * LPS) : "memory");
}

}  // namespace nos
