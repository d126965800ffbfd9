// The primitives every hand-scheduled kernel of this library is built from: LDS addresses, the LDS-DMA issue forms, the asm-hidden global
// load, the scheduling-tight barrier, the 16-bit pack and the compile-time loop.  One copy each; like fsvit_common.h the header lives in
// FSVIT_NS, so the bf16 and the -DFSVIT_HALF_F16 build of a source get their own instances.
//
// LDS-DMA (global_load_lds_dwordx4: 64 lanes x 16 bytes = 1 KiB per instruction, lane-linear at the LDS byte address in M0) is issued from
// inline asm so that hipcc's waitcnt pass does not see it: with the builtin, any ordinary global load in the loop made the pass plant
// `s_waitcnt vmcnt(0)` in front of the first ds_read of every k-step, i.e. drain the DMA right after issuing it.  Hidden from the pass, the
// DMAs are ordered by hand: LDS-DMA data is visible to a ds_read only after the ISSUING wave's counted vmcnt followed by a barrier the
// reader passes.  The compiler's own counted waits for its ordinary loads stay safe: extra operations in flight only make vmcnt(N)
// stricter.  M0 is saved, written and restored inside the statement that consumes it - once per statement, whatever the number of pieces.
#pragma once
#include <type_traits>
#include <utility>

#include "fsvit_common.h"

namespace FSVIT_NS {

typedef __attribute__((address_space(3))) void* lds_ptr_t;
__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(size_t)(lds_ptr_t)p; }

// pieces of an LDS-DMA statement: M0 := an LDS address operand; one 1 KiB piece with source = scalar base `s` + lane offset `v` (+ offset)
#define LDS_DMA_M0(m) "s_mov_b32 m0, " m "\n\ts_nop 0\n\t"
#define LDS_DMA_P(v, s, off) "global_load_lds_dwordx4 " v ", " s off "\n\t"
// 1 ... 4 consecutive pieces on one M0 value: the immediate offset moves the LDS destination together with the global source (tools/probes/
// ldsdma_offset.hip, measured on gfx950), so a linear copy needs no address arithmetic; the 13-bit offset field covers 4 pieces
#define LDS_DMA_P1(v, s) LDS_DMA_P(v, s, "")
#define LDS_DMA_P2(v, s) LDS_DMA_P1(v, s) LDS_DMA_P(v, s, " offset:1024")
#define LDS_DMA_P3(v, s) LDS_DMA_P2(v, s) LDS_DMA_P(v, s, " offset:2048")
#define LDS_DMA_P4(v, s) LDS_DMA_P3(v, s) LDS_DMA_P(v, s, " offset:3072")
#define LDS_DMA_BEGIN "s_mov_b32 %0, m0\n\t"
#define LDS_DMA_END "s_mov_b32 m0, %0"

// One piece, per-lane 64-bit source.
__device__ __forceinline__ void dma1_lane(const void* gsrc, unsigned lds) {
  unsigned keep;
  asm volatile(LDS_DMA_BEGIN LDS_DMA_M0("%2") LDS_DMA_P1("%1", "off") LDS_DMA_END : "=&s"(keep) : "v"(gsrc), "s"(lds) : "memory");
}
// One piece, scalar base + per-lane 32-bit byte offset.  A VMEM instruction of 64 x 16 bytes keeps the wave's issue stage for ~64 cycles;
// back to back they queue behind each other and hold up the MFMAs that follow, so inside an MFMA loop a refill goes out one piece at a time.
__device__ __forceinline__ void dma1(unsigned voff, const void* sbase, unsigned lds) {
  unsigned keep;
  asm volatile(LDS_DMA_BEGIN LDS_DMA_M0("%3") LDS_DMA_P1("%1", "%2") LDS_DMA_END : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds) : "memory");
}
// Two pieces on one scalar base: two lane offsets, two M0 values.
__device__ __forceinline__ void dma2(unsigned off0, unsigned off1, const void* sbase, unsigned lds0, unsigned lds1) {
  unsigned keep;
  asm volatile(LDS_DMA_BEGIN LDS_DMA_M0("%4") LDS_DMA_P1("%1", "%3") LDS_DMA_M0("%5") LDS_DMA_P1("%2", "%3") LDS_DMA_END
               : "=&s"(keep)
               : "v"(off0), "v"(off1), "s"(sbase), "s"(lds0), "s"(lds1)
               : "memory");
}
// PW consecutive pieces: source = sbase + voff + i * 1024, destination = lds + i * 1024; a second M0 value (and lane offset) past four pieces.
template <int PW> __device__ __forceinline__ void dma_n(unsigned voff, const void* sbase, unsigned lds) {
  static_assert(PW == 8 || PW == 6 || PW == 4 || PW == 3 || PW == 2, "pieces per statement");
  unsigned keep;
#define LDS_DMA_LE4(P) \
  asm volatile(LDS_DMA_BEGIN LDS_DMA_M0("%3") P("%1", "%2") LDS_DMA_END : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds) : "memory")
#define LDS_DMA_GT4(P)                                                                                          \
  asm volatile(LDS_DMA_BEGIN LDS_DMA_M0("%4") LDS_DMA_P4("%1", "%3") LDS_DMA_M0("%5") P("%2", "%3") LDS_DMA_END \
               : "=&s"(keep)                                                                                    \
               : "v"(voff), "v"(voff + 4096u), "s"(sbase), "s"(lds), "s"(lds + 4096u)                           \
               : "memory")
  if constexpr (PW == 2) LDS_DMA_LE4(LDS_DMA_P2);
  else if constexpr (PW == 3) LDS_DMA_LE4(LDS_DMA_P3);
  else if constexpr (PW == 4) LDS_DMA_LE4(LDS_DMA_P4);
  else if constexpr (PW == 6) LDS_DMA_GT4(LDS_DMA_P2);
  else LDS_DMA_GT4(LDS_DMA_P4);
#undef LDS_DMA_LE4
#undef LDS_DMA_GT4
}

// 16-byte global load through inline asm: a compiler-visible global_load inside a loop that also carries LDS-DMAs makes hipcc's waitcnt
// pass carry "load pending" around the back edge and plant s_waitcnt vmcnt(15..0) between the MFMAs - which drains the DMA ring (issued
// from asm, invisible to that pass) at every step.  Counted by hand like the DMAs.
__device__ __forceinline__ u32x4 gload16(const void* p) {
  u32x4 v;
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
  return v;
}
// workgroup barrier that the instruction scheduler may not move anything across
__device__ __forceinline__ void bar() {
  asm volatile("s_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
// two floats -> one register of this build's 16-bit type (round to nearest even)
__device__ __forceinline__ unsigned pk2(float a, float b) {
  typedef __attribute__((ext_vector_type(2))) bf16 bf16x2_t;
  const bf16x2_t v = {(bf16)a, (bf16)b};
  return __builtin_bit_cast(unsigned, v);
}

// compile-time loop: f(std::integral_constant<int, 0>{}) ... f(std::integral_constant<int, N - 1>{}).  The index is a type, every schedule
// test on it an `if constexpr` (a `#pragma unroll` loop over a body of a few hundred instructions is refused by the unroller's cost model -
// and the register arrays it indexes then live in scratch).
template <int... I, typename F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, I...>, F&& f) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl(std::make_integer_sequence<int, N>{}, static_cast<F&&>(f)); }

}  // namespace FSVIT_NS

#undef LDS_DMA_M0
#undef LDS_DMA_P
#undef LDS_DMA_P1
#undef LDS_DMA_P2
#undef LDS_DMA_P3
#undef LDS_DMA_P4
#undef LDS_DMA_BEGIN
#undef LDS_DMA_END
