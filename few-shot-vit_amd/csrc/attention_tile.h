// Building blocks shared by the stand-alone attention kernels (attention.hip in both 16-bit builds, attention_bwd.hip): the register softmax over
// the transposed MFMA result layout, the dS pieces of the backward, all-loads-first 16-bit staging, the fp32 row epilogue, the transposing
// A-fragment read and the bf16x8 pack, the two FMA fallback loops - and, on the host side, the one launch sequence, the route id and the LDS budget.
// Every device function is force-inlined and keeps the order of floating-point operations of the block it replaced.
// A helper is optimised on its own before hipcc inlines it (its loops are unrolled first), which moves the register allocation of some callers: a
// kernel uses a helper only where no instantiation's VGPR count, spills or scratch rise (tools/kernel_regs.sh).  That leaves three blocks written
// out: the softmax of attention_v2_kernel (as a call its mask compares hoist out of the unrolled query-tile loop: +10 VGPRs in <f32x2l, 7, 1, 4>,
// 18 -> 78 spilled SGPRs in <f32x2l, 13, 1, 7>), and in the exact-fp32 backward kernels the fp32 staging (+4 VGPRs in attention_bwd_f32mfma_kernel<2, 6>, 160 -> 194 spilled SGPRs in
// the long kernel) and phase C of attention_bwd_f32mfma_kernel (tile_ds: +2 VGPRs in <7, 3>).
#pragma once
#include "fsvit_common.h"

namespace FSVIT_NS {

// ------------------------------------------------------------------------------------------------------------ device: register tiles
// A [key x query] score tile as K . Q^T leaves it in the MFMA result registers: sc[kt][r] = key 16 kt + 4 lq + r of query lrow, so one query's
// keys live in the 4 lanes {lrow + 16 j} and a row statistic is an in-lane reduction plus the two shuffles at 16 and 32.

// Masks keys >= S, scales, and leaves the UNNORMALISED exponentials in sc; m = row maximum (of the scaled scores), inv = 1 / row sum.
// FAST_EXP: the hardware exp2 (v_exp_f32) - the caller folds log2(e) into sscale; otherwise expf.
template <int KT, bool FAST_EXP>
__device__ __forceinline__ void tile_softmax(f32x4 (&sc)[KT], int S, float sscale, int lq, float& m, float& inv) {
  float mx = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < KT; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool ok = kt * 16 + lq * 4 + r < S;
      sc[kt][r] = ok ? sc[kt][r] * sscale : -INFINITY;
      mx = fmaxf(mx, sc[kt][r]);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int kt = 0; kt < KT; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float d = sc[kt][r] - mx;                  // -inf for masked keys -> exp = 0
      const float e = FAST_EXP ? __builtin_amdgcn_exp2f(d) : expf(d);
      sc[kt][r] = e;
      sum += e;
    }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  m = mx;
  inv = 1.0f / sum;
}

// sc = P = sc * inv;  dot = D = rowsum(P o dP)
template <int KT>
__device__ __forceinline__ void tile_normalise_dot(f32x4 (&sc)[KT], const f32x4 (&dp)[KT], float inv, float& dot) {
  dot = 0.f;
#pragma unroll
  for (int kt = 0; kt < KT; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float pr = sc[kt][r] * inv;
      sc[kt][r] = pr;
      dot += pr * dp[kt][r];
    }
  dot += __shfl_xor(dot, 16, 64);
  dot += __shfl_xor(dot, 32, 64);
}

// sc = dS = scale * P o (dP - D)
template <int KT>
__device__ __forceinline__ void tile_ds(f32x4 (&sc)[KT], const f32x4 (&dp)[KT], float dot, float scale) {
#pragma unroll
  for (int kt = 0; kt < KT; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) sc[kt][r] = scale * sc[kt][r] * (dp[kt][r] - dot);
}

// Two result registers (keys / queries 4 lq + 0..3 of two consecutive 16-tiles) as the 8 K slots of one 16-bit MFMA B operand
__device__ __forceinline__ u32x4 pack_bf16x8(f32x4 a, f32x4 b) {
  const bf16x8 p = {(bf16)a[0], (bf16)a[1], (bf16)a[2], (bf16)a[3], (bf16)b[0], (bf16)b[1], (bf16)b[2], (bf16)b[3]};
  return __builtin_bit_cast(u32x4, p);
}

__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(size_t)(__attribute__((address_space(3))) const void*)p; }

// A fragment of a ROW-major 16-bit LDS image (row stride rs bytes) for a product that contracts over its rows: the 16 columns c0 .. c0 + 15 become
// the MFMA rows, the K slots are rows r0 + 4 lq + j and r0 + 16 + 4 lq + j - the order pack_bf16x8 gives the B operand.  ds_read_b64_tr_b16: the
// lane supplies a = the address of columns c0 + 4 (lrow & 3) .. of row r0 + 4 lq + (lrow >> 2) and receives rows r0 + 4 lq + 0..3 (+ 16) of
// column c0 + lrow (tools/probes/tr_read_probe.hip).
__device__ __forceinline__ u32x4 tr_read_a(unsigned a, int rs) {
  typedef short s4t __attribute__((ext_vector_type(4)));
  const u32x2 v0 = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4t*)(size_t)a));
  const u32x2 v1 = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4t*)(size_t)(a + 16 * rs)));
  return u32x4{v0[0], v0[1], v1[0], v1[1]};
}

// ------------------------------------------------------------------------------------------------------------ device: staging and epilogue
// N row-major matrices of HDP 16-bit columns (row strides in elements) -> LDS images of SKP rows of RS bytes, rows >= S zero.  Every global load is
// issued before the first LDS store, UNCONDITIONALLY on clamped rows.  The loop form - `if (row < S) { loads }`, stores, next iteration - waited for each iteration's loads before issuing the next ones: N HBM
// latencies per head.
template <int N, int SKP, int HDP, int RS, int NT>
__device__ __forceinline__ void stage_rows_b16(const bf16* const (&src)[N], const size_t (&stride)[N], unsigned char* const (&lds)[N], int S, int t) {
  constexpr int CPR = HDP / 8, NIT = (SKP * CPR + NT - 1) / NT;          // 16-byte chunks per row
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  u32x4 v[NIT][N];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int idx = t + it * NT, row = idx / CPR, ch = idx - row * CPR;
    const int rc = row < S ? row : S - 1;
#pragma unroll
    for (int n = 0; n < N; ++n) v[it][n] = *reinterpret_cast<const u32x4*>(src[n] + (size_t)rc * stride[n] + ch * 8);
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int idx = t + it * NT, row = idx / CPR, ch = idx - row * CPR;
    if (idx < SKP * CPR) {
#pragma unroll
      for (int n = 0; n < N; ++n) *reinterpret_cast<u32x4*>(lds[n] + row * RS + ch * 16) = row < S ? v[it][n] : zero4;
    }
  }
}

// One fp32 output row from transposed accumulators: acc[dt] = columns 16 dt + 4 lq + 0..3.  Columns hd .. hdp are written too (the operand is zero
// there -> exact zeros); hdp need not be a multiple of 16, so the last register may end in a per-element tail.
template <int DT>
__device__ __forceinline__ void store_rows_f32(const f32x4 (&acc)[DT], float* row, int hdp, int lq) {
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    const int d = dt * 16 + 4 * lq;
    if (d + 3 < hdp) *reinterpret_cast<f32x4*>(row + d) = acc[dt];
    else
#pragma unroll
      for (int r = 0; r < 4; ++r) if (d + r < hdp) row[d + r] = acc[dt][r];
  }
}

// ------------------------------------------------------------------------------------------------------------ device: the FMA fallbacks
// 256 threads over fp32 LDS matrices: Q / dO [rows][ld], K / V [S][ld], P / dP [rows][ls].
// P = scale * Q K^T (the scaled scores),  dP = dO V^T
__device__ __forceinline__ void fma_scores_dp(const float* Q, const float* dO, const float* K, const float* V, float* P, float* dP,
                                              int rows, int S, int hd, int ld, int ls, float scale, int t) {
  for (int idx = t; idx < rows * S; idx += 256) {
    const int i = idx / S, j = idx - i * S;
    float s = 0.f, dp = 0.f;
    for (int d = 0; d < hd; ++d) { s += Q[i * ld + d] * K[j * ld + d]; dp += dO[i * ld + d] * V[j * ld + d]; }
    P[i * ls + j] = s * scale;
    dP[i * ls + j] = dp;
  }
}

// One wave per row: P = softmax(P) in place, dS = scale * P o (dP - rowsum(P o dP)) over dP.  Rows nq .. rows (past the end of the head): P = dS = 0.
__device__ __forceinline__ void fma_softmax_ds(float* P, float* dS, int rows, int nq, int S, int ls, float scale, int lane, int wave) {
  for (int i = wave; i < rows; i += 4) {
    float m = -INFINITY;
    for (int j = lane; j < S; j += 64) m = fmaxf(m, P[i * ls + j]);
    m = wave_max(m);
    float sum = 0.f;
    for (int j = lane; j < S; j += 64) { const float e = expf(P[i * ls + j] - m); P[i * ls + j] = e; sum += e; }
    const float inv = i < nq ? 1.0f / wave_sum(sum) : 0.f;
    float dot = 0.f;
    for (int j = lane; j < S; j += 64) { const float p = P[i * ls + j] * inv; P[i * ls + j] = p; dot += p * dS[i * ls + j]; }
    dot = wave_sum(dot);
    for (int j = lane; j < S; j += 64) dS[i * ls + j] = scale * P[i * ls + j] * (dS[i * ls + j] - dot);
  }
}

// ------------------------------------------------------------------------------------------------------------ host
constexpr size_t kAttnLdsMax = 160 * 1024;          // the LDS of one CU: what an (image, head) workgroup may hold

// One workgroup per (image, head): raises the kernel's dynamic-LDS limit where the image needs more than the default 64 KB, launches, and returns
// the launch error.  Arguments are passed on with the kernel's own parameter types.
template <typename... KA, typename... A>
inline int launch_head(void (*kern)(KA...), size_t lds_bytes, int blocks, int threads, hipStream_t s, A... a) {
  if (lds_bytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return (int)e;
  }
  return launch(kern, dim3(blocks), dim3(threads), lds_bytes, s, a...);
}

// What attention_route / attention_bwd_route return (fsvit.h fsvit_op_attention_route, fsvit_op_attention_bwd_route):
// family * 100000 + elem * 10000 + KT * 100 + DT - key tiles and head-dim tiles of the instantiation, 0 where the kernel has none.
struct AttnRoute { int family, elem, kt, dt; };
inline int route_id(int family, int elem, int kt, int dt) { return family * 100000 + elem * 10000 + kt * 100 + dt; }
inline AttnRoute route_decode(int id) { return {id / 100000, id / 10000 % 10, id / 100 % 100, id % 100}; }

}  // namespace FSVIT_NS
