// Attention backward for the training steps (backward of test_phase/models/visformer.py:183-190 and of the ViT / DeiT blocks):
// given q, k, v (the qkv GEMM output, head dim padded to hdp) and d(ctx), recompute P = softmax(scale q k^T) and form
//   dV = P^T dO,  dP = dO V^T,  dS = scale * P o (dP - rowsum(dP o P)),  dQ = dS K,  dK = dS^T Q.
// One workgroup per (image, head) in every kernel.  attention_bwd_route picks the kernel (route family in brackets); the blocks they share -
// register softmax, dS, staging, fp32 epilogue, transposing fragment read, the FMA loops, the launch sequence - are attention_tile.h.
//   [1] attention_bwd_mfma_kernel<KT, DT, NW>          bf16 MFMA, S <= 224, hdp a multiple of 32: the whole head row-major in LDS, two passes
//   [2] attention_bwd_f32mfma_kernel<KT, DT>           exact fp32 MFMA where Q, K, V, dO and one [S][S] matrix fit the LDS (Visformer stages)
//   [3] attention_bwd_f32mfma_long_kernel<13, 4, 7>    exact fp32 MFMA, S <= 208 x hdp <= 64 (ViT / DeiT): two matrices resident at a time, two passes
//   [4] attention_bwd_kernel<T>                        FMA loops, everything in LDS as fp32: the shapes without an MFMA instantiation, both dtypes
//   [5] attention_bwd_tiled_f32_kernel<16>             FMA loops, fp32, K / V resident and the queries in blocks of 16: what [4] cannot hold
#include "attention_tile.h"
#include "train_kernels.h"

#include <cstdlib>

namespace fsvit {

template <typename T>
__global__ __launch_bounds__(256) void attention_bwd_kernel(const T* __restrict__ qkv, const T* __restrict__ dctx, T* __restrict__ dqkv,
                                                            int S, int heads, int hd, int hdp, float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int ld = hd + 1, ls = S + 1;
  float* Q = reinterpret_cast<float*>(smem);
  float* K = Q + S * ld;
  float* V = K + S * ld;
  float* dO = V + S * ld;
  float* P = dO + S * ld;          // [S][S+1]
  float* dP = P + S * ls;          // [S][S+1]  (dP, then dS)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const int rowlen = 3 * heads * hdp;
  const T* base = qkv + (size_t)b * S * rowlen + h * hdp;
  const T* dob = dctx + (size_t)b * S * heads * hdp + h * hdp;
  for (int idx = t; idx < S * hd; idx += 256) {
    const int i = idx / hd, d = idx - i * hd;
    const T* r = base + (size_t)i * rowlen + d;
    Q[i * ld + d] = to_f32<T>(r[0]);
    K[i * ld + d] = to_f32<T>(r[heads * hdp]);
    V[i * ld + d] = to_f32<T>(r[2 * heads * hdp]);
    dO[i * ld + d] = to_f32<T>(dob[(size_t)i * heads * hdp + d]);
  }
  __syncthreads();
  fma_scores_dp(Q, dO, K, V, P, dP, S, S, hd, ld, ls, scale, t);
  __syncthreads();
  fma_softmax_ds(P, dP, S, S, S, ls, scale, lane, wave);
  __syncthreads();
  T* dq = dqkv + (size_t)b * S * rowlen + h * hdp;
  for (int idx = t; idx < S * hdp; idx += 256) {
    const int i = idx / hdp, d = idx - i * hdp;
    float gq = 0.f, gk = 0.f, gv = 0.f;
    if (d < hd) {
      for (int j = 0; j < S; ++j) {
        gq += dP[i * ls + j] * K[j * ld + d];          // dQ[i] = sum_j dS[i][j] K[j]
        gk += dP[j * ls + i] * Q[j * ld + d];          // dK[i] = sum_j dS[j][i] Q[j]
        gv += P[j * ls + i] * dO[j * ld + d];          // dV[i] = sum_j P[j][i] dO[j]
      }
    }
    T* r = dq + (size_t)i * rowlen + d;                // padded head dims get exact zeros
    r[0] = from_f32<T>(gq);
    r[heads * hdp] = from_f32<T>(gk);
    r[2 * heads * hdp] = from_f32<T>(gv);
  }
}

// fp32, longer sequences (ViT: 197 tokens x head dim 64 do not fit the all-in-LDS kernel above): K and V stay resident, the queries go through in
// blocks of QB rows (Q, dO, P and dS tiles of the block in LDS); dQ of the block is final, dK / dV accumulate in the fp32 output rows themselves -
// element (key, d) is always updated by the same thread of the one workgroup that owns this (image, head), so plain read-modify-write is ordered.
template <int QB>
__global__ __launch_bounds__(256) void attention_bwd_tiled_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ dctx, float* __restrict__ dqkv,
                                                                      int S, int heads, int hd, int hdp, float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int ld = hd + 1, ls = S + 1;
  float* K = reinterpret_cast<float*>(smem);
  float* V = K + S * ld;
  float* Q = V + S * ld;           // [QB][ld]
  float* dO = Q + QB * ld;
  float* P = dO + QB * ld;         // [QB][ls]
  float* dS = P + QB * ls;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const int rowlen = 3 * heads * hdp;
  const float* base = qkv + (size_t)b * S * rowlen + h * hdp;
  const float* dob = dctx + (size_t)b * S * heads * hdp + h * hdp;
  float* dq = dqkv + (size_t)b * S * rowlen + h * hdp;
  for (int idx = t; idx < S * hd; idx += 256) {
    const int i = idx / hd, d = idx - i * hd;
    K[i * ld + d] = base[(size_t)i * rowlen + heads * hdp + d];
    V[i * ld + d] = base[(size_t)i * rowlen + 2 * heads * hdp + d];
  }
  for (int idx = t; idx < S * hdp; idx += 256) {             // dK, dV start at 0 (padded head dims stay exact zeros)
    const int i = idx / hdp, d = idx - i * hdp;
    dq[(size_t)i * rowlen + heads * hdp + d] = 0.f;
    dq[(size_t)i * rowlen + 2 * heads * hdp + d] = 0.f;
  }
  for (int q0 = 0; q0 < S; q0 += QB) {
    const int nq = S - q0 < QB ? S - q0 : QB;
    __syncthreads();
    for (int idx = t; idx < QB * hd; idx += 256) {
      const int i = idx / hd, d = idx - i * hd;
      Q[i * ld + d] = i < nq ? base[(size_t)(q0 + i) * rowlen + d] : 0.f;
      dO[i * ld + d] = i < nq ? dob[(size_t)(q0 + i) * heads * hdp + d] : 0.f;
    }
    __syncthreads();
    fma_scores_dp(Q, dO, K, V, P, dS, QB, S, hd, ld, ls, scale, t);
    __syncthreads();
    fma_softmax_ds(P, dS, QB, nq, S, ls, scale, lane, wave);
    __syncthreads();
    for (int idx = t; idx < nq * hdp; idx += 256) {            // dQ of this block
      const int i = idx / hdp, d = idx - i * hdp;
      float g = 0.f;
      if (d < hd) for (int j = 0; j < S; ++j) g += dS[i * ls + j] * K[j * ld + d];
      dq[(size_t)(q0 + i) * rowlen + d] = g;
    }
    for (int idx = t; idx < S * hd; idx += 256) {              // dK, dV contributions of this block (thread <-> element mapping fixed)
      const int j = idx / hd, d = idx - j * hd;
      float gk = 0.f, gv = 0.f;
      for (int i = 0; i < QB; ++i) { gk += dS[i * ls + j] * Q[i * ld + d]; gv += P[i * ls + j] * dO[i * ld + d]; }
      dq[(size_t)j * rowlen + heads * hdp + d] += gk;
      dq[(size_t)j * rowlen + 2 * heads * hdp + d] += gv;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// fp32 MFMA version (round 3; the `parity` and `bf16x2` trainers, Visformer shapes): exact fp32 products on v_mfma_f32_16x16x4_f32 instead of the FMA
// loops above (7.9 of the 66 ms of a two-limb training step).  One workgroup per (image, head), one wave per block of 16 tokens; Q, K, V, dO resident
// in LDS as [KT * 16 rows][DT * 16 + 1] fp32 (rows >= S and columns >= hd zero) plus ONE [query][key] matrix that holds P, then dS.
// A 16x16x4 MFMA takes one float per lane and operand - A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15] - so either orientation of a
// row-major LDS array is a plain ds_read_b32 (no transposed copies), and the result D[4 (lane >> 4) + r][lane & 15] puts 4 consecutive A-rows of one
// B-row in a lane.  Four phases, three barriers, no cross-wave reduction (every output element has ONE owner: bit-reproducible):
//   A  wave = query block: S^T and dP^T over all keys (A = K / V rows, B = Q / dO rows: a lane holds 4 keys of ITS query), softmax statistics inside the
//      4 lanes of a query (two shuffles), P -> LDS;            B  wave = key block: dV^T = dO^T P over all queries -> global;
//   C  wave = query block: dS = scale P (dP - sum_j P dP) from the registers of phase A -> LDS over P;
//   D  wave = key block: dK^T = Q^T dS -> global; wave = query block: dQ^T = K^T dS^T -> global.
template <int KT, int DT>
__global__ __launch_bounds__(KT * 64) void attention_bwd_f32mfma_kernel(const float* __restrict__ qkv, const float* __restrict__ dctx, float* __restrict__ dqkv,
                                                                        int S, int heads, int hd, int hdp, float scale) {
  constexpr int SP = KT * 16, HD = DT * 16, LD = HD + 1, PP = SP + 4, NT = KT * 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Q = reinterpret_cast<float*>(smem);
  float* K = Q + SP * LD;
  float* V = K + SP * LD;
  float* dO = V + SP * LD;
  float* PS = dO + SP * LD;                             // [SP queries][PP]: P, then dS
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lrow = lane & 15, lq = lane >> 4;
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const int rowlen = 3 * heads * hdp;
  const float* base = qkv + (size_t)b * S * rowlen + h * hdp;
  const float* dob = dctx + (size_t)b * S * heads * hdp + h * hdp;
  float* dq = dqkv + (size_t)b * S * rowlen + h * hdp;
  {   // 16-byte global loads (hdp % 4 == 0: the launcher checks), ALL in flight before the first LDS store: unconditional on clamped coordinates
      // (this and stage2 of the long kernel are one block for four and for two matrices; as a shared function it costs registers in both, attention_tile.h)
    constexpr int NIT = (SP * (HD / 4) + NT - 1) / NT;
    f32x4 vq[NIT], vk[NIT], vv[NIT], vo[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = t + it * NT, i = idx / (HD / 4), d = (idx - i * (HD / 4)) * 4;
      const bool in = i < S && d < hdp;
      const float* r = base + (size_t)(in ? i : 0) * rowlen + (in ? d : 0);
      vq[it] = *reinterpret_cast<const f32x4*>(r);
      vk[it] = *reinterpret_cast<const f32x4*>(r + heads * hdp);
      vv[it] = *reinterpret_cast<const f32x4*>(r + 2 * heads * hdp);
      vo[it] = *reinterpret_cast<const f32x4*>(dob + (size_t)(in ? i : 0) * heads * hdp + (in ? d : 0));
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = t + it * NT, i = idx / (HD / 4), d = (idx - i * (HD / 4)) * 4;
      if (idx < SP * (HD / 4)) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool ok = i < S && d + e < hd;
          Q[i * LD + d + e] = ok ? vq[it][e] : 0.f;
          K[i * LD + d + e] = ok ? vk[it][e] : 0.f;
          V[i * LD + d + e] = ok ? vv[it][e] : 0.f;
          dO[i * LD + d + e] = ok ? vo[it][e] : 0.f;
        }
      }
    }
  }
  __syncthreads();
  const int qb = wave, kb = wave;                       // this wave's query block and key block
  const float* Qb = Q + (qb * 16) * LD;
  const float* Ob = dO + (qb * 16) * LD;
  // ---- A: S^T / dP^T (lane = query qb*16 + lrow, keys kt*16 + 4 lq + r); k outermost: 2 KT independent accumulators per step
  f32x4 sc[KT], dp[KT];
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) sc[kt] = dp[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k0 = 0; k0 < HD; k0 += 4) {
    const float bq = Qb[lrow * LD + k0 + lq], bo = Ob[lrow * LD + k0 + lq];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      sc[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(K[(kt * 16 + lrow) * LD + k0 + lq], bq, sc[kt], 0, 0, 0);
      dp[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(V[(kt * 16 + lrow) * LD + k0 + lq], bo, dp[kt], 0, 0, 0);
    }
  }
  float m, inv, dot;
  tile_softmax<KT, false>(sc, S, scale, lq, m, inv);
  tile_normalise_dot<KT>(sc, dp, inv, dot);
  float* PSq = PS + (qb * 16 + lrow) * PP;
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) *reinterpret_cast<f32x4*>(PSq + kt * 16 + 4 * lq) = sc[kt];
  __syncthreads();
  // ---- B: dV^T[d][key] = sum_q dO[q][d] P[q][key] for this wave's key block -> global (lane: key kb*16 + lrow, d = dt*16 + 4 lq + r)
  auto key_block_product = [&](const float* X, int which) {      // X = dO (-> dV, which = 2) or Q (-> dK, which = 1)
    f32x4 acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k0 = 0; k0 < SP; k0 += 4) {
      const float bp = PS[(k0 + lq) * PP + kb * 16 + lrow];
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(X[(k0 + lq) * LD + dt * 16 + lrow], bp, acc[dt], 0, 0, 0);
    }
    const int key = kb * 16 + lrow;
    if (key < S) store_rows_f32<DT>(acc, dq + (size_t)key * rowlen + which * heads * hdp, hdp, lq);      // (columns hd .. hdp: the operand is zero there -> exact zeros)
  };
  key_block_product(dO, 2);
  __syncthreads();
  // ---- C: dS over P (tile_ds written out: as a call it costs <7, 3> two VGPRs, attention_tile.h)
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) {
    f32x4 ds;
#pragma unroll
    for (int r = 0; r < 4; ++r) ds[r] = scale * sc[kt][r] * (dp[kt][r] - dot);
    *reinterpret_cast<f32x4*>(PSq + kt * 16 + 4 * lq) = ds;
  }
  __syncthreads();
  // ---- D: dK^T for the key block; dQ^T[d][q] = sum_key K[key][d] dS[q][key] for the query block (lane: query lrow, d = dt*16 + 4 lq + r)
  key_block_product(Q, 1);
  {
    f32x4 acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k0 = 0; k0 < SP; k0 += 4) {
      const float bs = PSq[k0 + lq];
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(K[(k0 + lq) * LD + dt * 16 + lrow], bs, acc[dt], 0, 0, 0);
    }
    const int qrow = qb * 16 + lrow;
    if (qrow < S) store_rows_f32<DT>(acc, dq + (size_t)qrow * rowlen, hdp, lq);
  }
}

// LDS image of attention_bwd_f32mfma_kernel: Q, K, V, dO [SP][HD + 1] and P / dS [SP][SP + 4]
static constexpr size_t bwd_f32mfma_lds(int kt, int dt) { return ((size_t)4 * kt * 16 * (dt * 16 + 1) + (size_t)kt * 16 * (kt * 16 + 4)) * sizeof(float); }

template <int KT, int DT>
static int launch_bwd_f32mfma(const void* qkv, const void* dctx, void* dqkv, int B, int S, int heads, int hd, int hdp, float scale, hipStream_t s) {
  static_assert(bwd_f32mfma_lds(KT, DT) <= kAttnLdsMax, "attention_bwd_f32mfma_kernel<KT, DT>: the image does not fit the LDS");
  if ((hdp & 3) || hdp > DT * 16) return (int)hipErrorInvalidValue;
  return launch_head(attention_bwd_f32mfma_kernel<KT, DT>, bwd_f32mfma_lds(KT, DT), B * heads, KT * 64, s, qkv, dctx, dqkv, S, heads, hd, hdp, scale);
}

// ---------------------------------------------------------------------------------------------------------------
// fp32 MFMA, long sequences (ViT / DeiT: 197 tokens x 64; the `parity` and `bf16x2` ViT trainers): Q, K, V, dO do not fit the LDS together (216 KB),
// so the head is walked twice, flash-style, with TWO of the four matrices resident at a time (111 KB) and the other two entering as per-lane B operands
// straight from global memory (16 floats per lane and matrix).  attention_bwd_tiled_f32_kernel (FMA loops) took 9.6 ms per DeiT-S launch = 73 % of a
// two-limb training step.
//   pass 1 (K, V resident; a wave owns query blocks): S^T / dP^T over all keys (lane = query lrow, keys 4 lq + r), the softmax statistics
//          (max, 1 / sum, sum_j P dP) -> LDS, dS in registers, dQ^T = K^T dS^T -> global;
//   pass 2 (Q, dO resident; a wave owns key blocks): per query block S / dP recomputed in the OTHER orientation (lane = key lrow, queries 4 lq + r),
//          P and dS from the stored statistics, dV^T += dO^T P, dK^T += Q^T dS -> global.
// No matrix is ever transposed or staged for the second product of a chain: a 16x16x4 step may sum ANY four k indices as long as both operands agree,
// so step (tile, r) takes k = lane >> 4 -> index 16 tile + 4 (lane >> 4) + r: the B operand is the lane's own result register [r] of the previous product.
template <int KT, int DT, int NW>
__global__ __launch_bounds__(NW * 64) void attention_bwd_f32mfma_long_kernel(const float* __restrict__ qkv, const float* __restrict__ dctx, float* __restrict__ dqkv,
                                                                             int S, int heads, int hd, int hdp, float scale) {
  constexpr int SP = KT * 16, HD = DT * 16, LD = HD + 1, NT = NW * 64, KS = HD / 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* A0 = reinterpret_cast<float*>(smem);          // pass 1: K, pass 2: Q        [SP][LD]
  float* A1 = A0 + SP * LD;                            // pass 1: V, pass 2: dO
  float* st_m = A1 + SP * LD;                          // per query: row maximum (scaled scores), 1 / sum, sum_j P dP
  float* st_i = st_m + SP;
  float* st_d = st_i + SP;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lrow = lane & 15, lq = lane >> 4;
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const int rowlen = 3 * heads * hdp;
  const float* base = qkv + (size_t)b * S * rowlen + h * hdp;
  const float* dob = dctx + (size_t)b * S * heads * hdp + h * hdp;
  const size_t dorow = (size_t)heads * hdp;
  float* dq = dqkv + (size_t)b * S * rowlen + h * hdp;
  // two matrices ([S][hd], row strides sa / sb floats) -> A0 / A1, zero padded; all loads in flight before the first LDS store
  auto stage2 = [&](const float* pa, size_t sa, const float* pb, size_t sb) {
    constexpr int NIT = (SP * (HD / 4) + NT - 1) / NT;
    f32x4 va[NIT], vb[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = t + it * NT, i = idx / (HD / 4), d = (idx - i * (HD / 4)) * 4;
      const bool in = i < S && d < hdp;
      va[it] = *reinterpret_cast<const f32x4*>(pa + (size_t)(in ? i : 0) * sa + (in ? d : 0));
      vb[it] = *reinterpret_cast<const f32x4*>(pb + (size_t)(in ? i : 0) * sb + (in ? d : 0));
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = t + it * NT, i = idx / (HD / 4), d = (idx - i * (HD / 4)) * 4;
      if (idx < SP * (HD / 4)) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool ok = i < S && d + e < hd;
          A0[i * LD + d + e] = ok ? va[it][e] : 0.f;
          A1[i * LD + d + e] = ok ? vb[it][e] : 0.f;
        }
      }
    }
  };
  // the rows blk * 16 + lrow of a matrix as B operands: element [k = 4 s + lq] for the KS steps (zero past the row / the head dim)
  auto rows_b = [&](const float* pm, size_t stride, int blk, float (&o)[KS]) {
    const int row = blk * 16 + lrow;
#pragma unroll
    for (int s0 = 0; s0 < KS; ++s0) {
      const int d = 4 * s0 + lq;
      const bool in = row < S && d < hd;
      const float v = pm[(size_t)(in ? row : 0) * stride + (in ? d : 0)];
      o[s0] = in ? v : 0.f;
    }
  };

  // ---------------- pass 1
  stage2(base + heads * hdp, rowlen, base + 2 * heads * hdp, rowlen);          // K, V
  __syncthreads();
  for (int qb = wave; qb < KT; qb += NW) {
    float bq[KS], bo[KS];
    rows_b(base, rowlen, qb, bq);
    rows_b(dob, dorow, qb, bo);
    f32x4 sc[KT], dp[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) sc[kt] = dp[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s0 = 0; s0 < KS; ++s0) {
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        sc[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(A0[(kt * 16 + lrow) * LD + 4 * s0 + lq], bq[s0], sc[kt], 0, 0, 0);
        dp[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(A1[(kt * 16 + lrow) * LD + 4 * s0 + lq], bo[s0], dp[kt], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);               // (keeps hipcc from hoisting every fragment read of the 416-MFMA block to its top: 98 spilled VGPRs)
    }
    float m, inv, dot;
    tile_softmax<KT, false>(sc, S, scale, lq, m, inv);
    tile_normalise_dot<KT>(sc, dp, inv, dot);
    const int qrow = qb * 16 + lrow;
    if (lq == 0) { st_m[qrow] = m; st_i[qrow] = qrow < S ? inv : 0.f; st_d[qrow] = dot; }      // (queries past the end: P = 0 in pass 2)
    tile_ds<KT>(sc, dp, dot, scale);
    // dQ^T[d][q] = sum_key K[key][d] dS[q][key]: step (kt, r) sums the keys 16 kt + 4 lq + r
    f32x4 acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(A0[(kt * 16 + 4 * lq + r) * LD + dt * 16 + lrow], sc[kt][r], acc[dt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (qrow < S) store_rows_f32<DT>(acc, dq + (size_t)qrow * rowlen, hdp, lq);      // (columns hd .. hdp: K is zero there -> exact zeros)
  }
  __syncthreads();
  // ---------------- pass 2
  stage2(base, rowlen, dob, dorow);                                            // Q, dO
  __syncthreads();
  for (int kb = wave; kb < KT; kb += NW) {
    float bk[KS], bv[KS];
    rows_b(base + heads * hdp, rowlen, kb, bk);
    rows_b(base + 2 * heads * hdp, rowlen, kb, bv);
    const bool key_ok = kb * 16 + lrow < S;
    f32x4 accV[DT], accK[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) accV[dt] = accK[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int qb = 0; qb < KT; ++qb) {
      f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, p4 = s4;          // lane = key lrow, queries qb*16 + 4 lq + r
#pragma unroll
      for (int s0 = 0; s0 < KS; ++s0) {
        s4 = __builtin_amdgcn_mfma_f32_16x16x4f32(A0[(qb * 16 + lrow) * LD + 4 * s0 + lq], bk[s0], s4, 0, 0, 0);
        p4 = __builtin_amdgcn_mfma_f32_16x16x4f32(A1[(qb * 16 + lrow) * LD + 4 * s0 + lq], bv[s0], p4, 0, 0, 0);
      }
      const f32x4 m4 = *reinterpret_cast<const f32x4*>(st_m + qb * 16 + 4 * lq), i4 = *reinterpret_cast<const f32x4*>(st_i + qb * 16 + 4 * lq),
                  d4 = *reinterpret_cast<const f32x4*>(st_d + qb * 16 + 4 * lq);
      f32x4 P, dS;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pr = key_ok ? expf(s4[r] * scale - m4[r]) * i4[r] : 0.f;
        P[r] = pr;
        dS[r] = scale * pr * (p4[r] - d4[r]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          accV[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(A1[(qb * 16 + 4 * lq + r) * LD + dt * 16 + lrow], P[r], accV[dt], 0, 0, 0);
          accK[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(A0[(qb * 16 + 4 * lq + r) * LD + dt * 16 + lrow], dS[r], accK[dt], 0, 0, 0);
        }
    }
    const int key = kb * 16 + lrow;
    if (key < S) {
      float* rk = dq + (size_t)key * rowlen + heads * hdp;
      store_rows_f32<DT>(accK, rk, hdp, lq);
      store_rows_f32<DT>(accV, rk + heads * hdp, hdp, lq);
    }
  }
}

// LDS image of attention_bwd_f32mfma_long_kernel: two matrices [SP][HD + 1] and the three per-query statistics
static constexpr size_t bwd_f32mfma_long_lds(int kt, int dt) { return ((size_t)2 * kt * 16 * (dt * 16 + 1) + (size_t)3 * kt * 16) * sizeof(float); }

template <int KT, int DT, int NW>
static int launch_bwd_f32mfma_long(const void* qkv, const void* dctx, void* dqkv, int B, int S, int heads, int hd, int hdp, float scale, hipStream_t s) {
  static_assert(bwd_f32mfma_long_lds(KT, DT) <= kAttnLdsMax, "attention_bwd_f32mfma_long_kernel<KT, DT, .>: the image does not fit the LDS");
  if ((hdp & 3) || hdp > DT * 16) return (int)hipErrorInvalidValue;
  return launch_head(attention_bwd_f32mfma_long_kernel<KT, DT, NW>, bwd_f32mfma_long_lds(KT, DT), B * heads, NW * 64, s, qkv, dctx, dqkv, S, heads, hd, hdp, scale);
}

// ---------------------------------------------------------------------------------------------------------------
// bf16 MFMA version.  One workgroup per (image, head); S <= 224 keys, everything of the head lives in LDS, ROW-major only:
//   Q, K, V, dO  [SKP][HDP]   score-type products read 16-byte k-chunks of a row; the three products that contract over keys / queries take
//   their A operand (8 consecutive rows of one column) from the same images with ds_read_b64_tr_b16 (tools/probes/tr_read_probe.hip) -
//   round 1 kept transposed copies K^T, Q^T, dO^T written with 2-byte stores (126 KB at 100 tokens, S <= 128)
// pass 1 (per 16-query tile, one wave): S^T = K Q^T and dP^T = V dO^T in the [key x query] orientation, in-register
//   softmax (2 shuffles), D = rowsum(P o dP), dS = scale P o (dP - D); dQ^T = K^T dS^T with dS fed back as the MFMA B
//   operand straight from registers (keys permuted consistently in both operands, as attention_v2 does for P V).
//   The per-query statistics (max, 1/sum, D) go to LDS.
// pass 2 (per 16-key tile, one wave): S and dP recomputed in the [query x key] orientation from the statistics, so
//   P and dS are again B operands from registers: dV^T = dO^T P, dK^T = Q^T dS.
template <int NKT, int NDT, int NW>
__global__ __launch_bounds__(NW * 64) void attention_bwd_mfma_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ dctx,
                                                                     bf16* __restrict__ dqkv, int S, int heads, float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int HDP = NDT * 16, SKP = NKT * 16;
  constexpr int RS = HDP * 2 + 32;             // row-major row stride (bytes): 32 mod 64 - the conflict-free pitch for b128 reads whose 16-lane groups mix rows of two lq (round 6: 244 -> 233 us at the stage-2 shape; an odd multiple of 16 - 144 before - reads 2-way)
  constexpr int NKC = HDP / 32;                // 32-element MFMA chunks along the head dim
  unsigned char* const Qr = smem;
  unsigned char* const Kr = Qr + SKP * RS;
  unsigned char* const Vr = Kr + SKP * RS;
  unsigned char* const Or = Vr + SKP * RS;
  float* const st_m = reinterpret_cast<float*>(Or + SKP * RS);
  float* const st_inv = st_m + SKP;
  float* const st_D = st_inv + SKP;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lrow = lane & 15, lq = lane >> 4;
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const int rowlen = 3 * heads * HDP;
  const bf16* base = qkv + (size_t)b * S * rowlen + h * HDP;
  const bf16* dob = dctx + (size_t)b * S * heads * HDP + h * HDP;
  bf16* dbase = dqkv + (size_t)b * S * rowlen + h * HDP;

  {   // all staging loads of the head in flight at once
    const bf16* const src[4] = {base, base + heads * HDP, base + 2 * heads * HDP, dob};
    const size_t stride[4] = {(size_t)rowlen, (size_t)rowlen, (size_t)rowlen, (size_t)heads * HDP};
    unsigned char* const img[4] = {Qr, Kr, Vr, Or};
    stage_rows_b16<4, SKP, HDP, RS, NW * 64>(src, stride, img, S, t);
  }
  __syncthreads();

  const float sscale = scale * 1.44269504088896340736f;        // exp2 domain, exactly as the forward kernel
  // rows r0 .. r0 + 31 x columns c0 .. c0 + 15 of a row-major image as the A fragment of a product over its rows
  auto trA = [&](const unsigned char* img, int r0, int c0) { return tr_read_a(lds_addr(img) + (r0 + lq * 4 + (lrow >> 2)) * RS + (c0 + (lrow & 3) * 4) * 2, RS); };
  const int nt = (S + 15) / 16;

  // ------------------------------------------------------------------ pass 1: dQ + per-query statistics
  for (int qt = wave; qt < NKT; qt += NW) {
    const int q = qt * 16 + lrow;
    if (qt >= nt) {                                               // padded query tile: P = 0 in pass 2
      if (lq == 0) { st_m[q] = 0.f; st_inv[q] = 0.f; st_D[q] = 0.f; }
      continue;
    }
    u32x4 qf[NKC], of[NKC];
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) {
      qf[kc] = *reinterpret_cast<const u32x4*>(Qr + q * RS + (kc * 4 + lq) * 16);
      of[kc] = *reinterpret_cast<const u32x4*>(Or + q * RS + (kc * 4 + lq) * 16);
    }
    f32x4 sc[NKT], dp[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
      const int krow = (kt * 16 + lrow) * RS + lq * 16;
#pragma unroll
      for (int kc = 0; kc < NKC; ++kc) {
        a0 = mma_chunk<bf16>(*reinterpret_cast<const u32x4*>(Kr + krow + kc * 64), qf[kc], a0);
        a1 = mma_chunk<bf16>(*reinterpret_cast<const u32x4*>(Vr + krow + kc * 64), of[kc], a1);
      }
      sc[kt] = a0;                       // keys kt*16 + lq*4 + r  x  query lrow
      dp[kt] = a1;
    }
    float m, inv, D;
    tile_softmax<NKT, true>(sc, S, sscale, lq, m, inv);
    tile_normalise_dot<NKT>(sc, dp, inv, D);
    const bool qok = q < S;
    if (lq == 0) { st_m[q] = m; st_inv[q] = qok ? inv : 0.f; st_D[q] = D; }
    tile_ds<NKT>(sc, dp, D, scale);
    // dQ^T[d][q] = sum_key K^T[d][key] * dS[q][key]
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kc = 0; kc < NKT / 2; ++kc)
        acc = mma_chunk<bf16>(trA(Kr, 32 * kc, dt * 16), pack_bf16x8(sc[2 * kc], sc[2 * kc + 1]), acc);
      if (qok) store4<bf16>(dbase + (size_t)q * rowlen + dt * 16 + lq * 4, acc);
    }
  }
  __syncthreads();

  // ------------------------------------------------------------------ pass 2: dK, dV
  for (int jt = wave; jt < nt; jt += NW) {
    const int key = jt * 16 + lrow;
    const bool kok = key < S;
    u32x4 kf[NKC], vf[NKC];
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) {
      kf[kc] = *reinterpret_cast<const u32x4*>(Kr + key * RS + (kc * 4 + lq) * 16);
      vf[kc] = *reinterpret_cast<const u32x4*>(Vr + key * RS + (kc * 4 + lq) * 16);
    }
    f32x4 accK[NDT], accV[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) { accK[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; accV[dt] = accK[dt]; }
#pragma unroll
    for (int qc = 0; qc < NKT / 2; ++qc) {
      f32x4 P[2], dS[2];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int it = 2 * qc + half;
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
        const int qrow = (it * 16 + lrow) * RS + lq * 16;
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc) {
          a0 = mma_chunk<bf16>(*reinterpret_cast<const u32x4*>(Qr + qrow + kc * 64), kf[kc], a0);    // queries it*16 + lq*4 + r  x  key lrow
          a1 = mma_chunk<bf16>(*reinterpret_cast<const u32x4*>(Or + qrow + kc * 64), vf[kc], a1);
        }
        const f32x4 m4 = *reinterpret_cast<const f32x4*>(st_m + it * 16 + lq * 4);
        const f32x4 i4 = *reinterpret_cast<const f32x4*>(st_inv + it * 16 + lq * 4);
        const f32x4 D4 = *reinterpret_cast<const f32x4*>(st_D + it * 16 + lq * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pr = kok ? __builtin_amdgcn_exp2f(a0[r] * sscale - m4[r]) * i4[r] : 0.f;
          P[half][r] = pr;
          dS[half][r] = scale * pr * (a1[r] - D4[r]);
        }
      }
      const u32x4 pb = pack_bf16x8(P[0], P[1]), sb = pack_bf16x8(dS[0], dS[1]);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        accV[dt] = mma_chunk<bf16>(trA(Or, 32 * qc, dt * 16), pb, accV[dt]);
        accK[dt] = mma_chunk<bf16>(trA(Qr, 32 * qc, dt * 16), sb, accK[dt]);
      }
    }
    if (kok) {
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        bf16* r = dbase + (size_t)key * rowlen + heads * HDP + dt * 16 + lq * 4;
        store4<bf16>(r, accK[dt]);
        store4<bf16>(r + heads * HDP, accV[dt]);
      }
    }
  }
}

// LDS image of attention_bwd_mfma_kernel: Q, K, V, dO [SKP] rows at the kernel's stride and the three per-query statistics
static constexpr size_t bwd_mfma_lds(int nkt, int ndt) { return (size_t)4 * nkt * 16 * (ndt * 16 * 2 + 32) + (size_t)3 * nkt * 16 * sizeof(float); }

template <int NKT, int NDT, int NW>
static int launch_bwd_mfma(const void* qkv, const void* dctx, void* dqkv, int B, int S, int heads, float scale, hipStream_t s) {
  static_assert(bwd_mfma_lds(NKT, NDT) <= kAttnLdsMax, "attention_bwd_mfma_kernel<NKT, NDT, .>: the image does not fit the LDS");
  return launch_head(attention_bwd_mfma_kernel<NKT, NDT, NW>, bwd_mfma_lds(NKT, NDT), B * heads, NW * 64, s, qkv, dctx, dqkv, S, heads, scale);
}

// ---- the ONE place that chooses a kernel (fsvit.h fsvit_op_attention_bwd_route): family * 100000 + dtype * 10000 + KT * 100 + DT, -1 = refused.
//   family 1  attention_bwd_mfma_kernel<KT, DT, .> (bf16)      2  attention_bwd_f32mfma_kernel<KT, DT>      3  attention_bwd_f32mfma_long_kernel<13, 4, 7>
//          4  attention_bwd_kernel<T> (FMA loops, all in LDS)   5  attention_bwd_tiled_f32_kernel<16>       (4 and 5: KT = DT = 0)
constexpr int kBwdTiledQB = 16;
static constexpr size_t bwd_fma_lds(int S, int hd) { return ((size_t)4 * S * (hd + 1) + (size_t)2 * S * (S + 1)) * sizeof(float); }
static constexpr size_t bwd_tiled_lds(int S, int hd) {
  return ((size_t)2 * S * (hd + 1) + (size_t)2 * kBwdTiledQB * (hd + 1) + (size_t)2 * kBwdTiledQB * (S + 1)) * sizeof(float);
}

int attention_bwd_route(int S, int hd, int hdp, int dtype) {
  if ((dtype != 0 && dtype != 1) || S < 1 || hd < 1 || hdp < hd) return -1;
  if (dtype == 1 && hdp % 32 == 0 && S <= 224) {      // bf16: MFMA kernel
    const int ndt = hdp / 16;
    // (128 tokens on 4 waves: with 8 the 512-thread bound left 256 registers per wave and the kernel spilled 228 .. 928 bytes per lane; one wave per SIMD
    //  takes accumulators in AGPRs: 311 -> 249 us at S = 100.  224: ViT, 196 patches + cls)
    const int nkt = S <= 32 ? 2 : S <= 128 ? 8 : 14;
    const bool built = nkt == 2 ? (ndt == 2 || ndt == 4 || ndt == 6 || ndt == 8) : nkt == 8 ? (ndt == 2 || ndt == 4 || ndt == 6) : (ndt == 2 || ndt == 4);
    if (built && bwd_mfma_lds(nkt, ndt) <= kAttnLdsMax) return route_id(1, 1, nkt, ndt);
  }
  if (dtype == 0 && (hdp & 3) == 0) {                 // exact-fp32 MFMA kernel where the head fits the LDS (Visformer stages: 100 x 42, 25 x 85)
    if (S <= 32 && hdp <= 48) return route_id(2, 0, 2, 3);
    if (S <= 32 && hdp <= 96) return route_id(2, 0, 2, 6);
    if (S <= 48 && hdp <= 64) return route_id(2, 0, 3, 4);
    if (S <= 112 && hdp <= 48) return route_id(2, 0, 7, 3);
    if (S <= 208 && hdp <= 64) return route_id(3, 0, 13, 4);      // ViT / DeiT: 196 patches + cls
  }
  if (bwd_fma_lds(S, hd) <= kAttnLdsMax) return route_id(4, dtype, 0, 0);
  if (dtype == 0 && bwd_tiled_lds(S, hd) <= kAttnLdsMax) return route_id(5, 0, 0, 0);
  return -1;
}

int launch_attention_bwd(const void* qkv, const void* dctx, void* dqkv, int B, int S, int heads, int hd, int hdp, float scale, int dtype, hipStream_t s) {
  if (B <= 0) return 0;
  const int route = attention_bwd_route(S, hd, hdp, dtype);
  if (route < 0) return (int)hipErrorInvalidValue;
  const AttnRoute r = route_decode(route);
  switch (r.family) {                                   // the table of instantiations: no condition of its own
    case 1:
      switch (r.kt * 100 + r.dt) {
#define BWD_MFMA(KT, DT, NW) case KT * 100 + DT: return launch_bwd_mfma<KT, DT, NW>(qkv, dctx, dqkv, B, S, heads, scale, s);
        BWD_MFMA(2, 2, 2) BWD_MFMA(2, 4, 2) BWD_MFMA(2, 6, 2) BWD_MFMA(2, 8, 2)
        BWD_MFMA(8, 2, 4) BWD_MFMA(8, 4, 4) BWD_MFMA(8, 6, 4)
        BWD_MFMA(14, 2, 4) BWD_MFMA(14, 4, 4)
#undef BWD_MFMA
      }
      break;
    case 2:
      switch (r.kt * 100 + r.dt) {
#define BWD_F32(KT, DT) case KT * 100 + DT: return launch_bwd_f32mfma<KT, DT>(qkv, dctx, dqkv, B, S, heads, hd, hdp, scale, s);
        BWD_F32(2, 3) BWD_F32(2, 6) BWD_F32(3, 4) BWD_F32(7, 3)
#undef BWD_F32
      }
      break;
    case 3:
      if (r.kt == 13 && r.dt == 4) return launch_bwd_f32mfma_long<13, 4, 7>(qkv, dctx, dqkv, B, S, heads, hd, hdp, scale, s);
      break;
    case 4:
      return with_elem(r.elem, [&](auto e) {
        return launch_head(attention_bwd_kernel<elem_t<decltype(e)>>, bwd_fma_lds(S, hd), B * heads, 256, s, qkv, dctx, dqkv, S, heads, hd, hdp, scale);
      });
    case 5:
      return launch_head(attention_bwd_tiled_f32_kernel<kBwdTiledQB>, bwd_tiled_lds(S, hd), B * heads, 256, s, qkv, dctx, dqkv, S, heads, hd, hdp, scale);
  }
  return (int)hipErrorInvalidValue;                     // a route without an instantiation is an error, never a fallback
}

}  // namespace fsvit
