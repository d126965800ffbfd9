// Fused Visformer stage-1 block, second design ("ring"):   y = x + conv3( GELU( conv2_g8_3x3( GELU( conv1( BN(x) ) ) ) ) )
// (test_phase/models/visformer.py:259-263 Block.forward with attn_disabled, Mlp :152-163; eval BatchNorm folded into conv1 by the packer).
//
// The first design (a half image per workgroup, all 16 waves walking the 8 channel groups in phase; retired in round 4, git history) queued the LDS
// reads (2.9 k cycles), the MFMAs (1.8 k) and the GELUs (~2 k) of a group interval behind two barriers, fed every MFMA with 1 .. 1.5 ds_read_b128 because
// the weights came from LDS, and kept the MFMA pipe busy 32 % of the time (profiles/r02_stage1_pmc.txt).  This kernel turns the decomposition
// round - the same move that took the grouped conv of the training step from 213 to 91 us (wgrad3x3.hip gconv3x3_kernel):
//   * WAVE g IS CHANNEL GROUP g for conv1 and conv2, and a (32 output channels x 32 pixels) block for conv3; all of its weights live in registers
//     for the whole launch: 8 fragments of W1 (32 hidden channels x 128), 18 of W2 (9 taps x 32 x 32), 16 of W3 (32 output channels x 256) = 168
//     VGPRs.  Only activations move through LDS: 0.5 fragment reads per MFMA;
//   * the workgroup walks the batch as ONE sequence of pixels in chunks of 64 (any image geometry with W <= 20): x and the first hidden map h1
//     live in RINGS of 128 pixel slots (slot = linear pixel index & 127, one plane per 8 channels, [plane][slot][16 B], plane pitch 2 KB).  A chunk stages only its
//     64 NEW pixels of x, computes h1 for exactly those (conv1 is pointwise: no halo recomputation), then conv2 for its 64 pixels reads the 3x3
//     neighbourhoods out of the h1 ring - a tap is an address, taps outside the image read a zero slot;
//   * h1 is written and read by the SAME wave (its group's 4 planes): no barrier between conv1 and conv2.  h2 crosses waves once (conv3 contracts
//     over all 256 hidden channels): [32 planes][64 pixels], one barrier.  The output tile goes through LDS for 16-byte coalesced stores;
//   * per chunk and wave: 32 + 72 + 32 = 136 MFMAs (the algorithmic minimum) fed by 16 + 36 + 16 fragment reads, 64 GELUs per lane (packed pairs), 4 barriers; the next chunk's x
//     batch (2 x 16 B per thread) is in flight under the MFMAs.
// Numerics: h1 and h2 are rounded to the 16-bit storage type where they are stored, everything else fp32; a pixel's value does
// not depend on its position in a chunk (batching never changes a result).
#include <stdlib.h>

#include "fsvit_common.h"
#include "kernels.h"

#ifndef S1R_UNROLL
#define S1R_UNROLL 4
#endif

#define S1R_SYNC() __syncthreads()

namespace FSVIT_NS {

namespace s1r {
constexpr int C1 = 128, HID = 256, G = 8, CH = 64, RING = 128, HALO = 21, KW2 = 320;
constexpr int PITCH = RING * 16;                // ring plane pitch: 0 mod 256 B.  A ds_read_b128 is serviced in four 16-lane groups that mix lanes of two
                                                 // lq values (MI355X_MICROARCH.md, LDS): {lq 0: rows 0-3, 12-15; lq 1: rows 4-11}, ... - with lq = plane and
                                                 // row = slot the two halves tile one 256-byte bank row exactly when the plane pitch is a multiple of it.  (The
                                                 // first build padded the planes by one slot for the staging stores: every fragment read 2-way, 48 % of the
                                                 // kernel's LDS cycles were conflicts, profiles/r02_stage1_pmc.txt)
constexpr int XR = 0;                            // x ring: 16 planes of 8 channels
constexpr int H1R = XR + (C1 / 8) * PITCH;       // h1 ring: 32 planes
constexpr int H2P = CH * 16;                     // h2 plane pitch (0 mod 256 B, as above)
constexpr int H2 = H1R + (HID / 8) * PITCH;      // h2 of the current chunk: 32 planes x 64 pixels
constexpr int OROW = C1 * 2 + 16;                // output tile row pitch (272 B: conflict-free 8-byte column writes)
constexpr int OUT = H2 + (HID / 8) * H2P;        // output tile [64 pixels][128 channels]
constexpr int ZERO = OUT + CH * OROW;            // 16 zero bytes
constexpr int BIAS = ZERO + 16;                  // MODE 3: conv1's folded bias [256] fp32 (8 VGPRs the training variant does not have)
constexpr int LDS_BYTES = BIAS + HID * 4;        // 149 520
}  // namespace s1r

typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_r;

__device__ __forceinline__ u32x2_r s1r_pack4(f32x4 v) {
  const bf16x4 o = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
  return __builtin_bit_cast(u32x2_r, o);
}
__device__ __forceinline__ u32x4 s1r_pack8(f32x4 a, f32x4 b) {
  const bf16x8 o = {(bf16)a[0], (bf16)a[1], (bf16)a[2], (bf16)a[3], (bf16)b[0], (bf16)b[1], (bf16)b[2], (bf16)b[3]};
  return __builtin_bit_cast(u32x4, o);
}
__device__ __forceinline__ f32x4 s1r_gelu4(f32x4 v) {
  const f32x2 a = gelu_sig2(f32x2{v[0], v[1]}), b = gelu_sig2(f32x2{v[2], v[3]});
  return f32x4{a[0], a[1], b[0], b[1]};
}

// The training kernels' HBM maps ([M][256] each): MODE 3 writes the hidden maps h1 / h2 and the GELU derivatives g1 / g2 at their pre-activations for
// the backward pass; MODE 2 reads the derivatives and writes dz2 / dz1.
struct S1Train { bf16 *h1, *g1, *h2, *g2; };
// MODE 3 (the training forward of a whole stage-1 BLOCK, train_engine.hip): x = the block's RAW input, the batch-statistics BatchNorm folded into conv1
// exactly as the eval engine folds the running statistics (w1 = W1 diag(sa) rounded once, b1 = W1 sb; fold_prenorm_kernel makes them after the
// BatchNorm's finalize), the residual from the x ring with the block's DropPath scale per image: y = x + scale[image] * conv3(h2).  Also written:
// h1 / g1 / h2 / g2 and the normalised input xn = sa x + sb of the workgroup's own pixels (the backward's weight-gradient operand).  `stats` is not
// written: the output statistics from this kernel cost 16 VGPRs more than it has (train_engine.hip).
struct S1Fused { bf16* xn; const float *sa, *sb, *scale; float* stats; };
__device__ __forceinline__ void s1r_gelu4_d(f32x4 v, f32x4& h, f32x4& d) {
  f32x2 da, db;
  const f32x2 a = gelu_sig2_d(f32x2{v[0], v[1]}, da), b = gelu_sig2_d(f32x2{v[2], v[3]}, db);
  h = f32x4{a[0], a[1], b[0], b[1]};
  d = f32x4{da[0], da[1], db[0], db[1]};
}

// MODE 2 (the block's data-gradient chain, train_engine.hip): the SAME ring walk over the transposed packs - x = dz3, "conv1" = W3^T (128 -> 256)
// times g2' -> dz2, "conv2" = the grouped 3x3 with flipped taps times g1' -> dz1, "conv3" = W1^T (256 -> 128) -> d(xn); the multipliers come from HBM
// ([M][256], the derivatives the forward variant stored), dz2 / dz1 go to HBM for the weight gradients (tr.h1 = dz2, tr.h2 = dz1; tr.g1 = g2', tr.g2 = g1').
template <int MODE>
__device__ __forceinline__ void stage1_ring_body(const bf16* __restrict__ x, bf16* __restrict__ y, const bf16* __restrict__ w1,
                                                 const float* __restrict__ b1, const bf16* __restrict__ w2, const bf16* __restrict__ w3, int M,
                                                 int H, int W, int n_chunks, int chunks_per_wg, const S1Train tr, const S1Fused fu = S1Fused{}) {
  using namespace s1r;
  constexpr bool FUSED = MODE == 3;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x, lane = t & 63, lrow = lane & 15, lq = lane >> 4;
  const int g = __builtin_amdgcn_readfirstlane(t >> 6);
  const int q0 = blockIdx.x * chunks_per_wg;
  int q1 = q0 + chunks_per_wg; q1 = q1 < n_chunks ? q1 : n_chunks;
  if (q0 >= q1) return;
  if (t < 4) reinterpret_cast<unsigned*>(smem + ZERO)[t] = 0u;

  // ---- this wave's weights (A operands: row = output channel of the product, 8 consecutive k per lane)
  u32x4 wf1[2][4], wf2[9][2], wf3[2][8];
  const int np3 = g >> 1, ph3 = g & 1;          // conv3: this wave = output channels 32 np3 .. + 31 of the pixel tiles 2 ph3, 2 ph3 + 1
  // Which channel of a 32-channel block sits in which MFMA row is the loader's choice: row R of tile nt carries channel 8 (R >> 2) + 4 nt + (R & 3),
  // so the 4 + 4 accumulators a lane holds of the tile pair are 8 CONSECUTIVE channels 8 lq .. 8 lq + 7 of its pixel = one 16-byte slot of plane lq:
  // h1 / h2 / the output tile are written with ds_write_b128 (8 lanes = 128 contiguous bytes, conflict-free) instead of two 8-byte stores whose
  // 16-lane groups met 2-way on the banks (28.6 % of the kernel's LDS cycles, profiles/r02_stage1_pmc.txt), and the residual is one 16-byte read.
  const int prow = 8 * (lrow >> 2) + (lrow & 3);
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) wf1[nt][kc] = *reinterpret_cast<const u32x4*>(w1 + (size_t)(g * 32 + prow + 4 * nt) * C1 + kc * 32 + lq * 8);
#pragma unroll
  for (int tp = 0; tp < 9; ++tp)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) wf2[tp][nt] = *reinterpret_cast<const u32x4*>(w2 + (size_t)(g * 32 + prow + 4 * nt) * KW2 + tp * 32 + lq * 8);
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int kc = 0; kc < 8; ++kc) wf3[nt][kc] = *reinterpret_cast<const u32x4*>(w3 + (size_t)(np3 * 32 + prow + 4 * nt) * HID + kc * 32 + lq * 8);
  f32x4 bias1[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  if constexpr (MODE == 0) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) bias1[nt] = *reinterpret_cast<const f32x4*>(b1 + g * 32 + lq * 8 + nt * 4);
  }
  if constexpr (FUSED) {
    if (t < HID) reinterpret_cast<float*>(smem + BIAS)[t] = b1[t];      // (visible after the first barrier below)
  }
  const long own_lo = (long)q0 * CH;                                   // MODE 2 / 3: this workgroup stores h1 / g1 of its OWN pixels only (the halo is recomputed by the neighbours)
  long own_hi = (long)q1 * CH; own_hi = own_hi < M ? own_hi : M;

  // ---- x batches: 64 consecutive pixels from linear index P0 (pixels outside [0, M) are stored as zeros); 2 x 16 B per thread
  u32x4 px[2];
  unsigned pxok = 0;
  auto gload = [&](long P0) {
    pxok = 0;
#pragma unroll
    for (int u0 = 0; u0 < 2; ++u0) {
      const int u = t + 512 * u0, p = (u & 7) + 8 * (u >> 7), c8 = (u >> 3) & 15;      // 8 consecutive lanes = 8 consecutive pixels of one plane: the
      const long m = P0 + p;                                                             // 16-byte stores of a lane group fill 128 contiguous LDS bytes
      const bool ok = m >= 0 && m < M;
      px[u0] = *reinterpret_cast<const u32x4*>(x + (size_t)(ok ? m : 0) * C1 + c8 * 8);      // unconditional, clamped (no exec-masked branch per load)
      pxok |= ok ? (1u << u0) : 0u;
    }
  };
  auto lstore = [&](long P0) {
#pragma unroll
    for (int u0 = 0; u0 < 2; ++u0) {
      const int u = t + 512 * u0, p = (u & 7) + 8 * (u >> 7), c8 = (u >> 3) & 15;
      const u32x4 v = ((pxok >> u0) & 1u) ? px[u0] : u32x4{0u, 0u, 0u, 0u};
      *reinterpret_cast<u32x4*>(smem + XR + c8 * PITCH + (int)((P0 + p) & (RING - 1)) * 16) = v;
      if constexpr (FUSED) {             // the normalised input of the workgroup's own pixels, for the backward pass (c8 is the same for both u0)
        const long m = P0 + p;
        if (m >= own_lo && m < own_hi) {
          const f32x4 a0 = *reinterpret_cast<const f32x4*>(fu.sa + c8 * 8), a1 = *reinterpret_cast<const f32x4*>(fu.sa + c8 * 8 + 4);
          const f32x4 s0 = *reinterpret_cast<const f32x4*>(fu.sb + c8 * 8), s1 = *reinterpret_cast<const f32x4*>(fu.sb + c8 * 8 + 4);
          const bf16x8 r = __builtin_bit_cast(bf16x8, v);
          *reinterpret_cast<u32x4*>(fu.xn + (size_t)m * C1 + c8 * 8) =
              s1r_pack8(f32x4{(float)r[0], (float)r[1], (float)r[2], (float)r[3]} * a0 + s0, f32x4{(float)r[4], (float)r[5], (float)r[6], (float)r[7]} * a1 + s1);
        }
      }
    }
  };
  // conv1 + bias + GELU for the 64 pixels from P0: wave g computes hidden channels 32 g .. 32 g + 31 into ITS planes of the h1 ring
  const unsigned char* const xplane = smem + XR + lq * PITCH;                 // k-chunk kc adds 4 planes
  unsigned char* const h1w = smem + H1R + (g * 4 + lq) * PITCH;                           // this lane's 8 channels = plane lq of the group
  auto conv1 = [&](long P0) {
    // MODE 2: the multipliers of the batch's four tiles are requested up front (a load issued in a tile's epilogue right before its use exposed one
    // HBM latency per tile)
    u32x4 mgp[MODE == 2 ? CH / 16 : 1];
    if constexpr (MODE == 2) {
#pragma unroll
      for (int mt = 0; mt < CH / 16; ++mt) {
        const long pp = P0 + mt * 16 + lrow;
        mgp[mt] = *reinterpret_cast<const u32x4*>(tr.g1 + (size_t)(pp >= 0 && pp < M ? pp : 0) * HID + g * 32 + lq * 8);
      }
    }
#pragma unroll S1R_UNROLL
    for (int mt = 0; mt < CH / 16; ++mt) {
      const int slot = (int)((P0 + mt * 16 + lrow) & (RING - 1)) * 16;
      f32x4 acc[2] = {bias1[0], bias1[1]};
      if constexpr (FUSED) {
        acc[0] = *reinterpret_cast<const f32x4*>(smem + BIAS + (g * 32 + lq * 8) * 4);
        acc[1] = *reinterpret_cast<const f32x4*>(smem + BIAS + (g * 32 + lq * 8 + 4) * 4);
      }
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        const u32x4 xf = *reinterpret_cast<const u32x4*>(xplane + kc * (4 * PITCH) + slot);
        acc[0] = mma_chunk<bf16>(wf1[0][kc], xf, acc[0]);
        acc[1] = mma_chunk<bf16>(wf1[1][kc], xf, acc[1]);
      }
      if constexpr (MODE == 2) {
        const long pp = P0 + mt * 16 + lrow;
        const bool inr = pp >= 0 && pp < M;
        const size_t o = (size_t)(inr ? pp : 0) * HID + g * 32 + lq * 8;
        const bf16x8 mg = __builtin_bit_cast(bf16x8, mgp[mt]);
        const u32x4 hp = s1r_pack8(acc[0] * f32x4{(float)mg[0], (float)mg[1], (float)mg[2], (float)mg[3]},
                                   acc[1] * f32x4{(float)mg[4], (float)mg[5], (float)mg[6], (float)mg[7]});
        *reinterpret_cast<u32x4*>(h1w + slot) = hp;
        if (pp >= own_lo && pp < own_hi) *reinterpret_cast<u32x4*>(tr.h1 + o) = hp;
      } else if constexpr (FUSED) {
        f32x4 h0, h1v, d0, d1;
        s1r_gelu4_d(acc[0], h0, d0);
        s1r_gelu4_d(acc[1], h1v, d1);
        const u32x4 hp = s1r_pack8(h0, h1v);
        *reinterpret_cast<u32x4*>(h1w + slot) = hp;
        const long pp = P0 + mt * 16 + lrow;
        if (pp >= own_lo && pp < own_hi) {
          const size_t o = (size_t)pp * HID + g * 32 + lq * 8;
          *reinterpret_cast<u32x4*>(tr.h1 + o) = hp;
          *reinterpret_cast<u32x4*>(tr.g1 + o) = s1r_pack8(d0, d1);
        }
      } else {
        *reinterpret_cast<u32x4*>(h1w + slot) = s1r_pack8(s1r_gelu4(acc[0]), s1r_gelu4(acc[1]));
      }
    }
  };

  const unsigned char* const h1plane = smem + H1R + (g * 4 + lq) * PITCH;      // conv2 B operand: channels 32 g + 8 lq .. of a pixel
  unsigned char* const h2w = smem + H2 + (g * 4 + lq) * H2P;
  const unsigned char* const h2plane = smem + H2 + lq * H2P;                   // conv3 B operand: k-chunk kc adds 4 planes
  const unsigned char* const xres = smem + XR + (np3 * 4 + lq) * PITCH;          // residual: channels 32 np3 + 8 lq .. + 7 of a pixel
  unsigned char* const outw = smem + OUT + (np3 * 32 + lq * 8) * 2;
  const int HW = H * W;

  // ---- the first window: x pixels [64 q0 - 21, 64 q0 + 107) = the whole ring in two batches; h1 of the first batch here, of the second in the loop
  gload((long)q0 * CH - HALO);
  lstore((long)q0 * CH - HALO);
  gload((long)q0 * CH - HALO + CH);
  __syncthreads();
  conv1((long)q0 * CH - HALO);

  for (int q = q0; q < q1; ++q) {
    const long Pn = (long)q * CH - HALO + CH;                       // the 64 pixels this chunk adds: [64 q + 43, 64 q + 107)
    S1R_SYNC();                                                // A: the previous chunk's h2 / output tile / oldest ring slots are free
    lstore(Pn);
    S1R_SYNC();                                                // B: the new x pixels are visible
    if (q + 1 < q1) gload(Pn + CH);
    conv1(Pn);

    // conv2 (grouped 3x3) + GELU for pixels [64 q, 64 q + 64): taps out of this wave's own h1 planes
    const int m0 = q * CH;
    int oyc, oxc;
    {
      const int mm = m0 + lrow, rem = mm % HW;
      oyc = rem / W;
      oxc = rem - oyc * W;
    }
    u32x4 mgq[MODE == 2 ? CH / 16 : 1];                              // MODE 2: the chunk's g1' multipliers, requested before the tap loops
    if constexpr (MODE == 2) {
#pragma unroll
      for (int mt = 0; mt < CH / 16; ++mt) {
        const int mm = m0 + mt * 16 + lrow;
        mgq[mt] = *reinterpret_cast<const u32x4*>(tr.g2 + (size_t)(mm < M ? mm : 0) * HID + g * 32 + lq * 8);
      }
    }
#pragma unroll S1R_UNROLL
    for (int mt = 0; mt < CH / 16; ++mt) {
      const int m = m0 + mt * 16 + lrow;
      const int oy = m < M ? oyc : -4, ox = oxc;
      oxc += 16;
      while (oxc >= W) { oxc -= W; ++oyc; }
      if (oyc >= H) oyc -= H;
      f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int tp = 0; tp < 9; ++tp) {
        const int dy = tp / 3 - 1, dx = tp % 3 - 1;
        const bool ok = (unsigned)(oy + dy) < (unsigned)H && (unsigned)(ox + dx) < (unsigned)W;
        const u32x4 hf = *reinterpret_cast<const u32x4*>(ok ? h1plane + ((m + dy * W + dx) & (RING - 1)) * 16 : smem + ZERO);
        acc[0] = mma_chunk<bf16>(wf2[tp][0], hf, acc[0]);
        acc[1] = mma_chunk<bf16>(wf2[tp][1], hf, acc[1]);
      }
      if constexpr (MODE == 2) {
        const size_t o = (size_t)(m < M ? m : 0) * HID + g * 32 + lq * 8;
        const bf16x8 mg = __builtin_bit_cast(bf16x8, mgq[mt]);
        const u32x4 hp = s1r_pack8(acc[0] * f32x4{(float)mg[0], (float)mg[1], (float)mg[2], (float)mg[3]},
                                   acc[1] * f32x4{(float)mg[4], (float)mg[5], (float)mg[6], (float)mg[7]});
        *reinterpret_cast<u32x4*>(h2w + (mt * 16 + lrow) * 16) = hp;
        if (m < M) *reinterpret_cast<u32x4*>(tr.h2 + o) = hp;
      } else if constexpr (FUSED) {
        f32x4 h0, h1v, d0, d1;
        s1r_gelu4_d(acc[0], h0, d0);
        s1r_gelu4_d(acc[1], h1v, d1);
        const u32x4 hp = s1r_pack8(h0, h1v);
        *reinterpret_cast<u32x4*>(h2w + (mt * 16 + lrow) * 16) = hp;
        if (m < M) {
          const size_t o = (size_t)m * HID + g * 32 + lq * 8;
          *reinterpret_cast<u32x4*>(tr.h2 + o) = hp;
          *reinterpret_cast<u32x4*>(tr.g2 + o) = s1r_pack8(d0, d1);
        }
      } else {
        *reinterpret_cast<u32x4*>(h2w + (mt * 16 + lrow) * 16) = s1r_pack8(s1r_gelu4(acc[0]), s1r_gelu4(acc[1]));
      }
    }
    S1R_SYNC();                                                // C: h2 of all groups is complete

    // conv3 + residual: 32 output channels x 32 pixels per wave (an h2 fragment feeds two MFMAs: with 16 channels x 64 pixels per wave every
    // fragment fed one, and the 8 waves read the whole h2 tile eight times instead of four)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const int mt = ph3 * 2 + mi;
      f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int kc = 0; kc < 8; ++kc) {
        const u32x4 hf = *reinterpret_cast<const u32x4*>(h2plane + kc * (4 * H2P) + (mt * 16 + lrow) * 16);
        acc[0] = mma_chunk<bf16>(wf3[0][kc], hf, acc[0]);
        acc[1] = mma_chunk<bf16>(wf3[1][kc], hf, acc[1]);
      }
      if constexpr (MODE == 0) {
        const int m = m0 + mt * 16 + lrow;
        const bf16x8 r = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(xres + (m & (RING - 1)) * 16));
        acc[0] += f32x4{(float)r[0], (float)r[1], (float)r[2], (float)r[3]};
        acc[1] += f32x4{(float)r[4], (float)r[5], (float)r[6], (float)r[7]};
      }
      if constexpr (FUSED) {
        const int m = m0 + mt * 16 + lrow;
        const bool inr = m < M;
        const float sc = fu.scale ? fu.scale[(inr ? m : 0) / HW] : 1.0f;
        const bf16x8 r = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(xres + (m & (RING - 1)) * 16));
        acc[0] = acc[0] * sc + f32x4{(float)r[0], (float)r[1], (float)r[2], (float)r[3]};
        acc[1] = acc[1] * sc + f32x4{(float)r[4], (float)r[5], (float)r[6], (float)r[7]};
      }
      *reinterpret_cast<u32x4*>(outw + (mt * 16 + lrow) * OROW) = s1r_pack8(acc[0], acc[1]);
    }
    S1R_SYNC();                                                // D: the output tile is complete
#pragma unroll
    for (int u0 = 0; u0 < 2; ++u0) {
      const int u = t + 512 * u0, p = u >> 4, c8 = u & 15;
      const long m = (long)m0 + p;
      if (m < M) *reinterpret_cast<u32x4*>(y + (size_t)m * C1 + c8 * 8) = *reinterpret_cast<const u32x4*>(smem + OUT + p * OROW + c8 * 16);
    }
  }
}

__global__ __launch_bounds__(512, 1) void stage1_ring_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, const bf16* __restrict__ w1,
                                                             const float* __restrict__ b1, const bf16* __restrict__ w2, const bf16* __restrict__ w3, int M,
                                                             int H, int W, int n_chunks, int chunks_per_wg) {
  stage1_ring_body<0>(x, y, w1, b1, w2, w3, M, H, W, n_chunks, chunks_per_wg, S1Train{nullptr, nullptr, nullptr, nullptr});
}
__global__ __launch_bounds__(512, 1) void stage1_ring_dgrad_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, const bf16* __restrict__ w1,
                                                                   const bf16* __restrict__ w2, const bf16* __restrict__ w3, int M, int H, int W, int n_chunks,
                                                                   int chunks_per_wg, const S1Train tr) {
  stage1_ring_body<2>(x, y, w1, nullptr, w2, w3, M, H, W, n_chunks, chunks_per_wg, tr);
}

__global__ __launch_bounds__(512, 1) void stage1_ring_block_train_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, const bf16* __restrict__ w1,
                                                                         const float* __restrict__ b1, const bf16* __restrict__ w2, const bf16* __restrict__ w3, int M,
                                                                         int H, int W, int n_chunks, int chunks_per_wg, const S1Train tr, const S1Fused fu) {
  stage1_ring_body<3>(x, y, w1, b1, w2, w3, M, H, W, n_chunks, chunks_per_wg, tr, fu);
}

bool stage1_ring_supported(int dtype, int C1, int hid, int group, int H1) {
  return dtype == 1 && C1 == s1r::C1 && hid == s1r::HID && group == s1r::G && H1 >= 4 && H1 <= 20;
}
// The engines run the block as one launch for every supported map (stage1_w4.hip in eval; this file's kernels in the training modes and behind
// fsvit_stage1_block).  Other geometries and numerics modes take the three-launch route (conv1 / grouped conv2 / conv3 through the GEMM kernels).
// w1 [256][128], w2 [256][320] (columns (tap, c)), w3 [128][256]: the packed layers of the block (engine.hip pack_layer); w3s: 8 x w3 or null
int launch_stage1_ring(const void* x, void* y, const void* w1, const float* b1, const void* w2, const void* w3, int B, int H, int W, hipStream_t s, const void* w3s) {
  return launch_stage1_w4(x, y, w1, b1, w2, w3, B, H, W, s, w3s);
}
// persistent grid: one 8-wave workgroup per CU (150 KB of LDS), the chunks spread evenly; returns the number of 64-pixel chunks
static inline int s1r_grid(int M, int* wgs, int* cpw) {
  const int n_chunks = (M + s1r::CH - 1) / s1r::CH;
  int w = n_chunks < 256 ? n_chunks : 256;
  *cpw = (n_chunks + w - 1) / w;
  *wgs = (n_chunks + *cpw - 1) / *cpw;
  return n_chunks;
}
// this file's kernel (fsvit_stage1_block: the cross-check of the two kernels in one process)
int launch_stage1_ring16(const void* x, void* y, const void* w1, const float* b1, const void* w2, const void* w3, int B, int H, int W, hipStream_t s) {
  const long Ml = (long)B * H * W;
  if (Ml <= 0) return 0;
  if (Ml >= (1L << 31) - 256 || W > 20 || H * W < 16) return (int)hipErrorInvalidValue;
  const int M = (int)Ml;
  int wgs, cpw;
  const int n_chunks = s1r_grid(M, &wgs, &cpw);
  {    // per launch: the attribute is per DEVICE (a process-wide "done" flag skipped it on a second GPU), and the call is cheap
    hipError_t e = hipFuncSetAttribute((const void*)stage1_ring_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, s1r::LDS_BYTES);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(stage1_ring_kernel, dim3(wgs), dim3(512), s1r::LDS_BYTES, s, (const bf16*)x, (bf16*)y, (const bf16*)w1, b1, (const bf16*)w2, (const bf16*)w3, M, H, W,
                     n_chunks, cpw);
  return (int)hipGetLastError();
}

// Training forward of a whole stage-1 block (MODE 3, see S1Fused): x [M][128] raw block input, w1f / b1f = conv1 with the batch-statistics BatchNorm folded
// (fold_prenorm), scale = DropPath scale per image or NULL, out = x + scale * conv3(...), xn = sa x + sb; h1 / g1 / h2 / g2 [M][256].
int launch_stage1_ring_block_train(const void* x, void* out, const void* w1f, const float* b1f, const void* w2, const void* w3, void* h1, void* g1, void* h2, void* g2,
                                   void* xn, const float* sa, const float* sb, const float* scale, float* stats, int B, int H, int W, hipStream_t s) {
  const long Ml = (long)B * H * W;
  if (Ml <= 0) return 0;
  if (Ml >= (1L << 31) - 256 || W > 20 || H * W < 16 || x == out) return (int)hipErrorInvalidValue;
  const int M = (int)Ml;
  int wgs, cpw;
  const int n_chunks = s1r_grid(M, &wgs, &cpw);
  hipError_t e = hipFuncSetAttribute((const void*)stage1_ring_block_train_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, s1r::LDS_BYTES);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(stage1_ring_block_train_kernel, dim3(wgs), dim3(512), s1r::LDS_BYTES, s, (const bf16*)x, (bf16*)out, (const bf16*)w1f, b1f, (const bf16*)w2, (const bf16*)w3,
                     M, H, W, n_chunks, cpw, S1Train{(bf16*)h1, (bf16*)g1, (bf16*)h2, (bf16*)g2}, S1Fused{(bf16*)xn, sa, sb, scale, stats});
  return (int)hipGetLastError();
}
// data-gradient chain of the block: dz3 [M][128] -> dz2 = (dz3 W3) * g2', dz1 = (grouped conv^T of dz2) * g1', dxn = dz1 W1  (w3t / w2t / w1t: the transposed
// ("dgrad") packs [256][128], [256][320] tap-flipped, [128][256]); dxn must not alias dz3
int launch_stage1_ring_dgrad(const void* dz3, void* dxn, const void* w3t, const void* w2t, const void* w1t, const void* g2, const void* g1, void* dz2, void* dz1,
                             int B, int H, int W, hipStream_t s) {
  const long Ml = (long)B * H * W;
  if (Ml <= 0) return 0;
  if (Ml >= (1L << 31) - 256 || W > 20 || H * W < 16 || dz3 == dxn) return (int)hipErrorInvalidValue;
  const int M = (int)Ml;
  int wgs, cpw;
  const int n_chunks = s1r_grid(M, &wgs, &cpw);
  hipError_t e = hipFuncSetAttribute((const void*)stage1_ring_dgrad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, s1r::LDS_BYTES);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(stage1_ring_dgrad_kernel, dim3(wgs), dim3(512), s1r::LDS_BYTES, s, (const bf16*)dz3, (bf16*)dxn, (const bf16*)w3t, (const bf16*)w2t, (const bf16*)w1t, M, H,
                     W, n_chunks, cpw, S1Train{(bf16*)dz2, (bf16*)g2, (bf16*)dz1, (bf16*)g1});
  return (int)hipGetLastError();
}

}  // namespace FSVIT_NS
