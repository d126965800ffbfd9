// The strong / weak view pair of the distillation phase (sun_meta_training/datasets/mini_imagenet.py:110-124, :194-204) for a batch of uint8 weak
// views [B][80][80][3] (fsvit_image_transform_rrc_u8, transform.hip):
//   weak   = Normalize(ToTensor(view))
//   strong = RandomErasing('pixel')(Normalize(ToTensor(view or strong_transform(view))))
//   strong_transform = ColorJitter(brightness, contrast, saturation in a drawn order) -> GaussianBlur -> Solarization -> RandomGrayscale
// One workgroup per image, the image as three uint8 planes in LDS (19.2 KB) with a second copy to ping-pong the six box-blur passes (38.4 KB + the
// 3 KB Normalize table: three workgroups per CU); every stage reads and writes LDS, HBM sees 19 KB in and 154 KB out per image.  The byte arithmetic
// is Pillow's C restated (Convert.c L24, Blend.c, BoxBlur.c, ImageOps.solarize), bit-exact; the host draws every parameter (datasets/transforms.py:
// strong_weak_table) and the only randomness made here is the erase noise, a counter-based N(0, 1) keyed by (seed, image slot, channel, pixel), so a
// relaunch with the same seed reproduces the batch and no noise tensor crosses HBM.  Latency- and LDS-bound byte work; no MFMA, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pil_bytes.h"

namespace fsvit {

constexpr int SW_S = 80, SW_PIX = SW_S * SW_S;             // the view is 80 x 80 (argument error otherwise)
// columns of the int32 parameter row (datasets/transforms.py SW_*)
enum { SWC_STRONG = 0, SWC_ORDER = 1, SWC_FACTOR = 4, SWC_BLUR = 7, SWC_R = 8, SWC_WW = 9, SWC_FW = 10, SWC_SOLARIZE = 11, SWC_GRAY = 12,
       SWC_ERASE = 13, SWC_COLS = 17 };

struct StrongWeakParams {
  const uint8_t* views;        // [B][80][80][3]
  const int32_t* table;        // [B][SWC_COLS]
  float* weak;                 // [B][3][80][80]
  float* strong;               // [B][3][80][80]
  float mean[3], stdv[3];
  uint32_t seed_lo, seed_hi;
};

// Philox-4x32-10 (Salmon et al. 2011): counter (c0..c3), key (k0, k1) -> first two output words
__device__ __forceinline__ uint2 philox2(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return make_uint2(c0, c1);
}

// N(0, 1) by Box-Muller from two 24-bit uniforms in (0, 1)
__device__ __forceinline__ float normal01(uint2 r) {
  const float u1 = ((float)(r.x >> 8) + 0.5f) * (1.0f / 16777216.0f), u2 = ((float)(r.y >> 8) + 0.5f) * (1.0f / 16777216.0f);
  return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

// One box-blur pass of BoxBlur.c ImagingLineBoxBlur8 along x (STEP 1) or y (STEP 80) over the three planes, edge-clamped: r inner taps on each side at
// weight ww, the two far taps at fw, 24-bit fixed point.  (2r + 1) * ww + 2 * fw <= 2^24, so the sum stays below 2^32.
template <bool VERTICAL>
__device__ __forceinline__ void box_pass(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, int r, uint32_t ww, uint32_t fw, int t) {
  for (int i = t; i < 3 * SW_PIX; i += 256) {
    const int pl = i / SW_PIX, pix = i - pl * SW_PIX, y = pix / SW_S, x = pix - y * SW_S;
    const int pos = VERTICAL ? y : x;
    const unsigned char* line = in + pl * SW_PIX + (VERTICAL ? x : y * SW_S);
    constexpr int STEP = VERTICAL ? SW_S : 1;
    uint32_t acc = 0;
    for (int k = -r; k <= r; ++k) {
      int q = pos + k;
      q = q < 0 ? 0 : (q > SW_S - 1 ? SW_S - 1 : q);
      acc += line[q * STEP];
    }
    int ql = pos - r - 1, qr = pos + r + 1;
    ql = ql < 0 ? 0 : ql;
    qr = qr > SW_S - 1 ? SW_S - 1 : qr;
    const uint32_t far = (uint32_t)line[ql * STEP] + (uint32_t)line[qr * STEP];
    out[i] = (unsigned char)((acc * ww + far * fw + (1u << 23)) >> 24);
  }
}

__global__ __launch_bounds__(256) void strong_weak_kernel(StrongWeakParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char pa[3 * SW_PIX];      // planes R | G | B
  __shared__ __attribute__((aligned(16))) unsigned char pb[3 * SW_PIX];      // blur ping-pong
  __shared__ float lut[768];
  __shared__ int red[4];
  const int t = threadIdx.x, b = blockIdx.x;
  const int32_t* row = p.table + (size_t)b * SWC_COLS;
  load_planes<SW_PIX>(p.views + (size_t)b * 3 * SW_PIX, pa, t);      // [80][80][3] bytes (19 200, a multiple of 16) -> planes
  for (int i = t; i < 768; i += 256) {
    const int c = i >> 8;
    const float v = (float)(i & 255) / 255.0f;                        // ToTensor
    lut[i] = (v - p.mean[c]) / p.stdv[c];                              // Normalize (IEEE division, as torch does)
  }
  __syncthreads();
  // the weak view, normalised: x fastest (coalesced fp32 rows)
  float* weak = p.weak + (size_t)b * 3 * SW_PIX;
  for (int i = t; i < 3 * SW_PIX; i += 256) weak[i] = lut[(i / SW_PIX) * 256 + pa[i]];
  if (row[SWC_STRONG] != 0) {                              // every branch below is uniform over the workgroup (one parameter row per image)
    // ColorJitter: a thread owns pixels t, t + 256, ... through the point operations, so only the contrast mean needs a barrier
    for (int s = 0; s < 3; ++s) {
      const int op = row[SWC_ORDER + s];
      if (op < 0 || op > 2) continue;
      enhance_planes<SW_PIX>(pa, op, __int_as_float(row[SWC_FACTOR + op]), red, t);      // 0 brightness, 1 contrast, 2 saturation = ENH_*
    }
    if (row[SWC_BLUR] != 0) {                              // ImageFilter.GaussianBlur: three box passes along x, then three along y
      int r = row[SWC_R];
      r = r < 0 ? 0 : (r > 3 ? 3 : r);
      const uint32_t ww = (uint32_t)row[SWC_WW], fw = (uint32_t)row[SWC_FW];
      __syncthreads();
      box_pass<false>(pa, pb, r, ww, fw, t); __syncthreads();
      box_pass<false>(pb, pa, r, ww, fw, t); __syncthreads();
      box_pass<false>(pa, pb, r, ww, fw, t); __syncthreads();
      box_pass<true>(pb, pa, r, ww, fw, t); __syncthreads();
      box_pass<true>(pa, pb, r, ww, fw, t); __syncthreads();
      box_pass<true>(pb, pa, r, ww, fw, t); __syncthreads();
    }
    // after the blur's barriers (or without a blur) pixel i is again written only by thread i % 256
    if (row[SWC_SOLARIZE] != 0)                            // ImageOps.solarize(threshold 128)
      for (int i = t; i < 3 * SW_PIX; i += 256) { const int v = pa[i]; pa[i] = (unsigned char)(v < 128 ? v : 255 - v); }
    if (row[SWC_GRAY] != 0)                                // RandomGrayscale: convert('L') on all three channels
      for (int i = t; i < SW_PIX; i += 256) {
        const unsigned char l = (unsigned char)luma(pa[i], pa[SW_PIX + i], pa[2 * SW_PIX + i]);
        pa[i] = l; pa[SW_PIX + i] = l; pa[2 * SW_PIX + i] = l;
      }
  }
  // Normalize + RandomErasing('pixel'): N(0, 1) per value inside the box.  Element i is read by the thread that last wrote it (i % 256 == t, 6400 and
  // 19 200 being multiples of 256), so no barrier is needed here.
  float* strong = p.strong + (size_t)b * 3 * SW_PIX;
  const int et = row[SWC_ERASE], el = row[SWC_ERASE + 1], eh = row[SWC_ERASE + 2], ew = row[SWC_ERASE + 3];
  for (int i = t; i < 3 * SW_PIX; i += 256) {
    const int c = i / SW_PIX, pix = i - c * SW_PIX, y = pix / SW_S, x = pix - y * SW_S;
    float v = lut[c * 256 + pa[i]];
    if (eh > 0 && y >= et && y - et < eh && x >= el && x - el < ew)
      v = normal01(philox2((uint32_t)b, (uint32_t)c, (uint32_t)pix, 0u, p.seed_lo, p.seed_hi));
    strong[i] = v;
  }
}

}  // namespace fsvit

int fsvit_set_error(int code, const char* fmt, ...);      // engine.hip (library-internal, C++ linkage)

extern "C" int fsvit_image_strong_weak(const uint8_t* views_dev, int B, int H, int W, const int32_t* table_dev, int cols, const float* mean3_host,
                                       const float* std3_host, uint64_t seed, float* weak_dev, float* strong_dev, void* stream) {
  if (!views_dev || !table_dev || !mean3_host || !std3_host || !weak_dev || !strong_dev)
    return fsvit_set_error(-1, "%s", "fsvit_image_strong_weak: null argument");
  if (H != fsvit::SW_S || W != fsvit::SW_S) return fsvit_set_error(-1, "fsvit_image_strong_weak: built for 80 x 80 views, got %d x %d", H, W);
  if (cols != fsvit::SWC_COLS) return fsvit_set_error(-1, "fsvit_image_strong_weak: the parameter table has %d columns, not %d", cols, fsvit::SWC_COLS);
  if (B < 0) return fsvit_set_error(-1, "%s", "fsvit_image_strong_weak: negative batch");
  if (((uintptr_t)views_dev & 15) != 0) return fsvit_set_error(-1, "%s", "fsvit_image_strong_weak: views_dev must be 16-byte aligned");
  if (B == 0) return 0;
  fsvit::StrongWeakParams p;
  p.views = views_dev; p.table = table_dev; p.weak = weak_dev; p.strong = strong_dev;
  for (int c = 0; c < 3; ++c) { p.mean[c] = mean3_host[c]; p.stdv[c] = std3_host[c]; }
  p.seed_lo = (uint32_t)seed; p.seed_hi = (uint32_t)(seed >> 32);
  hipLaunchKernelGGL(fsvit::strong_weak_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, p);
  const int rc = (int)hipGetLastError();
  if (rc) return fsvit_set_error(rc, "%s", "fsvit_image_strong_weak: launch failed");
  return 0;
}
