// Pillow's byte arithmetic shared by the augmentation kernels (augment.hip, randaug.hip): convert('L'), Image.blend and the three ImageEnhance
// operations built on them, over an image held as three uint8 planes in LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fsvit {

__device__ __forceinline__ int luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }    // Convert.c L24

// Blend.c ImagingBlend(degenerate d, image x, alpha): one fp32 multiply, one fp32 add, then truncation when 0 <= alpha <= 1, else clamp to [0, 255]
// first.  Contraction is switched off: a fused multiply-add changes the truncation (and __fmul_rn / __fadd_rn are plain operators to this compiler,
// which it would fuse).
__device__ __forceinline__ int blend(int d, int x, float alpha, bool clamp) {
#pragma clang fp contract(off)
  const float prod = alpha * (float)(x - d);
  float t = (float)d + prod;
  if (clamp) t = t <= 0.0f ? 0.0f : (t >= 255.0f ? 255.0f : t);
  return (int)t;
}

enum { ENH_BRIGHTNESS = 0, ENH_CONTRAST = 1, ENH_COLOR = 2 };

// ImageEnhance.Brightness / Contrast / Color(factor alpha) in place on the planes pa[3][NPIX] (NPIX a multiple of 256), by 256 threads.  A thread
// owns elements t, t + 256, ... of each plane through the point operations, so only the contrast mean needs barriers (red: 4 ints of LDS).  `op` is
// uniform over the workgroup.
template <int NPIX>
__device__ __forceinline__ void enhance_planes(unsigned char* pa, int op, float alpha, int* red, int t) {
  const bool clamp = !(alpha >= 0.0f && alpha <= 1.0f);
  if (op == ENH_BRIGHTNESS) {                            // degenerate = black
    for (int i = t; i < 3 * NPIX; i += 256) pa[i] = (unsigned char)blend(0, pa[i], alpha, clamp);
  } else if (op == ENH_CONTRAST) {                       // degenerate = int(mean(L) + 0.5), the sum exact in int32
    int sum = 0;
    for (int i = t; i < NPIX; i += 256) sum += luma(pa[i], pa[NPIX + i], pa[2 * NPIX + i]);
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
    if ((t & 63) == 0) red[t >> 6] = sum;
    __syncthreads();
    const int d = (int)((double)(red[0] + red[1] + red[2] + red[3]) / (double)NPIX + 0.5);
    __syncthreads();
    for (int i = t; i < 3 * NPIX; i += 256) pa[i] = (unsigned char)blend(d, pa[i], alpha, clamp);
  } else {                                               // ImageEnhance.Color: degenerate = L
    for (int i = t; i < NPIX; i += 256) {
      const int r = pa[i], g = pa[NPIX + i], bl = pa[2 * NPIX + i], l = luma(r, g, bl);
      pa[i] = (unsigned char)blend(l, r, alpha, clamp);
      pa[NPIX + i] = (unsigned char)blend(l, g, alpha, clamp);
      pa[2 * NPIX + i] = (unsigned char)blend(l, bl, alpha, clamp);
    }
  }
}

// uint8 [NPIX][3] in HBM (16-byte aligned, 3 * NPIX a multiple of 16) -> planes pa[3][NPIX] in LDS
template <int NPIX>
__device__ __forceinline__ void load_planes(const uint8_t* __restrict__ src, unsigned char* pa, int t) {
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  for (int i = t; i < 3 * NPIX / 16; i += 256) {
    const uint4 v = s4[i];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int g = 16 * i + j, pix = g / 3, c = g - 3 * pix;
      pa[c * NPIX + pix] = (unsigned char)(w[j >> 2] >> (8 * (j & 3)));
    }
  }
}

}  // namespace fsvit
