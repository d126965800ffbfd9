// RandAugment ('rand-m9-mstd0.5-inc1', timm) in place on a batch of uint8 views [B][80][80][3] (fsvit_image_transform_rrc_u8, transform.hip): the
// weak view's RandomApply([RandAugment], p = 0.2) of the distillation phase (sun_meta_training/datasets/mini_imagenet.py:91-108) and the RandAugment
// stage of the classifier phase's timm pipeline.  One workgroup per LISTED image - the host passes the indices of the images that have an operation to
// apply, the others are never read or written - with the image as three uint8 planes in LDS and a second copy (38.4 KB, as in augment.hip) for the
// two operations that read neighbours (the affine resampling and the 3 x 3 smoothing), a 3 x 256 int32 histogram and a 768-byte point table.  Two
// operation slots per image, applied in order.  The byte arithmetic is Pillow's C and Python restated (Geometry.c affine_transform +
// bicubic_filter32RGB, ImageOps.autocontrast / equalize, ImageEnhance, Filter.c ImagingFilter3x3), bit-exact: float64 / float32 exactly where
// Pillow uses them, contraction off (the x86 build has no FMA and a fused multiply-add moves the truncation).  The host maps timm's fifteen named
// operations and their magnitudes onto the codes below (datasets/transforms.py: rand_augment_op) and validates every row.  Every branch is uniform
// over the workgroup; the per-pixel cases (outside the source, border, rows past the edge) are selects.  No MFMA, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pil_bytes.h"

namespace fsvit {

constexpr int RA_S = 80, RA_PIX = RA_S * RA_S;             // the view is 80 x 80 (argument error otherwise)
// one operation slot of the int32 parameter row (datasets/transforms.py RA_*): code, argument, six float64 coefficients
enum { RAC_CODE = 0, RAC_ARG = 1, RAC_COEF = 2, RAC_OP_COLS = 14, RAC_SLOTS = 2, RAC_COLS = RAC_SLOTS * RAC_OP_COLS };
enum { RA_NONE = 0, RA_AFFINE, RA_INVERT, RA_POSTERIZE, RA_SOLARIZE, RA_SOLARIZE_ADD, RA_AUTOCONTRAST, RA_EQUALIZE, RA_COLOR, RA_CONTRAST,
       RA_BRIGHTNESS, RA_SHARPNESS };

struct RandAugParams {
  uint8_t* views;              // [B][80][80][3], in place
  const int32_t* slots;        // [n_slots] image indices
  const int32_t* table;        // [n_slots][RAC_COLS]
  int B;
  int fill[3];
};

// Geometry.c BICUBIC: not the resize filter
__device__ __forceinline__ double geometry_cubic(double v1, double v2, double v3, double v4, double d) {
#pragma clang fp contract(off)
  const double p1 = v2, p2 = -v1 + v3, p3 = 2 * (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}

// Image.transform(size, AFFINE, a, BICUBIC, fillcolor): in -> out, both three planes
__device__ __forceinline__ void affine_pass(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, const double* a, const int* fill,
                                            int t) {
#pragma clang fp contract(off)
  for (int pix = t; pix < RA_PIX; pix += 256) {
    const int y = pix / RA_S, x = pix - y * RA_S;
    const double xc = (double)x + 0.5, yc = (double)y + 0.5;
    double xin = a[0] * xc + a[1] * yc + a[2];
    double yin = a[3] * xc + a[4] * yc + a[5];
    const bool inside = xin >= 0.0 && xin < (double)RA_S && yin >= 0.0 && yin < (double)RA_S;      // false for a NaN too
    xin = (inside ? xin : 0.5) - 0.5;
    yin = (inside ? yin : 0.5) - 0.5;
    const double fxd = floor(xin), fyd = floor(yin);
    const double dx = xin - fxd, dy = yin - fyd;
    const int fx = (int)fxd, fy = (int)fyd;                // in [-1, 79]
    int col[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = fx - 1 + k;
      col[k] = c < 0 ? 0 : (c > RA_S - 1 ? RA_S - 1 : c);
    }
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
      const unsigned char* plane = in + pl * RA_PIX;
      double v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {                        // the first row is clamped; a later row outside the image repeats the previous value
        const int r = fy - 1 + j;
        const int rc = r < 0 ? 0 : (r > RA_S - 1 ? RA_S - 1 : r);
        const unsigned char* line = plane + rc * RA_S;
        const double h = geometry_cubic((double)line[col[0]], (double)line[col[1]], (double)line[col[2]], (double)line[col[3]], dx);
        v[j] = (j == 0 || (r >= 0 && r < RA_S)) ? h : v[j > 0 ? j - 1 : 0];
      }
      const double r = geometry_cubic(v[0], v[1], v[2], v[3], dy);
      const int byte = r <= 0.0 ? 0 : (r >= 255.0 ? 255 : (int)r);                                   // truncation
      out[pl * RA_PIX + pix] = (unsigned char)(inside ? byte : fill[pl]);
    }
  }
}

// filter(ImageFilter.SMOOTH) (Filter.c ImagingFilter3x3, kernel (1 1 1 / 1 5 1 / 1 1 1) / 13 as float32): in -> out.  The 1-pixel border is copied;
// inside, the float32 sum starts at 0.5 and takes the rows y + 1, y, y - 1, each row's three products added first.
__device__ __forceinline__ void smooth_pass(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, int t) {
#pragma clang fp contract(off)
  const float k1 = (float)(1.0 / 13.0), k5 = (float)(5.0 / 13.0);
  for (int i = t; i < 3 * RA_PIX; i += 256) {
    const int pl = i / RA_PIX, pix = i - pl * RA_PIX, y = pix / RA_S, x = pix - y * RA_S;
    const bool inner = x > 0 && x < RA_S - 1 && y > 0 && y < RA_S - 1;
    const int xc = inner ? x : 1, yc = inner ? y : 1;      // a border thread computes a value it does not keep, inside the plane
    const unsigned char* c = in + pl * RA_PIX + yc * RA_S + xc;
    float ss = 0.5f;
    ss += (float)c[RA_S - 1] * k1 + (float)c[RA_S] * k1 + (float)c[RA_S + 1] * k1;
    ss += (float)c[-1] * k1 + (float)c[0] * k5 + (float)c[1] * k1;
    ss += (float)c[-RA_S - 1] * k1 + (float)c[-RA_S] * k1 + (float)c[-RA_S + 1] * k1;
    const int byte = ss <= 0.0f ? 0 : (ss >= 255.0f ? 255 : (int)ss);
    out[i] = (unsigned char)(inner ? byte : in[i]);
  }
}

__global__ __launch_bounds__(256) void rand_augment_kernel(RandAugParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char planes[2 * 3 * RA_PIX];      // R | G | B, and the second copy
  __shared__ int hist[768];
  __shared__ unsigned char lut[768];
  __shared__ int red[4];
  __shared__ int lohi[6];
  const int t = threadIdx.x;
  const int b = p.slots[blockIdx.x];
  if (b < 0 || b >= p.B) return;                           // (the host validates the list; whatever it holds, nothing outside the batch is touched)
  const int32_t* row = p.table + (size_t)blockIdx.x * RAC_COLS;
  uint8_t* view = p.views + (size_t)b * 3 * RA_PIX;
  int co = 0;                                              // the current copy starts at planes + co, the other one at planes + (3 * RA_PIX - co)
  load_planes<RA_PIX>(view, planes, t);
  __syncthreads();
  // Every operation starts and ends with the current copy complete and visible to all threads; `code` is uniform over the workgroup.
  for (int s = 0; s < RAC_SLOTS; ++s) {
    const int32_t* op = row + s * RAC_OP_COLS;
    const int code = op[RAC_CODE], arg = op[RAC_ARG];
    unsigned char* cur = planes + co;
    unsigned char* alt = planes + (3 * RA_PIX - co);
    if (code == RA_AFFINE) {
      double a[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) a[k] = __hiloint2double(op[RAC_COEF + 2 * k + 1], op[RAC_COEF + 2 * k]);
      affine_pass(cur, alt, a, p.fill, t);
      co = 3 * RA_PIX - co;
      __syncthreads();
    } else if (code >= RA_INVERT && code <= RA_EQUALIZE) { // a point table per channel, built by thread i for value i
      if (code == RA_AUTOCONTRAST || code == RA_EQUALIZE) {
        for (int i = t; i < 768; i += 256) hist[i] = 0;
        if (t < 3) { lohi[t] = 255; lohi[3 + t] = 0; }
        __syncthreads();
        for (int i = t; i < 3 * RA_PIX; i += 256) atomicAdd(&hist[(i / RA_PIX) * 256 + cur[i]], 1);    // integer: order-independent
        __syncthreads();
      }
      if (code == RA_AUTOCONTRAST) {                       // ImageOps.autocontrast(cutoff 0): lo / hi = lowest / highest occupied value
        for (int c = 0; c < 3; ++c)
          if (hist[c * 256 + t] > 0) { atomicMin(&lohi[c], t); atomicMax(&lohi[3 + c], t); }
        __syncthreads();
        for (int c = 0; c < 3; ++c) {
#pragma clang fp contract(off)
          const int lo = lohi[c], hi = lohi[3 + c];
          int v = t;
          if (hi > lo) {
            const double scale = 255.0 / (double)(hi - lo), offset = (double)(-lo) * scale;
            v = (int)((double)t * scale + offset);
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
          }
          lut[c * 256 + t] = (unsigned char)v;
        }
      } else if (code == RA_EQUALIZE) {                    // ImageOps.equalize: every thread scans the 256 counts (LDS broadcasts)
        for (int c = 0; c < 3; ++c) {
          int before = 0, occupied = 0, last = 0;
          for (int j = 0; j < 256; ++j) {
            const int h = hist[c * 256 + j];
            before += j < t ? h : 0;
            occupied += h > 0 ? 1 : 0;
            last = h > 0 ? h : last;
          }
          const int step = (RA_PIX - last) / 255;
          int v = t;
          if (occupied > 1 && step > 0) {
            v = (step / 2 + before) / step;                // passes 255 on a narrow histogram: Pillow clamps, it does not wrap
            v = v > 255 ? 255 : v;
          }
          lut[c * 256 + t] = (unsigned char)v;
        }
      } else {
        int v;
        if (code == RA_INVERT) v = 255 - t;
        else if (code == RA_POSTERIZE) v = t & (~((1 << (8 - (arg < 0 ? 0 : (arg > 8 ? 8 : arg)))) - 1) & 255);      // arg = bits to keep, 0 .. 8
        else if (code == RA_SOLARIZE) v = t < arg ? t : 255 - t;
        else v = t < 128 ? (t + arg > 255 ? 255 : (t + arg < 0 ? 0 : t + arg)) : t;                                  // RA_SOLARIZE_ADD
        const unsigned char u = (unsigned char)v;
        lut[t] = u; lut[256 + t] = u; lut[512 + t] = u;
      }
      __syncthreads();
      for (int i = t; i < 3 * RA_PIX; i += 256) cur[i] = lut[(i / RA_PIX) * 256 + cur[i]];
      __syncthreads();
    } else if (code >= RA_COLOR && code <= RA_BRIGHTNESS) {
      enhance_planes<RA_PIX>(cur, code == RA_COLOR ? ENH_COLOR : (code == RA_CONTRAST ? ENH_CONTRAST : ENH_BRIGHTNESS), __int_as_float(arg), red, t);
      __syncthreads();
    } else if (code == RA_SHARPNESS) {                     // ImageEnhance.Sharpness: degenerate = the smoothed image
      const float alpha = __int_as_float(arg);
      const bool clamp = !(alpha >= 0.0f && alpha <= 1.0f);
      smooth_pass(cur, alt, t);
      __syncthreads();
      for (int i = t; i < 3 * RA_PIX; i += 256) cur[i] = (unsigned char)blend(alt[i], cur[i], alpha, clamp);
      __syncthreads();
    }                                                      // RA_NONE (a skipped operation) and unknown codes: nothing
  }
  {                                                        // planes -> [80][80][3] bytes, 16 per store
    const unsigned char* cur = planes + co;
    uint4* d4 = reinterpret_cast<uint4*>(view);
    for (int i = t; i < 3 * RA_PIX / 16; i += 256) {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int g = 16 * i + j, pix = g / 3, c = g - 3 * pix;
        w[j >> 2] |= (uint32_t)cur[c * RA_PIX + pix] << (8 * (j & 3));
      }
      d4[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
}

}  // namespace fsvit

int fsvit_set_error(int code, const char* fmt, ...);      // engine.hip (library-internal, C++ linkage)

extern "C" int fsvit_image_rand_augment(uint8_t* views_dev, int B, int H, int W, const int32_t* slots_dev, int n_slots, const int32_t* table_dev,
                                        int cols, const uint8_t* fill3_host, void* stream) {
  if (!views_dev || !fill3_host) return fsvit_set_error(-1, "%s", "fsvit_image_rand_augment: null argument");
  if (H != fsvit::RA_S || W != fsvit::RA_S) return fsvit_set_error(-1, "fsvit_image_rand_augment: built for 80 x 80 views, got %d x %d", H, W);
  if (cols != fsvit::RAC_COLS) return fsvit_set_error(-1, "fsvit_image_rand_augment: the parameter table has %d columns, not %d", cols, fsvit::RAC_COLS);
  if (B < 0) return fsvit_set_error(-1, "%s", "fsvit_image_rand_augment: negative batch");
  if (n_slots < 0 || n_slots > B) return fsvit_set_error(-1, "fsvit_image_rand_augment: %d slots for a batch of %d", n_slots, B);
  if (((uintptr_t)views_dev & 15) != 0) return fsvit_set_error(-1, "%s", "fsvit_image_rand_augment: views_dev must be 16-byte aligned");
  if (n_slots == 0) return 0;                              // nothing listed: no launch (and the two arrays may be empty)
  if (!slots_dev || !table_dev) return fsvit_set_error(-1, "%s", "fsvit_image_rand_augment: null argument");
  fsvit::RandAugParams p;
  p.views = views_dev; p.slots = slots_dev; p.table = table_dev; p.B = B;
  for (int c = 0; c < 3; ++c) p.fill[c] = fill3_host[c];
  hipLaunchKernelGGL(fsvit::rand_augment_kernel, dim3(n_slots), dim3(256), 0, (hipStream_t)stream, p);
  const int rc = (int)hipGetLastError();
  if (rc) return fsvit_set_error(rc, "%s", "fsvit_image_rand_augment: launch failed");
  return 0;
}
