// Device-resident dataset transform: the reference's per-image CPU pipeline
//   Image.fromarray(uint8 HxWx3) -> Resize (Pillow BILINEAR, two 8-bit passes) -> CenterCrop -> ToTensor -> Normalize
// (test_phase/datasets/mini_imagenet.py:47-56, tiered_imagenet.py:53-57), executed for a gathered batch of dataset
// indices on the GPU: the uint8 dataset stays in HBM (60 000 x 84x84x3 = 1.27 GB), one workgroup per output image.
// Byte/integer work, bit-exact with Pillow: the 22-bit fixed-point coefficient tables are computed on the host exactly as
// Resample.c does (datasets/transforms.py) and both passes round to uint8 like ImagingResampleHorizontal/Vertical_8bpc.
// HBM-bound: 21 KB in, 77 KB out per image; the image is staged in LDS once, the horizontal pass result lives in LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fsvit {

struct TransformParams {
  const uint8_t* images;       // [N][H][W][3]
  const int64_t* index;        // [B]
  const int32_t *xmin_h, *cnt_h, *coef_h;      // [RW], [RW], [RW][ksize_h]
  const int32_t *xmin_v, *cnt_v, *coef_v;      // [RH], [RH], [RH][ksize_v]
  float* out;                  // [B][3][OH][OW]
  int H, W, ksize_h, ksize_v, crop_y0, crop_x0, OH, OW;
  float mean[3], inv255, stdv[3];
};

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Round 5: a thread owns one (column, channel) pair of a pass and walks the rows - its coefficients stay in registers, no division in the loops (the
// first version decomposed a flat output index with two div / mod pairs per output and re-read its coefficients from global memory per output:
// 1.5 ms per 12 800-image gather, 4.4 % of the test_few_shot loop, profiles/r05_e2e_gaps.txt) - and ToTensor + Normalize come from a 3 x 256-entry table
// built per workgroup with the SAME IEEE operations (u / 255, then (v - mean) / std), so the bytes -> floats map is unchanged bit for bit.
__global__ __launch_bounds__(256) void transform_gather_kernel(TransformParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int PB = 22;                                 // Pillow PRECISION_BITS = 32 - 8 - 2
  constexpr int KMAX = 6;                                // coefficients kept in registers (Pillow bilinear: support 1 / scale, 3 for an upscale)
  const int t = threadIdx.x;
  const size_t img_bytes = (size_t)p.H * p.W * 3;
  const size_t raw_pad = (img_bytes + 15) & ~(size_t)15, hp_pad = ((size_t)p.H * p.OW * 3 + 15) & ~(size_t)15;
  unsigned char* raw = smem;                             // [H][W][3]
  unsigned char* hp = smem + raw_pad;                    // [H][OW][3]: horizontal pass, cropped columns only
  float* lut = reinterpret_cast<float*>(smem + raw_pad + hp_pad);      // [3][256]
  const uint8_t* src = p.images + (size_t)p.index[blockIdx.x] * img_bytes;
  if ((img_bytes & 15) == 0 && (((uintptr_t)src) & 15) == 0) {
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(raw);
    for (int i = t; i < (int)(img_bytes >> 4); i += 256) d4[i] = s4[i];
  } else if ((img_bytes & 3) == 0 && (((uintptr_t)src) & 3) == 0) {
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d4 = reinterpret_cast<uint32_t*>(raw);
    for (int i = t; i < (int)(img_bytes >> 2); i += 256) d4[i] = s4[i];
  } else {
    for (int i = t; i < (int)img_bytes; i += 256) raw[i] = src[i];
  }
  for (int i = t; i < 768; i += 256) {
    const int c = i >> 8;
    const float v = (float)(i & 255) / 255.0f;                        // ToTensor
    lut[i] = (v - p.mean[c]) / p.stdv[c];                              // Normalize (IEEE division, as torch does)
  }
  __syncthreads();
  // horizontal pass: thread = (output column x, channel c), all input rows
  const int rowb = p.W * 3;
  for (int pc = t; pc < p.OW * 3; pc += 256) {
    const int x = pc / 3, c = pc - 3 * x, xo = x + p.crop_x0;
    const int x0 = p.xmin_h[xo], n = p.cnt_h[xo];
    const int32_t* k = p.coef_h + (size_t)xo * p.ksize_h;
    const unsigned char* rp = raw + x0 * 3 + c;
    unsigned char* op = hp + pc;
    if (n <= KMAX) {
      int kr[KMAX];
#pragma unroll
      for (int j = 0; j < KMAX; ++j) kr[j] = j < n ? k[j] : 0;
      for (int r = 0; r < p.H; ++r, rp += rowb, op += p.OW * 3) {
        int acc = 1 << (PB - 1);
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
          if (j < n) acc += (int)rp[3 * j] * kr[j];
        *op = (unsigned char)clip8(acc >> PB);
      }
    } else {
      for (int r = 0; r < p.H; ++r, rp += rowb, op += p.OW * 3) {
        int acc = 1 << (PB - 1);
        for (int j = 0; j < n; ++j) acc += (int)rp[3 * j] * k[j];
        *op = (unsigned char)clip8(acc >> PB);
      }
    }
  }
  __syncthreads();
  // vertical pass + ToTensor + Normalize, NCHW fp32: thread = (channel c, output column x) with x fastest (coalesced stores), all output rows; the row's
  // coefficients are the same for every thread (scalar loads)
  float* out = p.out + (size_t)blockIdx.x * 3 * p.OH * p.OW;
  const int hrow = p.OW * 3;
  for (int pc = t; pc < 3 * p.OW; pc += 256) {
    const int c = pc / p.OW, x = pc - c * p.OW;
    const unsigned char* hb = hp + x * 3 + c;
    const float* lc = lut + 256 * c;
    float* oc = out + (size_t)c * p.OH * p.OW + x;
    for (int y = 0; y < p.OH; ++y) {
      const int yo = y + p.crop_y0;
      const int y0 = p.xmin_v[yo], n = p.cnt_v[yo];
      const int32_t* k = p.coef_v + (size_t)yo * p.ksize_v;
      const unsigned char* hr = hb + y0 * hrow;
      int acc = 1 << (PB - 1);
      for (int j = 0; j < n; ++j) acc += (int)hr[j * hrow] * k[j];
      oc[(size_t)y * p.OW] = lc[clip8(acc >> PB)];
    }
  }
}

int launch_transform_gather(const TransformParams& p, int B, hipStream_t s) {
  if (B <= 0) return 0;
  const size_t img_bytes = (size_t)p.H * p.W * 3;
  const size_t lds = ((img_bytes + 15) & ~(size_t)15) + (((size_t)p.H * p.OW * 3 + 15) & ~(size_t)15) + 768 * sizeof(float);
  if (lds > 160 * 1024) return (int)hipErrorInvalidValue;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)transform_gather_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(transform_gather_kernel, dim3(B), dim3(256), lds, s, p);
  return (int)hipGetLastError();
}

}  // namespace fsvit

int fsvit_set_error(int code, const char* fmt, ...);      // engine.hip (library-internal, C++ linkage)

extern "C" int fsvit_image_transform_gather(const uint8_t* images_dev, int H, int W, const int64_t* index_dev, int B, const int32_t* xmin_h,
                                            const int32_t* cnt_h, const int32_t* coef_h, int ksize_h, const int32_t* xmin_v,
                                            const int32_t* cnt_v, const int32_t* coef_v, int ksize_v, int crop_y0, int crop_x0, int OH, int OW,
                                            const float* mean3_host, const float* std3_host, float* out_dev, void* stream) {
  if (!images_dev || !index_dev || !xmin_h || !cnt_h || !coef_h || !xmin_v || !cnt_v || !coef_v || !mean3_host || !std3_host || !out_dev)
    return fsvit_set_error(-1, "%s", "fsvit_image_transform_gather: null argument");
  if (H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || ksize_h <= 0 || ksize_v <= 0 || crop_y0 < 0 || crop_x0 < 0)
    return fsvit_set_error(-1, "%s", "fsvit_image_transform_gather: bad geometry");
  fsvit::TransformParams p;
  p.images = images_dev; p.index = index_dev;
  p.xmin_h = xmin_h; p.cnt_h = cnt_h; p.coef_h = coef_h;
  p.xmin_v = xmin_v; p.cnt_v = cnt_v; p.coef_v = coef_v;
  p.out = out_dev;
  p.H = H; p.W = W; p.ksize_h = ksize_h; p.ksize_v = ksize_v; p.crop_y0 = crop_y0; p.crop_x0 = crop_x0; p.OH = OH; p.OW = OW;
  for (int c = 0; c < 3; ++c) { p.mean[c] = mean3_host[c]; p.stdv[c] = std3_host[c]; }
  p.inv255 = 1.0f / 255.0f;
  int rc = fsvit::launch_transform_gather(p, B, (hipStream_t)stream);
  if (rc) return fsvit_set_error(rc, "%s", "fsvit_image_transform_gather: launch failed (image too large for LDS?)");
  return 0;
}

// ---------------------------------------------------------------- train-time augment 'resize' (sun_train_teacher/datasets/mini_imagenet.py:57-63)
//   RandomResizedCrop(80) (Pillow crop, then Pillow BILINEAR resize) -> RandomHorizontalFlip -> ToTensor -> Normalize
// for a gathered batch: the crop box differs per image, so each workgroup builds its own image's tap tables in LDS - the same integers as
// datasets/transforms.py:pil_bilinear_tables(w, OW) / (h, OH), in fp64 with the same association and NO contraction (an FMA changes
// int(center - support + 0.5) at scales such as 0.6 or 1.2) - and applies them at the box offset.  The host draws the boxes and flips; nothing else is
// uploaded per batch.  Taps are clipped to the crop, not to the source image (torchvision crops first, then resizes).
namespace fsvit {

struct RrcParams {
  const uint8_t* images;       // [N][H][W][3]
  const int64_t* index;        // [B]
  const int32_t* box;          // [B][4] top, left, height, width
  const uint8_t* flip;         // [B]
  void* out;                   // float [B][3][OH][OW] normalised, or (U8 epilogue) uint8 [B][OH][OW][3]
  int H, W, OH, OW, kh, kv;    // kh / kv: table row stride = tap count of the largest box (w = W, h = H)
  float mean[3], stdv[3];
};

enum { RRC_BILINEAR = 0, RRC_BICUBIC = 1 };

// ceil(support * max(in / out, 1)) * 2 + 1 with support 1 (bilinear) or 2 (bicubic)
__host__ __device__ inline int rrc_ksize(int in, int out, int filter = RRC_BILINEAR) {
  const int c = filter == RRC_BICUBIC ? (2 * in + out - 1) / out : (in + out - 1) / out, cmin = filter == RRC_BICUBIC ? 2 : 1;
  return 2 * (c < cmin ? cmin : c) + 1;
}

// Resample.c bilinear_filter / bicubic_filter (a = -0.5), each double operation one IEEE operation in C's order
template <int FILTER>
__device__ __forceinline__ double rrc_filter(double x) {
#pragma clang fp contract(off)
  x = fabs(x);
  if (FILTER == RRC_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
  if (x < 1.0) return ((-0.5 + 2.0) * x - (-0.5 + 3.0)) * x * x + 1.0;
  if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5;
  return 0.0;
}

// One row of pil_resample_tables(in, out, filter): first input index, tap count, 22-bit taps.  Every double operation is one IEEE operation, in Python's
// order.
template <int FILTER>
__device__ void rrc_table_row(int in, int out, int o, int stride, int32_t* xmin, int32_t* cnt, int32_t* coef) {
#pragma clang fp contract(off)
  const double scale = (double)in / (double)out;
  const double fscale = scale > 1.0 ? scale : 1.0;
  const double support = FILTER == RRC_BICUBIC ? 2.0 * fscale : fscale;
  const double inv = 1.0 / fscale;
  const double center = ((double)o + 0.5) * scale;
  int lo = (int)(center - support + 0.5), hi = (int)(center + support + 0.5);
  lo = lo < 0 ? 0 : lo;
  hi = hi > in ? in : hi;
  int n = hi - lo;
  n = n < 0 ? 0 : (n > stride ? stride : n);             // never taken for Pillow's tables (hi - lo <= ksize); keeps the row inside its LDS slot
  double total = 0.0;
  for (int x = lo; x < lo + n; ++x) {
    total += rrc_filter<FILTER>(((double)x - center + 0.5) * inv);
  }
  for (int j = 0; j < n; ++j) {
    double w = rrc_filter<FILTER>(((double)(lo + j) - center + 0.5) * inv);
    if (total != 0.0) w = w / total;
    const double v = w * (double)(1 << 22);
    coef[(size_t)o * stride + j] = w < 0.0 ? (int)(v - 0.5) : (int)(v + 0.5);
  }
  xmin[o] = lo;
  cnt[o] = n;
}

// FILTER picks the tap tables; U8OUT the epilogue: the resized (and mirrored) bytes as [OH][OW][3] for the colour stage instead of the normalised planes.
template <int FILTER, bool U8OUT>
__global__ __launch_bounds__(256) void transform_rrc_gather_kernel(RrcParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int PB = 22;
  constexpr int KMAX = 6;                                // taps kept in registers: covers every box up to 2.5 x the output size
  const int t = threadIdx.x, b = blockIdx.x;
  const int rowb = p.W * 3, hrow = p.OW * 3;
  // the box, clamped to the image: no box can read outside its image
  int bi = p.box[4 * b], bj = p.box[4 * b + 1], bh = p.box[4 * b + 2], bw = p.box[4 * b + 3];
  bi = bi < 0 ? 0 : (bi > p.H - 1 ? p.H - 1 : bi);
  bj = bj < 0 ? 0 : (bj > p.W - 1 ? p.W - 1 : bj);
  bh = bh < 1 ? 1 : (bh > p.H - bi ? p.H - bi : bh);
  bw = bw < 1 ? 1 : (bw > p.W - bj ? p.W - bj : bw);
  const bool flip = p.flip[b] != 0;
  // LDS: the box's rows (full width, at the global address's 16-byte phase) | horizontal pass | Normalize table | tap tables
  const size_t raw_pad = (((size_t)p.H * rowb + 15) & ~(size_t)15) + 16, hp_pad = ((size_t)p.H * hrow + 15) & ~(size_t)15;
  float* lut = reinterpret_cast<float*>(smem + raw_pad + hp_pad);      // [3][256]
  int32_t* xmin_h = reinterpret_cast<int32_t*>(lut + 768);
  int32_t* cnt_h = xmin_h + p.OW;
  int32_t* coef_h = cnt_h + p.OW;                         // [OW][kh]
  int32_t* xmin_v = coef_h + (size_t)p.OW * p.kh;
  int32_t* cnt_v = xmin_v + p.OH;
  int32_t* coef_v = cnt_v + p.OH;                         // [OH][kv]
  const uint8_t* src = p.images + (size_t)p.index[b] * p.H * rowb + (size_t)bi * rowb;
  const int nbytes = bh * rowb;
  const int mis = (int)(((uintptr_t)src) & 15);
  unsigned char* raw = smem + mis;                        // [bh][W][3]
  unsigned char* hp = smem + raw_pad;                     // [bh][OW][3]
  {
    int head = (16 - mis) & 15;
    head = head > nbytes ? nbytes : head;
    const int body = (nbytes - head) >> 4, tail0 = head + (body << 4);
    const uint4* s4 = reinterpret_cast<const uint4*>(src + head);
    uint4* d4 = reinterpret_cast<uint4*>(raw + head);
    for (int i = t; i < body; i += 256) d4[i] = s4[i];
    if (t < head) raw[t] = src[t];
    if (tail0 + t < nbytes) raw[tail0 + t] = src[tail0 + t];           // < 16 bytes
  }
  if constexpr (!U8OUT)
    for (int i = t; i < 768; i += 256) {
      const int c = i >> 8;
      const float v = (float)(i & 255) / 255.0f;                      // ToTensor
      lut[i] = (v - p.mean[c]) / p.stdv[c];                            // Normalize (IEEE division, as torch does)
    }
  for (int o = t; o < p.OW + p.OH; o += 256) {
    if (o < p.OW) rrc_table_row<FILTER>(bw, p.OW, o, p.kh, xmin_h, cnt_h, coef_h);
    else rrc_table_row<FILTER>(bh, p.OH, o - p.OW, p.kv, xmin_v, cnt_v, coef_v);
  }
  __syncthreads();
  // horizontal pass over the box's rows: thread = (output column x, channel c)
  for (int pc = t; pc < hrow; pc += 256) {
    const int x = pc / 3, c = pc - 3 * x;
    const int n = cnt_h[x];
    const int32_t* k = coef_h + (size_t)x * p.kh;
    const unsigned char* rp = raw + (bj + xmin_h[x]) * 3 + c;
    unsigned char* op = hp + pc;
    if (n <= KMAX) {
      int kr[KMAX];
#pragma unroll
      for (int j = 0; j < KMAX; ++j) kr[j] = j < n ? k[j] : 0;
      for (int r = 0; r < bh; ++r, rp += rowb, op += hrow) {
        int acc = 1 << (PB - 1);
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
          if (j < n) acc += (int)rp[3 * j] * kr[j];
        *op = (unsigned char)clip8(acc >> PB);
      }
    } else {
      for (int r = 0; r < bh; ++r, rp += rowb, op += hrow) {
        int acc = 1 << (PB - 1);
        for (int j = 0; j < n; ++j) acc += (int)rp[3 * j] * k[j];
        *op = (unsigned char)clip8(acc >> PB);
      }
    }
  }
  __syncthreads();
  // vertical pass + flip + ToTensor + Normalize, NCHW fp32: thread = (channel c, output column x), x fastest (coalesced stores); a flipped image reads
  // the mirrored column of the resized image (the flip follows the resize in the reference's transform order)
  // U8OUT: thread = (output column x, channel c) with c fastest, as the bytes lie in [OH][OW][3]
  for (int pc = t; pc < 3 * p.OW; pc += 256) {
    const int c = U8OUT ? pc % 3 : pc / p.OW, x = U8OUT ? pc / 3 : pc - c * p.OW;
    const unsigned char* hb = hp + (flip ? p.OW - 1 - x : x) * 3 + c;
    [[maybe_unused]] const float* lc = nullptr;
    [[maybe_unused]] float* oc = nullptr;
    [[maybe_unused]] unsigned char* out8 = nullptr;
    if constexpr (U8OUT) {
      out8 = static_cast<unsigned char*>(p.out) + (size_t)b * 3 * p.OH * p.OW + pc;
    } else {
      lc = lut + 256 * c;
      oc = static_cast<float*>(p.out) + (size_t)b * 3 * p.OH * p.OW + (size_t)c * p.OH * p.OW + x;
    }
    for (int y = 0; y < p.OH; ++y) {
      const int n = cnt_v[y];
      const int32_t* k = coef_v + (size_t)y * p.kv;
      const unsigned char* hr = hb + xmin_v[y] * hrow;
      int acc = 1 << (PB - 1);
      for (int j = 0; j < n; ++j) acc += (int)hr[j * hrow] * k[j];
      if constexpr (U8OUT) out8[(size_t)y * hrow] = (unsigned char)clip8(acc >> PB);
      else oc[(size_t)y * p.OW] = lc[clip8(acc >> PB)];
    }
  }
}

template <int FILTER, bool U8OUT>
int launch_transform_rrc(const RrcParams& p, int B, hipStream_t s) {
  if (B <= 0) return 0;
  const size_t lds = (((size_t)p.H * p.W * 3 + 15) & ~(size_t)15) + 16 + (((size_t)p.H * p.OW * 3 + 15) & ~(size_t)15) + 768 * sizeof(float) +
                     ((size_t)p.OW * (2 + p.kh) + (size_t)p.OH * (2 + p.kv)) * sizeof(int32_t);
  if (lds > 160 * 1024) return (int)hipErrorInvalidValue;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)transform_rrc_gather_kernel<FILTER, U8OUT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL((transform_rrc_gather_kernel<FILTER, U8OUT>), dim3(B), dim3(256), lds, s, p);
  return (int)hipGetLastError();
}

}  // namespace fsvit

extern "C" int fsvit_image_transform_rrc_gather(const uint8_t* images_dev, int H, int W, const int64_t* index_dev, int B, const int32_t* box_dev,
                                                const uint8_t* flip_dev, int OH, int OW, const float* mean3_host, const float* std3_host,
                                                float* out_dev, void* stream) {
  if (!images_dev || !index_dev || !box_dev || !flip_dev || !mean3_host || !std3_host || !out_dev)
    return fsvit_set_error(-1, "%s", "fsvit_image_transform_rrc_gather: null argument");
  if (H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || B < 0)
    return fsvit_set_error(-1, "%s", "fsvit_image_transform_rrc_gather: bad geometry");
  fsvit::RrcParams p;
  p.images = images_dev; p.index = index_dev; p.box = box_dev; p.flip = flip_dev; p.out = out_dev;
  p.H = H; p.W = W; p.OH = OH; p.OW = OW;
  p.kh = fsvit::rrc_ksize(W, OW); p.kv = fsvit::rrc_ksize(H, OH);
  for (int c = 0; c < 3; ++c) { p.mean[c] = mean3_host[c]; p.stdv[c] = std3_host[c]; }
  int rc = fsvit::launch_transform_rrc<fsvit::RRC_BILINEAR, false>(p, B, (hipStream_t)stream);
  if (rc) return fsvit_set_error(rc, "%s", "fsvit_image_transform_rrc_gather: launch failed (image too large for LDS?)");
  return 0;
}

// The weak view of the distillation phase (sun_meta_training/datasets/mini_imagenet.py:100-102): the same crop + resize + flip with Pillow's BICUBIC
// (or BILINEAR) taps, left as uint8 [B][OH][OW][3] for fsvit_image_strong_weak (augment.hip).  The negative bicubic taps overshoot: clip8 is live here.
extern "C" int fsvit_image_transform_rrc_u8(const uint8_t* images_dev, int H, int W, const int64_t* index_dev, int B, const int32_t* box_dev,
                                            const uint8_t* flip_dev, int OH, int OW, int filter, uint8_t* out_dev, void* stream) {
  if (!images_dev || !index_dev || !box_dev || !flip_dev || !out_dev) return fsvit_set_error(-1, "%s", "fsvit_image_transform_rrc_u8: null argument");
  if (H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || B < 0) return fsvit_set_error(-1, "%s", "fsvit_image_transform_rrc_u8: bad geometry");
  if (filter != fsvit::RRC_BILINEAR && filter != fsvit::RRC_BICUBIC)
    return fsvit_set_error(-1, "%s", "fsvit_image_transform_rrc_u8: filter must be 0 (bilinear) or 1 (bicubic)");
  fsvit::RrcParams p;
  p.images = images_dev; p.index = index_dev; p.box = box_dev; p.flip = flip_dev; p.out = out_dev;
  p.H = H; p.W = W; p.OH = OH; p.OW = OW;
  p.kh = fsvit::rrc_ksize(W, OW, filter); p.kv = fsvit::rrc_ksize(H, OH, filter);
  for (int c = 0; c < 3; ++c) { p.mean[c] = 0.0f; p.stdv[c] = 1.0f; }
  int rc = filter == fsvit::RRC_BICUBIC ? fsvit::launch_transform_rrc<fsvit::RRC_BICUBIC, true>(p, B, (hipStream_t)stream)
                                        : fsvit::launch_transform_rrc<fsvit::RRC_BILINEAR, true>(p, B, (hipStream_t)stream);
  if (rc) return fsvit_set_error(rc, "%s", "fsvit_image_transform_rrc_u8: launch failed (image too large for LDS?)");
  return 0;
}
