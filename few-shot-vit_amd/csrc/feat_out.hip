// Encoder output, storage type -> fp32: what leaves an encoder's 16-bit (or fp32) activation maps for the fp32 heads.
//  * pool_affine: final BatchNorm (eval, folded to scale/shift) + AdaptiveAvgPool2d(1) + flatten
//    (test_phase/models/visformer.py:455-462): feat[b][c] = scale[c] * mean_hw x[b][hw][c] + shift[c].
//  * tokens_to_f32 / add_f32_into: the post-norm token map of the distillation phase (sun_meta_training/models/visformer.py:464) in fp32,
//    and its fp32 gradient added back into the storage-type gradient map.
// The only kernels of the heads that touch the 16-bit type, hence built twice (Makefile DUAL); head.hip and token_label.hip are fp32, one build.
#include "fsvit_common.h"
#include "kernels.h"

namespace FSVIT_NS {

template <typename T>
__global__ __launch_bounds__(256) void pool_affine_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, float* __restrict__ feat,
                                                          int HW, int C) {
  const int b = blockIdx.x;
  const T* xb = x + (size_t)b * HW * C;
  const float inv = 1.0f / (float)HW;
  for (int c4 = threadIdx.x; c4 < C / 4; c4 += 256) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < HW; ++p) acc += load4<T>(xb + (size_t)p * C + c4 * 4);
    const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + c4 * 4);
    const f32x4 sh = *reinterpret_cast<const f32x4*>(shift + c4 * 4);
    *reinterpret_cast<f32x4*>(feat + (size_t)b * C + c4 * 4) = acc * inv * sc + sh;
  }
}

int launch_pool_affine(const void* x, const float* scale, const float* shift, float* feat, int B, int HW, int C, int dtype, hipStream_t s) {
  if (B <= 0) return 0;
  return with_elem(dtype, [&](auto e) { return launch(pool_affine_kernel<elem_t<decltype(e)>>, B, 256, 0, s, x, scale, shift, feat, HW, C); });
}

// token map plumbing: storage dtype <-> fp32
template <typename T>
__global__ void tokens_to_f32_kernel(const T* __restrict__ in, const float* __restrict__ scale, const float* __restrict__ shift, float* __restrict__ out, size_t n, int C) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % C);
  const float v = to_f32<T>(in[i]);
  out[i] = scale ? v * scale[c] + shift[c] : v;
}
template <typename T>
__global__ void add_f32_into_kernel(T* __restrict__ inout, const float* __restrict__ add, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) inout[i] = from_f32<T>(to_f32<T>(inout[i]) + add[i]);
}
// out[i] = in[i] (* scale[c] + shift[c] when scale != NULL): the post-norm token map in fp32
int launch_tokens_to_f32(const void* in, const float* scale, const float* shift, float* out, size_t n, int C, int dtype, hipStream_t s) {
  if (n == 0) return 0;
  const unsigned g = (unsigned)((n + 255) / 256);
  return with_elem(dtype, [&](auto e) { return launch(tokens_to_f32_kernel<elem_t<decltype(e)>>, g, 256, 0, s, in, scale, shift, out, n, C); });
}
int launch_add_f32_into(void* inout, const float* add, size_t n, int dtype, hipStream_t s) {
  if (n == 0) return 0;
  const unsigned g = (unsigned)((n + 255) / 256);
  return with_elem(dtype, [&](auto e) { return launch(add_f32_into_kernel<elem_t<decltype(e)>>, g, 256, 0, s, inout, add, n); });
}

}  // namespace FSVIT_NS
