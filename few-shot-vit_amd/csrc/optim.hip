// Parameter updates of the training drivers, fp32, one build: SGD with momentum (plain and Nesterov), AdamW, and the NaN-gradient guard.
// Each update is ONE functor over (item, idx); two kernel templates run it - optim_kernel over one tensor (grid-stride, gs_grid) and
// optim_multi_kernel over a table of tensors in one launch (blockIdx.y = tensor: the meta-tuning step has 86 parameter tensors, the
// distillation phase 89, i.e. as many launches of ~4 us and host calls per step otherwise - profiles/r05_distill_kernel_stats.csv).
// The item layouts are the rows of the int64 tables engine.py builds (ops._ptr_table).
#include <math.h>

#include "fsvit_common.h"
#include "train_kernels.h"

namespace fsvit {

struct SgdItem { float* p; const float* g; float* buf; size_t n; };
struct AdamwItem { float* p; const float* g; float* m; float* v; size_t n; };
struct GradItem { float* g; size_t n; };

// what an update may override in the multi kernel: leave a whole tensor alone, act once per thread behind its loop
struct Update {
  __device__ __forceinline__ bool skip(unsigned tensor) const { return false; }
  __device__ __forceinline__ void finish(unsigned tensor) const {}
};

// SGD with momentum and weight decay, torch.optim.SGD semantics (utils/__init__.py:131-132): d = g + wd*p; buf = mom*buf + d (buf = d on the
// first step); p -= lr * buf.  NESTEROV: torch.optim.SGD(nesterov=True, dampening=0) (meta_tuning_sun_d/train_meta.py:115): p -= lr * (d + mom*buf)
template <bool NESTEROV>
struct SgdUpdate : Update {
  using Item = SgdItem;
  float lr, momentum, wd;
  int first;
  __device__ __forceinline__ void operator()(const Item& it, size_t idx) const { step(it.p, it.g, it.buf, idx); }
  __device__ __forceinline__ void step(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, size_t idx) const {
    const float d = g[idx] + wd * p[idx];
    const float b = first ? d : momentum * buf[idx] + d;
    buf[idx] = b;
    if (NESTEROV) p[idx] -= lr * (d + momentum * b);
    else p[idx] -= lr * b;
  }
};

// torch.optim.AdamW / timm AdamW (decoupled weight decay); bc1 = 1 - beta1^step, rsqrt_bc2 = 1 / sqrt(1 - beta2^step) of the 1-based update number
struct AdamwUpdate : Update {
  using Item = AdamwItem;
  float lr, beta1, beta2, eps, wd, bc1, rsqrt_bc2;
  __device__ __forceinline__ void operator()(const Item& it, size_t i) const { step(it.p, it.g, it.m, it.v, i); }
  __device__ __forceinline__ void step(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, size_t i) const {
    const float gi = g[i];
    const float pi = p[i] * (1.0f - lr * wd);
    const float mi = beta1 * m[i] + (1.0f - beta1) * gi;
    const float vi = beta2 * v[i] + (1.0f - beta2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) * rsqrt_bc2 + eps;
    p[i] = pi - (lr / bc1) * (mi / denom);
  }
};

// detect_grad_nan (meta_tuning_sun_d/Models/utils.py:115-118) for a table of gradient tensors: a tensor holding any NaN (g != g; Inf does not
// count) is zeroed entirely.  Pass 1 flags, pass 2 zeroes the flagged tensors; the flags stay on the device.  Every wave that saw a NaN stores the
// same 1 with a plain vector store: no atomics.
struct NanFlag : Update {
  using Item = GradItem;
  int* __restrict__ flags;
  bool nan;                                                  // per thread; the launcher passes false
  __device__ __forceinline__ void operator()(const Item& it, size_t idx) {
    const float v = it.g[idx];
    nan |= v != v;
  }
  __device__ __forceinline__ void finish(unsigned tensor) const {
    if (__ballot(nan) != 0 && (threadIdx.x & 63) == 0) flags[tensor] = 1;
  }
};
struct NanZero : Update {
  using Item = GradItem;
  const int* __restrict__ flags;
  __device__ __forceinline__ bool skip(unsigned tensor) const { return flags[tensor] == 0; }
  __device__ __forceinline__ void operator()(const Item& it, size_t idx) const { it.g[idx] = 0.f; }
};

template <typename U>
__global__ __launch_bounds__(256) void optim_kernel(const typename U::Item it, U u) {
  GS_LOOP(idx, it.n) u(it, idx);
}
template <typename U>
__global__ __launch_bounds__(256) void optim_multi_kernel(const typename U::Item* __restrict__ items, U u) {
  if (u.skip(blockIdx.y)) return;
  const typename U::Item it = items[blockIdx.y];
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < it.n; idx += (size_t)gridDim.x * 256) u(it, idx);
  u.finish(blockIdx.y);
}

template <typename U>
static int launch_single(typename U::Item it, U u, hipStream_t s) {
  if (it.n == 0) return 0;
  return launch(optim_kernel<U>, gs_grid(it.n), 256, 0, s, it, u);
}
// the grid of every multi launch: 4 elements per thread at the largest tensor (smaller ones leave blocks idle), 256 blocks at most
static unsigned multi_grid_x(size_t max_numel) {
  const size_t gx = (max_numel + 1023) / 1024;
  return (unsigned)(gx > 256 ? 256 : gx);
}
template <typename U>
static int launch_multi(const void* items_dev, int n_items, size_t max_numel, U u, hipStream_t s) {
  if (n_items <= 0 || max_numel == 0) return 0;
  return launch(optim_multi_kernel<U>, dim3(multi_grid_x(max_numel), (unsigned)n_items), 256, 0, s, items_dev, u);
}

int launch_sgd(float* p, const float* g, float* buf, size_t n, float lr, float momentum, float wd, int first, hipStream_t s) {
  return launch_single(SgdItem{p, g, buf, n}, SgdUpdate<false>{{}, lr, momentum, wd, first}, s);
}
int launch_sgd_multi(const void* items_dev, int n_items, size_t max_numel, float lr, float momentum, float wd, int first, hipStream_t s) {
  return launch_multi(items_dev, n_items, max_numel, SgdUpdate<false>{{}, lr, momentum, wd, first}, s);
}
int launch_sgd_nesterov(float* p, const float* g, float* buf, size_t n, float lr, float momentum, float wd, int first, hipStream_t s) {
  return launch_single(SgdItem{p, g, buf, n}, SgdUpdate<true>{{}, lr, momentum, wd, first}, s);
}
int launch_sgd_nesterov_multi(const void* items_dev, int n_items, size_t max_numel, float lr, float momentum, float wd, int first, hipStream_t s) {
  return launch_multi(items_dev, n_items, max_numel, SgdUpdate<true>{{}, lr, momentum, wd, first}, s);
}

static AdamwUpdate adamw_update(float lr, float beta1, float beta2, float eps, float wd, int step) {
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  return AdamwUpdate{{}, lr, beta1, beta2, eps, wd, (float)bc1, (float)(1.0 / sqrt(bc2))};
}
int launch_adamw(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps, float wd, int step, hipStream_t s) {
  return launch_single(AdamwItem{p, g, m, v, n}, adamw_update(lr, beta1, beta2, eps, wd, step), s);
}
int launch_adamw_multi(const void* items_dev, int n_items, size_t max_numel, float lr, float beta1, float beta2, float eps, float wd, int step, hipStream_t s) {
  return launch_multi(items_dev, n_items, max_numel, adamw_update(lr, beta1, beta2, eps, wd, step), s);
}

int launch_grad_nan_guard_multi(const void* items_dev, int n_items, size_t max_numel, int* flags_dev, hipStream_t s) {
  if (n_items <= 0) return 0;
  int rc = (int)hipMemsetAsync(flags_dev, 0, (size_t)n_items * sizeof(int), s);
  if (rc || max_numel == 0) return rc;
  rc = launch_multi(items_dev, n_items, max_numel, NanFlag{{}, flags_dev, false}, s);
  if (rc) return rc;
  return launch_multi(items_dev, n_items, max_numel, NanZero{{}, flags_dev}, s);
}

}  // namespace fsvit
