// What the two host files (engine.hip, train_engine.hip) share: the error setter and its macros, the dtype dispatch, small integer helpers and
// the workspace arena.  Host code only - never included by a kernel source.
#pragma once

#include "../../include/fsvit.h"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

// ------------------------------------------------------------------------------------ errors
// Sets the thread's fsvit_last_error() text and returns `code` (the one definition is in engine.hip).
int fsvit_set_error(int code, const char* fmt, ...);
template <class... A>
static inline int fail(int code, const char* fmt, A... a) { return fsvit_set_error(code, fmt, a...); }
static inline int hipfail(hipError_t e, const char* what) { return fsvit_set_error((int)e, "%s: %s", what, hipGetErrorString(e)); }

#define HIP_TRY(expr)                                   \
  do {                                                  \
    hipError_t _e = (expr);                             \
    if (_e != hipSuccess) return hipfail(_e, #expr);    \
  } while (0)
// expr: 0, a negative FSVIT_ERR_* whose text is already set (handed on), or a positive hipError_t (reported as `what`)
#define RC_TRY_AS(expr, what)                                                     \
  do {                                                                            \
    int _rc = (expr);                                                             \
    if (_rc != 0) return _rc > 0 ? hipfail((hipError_t)_rc, what) : _rc;          \
  } while (0)
#define RC_TRY(expr) RC_TRY_AS(expr, #expr)

// ------------------------------------------------------------------------------------ dtype dispatch
// Every kernel that touches 16-bit activations exists for the two 16-bit storage types (namespace fsvit = bf16, fsvit_f16 = fp16; see
// fsvit_common.h).  K(fn) picks the build that matches `kdt` (a FSVIT_* dtype in scope); kd() maps the public dtype to the kernels' own
// convention (0 = f32, 1 = the namespace's 16-bit type).  The fp32-only heads (kernels.h, bottom) are fsvit:: alone.
// The two-limb modes (FSVIT_BF16X2 / FSVIT_F16X2) are fp32 STORAGE (kd() = 0: every kernel but the GEMM is the fp32 path's) with the GEMM
// arithmetic selected by kg() = 2 (conv_gemm_v2.hip: x2_split) and the weights uploaded pre-split.
#define K(fn) ((kdt == FSVIT_F16 || kdt == FSVIT_F16X2) ? fsvit_f16::fn : fsvit::fn)
static inline bool is_x2(int dtype) { return dtype == FSVIT_BF16X2 || dtype == FSVIT_F16X2; }
static inline bool known_dtype(int dtype) { return dtype >= FSVIT_F32 && dtype <= FSVIT_F16X2; }
static inline int kd(int dtype) { return (dtype == FSVIT_F32 || is_x2(dtype)) ? 0 : 1; }
static inline int kg(int dtype) { return is_x2(dtype) ? 2 : kd(dtype); }
static inline int storage_bytes(int dtype) { return kd(dtype) == 0 ? 4 : 2; }
static inline bool half_dtype(int dtype) { return dtype == FSVIT_BF16 || dtype == FSVIT_F16; }

// ------------------------------------------------------------------------------------ helpers
static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
static inline bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
static inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
static inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// Bump allocator over a caller-owned workspace: every buffer starts on a 256-byte boundary.  A dry arena only measures (fake non-null
// addresses); a real one returns nullptr once the workspace is exhausted.  Regions that are live at different times overlap: mark() where
// the first begins, rewind() to it before the next is laid out; `peak` is the high-water mark across rewinds.
struct Arena {
  unsigned char* base = nullptr;
  size_t size = 0, off = 0, peak = 0;
  bool dry = false;                       // dry run: only measure
  void* take(size_t bytes) {
    size_t o = off;
    off += align256(bytes);
    if (off > peak) peak = off;
    if (dry) return (void*)(uintptr_t)(o + 256);
    return off <= size ? base + o : nullptr;
  }
  size_t mark() const { return off; }
  void rewind(size_t m) { off = m; }
};
