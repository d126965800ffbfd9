// Internal launchers of the fsvit gfx950 kernels.  Every kernel source that touches 16-bit activations is compiled twice
// (fsvit_common.h): the same declarations exist in namespace fsvit (bf16) and namespace fsvit_f16 (fp16).
#pragma once
#include <hip/hip_runtime.h>
#include "conv_gemm.h"

#define FSVIT_DECL_NS fsvit
#include "kernels_decl.inc"
#undef FSVIT_DECL_NS
#define FSVIT_DECL_NS fsvit_f16
#include "kernels_decl.inc"
#undef FSVIT_DECL_NS

// DeepEMD head (emd_head.hip): fp32 only, one build.  workspace = emd_head_workspace_bytes(E, P, Q, N, C); N <= 32, C a multiple of 64 (checked by the C entries)
namespace fsvit {
size_t emd_head_workspace_bytes(int E, int P, int Q, int N, int C);
int launch_emd_head_forward(const float* shot_tok, const float* query_tok, int E, int P, int Q, int N, int C, float temperature, float* logits, float* flow,
                            int* status, void* ws, hipStream_t s);
int launch_emd_head_backward(const float* shot_tok, const float* query_tok, const float* dlogits, const float* flow, int E, int P, int Q, int N, int C,
                             float temperature, float* d_shot, float* d_query, void* ws, hipStream_t s);
int launch_emd_solve(const float* cost, const float* w1, const float* w2, int B, int N, float* flow, int* status, int* naug, hipStream_t s);
}  // namespace fsvit
