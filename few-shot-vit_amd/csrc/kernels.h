// Internal launchers of the fsvit gfx950 kernels.  Every kernel source that touches 16-bit activations is compiled twice
// (fsvit_common.h): the declarations of kernels_decl.inc exist in namespace fsvit (bf16) and namespace fsvit_f16 (fp16).  The fp32-only
// heads at the bottom are built once; the training-path and optimizer launchers are in train_kernels.h.
#pragma once
#include <hip/hip_runtime.h>
#include "conv_gemm.h"

#define FSVIT_DECL_NS fsvit
#include "kernels_decl.inc"
#undef FSVIT_DECL_NS
#define FSVIT_DECL_NS fsvit_f16
#include "kernels_decl.inc"
#undef FSVIT_DECL_NS

// ---- fp32 only, one build: namespace fsvit alone
namespace fsvit {
// cosine / squared-distance prototype head (head.hip; meta_baseline.py:33-47, utils/__init__.py:78-109); its backwards: train_kernels.h
int launch_proto_head(const float* feat_shot, const float* feat_query, int E, int way, int shot, int Q, int D,
                      float temp, int method, float* logits, float* acc, float* loss, hipStream_t s, const float* temp_dev = nullptr);
int launch_proto_head_ce(const float* feat_shot, const float* feat_query, const long long* labels, int E, int way, int shot, int Q, int D, float temp, int method,
                         float* logits, float* acc, float* loss, float* dlogits, float* mean_out, unsigned* ticket, hipStream_t s, const float* temp_dev = nullptr);
// the same head over rows of a feature table [N][D] addressed by idx [E][way][shot + n_query] (int32 / int64 slots); limits: fsvit_proto_head_gather of fsvit.h
int launch_proto_head_gather(const float* table, int N, int D, const void* idx, int idx_is_int64, int E, int way, int shot, int n_query, float temp, int method,
                             float* logits, float* acc, float* loss, int* invalid, hipStream_t s, const float* temp_dev = nullptr);
// prototype bank over a labelled support set and the single-prototype ROC-AUC of --sauc (proto_bank.hip); limits: the fsvit_proto_bank_* entries of fsvit.h
int launch_proto_bank_accumulate(const float* feat, const void* label, int label_is_int64, int S, int way, int D, float* sum, int* count, int* invalid,
                                 hipStream_t s);
int launch_proto_bank_finalize(const float* sum, const int* count, int way, int D, int method, float* proto, int* empty, hipStream_t s);
int launch_proto_bank_logits(const float* query, const float* proto, const int* empty, int Q, int way, int D, float temp, const float* temp_dev, int method,
                             float* logits, int* pred, hipStream_t s);
// top-k + log-sum-exp per row on a (query tile, class split) grid; 1 <= K <= 32, 1 <= n_split <= ceil(way / 1024), workspace = proto_bank_topk_workspace_bytes
size_t proto_bank_topk_workspace_bytes(int Q, int way, int K, int n_split);
int launch_proto_bank_topk(const float* query, const float* proto, const int* empty, int Q, int way, int D, float temp, const float* temp_dev, int method, int K,
                           int n_split, float* values, int* indices, float* lse, void* ws, hipStream_t s);
int launch_proto_auc(const float* feat_shot, const float* feat_query, int E, int shot, int Q, int D, float* auc, float* score, hipStream_t s);
// the same reduction over rows of a feature table [N][D]: shot_slots [E][shot], query_slots [E][Q] (int32 / int64 slots); limits: fsvit_proto_auc_gather of fsvit.h
int launch_proto_auc_gather(const float* table, int N, int D, const void* shot_slots, const void* query_slots, int idx_is_int64, int E, int shot, int Q,
                            float* auc, float* score, int* invalid, hipStream_t s);
// distillation head (token_label.hip): LinearClassifier forward / backward, generate_softlabel, SoftTargetCrossEntropy, F.normalize on rows
int launch_linear_fwd(const float* x, const float* w, const float* b, float* y, int M, int N, int K, hipStream_t s);
int launch_linear_bwd(const float* dy, const float* x, const float* w, float* dx, int accumulate_dx, float* dw, float* db, int M, int N, int K, hipStream_t s);
int launch_token_softlabel(const float* lt, float* soft, int B, int T, int C, int k, int bp, double smoothing, hipStream_t s);
int launch_soft_target_ce(const float* z, const float* tgt, float* rowloss, float* dz, int R, int C, float gscale, hipStream_t s);
int launch_row_normalize(const float* x, float* y, float* inv, int R, int D, hipStream_t s);
int launch_row_normalize_bwd(const float* y, const float* inv, const float* dy, float* dx, int R, int D, hipStream_t s);
// DeepEMD head (emd_head.hip).  workspace = emd_head_workspace_bytes(E, P, Q, N, C); N <= 32, C a multiple of 64 (checked by the C entries)
size_t emd_head_workspace_bytes(int E, int P, int Q, int N, int C);
int launch_emd_head_forward(const float* shot_tok, const float* query_tok, int E, int P, int Q, int N, int C, float temperature, float* logits, float* flow,
                            int* status, void* ws, hipStream_t s);
int launch_emd_head_backward(const float* shot_tok, const float* query_tok, const float* dlogits, const float* flow, int E, int P, int Q, int N, int C,
                             float temperature, float* d_shot, float* d_query, void* ws, hipStream_t s);
// the head's forward over rows of a token-map table (limits: fsvit_emd_head_gather of fsvit.h); ws is read in the dense-prototype form only
int launch_emd_table_prep(const float* tok, int n_img, int N, int C, float* xhat, float* pooled, hipStream_t s);
size_t emd_head_gather_workspace_bytes(int E, int P, int N, int C);
int launch_emd_head_gather(const float* tok, const float* xhat, const float* pooled, int n_slots, const void* query_slots, const void* proto_slots,
                           int slots_are_int64, const float* proto_tok, int E, int P, int Q, int N, int C, float temperature, float* logits, int* status,
                           int* invalid, void* ws, hipStream_t s);
// a bank of class token maps over a labelled support set, and the exact re-rank of a shortlist (limits: fsvit_emd_bank_* / fsvit_emd_rerank of fsvit.h)
int launch_emd_bank_accumulate(const float* tok, const void* label, int label_is_int64, int S, int n_classes, int N, int C, float* sum, int* count,
                               int* invalid, hipStream_t s);
int launch_emd_bank_finalize(const float* sum, const int* count, int n_classes, int N, int C, float* tok, float* xhat, float* pooled, float* proto, int* empty,
                             hipStream_t s);
int launch_emd_rerank(const float* qtok, const float* qxhat, const float* qpooled, int Q, const float* btok, const float* bxhat, const float* bpooled,
                      const int* empty, int n_classes, const int* cand, int M, int N, int C, float temperature, int K, float* logits, int* classes,
                      float* values, float* prob, int* status_count, int* invalid, hipStream_t s);
int launch_emd_solve(const float* cost, const float* w1, const float* w2, int B, int N, float* flow, int* status, int* naug, hipStream_t s);
// The 5-shot SFC fine-tune on the device, one workgroup per episode.  workspace = emd_sfc_workspace_bytes(E, way, n, bs, N, C)
size_t emd_sfc_workspace_bytes(int E, int way, int n, int bs, int N, int C);
int launch_emd_sfc_steps(const float* support, const int* label, const int* ids, int n_steps, int first, int E, int way, int n, int bs, int N, int C,
                         float temperature, float lr, float momentum, float dampening, float* sfc, float* buf, int* status_count, void* ws, hipStream_t s);
}  // namespace fsvit
