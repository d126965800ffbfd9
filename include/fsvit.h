/* fsvit — C-ABI of the MI355X-native few-shot ViT hot path (libfsvit.so).
 *
 * The reference (DongSky/few-shot-vit) is 100 % Python: its boundary for this path is the
 * `models.make / nn.Module.forward` contract, not an FFI.  These entry points are
 * what a ctypes binding of that contract calls; each one names the reference
 * interface it replaces.  Plain pointers and sizes only — no torch types.
 *
 * Conventions
 *   - every `*_dev` / activation / output pointer is a DEVICE pointer owned by the caller;
 *     `fsvit_tensor.data` pointers are HOST pointers (state-dict tensors, fp32, contiguous);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only enqueue work;
 *   - return 0 on success; > 0 is a hipError_t, < 0 an fsvit error; `fsvit_last_error()` (thread
 *     local) describes the last failure;
 *   - `dtype` selects storage + MFMA arithmetic of activations/weights: FSVIT_F32 = exact fp32
 *     MFMA (v_mfma_f32_16x16x4_f32, the parity mode), FSVIT_BF16 = bf16 MFMA with fp32 accumulate, FSVIT_F16 = fp16 MFMA with
 *     fp32 accumulate (eval engines only: same kernels, same rate, 3 more mantissa bits than bf16; |activations| must stay
 *     below 65504, which BatchNorm / LayerNorm networks do with a wide margin).  FSVIT_BF16X2 / FSVIT_F16X2 (eval engines,
 *     fsvit_conv_gemm and - FSVIT_BF16X2 only - the two trainers, which pack the limb words of the weights and of the weight-gradient
 *     GEMM's activation operand on the device every step): fp32 storage as FSVIT_F32, but every GEMM runs on the 16-bit MFMA with both operands split into two 16-bit
 *     limbs (hi + lo; two MFMAs per K chunk = all four limb products, fp32 accumulate): 16 (bf16 limbs) / 22 (fp16 limbs) significand
 *     bits per operand at 1/4 of the 16-bit MFMA rate = 4 x the fp32-MFMA rate.  Weights given to fsvit_conv_gemm in these modes are
 *     4-byte limb pairs (upper half hi, lower half lo).
 */
#ifndef FSVIT_H
#define FSVIT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { FSVIT_F32 = 0, FSVIT_BF16 = 1, FSVIT_F16 = 2, FSVIT_BF16X2 = 3, FSVIT_F16X2 = 4 };
enum { FSVIT_ACT_NONE = 0, FSVIT_ACT_GELU = 1, FSVIT_ACT_LRELU = 2,
       FSVIT_ACT_MUL = 3 /* fsvit_op_conv_train only: y = conv(x) * mul, the data-gradient GEMM times the saved GELU derivative */ };
enum { FSVIT_HEAD_COS = 0, FSVIT_HEAD_SQR = 1, FSVIT_HEAD_DOT = 2 };
enum {
  FSVIT_ERR_ARG = -1,        /* bad argument / unsupported configuration        */
  FSVIT_ERR_KEY = -2,        /* state-dict key missing or wrong shape (KeyError) */
  FSVIT_ERR_IMG_SIZE = -3,   /* input image size does not match the model (AssertionError) */
  FSVIT_ERR_WORKSPACE = -4   /* workspace too small                              */
};

const char* fsvit_last_error(void);
/* Build identification: "fsvit <version> gfx950". */
const char* fsvit_version(void);

/* ---------------------------------------------------------------- Visformer encoder
 * Replaces `Visformer.__init__` + `load_state_dict` + `Visformer.forward` in eval mode
 * (test_phase/models/visformer.py:291-462; factory visformer_small_80 :482-487). */
typedef struct fsvit_visformer fsvit_visformer;

typedef struct fsvit_tensor {
  const char* name;       /* state-dict key relative to the encoder, e.g. "stem.conv1.weight" */
  const float* data;      /* HOST pointer, fp32, contiguous, PyTorch layout ([O,I,kh,kw], [C], [1,C,H,W]) */
  int ndim;
  int64_t shape[4];
} fsvit_tensor;

typedef struct fsvit_visformer_cfg {   /* visformer.py:292-295 arguments that shape the eval path */
  int img_size;
  int init_channels;
  int embed_dim;
  int depth[3];
  int num_heads;
  float mlp_ratio;
  int group;
  float bn_eps;
} fsvit_visformer_cfg;

/* Folds every eval-mode BatchNorm into the adjacent conv (visformer.py:118-124), reorders conv
 * weights to K-major (ky,kx,c), pads head dims for MFMA, converts to `dtype` and uploads.
 * Fails with FSVIT_ERR_KEY when a key of SURVEY.md Appendix A is absent or mis-shaped
 * (load_state_dict(strict=True) behaviour, models/models.py:21-26). */
int fsvit_visformer_create(const fsvit_visformer_cfg* cfg, const fsvit_tensor* state_dict, int n_tensors,
                           int dtype, fsvit_visformer** out);
void fsvit_visformer_destroy(fsvit_visformer* h);
int fsvit_visformer_out_dim(const fsvit_visformer* h);            /* `.out_dim` (visformer.py:298) */
int fsvit_visformer_dtype(const fsvit_visformer* h);
/* Bytes of scratch needed to push `chunk_images` images through the encoder at once. */
size_t fsvit_visformer_workspace_bytes(const fsvit_visformer* h, int chunk_images);
/* x_nchw_dev: [n_img,3,img,img] fp32 (what `data.cuda()` hands the model, test_few_shot.py:81).
 * feat_dev:   [n_img,out_dim] fp32 pooled features (visformer.py:462).
 * Images are processed in chunks sized to `ws_bytes` (at least one image must fit). */
int fsvit_visformer_forward(fsvit_visformer* h, const float* x_nchw_dev, int n_img, int img_h, int img_w,
                            float* feat_dev, void* ws_dev, size_t ws_bytes, void* stream);
/* Test hook: copy the named residual-stream activation of the FIRST chunk (NHWC, storage dtype) to
 * dst_dev during the next forwards.  Names: "stem" (after max-pool + pos_embed1), "stage1.N",
 * "patch_embed2"/"patch_embed3" (incl. pos_embed), "stage2.N", "stage3.N".  dst_dev NULL clears. */
int fsvit_encoder_set_tap(void* encoder, const char* name, void* dst_dev, size_t bytes);   /* ViT names: "embed", "blocks.N" */

/* Live per-launch timing (bench.py roofline leg): between begin and end every kernel launch of
 * fsvit_visformer_forward / fsvit_vit_forward is bracketed by HIP events ON THE STREAM IT IS LAUNCHED ON.  `end`
 * synchronises and returns one record per (layer, kernel) with summed algorithmic FLOPs (2*MAC,
 * unpadded dims), summed milliseconds and the launch count. */
typedef struct fsvit_prof_rec {
  char layer[48];     /* e.g. "stem.conv3", "stage2.attn.qkv" */
  int kernel_id;      /* see fsvit_kernel_name */
  int launches;
  double flops;
  double ms;
} fsvit_prof_rec;
int fsvit_encoder_profile_begin(void* encoder);
int fsvit_encoder_profile_end(void* encoder, fsvit_prof_rec* out, int max_recs, int* n_out);
/* Device kernel (template instantiation) behind a kernel_id, as rocprofv3 --kernel-trace names it. */
const char* fsvit_kernel_name(int kernel_id, int dtype);

/* ---------------------------------------------------------------- ViT / DeiT encoder
 * Replaces `VisionTransformer.__init__` + `load_state_dict` + `forward` in eval mode (test_phase/models/deit.py:139-218;
 * factories deit_{tiny,small,base,nano}_patch16_224, deit_{nano,micro}_patch6_84, :220-357).  LayerNorm eps 1e-6,
 * Linear layers with bias, qkv_bias=True, cls token at index 0, features = norm(x)[:, 0].  Same conventions as the
 * Visformer handle; state-dict keys of SURVEY.md Appendix A (DeiT part). */
typedef struct fsvit_vit fsvit_vit;
typedef struct fsvit_vit_cfg {          /* deit.py:142-144 */
  int img_size;
  int patch_size;
  int embed_dim;
  int depth;
  int num_heads;
  float mlp_ratio;
  float ln_eps;
} fsvit_vit_cfg;
int fsvit_vit_create(const fsvit_vit_cfg* cfg, const fsvit_tensor* state_dict, int n_tensors, int dtype, fsvit_vit** out);
void fsvit_vit_destroy(fsvit_vit* h);
int fsvit_vit_out_dim(const fsvit_vit* h);                           /* `.out_dim` (deit.py:147) */
size_t fsvit_vit_workspace_bytes(const fsvit_vit* h, int chunk_images);
int fsvit_vit_forward(fsvit_vit* h, const float* x_nchw_dev, int n_img, int img_h, int img_w, float* feat_dev,
                      void* ws_dev, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- LV-ViT encoder
 * Replaces `LV_ViT.__init__` + `load_state_dict` + `forward` in eval mode for the `lvvit_micro_80` factory
 * (meta_tuning_sun_m/models/lvvit.py:413-546, :583): ConvBlock stem (conv1 s2 / conv2 / conv3 + downsample at stem_channels, eval
 * BatchNorm, LeakyReLU(0.1), MaxPool2d(2)), a 4x4 / stride 4 projection to embed_dim, cls token + pos_embed, pre-LN blocks
 * (qkv_bias=False, residual branches divided by skip_lam), features = norm(x)[:, 0].  Same conventions as the ViT handle;
 * state-dict keys `patch_embed.{conv1,bn1,conv2,bn2,conv3,bn3,downsample.0,downsample.1,proj}.*`, `cls_token`, `pos_embed`,
 * `blocks.N.*`, `norm.*`.  This handle is the eval engine; training runs on the fsvit_lvvit_trainer handle further down. */
typedef struct fsvit_lvvit fsvit_lvvit;
typedef struct fsvit_lvvit_cfg {        /* lvvit.py:583-587 */
  int img_size;                         /* 80 */
  int stem_channels;                    /* 96: a multiple of 32 */
  int embed_dim;                        /* 384 */
  int depth;                            /* 8 */
  int num_heads;                        /* 6 */
  float mlp_ratio;                      /* 3 */
  float skip_lam;                       /* 2 */
  float ln_eps;                         /* 1e-5 (nn.LayerNorm default) */
  float bn_eps;                         /* 1e-5 */
} fsvit_lvvit_cfg;
int fsvit_lvvit_create(const fsvit_lvvit_cfg* cfg, const fsvit_tensor* state_dict, int n_tensors, int dtype, fsvit_lvvit** out);
void fsvit_lvvit_destroy(fsvit_lvvit* h);
int fsvit_lvvit_out_dim(const fsvit_lvvit* h);
size_t fsvit_lvvit_workspace_bytes(const fsvit_lvvit* h, int chunk_images);
int fsvit_lvvit_forward(fsvit_lvvit* h, const float* x_nchw_dev, int n_img, int img_h, int img_w, float* feat_dev,
                        void* ws_dev, size_t ws_bytes, void* stream);
/* The same forward with the token map next to the cls feature (sun_meta_training/models/lvvit.py:552 returns x_local, x1): tokens_dev
 * [n_img][25][embed_dim] fp32 = norm(x)[:, 1:], token-major (the caller's permute gives the reference's [n_img, embed_dim, 5, 5]).  Chunked like the plain
 * forward, every chunk's rows at its image offset - any n_img; feat_dev holds the same bits as the plain forward's. */
int fsvit_lvvit_forward_map(fsvit_lvvit* h, const float* x_nchw_dev, int n_img, int img_h, int img_w, float* feat_dev, float* tokens_dev, void* ws_dev,
                            size_t ws_bytes, void* stream);

/* LV-ViT stem conv2 (pool = 0) or conv3 + downsample tail + LeakyReLU + MaxPool2d(2) (pool = 1) at 96 channels on the dedicated kernel: x NHWC
 * [B][H][W][96] (bf16 / f16, W = 40, H a multiple of 8), w the 128-channel weight image [128][9 * 128 (+ 64)] (k = tap * 128 + c, zero past 96
 * channels and rows; tail slice last), bias [96] fp32 or NULL, x2 the im2col rows [B*H*W][x2_cstride] (pool = 1, K2 = 32); y NHWC, 96 channels. */
int fsvit_stem96_conv(const void* x_dev, const void* w_dev, const float* bias_dev, const void* x2_dev, int x2_cstride, int K2, void* y_dev,
                      int B, int H, int W, int pool, int dtype, void* stream);

/* ---------------------------------------------------------------- episode head
 * Replaces MetaBaseline.forward after the encoder call (test_phase/models/meta_baseline.py:33-47),
 * utils.compute_logits (utils/__init__.py:78-101) and, per episode, F.cross_entropy +
 * utils.compute_acc with fs.make_nk_label labels (test_few_shot.py:87-90).
 * feat_shot_dev [E,way,shot,D], feat_query_dev [E,Q,D] fp32 -> logits_dev [E,Q,way];
 * acc_dev / loss_dev [E] may be NULL. */
int fsvit_proto_head(const float* feat_shot_dev, const float* feat_query_dev, int E, int way, int shot, int Q, int D,
                     float temp, int method, float* logits_dev, float* acc_dev, float* loss_dev, void* stream);

/* The same with the temperature read from DEVICE memory (`self.temp` is an nn.Parameter the optimizer updates on the GPU, meta_baseline.py:20-21):
 * the meta-tuning step never brings it to the host, so the step issues no stream synchronisation. */
int fsvit_proto_head_devtemp(const float* feat_shot_dev, const float* feat_query_dev, int E, int way, int shot, int Q, int D,
                             const float* temp_dev, int method, float* logits_dev, float* acc_dev, float* loss_dev, void* stream);

/* The same head over rows gathered from a feature table (one encoder feature per image, kept across episodes): table_dev [N,D] fp32, idx_dev
 * [E,way,shot+n_query] slot numbers into it (int64 when idx_is_int64, else int32) in the sampler's class-major order - the first `shot` entries of a class
 * are its shots (fs.split_shot_query), query q = c * n_query + j is idx[e][c][shot + j], labels follow make_nk_label -> logits_dev [E,way*n_query,way];
 * acc_dev / loss_dev [E] may be NULL.  The temperature is *temp_dev (device) when temp_dev != NULL, else `temp`.  For the same rows the outputs carry the
 * bits of fsvit_proto_head (one device body serves both kernels); they do not depend on E or on the other episodes.
 * A slot outside [0, N) never becomes an address: the row is read from slot 0, the episode's acc, loss and logits block are written as NaN and
 * *invalid_dev (an int the caller zeroes once) is raised by one per such entry.
 * Limits and refusals (FSVIT_ERR_ARG, nothing launched): those of fsvit_proto_head - (way * D + 2 * way * n_query) * 4 bytes of LDS <= 160 KiB, i.e.
 * way <= 79 at D = 512 - and N >= 1, shot >= 1, n_query >= 1, non-NULL table / idx / logits / invalid.  E == 0 is a no-op. */
int fsvit_proto_head_gather(const float* table_dev, int N, int D, const void* idx_dev, int idx_is_int64, int E, int way, int shot, int n_query, float temp,
                            const float* temp_dev, int method, float* logits_dev, float* acc_dev, float* loss_dev, int* invalid_dev, void* stream);

/* Whole `MetaBaseline.forward(x_shot, x_query)` (meta_baseline.py:24-47) in eval mode:
 * x_shot_dev [E,way,shot,3,H,W], x_query_dev [E,Q,3,H,W] fp32 -> logits_dev [E,Q,way].
 * feat_dev: scratch [(E*way*shot + E*Q), out_dim] fp32. */
int fsvit_meta_baseline_forward(void* encoder /* fsvit_visformer*, fsvit_vit* or fsvit_lvvit* */, const float* x_shot_dev, const float* x_query_dev,
                                int E, int way, int shot, int Q, int img_h, int img_w, float temp, int method,
                                float* logits_dev, float* acc_dev, float* loss_dev, float* feat_dev,
                                void* ws_dev, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- prototype bank: a labelled support set, encoded once and queried many times
 * The head above re-forms the prototypes of one rectangular episode on every call.  These four entries serve a support set with any number of
 * examples per class, filled in any number of calls, and any number of classes (proto_bank.hip).  All tensors fp32 and dense; `method` as above.
 * Shared refusals (FSVIT_ERR_ARG, nothing launched): a NULL pointer that is not marked optional, way < 1 or way > 65536, D < 1 or D > 8192.
 *
 * Accumulate: feat_dev [S,D], label_dev [S] (int64 when label_is_int64, else int32) -> sum_dev [way,D] +=, count_dev [way] +=, *invalid_dev += the number
 * of labels outside [0, way), which contribute nothing else.  The caller zeroes the three outputs once.  A class's rows are added in ascending support
 * index on top of the stored sum: deterministic, and two calls over a split give the bits of one chain.  S == 0 is a no-op, S < 0 refused. */
int fsvit_proto_bank_accumulate(const float* feat_dev, const void* label_dev, int label_is_int64, int S, int way, int D, float* sum_dev, int* count_dev,
                                int* invalid_dev, void* stream);
/* Finalize: proto_dev [way,D] = sum / count, for FSVIT_HEAD_COS followed by F.normalize with its 1e-12 clamp (meta_baseline.py:37-38);
 * empty_dev [way] = 1 and a zero prototype row where count == 0, else 0. */
int fsvit_proto_bank_finalize(const float* sum_dev, const int* count_dev, int way, int D, int method, float* proto_dev, int* empty_dev, void* stream);
/* Logits: utils.compute_logits (utils/__init__.py:78-101) of query_dev [Q,D] against proto_dev [way,D] as fsvit_proto_bank_finalize wrote it ->
 * logits_dev [Q,way]; COS normalises the query rows (1e-12 clamp), SQR is the negative squared distance, DOT the plain product, each times the
 * temperature: *temp_dev (device) when temp_dev != NULL, else `temp`, which must be finite.  The device value is not checked (reading it would be a host
 * synchronisation): a NaN or inf there goes into the logits, as with fsvit_proto_head_devtemp.  Classes flagged in empty_dev (NULL = none) score -inf.
 * pred_dev [Q] (optional) = the first maximum of each row.  Limits: D a multiple of 4, query_dev and proto_dev 16-byte aligned.  Q == 0 is a no-op. */
int fsvit_proto_bank_logits(const float* query_dev, const float* proto_dev, const int* empty_dev, int Q, int way, int D, float temp, const float* temp_dev,
                            int method, float* logits_dev, int* pred_dev, void* stream);
/* Top-k: the K best classes of every row of the matrix fsvit_proto_bank_logits would write, their logits and the row's log-sum-exp, without that
 * matrix.  values_dev [Q,K] fp32 and indices_dev [Q,K] int32 are the first K entries of a stable descending sort of the row (larger logit first, then
 * the lower class; every logit carries the bits fsvit_proto_bank_logits gives it); an empty class takes part with -inf, ranks beyond `way` hold
 * (-inf, -1).  lse_dev [Q] (optional) = log sum exp over the non-empty classes, -inf for a row that has none.  The class axis is cut into segments of
 * 1024 classes, n_seg = ceil(way / 1024), and the grid is ceil(Q / 64) x n_split workgroups, each over a contiguous run of whole segments; a second
 * launch merges the n_split lists per row and folds the per-segment sums in ascending segment order.  values / indices are the same bits for every
 * n_split, and lse_dev[q] depends on (way, D, method, temperature, row q) alone - not on n_split, Q or the other rows.
 * n_split == 0 lets the library choose: min(n_seg, max(1, ceil(CUs / ceil(Q / 64)))) with the CU count of the current device - the fewest splits
 * that give every CU a workgroup, as far as the bank has segments for it.
 * Limits and refusals: those of fsvit_proto_bank_logits, and 1 <= K <= 32, 0 <= n_split <= n_seg, workspace_dev non-NULL, 4-byte aligned and of at
 * least fsvit_proto_bank_topk_workspace_bytes(Q, way, K, n_split) bytes (the same n_split; 0 bytes are returned for arguments the call would refuse).
 * Q == 0 is a no-op that touches no output.  Inputs are finite by contract: a NaN logit has no place in the order. */
size_t fsvit_proto_bank_topk_workspace_bytes(int Q, int way, int K, int n_split);
int fsvit_proto_bank_topk(const float* query_dev, const float* proto_dev, const int* empty_dev, int Q, int way, int D, float temp, const float* temp_dev,
                          int method, int K, int n_split /* 0: the library chooses */, float* values_dev, int* indices_dev, float* lse_dev /* may be NULL */,
                          void* workspace_dev, size_t workspace_bytes, void* stream);
/* `--sauc` of the reference's test_few_shot.py (meta_tuning_sun_m/test_few_shot.py:95-112): feat_shot_dev [E,shot,D] (the shots of class 0),
 * feat_query_dev [E,Q,D], the first Q / 2 queries positive -> auc_dev [E] = roc_auc_score of the cosine scores against the normalised mean shot
 * = (#{pos > neg} + #{pos == neg} / 2) / (Q / 2)^2; score_dev [E,Q] optional.  Limits: shot >= 1, Q even, 2 <= Q <= 4096.  E == 0 is a no-op. */
int fsvit_proto_auc(const float* feat_shot_dev, const float* feat_query_dev, int E, int shot, int Q, int D, float* auc_dev, float* score_dev, void* stream);
/* The same reduction over rows gathered from a feature table (one encoder feature per image, kept across episodes): table_dev [N,D] fp32,
 * shot_slots_dev [E,shot] the slots of class 0's shots (class 1's shots are never read), query_slots_dev [E,Q] the slots of the queries, the first Q / 2
 * positive (both int64 when idx_is_int64, else int32) -> auc_dev [E], score_dev [E,Q] (optional).  For the same rows the outputs carry the bits of
 * fsvit_proto_auc (one device body serves both kernels); they do not depend on E or on the other episodes.
 * A slot outside [0, N) never becomes an address: the row is read from slot 0, the episode's auc and score row are written as NaN and *invalid_dev (an int
 * the caller zeroes once) is raised by one per such entry.
 * Limits and refusals (FSVIT_ERR_ARG, nothing launched, nothing written): those of fsvit_proto_auc - shot >= 1, Q even, 2 <= Q <= 4096, 1 <= D <= 8192 - and
 * N >= 1, non-NULL table / shot_slots / query_slots / auc / invalid.  E == 0 is a no-op. */
int fsvit_proto_auc_gather(const float* table_dev, int N, int D, const void* shot_slots_dev, const void* query_slots_dev, int idx_is_int64, int E, int shot,
                           int Q, float* auc_dev, float* score_dev, int* invalid_dev, void* stream);

/* ---------------------------------------------------------------- operator level (tests, reuse)
 * Implicit-GEMM conv with fused epilogue; see few-shot-vit_amd/csrc/conv_gemm.h for the layout.
 * x NHWC [B,H,W,x_cstride]; w [groups][N][Kw] K-major (ky,kx,c); y NHWC [B,OH,OW,y_cstride]. */
int fsvit_conv_gemm(const void* x_dev, const void* w_dev, const float* bias_dev, const void* res_dev,
                    const float* pos_dev, void* y_dev, int B, int H, int W, int Cin, int x_cstride,
                    int KH, int KW, int stride, int pad, int N, int y_cstride, int Kw, int groups,
                    int act, int res_first, int dtype, void* stream);
/* Fused tail of the stem ConvBlock (visformer.py:213 conv3, :216-217 downsample, :232-237 add + LeakyReLU + MaxPool2d(2)) + pos_embed1
 * (:431): y [B, H/2, W/2, N] = maxpool2(lrelu(conv3x3_pad1(x [B,H,W,Cin], w[:, 0:9*Cin]) + x2 [B*H*W][x2_cstride](:, 0:K2) . w[:, Kw-bke : Kw-bke+K2]
 * + bias)) + pos [(H/2)*(W/2)][N]; BatchNorms folded into w / bias by the caller; bke = 128 bytes of K (64 bf16 / 32 fp32). */
int fsvit_conv_stem_tail(const void* x_dev, const void* w_dev, const float* bias_dev, const float* pos_dev, const void* x2_dev, int x2_cstride,
                         int K2, void* y_dev, int B, int H, int W, int Cin, int N, int Kw, int dtype, void* stream);
/* qkv [B*S][3*heads*hdp] -> ctx [B*S][heads*hdp] = softmax(scale q k^T) v per (image, head) (visformer.py:183-190).  Row layout of qkv: (q | k | v, head,
 * channel), every head padded from its hd channels to hdp.  dtype: any of the five; FSVIT_BF16X2 / FSVIT_F16X2 take fp32 rows and form every product
 * from two 16-bit limbs per operand (a shape without a two-limb kernel runs the exact-fp32 one).
 * PAD CONTRACT: the kernels contract over all hdp channels, so the pad channels hd .. hdp-1 of q, k and v must be ZERO (the weight packers write them
 * so); the pad channels of ctx are then written as exact zeros.
 * Refused with FSVIT_ERR_ARG and a message, nothing launched: an unknown dtype, a null pointer, B < 0, heads < 1, S < 1, hdp < 16 or not a multiple of 16,
 * and a shape no kernel covers - 16-bit: S > 224, or S > 128 where hdp / 16 is not one of 2, 3, 4, 6, 8; fp32 and two-limb: S > 208, or S > 128 where
 * hdp / 16 is not one of 1 .. 5 (13 key tiles of fp32 rows at hdp 96 / 128 pass the 160 KB of LDS), or 113 <= S <= 128 at hdp >= 96; any type: the generic
 * kernel's (S <= 128) LDS image past 160 KB.  B == 0 returns 0. */
int fsvit_attention(const void* qkv_dev, void* ctx_dev, int B, int S, int heads, int hdp, float scale,
                    int dtype, void* stream);
/* The kernel fsvit_attention takes for (S, hdp, dtype), host only, nothing launched: family * 100000 + elem * 10000 + NKT * 100 + NDT with family 1 =
 * attention_v2_kernel<elem, NKT key tiles, NDT head-dim tiles>, 2 = the generic attention_kernel<elem> (NKT = NDT = 0); elem 0 = float, 1 = the 16-bit
 * type, 2 = two-limb; -1 = refused.  The launcher decides by this very function (attention.hip attention_route). */
int fsvit_op_attention_route(int S, int hdp, int dtype);
/* Fused qkv conv + attention core of a Visformer stage-2 Attention block (visformer.py:172-190; the eval BatchNorm folded into the
 * conv as column scale + bias by the caller), bf16, Visformer-S geometry only (C = 256, 6 heads, head dim padded to 48, S <= 112):
 * x rows [B*S][C] -> ctx rows [B*S][heads*hdp].  wqkv [3*heads*hdp][kw] K-major bf16, rows ordered (q|k|v, head, z); bias fp32
 * [3*heads*hdp] or NULL.  Equals fsvit_conv_gemm (1x1, N = 3*heads*hdp) followed by fsvit_attention without the qkv tensor.
 * Also the stage-3 geometry on the row-wise kernel: C = 512, head dim padded to 96, S <= 32 (one image per wave). */
int fsvit_qkv_attention(const void* x_dev, const void* wqkv_dev, int kw, const float* bias_dev, void* ctx_dev, int B, int S, int C,
                        int heads, int hdp, float scale, void* stream);
/* norm1 + qkv Linear + attention core of a ViT / DeiT block in one launch (deit.py:40-58 Attention.forward, :69 `x + attn(norm1(x))` without the
 * proj): x rows [B*S][C] bf16 -> ctx rows [B*S][heads*hdp]; LayerNorm without affine (gamma / beta folded into wqkv / bias by the caller),
 * wqkv [3*heads*hdp][kw] K-major bf16 rows ordered (q|k|v, head, z), bias fp32 or NULL.  Built for C = 384, head dim 64, S <= 256
 * (DeiT-S/16: 197 tokens).  Equals fsvit_ln_linear_rows followed by fsvit_attention without the qkv tensor in HBM. */
int fsvit_vit_ln_qkv_attention(const void* x_dev, const void* wqkv_dev, int kw, const float* bias_dev, void* ctx_dev, int B, int S, int C,
                               int heads, int hdp, float eps, float scale, void* stream);
/* One fused Visformer stage-1 block (visformer.py:259-263 with attn_disabled + spatial_conv Mlp :152-163), bf16,
 * 20x20 tokens, 128 channels, 256 hidden, 8 groups: y = x + conv3(GELU(conv2_g(GELU(conv1(x)+b1)))).
 * x, y NHWC [B,20,20,128] bf16 (distinct buffers); w1 [256][128], w2 [8][32][320], w3 [128][256] packed K-major bf16.
 * Always the 16-wave ring kernel (stage1_ring.hip): the in-process cross-check of fsvit_stage1_block_hw. */
int fsvit_stage1_block(const void* x_dev, void* y_dev, const void* w1_dev, const float* b1_dev, const void* w2_dev,
                       const void* w3_dev, int B, void* stream);
/* The same block for any square token map of 4 .. 20 a side: x, y NHWC [B,H,W,128], dtype FSVIT_BF16 / FSVIT_F16; weights as above.  This is the launch the
 * engines run: stage1_w4.hip (one wave per SIMD, weights in registers / AGPRs, x and the first hidden map in pixel rings; bf16: GELU by table look-up on
 * the bf16-rounded pre-activation). */
int fsvit_stage1_block_hw(const void* x_dev, void* y_dev, const void* w1_dev, const float* b1_dev, const void* w2_dev, const void* w3_dev, int B, int H, int W,
                          int dtype, void* stream);
/* Fused Mlp of a Visformer attention block (visformer.py:146-150 with spatial_conv=False, + the residual of :262):
 * y = x + W2 GELU(W1 x + b1) (+ b2), rows = tokens.  bf16; C = 256 / hidden = 1024 and C = 512 / hidden = 2048 (stages 2, 3 of
 * Visformer-S).  x, y [M][C]
 * (y may alias x); w1 [hid][k1w], w2 [C][k2w] K-contiguous bf16 rows (BatchNorm already folded into w1 / b1); b1 [hid], b2 [C]
 * fp32 or NULL.  The operator form packs the weights on every call (the engine packs once per checkpoint). */
int fsvit_mlp_rows(const void* x_dev, void* y_dev, const void* w1_dev, int k1w, const float* b1_dev, const void* w2_dev, int k2w,
                   const float* b2_dev, int M, int C, int hid, void* stream);
/* The same with the attention block's proj conv + residual (visformer.py:176,:261) as a prologue on the same rows:
 * x1 = x + wp ctx; y = x1 + W2 GELU(W1 x1 + b1) (+ b2).  ctx [M][KC] = attention output with zero-padded head dims, wp [C][kpw];
 * (C, KC) = (256, 288) or (512, 576).  ctx == NULL: plain fsvit_mlp_rows. */
int fsvit_proj_mlp_rows(const void* x_dev, void* y_dev, const void* ctx_dev, const void* wp_dev, int kpw, int KC, const void* w1_dev, int k1w,
                        const float* b1_dev, const void* w2_dev, int k2w, const float* b2_dev, int M, int C, int hid, void* stream);
/* The ViT / DeiT block tail (test_phase/models/deit.py:69-72, `x = x + attn.proj(ctx); x = x + mlp(norm2(x))`) on token-major rows, bf16,
 * (C, hidden, KC) = (384, 1536, 384):  x1 = x + bp + wp ctx;  y = x1 + b2 + W2 GELU(W1 LN(x1) + b1), LN = (x1 - mean) / sqrt(var + eps) without
 * affine - the caller folds norm2's gamma / beta into w1 / b1 (W1 diag(gamma), b1 + W1 beta).  In place (y == x) allowed. */
int fsvit_vit_block_tail(const void* x_dev, void* y_dev, const void* ctx_dev, const void* wp_dev, int kpw, int KC, const float* bp_dev,
                         const void* w1_dev, int k1w, const float* b1_dev, const void* w2_dev, int k2w, const float* b2_dev, int M, int C, int hid,
                         float eps, void* stream);
/* The ViT / DeiT block head up to the qkv Linear (deit.py:40-47,:69 `attn(norm1(x))`): y [M][N] = b + W LN(x [M][C]) on token-major bf16 rows,
 * C = 384, N a multiple of 32, LN without affine (the caller folds norm1's gamma / beta into w [N][kw] / b).  C = 512: the same row-wise kernel
 * WITHOUT the LayerNorm, y = b + W x (the Visformer stage-3 qkv conv with its eval BatchNorm folded, visformer.py:175; eps ignored, b may be NULL). */
int fsvit_ln_linear_rows(const void* x_dev, void* y_dev, const void* w_dev, int kw, const float* b_dev, int M, int C, int N, float eps, void* stream);
/* PatchEmbed of a Visformer stage (test_phase/models/visformer.py:266-288: Conv2d k2 s2 -> BatchNorm, then `x + pos_embed`, :437-447) on the
 * row-wise kernel: x NHWC bf16 [B][H][H][Ci], 4 Ci = 512; w [N][kw] K-major in (ky, kx, c) order with the eval BatchNorm folded in, bias fp32 [N]
 * or NULL, pos fp32 [(H/2)^2][N]; y [B (H/2)^2][N] bf16. */
int fsvit_patch_embed2x2(const void* x_dev, void* y_dev, const void* w_dev, int kw, const float* bias_dev, const float* pos_dev, int B, int H, int Ci,
                         int N, void* stream);
/* The row-kernel operators with the storage type spelled out: NAME_dt(..., dtype, stream) runs the bf16 (FSVIT_BF16) or the fp16 (FSVIT_F16) build of
 * NAME's kernel on tensors of that type; any other dtype is FSVIT_ERR_ARG.  NAME(..., stream) above / below is NAME_dt(..., FSVIT_BF16, stream). */
int fsvit_mlp_rows_dt(const void* x_dev, void* y_dev, const void* w1_dev, int k1w, const float* b1_dev, const void* w2_dev, int k2w,
                      const float* b2_dev, int M, int C, int hid, int dtype, void* stream);
int fsvit_proj_mlp_rows_dt(const void* x_dev, void* y_dev, const void* ctx_dev, const void* wp_dev, int kpw, int KC, const void* w1_dev, int k1w,
                           const float* b1_dev, const void* w2_dev, int k2w, const float* b2_dev, int M, int C, int hid, int dtype, void* stream);
int fsvit_vit_block_tail_dt(const void* x_dev, void* y_dev, const void* ctx_dev, const void* wp_dev, int kpw, int KC, const float* bp_dev,
                            const void* w1_dev, int k1w, const float* b1_dev, const void* w2_dev, int k2w, const float* b2_dev, int M, int C, int hid,
                            float eps, int dtype, void* stream);
int fsvit_ln_linear_rows_dt(const void* x_dev, void* y_dev, const void* w_dev, int kw, const float* b_dev, int M, int C, int N, float eps, int dtype,
                            void* stream);
int fsvit_patch_embed2x2_dt(const void* x_dev, void* y_dev, const void* w_dev, int kw, const float* bias_dev, const float* pos_dev, int B, int H, int Ci,
                            int N, int dtype, void* stream);
int fsvit_qkv_attention_dt(const void* x_dev, const void* wqkv_dev, int kw, const float* bias_dev, void* ctx_dev, int B, int S, int C,
                           int heads, int hdp, float scale, int dtype, void* stream);
int fsvit_vit_ln_qkv_attention_dt(const void* x_dev, const void* wqkv_dev, int kw, const float* bias_dev, void* ctx_dev, int B, int S, int C,
                                  int heads, int hdp, float eps, float scale, int dtype, void* stream);
int fsvit_stem_conv1_dt(const float* x_nchw_dev, const void* w_dev, int kw, const float* bias_dev, void* patches_dev, void* c1_dev,
                        int B, int H, int W, int dtype, void* stream);
/* ---------------------------------------------------------------- operator entries of the evaluation stem / conv / stage-1 kernels (tests)
 * fsvit_stem_conv1_dt with the layout of c1 spelled out: c1_planar != 0 stores c1 row-chunk-planar (element (b, row, col, c) at
 * ((b * 40 + row) * 8 + c / 8) * 320 + col * 8 + c % 8), the layout the planar eval stem hands to conv2; 0: NHWC rows. */
int fsvit_op_stem_conv1(const float* x_nchw_dev, const void* w_dev, int kw, const float* bias_dev, void* patches_dev, void* c1_dev,
                        int B, int H, int W, int dtype, int c1_planar, void* stream);
/* fsvit_stage1_block_hw as the engines launch it: prescaled != 0 runs the kernel on the 8 x W3 image (built per call by the same prescale launch the
 * engines use at load time), prescaled == 0 on W3 itself.  The two are specified to be bit-identical.  A test entry: with prescaled != 0 it allocates the
 * image, SYNCHRONISES the stream and frees it on every call. */
int fsvit_op_stage1_block_eval(const void* x_dev, void* y_dev, const void* w1_dev, const float* b1_dev, const void* w2_dev, const void* w3_dev, int B, int H,
                               int W, int dtype, int prescaled, void* stream);
/* One conv / GEMM launch through the evaluation dispatcher with every operand an engine can set.  Fields as in fsvit_conv_gemm, plus:
 *   x2 / x2_cstride / K2   the tail operand (one more K slice over rows aligned with the output pixels; its weights are the last slice of the packed rows);
 *   pool2                  2 x 2 max-pool behind the activation, pos added to the pooled pixels;
 *   y_rpi / y_row0         output row m of image b goes to row b * y_rpi + y_row0 + m % (OH * OW) (0 / 0: dense);
 *   x_planar / y_planar    that map is row-chunk-planar: element (b, row, col, c) at ((b * H + row) * (C / 8) + c / 8) * W * 8 + col * 8 + c % 8;
 *   w_cpad                 128: the weights are the 128-channel image of a 96-channel layer;
 *   c1f_*                  conv2 of the eval stem builds conv1's map on-chip from the raw NCHW fp32 images (x is not read) - images [0, c1f_split)
 *                          from c1f_raw, the rest from c1f_raw2 - and stores the im2col patch rows [B * H * W][32] to c1f_patches;
 *   stats                  per-workgroup partial sums of y and y^2 of the training forward: *stats_rows partial rows [rows][2][y_cstride] fp32.
 * Planar operands, w_cpad, the C1F fields and stats are accepted only for the layers whose kernel has them (FSVIT_ERR_ARG otherwise).
 * *route (may be NULL): 0 conv3x3_halo, 1 gemm256, 2 conv_gemm_v2, 3 the two-limb grouped 3x3 kernel. */
typedef struct fsvit_conv_eval_args {
  const void *x, *w;
  const float* bias;
  const void* res;
  const float* pos;
  void* y;
  const void* x2;
  float* stats;
  const float *c1f_raw, *c1f_raw2;
  void* c1f_patches;
  const void* c1f_w;
  const float* c1f_bias;
  int B, H, W, Cin, x_cstride, KH, KW, stride, pad, N, y_cstride, Kw, groups, act, res_first;
  int x2_cstride, K2, pool2, y_rpi, y_row0, x_planar, y_planar, w_cpad, c1f_split, c1f_kw;
} fsvit_conv_eval_args;
int fsvit_op_conv_eval(const fsvit_conv_eval_args* args, int dtype, int* route, int* stats_rows, void* stream);
/* ---------------------------------------------------------------- distillation head
 * Replaces, for sun_meta_training/offline.py: `LinearClassifier.forward` / its autograd (models/classifier.py:27-34) as used by
 * `TokenLabelOffline` (models/token_label.py:36-60) on the 25 tokens and on the pooled feature, `generate_softlabel`
 * (offline.py:57-76), `SoftTargetCrossEntropy` (offline.py:34-45) and the AdamW update (offline.py:233).  fp32, token-major rows. */
/* The distillation phase's encoder returns `(x, pooled)` (sun_meta_training/models/visformer.py:464): the post-norm token map
 * [n_img][25][512] fp32 (token-major; the reference's [B, 512, 5, 5] permuted by (0, 2, 3, 1)) of the last eval forward / train forward,
 * and the gradient hand-over for the train backward (added to the pooled feature's gradient path; consumed by the next backward). */
int fsvit_visformer_last_tokens(fsvit_visformer* h, const void* ws_dev, size_t ws_bytes, int n_img, float* tokens_dev, void* stream);
/* (train-mode counterparts: fsvit_visformer_train_tokens / fsvit_visformer_train_set_token_grad, declared with the trainer below) */
/* y [M][N] = x [M][K] w[N][K]^T + b[N] (b may be NULL); K % 4 == 0. */
int fsvit_linear_forward(const float* x_dev, const float* w_dev, const float* b_dev, float* y_dev, int M, int N, int K, void* stream);
/* dx [M][K] (+)= dy w (NULL: skipped), dw [N][K] = dy^T x and db [N] = column sums of dy (NULL: skipped); any N (dy is staged 256 classes at a time). */
int fsvit_linear_backward(const float* dy_dev, const float* x_dev, const float* w_dev, float* dx_dev, int accumulate_dx, float* dw_dev,
                          float* db_dev, int M, int N, int K, void* stream);
/* teacher token logits [B][T][C] (T = 25 tokens in (h, w) order = the reference's [B, C, 5, 5].permute(0, 2, 3, 1)) -> soft labels
 * [B*T][C+1]: top-k scatter for the T - bp tokens with the largest max logit, the reference's background row (on_value at column 1,
 * offline.py:61,71) for the other bp. */
int fsvit_token_softlabel(const float* teacher_logits_dev, float* soft_dev, int B, int T, int C, int k, int bp, double smoothing, void* stream);
/* row_loss [R] = -sum_c target log_softmax(logits) (the caller's mean is over R), dlogits [R][C] = grad_scale (softmax * sum(target) -
 * target) or NULL; any C. */
int fsvit_soft_target_ce(const float* logits_dev, const float* target_dev, float* row_loss_dev, float* dlogits_dev, int R, int C,
                         float grad_scale, void* stream);
/* F.normalize(x, dim=-1) of R rows of length D (utils.compute_logits metric 'cos', test_phase/utils/__init__.py:82-84; the
 * `nn-classifier` head, test_phase/models/classifier.py:38-55): y = x / max(|x|, 1e-12), inv_norm [R] for the backward
 * dx = (dy - y <y, dy>) * inv_norm. */
int fsvit_row_normalize(const float* x_dev, float* y_dev, float* inv_norm_dev, int R, int D, void* stream);
int fsvit_row_normalize_backward(const float* y_dev, const float* inv_norm_dev, const float* dy_dev, float* dx_dev, int R, int D, void* stream);
/* AdamW (decoupled weight decay), update number `step` >= 1: p, exp_avg m, exp_avg_sq v updated in place. */
int fsvit_adamw_step(float* p_dev, const float* g_dev, float* m_dev, float* v_dev, size_t n, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int step, void* stream);
/* The same update for a table of tensors in ONE launch (offline.py:233 `optimizer.step()` over every parameter of the student): items_dev = n_items rows of
 * five 8-byte words {p, g, m, v, numel} in device memory; every tensor at update number `step`; max_numel = the largest numel (sizes the grid). */
int fsvit_adamw_step_multi(const void* items_dev, int n_items, size_t max_numel, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                           void* stream);

int fsvit_im2col27(const float* x_nchw_dev, void* out_dev, int B, int H, int W, int dtype, void* stream);
/* im2col27 + stem conv1 + bn1 (folded) + LeakyReLU(0.1) in one pass (visformer.py:209-210,218), bf16, 80x80 images, 64 channels:
 * patches [B*1600][32] (the rows fsvit_im2col27 writes) and c1 [B*1600][64]; w [64][kw] K-major bf16 with K columns (ky,kx,c), kw >= 32. */
int fsvit_stem_conv1(const float* x_nchw_dev, const void* w_dev, int kw, const float* bias_dev, void* patches_dev, void* c1_dev,
                     int B, int H, int W, void* stream);
int fsvit_maxpool2_pos(const void* in_dev, const float* pos_dev, void* out_dev, int B, int OH, int OW, int C,
                       int dtype, void* stream);
/* feat [B][C] fp32 = scale[c] * mean over HW of x [B][HW][C] + shift[c];  HW >= 1, C >= 4, C % 4 == 0 (FSVIT_ERR_ARG otherwise). */
int fsvit_pool_affine(const void* x_dev, const float* scale_dev, const float* shift_dev, float* feat_dev,
                      int B, int HW, int C, int dtype, void* stream);

/* ---------------------------------------------------------------- meta-tuning step
 * Replaces the encoder part of `model.train(); logits = model(x_shot, x_query); loss.backward(); optimizer.step()`
 * (meta_tuning_sun_m/train_meta.py:161-177): train-mode Visformer forward (batch-statistics BatchNorm that also
 * updates running_mean / running_var in place, momentum 0.1, visformer.py:53-64; DropPath visformer.py:89-96)
 * with saved activations, and the backward to every parameter gradient.
 * Parameters stay in the framework's own fp32 tensors ON THE DEVICE (they change every step):
 *   name  reference state-dict key of the encoder ("stem.conv1.weight", "stage2.0.attn.qkv.weight", "norm.bn.running_var", ...)
 *   data  device pointer, fp32, PyTorch layout;  grad  device pointer of the same shape that train_backward OVERWRITES
 *         (NULL: not wanted; buffers such as running stats never get one). */
typedef struct fsvit_param {
  const char* name;
  float* data;
  float* grad;
  int64_t numel;
} fsvit_param;
typedef struct fsvit_visformer_trainer fsvit_visformer_trainer;
/* post-norm token map of the last train_forward / gradient hand-over for the next train_backward (distillation head, see above) */
int fsvit_visformer_train_tokens(fsvit_visformer_trainer* t, float* tokens_dev, void* stream);
int fsvit_visformer_train_set_token_grad(fsvit_visformer_trainer* t, const float* dtokens_dev);
int fsvit_visformer_trainer_create(const fsvit_visformer_cfg* cfg, int dtype, fsvit_visformer_trainer** out);
void fsvit_visformer_trainer_destroy(fsvit_visformer_trainer* t);
/* bytes of workspace one forward+backward over n_img images needs (saved activations + temporaries) */
size_t fsvit_visformer_trainer_workspace_bytes(fsvit_visformer_trainer* t, const fsvit_param* params, int n_params, int n_img,
                                               float drop_path_rate);
/* BatchNorm layers frozen inside the training step (utils.freeze_bn, meta_tuning_sun_m/train_meta.py:156-157, utils/__init__.py:150-153):
 * train_forward normalises with the running statistics and leaves them untouched; train_backward returns dz = gamma * invstd * dy and the
 * gamma / beta gradients against the running statistics.  Default off. */
int fsvit_visformer_trainer_set_freeze_bn(fsvit_visformer_trainer* t, int on);

/* x_nchw_dev [n_img,3,H,W] fp32 -> feat_dev [n_img,out_dim] fp32.  masks_dev: the DropPath Bernoulli draws, one row of
 * n_img 0/1 floats per DropPath call with a non-zero rate, in call order (stage-1 blocks: one call; stage-2/3 blocks: attn
 * then mlp) - the caller draws them (floor(keep + rand), visformer.py:93-95) so the random stream stays the framework's.
 * The workspace must stay untouched until train_backward returns. */
int fsvit_visformer_train_forward(fsvit_visformer_trainer* t, const fsvit_param* params, int n_params, const float* x_nchw_dev,
                                  int n_img, int img_h, int img_w, float drop_path_rate, const float* masks_dev, float* feat_dev,
                                  void* ws_dev, size_t ws_bytes, void* stream);
/* dfeat_dev [n_img,out_dim] fp32 -> every params[i].grad */
int fsvit_visformer_train_backward(fsvit_visformer_trainer* t, const fsvit_param* params, int n_params, const float* dfeat_dev,
                                   void* stream);
/* ---- ViT / DeiT training step (test_phase/models/deit.py:61-78 Block, :139-218 VisionTransformer in train mode; what loss.backward() does for
 * the DeiT encoders in meta_tuning_sun_m/train_meta.py:161-177).  Same contract as the Visformer trainer above: parameters stay in the caller's
 * fp32 device tensors (fsvit_param table with the reference's state-dict names: cls_token, pos_embed, patch_embed.proj.*, blocks.N.{norm1,norm2}.*,
 * blocks.N.attn.{qkv,proj}.*, blocks.N.mlp.{fc1,fc2}.*, norm.*), train_forward saves the activations in ws_dev, train_backward overwrites every
 * params[i].grad.  DropPath: 2 calls per block whose rate linspace(0, drop_path_rate, depth)[i] is non-zero, masks_dev [calls][n_img] of 0 / 1 in
 * forward order (fsvit_vit_trainer_droppath_calls); Dropout rates are 0 in every shipped factory and are not built.  dtype FSVIT_F32 or FSVIT_BF16
 * (both cover the 197-token factories; fp32 runs plain FMA loops). */
typedef struct fsvit_vit_trainer fsvit_vit_trainer;
int fsvit_vit_trainer_create(const fsvit_vit_cfg* cfg, int dtype, fsvit_vit_trainer** out);
void fsvit_vit_trainer_destroy(fsvit_vit_trainer* t);
int fsvit_vit_trainer_droppath_calls(const fsvit_vit_trainer* t, float drop_path_rate);
size_t fsvit_vit_trainer_workspace_bytes(fsvit_vit_trainer* t, const fsvit_param* params, int n_params, int n_img, float drop_path_rate);
int fsvit_vit_train_forward(fsvit_vit_trainer* t, const fsvit_param* params, int n_params, const float* x_nchw_dev, int n_img, int img_h, int img_w,
                            float drop_path_rate, const float* masks_dev, float* feat_dev, void* ws_dev, size_t ws_bytes, void* stream);
int fsvit_vit_train_backward(fsvit_vit_trainer* t, const fsvit_param* params, int n_params, const float* dfeat_dev, void* stream);

/* ---- Train-mode LV-ViT (meta_tuning_sun_m/models/lvvit.py:277-317 ConvBlock stem, :134-155 blocks, :415-552): the third trainer on the shared step
 * driver.  Parameters and BatchNorm running statistics under the reference's state-dict names (patch_embed.{conv1,bn1,conv2,bn2,conv3,bn3,
 * downsample.0,downsample.1,proj}.*, cls_token, pos_embed, blocks.N.*, norm.*; no qkv bias).  BatchNorm: batch statistics with the running update, or
 * frozen (set_freeze_bn, as fsvit_visformer_trainer_set_freeze_bn).  Every residual branch is scaled by 1 / skip_lam; the factor lives in the per-image
 * DropPath scales, never in the parameters.  DropPath: 2 calls per block whose rate linspace(0, drop_path_rate, depth)[i] is non-zero (get_dpr 'linear'),
 * masks_dev [calls][n_img] of 0 / 1 in forward order (fsvit_lvvit_trainer_droppath_calls).  img_size must be 80 (5 x 5 patch grid).
 * dtype FSVIT_F32 | FSVIT_BF16 | FSVIT_BF16X2. */
typedef struct fsvit_lvvit_trainer fsvit_lvvit_trainer;
int fsvit_lvvit_trainer_create(const fsvit_lvvit_cfg* cfg, int dtype, fsvit_lvvit_trainer** out);
void fsvit_lvvit_trainer_destroy(fsvit_lvvit_trainer* t);
int fsvit_lvvit_trainer_droppath_calls(const fsvit_lvvit_trainer* t, float drop_path_rate);
size_t fsvit_lvvit_trainer_workspace_bytes(fsvit_lvvit_trainer* t, const fsvit_param* params, int n_params, int n_img, float drop_path_rate);
int fsvit_lvvit_trainer_set_freeze_bn(fsvit_lvvit_trainer* t, int on);
int fsvit_lvvit_train_forward(fsvit_lvvit_trainer* t, const fsvit_param* params, int n_params, const float* x_nchw_dev, int n_img, int img_h, int img_w,
                              float drop_path_rate, const float* masks_dev, float* feat_dev, void* ws_dev, size_t ws_bytes, void* stream);
int fsvit_lvvit_train_backward(fsvit_lvvit_trainer* t, const fsvit_param* params, int n_params, const float* dfeat_dev, void* stream);
/* The token map of the pending train_forward (tokens_dev [n_img][25][embed_dim] fp32, the final norm on the patch rows) and its gradient for the
 * train_backward of that forward - the contract of the Visformer pair above.  train_tokens is valid between a train_forward and its train_backward
 * (FSVIT_ERR_ARG otherwise).  set_token_grad arms the next train_backward only, which then needs train_tokens to have run and accepts a NULL dfeat_dev
 * (no gradient on the cls feature); without it the backward is the cls-only one, bit for bit. */
int fsvit_lvvit_train_tokens(fsvit_lvvit_trainer* t, float* tokens_dev, void* stream);
int fsvit_lvvit_train_set_token_grad(fsvit_lvvit_trainer* t, const float* dtokens_dev);

/* Backward of fsvit_proto_head, method 'cos' (meta_baseline.py:33-47): dlogits [E,Q,way] -> dfeat_shot [E,way,shot,D],
 * dfeat_query [E,Q,D], dtemp_per_episode [E] (sum it for the learnable temperature, meta_baseline.py:20-21).  way, shot, Q, D >= 1 in every backward
 * entry below (FSVIT_ERR_ARG otherwise, nothing written). */
int fsvit_proto_head_backward(const float* feat_shot_dev, const float* feat_query_dev, const float* dlogits_dev, int E, int way,
                              int shot, int Q, int D, float temp, float* dfeat_shot_dev, float* dfeat_query_dev,
                              float* dtemp_per_episode_dev, void* stream);
/* The same for method 'sqr' (meta_baseline.py:38-41: logits = -temp * |q - mean_shot|^2). */
int fsvit_proto_head_backward_sqr(const float* feat_shot_dev, const float* feat_query_dev, const float* dlogits_dev, int E, int way,
                                  int shot, int Q, int D, float temp, float* dfeat_shot_dev, float* dfeat_query_dev,
                                  float* dtemp_per_episode_dev, void* stream);
/* Both backward forms with the temperature read from device memory (method FSVIT_HEAD_COS or FSVIT_HEAD_SQR). */
int fsvit_proto_head_backward_devtemp(const float* feat_shot_dev, const float* feat_query_dev, const float* dlogits_dev, int E, int way,
                                      int shot, int Q, int D, const float* temp_dev, int method, float* dfeat_shot_dev,
                                      float* dfeat_query_dev, float* dtemp_per_episode_dev, void* stream);
/* Head + loss of the meta-tuning step in one launch (train_meta.py:167-169: `logits = model(x_shot, x_query).view(-1, n_way); loss = F.cross_entropy(logits,
 * label); acc = utils.compute_acc(logits, label)`): logits [E,Q,way], per-episode accuracy / mean cross entropy [E], dlogits [E,Q,way] = d(mean CE over all
 * E * Q rows) / dlogits (may be NULL), and loss_acc_mean_dev[2] = {F.cross_entropy value, compute_acc value} (may be NULL).  labels_dev: int64 [E*Q] class
 * indices, or NULL for fs.make_nk_label's (few_shot.py:13-16: q / (Q / way)).  temp_dev (may be NULL): the temperature read from device memory instead of
 * `temp`.  ticket_dev: a zero-initialised 4-byte device word (required with loss_acc_mean_dev): the last workgroup to finish sums the episodes in index order
 * and leaves the word at zero - no second launch, no atomics on floating-point data, results bit-reproducible.
 * A label outside [0, way) - including F.cross_entropy's ignore_index, which this head does not implement - makes the episode's loss (and the batch mean) NaN. */
int fsvit_proto_head_ce(const float* feat_shot_dev, const float* feat_query_dev, const long long* labels_dev, int E, int way, int shot, int Q, int D, float temp,
                        const float* temp_dev, int method, float* logits_dev, float* dlogits_dev, float* acc_per_episode_dev, float* loss_per_episode_dev,
                        float* loss_acc_mean_dev, unsigned* ticket_dev, void* stream);
/* Its backward (methods FSVIT_HEAD_COS / FSVIT_HEAD_SQR): dlogits of fsvit_proto_head_ce times the upstream gradient *dloss_dev (NULL = 1) -> dfeat_shot,
 * dfeat_query, dtemp_dev [E] per episode (may be NULL) and, with ticket_dev, dtemp_dev[E] = their sum (dtemp_dev then holds E + 1 floats). */
int fsvit_proto_head_ce_backward(const float* feat_shot_dev, const float* feat_query_dev, const float* dlogits_dev, const float* dloss_dev, int E, int way,
                                 int shot, int Q, int D, float temp, const float* temp_dev, int method, float* dfeat_shot_dev, float* dfeat_query_dev,
                                 float* dtemp_dev, unsigned* ticket_dev, void* stream);
/* The same update for a table of tensors in one launch.  items_dev: DEVICE array of n_items records {float* param; const float* grad;
 * float* momentum_buf; size_t numel} (4 x 8 bytes each); max_numel = the largest numel.  All tensors share lr / momentum / weight_decay /
 * first_step (one param_group of torch.optim.SGD, meta_tuning_sun_m/utils/__init__.py:128-139). */
int fsvit_sgd_step_multi(const void* items_dev, int n_items, size_t max_numel, float lr, float momentum, float weight_decay, int first_step,
                         void* stream);

/* torch.optim.SGD(momentum, weight_decay) update of one fp32 tensor (utils/__init__.py:127-139) */
int fsvit_sgd_step(float* param_dev, const float* grad_dev, float* momentum_buf_dev, size_t n, float lr, float momentum,
                   float weight_decay, int first_step, void* stream);
/* torch.optim.SGD(momentum, weight_decay, nesterov=True, dampening=0) (meta_tuning_sun_d/train_meta.py:115): d = g + wd p; buf = d on the first
 * step, else momentum buf + d; p -= lr (d + momentum buf).  The multi form takes the table of fsvit_sgd_step_multi. */
int fsvit_sgd_nesterov_step_multi(const void* items_dev, int n_items, size_t max_numel, float lr, float momentum, float weight_decay,
                                  int first_step, void* stream);
int fsvit_sgd_nesterov_step(float* param_dev, const float* grad_dev, float* momentum_buf_dev, size_t n, float lr, float momentum,
                            float weight_decay, int first_step, void* stream);
/* detect_grad_nan (meta_tuning_sun_d/Models/utils.py:115-118) without a host round trip.  items_dev: DEVICE array of n_items records
 * {float* grad; size_t numel} (2 x 8 bytes each); max_numel = the largest numel; flags_dev: int32 [n_items].  In stream order: flags are
 * cleared; flags[i] = 1 for every tensor holding a NaN (g != g: +-Inf does not count); the flagged tensors are zeroed entirely.  The flags
 * stay on the device for the caller to sum. */
int fsvit_grad_nan_guard_multi(const void* items_dev, int n_items, size_t max_numel, int32_t* flags_dev, void* stream);
/* ---------------------------------------------------------------- device-resident dataset transform
 * Replaces, for a gathered batch of dataset indices, the per-image CPU pipeline of the reference's datasets
 * (test_phase/datasets/mini_imagenet.py:47-56: Resize((88,88)) -> CenterCrop(80) -> ToTensor -> Normalize;
 * tiered_imagenet.py:53-57: Resize(80) -> ToTensor -> Normalize): images_dev uint8 [N,H,W,3] resident in HBM,
 * index_dev int64 [B] -> out_dev fp32 [B,3,OH,OW].  The resize is Pillow's BILINEAR (two 8-bit passes, 22-bit fixed point),
 * bit-exact: the caller passes Pillow's coefficient tables (xmin / count / coef[ksize] per resized column and row, device
 * int32; few-shot-vit_amd/datasets/transforms.py computes them as Resample.c does).  crop_*0 = offset of the OHxOW crop in
 * the resized image; mean3 / std3 are HOST pointers to 3 floats. */
int fsvit_image_transform_gather(const uint8_t* images_dev, int H, int W, const int64_t* index_dev, int B, const int32_t* xmin_h_dev,
                                 const int32_t* cnt_h_dev, const int32_t* coef_h_dev, int ksize_h, const int32_t* xmin_v_dev,
                                 const int32_t* cnt_v_dev, const int32_t* coef_v_dev, int ksize_v, int crop_y0, int crop_x0, int OH, int OW,
                                 const float* mean3_host, const float* std3_host, float* out_dev, void* stream);
/* The train-time augmentation `augment: resize` of the supervised phase (sun_train_teacher/datasets/mini_imagenet.py:57-63,
 * tiered_imagenet.py:75-81) for a gathered batch: RandomResizedCrop(OH) -> RandomHorizontalFlip -> ToTensor -> Normalize.  The caller draws
 * the randomness: box_dev int32 [B][4] = top i, left j, height h, width w of each image's crop, flip_dev uint8 [B] (non-zero = mirror the
 * output columns; the flip acts on the resized image).  The crop is resized to OH x OW with Pillow's BILINEAR arithmetic, bit-exact with
 * Image.crop(box).resize(...): each workgroup computes its box's coefficient tables itself (fp64, the integers of
 * datasets/transforms.py:pil_bilinear_tables(w, OW) and (h, OH), taps clipped to the crop), so nothing but index, boxes and flips is uploaded
 * per batch.  A box is clamped to the image on the device; callers validate it.  mean3 / std3 are HOST pointers to 3 floats. */
int fsvit_image_transform_rrc_gather(const uint8_t* images_dev, int H, int W, const int64_t* index_dev, int B, const int32_t* box_dev,
                                     const uint8_t* flip_dev, int OH, int OW, const float* mean3_host, const float* std3_host,
                                     float* out_dev, void* stream);
/* The same crop + resize + flip left as bytes: out_dev uint8 [B,OH,OW,3], filter 0 = Pillow BILINEAR (the bytes fsvit_image_transform_rrc_gather
 * normalises), 1 = Pillow BICUBIC (a = -0.5, support 2; negative taps, so the clip to 0..255 is live).  With filter 1 this is the weak view of the
 * distillation phase before ToTensor (sun_meta_training/datasets/mini_imagenet.py:100-102: RandomResizedCropAndInterpolation(80, 'bicubic') ->
 * RandomHorizontalFlip; its RandomApply([RandAugment], p = 0.2) is fsvit_image_rand_augment below, on these bytes in place). */
int fsvit_image_transform_rrc_u8(const uint8_t* images_dev, int H, int W, const int64_t* index_dev, int B, const int32_t* box_dev,
                                 const uint8_t* flip_dev, int OH, int OW, int filter, uint8_t* out_dev, void* stream);
/* The strong / weak pair of the distillation phase (mini_imagenet.py:110-124, :194-204) from uint8 weak views views_dev [B,80,80,3] (16-byte
 * aligned; H = W = 80 or argument error): weak_dev [B,3,80,80] = Normalize(ToTensor(view)); strong_dev [B,3,80,80] = the same of the view after,
 * when the row's strong flag is set, ColorJitter (brightness / contrast / saturation in the row's order) -> GaussianBlur -> Solarization ->
 * RandomGrayscale, bit-exact with Pillow; then RandomErasing('pixel'): inside the row's erase box every value is an N(0, 1) draw of a counter-based
 * generator keyed by (seed, image slot, channel, pixel).  table_dev int32 [B, cols = 17], one row per image, the caller draws it:
 *   0 strong flag | 1-3 operation order (0 brightness, 1 contrast, 2 saturation) | 4-6 their factors as float32 bits | 7 blur flag, 8 box radius r,
 *   9 ww, 10 fw (Pillow's 24-bit box weights; datasets/transforms.py:gaussian_blur_box) | 11 solarize | 12 grayscale | 13-16 erase top, left,
 *   height, width (height 0 = none).  Callers validate the rows; the kernel reads nothing outside its image whatever they hold. */
int fsvit_image_strong_weak(const uint8_t* views_dev, int B, int H, int W, const int32_t* table_dev, int cols, const float* mean3_host,
                            const float* std3_host, uint64_t seed, float* weak_dev, float* strong_dev, void* stream);
/* RandAugment (timm 'rand-m9-mstd0.5-inc1') in place on uint8 views views_dev [B,80,80,3] (16-byte aligned; H = W = 80 or argument error), between
 * fsvit_image_transform_rrc_u8 and fsvit_image_strong_weak: the weak view's RandomApply([RandAugment], p = 0.2) of the distillation phase
 * (sun_meta_training/datasets/mini_imagenet.py:91-108) and the RandAugment stage of the classifier phase's timm pipeline.  slots_dev int32
 * [n_slots], strictly increasing image indices in [0, B): only these images are read and written, one workgroup each (n_slots <= B; n_slots = 0
 * returns 0 without a launch).  table_dev int32 [n_slots, cols = 28]: two operation slots of 14 columns, applied in order -
 *   0 code | 1 argument | 2-13 six float64 coefficients a0..a5 (low word first)
 * with the codes 0 none, 1 affine (Image.transform(AFFINE, a, BICUBIC, fillcolor = fill3_host): shear, translate, rotate), 2 invert,
 * 3 posterize (argument = bits kept, 0..8), 4 solarize (threshold 0..256), 5 solarize-add (addend 0..255, below 128), 6 autocontrast,
 * 7 equalize, 8 color, 9 contrast, 10 brightness, 11 sharpness (ImageEnhance; argument = the factor as float32 bits).  Bit-exact with Pillow.
 * The caller draws and validates the rows (datasets/transforms.py: rand_augment_table); the kernel touches nothing outside the batch whatever
 * they hold. */
int fsvit_image_rand_augment(uint8_t* views_dev, int B, int H, int W, const int32_t* slots_dev, int n_slots, const int32_t* table_dev, int cols,
                             const uint8_t* fill3_host, void* stream);

/* Operator level of the training path: attention backward (qkv, dctx -> dqkv; hd real / hdp padded head dim). */
/* Weight gradient of a 3x3 / stride 1 / pad 1 convolution straight from the NHWC activations (no im2col, no transposed copies):
 * dw[O][Ig][3][3] (fp32, overwritten) = sum_m dz[m][o] * x[pix(m) + tap][i].  x [B,H,W,groups*Ig], dz [B*H*W][O], dtype FSVIT_BF16 / FSVIT_F16, or
 * FSVIT_BF16X2 / FSVIT_F16X2 = fp32 activations split into two 16-bit limbs on the way into LDS (the two-limb trainers' kernel).
 * Replaces what autograd computes for stem.conv2 / conv3 and stage1.*.mlp.conv2 in train_meta.py:228-232 (visformer.py:152-163, :209-237).
 * Built shapes: groups = 8 with 32 -> 32 channels per group (W <= 20); dense O = 128, Ig = 64 / 128 (W <= 40). */
int fsvit_conv3x3_wgrad(const void* x_dev, const void* dz_dev, float* dw_dev, int B, int H, int W, int O, int Ig, int groups, int dtype, void* stream);

/* The grouped 3x3 / stride 1 / pad 1 convolution of the stage-1 Mlp (visformer.py:148: conv2, 8 groups of 32 -> 32 channels) as the training step
 * runs it, forward and - on the transposed, tap-flipped pack - as its data gradient: one wave per group, weights resident in registers.
 * x, y [B,H,W,256] NHWC; w_packed [256][Kw], row o = output channel, columns (ky, kx, c) of its group, Kw >= 288; dtype FSVIT_BF16 / FSVIT_F16; W <= 20. */
int fsvit_gconv3x3(const void* x_dev, const void* w_packed_dev, int Kw, void* y_dev, int B, int H, int W, int dtype, void* stream);

/* Weight gradient of a 1x1 convolution / Linear from the row-major activations: dw[N][C] (fp32, overwritten) = sum_m dz[m][n] * x[m][c].
 * x [M][C], dz [M][N], dtype FSVIT_BF16 / FSVIT_F16 (16-bit rows) or FSVIT_BF16X2 / FSVIT_F16X2 (fp32 rows, split into two 16-bit limbs on the way into
 * LDS: the two-limb trainers' kernel); N and C multiples of 8.  (conv1 / conv3 of the Mlps, qkv, proj in train_meta.py:228-232.) */
int fsvit_conv1x1_wgrad(const void* x_dev, const void* dz_dev, float* dw_dev, int M, int N, int C, int dtype, void* stream);

/* Backward of fsvit_attention: qkv [B*S][3*heads*hdp] (the forward's input) and dctx [B*S][heads*hdp] -> dqkv [B*S][3*heads*hdp] = (dQ | dK | dV):
 * P = softmax(scale q k^T), dV = P^T dO, dP = dO V^T, dS = scale P o (dP - rowsum(dP o P)), dQ = dS K, dK = dS^T Q.  hd = the real head dim, hdp its
 * padded size.  dtype: FSVIT_F32 or FSVIT_BF16 only (the training kernels' two storage types; the two-limb trainers call it with FSVIT_F32).
 * PAD CONTRACT: the pad channels hd .. hdp-1 of every head of qkv AND of dctx must be ZERO - the bf16 MFMA kernels take no hd and contract over all hdp
 * channels; the fp32 kernels mask by hd and ignore what the input pads hold.  The pad channels of dqkv are written as exact zeros by every kernel.
 * Refused with FSVIT_ERR_ARG and a message, nothing launched: any other dtype, a null pointer, B < 0, S < 1, heads < 1, hd < 1, hdp < hd, and a shape no
 * kernel covers (bf16: S > 224, or a head whose fp32 image 4 S (hd + 1) + 2 S (S + 1) floats is past 160 KB where hdp / 16 has no MFMA kernel at that S -
 * 2, 4, 6, 8 for S <= 32; 2, 4, 6 for S <= 128; 2, 4 for S <= 224; fp32: 2 (S + 16) (hd + 1) + 32 (S + 1) floats past 160 KB).  B == 0 returns 0. */
int fsvit_attention_backward(const void* qkv_dev, const void* dctx_dev, void* dqkv_dev, int B, int S, int heads, int hd, int hdp,
                             float scale, int dtype, void* stream);
/* The kernel fsvit_attention_backward takes, host only, nothing launched: family * 100000 + dtype * 10000 + KT * 100 + DT with family 1 =
 * attention_bwd_mfma_kernel<KT, DT> (bf16), 2 = attention_bwd_f32mfma_kernel<KT, DT>, 3 = attention_bwd_f32mfma_long_kernel<13, 4>, 4 = attention_bwd_kernel
 * (FMA loops, the head in LDS), 5 = attention_bwd_tiled_f32_kernel (4 and 5: KT = DT = 0); -1 = refused.  The launcher decides by this very function. */
int fsvit_op_attention_bwd_route(int S, int hd, int hdp, int dtype);

/* ================================================================ operator entry points (tests, tools)
 * The memory-bound kernels of the training step (train_kernels.hip), one entry per engine-level operation, so that each can be held against a
 * plain reference on its own (tests/test_gpu_train_ops.py, tests/test_gpu_train_conv_ops.py).  No engine path calls them.  dtype = storage type of the maps: FSVIT_F32 or FSVIT_BF16
 * (the training kernels are built for these two; anything else is FSVIT_ERR_ARG).  Statistics, parameters and parameter gradients are fp32.  A shape a
 * kernel does not cover is rejected with FSVIT_ERR_ARG and a message; nothing is launched on it.  Maps are row-major [M][C] / NHWC.
 *
 * Scratch sizes (floats): `partial` of the BatchNorm / colsum entries: fsvit_op_bn_reduce_blocks(M) * 2 * C; of ln_train_backward:
 * fsvit_op_ln_bwd_blocks(M) * 2 * D; of stem_tail_train_backward: fsvit_op_pool_bn_bwd_blocks(..) * 4 * C (0 blocks: that C has no fused form). */
int fsvit_op_bn_reduce_blocks(int M);
int fsvit_op_ln_bwd_blocks(int M);
int fsvit_op_pool_bn_bwd_blocks(int B, int OH, int OW, int C, int dtype);

/* Train-mode BatchNorm over the rows of z [M][C]: bn_reduce -> bn_fwd_finalize -> bn_apply.  stats [4][C] = mean | invstd | sa | sb (y = sa z + sb).
 * add_b != NULL: the residual add in front rides in the reduce pass - z := T(add_a + add_scale[row / rows_per_img] * add_b) is STORED and the
 * statistics are taken of the stored values (add_scale NULL: 1; with add_scale M must be images * rows_per_img).  running_mean / running_var (may both
 * be NULL) are updated with `momentum` and the unbiased variance.  frozen: the running statistics normalise, nothing is updated, the add runs on
 * its own.  y may be NULL (statistics only); res (may be NULL) is added before `act` (FSVIT_ACT_NONE | FSVIT_ACT_LRELU, slope 0.1).  M >= 2 unless frozen.
 * C: a multiple of 4; beyond 256 channel lanes (4 channels, bf16: 8 where C % 8 == 0) a multiple of 256 lanes. */
int fsvit_op_bn_train_forward(void* z_dev, int M, int C, int dtype, const float* gamma, const float* beta, float* running_mean, float* running_var, float eps,
                              float momentum, int frozen, const void* add_a, const void* add_b, const float* add_scale, int rows_per_img, const void* res,
                              int act, void* y_dev, float* stats, float* partial, void* stream);
/* Its backward: bn_reduce (backward form) -> bn_bwd_finalize -> bn_bwd_apply.  dz = ca dy + cb + cc xhat (+ acc; dz may be acc), coef [3][C] = ca | cb | cc.
 * act_sa / act_sb != NULL: dy is the gradient BEHIND a LeakyReLU(0.1) that followed this BatchNorm (y = act_sa z + act_sb), the slope is applied on the
 * fly.  out2 != NULL (may be dy): out2 = scale2[row / rows_per_img] * T(dz) (scale2 NULL: 1). */
int fsvit_op_bn_train_backward(const void* dy, const void* z, const float* mean, const float* invstd, const float* gamma, int M, int C, int dtype, int frozen,
                               const float* act_sa, const float* act_sb, const void* acc, const float* scale2, void* out2, int rows_per_img, void* dz,
                               float* dgamma, float* dbeta, float* coef, float* partial, void* stream);
/* g = dout * lrelu'(sa z + sb (+ res)) */
int fsvit_op_bn_act_bwd(const void* dout, const void* z, const float* sa, const float* sb, const void* res, void* g, int M, int C, int dtype, void* stream);

/* Stem tail (bn_pool_fwd): out [B,OH,OW,C] = MaxPool2d(2)(LeakyReLU(sa z + sb + r)) + pos, z / res [B,2OH,2OW,C]; r = res, or with rsa / rsb the
 * identity path's BatchNorm T(rsa res + rsb); arg = window position of the maximum (first of equals) | 4 if it is positive.  C % 8 == 0. */
int fsvit_op_stem_tail_train_forward(const void* z, const float* sa, const float* sb, const void* res, const float* rsa, const float* rsb, const float* pos,
                                     void* out, unsigned char* arg, int B, int OH, int OW, int C, int dtype, void* stream);
/* Both BatchNorm backwards behind that tail straight from the pooled gradient (pool_bn_bwd_reduce -> 2 x bn_bwd_finalize -> pool_bn_bwd_apply).
 * stats3 / statsd [2][C] = mean | invstd; coef [6][C] scratch.  Only where the channel lanes divide 256 (fsvit_op_pool_bn_bwd_blocks() != 0); other C:
 * FSVIT_ERR_ARG - the unfused chain pool_act_bwd + two bn_train_backward is the engine's path there. */
int fsvit_op_stem_tail_train_backward(const void* dout, const unsigned char* arg, const void* z3, const void* zd, const float* stats3, const float* statsd,
                                      const float* gamma3, const float* gammad, void* dz3, void* dzd, float* dgamma3, float* dbeta3, float* dgammad,
                                      float* dbetad, float* coef, float* partial, int B, int OH, int OW, int C, int dtype, int frozen, void* stream);
int fsvit_op_pool_act_bwd(const void* dout, const unsigned char* arg, void* g, int B, int OH, int OW, int C, int dtype, void* stream);
int fsvit_op_maxpool2_idx(const void* in, const float* pos, void* out, unsigned char* arg, int B, int OH, int OW, int C, int dtype, void* stream);
int fsvit_op_maxpool2_bwd(const void* dout, const unsigned char* arg, void* din, int B, int OH, int OW, int C, int dtype, void* stream);

/* LayerNorm with kept row statistics and its backward (dx = LN backward of dy (+ add; add may be dx); dgamma / dbeta may be NULL).  D % 4 == 0, D <= 2048. */
int fsvit_op_ln_train_forward(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int M, int D, float eps, int dtype,
                              void* stream);
int fsvit_op_ln_train_backward(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma, const void* add, void* dx,
                               float* partial, float* dgamma, float* dbeta, int M, int D, int dtype, void* stream);
/* tokens[b][0] = cls + pos[0], tokens[b][1 + i] = zpe[b (S - 1) + i] + pos[1 + i]; dzpe = the patch rows of dtok; the final norm on the cls row (fp32
 * feat) and its backward (dtok is zeroed, its cls rows written; partial B * 2 * D floats) */
int fsvit_op_vit_assemble(const void* zpe, const float* cls, const float* pos, void* tokens, int B, int S, int D, int dtype, void* stream);
int fsvit_op_vit_patch_rows(const void* dtok, void* dzpe, int B, int S, int D, int dtype, void* stream);
int fsvit_op_vit_cls_ln_forward(const void* tokens, const float* gamma, const float* beta, float* feat, float* mean, float* rstd, int B, int S, int D, float eps,
                                int dtype, void* stream);
int fsvit_op_vit_cls_ln_backward(const float* dfeat, const void* tokens, const float* mean, const float* rstd, const float* gamma, void* dtok, float* partial,
                                 float* dgamma, float* dbeta, int B, int S, int D, int dtype, void* stream);
/* The final norm on the patch rows (map [B][S - 1][D] fp32, mean / rstd [B * (S - 1)]) and the fused backward of both outputs: row 0 of dtok[b] from
 * dfeat[b] (statistics mean0 / rstd0 [B] of the cls forward), row 1 + i from dmap[b][i] (meanp / rstdp of the map forward); a NULL source gives zero rows
 * and adds nothing to dgamma / dbeta; every row of dtok is written.  S >= 2, D a multiple of 4 up to 2052; partial: the block count below * 2 * D floats. */
int fsvit_op_vit_map_ln_forward(const void* tokens, const float* gamma, const float* beta, float* map, float* mean, float* rstd, int B, int S, int D, float eps,
                                int dtype, void* stream);
int fsvit_op_vit_map_ln_bwd_blocks(int B, int S);
int fsvit_op_vit_map_ln_backward(const float* dfeat, const float* dmap, const void* tokens, const float* mean0, const float* rstd0, const float* meanp,
                                 const float* rstdp, const float* gamma, void* dtok, float* partial, float* dgamma, float* dbeta, int B, int S, int D, int dtype,
                                 void* stream);

/* Elementwise / small reductions.  gelu: dh NULL -> out = gelu(z), else out = dh * gelu'(z) (erf form); add_scaled: out = a + scale[i / per_img] * br
 * (a, scale may be NULL); avgpool_bwd: dx[b][hw][c] = dfeat[b][c] / HW; batch_sum: out[i] = sum_b g[b][i]; bcast_add: y[b][i] = x[b][i] + p[i];
 * colsum: out[c] = sum_m a[m][c]; unpatch2: g [B*OH*OW][4C] -> dx [B,2OH,2OW,C]; droppath_scales: scales[k][b] = masks[k][b] / keep_host[k];
 * fold_prenorm: wf[n][c] = T(W[n][c] sa[c]) ([N][Kw], zero padded), bf[n] = sum_c W[n][c] sb[c].  n, per_img: multiples of 4. */
int fsvit_op_gelu(const void* dh, const void* z, void* out, size_t n, int dtype, void* stream);
int fsvit_op_add_scaled(const void* a, const void* br, const float* scale, void* out, size_t n, size_t per_img, int dtype, void* stream);
int fsvit_op_avgpool_bwd(const float* dfeat, void* dx, int B, int HW, int C, int dtype, void* stream);
int fsvit_op_batch_sum(const void* g, float* out, int B, size_t per_img, int dtype, void* stream);
int fsvit_op_bcast_add(const void* x, const float* p, void* y, int B, size_t per_img, int dtype, void* stream);
int fsvit_op_colsum(const void* a, float* partial, float* out, int M, int C, int dtype, void* stream);
int fsvit_op_unpatch2(const void* g, void* dx, int B, int OH, int OW, int C, int dtype, void* stream);
int fsvit_op_droppath_scales(const float* masks, float* scales, int ncalls, int n_img, const float* keep_host, void* stream);
int fsvit_op_fill_f32(float* p, float v, size_t n, void* stream);                                   /* p[i] = v */
int fsvit_op_scale_copy(const float* in, float* out, size_t n, float scale, void* stream);          /* out[i] = in[i] * scale */
int fsvit_op_fold_prenorm(const float* W, const float* sa, const float* sb, void* wf, float* bf, int N, int C, int Kw, int dtype, void* stream);

/* ---- the MFMA side of the training step, one launcher per entry (tests/test_gpu_train_conv_ops.py)
 * Weight packs (launch_pack_weight_multi): PyTorch conv weight w [O][Ig][KH][KW] fp32 -> out [groups][rows_pad][Kw] in `dtype` = FSVIT_F32, FSVIT_BF16 or
 * FSVIT_BF16X2 (the two-limb words hi << 16 | lo, 4 bytes each).  mode 0: forward rows (row = output channel of the group, k = (ky, kx, i)); 1: the
 * transposed pack of the data gradient (row = input channel, k = (flipped tap, output channel)); 2: the non-overlapping patch conv's data gradient
 * (row = (ky, kx, i), k = output channel).  Modes >= 3 (fragment images) are refused.  hd / hdp: head-dim padding of the rows / columns (index j ->
 * (j / hd) * hdp + j % hd; hd == hdp: none; modes 0 / 1 only).  rows_pad and Kw must hold the padded rows / columns; everything else is zero.
 * fields [n][12] = O, Ig, KH, KW, groups, mode, rows_pad, Kw, hd_rows, hdp_rows, hd_cols, hdp_cols per job; any n >= 1 (the launcher walks its 40-job table). */
int fsvit_op_pack_weight(const float* w, void* out, int O, int Ig, int KH, int KW, int groups, int mode, int rows_pad, int Kw, int hd_rows, int hdp_rows,
                         int hd_cols, int hdp_cols, int dtype, void* stream);
int fsvit_op_pack_weight_multi(const float* const* w, void* const* out, const int* fields, int n, int dtype, void* stream);
/* launch_conv_gemm with the training epilogues (geometry arguments as fsvit_conv_gemm; dtype FSVIT_F32 | FSVIT_BF16): act FSVIT_ACT_GELU with y2 != NULL -
 * y = GELU(conv + bias), y2 = the GELU's derivative at the pre-activation; act FSVIT_ACT_MUL - y = (conv + bias) * mul (mul [M][y_cstride], required);
 * FSVIT_ACT_NONE / FSVIT_ACT_GELU without y2: the plain forms.  y2 without GELU and mul without FSVIT_ACT_MUL are refused.  *route (may be NULL) receives
 * the kernel that ran: 0 conv3x3_halo, 1 gemm256, 2 conv_gemm_v2. */
int fsvit_op_conv_train(const void* x, const void* w, const float* bias, const void* mul, void* y, void* y2, int B, int H, int W, int Cin, int x_cstride, int KH,
                        int KW, int stride, int pad, int N, int y_cstride, int Kw, int groups, int act, int dtype, int* route, void* stream);
/* launch_gconv3x3 (fsvit_gconv3x3's kernel, FSVIT_BF16) with y2 != NULL: y = GELU(conv), y2 = the derivative; or mul != NULL: y = conv * mul.  The kernel has
 * no form with both: refused. */
int fsvit_op_gconv3x3_train(const void* x, const void* w_packed, int Kw, void* y, void* y2, const void* mul, int B, int H, int W, int dtype, void* stream);
/* launch_stage1_ring_block_train: the training forward of a whole stage-1 block in one launch.  x, out, xn [B*H*W][128], h1 / g1 / h2 / g2 [B*H*W][256],
 * w1f [256][128] + b1f [256] (conv1 with the BatchNorm folded, fsvit_op_fold_prenorm), w2 [256][w2_ld] (w2_ld must be 320), w3 [128][256], sa / sb [128],
 * scale [B] or NULL.  out = x + scale[b] * conv3(h2), h1 = GELU(conv1(x)), g1 its derivative, h2 = GELU(conv2(h1)), g2, xn = sa x + sb.  FSVIT_BF16 only,
 * 1 <= W <= 20, H * W >= 16, no output may overlap an input or another output. */
int fsvit_op_stage1_block_train(const void* x, void* out, const void* w1f, const float* b1f, const void* w2, int w2_ld, const void* w3, void* h1, void* g1,
                                void* h2, void* g2, void* xn, const float* sa, const float* sb, const float* scale, int B, int H, int W, int dtype, void* stream);
/* launch_stage1_ring_dgrad: dz2 = (dz3 W3) * g2, dz1 = (grouped conv^T of dz2) * g1, dxn = dz1 W1 on the transposed packs w3t [256][128], w2t [256][w2_ld]
 * (tap-flipped, w2_ld must be 320), w1t [128][256].  The same checks. */
int fsvit_op_stage1_block_dgrad(const void* dz3, void* dxn, const void* w3t, const void* w2t, int w2_ld, const void* w1t, const void* g2, const void* g1,
                                void* dz2, void* dz1, int B, int H, int W, int dtype, void* stream);

/* ---------------------------------------------------------------- DeepEMD head (SUN-D: meta_tuning_sun_d/Models/models/Network.py:48-175, emd_utils.py:65-76)
 * fp32 in every numerics mode.  shot_tok [E][P][N][C] are the class prototypes' token maps (token-major), query_tok [E][Q][N][C] the queries'; N <= 32
 * nodes, C a multiple of 64.  Per (query, proto) pair the transportation problem  min sum c F,  c = 1 - cosine similarity of the channel-centred tokens,
 * F >= 0, row sums w1, column sums w2 (the reference's weights, both scaled to sum N)  is solved exactly (successive shortest paths, every loop bounded):
 * logits [E][Q][P] = temperature / N * sum (1 - c) F; flow_or_null [E][Q][P][N][N] (first index the query node) is what the backward needs;
 * status [E][Q][P] is 0, or 1 where a problem reached a loop bound (its logit is then not the optimum).  workspace: fsvit_emd_head_workspace_bytes
 * (0 for a refused shape).  Refused with FSVIT_ERR_ARG and a message, nothing launched: a null pointer, N < 1 or N > 32, C not a multiple of 64, negative
 * E / P / Q, a temperature that is not finite; FSVIT_ERR_WORKSPACE for a workspace that is too small.
 * Backward: the flows are constants (the reference's `solver: opencv`), dS = dlogit * temperature / N * F, the weights carry no gradient; d_shot_tok /
 * d_query_tok have the shapes of the token maps.  Deterministic (no atomics). */
size_t fsvit_emd_head_workspace_bytes(int E, int P, int Q, int N, int C);
int fsvit_emd_head_forward(const float* shot_tok_dev, const float* query_tok_dev, int E, int P, int Q, int N, int C, float temperature, float* logits_dev,
                           float* flow_or_null_dev, int* status_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int fsvit_emd_head_backward(const float* shot_tok_dev, const float* query_tok_dev, const float* dlogits_dev, const float* flow_dev, int E, int P, int Q,
                            int N, int C, float temperature, float* d_shot_tok_dev, float* d_query_tok_dev, void* workspace_dev, size_t workspace_bytes,
                            void* stream);
/* The head's forward over a token-map table (feature_table.TokenTable): every image is encoded and prepared once, the episodes address its rows.
 * fsvit_emd_table_prep fills rows of the table: tok [n_img][N][C] -> xhat [n_img][N][C] (the channel-centred, L2-normalised nodes) and pooled [n_img][C]
 * (the token mean of the un-centred map) - the values fsvit_emd_head_forward prepares for the same map, whatever launch it sits in.
 * fsvit_emd_head_gather: query (e, q) is the table row query_slots[e][q]; the class side is either the table row proto_slots[e][p] (1-shot) or the dense
 * map proto_tok[e][p] of [E][P][N][C] (the 5-shot SFC, prepared into the workspace by this call) - exactly one of the two is non-NULL.  Slots are int32, or
 * int64 with slots_are_int64 != 0.  logits / status [E][Q][P] are, for the same maps, the bits of fsvit_emd_head_forward.  A slot outside [0, n_slots) is
 * detected before any table read and never becomes an address: *invalid_dev (an int the caller zeroes once) is raised by one per such entry, and the
 * problems the entry takes part in get a NaN logit and status 0.  workspace: fsvit_emd_head_gather_workspace_bytes (0 for a refused shape), needed by the
 * dense-prototype form only (the slot form accepts NULL).  Refused with FSVIT_ERR_ARG and a message, nothing launched: a null pointer, both or neither
 * of proto_slots / proto_tok, n_slots < 1, the shape limits of fsvit_emd_head_forward (N 1 .. 32, C a positive multiple of 64, the problem counts), a
 * temperature that is not finite; FSVIT_ERR_WORKSPACE for a workspace that is too small.  E, P or Q == 0 is a no-op. */
int fsvit_emd_table_prep(const float* tok_dev, int n_img, int N, int C, float* xhat_dev, float* pooled_dev, void* stream);
size_t fsvit_emd_head_gather_workspace_bytes(int E, int P, int N, int C);
int fsvit_emd_head_gather(const float* tok_dev, const float* xhat_dev, const float* pooled_dev, int n_slots, const void* query_slots_dev,
                          const void* proto_slots_or_null_dev, int slots_are_int64, const float* proto_tok_or_null_dev, int E, int P, int Q, int N, int C,
                          float temperature, float* logits_dev, int* status_dev, int* invalid_dev, void* workspace_or_null_dev, size_t workspace_bytes,
                          void* stream);
/* The solver alone, for operator tests: cost [B][N][N], w1 / w2 [B][N] already normalised (equal sums) -> flow [B][N][N], status [B]; _counts also
 * writes the number of augmenting paths of every problem (n_augment [B]). */
int fsvit_op_emd_solve(const float* cost_dev, const float* w1_dev, const float* w2_dev, int B, int N, float* flow_dev, int* status_dev, void* stream);
int fsvit_op_emd_solve_counts(const float* cost_dev, const float* w1_dev, const float* w2_dev, int B, int N, float* flow_dev, int* status_dev,
                              int* n_augment_dev, void* stream);
/* The 5-shot structured-FC fine-tune (Network.py:83-107, get_sfc) kept on the device: one workgroup per episode runs n_steps consecutive mini-batch
 * updates of sfc [E][way][N][C] (in / out; the caller initialises it with the shot mean) against the support maps support [E][n][N][C] (n = way * shot
 * images, label [n] their classes).  ids [n_steps][E][bs] holds the support images of every mini-batch: an index in [0, n), or -1 for an empty slot
 * (a partial last batch); a slot outside [0, n) is skipped and never used as an address.  Per step: the head's forward of every (slot, class) pair
 * (the arithmetic of fsvit_emd_head_forward with the mini-batch as the queries), dlogits = (softmax - onehot(label)) / (slots in use), the head's
 * backward onto sfc with the flows as constants, then torch.optim.SGD's update: buf = grad on the first update of a fine-tune (`first` != 0 and
 * step 0 of this call), else buf = momentum * buf + (1 - dampening) * grad; sfc -= lr * buf.  buf [E][way][N][C] in / out.  sfc and buf persist
 * between calls, so a fine-tune may be cut into several calls (first = 0 from the second on) with identical results.  status_count [E] in / out:
 * the number of problems that reached a loop bound of the solver is ADDED.  No atomics, deterministic.  workspace:
 * fsvit_emd_sfc_workspace_bytes (0 for a refused shape).  Refused with FSVIT_ERR_ARG and a message, nothing launched: a null pointer, N < 1 or
 * N > 32, C not a positive multiple of 64, way / n / bs < 1, n_steps < 0, E < 0 or E > 65535, shapes whose workspace per episode exceeds 2^31 - 1
 * floats, a temperature / lr / momentum / dampening that is not finite; FSVIT_ERR_WORKSPACE for a workspace that is too small.  n_steps = 0 or E = 0
 * is a no-op. */
size_t fsvit_emd_sfc_workspace_bytes(int E, int way, int n, int bs, int N, int C);
int fsvit_emd_sfc_steps(const float* support_dev, const int* label_dev, const int* ids_dev, int n_steps, int first, int E, int way, int n, int bs, int N,
                        int C, float temperature, float lr, float momentum, float dampening, float* sfc_dev, float* buf_dev, int* status_count_dev,
                        void* workspace_dev, size_t workspace_bytes, void* stream);
/* The head over a labelled support set: a bank of class token maps, filled once (ragged classes, any number of calls) and queried many times, and the
 * exact re-rank of a shortlist of classes per query (models/emd_bank.TokenBank).  All tensors fp32 and dense.  Shared refusals (FSVIT_ERR_ARG and a
 * message, nothing launched): a NULL pointer that is not marked optional, n_classes < 1 or > 65536, N < 1 or N > 32, C not a positive multiple of 64 or above 16384.
 *
 * Accumulate: tok_dev [S][N][C], label_dev [S] (int64 when label_is_int64, else int32) -> sum_dev [n_classes][N][C] +=, count_dev [n_classes] +=,
 * *invalid_dev += the number of labels outside [0, n_classes), which contribute nothing else (their rows are not read).  The caller zeroes the three
 * outputs once.  A class's rows are added in ascending support index on top of the stored sum, without floating-point atomics: deterministic, and two
 * calls over a split give the bits of one call (the contract of fsvit_proto_bank_accumulate, whose rows end at D = 8192).  S == 0 is a no-op; S < 0 or
 * S > 2^24 refused. */
int fsvit_emd_bank_accumulate(const float* tok_dev, const void* label_dev, int label_is_int64, int S, int n_classes, int N, int C, float* sum_dev,
                              int* count_dev, int* invalid_dev, void* stream);
/* Finalize: tok_dev [n_classes][N][C] = sum / count (the class map: the mean of the class's support maps, what get_sfc starts from); xhat_dev
 * [n_classes][N][C] and pooled_dev [n_classes][C] = the bits fsvit_emd_table_prep gives for that tok; proto_dev [n_classes][C] = pooled / max(|pooled|,
 * 1e-12) (F.normalize), a row for a cosine shortlist (fsvit_proto_bank_topk); empty_dev [n_classes] = 1 where count == 0 - all outputs of such a class
 * are zero rows - else 0. */
int fsvit_emd_bank_finalize(const float* sum_dev, const int* count_dev, int n_classes, int N, int C, float* tok_dev, float* xhat_dev, float* pooled_dev,
                            float* proto_dev, int* empty_dev, void* stream);
/* Re-rank: query q (rows of query_tok / query_xhat [Q][N][C], query_pooled [Q][C] as fsvit_emd_table_prep writes them) is scored against the classes
 * cand_dev [Q][M] (int32 class numbers) of a finalized bank, only those M problems are solved, and the row is ranked in the same launch.  For the same
 * prepared rows a logit has the bits of fsvit_emd_head_gather.  A candidate: -1 is an empty slot; an entry < -1 or >= n_classes raises *invalid_dev by
 * one and is treated as -1 - it never becomes an address; an empty slot and a class flagged in bank_empty_dev score -inf and are not solved; duplicates
 * are allowed and each is scored.  Outputs: logits_or_null_dev [Q][M] in candidate order; classes_dev [Q][K] (int32), values_dev [Q][K], prob_dev [Q][K]:
 * the K first of the row in the order larger logit, then lower class, then lower candidate position, where an empty slot (it keeps class -1) comes
 * after every class, as the (-inf, -1) tail of fsvit_proto_bank_topk does; prob = the softmax over the finite entries of the row's M logits, 0 for a
 * -inf entry and for a row without a finite entry.  *status_count_dev (an int the caller zeroes once) is raised by one per problem that stopped at a
 * loop bound of the solver; *invalid_dev likewise per bad candidate (integer atomic adds).  Limits: 1 <= K <= M <= 32, 0 <= Q <= 2^24 (Q == 0 touches
 * nothing), a finite temperature; refusals as above. */
int fsvit_emd_rerank(const float* query_tok_dev, const float* query_xhat_dev, const float* query_pooled_dev, int Q, const float* bank_tok_dev,
                     const float* bank_xhat_dev, const float* bank_pooled_dev, const int* bank_empty_dev, int n_classes, const int* cand_dev, int M, int N,
                     int C, float temperature, int K, float* logits_or_null_dev, int* classes_dev, float* values_dev, float* prob_dev,
                     int* status_count_dev, int* invalid_dev, void* stream);

/* ---------------------------------------------------------------- episode sampler (host only, no GPU)
 * The draws of `CategoriesSampler.__iter__` (test_phase/datasets/samplers.py:19-35) replayed natively on the legacy numpy generator state: per episode
 * `np.random.choice(n_cat, n_cls, replace=False)`, then per chosen class `np.random.choice(catlocs[c], n_per, replace=False)`.  mt_key [624] / mt_pos =
 * the MT19937 state of `np.random.get_state()` (updated in place: hand it back with `np.random.set_state`); cat_items = the concatenated `catlocs`,
 * cat_offsets [n_cat + 1] their boundaries; out [n_batch][ep_per_batch][n_cls][n_per] dataset indices.  Bit-identical to numpy's stream. */
int fsvit_sampler_draw(unsigned int* mt_key, int* mt_pos, const long long* cat_offsets, const long long* cat_items, int n_cat, int n_batch, int ep_per_batch,
                       int n_cls, int n_per, long long* out_indices);

#ifdef __cplusplus
}
#endif
#endif /* FSVIT_H */
