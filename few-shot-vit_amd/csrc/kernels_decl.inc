// Launcher declarations of the fsvit gfx950 kernels; included by kernels.h once per kernel namespace (FSVIT_DECL_NS).
// dtype: 0 = f32, 1 = the namespace's 16-bit storage type (fsvit: __bf16, fsvit_f16: _Float16).
namespace FSVIT_DECL_NS {
using namespace fsvit_types;


int launch_im2col27(const float* x_nchw, void* out, int B, int H, int W, int OH, int OW, int dtype, hipStream_t s);
// im2col + stem conv1 + bn1 + LeakyReLU in one pass (bf16, 80x80 images, 64 channels): patches [B*1600][32], c1 [B*1600][64]; w = the packed conv1 layer [64][kw]
bool stem_conv1_supported(int dtype, int img, int C0);
int launch_stem_conv1(const float* x_nchw, void* patches, void* c1, const void* w, int kw, const float* bias, int B, hipStream_t s, int c1_planar = 0);
int launch_maxpool2_pos(const void* in, const float* pos, void* out, int B, int OH, int OW, int C, int dtype, hipStream_t s);

// qkv [B*S][3*heads*hdp] (channel = x*heads*hdp + y*hdp + z) -> ctx [B*S][heads*hdp]
int launch_attention(const void* qkv, void* ctx, int B, int S, int heads, int hdp, float scale, int dtype, hipStream_t s);
int attention_route(int S, int hdp, int dtype);      // the kernel launch_attention takes (attention.hip), -1 = refused; host only
size_t attention_lds_bytes(int S, int hdp, int dtype);
int attention_padded_head_dim(int hd, int S, int dtype);      // what the weight packer pads a head to

// x [B][HW][C] -> feat [B][C] fp32 = scale[c] * mean_hw(x) + shift[c]  (feat_out.hip)
int launch_pool_affine(const void* x, const float* scale, const float* shift, float* feat, int B, int HW, int C, int dtype, hipStream_t s);

// fused stage-1 block; x and y must be different buffers.  stage1_ring.hip: wave = channel group and register-resident weights, on the packed layers themselves (w1 [256][128], w2 [256][320], w3 [128][256])
bool stage1_ring_supported(int dtype, int C1, int hid, int group, int H1);
int launch_stage1_ring(const void* x, void* y, const void* w1, const float* b1, const void* w2, const void* w3, int B, int H, int W, hipStream_t s, const void* w3s = nullptr);
int launch_stage1_ring16(const void* x, void* y, const void* w1, const float* b1, const void* w2, const void* w3, int B, int H, int W, hipStream_t s);
// stage1_w4.hip: the block at one wave per SIMD with 32x32x16 MFMAs and hand-slotted GELUs (same arguments as launch_stage1_ring)
int launch_stage1_w4(const void* x, void* y, const void* w1, const float* b1, const void* w2, const void* w3, int B, int H, int W, hipStream_t s, const void* w3s = nullptr);
int launch_stage1_w4_prescale(const void* w, void* ws, int n, hipStream_t s);
int launch_stage1_ring_block_train(const void* x, void* out, const void* w1f, const float* b1f, const void* w2, const void* w3, void* h1, void* g1, void* h2, void* g2,
                                   void* xn, const float* sa, const float* sb, const float* scale, float* stats, int B, int H, int W, hipStream_t s);
int launch_stage1_ring_dgrad(const void* dz3, void* dxn, const void* w3t, const void* w2t, const void* w1t, const void* g2, const void* g1, void* dz2, void* dz1,
                             int B, int H, int W, hipStream_t s);

// fused row-wise Mlp of the attention blocks (mlp_rows.hip; bf16, C = 256, hidden = 1024): y = x + W2 GELU(W1 x + b1) (+ b2), in place allowed.
// wimg / b1img are built once by launch_mlp_pack from the standard packed layers (w1 [hid][k1w], w2 [C][k2w]).
bool mlp_rows_supported(int dtype, int C, int hid);
bool mlp_rows_proj_supported(int C, int hid, int KC);        // the attention block's proj conv + residual as a prologue on the same rows
size_t mlp_rows_image_bytes(int C, int hid, int KC);
int launch_mlp_pack(const void* w1, int k1w, const float* b1, const void* w2, int k2w, const void* wp, int kpw, int KC, void* wimg, float* b1img, int C,
                    int hid, hipStream_t s);
int launch_mlp_rows(const void* x, void* y, const void* wimg, const float* b1img, const float* b2, const void* ctx, int KC, int M, int C, int hid,
                    hipStream_t s);
// the ViT / DeiT block tail (deit.py:69-72; C = 384, hidden = 1536, KC = 384): y = x1 + b2 + W2 GELU(W1' LN(x1) + b1'), x1 = x + bp + Wp ctx, with the
// LayerNorm's gamma / beta folded into W1' / b1' (image from launch_mlp_pack with the proj weights).
bool mlp_rows_ln_supported(int dtype, int C, int hid, int KC);
int launch_mlp_rows_ln(const void* x, void* y, const void* wimg, const float* b1img, const float* bproj, const float* b2, const void* ctx, int KC, int M,
                       int C, int hid, float eps, hipStream_t s);

// LayerNorm + Linear on token rows (mlp_rows.hip; bf16, C = 384): y [M][N] = bias + W' LN(x), the DeiT block's norm1 + qkv (deit.py:40-47,:69)
bool ln_gemm_rows_supported(int dtype, int C, int N);
size_t ln_gemm_rows_image_bytes(int C, int N);
int launch_ln_gemm_pack(const void* w, int kw, void* wimg, int C, int N, hipStream_t s);
int launch_ln_gemm_rows(const void* x, void* y, const void* wimg, const float* bias, int M, int C, int N, float eps, hipStream_t s);
// the same kernel without the LayerNorm at C = 512: y = bias + W x (the Visformer stage-3 qkv conv, visformer.py:175; image from launch_ln_gemm_pack)
bool gemm_rows_supported(int dtype, int C, int N);
int launch_gemm_rows(const void* x, void* y, const void* wimg, const float* bias, int M, int C, int N, hipStream_t s);

// 2 x 2 / stride-2 patch-embedding conv + pos_embed on the rows kernel (visformer.py:266-288; 4 Ci = 512: patch_embed2; image from launch_ln_gemm_pack)
bool patch_embed_rows_supported(int dtype, int Ci, int H, int N);
int launch_patch_embed_rows(const void* x, void* y, const void* wimg, const float* bias, const float* pos, int B, int H, int Ci, int N, hipStream_t s);

// qkv conv + attention core for maps of at most 32 tokens on the rows kernel (mlp_rows.hip; bf16, C = 512, head dim padded to 96: Visformer stage 3)
bool qkv_attn_rows_supported(int dtype, int C, int heads, int hdp, int S);
int launch_qkv_attn_rows_pack(const void* w, int kw, void* wimg, int C, int heads, int hdp, hipStream_t s);
int launch_qkv_attn_rows(const void* x, void* ctx, const void* wimg, const float* bias, int B, int S, int C, int heads, int hdp, float scale, hipStream_t s);
// norm1 + qkv Linear + attention core of a ViT / DeiT block in one launch (deit.py:40-58,:69; C = 384, head dim 64, <= 256 tokens; image from launch_qkv_attn_rows_pack)
bool vit_attn_rows_supported(int dtype, int C, int heads, int hdp, int S);
int launch_vit_attn_rows(const void* x, void* ctx, const void* wimg, const float* bias, int B, int S, int C, int heads, int hdp, float eps, float scale, hipStream_t s);

// fused qkv conv + attention core of the Visformer stage-2 block (qkv_attn.hip; bf16, C = 256, 6 heads x 48, S <= 112): ctx rows
// [B*S][heads*hdp] from x rows [B*S][C]; wimg is built once by launch_qkv_attn_pack from the packed qkv layer (w [3*heads*hdp][kw])
bool qkv_attn_supported(int dtype, int C, int heads, int hdp, int S);
size_t qkv_attn_image_bytes();
int launch_qkv_attn_pack(const void* w, int kw, void* img, hipStream_t s);
int launch_qkv_attn(const void* x, void* ctx, const void* wimg, const float* bias, int B, int S, float scale, hipStream_t s);

// token map plumbing (feat_out.hip): out[i] = in[i] (* scale[c] + shift[c] when scale != NULL) in fp32; inout += add
int launch_tokens_to_f32(const void* in, const float* scale, const float* shift, float* out, size_t n, int C, int dtype, hipStream_t s);
int launch_add_f32_into(void* inout, const float* add, size_t n, int dtype, hipStream_t s);

// ViT / DeiT helpers (vit.hip)
int launch_patchify(const float* x_nchw, void* out, int B, int img, int p, int Kp, int dtype, hipStream_t s);
int launch_cls_pos(const float* cls_plus_pos0, void* tokens, int B, int S, int D, int dtype, hipStream_t s);
int launch_layernorm(const void* x, void* y, int M, int D, float eps, int dtype, hipStream_t s);
int launch_final_ln_cls(const void* tokens, const float* gamma, const float* beta, float* feat, int B, int S, int D, float eps, int dtype, hipStream_t s);
int launch_final_ln_map(const void* tokens, const float* gamma, const float* beta, float* feat, float* map, int B, int S, int D, float eps, int dtype, hipStream_t s);

// direct 3x3 / s1 / p1 weight gradient from NHWC activations (wgrad3x3.hip; dtype 1 = 16-bit storage, 2 = fp32 storage with two-limb arithmetic): dw [O][Ig][3][3] fp32 overwritten
bool wgrad3x3_supported(int dtype, int O, int Ig, int groups, int W);
size_t wgrad3x3_scratch_bytes(int O, int Ig, int groups, int M, int dtype = 1);
// 1x1: Y[n][split * Kc_pad + c] split-K partials for wgrad_finalize_multi_kernel (splits = wgrad1x1_splits)
bool wgrad1x1_supported(int dtype, int N, int C);
int wgrad1x1_splits(int N, int C, int M, int dtype = 1);
int launch_wgrad1x1(const void* x, int xld, int C, const void* dz, int zld, int N, float* y, int M, int Kc_pad, hipStream_t s, int dtype = 1);   // dtype 2: fp32 rows, two-limb arithmetic
// the grouped 3x3 conv itself (8 groups of 32 -> 32, 16-bit storage); w_packed = [256][Kw] rows (ky, kx, c) as launch_pack_weight_multi writes them
bool gconv3x3_supported(int dtype, int O, int Ig, int groups, int KH, int KW, int stride, int pad, int W);
int launch_gconv3x3(const void* x, const void* w_packed, int Kw, void* y, int B, int H, int W, hipStream_t s, void* y2 = nullptr, const void* mul = nullptr);
int launch_wgrad3x3(const void* x, int xld, const void* dz, int zld, float* dw, float* scratch, int B, int H, int W, int O, int Ig, int groups, hipStream_t s,
                    int* defer = nullptr, int dtype = 1);      // dtype 2: fp32 activations, two-limb arithmetic

}  // namespace FSVIT_DECL_NS
