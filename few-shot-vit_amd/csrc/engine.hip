// fsvit eval engines and the C boundary declared in include/fsvit.h.  In file order:
//  - state-dict packing: eval BatchNorm folding, K-major weight layout, head-dim padding, the weight-rounding bias correction;
//  - EvalStem: the ConvBlock stem that Visformer and LV-ViT share - one packer, one scratch layout, one slice loop over its four routes;
//  - the Visformer eval forward: a fixed chain of kernel launches on one HIP stream, its workspace laid out by an Arena that runs dry for
//    fsvit_*_workspace_bytes and for real inside a chunk;
//  - the handle plumbing of every encoder (create / workspace_bytes / chunked forward), the operator entry points, the profiler;
//  - the ViT / DeiT and LV-ViT encoders on the same plumbing.
#include "../../include/fsvit.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <utility>
#include <cstdint>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "host_common.h"
#include "kernels.h"
#include "train_kernels.h"

using namespace fsvit;

// ------------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
int fsvit_set_error(int code, const char* fmt, ...) {      // host_common.h: every error of engine.hip and train_engine.hip ends here
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

extern "C" const char* fsvit_last_error(void) { return g_err; }
extern "C" const char* fsvit_version(void) { return "fsvit 0.1.0 gfx950"; }

// ------------------------------------------------------------------------------------ helpers
static inline uint16_t f32_to_bf16(float f) {   // round to nearest even
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static inline uint16_t f32_to_f16(float f) {    // IEEE binary16, round to nearest even, gradual underflow, overflow -> inf
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
  const uint32_t a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);                    // NaN
  if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                   // >= 65520 rounds to inf
  if (a < 0x33000001u) return sign;                                          // < 2^-25 (or exactly 2^-25: ties to even = 0)
  const int e = (int)(a >> 23) - 127;                                        // unbiased exponent
  uint32_t m = (a & 0x7fffffu) | 0x800000u;                                  // 24-bit significand
  int shift = e >= -14 ? 13 : 13 + (-14 - e);                                // bits dropped (subnormal halves drop more)
  const uint32_t half = 1u << (shift - 1), rest = m & ((1u << shift) - 1u);
  uint32_t q = m >> shift;
  if (rest > half || (rest == half && (q & 1u))) ++q;
  if (e >= -14) return (uint16_t)(sign | (uint16_t)(((uint32_t)(e + 15 - 1) << 10) + q));   // the hidden bit carries into the exponent
  return (uint16_t)(sign | (uint16_t)q);                                     // subnormal (q may carry into the smallest normal)
}
static inline float f16_to_f32(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
  float f;
  if (e == 0) { f = std::ldexp((float)m, -24); uint32_t u; memcpy(&u, &f, 4); u |= sign; memcpy(&f, &u, 4); return f; }
  const uint32_t u = sign | (e == 31 ? 0x7f800000u | (m << 13) : ((e + 112) << 23) | (m << 13));
  memcpy(&f, &u, 4);
  return f;
}
// One fp32 weight as the two-limb dword of the x2 GEMM (conv_gemm_v2.hip): upper half = hi = w rounded to the 16-bit type, lower half =
// lo = (w - hi) rounded to it.
static inline uint32_t x2_limbs(float w, bool f16) {
  uint16_t hi, lo;
  if (f16) { hi = f32_to_f16(w); lo = f32_to_f16(w - f16_to_f32(hi)); }
  else {
    hi = f32_to_bf16(w);
    uint32_t hu = (uint32_t)hi << 16; float hf; memcpy(&hf, &hu, 4);
    lo = f32_to_bf16(w - hf);
  }
  return ((uint32_t)hi << 16) | lo;
}

struct Layer {
  void* w = nullptr;      // [groups][N][Kw] storage dtype
  float* bias = nullptr;  // [groups*N] fp32 or null
  int N = 0, K = 0, Kw = 0, groups = 1;
};
struct Block1 {
  Layer c1, c2, c3;
  void* c3s = nullptr;      // 8 x the packed conv3 weights (stage1_w4.hip: the residual and the output then need no scaling)
};
struct BlockA {
  Layer qkv, proj, fc1, fc2;
  void* mlp_img = nullptr;     // mlp_rows.hip: fragment-major image of [proj |] fc1 + fc2 (null: the GEMM launches are used)
  float* mlp_b1 = nullptr;
  int mlp_kc = 0;              // > 0: the image starts with the proj fragments and mlp_rows also computes x += proj(ctx)
  void* qa_img = nullptr;      // qkv_attn.hip: fragment-major image of the qkv conv (null: qkv GEMM + attention launches)
  void* qr_img = nullptr;      // mlp_rows.hip gemm_rows: fragment-major image of the qkv conv (row-wise GEMM instead of the 256-tile one)
  void* qar_img = nullptr;     // mlp_rows.hip qkv_attn_rows: head-major image of the qkv conv (qkv + attention in one launch, maps of <= 32 tokens)
};

// images per slice of the dedicated stem (stem_forward): swept 1600 / 3200 / 6400 / 12 800 on one box - 29.14 / 29.06 / 29.24 / 29.26 ms per 12 800-image step;
// again with conv1 inside the conv2 kernel (medians of three interleaved rounds): 28.02 / 27.87 / 27.85 / 27.88 - 3200 and up within the run-to-run spread, 3200 stays
static constexpr int stem_slice_images() { return 3200; }

// The ConvBlock stem of Visformer (visformer.py:202-239) and LV-ViT (lvvit.py:277-318), packed by pack_stem and run by stem_forward:
// conv1 s2 -> conv2 -> conv3 + downsample identity (eval BatchNorm folded, LeakyReLU(0.1)) -> MaxPool2d(2) [+ pos].  Everything that
// decides which kernels run is fixed when the handle is created.
enum StemRoute {
  STEM_GENERAL,        // conv2 / conv3 wherever launch_conv_gemm routes them, NHWC maps: other image sizes, geometries and numerics modes
  STEM_HALO_NHWC,      // conv2 / conv3 on conv3x3_halo's 96-channel instantiation over the 128-padded images conv2h / conv3h (ConvGemmParams::w_cpad)
  STEM_PLANAR,         // stem_conv1 -> conv3x3_halo -> conv3x3_halo + tail, c1 / c2 row-chunk-planar (conv_gemm.h x_planar)
  STEM_PLANAR_C1F      // STEM_PLANAR with conv1 built inside the conv2 kernel (conv3x3_halo.hip, C1F): no stem_conv1 launch, c1 is never written
};
struct EvalStem {
  Layer conv1, conv2, conv3f;  // conv3f: conv3 + bn3 with the downsample conv + bn_d folded in as a tail K slice
  Layer conv2h, conv3h;        // STEM_HALO_NHWC only: the 128-channel weight images of conv2 / conv3f (biases shared with them)
  int C0 = 0, C1 = 0;          // channels of conv1's map, of conv2's / conv3's
  int H0 = 0, H1 = 0, img = 0; // side of the conv maps (img / 2), of the pooled map (img / 4), of the image
  const float* pos = nullptr;  // [H1 * H1][C1] added behind the pool, or null
  StemRoute route = STEM_GENERAL;
  bool conv1_direct = false;   // conv1 is stem_conv1 (im2col rows + conv1 + bn1 + LeakyReLU in one pass over the image), not im2col27 + a K = 32 GEMM
  int slice = 0;               // images per pass of the slice loop (stem_forward); 0: the whole chunk in one pass
};

struct Tap { void* dst; size_t bytes; };

// One timed launch: events bracket the kernel on the stream it was launched on.
struct ProfEntry { std::string layer; int kernel; double flops; hipEvent_t e0, e1; };

// State shared by every encoder handle (the C-ABI functions that take "any encoder" rely on it being
// the first base sub-object).
enum { KIND_VISFORMER = 1, KIND_VIT = 2, KIND_LVVIT = 3 };
struct EngineBase {
  int kind = 0;
  int dtype = 0, es = 4;
  int img_size = 0, out_dim = 0;       // input side; feature width (set by the build function)
  // what differs between the handle types behind the shared create / workspace_bytes / forward (encoder_create sets them): the workspace a chunk of
  // Bc images needs, the forward of one chunk, and the image-size message (printf format: got h, w, model h, w)
  size_t (*plan_bytes)(const EngineBase* h, size_t Bc) = nullptr;
  int (*chunk)(EngineBase* h, const float* x, int Bc, float* feat, unsigned char* ws, bool first, hipStream_t st) = nullptr;
  const char* size_fmt = nullptr;
  std::map<std::string, Tap> taps;
  std::vector<void*> allocs;
  bool profiling = false;
  std::vector<ProfEntry> prof;
  hipEvent_t prof_last = nullptr;      // end event of the previous launch = start of the next
};

struct fsvit_visformer : EngineBase {
  fsvit_visformer_cfg cfg;
  int C0 = 0, C1 = 0, C2 = 0, C3 = 0;
  int H0 = 0, H1 = 0, H2 = 0, H3 = 0;
  int hid1 = 0, hid2 = 0, hid3 = 0;
  int hd2 = 0, hdp2 = 0, hd3 = 0, hdp3 = 0;
  EvalStem stem;
  Layer pe2, pe3;
  void* pe_img[2] = {nullptr, nullptr};                // mlp_rows.hip: fragment-major image of patch_embed2 / 3 for the row-wise kernel (null: conv_gemm)
  float *pos2 = nullptr, *pos3 = nullptr;      // (pos_embed1 is the stem's)
  std::vector<Block1> s1;
  std::vector<BlockA> s2, s3;
  float *fscale = nullptr, *fshift = nullptr;
};

namespace {

struct SD {
  const fsvit_tensor* t;
  int n;
  const fsvit_tensor* find(const std::string& name) const {
    for (int i = 0; i < n; ++i)
      if (name == t[i].name) return &t[i];
    return nullptr;
  }
  // returns nullptr + sets error when missing / mis-shaped
  const float* get(const std::string& name, std::initializer_list<int64_t> shape) const {
    const fsvit_tensor* x = find(name);
    if (!x) { fail(FSVIT_ERR_KEY, "missing key in state_dict: %s", name.c_str()); return nullptr; }
    bool ok = x->ndim == (int)shape.size() && x->data != nullptr;
    int i = 0;
    for (int64_t s : shape) { if (ok && x->shape[i] != s) ok = false; ++i; }
    if (!ok) { fail(FSVIT_ERR_KEY, "size mismatch for %s", name.c_str()); return nullptr; }
    return x->data;
  }
};

struct Affine { std::vector<double> s, t; bool ok = false; };

Affine bn_affine(const SD& sd, const std::string& p, int C, double eps) {
  Affine a;
  const float* w = sd.get(p + ".weight", {C});
  const float* b = sd.get(p + ".bias", {C});
  const float* m = sd.get(p + ".running_mean", {C});
  const float* v = sd.get(p + ".running_var", {C});
  if (!w || !b || !m || !v) return a;
  a.s.resize(C); a.t.resize(C);
  for (int c = 0; c < C; ++c) {
    a.s[c] = (double)w[c] / std::sqrt((double)v[c] + eps);
    a.t[c] = (double)b[c] - (double)m[c] * a.s[c];
  }
  a.ok = true;
  return a;
}

int upload(EngineBase* h, const std::vector<float>& src, bool as_storage, void** out) {
  void* d = nullptr;
  if (as_storage && is_x2(h->dtype)) {          // GEMM weights of the two-limb modes: 4 bytes per value, (hi, lo) limbs
    std::vector<uint32_t> tmp(src.size());
    for (size_t i = 0; i < src.size(); ++i) tmp[i] = x2_limbs(src[i], h->dtype == FSVIT_F16X2);
    HIP_TRY(hipMalloc(&d, tmp.size() * 4));
    h->allocs.push_back(d);
    HIP_TRY(hipMemcpy(d, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice));
  } else if (as_storage && h->dtype != FSVIT_F32) {
    std::vector<uint16_t> tmp(src.size());
    for (size_t i = 0; i < src.size(); ++i) tmp[i] = h->dtype == FSVIT_F16 ? f32_to_f16(src[i]) : f32_to_bf16(src[i]);
    HIP_TRY(hipMalloc(&d, tmp.size() * 2));
    h->allocs.push_back(d);
    HIP_TRY(hipMemcpy(d, tmp.data(), tmp.size() * 2, hipMemcpyHostToDevice));
  } else {
    HIP_TRY(hipMalloc(&d, src.size() * 4));
    h->allocs.push_back(d);
    HIP_TRY(hipMemcpy(d, src.data(), src.size() * 4, hipMemcpyHostToDevice));
  }
  *out = d;
  return 0;
}

// A device buffer of `bytes` owned by the handle, filled by one pack launch `launch(buffer)` on the null stream (complete on return).
template <typename F>
int packed_image(EngineBase* h, size_t bytes, void** out, F&& launch) {
  void* img = nullptr;
  HIP_TRY(hipMalloc(&img, bytes));
  h->allocs.push_back(img);
  RC_TRY(launch(img));
  HIP_TRY(hipDeviceSynchronize());
  *out = img;
  return 0;
}

// ---- weight-rounding bias correction of the 16-bit modes (restated by oracle/visformer_emul.py operand_means / _corr)
// Rounding a folded weight W'[n][k] to the 16-bit type is the same perturbation dW for every token of every image, so its mean effect
// sum_k dW[n][k] E[a_k] survives the average pooling.  E[a_k] is in the checkpoint: the running mean of the BatchNorm that sees the operand
// (pre-norm 1x1 convs: exact), 0 for the normalised image, and elsewhere the mean of the activation of a Gaussian pre-activation whose
// moments follow from the preceding BatchNorm's (beta, gamma) under channel independence.  The correction is folded into the fp32 bias at
// pack time: no run-time cost.  Bias-free convs that feed the residual stream (conv3 / proj of a block) hand their correction on as a
// per-channel constant of the stream (`cst`), which is folded into the bias of every later consumer (W' cst) and into the pooled feature.
struct WRound {
  bool on = false, f16 = false;
  std::vector<double> cst;                       // deferred constant of the residual stream
  double rounded(double v) const {               // the value the 16-bit weight image holds for v
    const float f = (float)v;
    if (f16) return (double)f16_to_f32(f32_to_f16(f));
    uint32_t u = (uint32_t)f32_to_bf16(f) << 16;
    float r; memcpy(&r, &u, 4);
    return (double)r;
  }
};

// fraction of the output positions of a k x k conv (stride, zero padding pad) on an H x H map whose tap (ky, kx) lies inside the map
std::vector<double> tap_fraction(int H, int stride, int k, int pad) {
  const int Ho = (H + 2 * pad - k) / stride + 1;
  std::vector<double> f1(k), f((size_t)k * k);
  for (int t = 0; t < k; ++t) {
    int in = 0;
    for (int o = 0; o < Ho; ++o) { const int pos = o * stride - pad + t; in += (pos >= 0 && pos < H); }
    f1[t] = (double)in / Ho;
  }
  for (int y = 0; y < k; ++y) for (int x = 0; x < k; ++x) f[(size_t)y * k + x] = f1[y] * f1[x];
  return f;
}

inline double gelu_exact(double z) { return 0.5 * z * (1.0 + std::erf(z * 0.7071067811865476)); }

// E[GELU(y)] and Var[GELU(y)] for y ~ N(mu, sig^2): trapezoid rule on z in [-8, 8], 257 nodes
void gauss_moments_gelu(double mu, double sig, double* mean, double* var) {
  double sw = 0, s1 = 0, s2 = 0;
  for (int j = 0; j <= 256; ++j) {
    const double z = -8.0 + j / 16.0, w = std::exp(-0.5 * z * z), v = gelu_exact(mu + sig * z);
    sw += w; s1 += w * v; s2 += w * v * v;
  }
  *mean = s1 / sw;
  *var = std::max(0.0, s2 / sw - (s1 / sw) * (s1 / sw));
}

// E[LeakyReLU_0.1(N(mu, sig^2))] = mu (0.1 + 0.9 Phi(mu / sig)) + 0.9 sig phi(mu / sig)
double lrelu_mean(double mu, double sig) {
  if (sig <= 0) return mu > 0 ? mu : 0.1 * mu;
  const double t = mu / sig;
  return mu * (0.1 + 0.9 * 0.5 * (1.0 + std::erf(t * 0.7071067811865476))) + 0.9 * sig * std::exp(-0.5 * t * t) * 0.3989422804014327;
}

// Pack a conv weight W[O][Ig][KH][KW] (O = groups*N) into [groups][N][Kw], k = (ky*KW+kx)*Ig + c,
// with optional per-output-channel scale (BN after the conv) and per-input-channel scale (BN before
// a 1x1 conv).  `rowmap`/`colmap` (optional) scatter rows / K columns (head-dim padding).
// Weight-rounding correction (wr != null and on): `in_mean` [groups*Ig] = E[operand channel], `tapf` [KH*KW] = tap_fraction or null;
// the correction -sum_k dW f_tap E[a] and (`use_cst`) the stream constant's image sum_k W' cst go into the bias; a bias-free layer
// returns its correction in `corr_out` [O] instead.
int pack_layer(EngineBase* h, Layer* L, const float* W, int O, int Ig, int KH, int KW, int groups,
               const std::vector<double>* out_scale, const std::vector<double>* in_scale,
               const std::vector<double>& bias, bool has_bias,
               const std::vector<int>* rowmap, int Npad, const std::vector<int>* colmap, int Kpad,
               const WRound* wr = nullptr, const std::vector<double>* in_mean = nullptr, const double* tapf = nullptr,
               bool use_cst = false, std::vector<double>* corr_out = nullptr) {
  const int bke = 128 / h->es;
  const int N = (rowmap ? Npad : O) / groups;
  const int K = colmap ? Kpad : KH * KW * Ig;
  const int Kw = round_up(K, bke);
  // (an operand-mean / stream-constant vector that does not cover this layer's input channels - e.g. one handed on across a stage without blocks - is
  // not applied: no correction instead of another tensor's statistics)
  const bool fix = wr && wr->on && in_mean && in_mean->size() >= (size_t)groups * Ig;
  const bool cst = wr && wr->on && use_cst && wr->cst.size() >= (size_t)groups * Ig;
  if (corr_out) corr_out->assign(O, 0.0);
  std::vector<float> pk((size_t)groups * N * Kw, 0.0f);
  std::vector<float> pb((size_t)groups * N, 0.0f);
  for (int o = 0; o < O; ++o) {
    const int row = rowmap ? (*rowmap)[o] : o;
    const double so = out_scale ? (*out_scale)[o] : 1.0;
    const int g0 = (o / (O / groups)) * Ig;
    double corr = 0.0, wc = 0.0;
    for (int c = 0; c < Ig; ++c) {
      const double si = in_scale ? (*in_scale)[c] : 1.0;
      for (int ky = 0; ky < KH; ++ky)
        for (int kx = 0; kx < KW; ++kx) {
          int k = (ky * KW + kx) * Ig + c;
          if (colmap) k = (*colmap)[k];
          const double v = (double)W[(((size_t)o * Ig + c) * KH + ky) * KW + kx] * so * si;
          pk[(size_t)row * Kw + k] = (float)v;
          if (fix) corr -= (wr->rounded(v) - v) * (tapf ? tapf[ky * KW + kx] : 1.0) * (*in_mean)[g0 + c];
          if (cst) wc += v * wr->cst[g0 + c];
        }
    }
    if (has_bias) pb[row] = (float)(bias[o] + corr + wc);
    else if (corr_out) (*corr_out)[o] = corr;
  }
  L->N = N; L->K = K; L->Kw = Kw; L->groups = groups;
  RC_TRY(upload(h, pk, true, &L->w));
  if (has_bias) { void* b; RC_TRY(upload(h, pb, false, &b)); L->bias = (float*)b; }
  return 0;
}

// bias[n] = sum_c W[n][c] * t[c]  for a 1x1 conv that follows a BatchNorm
std::vector<double> prenorm_bias(const float* W, int O, int C, const std::vector<double>& t) {
  std::vector<double> b(O, 0.0);
  for (int o = 0; o < O; ++o) {
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += (double)W[(size_t)o * C + c] * t[c];
    b[o] = s;
  }
  return b;
}

// pos_embed [1,C,H,W] -> [H*W][C] fp32 (+ optional per-channel constant)
int pack_pos(EngineBase* h, const float* pos, int C, int HW, float** out) {
  std::vector<float> p((size_t)HW * C);
  for (int c = 0; c < C; ++c)
    for (int i = 0; i < HW; ++i) p[(size_t)i * C + c] = pos[(size_t)c * HW + i];
  void* d; RC_TRY(upload(h, p, false, &d));
  *out = (float*)d;
  return 0;
}

// A [C] state-dict entry as doubles (zeros when missing: the caller has checked the key through bn_affine).
std::vector<double> sd_vec(const SD& sd, const std::string& name, int C, bool absolute) {
  const float* p = sd.get(name, {C});
  std::vector<double> v(C, 0.0);
  for (int c = 0; p && c < C; ++c) v[c] = absolute ? std::fabs((double)p[c]) : (double)p[c];
  return v;
}

ConvGemmParams conv_params(const Layer& L, const void* x, void* y, int B, int H, int W, int Cin, int x_cstride,
                           int KH, int KW, int stride, int pad, int y_cstride, int act,
                           const void* res, int res_first, const float* pos) {
  ConvGemmParams p;
  p.x = x; p.w = L.w; p.bias = L.bias; p.res = res; p.pos = pos; p.y = y;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.x_cstride = x_cstride;
  p.OH = (H + 2 * pad - KH) / stride + 1; p.OW = (W + 2 * pad - KW) / stride + 1;
  p.KH = KH; p.KW = KW; p.stride = stride; p.pad = pad;
  p.N = L.N; p.y_cstride = y_cstride; p.K = L.K; p.Kw = L.Kw; p.M = B * p.OH * p.OW;
  p.groups = L.groups; p.act = act; p.res_first = res_first; p.log2Cin = ilog2(Cin);
  p.x2 = nullptr; p.x2_cstride = 0; p.K2 = 0; p.pool2 = 0; p.y_rpi = 0; p.y_row0 = 0;
  p.w_gstride = 0; p.w_rstride = 0; p.out_f32 = 0; p.y2 = nullptr; p.stats = nullptr;
  return p;
}

// conv2 and conv3 (+ downsample tail + LeakyReLU + MaxPool2d [+ pos]) of a stem for n images: c1 -> c2 -> out, the tail over the im2col rows `patches`
void stem_conv_params(const EvalStem& s, bool planar, const void* c1, void* c2, const void* patches, void* out, int n, ConvGemmParams* p2, ConvGemmParams* p3) {
  const bool halo = s.route == STEM_HALO_NHWC;
  *p2 = conv_params(halo ? s.conv2h : s.conv2, c1, c2, n, s.H0, s.H0, s.C0, s.C0, 3, 3, 1, 1, s.C1, ACT_LRELU, nullptr, 0, nullptr);
  *p3 = conv_params(halo ? s.conv3h : s.conv3f, c2, out, n, s.H0, s.H0, s.C1, s.C1, 3, 3, 1, 1, s.C1, ACT_LRELU, nullptr, 0, s.pos);
  p3->x2 = patches; p3->x2_cstride = 32; p3->K2 = 32; p3->pool2 = 1;
  // the two maps between the dedicated kernels are row-chunk-planar: the halo fetch of the consumer then reads row segments instead of 16 bytes of every 128-byte line
  p2->x_planar = p2->y_planar = p3->x_planar = planar ? 1 : 0;
  if (halo) p2->w_cpad = p3->w_cpad = 128;
}

// Packs <pfx>conv1 / conv2 / conv3 / downsample with their BatchNorms folded (conv -> BN as per-output-channel scale + shift) into `s` and fixes its
// route.  pos: the packed position table added behind the pool, or null.  wr: the weight-rounding correction (null: none - LV-ViT).
// direct_conv1: stem_conv1 may stand in for im2col27 + GEMM where it is built.  general_slice: EvalStem::slice of STEM_GENERAL (the other routes run in
// slices of stem_slice_images()).
int pack_stem(EngineBase* h, const SD& sd, const std::string& pfx, int C0, int C1, int img, double eps, const float* pos, const WRound* wr,
              bool direct_conv1, int general_slice, EvalStem* out) {
  EvalStem& s = *out;
  const int kdt = h->dtype;
  s.C0 = C0; s.C1 = C1; s.img = img; s.H0 = img / 2; s.H1 = img / 4; s.pos = pos;
  const float* w1 = sd.get(pfx + "conv1.weight", {C0, 3, 3, 3});
  const float* wd = sd.get(pfx + "downsample.0.weight", {C1, 3, 3, 3});
  const float* w2 = sd.get(pfx + "conv2.weight", {C1, C0, 3, 3});
  const float* w3 = sd.get(pfx + "conv3.weight", {C1, C1, 3, 3});
  Affine b1 = bn_affine(sd, pfx + "bn1", C0, eps), b2 = bn_affine(sd, pfx + "bn2", C1, eps);
  Affine b3 = bn_affine(sd, pfx + "bn3", C1, eps), bd = bn_affine(sd, pfx + "downsample.1", C1, eps);
  if (!w1 || !wd || !w2 || !w3 || !b1.ok || !b2.ok || !b3.ok || !bd.ok) return FSVIT_ERR_KEY;
  // conv1 (and the downsample taps inside conv3f) consume the 32-wide im2col rows: K columns 0..26 = (ky,kx,c), 27..31 = 0
  std::vector<int> cm(27);
  for (int k = 0; k < 27; ++k) cm[k] = k;
  // operand means: the normalised image 0 (no correction for conv1 / downsample); conv2 / conv3 read LeakyReLU(BN(z)), z_c ~ N(beta_c, gamma_c^2)
  const bool fix = wr && wr->on;
  std::vector<double> m2(C0), m3(C1);
  if (wr) {
    const std::vector<double> be1 = sd_vec(sd, pfx + "bn1.bias", C0, false), ga1 = sd_vec(sd, pfx + "bn1.weight", C0, true);
    const std::vector<double> be2 = sd_vec(sd, pfx + "bn2.bias", C1, false), ga2 = sd_vec(sd, pfx + "bn2.weight", C1, true);
    for (int c = 0; c < C0; ++c) m2[c] = lrelu_mean(be1[c], ga1[c]);
    for (int c = 0; c < C1; ++c) m3[c] = lrelu_mean(be2[c], ga2[c]);
  }
  const std::vector<double> tf0 = tap_fraction(s.H0, 1, 3, 1);
  RC_TRY(pack_layer(h, &s.conv1, w1, C0, 3, 3, 3, 1, &b1.s, nullptr, b1.t, true, nullptr, 0, &cm, 32));
  RC_TRY(pack_layer(h, &s.conv2, w2, C1, C0, 3, 3, 1, &b2.s, nullptr, b2.t, true, nullptr, 0, nullptr, 0, wr, &m2, tf0.data()));
  // Row image of a BN-scaled 3 x 3 conv: `rows` rows of Kw columns, k = tap * cstride + c (zeros elsewhere); tail: behind the Kmain main columns one
  // K slice of bn_d-scaled downsample taps over the im2col rows
  auto conv_image = [&](const float* w, int Cin, const std::vector<double>& scale, int cstride, int rows, int Kmain, int Kw, bool tail) {
    std::vector<float> pk((size_t)rows * Kw, 0.0f);
    for (int o = 0; o < C1; ++o) {
      for (int c = 0; c < Cin; ++c)
        for (int t9 = 0; t9 < 9; ++t9) pk[(size_t)o * Kw + t9 * cstride + c] = (float)((double)w[((size_t)o * Cin + c) * 9 + t9] * scale[o]);
      for (int c = 0; tail && c < 3; ++c)
        for (int t9 = 0; t9 < 9; ++t9) pk[(size_t)o * Kw + Kmain + t9 * 3 + c] = (float)((double)wd[((size_t)o * 3 + c) * 9 + t9] * bd.s[o]);
    }
    return pk;
  };
  {  // conv3f rows = [ bn3-scaled conv3 (K = 9*C1, padded to the K slice) | one tail slice: bn_d-scaled downsample taps ]
    const int bke = 128 / h->es, K = 9 * C1, Kmain = round_up(K, bke), Kw = Kmain + bke;
    std::vector<float> pb(C1);
    for (int o = 0; o < C1; ++o) {
      double bias = b3.t[o] + bd.t[o];
      if (wr) {
        double corr = 0.0;
        for (int c = 0; fix && c < C1; ++c)
          for (int t9 = 0; t9 < 9; ++t9) {
            const double v = (double)w3[((size_t)o * C1 + c) * 9 + t9] * b3.s[o];
            corr -= (wr->rounded(v) - v) * tf0[t9] * m3[c];
          }
        bias += corr;
      }
      pb[o] = (float)bias;
    }
    s.conv3f.N = C1; s.conv3f.K = K; s.conv3f.Kw = Kw; s.conv3f.groups = 1;
    RC_TRY(upload(h, conv_image(w3, C1, b3.s, C1, C1, Kmain, Kw, true), true, &s.conv3f.w));
    void* bdev; RC_TRY(upload(h, pb, false, &bdev)); s.conv3f.bias = (float*)bdev;
  }
  // ---- the route.  Two switches, each read once per build: FSVIT_LVVIT_STEM=gemm keeps the 96-channel convs on conv_gemm_v2 (the A/B switch of
  // tools/bench_lvvit.py); FSVIT_STEM_FUSE_C1=0 keeps stem_conv1 and the c1 map in HBM on the planar route (tests/test_gpu_stem_fused_c1.py)
  const char* stem_env = getenv("FSVIT_LVVIT_STEM");
  const char* fuse_env = getenv("FSVIT_STEM_FUSE_C1");
  s.route = STEM_GENERAL; s.slice = general_slice;
  s.conv1_direct = direct_conv1 && K(stem_conv1_supported)(kd(kdt), img, C0);
  if (kd(kdt) == 1 && C0 == 96 && C1 == 96 && !(stem_env && strcmp(stem_env, "gemm") == 0)) {
    // conv3x3_halo's images (ConvGemmParams::w_cpad = 128): 128 rows, k = tap * 128 + c, zeros past the 96 channels / rows; conv3's tail slice of
    // downsample taps behind the 9 * 128 main columns.  Same folded values as conv2 / conv3f (the bias tables are shared: 96 entries).
    s.route = STEM_HALO_NHWC; s.slice = stem_slice_images();
    for (int which = 0; which < 2; ++which) {
      Layer& L = which ? s.conv3h : s.conv2h;
      L.N = C1; L.K = 9 * C0; L.Kw = 9 * 128 + (which ? 64 : 0); L.groups = 1; L.bias = which ? s.conv3f.bias : s.conv2.bias;
      RC_TRY(upload(h, conv_image(which ? w3 : w2, C0, which ? b3.s : b2.s, 128, 128, 9 * 128, L.Kw, which == 1), true, &L.w));
    }
  } else if (s.conv1_direct) {
    // the whole stem on its dedicated kernels where both halo convs are built for the geometry (the probe stands in for the im2col rows of the tail)
    static const char probe = 0;
    ConvGemmParams p2, p3;
    stem_conv_params(s, false, nullptr, nullptr, &probe, nullptr, 1, &p2, &p3);
    if (K(conv_gemm_route)(p2, kg(kdt)) == 0 && K(conv_gemm_route)(p3, kg(kdt)) == 0) {
      s.route = STEM_PLANAR; s.slice = stem_slice_images();
      stem_conv_params(s, true, nullptr, nullptr, &probe, nullptr, 1, &p2, &p3);
      if (!(fuse_env && fuse_env[0] == '0') && K(conv3x3_halo_c1f_supported)(p2, kg(kdt)) && img == 80) s.route = STEM_PLANAR_C1F;
    }
  }
  return 0;
}

int build(fsvit_visformer* h, const SD& sd) {
  const int kdt = h->dtype;
  const fsvit_visformer_cfg& cf = h->cfg;
  const double eps = cf.bn_eps;
  const int epc = 16 / h->es;
  const int D = cf.embed_dim;
  h->C0 = cf.init_channels; h->C1 = D / 2; h->C2 = D; h->C3 = h->out_dim = D * 2;
  if (cf.img_size % 16 != 0) return fail(FSVIT_ERR_ARG, "img_size %d must be a multiple of 16", cf.img_size);
  h->H0 = cf.img_size / 2; h->H1 = cf.img_size / 4; h->H2 = cf.img_size / 8; h->H3 = cf.img_size / 16;
  if (cf.group < 2) return fail(FSVIT_ERR_ARG, "group < 2 ('net' setting, visformer.py:137-138) is not supported");
  h->hid1 = h->C1 * 2;
  h->hid2 = (int)(h->C2 * cf.mlp_ratio);
  h->hid3 = (int)(h->C3 * cf.mlp_ratio);
  h->hd2 = (int)std::lround((double)(h->C2 / cf.num_heads));  // round(dim // heads * 1.0), visformer.py:172
  h->hd3 = (int)std::lround((double)(h->C3 / cf.num_heads));
  h->hdp2 = K(attention_padded_head_dim)(h->hd2, h->H2 * h->H2, kd(kdt));
  h->hdp3 = K(attention_padded_head_dim)(h->hd3, h->H3 * h->H3, kd(kdt));
  const int Cg = h->hid1 / cf.group;
  if (h->C0 % epc || h->C1 % epc || h->hid1 % cf.group || Cg % epc)
    return fail(FSVIT_ERR_ARG, "channel counts must be multiples of %d for 16-byte K chunks", epc);
  if (!is_pow2(h->C0) || !is_pow2(h->C1) || !is_pow2(h->C2) || !is_pow2(Cg))
    return fail(FSVIT_ERR_ARG, "multi-tap conv input channels must be powers of two");
  if (h->H2 * h->H2 > 128) return fail(FSVIT_ERR_ARG, "attention supports at most 128 tokens (img_size <= 88)");

  std::vector<double> nob;
  WRound wr;                                    // weight-rounding bias correction: the 16-bit modes only (the two-limb modes carry 16+ bits)
  // FSVIT_WROUND=0 (read once per build): the plain 16-bit images without the correction - the ablation switch of the one eval route whose effect
  // rests on statistical assumptions (data that matches the running statistics); tests/test_gpu_unfused_paths.py
  const char* wr_env = getenv("FSVIT_WROUND");
  wr.on = (kdt == FSVIT_BF16 || kdt == FSVIT_F16) && !(wr_env && wr_env[0] == '0');
  wr.f16 = kdt == FSVIT_F16;
  if (wr.on) wr.cst.assign(h->C1, 0.0);
  auto vec = [&](const std::string& name, int C, bool absolute) { return sd_vec(sd, name, C, absolute); };
  {
    const float* p1 = sd.get("pos_embed1", {1, h->C1, h->H1, h->H1});
    const float* p2 = sd.get("pos_embed2", {1, h->C2, h->H2, h->H2});
    const float* p3 = sd.get("pos_embed3", {1, h->C3, h->H3, h->H3});
    if (!p1 || !p2 || !p3) return FSVIT_ERR_KEY;
    float* pos1;
    RC_TRY(pack_pos(h, p1, h->C1, h->H1 * h->H1, &pos1));
    RC_TRY(pack_pos(h, p2, h->C2, h->H2 * h->H2, &h->pos2));
    RC_TRY(pack_pos(h, p3, h->C3, h->H3 * h->H3, &h->pos3));
    // ---- stem (visformer.py:202-239): sliced on the dedicated routes only - the general route launches once per chunk
    RC_TRY(pack_stem(h, sd, "stem.", h->C0, h->C1, cf.img_size, eps, pos1, &wr, true, 0, &h->stem));
  }
  // ---- stage 1 (Block with attn_disabled, spatial_conv; visformer.py:241-263, Mlp :127-163)
  // WRound: estimated mean of the residual stream where the next PatchEmbed reads it.  Seeded with zeros (a stage without blocks hands on "no
  // estimate" of the right size: ADVICE r04 - depth (0, 1, 1) indexed an empty vector) and re-seeded behind every PatchEmbed.
  std::vector<double> x_mean(h->C1, 0.0);
  h->s1.resize(cf.depth[0]);
  for (int i = 0; i < cf.depth[0]; ++i) {
    const std::string p = "stage1." + std::to_string(i) + ".";
    Affine n2 = bn_affine(sd, p + "norm2.bn", h->C1, eps);
    const float* w1 = sd.get(p + "mlp.conv1.weight", {h->hid1, h->C1, 1, 1});
    const float* w2 = sd.get(p + "mlp.conv2.weight", {h->hid1, Cg, 3, 3});
    const float* w3 = sd.get(p + "mlp.conv3.weight", {h->C1, h->hid1, 1, 1});
    if (!n2.ok || !w1 || !w2 || !w3) return FSVIT_ERR_KEY;
    // operand means: conv1 reads the stream the BatchNorm saw (running mean); conv3 reads h2 = GELU(conv2(h1)), h1 = GELU(conv1(BN(x))) with
    // Gaussian pre-activations; the grouped conv2 has no bias and a GELU behind it: not corrected
    const std::vector<double> rm = vec(p + "norm2.bn.running_mean", h->C1, false);
    std::vector<double> mh2(h->hid1, 0.0), corr3;
    if (wr.on) {
      if (wr.cst.empty()) wr.cst.assign(h->C1, 0.0);
      const std::vector<double> be = vec(p + "norm2.bn.bias", h->C1, false), ga = vec(p + "norm2.bn.weight", h->C1, true);
      const std::vector<double> tf1 = tap_fraction(h->H1, 1, 3, 1);
      std::vector<double> mh1(h->hid1), vh1(h->hid1);
      for (int n = 0; n < h->hid1; ++n) {
        double mu = 0, var = 0;
        for (int c = 0; c < h->C1; ++c) { const double w = w1[(size_t)n * h->C1 + c]; mu += w * be[c]; var += w * w * ga[c] * ga[c]; }
        gauss_moments_gelu(mu, std::sqrt(var), &mh1[n], &vh1[n]);
      }
      for (int n = 0; n < h->hid1; ++n) {
        const int g0 = (n / (h->hid1 / cf.group)) * Cg;
        double mu = 0, var = 0, dummy;
        for (int c = 0; c < Cg; ++c)
          for (int t9 = 0; t9 < 9; ++t9) {
            const double w = w2[((size_t)n * Cg + c) * 9 + t9];
            mu += w * tf1[t9] * mh1[g0 + c]; var += w * w * tf1[t9] * vh1[g0 + c];
          }
        gauss_moments_gelu(mu, std::sqrt(var), &mh2[n], &dummy);
      }
    }
    RC_TRY(pack_layer(h, &h->s1[i].c1, w1, h->hid1, h->C1, 1, 1, 1, nullptr, &n2.s, prenorm_bias(w1, h->hid1, h->C1, n2.t), true, nullptr, 0, nullptr, 0,
                      &wr, &rm, nullptr, true));
    RC_TRY(pack_layer(h, &h->s1[i].c2, w2, h->hid1, Cg, 3, 3, cf.group, nullptr, nullptr, nob, false, nullptr, 0, nullptr, 0));
    RC_TRY(pack_layer(h, &h->s1[i].c3, w3, h->C1, h->hid1, 1, 1, 1, nullptr, nullptr, nob, false, nullptr, 0, nullptr, 0, &wr, &mh2, nullptr, false, &corr3));
    if (kd(kdt) == 1 && h->s1[i].c3.Kw == h->hid1) {
      const size_t n3 = (size_t)h->C1 * h->s1[i].c3.Kw;
      RC_TRY(packed_image(h, n3 * 2, &h->s1[i].c3s, [&](void* img) { return K(launch_stage1_w4_prescale)(h->s1[i].c3.w, img, (int)n3, nullptr); }));
    }
    if (wr.on) {
      x_mean.assign(h->C1, 0.0);                  // E[x] behind this block = running mean + conv3 E[h2]: the next PatchEmbed's operand mean
      for (int o = 0; o < h->C1; ++o) {
        double a = rm[o];
        for (int c = 0; c < h->hid1; ++c) a += (double)w3[(size_t)o * h->hid1 + c] * mh2[c];
        x_mean[o] = a;
        wr.cst[o] += corr3[o];
      }
    }
  }
  // ---- per stage s = 2, 3: PatchEmbed (visformer.py:266-288: conv k2 s2 + bias -> BN ; pos_embed added in the epilogue), then its
  // attention + MLP blocks (Attention :166-194, Block :259-263)
  for (int s = 2; s <= 3; ++s) {
   {
    const int Ci = s == 2 ? h->C1 : h->C2, Co = s == 2 ? h->C2 : h->C3;
    const std::string p = "patch_embed" + std::to_string(s) + ".";
    const float* w = sd.get(p + "proj.weight", {Co, Ci, 2, 2});
    const float* b = sd.get(p + "proj.bias", {Co});
    Affine bn = bn_affine(sd, p + "norm.bn", Co, eps);
    if (!w || !b || !bn.ok) return FSVIT_ERR_KEY;
    std::vector<double> bias(Co);
    for (int o = 0; o < Co; ++o) bias[o] = bn.s[o] * (double)b[o] + bn.t[o];
    // WRound: the operand is the residual stream leaving the previous stage (estimated mean x_mean); its deferred constant ends here
    RC_TRY(pack_layer(h, s == 2 ? &h->pe2 : &h->pe3, w, Co, Ci, 2, 2, 1, &bn.s, nullptr, bias, true, nullptr, 0, nullptr, 0, &wr, &x_mean, nullptr, true));
    if (wr.on) {
      wr.cst.assign(Co, 0.0);
      // the stream behind this PatchEmbed: E = BatchNorm beta + mean_hw(pos_embed) until a block of the stage refines it
      const std::vector<double> be = vec(p + "norm.bn.bias", Co, false);
      const int HW = (s == 2 ? h->H2 : h->H3) * (s == 2 ? h->H2 : h->H3);
      const float* pos = sd.get("pos_embed" + std::to_string(s), {1, Co, s == 2 ? h->H2 : h->H3, s == 2 ? h->H2 : h->H3});
      x_mean.assign(Co, 0.0);
      for (int o = 0; o < Co; ++o) {
        double a = 0.0;
        for (int q = 0; pos && q < HW; ++q) a += (double)pos[(size_t)o * HW + q];
        x_mean[o] = be[o] + a / HW;
      }
    }
    const Layer& pe = s == 2 ? h->pe2 : h->pe3;
    if (K(patch_embed_rows_supported)(kd(kdt), Ci, s == 2 ? h->H1 : h->H2, Co) && pe.Kw == 4 * Ci)
      RC_TRY(packed_image(h, K(ln_gemm_rows_image_bytes)(4 * Ci, Co), &h->pe_img[s - 2],
                          [&](void* img) { return K(launch_ln_gemm_pack)(pe.w, pe.Kw, img, 4 * Ci, Co, nullptr); }));
   }
    const int C = s == 2 ? h->C2 : h->C3, hid = s == 2 ? h->hid2 : h->hid3;
    const int hd = s == 2 ? h->hd2 : h->hd3, hdp = s == 2 ? h->hdp2 : h->hdp3;
    const int heads = cf.num_heads;
    if (C % epc || hid % epc) return fail(FSVIT_ERR_ARG, "channel counts must be multiples of %d", epc);
    std::vector<BlockA>& blocks = s == 2 ? h->s2 : h->s3;
    blocks.resize(cf.depth[s - 1]);
    // head-dim padding: qkv rows (x, y, z) -> x*heads*hdp + y*hdp + z ; proj K columns (y, z) -> y*hdp + z
    std::vector<int> rowmap(3 * heads * hd), colmap(heads * hd);
    for (int x = 0; x < 3; ++x)
      for (int y = 0; y < heads; ++y)
        for (int z = 0; z < hd; ++z) rowmap[(x * heads + y) * hd + z] = (x * heads + y) * hdp + z;
    for (int y = 0; y < heads; ++y)
      for (int z = 0; z < hd; ++z) colmap[y * hd + z] = y * hdp + z;
    for (int i = 0; i < cf.depth[s - 1]; ++i) {
      const std::string p = "stage" + std::to_string(s) + "." + std::to_string(i) + ".";
      Affine n1 = bn_affine(sd, p + "norm1.bn", C, eps), n2 = bn_affine(sd, p + "norm2.bn", C, eps);
      const float* wq = sd.get(p + "attn.qkv.weight", {3 * heads * hd, C, 1, 1});
      const float* wp = sd.get(p + "attn.proj.weight", {C, heads * hd, 1, 1});
      const float* w1 = sd.get(p + "mlp.conv1.weight", {hid, C, 1, 1});
      const float* w3 = sd.get(p + "mlp.conv3.weight", {C, hid, 1, 1});
      if (!n1.ok || !n2.ok || !wq || !wp || !w1 || !w3) return FSVIT_ERR_KEY;
      // WRound operand means: qkv / conv1 read the stream their BatchNorm saw (running means); proj reads ctx, E[ctx] ~ E[v] = W_v beta_1
      // (softmax rows sum to 1); conv3 reads GELU of a Gaussian pre-activation N(W1 beta_2, W1^2 gamma_2^2)
      const std::vector<double> rm1 = vec(p + "norm1.bn.running_mean", C, false), rm2 = vec(p + "norm2.bn.running_mean", C, false);
      std::vector<double> mctx(heads * hd, 0.0), mh(hid, 0.0), corr_p, corr_3;
      if (wr.on) {
        const std::vector<double> be1 = vec(p + "norm1.bn.bias", C, false);
        const std::vector<double> be2 = vec(p + "norm2.bn.bias", C, false), ga2 = vec(p + "norm2.bn.weight", C, true);
        for (int n = 0; n < heads * hd; ++n) {
          double a = 0;
          for (int c = 0; c < C; ++c) a += (double)wq[((size_t)2 * heads * hd + n) * C + c] * be1[c];
          mctx[n] = a;
        }
        for (int n = 0; n < hid; ++n) {
          double mu = 0, var = 0, dummy;
          for (int c = 0; c < C; ++c) { const double w = w1[(size_t)n * C + c]; mu += w * be2[c]; var += w * w * ga2[c] * ga2[c]; }
          gauss_moments_gelu(mu, std::sqrt(var), &mh[n], &dummy);
        }
      }
      RC_TRY(pack_layer(h, &blocks[i].qkv, wq, 3 * heads * hd, C, 1, 1, 1, nullptr, &n1.s, prenorm_bias(wq, 3 * heads * hd, C, n1.t), true, &rowmap, 3 * heads * hdp, nullptr, 0,
                        &wr, &rm1, nullptr, true));
      RC_TRY(pack_layer(h, &blocks[i].proj, wp, C, heads * hd, 1, 1, 1, nullptr, nullptr, nob, false, nullptr, 0, &colmap, heads * hdp, &wr, &mctx, nullptr, false, &corr_p));
      if (wr.on) for (int o = 0; o < C; ++o) wr.cst[o] += corr_p[o];
      RC_TRY(pack_layer(h, &blocks[i].fc1, w1, hid, C, 1, 1, 1, nullptr, &n2.s, prenorm_bias(w1, hid, C, n2.t), true, nullptr, 0, nullptr, 0, &wr, &rm2, nullptr, true));
      RC_TRY(pack_layer(h, &blocks[i].fc2, w3, C, hid, 1, 1, 1, nullptr, nullptr, nob, false, nullptr, 0, nullptr, 0, &wr, &mh, nullptr, false, &corr_3));
      if (wr.on) {
        x_mean.assign(C, 0.0);
        for (int o = 0; o < C; ++o) {
          double a = rm2[o];
          for (int c = 0; c < hid; ++c) a += (double)w3[(size_t)o * hid + c] * mh[c];
          x_mean[o] = a;
          wr.cst[o] += corr_3[o];
        }
      }
      if (K(mlp_rows_supported)(kd(kdt), C, hid)) {                // fused row-wise Mlp: re-pack [proj,] fc1, fc2 as the MFMA fragment stream
        const int kc = K(mlp_rows_proj_supported)(C, hid, heads * hdp) ? heads * hdp : 0;
        BlockA& b = blocks[i];
        void* b1i = nullptr;
        RC_TRY(packed_image(h, K(mlp_rows_image_bytes)(C, hid, kc), &b.mlp_img, [&](void* img) {
          HIP_TRY(hipMalloc(&b1i, (size_t)hid * 4));
          h->allocs.push_back(b1i);
          return K(launch_mlp_pack)(b.fc1.w, b.fc1.Kw, b.fc1.bias, b.fc2.w, b.fc2.Kw, b.proj.w, b.proj.Kw, kc, img, (float*)b1i, C, hid, nullptr);
        }));
        b.mlp_b1 = (float*)b1i;
        b.mlp_kc = kc;
      }
      if (K(qkv_attn_supported)(kd(kdt), C, heads, hdp, (s == 2 ? h->H2 : h->H3) * (s == 2 ? h->H2 : h->H3))) {   // fused qkv conv + attention: re-pack qkv as the MFMA fragment stream
        RC_TRY(packed_image(h, K(qkv_attn_image_bytes)(), &blocks[i].qa_img,
                            [&](void* img) { return K(launch_qkv_attn_pack)(blocks[i].qkv.w, blocks[i].qkv.Kw, img, nullptr); }));
      } else if (K(qkv_attn_rows_supported)(kd(kdt), C, heads, hdp, (s == 2 ? h->H2 : h->H3) * (s == 2 ? h->H2 : h->H3))) {   // stage 3, <= 32 tokens
        RC_TRY(packed_image(h, K(ln_gemm_rows_image_bytes)(C, 3 * heads * hdp), &blocks[i].qar_img,
                            [&](void* img) { return K(launch_qkv_attn_rows_pack)(blocks[i].qkv.w, blocks[i].qkv.Kw, img, C, heads, hdp, nullptr); }));
      } else if (K(gemm_rows_supported)(kd(kdt), C, 3 * heads * hdp)) {      // stage 3: the qkv conv as a row-wise GEMM
        RC_TRY(packed_image(h, K(ln_gemm_rows_image_bytes)(C, 3 * heads * hdp), &blocks[i].qr_img,
                            [&](void* img) { return K(launch_ln_gemm_pack)(blocks[i].qkv.w, blocks[i].qkv.Kw, img, C, 3 * heads * hdp, nullptr); }));
      }
    }
  }
  // ---- final BN -> pooled feature affine (visformer.py:455-462)
  {
    Affine bn = bn_affine(sd, "norm.bn", h->C3, eps);
    if (!bn.ok) return FSVIT_ERR_KEY;
    std::vector<float> s(h->C3), t(h->C3);
    for (int c = 0; c < h->C3; ++c) { s[c] = (float)bn.s[c]; t[c] = (float)(bn.t[c] + (wr.on ? bn.s[c] * wr.cst[c] : 0.0)); }
    void* d; RC_TRY(upload(h, s, false, &d)); h->fscale = (float*)d;
    RC_TRY(upload(h, t, false, &d)); h->fshift = (float*)d;
  }
  return 0;
}

int tap(EngineBase* h, const std::string& name, const void* src, size_t bytes, bool first, hipStream_t st) {
  if (!first || h->taps.empty()) return 0;
  auto it = h->taps.find(name);
  if (it == h->taps.end() || it->second.dst == nullptr) return 0;
  size_t n = bytes < it->second.bytes ? bytes : it->second.bytes;
  HIP_TRY(hipMemcpyAsync(it->second.dst, src, n, hipMemcpyDeviceToDevice, st));
  return 0;
}

// kernel ids reported by the profiler (names in fsvit_kernel_name)
enum {
  KID_GEMM256 = 0, KID_GEMM64 = 1, KID_GEMM32 = 2, KID_IM2COL = 3, KID_MAXPOOL = 4, KID_ATTN = 5, KID_POOL = 6, KID_HEAD = 7, KID_STAGE1 = 8, KID_GEMM128 = 9,
  KID_PATCHIFY = 10, KID_LN = 11, KID_HALO = 12, KID_MLPROWS = 13, KID_GCONV_X2 = 14, KID_QKVATTN = 15, KID_STEMCONV1 = 16, KID_STAGE1RING = 17, KID_LNGEMM = 18,
  KID_QKVATTNROWS = 19, KID_VITATTNROWS = 20
};

// Runs one launch; in profiling mode brackets it with HIP events on the same stream.
template <typename F>
int timed(EngineBase* h, hipStream_t st, const char* layer, int kernel, double flops, F&& launch) {
  if (!h->profiling) return launch();
  hipEvent_t e0 = h->prof_last, e1;
  if (!e0) { HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventRecord(e0, st)); }
  int rc = launch();
  if (rc != 0) return rc;
  HIP_TRY(hipEventCreate(&e1));
  HIP_TRY(hipEventRecord(e1, st));
  h->prof.push_back(ProfEntry{layer, kernel, flops, e0, e1});
  h->prof_last = e1;
  return 0;
}

int run_gemm(EngineBase* h, hipStream_t st, const char* layer, const Layer& L, const ConvGemmParams& p, double n_true, double k_true) {
  const int kdt = h->dtype;
  const double flops = 2.0 * (double)p.M * n_true * k_true * (double)p.groups;     // algorithmic: unpadded N and K
  static const int kid_of_cfg[4] = {KID_GEMM256, KID_GEMM64, KID_GEMM32, KID_GEMM128};
  const int route = K(conv_gemm_route)(p, kg(kdt));
  const int kid = route == 0 ? KID_HALO : route == 1 ? KID_GEMM256 : route == 3 ? KID_GCONV_X2 : kid_of_cfg[K(conv_gemm_v2_config)(p)];
  return timed(h, st, layer, kid, flops, [&]() { return K(launch_conv_gemm)(p, kg(kdt), st); });
}

// ---- the stem driver
// The images of a chunk: [0, B1) from x, the rest from x2 (the shot and query tensors of one MetaBaseline call: one pass over cat([shot, query]) as the
// reference does, meta_baseline.py:29-32, without materialising the concatenation); x2 == nullptr: one tensor
struct ImageSrc { const float* x; const float* x2; int B1; size_t isz; };   // isz: floats per image
struct ImageRun { const float* src; int a, n; };                            // images [a, a + n) of the chunk, contiguous from src
// the runs of cat(x[0:B1], x2) that intersect [a, b): one or two, the second (if any) starts at x2
int image_runs(const ImageSrc& in, int a, int b, ImageRun out[2]) {
  const int B1 = in.x2 ? in.B1 : b;
  int n = 0;
  if (a < B1) out[n++] = ImageRun{in.x + (size_t)a * in.isz, a, (b < B1 ? b : B1) - a};
  if (b > B1) { const int a2 = a > B1 ? a : B1; out[n++] = ImageRun{in.x2 + (size_t)(a2 - B1) * in.isz, a2, b - a2}; }
  return n;
}

// Scratch of ONE slice (at most s.slice images of a chunk of Bc): every slice overwrites the previous one's - in order on one stream, each map is produced
// and consumed within its slice.  c1: not on STEM_PLANAR_C1F, which never writes it.  pooled: for a caller that consumes the pooled map slice by slice.
struct StemScratch { void *patches = nullptr, *c1 = nullptr, *c2 = nullptr, *pooled = nullptr; };
StemScratch stem_scratch(const EvalStem& s, size_t es, size_t Bc, bool pooled, Arena& a) {
  const size_t n = s.slice && (size_t)s.slice < Bc ? (size_t)s.slice : Bc, P0 = (size_t)s.H0 * s.H0;
  StemScratch sc;
  sc.patches = a.take(n * P0 * 32 * es);
  if (s.route != STEM_PLANAR_C1F) sc.c1 = a.take(n * P0 * s.C0 * es);
  sc.c2 = a.take(n * P0 * s.C1 * es);
  if (pooled) sc.pooled = a.take(n * s.H1 * s.H1 * s.C1 * es);
  return sc;
}

// The stem of a chunk of Bc images in slices of s.slice.  The dedicated routes run sliced because the two halo convs take ~10 % less per image at
// 1600 ... 3200-image launches than at 12 800 (measured per launch size, profiles/r06_*; their halo fetch is bound by HBM latency, and a slice's maps are
// produced and consumed within a few ms), while every later kernel wants the whole chunk.  Per slice [g0, g0 + n): out_of(g0) is where its pooled map
// [n][H1][H1][C1] goes, after(g0, n, pooled map) runs behind it.
template <class Out, class After>
int stem_forward(EngineBase* h, const EvalStem& s, const StemScratch& sc, const ImageSrc& in, int Bc, hipStream_t st, Out&& out_of, After&& after) {
  const int kdt = h->dtype, dt = kd(kdt);
  const size_t s_pat = (size_t)s.H0 * s.H0 * 32 * h->es, s_c1 = (size_t)s.H0 * s.H0 * s.C0 * h->es;
  const double fl1 = 2.0 * 27.0 * s.C0 * s.H0 * s.H0;
  const bool planar = s.route == STEM_PLANAR || s.route == STEM_PLANAR_C1F, c1f = s.route == STEM_PLANAR_C1F, halo = s.route == STEM_HALO_NHWC;
  const int S = s.slice ? s.slice : Bc;
  for (int g0 = 0; g0 < Bc; g0 += S) {
    const int n = Bc - g0 < S ? Bc - g0 : S;
    ImageRun runs[2];
    const int n_runs = image_runs(in, g0, g0 + n, runs);
    for (int r = 0; r < n_runs && !c1f; ++r) {      // the im2col rows (and, direct, conv1's map) of each run, at the run's place in the slice
      const ImageRun& run = runs[r];
      void* pat = (unsigned char*)sc.patches + (run.a - g0) * s_pat;
      if (s.conv1_direct)
        RC_TRY(timed(h, st, "stem.im2col+conv1", KID_STEMCONV1, fl1 * run.n, [&]() {
          return K(launch_stem_conv1)(run.src, pat, (unsigned char*)sc.c1 + (run.a - g0) * s_c1, s.conv1.w, s.conv1.Kw, s.conv1.bias, run.n, st, planar ? 1 : 0); }));
      else
        RC_TRY(timed(h, st, "stem.im2col", KID_IM2COL, 0.0, [&]() { return K(launch_im2col27)(run.src, pat, run.n, s.img, s.img, s.H0, s.H0, dt, st); }));
    }
    if (!c1f && !s.conv1_direct)
      RC_TRY(run_gemm(h, st, "stem.conv1", s.conv1, conv_params(s.conv1, sc.patches, sc.c1, n, s.H0, s.H0, 32, 32, 1, 1, 1, 0, s.C0, ACT_LRELU, nullptr, 0, nullptr), s.C0, 27));
    void* out = out_of(g0);
    ConvGemmParams p2, p3;
    stem_conv_params(s, planar, sc.c1, sc.c2, sc.patches, out, n, &p2, &p3);
    if (c1f) {      // conv1 inside the conv2 kernel: it reads the raw images of the slice's runs and stores the patch rows for conv3's tail
      p2.c1f_raw = runs[0].src; p2.c1f_split = runs[0].n; p2.c1f_raw2 = in.x2;
      p2.c1f_patches = sc.patches;
      p2.c1f_w = s.conv1.w; p2.c1f_kw = s.conv1.Kw; p2.c1f_bias = s.conv1.bias;
      RC_TRY(timed(h, st, "stem.conv2", KID_HALO, 2.0 * (double)p2.M * s.C1 * 9.0 * s.C0 + fl1 * n, [&]() { return K(launch_conv_gemm)(p2, kg(kdt), st); }));
    } else
      RC_TRY(run_gemm(h, st, "stem.conv2", halo ? s.conv2h : s.conv2, p2, s.C1, 9.0 * s.C0));
    RC_TRY(run_gemm(h, st, "stem.conv3+down+pool", halo ? s.conv3h : s.conv3f, p3, s.C1, 9.0 * s.C1 + 27.0));
    RC_TRY(after(g0, n, out));
  }
  return 0;
}

// ---- Visformer: workspace of a chunk of Bc images.  The residual streams live for the whole chunk; behind them ONE region that the stem scratch of a
// slice, the stage-1 hidden maps and the stage-2 / 3 scratch (sized for the larger stage) take in turn.
struct Plan {
  void *x1, *x1b, *x2, *x3;              // residual streams (x1b: ping-pong partner for the fused stage-1 block)
  StemScratch stem;
  void *ha, *hb;                         // stage-1 hidden
  void *qkv, *ctx, *hid;                 // stage-2/3 scratch
};

Plan visformer_layout(const fsvit_visformer* h, size_t Bc, Arena& a) {
  Plan p;
  const size_t es = h->es, P1 = (size_t)h->H1 * h->H1, P2 = (size_t)h->H2 * h->H2, P3 = (size_t)h->H3 * h->H3;
  const int heads = h->cfg.num_heads;
  p.x1 = a.take(Bc * P1 * h->C1 * es);
  p.x1b = a.take(Bc * P1 * h->C1 * es);
  p.x2 = a.take(Bc * P2 * h->C2 * es);
  p.x3 = a.take(Bc * P3 * h->C3 * es);
  const size_t scratch0 = a.mark();
  p.stem = stem_scratch(h->stem, es, Bc, false, a);
  a.rewind(scratch0);
  p.ha = a.take(Bc * P1 * h->hid1 * es);
  p.hb = a.take(Bc * P1 * h->hid1 * es);
  a.rewind(scratch0);
  size_t q2 = Bc * P2 * 3 * heads * h->hdp2 * es, q3 = Bc * P3 * 3 * heads * h->hdp3 * es;
  size_t c2 = Bc * P2 * heads * h->hdp2 * es, c3 = Bc * P3 * heads * h->hdp3 * es;
  size_t h2 = Bc * P2 * h->hid2 * es, h3 = Bc * P3 * h->hid3 * es;
  p.qkv = a.take(q2 > q3 ? q2 : q3);
  p.ctx = a.take(c2 > c3 ? c2 : c3);
  p.hid = a.take(h2 > h3 ? h2 : h3);
  return p;
}

// What fsvit_*_workspace_bytes answers: the high-water mark of the encoder's layout run dry.  Monotone in Bc (every buffer grows with Bc or with
// min(Bc, slice)), which the chunk search of encoder_forward relies on.
template <class H, class P>
size_t layout_bytes(P (*layout)(const H*, size_t, Arena&), const EngineBase* h, size_t Bc) {
  Arena a;
  a.dry = true;
  layout(static_cast<const H*>(h), Bc, a);
  return a.peak;
}
// The arena of a chunk whose size the caller has already held against layout_bytes.
Arena chunk_arena(const void* ws) {
  Arena a;
  a.base = (unsigned char*)ws; a.size = SIZE_MAX;
  return a;
}

// xsrc2 != nullptr: images [0, B1) come from x, images [B1, Bc) from xsrc2 (ImageSrc)
int forward_chunk(fsvit_visformer* h, const float* x, int Bc, float* feat, unsigned char* ws, bool first, hipStream_t st,
                  const float* xsrc2 = nullptr, int B1 = 0) {
  Arena arena = chunk_arena(ws);
  const Plan pl = visformer_layout(h, Bc, arena);
  const int kdt = h->dtype, dt = kd(kdt);
  const size_t es = h->es;
  const int heads = h->cfg.num_heads;
  void *x1 = pl.x1, *x1b = pl.x1b, *x2 = pl.x2, *x3 = pl.x3, *ha = pl.ha, *hb = pl.hb;
  void *qkv = pl.qkv, *ctx = pl.ctx, *hid = pl.hid;

  // stem: every slice pools into its rows of x1
  h->prof_last = nullptr;
  const size_t s_x1 = (size_t)h->H1 * h->H1 * h->C1 * es;
  RC_TRY(stem_forward(h, h->stem, pl.stem, ImageSrc{x, xsrc2, B1, (size_t)3 * h->stem.img * h->stem.img}, Bc, st,
                      [&](int g0) { return (void*)((unsigned char*)x1 + g0 * s_x1); }, [](int, int, void*) { return 0; }));
  RC_TRY(tap(h, "stem", x1, (size_t)Bc * s_x1, first, st));

  // stage 1: x += conv3(GELU(conv2_g(GELU(conv1(BN(x))))))
  const int Cg = h->hid1 / h->cfg.group;
  // one LDS-resident kernel per block (stage1_w4.hip, any map up to 20 wide); other geometries / numerics modes take the three-launch route
  const bool fuse1 = K(stage1_ring_supported)(dt, h->C1, h->hid1, h->cfg.group, h->H1) && h->s1.size() && h->s1[0].c2.Kw == 320;
  for (size_t i = 0; i < h->s1.size(); ++i) {
    const Block1& b = h->s1[i];
    if (fuse1) {   // one LDS-resident kernel per block, ping-pong between x1 and x1b
      const double fl = 2.0 * Bc * h->H1 * h->H1 * ((double)h->hid1 * h->C1 + (double)h->hid1 * 9 * Cg + (double)h->C1 * h->hid1);
      RC_TRY(timed(h, st, "stage1.block", KID_STAGE1RING, fl,
                   [&]() { return K(launch_stage1_ring)(x1, x1b, b.c1.w, b.c1.bias, b.c2.w, b.c3.w, Bc, h->H1, h->H1, st, b.c3s); }));
      std::swap(x1, x1b);
    } else {
      RC_TRY(run_gemm(h, st, "stage1.mlp.conv1", b.c1, conv_params(b.c1, x1, ha, Bc, h->H1, h->H1, h->C1, h->C1, 1, 1, 1, 0, h->hid1, ACT_GELU, nullptr, 0, nullptr), h->hid1, h->C1));
      RC_TRY(run_gemm(h, st, "stage1.mlp.conv2", b.c2, conv_params(b.c2, ha, hb, Bc, h->H1, h->H1, Cg, h->hid1, 3, 3, 1, 1, h->hid1, ACT_GELU, nullptr, 0, nullptr), Cg, 9.0 * Cg));
      RC_TRY(run_gemm(h, st, "stage1.mlp.conv3", b.c3, conv_params(b.c3, hb, x1, Bc, h->H1, h->H1, h->hid1, h->hid1, 1, 1, 1, 0, h->C1, ACT_NONE, x1, 0, nullptr), h->C1, h->hid1));
    }
    RC_TRY(tap(h, "stage1." + std::to_string(i), x1, (size_t)Bc * h->H1 * h->H1 * h->C1 * es, first, st));
  }

  // stages 2 and 3
  for (int s = 2; s <= 3; ++s) {
    const int Ci = s == 2 ? h->C1 : h->C2, C = s == 2 ? h->C2 : h->C3;
    const int Hi = s == 2 ? h->H1 : h->H2, Ho = s == 2 ? h->H2 : h->H3;
    const int hidc = s == 2 ? h->hid2 : h->hid3, hd = s == 2 ? h->hd2 : h->hd3, hdp = s == 2 ? h->hdp2 : h->hdp3;
    void* xin = s == 2 ? x1 : x2;
    void* xs = s == 2 ? x2 : x3;
    const Layer& pe = s == 2 ? h->pe2 : h->pe3;
    const float* pos = s == 2 ? h->pos2 : h->pos3;
    const size_t xbytes = (size_t)Bc * Ho * Ho * C * es;
    const std::string sp = "stage" + std::to_string(s);
    if (h->pe_img[s - 2]) {
      RC_TRY(timed(h, st, s == 2 ? "patch_embed2" : "patch_embed3", KID_LNGEMM, 2.0 * Bc * Ho * Ho * 4.0 * Ci * C,
                   [&]() { return K(launch_patch_embed_rows)(xin, xs, h->pe_img[s - 2], pe.bias, pos, Bc, Hi, Ci, C, st); }));
    } else
    RC_TRY(run_gemm(h, st, s == 2 ? "patch_embed2" : "patch_embed3", pe, conv_params(pe, xin, xs, Bc, Hi, Hi, Ci, Ci, 2, 2, 2, 0, C, ACT_NONE, nullptr, 0, pos), C, 4.0 * Ci));
    RC_TRY(tap(h, "patch_embed" + std::to_string(s), xs, xbytes, first, st));
    const std::vector<BlockA>& blocks = s == 2 ? h->s2 : h->s3;
    const float scale = 1.0f / std::sqrt((float)hd);                       // head_dim ** -0.5 (visformer.py:174)
    const int S = Ho * Ho;
    for (size_t i = 0; i < blocks.size(); ++i) {
      const BlockA& b = blocks[i];
      if (b.qa_img) {     // qkv conv + attention core in one launch: q / k / v never leave the chip
        RC_TRY(timed(h, st, (sp + ".attn.qkv+core").c_str(), KID_QKVATTN, 2.0 * Bc * S * (3.0 * heads * hd) * C + 4.0 * Bc * heads * (double)S * S * hd,
                     [&]() { return K(launch_qkv_attn)(xs, ctx, b.qa_img, b.qkv.bias, Bc, S, scale, st); }));
      } else if (b.qar_img) {
        RC_TRY(timed(h, st, (sp + ".attn.qkv+core").c_str(), KID_QKVATTNROWS, 2.0 * Bc * S * (3.0 * heads * hd) * C + 4.0 * Bc * heads * (double)S * S * hd,
                     [&]() { return K(launch_qkv_attn_rows)(xs, ctx, b.qar_img, b.qkv.bias, Bc, S, C, heads, hdp, scale, st); }));
      } else {
      if (b.qr_img) {
        RC_TRY(timed(h, st, (sp + ".attn.qkv").c_str(), KID_LNGEMM, 2.0 * Bc * S * (3.0 * heads * hd) * C,
                     [&]() { return K(launch_gemm_rows)(xs, qkv, b.qr_img, b.qkv.bias, Bc * S, C, 3 * heads * hdp, st); }));
      } else
      RC_TRY(run_gemm(h, st, (sp + ".attn.qkv").c_str(), b.qkv, conv_params(b.qkv, xs, qkv, Bc, Ho, Ho, C, C, 1, 1, 1, 0, 3 * heads * hdp, ACT_NONE, nullptr, 0, nullptr), 3.0 * heads * hd, C));
      RC_TRY(timed(h, st, (sp + ".attn.core").c_str(), KID_ATTN, 4.0 * Bc * heads * (double)S * S * hd,
                   [&]() { return K(launch_attention)(qkv, ctx, Bc, S, heads, hdp, scale, is_x2(h->dtype) ? 2 : dt, st); }));
      }
      if (b.mlp_img && b.mlp_kc) {   // proj + residual + conv1 + GELU + conv3 + residual in one launch
        RC_TRY(timed(h, st, (sp + ".proj+mlp").c_str(), KID_MLPROWS, 2.0 * Bc * S * ((double)C * heads * hd + 2.0 * hidc * C),
                     [&]() { return K(launch_mlp_rows)(xs, xs, b.mlp_img, b.mlp_b1, b.fc2.bias, ctx, b.mlp_kc, Bc * S, C, hidc, st); }));
        RC_TRY(tap(h, sp + "." + std::to_string(i), xs, xbytes, first, st));
        continue;
      }
      RC_TRY(run_gemm(h, st, (sp + ".attn.proj").c_str(), b.proj, conv_params(b.proj, ctx, xs, Bc, Ho, Ho, heads * hdp, heads * hdp, 1, 1, 1, 0, C, ACT_NONE, xs, 0, nullptr), C, (double)heads * hd));
      if (b.mlp_img) {     // conv1 + GELU + conv3 + residual in one launch, the hidden map stays in registers
        RC_TRY(timed(h, st, (sp + ".mlp").c_str(), KID_MLPROWS, 4.0 * Bc * S * (double)hidc * C,
                     [&]() { return K(launch_mlp_rows)(xs, xs, b.mlp_img, b.mlp_b1, b.fc2.bias, nullptr, 0, Bc * S, C, hidc, st); }));
      } else {
        RC_TRY(run_gemm(h, st, (sp + ".mlp.conv1").c_str(), b.fc1, conv_params(b.fc1, xs, hid, Bc, Ho, Ho, C, C, 1, 1, 1, 0, hidc, ACT_GELU, nullptr, 0, nullptr), hidc, C));
        RC_TRY(run_gemm(h, st, (sp + ".mlp.conv3").c_str(), b.fc2, conv_params(b.fc2, hid, xs, Bc, Ho, Ho, hidc, hidc, 1, 1, 1, 0, C, ACT_NONE, xs, 0, nullptr), C, hidc));
      }
      RC_TRY(tap(h, sp + "." + std::to_string(i), xs, xbytes, first, st));
    }
  }
  RC_TRY(timed(h, st, "norm.pool", KID_POOL, 0.0, [&]() { return K(launch_pool_affine)(x3, h->fscale, h->fshift, feat, Bc, h->H3 * h->H3, h->C3, dt, st); }));
  return 0;
}

size_t visformer_plan_bytes(const EngineBase* h, size_t Bc) { return layout_bytes(visformer_layout, h, Bc); }
int visformer_chunk(EngineBase* h, const float* x, int Bc, float* feat, unsigned char* ws, bool first, hipStream_t st) {
  return forward_chunk(static_cast<fsvit_visformer*>(h), x, Bc, feat, ws, first, st);
}

// ---- the handle plumbing every encoder shares behind its fsvit_<encoder>_* entry points
template <class H>
void encoder_destroy(H* h) {
  if (!h) return;
  for (void* p : h->allocs) (void)hipFree(p);
  delete h;
}

// bad_cfg / bad_cfg_msg: the caller's range check of *cfg (false for a null cfg); build_fn packs the state dict into the new handle
template <class H, class Cfg>
int encoder_create(const Cfg* cfg, const fsvit_tensor* state_dict, int n_tensors, int dtype, H** out, bool bad_cfg, const char* bad_cfg_msg, int kind,
                   int (*build_fn)(H*, const SD&), size_t (*plan_bytes)(const EngineBase*, size_t),
                   int (*chunk)(EngineBase*, const float*, int, float*, unsigned char*, bool, hipStream_t), const char* size_fmt) {
  if (!cfg || !state_dict || !out || n_tensors <= 0) return fail(FSVIT_ERR_ARG, "null argument");
  if (!known_dtype(dtype)) return fail(FSVIT_ERR_ARG, "unknown dtype %d", dtype);
  if (bad_cfg) return fail(FSVIT_ERR_ARG, "%s", bad_cfg_msg);
  H* h = new H();
  h->kind = kind;
  h->cfg = *cfg;
  h->img_size = cfg->img_size;
  h->dtype = dtype;
  h->es = storage_bytes(dtype);
  h->plan_bytes = plan_bytes; h->chunk = chunk; h->size_fmt = size_fmt;
  SD sd{state_dict, n_tensors};
  int rc = build_fn(h, sd);
  if (rc != 0) { encoder_destroy(h); return rc; }
  *out = h;
  return 0;
}

size_t encoder_workspace_bytes(const EngineBase* h, int chunk_images) {
  if (!h || chunk_images <= 0) return 0;
  return h->plan_bytes(h, (size_t)chunk_images);
}

// the image-size messages restate the reference's asserts (visformer.py:283-284,431: "does not match"; deit.py:96-97 and lvvit.py: "doesn't match")
const char* const SIZE_FMT_VISFORMER = "Input image size (%d*%d) does not match model (%d*%d).";
const char* const SIZE_FMT_VIT = "Input image size (%d*%d) doesn't match model (%d*%d).";

int encoder_forward(EngineBase* h, const float* x, int n_img, int img_h, int img_w, float* feat, void* ws, size_t ws_bytes, void* stream) {
  if (h && n_img <= 0) return 0;
  if (!h || !x || !feat || !ws) return fail(FSVIT_ERR_ARG, "null argument");
  if (img_h != h->img_size || img_w != h->img_size) return fail(FSVIT_ERR_IMG_SIZE, h->size_fmt, img_h, img_w, h->img_size, h->img_size);
  if (((uintptr_t)ws & 255) != 0) return fail(FSVIT_ERR_ARG, "workspace must be 256-byte aligned");
  // largest chunk that fits the workspace (plan size is monotone in the chunk)
  int lo = 0, hi = n_img;
  while (lo < hi) {
    int mid = (lo + hi + 1) / 2;
    if (h->plan_bytes(h, (size_t)mid) <= ws_bytes) lo = mid; else hi = mid - 1;
  }
  if (lo < 1) return fail(FSVIT_ERR_WORKSPACE, "workspace of %zu bytes cannot hold one image (need %zu)", ws_bytes, h->plan_bytes(h, 1));
  const size_t img_elems = (size_t)3 * img_h * img_w;
  for (int off = 0; off < n_img; off += lo) {
    const int bc = n_img - off < lo ? n_img - off : lo;
    int rc = h->chunk(h, x + (size_t)off * img_elems, bc, feat + (size_t)off * h->out_dim, (unsigned char*)ws, off == 0, (hipStream_t)stream);
    if (rc != 0) return rc;
  }
  return 0;
}

}  // namespace

// ------------------------------------------------------------------------------------ C ABI
extern "C" int fsvit_visformer_create(const fsvit_visformer_cfg* cfg, const fsvit_tensor* state_dict, int n_tensors,
                                      int dtype, fsvit_visformer** out) {
  const bool bad = cfg && (cfg->num_heads < 1 || cfg->embed_dim < 2 || cfg->init_channels < 1 || cfg->depth[0] < 0 || cfg->depth[1] < 0 || cfg->depth[2] < 0);
  return encoder_create(cfg, state_dict, n_tensors, dtype, out, bad, "bad Visformer configuration", KIND_VISFORMER, build, visformer_plan_bytes, visformer_chunk,
                        SIZE_FMT_VISFORMER);
}
extern "C" void fsvit_visformer_destroy(fsvit_visformer* h) { encoder_destroy(h); }
extern "C" int fsvit_visformer_out_dim(const fsvit_visformer* h) { return h ? h->out_dim : 0; }
extern "C" int fsvit_visformer_dtype(const fsvit_visformer* h) { return h ? h->dtype : -1; }
extern "C" size_t fsvit_visformer_workspace_bytes(const fsvit_visformer* h, int chunk_images) { return encoder_workspace_bytes(h, chunk_images); }

extern "C" int fsvit_encoder_set_tap(void* hv, const char* name, void* dst_dev, size_t bytes) {
  EngineBase* h = static_cast<EngineBase*>(hv);
  if (!h || !name) return fail(FSVIT_ERR_ARG, "null argument");
  if (!dst_dev) h->taps.erase(name);
  else h->taps[name] = Tap{dst_dev, bytes};
  return 0;
}

extern "C" int fsvit_visformer_forward(fsvit_visformer* h, const float* x, int n_img, int img_h, int img_w,
                                       float* feat, void* ws, size_t ws_bytes, void* stream) {
  return encoder_forward(h, x, n_img, img_h, img_w, feat, ws, ws_bytes, stream);
}

/* Post-norm token map [n_img][H3*H3][C3] fp32 of the images of the LAST fsvit_visformer_forward call on this handle (same workspace,
 * untouched since; the call must have fitted one chunk): the `x` of `return x, pooled` in the distillation phase's encoder
 * (sun_meta_training/models/visformer.py:464) for the eval-mode teacher. */
extern "C" int fsvit_visformer_last_tokens(fsvit_visformer* h, const void* ws, size_t ws_bytes, int n_img, float* tokens, void* stream) {
  const int kdt = h ? h->dtype : FSVIT_BF16;
  if (!h || !ws || !tokens || n_img <= 0) return fail(FSVIT_ERR_ARG, "bad argument");
  if (visformer_plan_bytes(h, (size_t)n_img) > ws_bytes) return fail(FSVIT_ERR_WORKSPACE, "last_tokens: the forward of %d images did not fit one chunk of this workspace", n_img);
  Arena arena = chunk_arena(ws);
  RC_TRY(K(launch_tokens_to_f32)(visformer_layout(h, (size_t)n_img, arena).x3, h->fscale, h->fshift, tokens, (size_t)n_img * h->H3 * h->H3 * h->C3, h->C3, kd(kdt),
                              (hipStream_t)stream));
  return 0;
}

extern "C" int fsvit_proto_head(const float* fs, const float* fq, int E, int way, int shot, int Q, int D, float temp,
                                int method, float* logits, float* acc, float* loss, void* stream) {
  if (!fs || !fq || !logits) return fail(FSVIT_ERR_ARG, "null argument");
  if (method != FSVIT_HEAD_COS && method != FSVIT_HEAD_SQR && method != FSVIT_HEAD_DOT) return fail(FSVIT_ERR_ARG, "unknown head method %d", method);
  RC_TRY(fsvit::launch_proto_head(fs, fq, E, way, shot, Q, D, temp, method, logits, acc, loss, (hipStream_t)stream, nullptr));
  return 0;
}

extern "C" int fsvit_proto_head_devtemp(const float* fs, const float* fq, int E, int way, int shot, int Q, int D, const float* temp_dev,
                                        int method, float* logits, float* acc, float* loss, void* stream) {
  if (!fs || !fq || !logits || !temp_dev) return fail(FSVIT_ERR_ARG, "null argument");
  if (method != FSVIT_HEAD_COS && method != FSVIT_HEAD_SQR && method != FSVIT_HEAD_DOT) return fail(FSVIT_ERR_ARG, "unknown head method %d", method);
  RC_TRY(fsvit::launch_proto_head(fs, fq, E, way, shot, Q, D, 0.f, method, logits, acc, loss, (hipStream_t)stream, temp_dev));
  return 0;
}

extern "C" int fsvit_proto_head_gather(const float* table, int N, int D, const void* idx, int idx_is_int64, int E, int way, int shot, int n_query, float temp,
                                       const float* temp_dev, int method, float* logits, float* acc, float* loss, int* invalid, void* stream) {
  if (!table || !idx || !logits || !invalid) return fail(FSVIT_ERR_ARG, "fsvit_proto_head_gather: null argument");
  if (method != FSVIT_HEAD_COS && method != FSVIT_HEAD_SQR && method != FSVIT_HEAD_DOT) return fail(FSVIT_ERR_ARG, "unknown head method %d", method);
  if (E < 0 || N < 1 || D < 1 || way < 1 || shot < 1 || n_query < 1)
    return fail(FSVIT_ERR_ARG, "fsvit_proto_head_gather: E = %d, N = %d, D = %d, way = %d, shot = %d, n_query = %d", E, N, D, way, shot, n_query);
  const size_t lds = ((size_t)way * D + (size_t)way * n_query * 2) * sizeof(float);
  if (lds > 160 * 1024)
    return fail(FSVIT_ERR_ARG, "fsvit_proto_head_gather: way = %d prototypes of D = %d with %d queries per class need %zu bytes of LDS (limit 163840)", way, D, n_query, lds);
  RC_TRY(fsvit::launch_proto_head_gather(table, N, D, idx, idx_is_int64, E, way, shot, n_query, temp_dev ? 0.f : temp, method, logits, acc, loss, invalid,
                                         (hipStream_t)stream, temp_dev));
  return 0;
}

// ---- prototype bank (proto_bank.hip): limits as fsvit.h states them
static int proto_bank_dims(const char* what, int way, int D) {
  if (way < 1 || way > 65536) return fail(FSVIT_ERR_ARG, "%s: way = %d is outside [1, 65536]", what, way);
  if (D < 1 || D > 8192) return fail(FSVIT_ERR_ARG, "%s: D = %d is outside [1, 8192]", what, D);
  return 0;
}

extern "C" int fsvit_proto_bank_accumulate(const float* feat, const void* label, int label_is_int64, int S, int way, int D, float* sum, int* count,
                                           int* invalid, void* stream) {
  if (!feat || !label || !sum || !count || !invalid) return fail(FSVIT_ERR_ARG, "fsvit_proto_bank_accumulate: null argument");
  if (S < 0) return fail(FSVIT_ERR_ARG, "fsvit_proto_bank_accumulate: S = %d", S);
  RC_TRY(proto_bank_dims("fsvit_proto_bank_accumulate", way, D));
  RC_TRY(fsvit::launch_proto_bank_accumulate(feat, label, label_is_int64, S, way, D, sum, count, invalid, (hipStream_t)stream));
  return 0;
}

extern "C" int fsvit_proto_bank_finalize(const float* sum, const int* count, int way, int D, int method, float* proto, int* empty, void* stream) {
  if (!sum || !count || !proto || !empty) return fail(FSVIT_ERR_ARG, "fsvit_proto_bank_finalize: null argument");
  if (method != FSVIT_HEAD_COS && method != FSVIT_HEAD_SQR && method != FSVIT_HEAD_DOT) return fail(FSVIT_ERR_ARG, "unknown head method %d", method);
  RC_TRY(proto_bank_dims("fsvit_proto_bank_finalize", way, D));
  RC_TRY(fsvit::launch_proto_bank_finalize(sum, count, way, D, method, proto, empty, (hipStream_t)stream));
  return 0;
}

extern "C" int fsvit_proto_bank_logits(const float* query, const float* proto, const int* empty, int Q, int way, int D, float temp, const float* temp_dev,
                                       int method, float* logits, int* pred, void* stream) {
  if (!query || !proto || !logits) return fail(FSVIT_ERR_ARG, "fsvit_proto_bank_logits: null argument");
  if (method != FSVIT_HEAD_COS && method != FSVIT_HEAD_SQR && method != FSVIT_HEAD_DOT) return fail(FSVIT_ERR_ARG, "unknown head method %d", method);
  if (Q < 0) return fail(FSVIT_ERR_ARG, "fsvit_proto_bank_logits: Q = %d", Q);
  RC_TRY(proto_bank_dims("fsvit_proto_bank_logits", way, D));
  if (D % 4) return fail(FSVIT_ERR_ARG, "fsvit_proto_bank_logits: D = %d is not a multiple of 4", D);
  if (((uintptr_t)query | (uintptr_t)proto) & 15) return fail(FSVIT_ERR_ARG, "fsvit_proto_bank_logits: query / proto must be 16-byte aligned");
  if (!temp_dev && !std::isfinite(temp)) return fail(FSVIT_ERR_ARG, "fsvit_proto_bank_logits: the temperature is not finite");
  RC_TRY(fsvit::launch_proto_bank_logits(query, proto, empty, Q, way, D, temp_dev ? 0.f : temp, temp_dev, method, logits, pred, (hipStream_t)stream));
  return 0;
}

// n_split of fsvit_proto_bank_topk when the caller passes 0 (the rule is stated in fsvit.h); 0 when the arguments admit none
static int proto_bank_topk_split(int Q, int way, int n_split) {
  if (Q < 0 || way < 1 || way > 65536 || n_split < 0) return 0;
  const int n_seg = (way + 1023) / 1024;
  if (n_split > n_seg) return 0;
  if (n_split) return n_split;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
  const int q_tiles = Q > 0 ? (Q + 63) / 64 : 1;
  const int want = (cus + q_tiles - 1) / q_tiles;
  return want < 1 ? 1 : (want > n_seg ? n_seg : want);
}

extern "C" size_t fsvit_proto_bank_topk_workspace_bytes(int Q, int way, int K, int n_split) {
  const int ns = proto_bank_topk_split(Q, way, n_split);
  if (!ns || K < 1 || K > 32) return 0;
  return fsvit::proto_bank_topk_workspace_bytes(Q, way, K, ns);
}

extern "C" int fsvit_proto_bank_topk(const float* query, const float* proto, const int* empty, int Q, int way, int D, float temp, const float* temp_dev,
                                     int method, int K, int n_split, float* values, int* indices, float* lse, void* ws, size_t ws_bytes, void* stream) {
  if (!query || !proto || !values || !indices) return fail(FSVIT_ERR_ARG, "fsvit_proto_bank_topk: null argument");
  if (method != FSVIT_HEAD_COS && method != FSVIT_HEAD_SQR && method != FSVIT_HEAD_DOT) return fail(FSVIT_ERR_ARG, "unknown head method %d", method);
  if (Q < 0) return fail(FSVIT_ERR_ARG, "fsvit_proto_bank_topk: Q = %d", Q);
  RC_TRY(proto_bank_dims("fsvit_proto_bank_topk", way, D));
  if (D % 4) return fail(FSVIT_ERR_ARG, "fsvit_proto_bank_topk: D = %d is not a multiple of 4", D);
  if (((uintptr_t)query | (uintptr_t)proto) & 15) return fail(FSVIT_ERR_ARG, "fsvit_proto_bank_topk: query / proto must be 16-byte aligned");
  if (!temp_dev && !std::isfinite(temp)) return fail(FSVIT_ERR_ARG, "fsvit_proto_bank_topk: the temperature is not finite");
  if (K < 1 || K > 32) return fail(FSVIT_ERR_ARG, "fsvit_proto_bank_topk: K = %d is outside [1, 32]", K);
  const int ns = proto_bank_topk_split(Q, way, n_split);
  if (!ns) return fail(FSVIT_ERR_ARG, "fsvit_proto_bank_topk: n_split = %d is outside [0, %d] (one split per 1024 classes at most)", n_split, (way + 1023) / 1024);
  const size_t need = fsvit::proto_bank_topk_workspace_bytes(Q, way, K, ns);
  if (Q == 0) return 0;                                        // nothing to score: the workspace of 0 bytes may be null
  if (!ws || ((uintptr_t)ws & 3) || ws_bytes < need)
    return fail(FSVIT_ERR_ARG, "fsvit_proto_bank_topk: the workspace is null, misaligned or smaller than the %zu bytes of fsvit_proto_bank_topk_workspace_bytes", need);
  RC_TRY(fsvit::launch_proto_bank_topk(query, proto, empty, Q, way, D, temp_dev ? 0.f : temp, temp_dev, method, K, ns, values, indices, lse, ws,
                                       (hipStream_t)stream));
  return 0;
}

extern "C" int fsvit_proto_auc(const float* feat_shot, const float* feat_query, int E, int shot, int Q, int D, float* auc, float* score, void* stream) {
  if (!feat_shot || !feat_query || !auc) return fail(FSVIT_ERR_ARG, "fsvit_proto_auc: null argument");
  if (E < 0 || shot < 1) return fail(FSVIT_ERR_ARG, "fsvit_proto_auc: E = %d, shot = %d", E, shot);
  if (Q < 2 || Q > 4096 || Q % 2) return fail(FSVIT_ERR_ARG, "fsvit_proto_auc: Q = %d must be even and in [2, 4096] (positives first, as many negatives)", Q);
  RC_TRY(proto_bank_dims("fsvit_proto_auc", 1, D));
  RC_TRY(fsvit::launch_proto_auc(feat_shot, feat_query, E, shot, Q, D, auc, score, (hipStream_t)stream));
  return 0;
}

extern "C" int fsvit_proto_auc_gather(const float* table, int N, int D, const void* shot_slots, const void* query_slots, int idx_is_int64, int E, int shot,
                                      int Q, float* auc, float* score, int* invalid, void* stream) {
  if (!table || !shot_slots || !query_slots || !auc || !invalid) return fail(FSVIT_ERR_ARG, "fsvit_proto_auc_gather: null argument");
  if (E < 0 || N < 1 || shot < 1) return fail(FSVIT_ERR_ARG, "fsvit_proto_auc_gather: E = %d, N = %d, shot = %d", E, N, shot);
  if (Q < 2 || Q > 4096 || Q % 2)
    return fail(FSVIT_ERR_ARG, "fsvit_proto_auc_gather: Q = %d must be even and in [2, 4096] (positives first, as many negatives)", Q);
  RC_TRY(proto_bank_dims("fsvit_proto_auc_gather", 1, D));
  RC_TRY(fsvit::launch_proto_auc_gather(table, N, D, shot_slots, query_slots, idx_is_int64, E, shot, Q, auc, score, invalid, (hipStream_t)stream));
  return 0;
}

extern "C" int fsvit_meta_baseline_forward(void* hv, const float* x_shot, const float* x_query, int E, int way,
                                           int shot, int Q, int img_h, int img_w, float temp, int method, float* logits,
                                           float* acc, float* loss, float* feat, void* ws, size_t ws_bytes, void* stream) {
  if (!hv || !feat) return fail(FSVIT_ERR_ARG, "null argument");
  EngineBase* eb = static_cast<EngineBase*>(hv);
  if (!eb->chunk) return fail(FSVIT_ERR_ARG, "not an fsvit encoder handle");
  const int ns = E * way * shot, nq = E * Q, D = eb->out_dim;
  // the reference encodes cat([shots, queries]) in one call (meta_baseline.py:29-32); eval mode is
  // per-image independent, so two passes into one feature buffer are equivalent
  {   // Visformer: ONE pass over shots + queries when the workspace holds them all (larger launches, fewer tile tails)
    if (eb->kind == KIND_VISFORMER && x_shot && x_query && ns > 0 && nq > 0) {
      fsvit_visformer* h = static_cast<fsvit_visformer*>(eb);
      if (img_h != h->cfg.img_size || img_w != h->cfg.img_size)
        return fail(FSVIT_ERR_IMG_SIZE, SIZE_FMT_VISFORMER, img_h, img_w, h->cfg.img_size, h->cfg.img_size);
      if (ws && ((uintptr_t)ws & 255) == 0 && visformer_plan_bytes(h, (size_t)ns + nq) <= ws_bytes) {
        int rc1 = forward_chunk(h, x_shot, ns + nq, feat, (unsigned char*)ws, true, (hipStream_t)stream, x_query, ns);
        if (rc1 != 0) return rc1;
        return fsvit_proto_head(feat, feat + (size_t)ns * D, E, way, shot, Q, D, temp, method, logits, acc, loss, stream);
      }
    }
  }
  int rc = encoder_forward(eb, x_shot, ns, img_h, img_w, feat, ws, ws_bytes, stream);
  if (rc != 0) return rc;
  rc = encoder_forward(eb, x_query, nq, img_h, img_w, feat + (size_t)ns * D, ws, ws_bytes, stream);
  if (rc != 0) return rc;
  return fsvit_proto_head(feat, feat + (size_t)ns * D, E, way, shot, Q, D, temp, method, logits, acc, loss, stream);
}

extern "C" int fsvit_conv_gemm(const void* x, const void* w, const float* bias, const void* res, const float* pos, void* y,
                               int B, int H, int W, int Cin, int x_cstride, int KH, int KW, int stride, int pad, int N,
                               int y_cstride, int Kw, int groups, int act, int res_first, int dtype, void* stream) {
  const int kdt = dtype;
  if (!known_dtype(dtype)) return fail(FSVIT_ERR_ARG, "unknown dtype %d", dtype);
  if (!x || !w || !y) return fail(FSVIT_ERR_ARG, "null argument");
  const int es = storage_bytes(dtype), epc = 16 / es, bke = 128 / es;
  if (Cin % epc || x_cstride % epc || N % 4 || y_cstride % 4 || Kw % bke || Kw < KH * KW * Cin)
    return fail(FSVIT_ERR_ARG, "conv_gemm alignment: Cin/x_cstride %% %d, N/y_cstride %% 4, Kw %% %d", epc, bke);
  if (KH * KW > 1 && !is_pow2(Cin) && Cin % 32) return fail(FSVIT_ERR_ARG, "multi-tap conv needs a power-of-two Cin or a multiple of 32");
  Layer L; L.w = const_cast<void*>(w); L.bias = const_cast<float*>(bias); L.N = N; L.K = KH * KW * Cin; L.Kw = Kw; L.groups = groups;
  ConvGemmParams p = conv_params(L, x, y, B, H, W, Cin, x_cstride, KH, KW, stride, pad, y_cstride, act, res, res_first, pos);
  RC_TRY(K(launch_conv_gemm)(p, kg(dtype), (hipStream_t)stream));
  return 0;
}

/* The stem's fused tail (visformer.py:213,224-237 + :431): out = MaxPool2d(2)(LeakyReLU(conv3x3(x, w[:, :9*Cin]) + x2 . w[:, Kmain:] + bias)) + pos
 * - conv3 + bn3 with the downsample conv + bn_d riding as ONE extra K slice over the im2col rows x2, pooled and position-embedded in the
 * epilogue.  Routed exactly as the engine routes it (conv3x3_halo_kernel<128,true> for the Visformer-S geometry, conv_gemm_v2 otherwise). */
extern "C" int fsvit_conv_stem_tail(const void* x, const void* w, const float* bias, const float* pos, const void* x2, int x2_cstride, int K2,
                                    void* y, int B, int H, int W, int Cin, int N, int Kw, int dtype, void* stream) {
  const int kdt = dtype;
  if (!known_dtype(dtype)) return fail(FSVIT_ERR_ARG, "unknown dtype %d", dtype);
  if (!x || !w || !y || !x2 || !pos) return fail(FSVIT_ERR_ARG, "null argument");
  const int es = storage_bytes(dtype), epc = 16 / es, bke = 128 / es;
  if (Cin % epc || (!is_pow2(Cin) && Cin % 32) || N % 4 || Kw % bke || Kw < 9 * Cin + bke || K2 > bke || x2_cstride < K2 || (H & 1) || (W & 1))
    return fail(FSVIT_ERR_ARG, "fsvit_conv_stem_tail: bad geometry");
  Layer L; L.w = const_cast<void*>(w); L.bias = const_cast<float*>(bias); L.N = N; L.K = 9 * Cin; L.Kw = Kw; L.groups = 1;
  ConvGemmParams p = conv_params(L, x, y, B, H, W, Cin, Cin, 3, 3, 1, 1, N, ACT_LRELU, nullptr, 0, pos);
  p.x2 = x2; p.x2_cstride = x2_cstride; p.K2 = K2; p.pool2 = 1;
  RC_TRY(K(launch_conv_gemm)(p, kg(dtype), (hipStream_t)stream));
  return 0;
}

/* LV-ViT's 96-channel stem convs on the dedicated conv3x3_halo instantiation (bf16 / f16 only; an error where it does not apply): pool == 0: conv2,
 * y = LeakyReLU(conv3x3(x) + bias) [B][H][W][96]; pool == 1: conv3 + tail, y = MaxPool2d(2)(LeakyReLU(conv3x3(x) + x2 . tail + bias)) [B][H/2][W/2][96].
 * w: the 128-channel image [128][9 * 128 (+ 64)], k = tap * 128 + c, zero past 96 channels / rows, the tail slice (im2col rows x2, K2 <= 32) last. */
extern "C" int fsvit_stem96_conv(const void* x, const void* w, const float* bias, const void* x2, int x2_cstride, int K2, void* y, int B, int H, int W,
                                 int pool, int dtype, void* stream) {
  const int kdt = dtype;
  if (dtype != FSVIT_BF16 && dtype != FSVIT_F16) return fail(FSVIT_ERR_ARG, "fsvit_stem96_conv: bf16 / f16 only");
  if (!x || !w || !y || (pool && !x2)) return fail(FSVIT_ERR_ARG, "null argument");
  Layer L; L.w = const_cast<void*>(w); L.bias = const_cast<float*>(bias); L.N = 96; L.K = 9 * 96; L.Kw = 9 * 128 + (pool ? 64 : 0); L.groups = 1;
  ConvGemmParams p = conv_params(L, x, y, B, H, W, 96, 96, 3, 3, 1, 1, 96, ACT_LRELU, nullptr, 0, nullptr);
  p.w_cpad = 128;
  if (pool) { p.x2 = x2; p.x2_cstride = x2_cstride; p.K2 = K2; p.pool2 = 1; }
  if (K(conv_gemm_route)(p, kg(dtype)) != 0) return fail(FSVIT_ERR_ARG, "fsvit_stem96_conv: geometry not supported (W = 40, H a multiple of 8, K2 = 32)");
  RC_TRY(K(launch_conv_gemm)(p, kg(dtype), (hipStream_t)stream));
  return 0;
}

extern "C" int fsvit_stage1_block(const void* x, void* y, const void* w1, const float* b1, const void* w2, const void* w3, int B, void* stream) {
  const int kdt = FSVIT_BF16;
  if (!x || !y || !w1 || !b1 || !w2 || !w3 || x == y || B <= 0) return fail(FSVIT_ERR_ARG, "bad argument");
  RC_TRY(K(launch_stage1_ring16)(x, y, w1, b1, w2, w3, B, 20, 20, (hipStream_t)stream));
  return 0;
}

extern "C" int fsvit_stage1_block_hw(const void* x, void* y, const void* w1, const float* b1, const void* w2, const void* w3, int B, int H, int W, int dtype,
                                     void* stream) {
  const int kdt = dtype;
  if (!x || !y || !w1 || !b1 || !w2 || !w3 || x == y || B <= 0) return fail(FSVIT_ERR_ARG, "bad argument");
  if (dtype != FSVIT_BF16 && dtype != FSVIT_F16) return fail(FSVIT_ERR_ARG, "fsvit_stage1_block_hw: 16-bit storage only (bf16 / f16)");
  if (H != W || !K(stage1_ring_supported)(1, 128, 256, 8, W)) return fail(FSVIT_ERR_ARG, "fsvit_stage1_block_hw: square maps of 4 .. 20 tokens a side");
  RC_TRY(K(launch_stage1_ring)(x, y, w1, b1, w2, w3, B, H, W, (hipStream_t)stream, nullptr));
  return 0;
}

/* fsvit_stage1_block_hw with the conv3 weights the engines hand the kernel: prescaled != 0 builds the 8 x W3 image with launch_stage1_w4_prescale (as
 * visformer pack does for every stage-1 block) and launches stage1_w4_kernel<true, true> on it; prescaled == 0 is fsvit_stage1_block_hw (<true, false>). */
extern "C" int fsvit_op_stage1_block_eval(const void* x, void* y, const void* w1, const float* b1, const void* w2, const void* w3, int B, int H, int W, int dtype,
                                          int prescaled, void* stream) {
  const int kdt = dtype;
  if (!x || !y || !w1 || !b1 || !w2 || !w3 || x == y || B <= 0) return fail(FSVIT_ERR_ARG, "fsvit_op_stage1_block_eval: bad argument");
  if (dtype != FSVIT_BF16 && dtype != FSVIT_F16) return fail(FSVIT_ERR_ARG, "fsvit_op_stage1_block_eval: 16-bit storage only (bf16 / f16)");
  if (H != W || !K(stage1_ring_supported)(1, 128, 256, 8, W)) return fail(FSVIT_ERR_ARG, "fsvit_op_stage1_block_eval: square maps of 4 .. 20 tokens a side");
  if ((long)B * H * W >= (1L << 31) - 256) return fail(FSVIT_ERR_ARG, "fsvit_op_stage1_block_eval: map too large");
  hipStream_t st = (hipStream_t)stream;
  if (!prescaled) {
    RC_TRY(K(launch_stage1_ring)(x, y, w1, b1, w2, w3, B, H, W, st, nullptr));
    return 0;
  }
  const int n3 = 128 * 256;
  void* w3s = nullptr;
  HIP_TRY(hipMalloc(&w3s, (size_t)n3 * 2));
  int rc = K(launch_stage1_w4_prescale)(w3, w3s, n3, st);
  if (rc == 0) rc = K(launch_stage1_ring)(x, y, w1, b1, w2, w3, B, H, W, st, w3s);
  (void)hipStreamSynchronize(st);
  (void)hipFree(w3s);
  if (rc != 0) return hipfail((hipError_t)rc, "fsvit_op_stage1_block_eval");
  return 0;
}

/* Every field of ConvGemmParams an evaluation launch sets, through launch_conv_gemm (fsvit.h: fsvit_conv_eval_args).  Refuses what the kernels would misread:
 * the row-chunk-planar operands, the 128-channel weight image, the C1F fields and `stats` only where the eligibility functions accept them. */
extern "C" int fsvit_op_conv_eval(const fsvit_conv_eval_args* a, int dtype, int* route, int* stats_rows, void* stream) {
  const int kdt = dtype;
  static const char fn[] = "fsvit_op_conv_eval";
  if (!a) return fail(FSVIT_ERR_ARG, "%s: null argument", fn);
  if (!known_dtype(dtype)) return fail(FSVIT_ERR_ARG, "%s: unknown dtype %d", fn, dtype);
  if ((!a->x && !a->c1f_raw) || !a->w || !a->y || a->x == a->y) return fail(FSVIT_ERR_ARG, "%s: null argument, or y == x", fn);
  if (a->act != FSVIT_ACT_NONE && a->act != FSVIT_ACT_GELU && a->act != FSVIT_ACT_LRELU) return fail(FSVIT_ERR_ARG, "%s: act %d (none | GELU | LeakyReLU)", fn, a->act);
  if (a->B < 1 || a->H < 1 || a->W < 1 || a->Cin < 1 || a->N < 1 || a->groups < 1 || a->KH < 1 || a->KW < 1 || a->stride < 1 || a->pad < 0 ||
      a->H + 2 * a->pad < a->KH || a->W + 2 * a->pad < a->KW)
    return fail(FSVIT_ERR_ARG, "%s: bad geometry", fn);
  const int es = storage_bytes(dtype), epc = 16 / es, bke = 128 / es;
  if (a->Cin % epc || a->x_cstride % epc || a->x_cstride < a->groups * a->Cin || a->N % 4 || a->y_cstride % 4 || a->y_cstride < a->groups * a->N || a->Kw % bke ||
      a->Kw < a->KH * a->KW * a->Cin)
    return fail(FSVIT_ERR_ARG, "%s: alignment: Cin / x_cstride %% %d, N / y_cstride %% 4, Kw %% %d and >= KH * KW * Cin", fn, epc, bke);
  if (a->KH * a->KW > 1 && !is_pow2(a->Cin) && a->Cin % 32) return fail(FSVIT_ERR_ARG, "%s: a multi-tap conv needs a power-of-two Cin or a multiple of 32", fn);
  Layer L; L.w = const_cast<void*>(a->w); L.bias = const_cast<float*>(a->bias); L.N = a->N; L.K = a->KH * a->KW * a->Cin; L.Kw = a->Kw; L.groups = a->groups;
  ConvGemmParams p = conv_params(L, a->x, a->y, a->B, a->H, a->W, a->Cin, a->x_cstride, a->KH, a->KW, a->stride, a->pad, a->y_cstride, a->act, a->res,
                                 a->res_first ? 1 : 0, a->pos);
  if ((long)a->B * p.OH * p.OW > 0x7fffffffL - 256) return fail(FSVIT_ERR_ARG, "%s: map too large", fn);
  if (a->x2 || a->K2 || a->x2_cstride) {      // the tail operand: one more K slice behind the main columns
    if (!a->x2 || a->K2 < 1 || a->K2 > bke || a->x2_cstride < a->K2 || a->x2_cstride % epc || a->groups != 1 || a->Kw < (a->w_cpad ? 9 * a->w_cpad : L.K) + bke)
      return fail(FSVIT_ERR_ARG, "%s: tail operand: x2, 1 <= K2 <= %d <= x2_cstride, one group, Kw >= K + %d", fn, bke, bke);
    p.x2 = a->x2; p.x2_cstride = a->x2_cstride; p.K2 = a->K2;
  }
  if (a->pool2) {
    if (a->res || a->y_rpi || (p.OH & 1) || (p.OW & 1) || a->stride != 1) return fail(FSVIT_ERR_ARG, "%s: pool2 needs even OH / OW, stride 1, no residual, dense rows", fn);
    p.pool2 = 1;
  }
  if (a->y_rpi || a->y_row0) {
    if (a->y_row0 < 0 || a->y_rpi < a->y_row0 + p.OH * p.OW) return fail(FSVIT_ERR_ARG, "%s: y_rpi %d < y_row0 %d + OH * OW", fn, a->y_rpi, a->y_row0);
    p.y_rpi = a->y_rpi; p.y_row0 = a->y_row0;
  }
  p.x_planar = a->x_planar ? 1 : 0; p.y_planar = a->y_planar ? 1 : 0; p.w_cpad = a->w_cpad;
  if ((p.x_planar || p.y_planar || p.w_cpad) && !K(conv3x3_halo_eligible)(p, kg(dtype)))
    return fail(FSVIT_ERR_ARG, "%s: planar operands / the 128-channel weight image on a layer conv3x3_halo does not take", fn);
  if (a->c1f_raw || a->c1f_raw2 || a->c1f_patches || a->c1f_w || a->c1f_bias || a->c1f_kw || a->c1f_split) {
    if (!a->c1f_raw || !a->c1f_patches || !a->c1f_w || !a->c1f_bias || a->c1f_kw < 32 || a->c1f_split < 0 || a->c1f_split > a->B ||
        (a->c1f_split < a->B && !a->c1f_raw2) || !K(conv3x3_halo_c1f_supported)(p, kg(dtype)))
      return fail(FSVIT_ERR_ARG, "%s: C1F: raw images, patches, conv1 weights (row length >= 32) and bias on the planar 64 -> 128 layer of 40 x 40 maps only", fn);
    p.c1f_raw = a->c1f_raw; p.c1f_raw2 = a->c1f_raw2; p.c1f_split = a->c1f_split; p.c1f_patches = a->c1f_patches;
    p.c1f_w = a->c1f_w; p.c1f_bias = a->c1f_bias; p.c1f_kw = a->c1f_kw;
  } else if (!a->x) {
    return fail(FSVIT_ERR_ARG, "%s: null argument", fn);
  }
  int rows = 0;
  if (a->stats) {
    if (p.c1f_raw) return fail(FSVIT_ERR_ARG, "%s: stats with C1F", fn);
    rows = K(conv_stats_rows)(p, kg(dtype));
    if (rows <= 0) return fail(FSVIT_ERR_ARG, "%s: this layer's kernel has no statistics epilogue", fn);
    p.stats = a->stats;
    if ((p.x_planar || p.y_planar || p.w_cpad) && !K(conv3x3_halo_eligible)(p, kg(dtype)))
      return fail(FSVIT_ERR_ARG, "%s: stats with a planar output / the 128-channel weight image", fn);
  }
  if (stats_rows) *stats_rows = rows;
  if (route) *route = K(conv_gemm_route)(p, kg(dtype));
  RC_TRY(K(launch_conv_gemm)(p, kg(dtype), (hipStream_t)stream));
  return 0;
}

extern "C" int fsvit_conv3x3_wgrad(const void* x, const void* dz, float* dw, int B, int H, int W, int O, int Ig, int groups, int dtype, void* stream) {
  const int kdt = dtype;
  if (!x || !dz || !dw) return fail(FSVIT_ERR_ARG, "null argument");
  if (dtype != FSVIT_BF16 && dtype != FSVIT_F16 && !is_x2(dtype))
    return fail(FSVIT_ERR_ARG, "fsvit_conv3x3_wgrad: bf16 / f16 activations, or fp32 activations with two-limb arithmetic (FSVIT_BF16X2 / FSVIT_F16X2)");
  if (!K(wgrad3x3_supported)(kg(dtype), O, Ig, groups, W)) return fail(FSVIT_ERR_ARG, "fsvit_conv3x3_wgrad: built for 8 groups of 32 -> 32 channels (W <= 20) and dense 64 / 128 -> 128, 96 -> 96 (W <= 40)");
  hipStream_t st = (hipStream_t)stream;
  void* scratch = nullptr;
  HIP_TRY(hipMalloc(&scratch, K(wgrad3x3_scratch_bytes)(O, Ig, groups, B * H * W, kg(dtype))));
  int rc = K(launch_wgrad3x3)(x, groups * Ig, dz, O, dw, (float*)scratch, B, H, W, O, Ig, groups, st, nullptr, kg(dtype));
  (void)hipStreamSynchronize(st);
  (void)hipFree(scratch);
  if (rc != 0) return hipfail((hipError_t)rc, "fsvit_conv3x3_wgrad");
  return 0;
}

extern "C" int fsvit_gconv3x3(const void* x, const void* w_packed, int Kw, void* y, int B, int H, int W, int dtype, void* stream) {
  const int kdt = dtype;
  if (!x || !w_packed || !y || B <= 0) return fail(FSVIT_ERR_ARG, "bad argument");
  if (dtype != FSVIT_BF16 && dtype != FSVIT_F16) return fail(FSVIT_ERR_ARG, "fsvit_gconv3x3: 16-bit storage only (bf16 / f16)");
  if (!K(gconv3x3_supported)(1, 256, 32, 8, 3, 3, 1, 1, W) || Kw < 288 || (Kw & 7)) return fail(FSVIT_ERR_ARG, "fsvit_gconv3x3: 8 groups of 32 -> 32 channels, W <= 20, Kw >= 288");
  RC_TRY(K(launch_gconv3x3)(x, w_packed, Kw, y, B, H, W, (hipStream_t)stream, nullptr, nullptr));
  return 0;
}

extern "C" int fsvit_conv1x1_wgrad(const void* x, const void* dz, float* dw, int M, int N, int C, int dtype, void* stream) {
  const int kdt = dtype;
  if (!x || !dz || !dw || M <= 0) return fail(FSVIT_ERR_ARG, "bad argument");
  if (dtype != FSVIT_BF16 && dtype != FSVIT_F16 && !is_x2(dtype))
    return fail(FSVIT_ERR_ARG, "fsvit_conv1x1_wgrad: bf16 / f16 rows, or fp32 rows with two-limb arithmetic (FSVIT_BF16X2 / FSVIT_F16X2)");
  if (!K(wgrad1x1_supported)(kg(dtype), N, C)) return fail(FSVIT_ERR_ARG, "fsvit_conv1x1_wgrad: N and C must be multiples of 8");
  hipStream_t st = (hipStream_t)stream;
  const int splits = K(wgrad1x1_splits)(N, C, M, kg(dtype)), Kc_pad = (C + 3) / 4 * 4;
  void* ysp = nullptr;
  HIP_TRY(hipMalloc(&ysp, (size_t)((N + 3) / 4 * 4) * splits * Kc_pad * 4));
  int rc = K(launch_wgrad1x1)(x, C, C, dz, N, N, (float*)ysp, M, Kc_pad, st, kg(dtype));
  if (rc == 0) rc = fsvit::launch_wgrad_finalize((const float*)ysp, dw, N, C, 1, 1, 0, splits, Kc_pad, 1, 1, 1, 1, st);
  (void)hipStreamSynchronize(st);
  (void)hipFree(ysp);
  if (rc != 0) return hipfail((hipError_t)rc, "fsvit_conv1x1_wgrad");
  return 0;
}

// The row-kernel operators below exist as NAME_dt(..., dtype, stream) for the two 16-bit storage types (FSVIT_BF16 / FSVIT_F16: the fsvit / fsvit_f16
// builds of the same kernel) and, with the signature they always had, as NAME(..., stream) = NAME_dt(..., FSVIT_BF16, stream).
extern "C" int fsvit_mlp_rows(const void* x, void* y, const void* w1, int k1w, const float* b1, const void* w2, int k2w, const float* b2,
                              int M, int C, int hid, void* stream) {
  return fsvit_proj_mlp_rows_dt(x, y, nullptr, nullptr, 0, 0, w1, k1w, b1, w2, k2w, b2, M, C, hid, FSVIT_BF16, stream);
}
extern "C" int fsvit_mlp_rows_dt(const void* x, void* y, const void* w1, int k1w, const float* b1, const void* w2, int k2w, const float* b2,
                                 int M, int C, int hid, int dtype, void* stream) {
  return fsvit_proj_mlp_rows_dt(x, y, nullptr, nullptr, 0, 0, w1, k1w, b1, w2, k2w, b2, M, C, hid, dtype, stream);
}

extern "C" int fsvit_proj_mlp_rows(const void* x, void* y, const void* ctx, const void* wp, int kpw, int KC, const void* w1, int k1w, const float* b1,
                                   const void* w2, int k2w, const float* b2, int M, int C, int hid, void* stream) {
  return fsvit_proj_mlp_rows_dt(x, y, ctx, wp, kpw, KC, w1, k1w, b1, w2, k2w, b2, M, C, hid, FSVIT_BF16, stream);
}
extern "C" int fsvit_proj_mlp_rows_dt(const void* x, void* y, const void* ctx, const void* wp, int kpw, int KC, const void* w1, int k1w, const float* b1,
                                      const void* w2, int k2w, const float* b2, int M, int C, int hid, int dtype, void* stream) {
  const int kdt = dtype;
  if (!half_dtype(dtype)) return fail(FSVIT_ERR_ARG, "fsvit_mlp_rows: 16-bit storage only (bf16 / f16)");
  if (!x || !y || !w1 || !w2) return fail(FSVIT_ERR_ARG, "null argument");
  if (!K(mlp_rows_supported)(1, C, hid)) return fail(FSVIT_ERR_ARG, "fsvit_mlp_rows: only C = 256 / hidden = 1024 and C = 512 / hidden = 2048 are built");
  if (k1w < C || k2w < hid) return fail(FSVIT_ERR_ARG, "weight rows shorter than K");
  if (ctx && (!wp || kpw < KC || !K(mlp_rows_proj_supported)(C, hid, KC))) return fail(FSVIT_ERR_ARG, "proj fusion: (C, KC) must be (256, 288) or (512, 576)");
  if (!ctx) KC = 0;
  hipStream_t st = (hipStream_t)stream;
  void *img = nullptr, *b1i = nullptr;
  HIP_TRY(hipMalloc(&img, K(mlp_rows_image_bytes)(C, hid, KC)));
  hipError_t e = hipMalloc(&b1i, (size_t)hid * 4);
  if (e != hipSuccess) { (void)hipFree(img); return hipfail(e, "hipMalloc"); }
  int rc = K(launch_mlp_pack)(w1, k1w, b1, w2, k2w, wp, kpw, KC, img, (float*)b1i, C, hid, st);
  if (rc == 0) rc = K(launch_mlp_rows)(x, y, img, (const float*)b1i, b2, ctx, KC, M, C, hid, st);
  (void)hipStreamSynchronize(st);
  (void)hipFree(img);
  (void)hipFree(b1i);
  if (rc != 0) return hipfail((hipError_t)rc, "fsvit_mlp_rows");
  return 0;
}

// The ViT / DeiT block tail as one operator (deit.py:69-72): x1 = x + bp + wp ctx; y = x1 + b2 + W2 GELU(W1 LN(x1) + b1), LN without affine
// (fold gamma / beta into w1 / b1: W1 diag(gamma), b1 + W1 beta - what the engine's packer does).  Packs the weights on every call.
extern "C" int fsvit_vit_block_tail(const void* x, void* y, const void* ctx, const void* wp, int kpw, int KC, const float* bp, const void* w1, int k1w,
                                    const float* b1, const void* w2, int k2w, const float* b2, int M, int C, int hid, float eps, void* stream) {
  return fsvit_vit_block_tail_dt(x, y, ctx, wp, kpw, KC, bp, w1, k1w, b1, w2, k2w, b2, M, C, hid, eps, FSVIT_BF16, stream);
}
extern "C" int fsvit_vit_block_tail_dt(const void* x, void* y, const void* ctx, const void* wp, int kpw, int KC, const float* bp, const void* w1, int k1w,
                                    const float* b1, const void* w2, int k2w, const float* b2, int M, int C, int hid, float eps, int dtype, void* stream) {
  const int kdt = dtype;
  if (!half_dtype(dtype)) return fail(FSVIT_ERR_ARG, "fsvit_vit_block_tail: 16-bit storage only (bf16 / f16)");
  if (!x || !y || !ctx || !wp || !bp || !w1 || !b1 || !w2 || !b2) return fail(FSVIT_ERR_ARG, "null argument");
  if (!K(mlp_rows_ln_supported)(1, C, hid, KC)) return fail(FSVIT_ERR_ARG, "fsvit_vit_block_tail: only C = 384 / hidden = 1536 or 1152 / KC = 384 is built");
  if (k1w < C || k2w < hid || kpw < KC) return fail(FSVIT_ERR_ARG, "weight rows shorter than K");
  hipStream_t st = (hipStream_t)stream;
  void *img = nullptr, *b1i = nullptr;
  HIP_TRY(hipMalloc(&img, K(mlp_rows_image_bytes)(C, hid, KC)));
  hipError_t e = hipMalloc(&b1i, (size_t)hid * 4);
  if (e != hipSuccess) { (void)hipFree(img); return hipfail(e, "hipMalloc"); }
  int rc = K(launch_mlp_pack)(w1, k1w, b1, w2, k2w, wp, kpw, KC, img, (float*)b1i, C, hid, st);
  if (rc == 0) rc = K(launch_mlp_rows_ln)(x, y, img, (const float*)b1i, bp, b2, ctx, KC, M, C, hid, eps, st);
  (void)hipStreamSynchronize(st);
  (void)hipFree(img);
  (void)hipFree(b1i);
  if (rc != 0) return hipfail((hipError_t)rc, "fsvit_vit_block_tail");
  return 0;
}

// LayerNorm + Linear on token rows as one operator (the DeiT block's norm1 + qkv, deit.py:40-47,:69): y [M][N] = b + W LN(x), LN without affine
// (gamma / beta folded into w / b by the caller).  bf16, C = 384, N a multiple of 32.  Packs the weights on every call.
extern "C" int fsvit_ln_linear_rows(const void* x, void* y, const void* w, int kw, const float* b, int M, int C, int N, float eps, void* stream) {
  return fsvit_ln_linear_rows_dt(x, y, w, kw, b, M, C, N, eps, FSVIT_BF16, stream);
}
extern "C" int fsvit_ln_linear_rows_dt(const void* x, void* y, const void* w, int kw, const float* b, int M, int C, int N, float eps, int dtype, void* stream) {
  const int kdt = dtype;
  if (!half_dtype(dtype)) return fail(FSVIT_ERR_ARG, "fsvit_ln_linear_rows: 16-bit storage only (bf16 / f16)");
  if (!x || !y || !w || (!b && C != 512)) return fail(FSVIT_ERR_ARG, "null argument");
  const bool plain = C == 512;      // the Visformer stage-3 geometry runs the same kernel without the LayerNorm (eps ignored)
  if (!(plain ? K(gemm_rows_supported)(1, C, N) : K(ln_gemm_rows_supported)(1, C, N)) || kw < C)
    return fail(FSVIT_ERR_ARG, "fsvit_ln_linear_rows: C = 384 (LayerNorm + Linear) or 512 (Linear only), N a multiple of 32, rows of at least C weights");
  hipStream_t st = (hipStream_t)stream;
  void* img = nullptr;
  HIP_TRY(hipMalloc(&img, K(ln_gemm_rows_image_bytes)(C, N)));
  int rc = K(launch_ln_gemm_pack)(w, kw, img, C, N, st);
  if (rc == 0) rc = plain ? K(launch_gemm_rows)(x, y, img, b, M, C, N, st) : K(launch_ln_gemm_rows)(x, y, img, b, M, C, N, eps, st);
  (void)hipStreamSynchronize(st);
  (void)hipFree(img);
  if (rc != 0) return hipfail((hipError_t)rc, "fsvit_ln_linear_rows");
  return 0;
}

// PatchEmbed of the Visformer stages as one operator (visformer.py:266-288: conv k2 s2 -> BN, + pos_embed): x NHWC bf16 [B][H][H][Ci] with
// 4 Ci = 512 (patch_embed2 of Visformer-S), w [N][kw >= 4 Ci] K-major in (ky, kx, c) order with the eval BatchNorm folded, bias [N] or NULL,
// pos fp32 [(H/2)^2][N]; y [B (H/2)^2][N].  Packs the weights on every call.
extern "C" int fsvit_patch_embed2x2(const void* x, void* y, const void* w, int kw, const float* bias, const float* pos, int B, int H, int Ci, int N,
                                    void* stream) {
  return fsvit_patch_embed2x2_dt(x, y, w, kw, bias, pos, B, H, Ci, N, FSVIT_BF16, stream);
}
extern "C" int fsvit_patch_embed2x2_dt(const void* x, void* y, const void* w, int kw, const float* bias, const float* pos, int B, int H, int Ci, int N,
                                       int dtype, void* stream) {
  const int kdt = dtype;
  if (!half_dtype(dtype)) return fail(FSVIT_ERR_ARG, "fsvit_patch_embed2x2: 16-bit storage only (bf16 / f16)");
  if (!x || !y || !w || !pos) return fail(FSVIT_ERR_ARG, "null argument");
  if (!K(patch_embed_rows_supported)(1, Ci, H, N) || kw < 4 * Ci) return fail(FSVIT_ERR_ARG, "fsvit_patch_embed2x2: 4 Ci = 512, even H, N a multiple of 32");
  hipStream_t st = (hipStream_t)stream;
  void* img = nullptr;
  HIP_TRY(hipMalloc(&img, K(ln_gemm_rows_image_bytes)(4 * Ci, N)));
  int rc = K(launch_ln_gemm_pack)(w, kw, img, 4 * Ci, N, st);
  if (rc == 0) rc = K(launch_patch_embed_rows)(x, y, img, bias, pos, B, H, Ci, N, st);
  (void)hipStreamSynchronize(st);
  (void)hipFree(img);
  if (rc != 0) return hipfail((hipError_t)rc, "fsvit_patch_embed2x2");
  return 0;
}

// ---- distillation head (sun_meta_training/offline.py, models/token_label.py, models/classifier.py)
extern "C" int fsvit_linear_forward(const float* x, const float* w, const float* b, float* y, int M, int N, int K, void* stream) {
  if (!x || !w || !y || (K & 3) || N <= 0 || K <= 0) return fail(FSVIT_ERR_ARG, "fsvit_linear_forward: null argument or K %% 4 != 0");
  RC_TRY(fsvit::launch_linear_fwd(x, w, b, y, M, N, K, (hipStream_t)stream));
  return 0;
}
extern "C" int fsvit_linear_backward(const float* dy, const float* x, const float* w, float* dx, int accumulate_dx, float* dw, float* db,
                                     int M, int N, int K, void* stream) {
  if (!dy || (dx && !w) || (dw && !x) || N <= 0 || K <= 0) return fail(FSVIT_ERR_ARG, "fsvit_linear_backward: bad argument");
  RC_TRY(fsvit::launch_linear_bwd(dy, x, w, dx, accumulate_dx, dw, db, M, N, K, (hipStream_t)stream));
  return 0;
}
extern "C" int fsvit_token_softlabel(const float* teacher_logits, float* soft, int B, int T, int C, int k, int bp, double smoothing, void* stream) {
  if (!teacher_logits || !soft || T > 64 || T <= 0 || C < 2 || k < 1 || k > C || bp < 0 || bp > T)
    return fail(FSVIT_ERR_ARG, "fsvit_token_softlabel: bad argument (T <= 64, 1 <= k <= C, 0 <= bp <= T)");
  RC_TRY(fsvit::launch_token_softlabel(teacher_logits, soft, B, T, C, k, bp, smoothing, (hipStream_t)stream));
  return 0;
}
extern "C" int fsvit_soft_target_ce(const float* logits, const float* target, float* row_loss, float* dlogits, int R, int C, float grad_scale,
                                    void* stream) {
  if (!logits || !target || !row_loss || C <= 0) return fail(FSVIT_ERR_ARG, "fsvit_soft_target_ce: bad argument");
  RC_TRY(fsvit::launch_soft_target_ce(logits, target, row_loss, dlogits, R, C, grad_scale, (hipStream_t)stream));
  return 0;
}
extern "C" int fsvit_row_normalize(const float* x, float* y, float* inv_norm, int R, int D, void* stream) {
  if (!x || !y || !inv_norm || D <= 0) return fail(FSVIT_ERR_ARG, "fsvit_row_normalize: bad argument");
  RC_TRY(fsvit::launch_row_normalize(x, y, inv_norm, R, D, (hipStream_t)stream));
  return 0;
}
extern "C" int fsvit_row_normalize_backward(const float* y, const float* inv_norm, const float* dy, float* dx, int R, int D, void* stream) {
  if (!y || !inv_norm || !dy || !dx || D <= 0) return fail(FSVIT_ERR_ARG, "fsvit_row_normalize_backward: bad argument");
  RC_TRY(fsvit::launch_row_normalize_bwd(y, inv_norm, dy, dx, R, D, (hipStream_t)stream));
  return 0;
}
extern "C" int fsvit_qkv_attention(const void* x, const void* wqkv, int kw, const float* bias, void* ctx, int B, int S, int C, int heads, int hdp,
                                   float scale, void* stream) {
  return fsvit_qkv_attention_dt(x, wqkv, kw, bias, ctx, B, S, C, heads, hdp, scale, FSVIT_BF16, stream);
}
extern "C" int fsvit_qkv_attention_dt(const void* x, const void* wqkv, int kw, const float* bias, void* ctx, int B, int S, int C, int heads, int hdp,
                                   float scale, int dtype, void* stream) {
  const int kdt = dtype;
  if (!half_dtype(dtype)) return fail(FSVIT_ERR_ARG, "fsvit_qkv_attention: 16-bit storage only (bf16 / f16)");
  if (!x || !wqkv || !ctx) return fail(FSVIT_ERR_ARG, "null argument");
  hipStream_t st = (hipStream_t)stream;
  void* img = nullptr;
  if (C == 512) {       // the rows kernel (stage-3 geometry: head dim padded to 96, maps of at most 32 tokens)
    if (!K(qkv_attn_rows_supported)(1, C, heads, hdp, S) || kw < C)
      return fail(FSVIT_ERR_ARG, "fsvit_qkv_attention: C = 512 needs head dim 96 (padded) and S <= 32");
    HIP_TRY(hipMalloc(&img, K(ln_gemm_rows_image_bytes)(C, 3 * heads * hdp)));
    int rc = K(launch_qkv_attn_rows_pack)(wqkv, kw, img, C, heads, hdp, st);
    if (rc == 0) rc = K(launch_qkv_attn_rows)(x, ctx, img, bias, B, S, C, heads, hdp, scale, st);
    (void)hipStreamSynchronize(st);
    (void)hipFree(img);
    if (rc != 0) return hipfail((hipError_t)rc, "fsvit_qkv_attention");
    return 0;
  }
  if (!K(qkv_attn_supported)(1, C, heads, hdp, S) || kw < C)
    return fail(FSVIT_ERR_ARG, "fsvit_qkv_attention: only C = 256, 6 heads x 48 (padded), S <= 112 is built");
  HIP_TRY(hipMalloc(&img, K(qkv_attn_image_bytes)()));
  int rc = K(launch_qkv_attn_pack)(wqkv, kw, img, st);
  if (rc == 0) rc = K(launch_qkv_attn)(x, ctx, img, bias, B, S, scale, st);
  (void)hipStreamSynchronize(st);
  (void)hipFree(img);
  if (rc != 0) return hipfail((hipError_t)rc, "fsvit_qkv_attention");
  return 0;
}

extern "C" int fsvit_vit_ln_qkv_attention(const void* x, const void* wqkv, int kw, const float* bias, void* ctx, int B, int S, int C, int heads, int hdp,
                                          float eps, float scale, void* stream) {
  return fsvit_vit_ln_qkv_attention_dt(x, wqkv, kw, bias, ctx, B, S, C, heads, hdp, eps, scale, FSVIT_BF16, stream);
}
extern "C" int fsvit_vit_ln_qkv_attention_dt(const void* x, const void* wqkv, int kw, const float* bias, void* ctx, int B, int S, int C, int heads, int hdp,
                                          float eps, float scale, int dtype, void* stream) {
  const int kdt = dtype;
  if (!half_dtype(dtype)) return fail(FSVIT_ERR_ARG, "fsvit_vit_ln_qkv_attention: 16-bit storage only (bf16 / f16)");
  if (!x || !wqkv || !ctx) return fail(FSVIT_ERR_ARG, "null argument");
  if (!K(vit_attn_rows_supported)(1, C, heads, hdp, S) || kw < C)
    return fail(FSVIT_ERR_ARG, "fsvit_vit_ln_qkv_attention: built for C = 384, head dim 64, S <= 256");
  hipStream_t st = (hipStream_t)stream;
  void* img = nullptr;
  HIP_TRY(hipMalloc(&img, K(ln_gemm_rows_image_bytes)(C, 3 * heads * hdp)));
  int rc = K(launch_qkv_attn_rows_pack)(wqkv, kw, img, C, heads, hdp, st);
  if (rc == 0) rc = K(launch_vit_attn_rows)(x, ctx, img, bias, B, S, C, heads, hdp, eps, scale, st);
  (void)hipStreamSynchronize(st);
  (void)hipFree(img);
  if (rc != 0) return hipfail((hipError_t)rc, "fsvit_vit_ln_qkv_attention");
  return 0;
}

extern "C" int fsvit_op_attention_route(int S, int hdp, int dtype) {
  const int kdt = dtype;
  if (!known_dtype(dtype)) return -1;
  return K(attention_route)(S, hdp, kg(dtype));
}

extern "C" int fsvit_attention(const void* qkv, void* ctx, int B, int S, int heads, int hdp, float scale, int dtype, void* stream) {
  const int kdt = dtype;
  if (!known_dtype(dtype)) return fail(FSVIT_ERR_ARG, "unknown dtype %d", dtype);
  if (!qkv || !ctx) return fail(FSVIT_ERR_ARG, "null argument");
  if (B < 0 || heads < 1) return fail(FSVIT_ERR_ARG, "fsvit_attention: B = %d, heads = %d (B >= 0, heads >= 1)", B, heads);
  if (K(attention_route)(S, hdp, kg(dtype)) < 0)
    return fail(FSVIT_ERR_ARG, "fsvit_attention: no kernel covers S = %d, hdp = %d in dtype %d (fsvit.h)", S, hdp, dtype);
  int rc = K(launch_attention)(qkv, ctx, B, S, heads, hdp, scale, kg(dtype), (hipStream_t)stream);      // (kg: the two-limb dtypes run the two-limb kernels, as in the engines)
  if (rc != 0) return hipfail((hipError_t)rc, "attention");
  return 0;
}

extern "C" int fsvit_im2col27(const float* x, void* out, int B, int H, int W, int dtype, void* stream) {
  const int kdt = dtype;
  if (!known_dtype(dtype)) return fail(FSVIT_ERR_ARG, "unknown dtype %d", dtype);
  if (!x || !out || (H & 1) || (W & 1)) return fail(FSVIT_ERR_ARG, "bad argument");
  RC_TRY(K(launch_im2col27)(x, out, B, H, W, H / 2, W / 2, kd(dtype), (hipStream_t)stream));
  return 0;
}

extern "C" int fsvit_stem_conv1(const float* x, const void* w, int kw, const float* bias, void* patches, void* c1, int B, int H, int W, void* stream) {
  return fsvit_stem_conv1_dt(x, w, kw, bias, patches, c1, B, H, W, FSVIT_BF16, stream);
}
extern "C" int fsvit_stem_conv1_dt(const float* x, const void* w, int kw, const float* bias, void* patches, void* c1, int B, int H, int W, int dtype, void* stream) {
  return fsvit_op_stem_conv1(x, w, kw, bias, patches, c1, B, H, W, dtype, 0, stream);
}
extern "C" int fsvit_op_stem_conv1(const float* x, const void* w, int kw, const float* bias, void* patches, void* c1, int B, int H, int W, int dtype, int c1_planar,
                                   void* stream) {
  const int kdt = dtype;
  if (!half_dtype(dtype)) return fail(FSVIT_ERR_ARG, "fsvit_stem_conv1: 16-bit storage only (bf16 / f16)");
  if (!x || !w || !patches || !c1 || kw < 32) return fail(FSVIT_ERR_ARG, "bad argument");
  if (H != W || !K(stem_conv1_supported)(1, H, 64)) return fail(FSVIT_ERR_ARG, "fsvit_stem_conv1: only 80x80 images, 64 output channels are built");
  RC_TRY(K(launch_stem_conv1)(x, patches, c1, w, kw, bias, B, (hipStream_t)stream, c1_planar ? 1 : 0));
  return 0;
}

extern "C" int fsvit_maxpool2_pos(const void* in, const float* pos, void* out, int B, int OH, int OW, int C, int dtype, void* stream) {
  const int kdt = dtype;
  if (!known_dtype(dtype)) return fail(FSVIT_ERR_ARG, "unknown dtype %d", dtype);
  if (!in || !out || C % 4) return fail(FSVIT_ERR_ARG, "bad argument");
  RC_TRY(K(launch_maxpool2_pos)(in, pos, out, B, OH, OW, C, kd(dtype), (hipStream_t)stream));
  return 0;
}

extern "C" int fsvit_pool_affine(const void* x, const float* scale, const float* shift, float* feat, int B, int HW, int C,
                                 int dtype, void* stream) {
  const int kdt = dtype;
  if (!known_dtype(dtype)) return fail(FSVIT_ERR_ARG, "unknown dtype %d", dtype);
  if (!x || !scale || !shift || !feat || C % 4 || C < 4 || HW < 1)
    return fail(FSVIT_ERR_ARG, "fsvit_pool_affine: null argument, C %% 4 != 0 or HW < 1 (the mean over no positions divides by zero)");
  RC_TRY(K(launch_pool_affine)(x, scale, shift, feat, B, HW, C, kd(dtype), (hipStream_t)stream));
  return 0;
}

// ------------------------------------------------------------------------------------ profiling
extern "C" const char* fsvit_kernel_name(int kernel_id, int dtype) {
  // one table, instantiated for the element type as the compiler spells it
#define FSVIT_KERNEL_NAMES(T)                                                                                                                              \
  {"gemm256_kernel", "conv_gemm_v2_kernel<" T ",128,64,2,2,3>", "conv_gemm_v2_kernel<" T ",128,32,4,1,3>", "im2col27_kernel<" T ">", "maxpool2_pos_kernel<" T ">", \
   "attention_v2_kernel<" T ",...>", "pool_affine_kernel<" T ">", "proto_head_kernel", "stage1_block_kernel", "conv_gemm_v2_kernel<" T ",128,128,2,2,2>",          \
   "patchify_kernel<" T ">", "layernorm_kernel<" T ">", "conv3x3_halo_kernel", "mlp_rows_kernel", "-", "qkv_attn_kernel", "stem_conv1_kernel",                   \
   "stage1_ring_kernel", "ln_gemm_rows_kernel", "qkv_attn_rows_kernel", "vit_attn_rows_kernel"}
  static const char* const names[3][21] = {FSVIT_KERNEL_NAMES("float"), FSVIT_KERNEL_NAMES("__bf16"), FSVIT_KERNEL_NAMES("_Float16")};
#undef FSVIT_KERNEL_NAMES
  static const char* x2n[] = {"gemm256_x2_kernel", "conv_gemm_v2_kernel<f32x2l,128,64,2,2,3>", "conv_gemm_v2_kernel<f32x2l,128,32,4,1,3>", "", "", "", "", "", "", "conv_gemm_v2_kernel<f32x2l,128,128,2,2,2>"};
  if (kernel_id < 0 || kernel_id > 20) return "?";
  if (kernel_id == KID_STAGE1RING && kd(dtype) == 1) return "stage1_w4_kernel";      // (launch_stage1_ring forwards to stage1_w4.hip)
  if (is_x2(dtype)) return kernel_id == 14 ? "gconv3x3_x2_kernel" : (kernel_id == 0 || kernel_id == 1 || kernel_id == 2 || kernel_id == 9) ? x2n[kernel_id] : names[0][kernel_id];
  return names[dtype == FSVIT_F32 ? 0 : dtype == FSVIT_F16 ? 2 : 1][kernel_id];
}

extern "C" int fsvit_encoder_profile_begin(void* hv) {
  EngineBase* h = static_cast<EngineBase*>(hv);
  if (!h) return fail(FSVIT_ERR_ARG, "null argument");
  h->prof.clear();
  h->prof_last = nullptr;
  h->profiling = true;
  return 0;
}

extern "C" int fsvit_encoder_profile_end(void* hv, fsvit_prof_rec* out, int max_recs, int* n_out) {
  EngineBase* h = static_cast<EngineBase*>(hv);
  if (!h || !out || !n_out) return fail(FSVIT_ERR_ARG, "null argument");
  h->profiling = false;
  std::vector<fsvit_prof_rec> agg;
  hipEvent_t freed = nullptr;
  for (ProfEntry& e : h->prof) {
    HIP_TRY(hipEventSynchronize(e.e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e.e0, e.e1));
    size_t k = 0;
    for (; k < agg.size(); ++k)
      if (e.layer == agg[k].layer && e.kernel == agg[k].kernel_id) break;
    if (k == agg.size()) {
      fsvit_prof_rec r;
      memset(&r, 0, sizeof(r));
      snprintf(r.layer, sizeof(r.layer), "%s", e.layer.c_str());
      r.kernel_id = e.kernel;
      agg.push_back(r);
    }
    agg[k].flops += e.flops;
    agg[k].ms += ms;
    agg[k].launches += 1;
  }
  // events are shared between neighbours (e1 of launch i is e0 of launch i+1 inside a chunk)
  for (ProfEntry& e : h->prof) {
    if (e.e0 != freed) (void)hipEventDestroy(e.e0);
    (void)hipEventDestroy(e.e1);
    freed = e.e1;
  }
  h->prof.clear();
  h->prof_last = nullptr;
  *n_out = (int)agg.size();
  if ((int)agg.size() > max_recs) return fail(FSVIT_ERR_ARG, "profile has %zu records, buffer holds %d", agg.size(), max_recs);
  for (size_t i = 0; i < agg.size(); ++i) out[i] = agg[i];
  return 0;
}

// ==================================================================================== ViT / DeiT encoder
// test_phase/models/deit.py:139-218.  LayerNorm gains/shifts are folded into the following Linear
// (W' = W diag(gamma), b' = b + W beta); the normalisation itself is a one-wave-per-token kernel.
struct VitBlock {
  Layer qkv, proj, fc1, fc2;
  void* mlp_img = nullptr;      // mlp_rows.hip: fragment-major image of proj | fc1 | fc2 (null: GEMM + LayerNorm launches)
  float* mlp_b1 = nullptr;
  void* qkv_img = nullptr;      // mlp_rows.hip ln_gemm_rows: fragment-major image of the qkv Linear (null: LayerNorm launch + GEMM)
  void* attn_img = nullptr;     // mlp_rows.hip vit_attn_rows: head-major image of the qkv Linear (norm1 + qkv + attention in one launch)
};

struct fsvit_vit : EngineBase {
  fsvit_vit_cfg cfg;
  int D = 0, S = 0, np = 0, npw = 0, Kp = 0, hd = 0, hdp = 0, hid = 0;
  Layer pe;
  float *pos_patch = nullptr;      // pos_embed[1:]  [np][D]
  float *cls_pos0 = nullptr;       // cls_token + pos_embed[0]  [D]
  float *ng = nullptr, *nb = nullptr;
  std::vector<VitBlock> blocks;
};

namespace {

std::vector<double> add_vec(const std::vector<double>& a, const float* b, int n) {
  std::vector<double> r(n);
  for (int i = 0; i < n; ++i) r[i] = a[i] + (double)b[i];
  return r;
}

// Packs blocks.<i>.* (i < depth) of a pre-LN ViT encoder - DeiT (deit.py:62-77) and LV-ViT (lvvit.py:140-155) - into `blocks`.  LayerNorm gains /
// shifts are folded into the following Linear.  qkv_bias = false: the qkv Linear has no bias of its own (LV-ViT), the packed bias is then the
// folded norm1 shift W beta alone.  res_scale != 1 multiplies both residual branches (LV-ViT's 1 / skip_lam): it is folded into the proj and fc2
// weights and biases, exact for a power of two in every storage format.
int pack_vit_blocks(EngineBase* h, const SD& sd, int depth, int D, int heads, int hd, int hdp, int hid, int S, bool qkv_bias, double res_scale,
                    std::vector<VitBlock>* blocks_out) {
  std::vector<VitBlock>& blocks = *blocks_out;
  std::vector<int> rowmap(3 * heads * hd), colmap(heads * hd);
  for (int x = 0; x < 3; ++x)
    for (int y = 0; y < heads; ++y)
      for (int z = 0; z < hd; ++z) rowmap[(x * heads + y) * hd + z] = (x * heads + y) * hdp + z;
  for (int y = 0; y < heads; ++y)
    for (int z = 0; z < hd; ++z) colmap[y * hd + z] = y * hdp + z;
  const bool scaled = res_scale != 1.0;
  const std::vector<double> rs(D, res_scale);
  blocks.resize(depth);
  for (int i = 0; i < depth; ++i) {
    const std::string bp = "blocks." + std::to_string(i) + ".";
    const float* g1 = sd.get(bp + "norm1.weight", {D});
    const float* b1 = sd.get(bp + "norm1.bias", {D});
    const float* g2 = sd.get(bp + "norm2.weight", {D});
    const float* b2 = sd.get(bp + "norm2.bias", {D});
    const float* wq = sd.get(bp + "attn.qkv.weight", {3 * heads * hd, D});
    const float* bq = qkv_bias ? sd.get(bp + "attn.qkv.bias", {3 * heads * hd}) : nullptr;
    const float* wp = sd.get(bp + "attn.proj.weight", {D, heads * hd});
    const float* bpj = sd.get(bp + "attn.proj.bias", {D});
    const float* w1 = sd.get(bp + "mlp.fc1.weight", {hid, D});
    const float* bf1 = sd.get(bp + "mlp.fc1.bias", {hid});
    const float* w2 = sd.get(bp + "mlp.fc2.weight", {D, hid});
    const float* bf2 = sd.get(bp + "mlp.fc2.bias", {D});
    if (!g1 || !b1 || !g2 || !b2 || !wq || (qkv_bias && !bq) || !wp || !bpj || !w1 || !bf1 || !w2 || !bf2) return FSVIT_ERR_KEY;
    std::vector<double> s1(g1, g1 + D), t1(b1, b1 + D), s2(g2, g2 + D), t2(b2, b2 + D);
    std::vector<double> vbp(bpj, bpj + D), vb2(bf2, bf2 + D);
    if (scaled)
      for (int o = 0; o < D; ++o) { vbp[o] *= res_scale; vb2[o] *= res_scale; }
    const std::vector<double> bqkv = qkv_bias ? add_vec(prenorm_bias(wq, 3 * heads * hd, D, t1), bq, 3 * heads * hd) : prenorm_bias(wq, 3 * heads * hd, D, t1);
    RC_TRY(pack_layer(h, &blocks[i].qkv, wq, 3 * heads * hd, D, 1, 1, 1, nullptr, &s1, bqkv, true, &rowmap, 3 * heads * hdp, nullptr, 0));
    RC_TRY(pack_layer(h, &blocks[i].proj, wp, D, heads * hd, 1, 1, 1, scaled ? &rs : nullptr, nullptr, vbp, true, nullptr, 0, &colmap, heads * hdp));
    RC_TRY(pack_layer(h, &blocks[i].fc1, w1, hid, D, 1, 1, 1, nullptr, &s2, add_vec(prenorm_bias(w1, hid, D, t2), bf1, hid), true, nullptr, 0, nullptr, 0));
    RC_TRY(pack_layer(h, &blocks[i].fc2, w2, D, hid, 1, 1, 1, scaled ? &rs : nullptr, nullptr, vb2, true, nullptr, 0, nullptr, 0));
    const int kdt = h->dtype;
    VitBlock& b = blocks[i];
    if (K(mlp_rows_ln_supported)(kd(kdt), D, hid, heads * hdp)) {      // proj + residual + norm2 + Mlp in one row-wise kernel
      void* b1i = nullptr;
      RC_TRY(packed_image(h, K(mlp_rows_image_bytes)(D, hid, heads * hdp), &b.mlp_img, [&](void* img) {
        HIP_TRY(hipMalloc(&b1i, (size_t)hid * 4));
        h->allocs.push_back(b1i);
        return K(launch_mlp_pack)(b.fc1.w, b.fc1.Kw, b.fc1.bias, b.fc2.w, b.fc2.Kw, b.proj.w, b.proj.Kw, heads * hdp, img, (float*)b1i, D, hid, nullptr);
      }));
      b.mlp_b1 = (float*)b1i;
    }
    if (K(ln_gemm_rows_supported)(kd(kdt), D, 3 * heads * hdp))          // norm1 + qkv in one row-wise kernel
      RC_TRY(packed_image(h, K(ln_gemm_rows_image_bytes)(D, 3 * heads * hdp), &b.qkv_img,
                          [&](void* img) { return K(launch_ln_gemm_pack)(b.qkv.w, b.qkv.Kw, img, D, 3 * heads * hdp, nullptr); }));
    if (K(vit_attn_rows_supported)(kd(kdt), D, heads, hdp, S))        // norm1 + qkv + attention core in one launch: the qkv tensor never reaches HBM
      RC_TRY(packed_image(h, K(ln_gemm_rows_image_bytes)(D, 3 * heads * hdp), &b.attn_img,
                          [&](void* img) { return K(launch_qkv_attn_rows_pack)(b.qkv.w, b.qkv.Kw, img, D, heads, hdp, nullptr); }));
  }
  return 0;
}

// The token constants of a ViT handle H (fsvit_vit / fsvit_lvvit): pos_embed[1:] -> pos_patch [np][D], cls_token + pos_embed[0] -> cls_pos0 [D], the final
// LayerNorm's gain / shift -> ng / nb
template <class H>
int upload_token_consts(H* h, const float* cls, const float* pos, const float* g, const float* bt) {
  const int D = h->D;
  std::vector<float> pp((size_t)h->np * D), c0(D), gg(g, g + D), bb(bt, bt + D);
  for (int i = 0; i < h->np; ++i)
    for (int d = 0; d < D; ++d) pp[(size_t)i * D + d] = pos[(size_t)(i + 1) * D + d];
  for (int d = 0; d < D; ++d) c0[d] = cls[d] + pos[d];
  void* dv;
  RC_TRY(upload(h, pp, false, &dv)); h->pos_patch = (float*)dv;
  RC_TRY(upload(h, c0, false, &dv)); h->cls_pos0 = (float*)dv;
  RC_TRY(upload(h, gg, false, &dv)); h->ng = (float*)dv;
  RC_TRY(upload(h, bb, false, &dv)); h->nb = (float*)dv;
  return 0;
}

int build_vit(fsvit_vit* h, const SD& sd) {
  const fsvit_vit_cfg& cf = h->cfg;
  const int kch = 64 / h->es;
  const int D = cf.embed_dim, p = cf.patch_size, heads = cf.num_heads;
  if (cf.img_size % p || D % heads || D % 8) return fail(FSVIT_ERR_ARG, "unsupported ViT geometry");
  h->D = h->out_dim = D; h->npw = cf.img_size / p; h->np = h->npw * h->npw; h->S = h->np + 1;
  h->hd = D / heads; h->hdp = round_up(h->hd, kch); h->hid = (int)(D * cf.mlp_ratio);
  if (h->hid % 8) return fail(FSVIT_ERR_ARG, "hidden width must be a multiple of 8");
  if (h->S > (h->es == 4 ? 208 : 224)) return fail(FSVIT_ERR_ARG, "attention supports at most %d tokens", h->es == 4 ? 208 : 224);
  const int K = 3 * p * p;
  h->Kp = round_up(K, 8);
  {
    const float* w = sd.get("patch_embed.proj.weight", {D, 3, p, p});
    const float* b = sd.get("patch_embed.proj.bias", {D});
    const float* cls = sd.get("cls_token", {1, 1, D});
    const float* pos = sd.get("pos_embed", {1, h->S, D});
    const float* g = sd.get("norm.weight", {D});
    const float* bt = sd.get("norm.bias", {D});
    if (!w || !b || !cls || !pos || !g || !bt) return FSVIT_ERR_KEY;
    std::vector<int> cm(K);
    for (int k = 0; k < K; ++k) cm[k] = k;                       // conv weight [D][3][p][p] is already (c, py, px)-major
    std::vector<double> bias(D);
    for (int i = 0; i < D; ++i) bias[i] = b[i];
    RC_TRY(pack_layer(h, &h->pe, w, D, K, 1, 1, 1, nullptr, nullptr, bias, true, nullptr, 0, &cm, h->Kp));
    RC_TRY(upload_token_consts(h, cls, pos, g, bt));
  }
  return pack_vit_blocks(h, sd, cf.depth, D, heads, h->hd, h->hdp, h->hid, h->S, true, 1.0, &h->blocks);
}

struct VitPlan { void *patches, *tokens, *xn, *qkv, *ctx, *hid; };

VitPlan vit_layout(const fsvit_vit* h, size_t Bc, Arena& a) {
  VitPlan p;
  const size_t es = h->es;
  p.tokens = a.take(Bc * h->S * h->D * es);
  p.xn = a.take(Bc * h->S * h->D * es);
  p.qkv = a.take(Bc * h->S * 3 * h->cfg.num_heads * h->hdp * es);
  p.ctx = a.take(Bc * h->S * h->cfg.num_heads * h->hdp * es);
  const size_t pb = Bc * h->np * h->Kp * es, hb = Bc * h->S * h->hid * es;      // patches are dead once the tokens exist
  p.patches = p.hid = a.take(pb > hb ? pb : hb);
  return p;
}

// The encoder blocks of a pre-LN ViT (DeiT, LV-ViT) on the token rows `tokens` [Bc * S][D], in place; taps blocks.<i>.
int vit_blocks_forward(EngineBase* h, const std::vector<VitBlock>& blocks, void* tokens, void* xn, void* qkv, void* ctx, void* hid, int Bc, int S,
                       int D, int heads, int hd, int hdp, int hidc, float eps, bool first, hipStream_t st) {
  const int kdt = h->dtype, dt = kd(kdt);
  const size_t es = h->es;
  const int M = Bc * S;
  const float scale = 1.0f / std::sqrt((float)hd);
  for (size_t i = 0; i < blocks.size(); ++i) {
    const VitBlock& b = blocks[i];
    if (b.attn_img) {
      RC_TRY(timed(h, st, "blocks.norm1+qkv+attn", KID_VITATTNROWS, 2.0 * M * 3.0 * D * D + 4.0 * Bc * heads * (double)S * S * hd, [&]() {
        return K(launch_vit_attn_rows)(tokens, ctx, b.attn_img, b.qkv.bias, Bc, S, D, heads, hdp, eps, scale, st);
      }));
    } else {
    if (b.qkv_img) {
      RC_TRY(timed(h, st, "blocks.norm1+qkv", KID_LNGEMM, 2.0 * M * 3.0 * D * D, [&]() {
        return K(launch_ln_gemm_rows)(tokens, qkv, b.qkv_img, b.qkv.bias, M, D, 3 * heads * hdp, eps, st);
      }));
    } else {
      RC_TRY(timed(h, st, "blocks.norm1", KID_LN, 0.0, [&]() { return K(launch_layernorm)(tokens, xn, M, D, eps, dt, st); }));
      RC_TRY(run_gemm(h, st, "blocks.attn.qkv", b.qkv, conv_params(b.qkv, xn, qkv, Bc, S, 1, D, D, 1, 1, 1, 0, 3 * heads * hdp, ACT_NONE, nullptr, 0, nullptr), 3.0 * D, D));
    }
    RC_TRY(timed(h, st, "blocks.attn.core", KID_ATTN, 4.0 * Bc * heads * (double)S * S * hd,
                 [&]() { return K(launch_attention)(qkv, ctx, Bc, S, heads, hdp, scale, is_x2(h->dtype) ? 2 : dt, st); }));
    }
    if (b.mlp_img) {
      RC_TRY(timed(h, st, "blocks.proj+norm2+mlp", KID_MLPROWS, 2.0 * M * ((double)heads * hd * D + 2.0 * D * hidc), [&]() {
        return K(launch_mlp_rows_ln)(tokens, tokens, b.mlp_img, b.mlp_b1, b.proj.bias, b.fc2.bias, ctx, heads * hdp, M, D, hidc, eps, st);
      }));
      RC_TRY(tap(h, "blocks." + std::to_string(i), tokens, (size_t)M * D * es, first, st));
      continue;
    }
    RC_TRY(run_gemm(h, st, "blocks.attn.proj", b.proj, conv_params(b.proj, ctx, tokens, Bc, S, 1, heads * hdp, heads * hdp, 1, 1, 1, 0, D, ACT_NONE, tokens, 0, nullptr), D, D));
    RC_TRY(timed(h, st, "blocks.norm2", KID_LN, 0.0, [&]() { return K(launch_layernorm)(tokens, xn, M, D, eps, dt, st); }));
    RC_TRY(run_gemm(h, st, "blocks.mlp.fc1", b.fc1, conv_params(b.fc1, xn, hid, Bc, S, 1, D, D, 1, 1, 1, 0, hidc, ACT_GELU, nullptr, 0, nullptr), hidc, D));
    RC_TRY(run_gemm(h, st, "blocks.mlp.fc2", b.fc2, conv_params(b.fc2, hid, tokens, Bc, S, 1, hidc, hidc, 1, 1, 1, 0, D, ACT_NONE, tokens, 0, nullptr), D, hidc));
    RC_TRY(tap(h, "blocks." + std::to_string(i), tokens, (size_t)M * D * es, first, st));
  }
  return 0;
}

size_t vit_plan_bytes(const EngineBase* h, size_t Bc) { return layout_bytes(vit_layout, h, Bc); }

int vit_forward_chunk(EngineBase* hb, const float* x, int Bc, float* feat, unsigned char* ws, bool first, hipStream_t st) {
  fsvit_vit* h = static_cast<fsvit_vit*>(hb);
  Arena arena = chunk_arena(ws);
  const VitPlan pl = vit_layout(h, Bc, arena);
  const int kdt = h->dtype, dt = kd(kdt), D = h->D, S = h->S, heads = h->cfg.num_heads, hdp = h->hdp;
  const size_t es = h->es;
  void *patches = pl.patches, *tokens = pl.tokens, *xn = pl.xn, *qkv = pl.qkv, *ctx = pl.ctx, *hid = pl.hid;
  const int M = Bc * S;
  h->prof_last = nullptr;
  RC_TRY(timed(h, st, "patch_embed.patchify", KID_PATCHIFY, 0.0, [&]() { return K(launch_patchify)(x, patches, Bc, h->cfg.img_size, h->cfg.patch_size, h->Kp, dt, st); }));
  {
    ConvGemmParams p = conv_params(h->pe, patches, tokens, Bc, h->npw, h->npw, h->Kp, h->Kp, 1, 1, 1, 0, D, ACT_NONE, nullptr, 0, h->pos_patch);
    p.y_rpi = S; p.y_row0 = 1;                                   // patch token i of image b -> row b*S + 1 + i
    RC_TRY(run_gemm(h, st, "patch_embed.proj", h->pe, p, D, 3.0 * h->cfg.patch_size * h->cfg.patch_size));
  }
  RC_TRY(timed(h, st, "cls_token", KID_PATCHIFY, 0.0, [&]() { return K(launch_cls_pos)(h->cls_pos0, tokens, Bc, S, D, dt, st); }));
  RC_TRY(tap(h, "embed", tokens, (size_t)M * D * es, first, st));
  RC_TRY(vit_blocks_forward(h, h->blocks, tokens, xn, qkv, ctx, hid, Bc, S, D, heads, h->hd, hdp, h->hid, h->cfg.ln_eps, first, st));
  RC_TRY(timed(h, st, "norm.cls", KID_LN, 0.0, [&]() { return K(launch_final_ln_cls)(tokens, h->ng, h->nb, feat, Bc, S, D, h->cfg.ln_eps, dt, st); }));
  return 0;
}

}  // namespace

extern "C" int fsvit_vit_create(const fsvit_vit_cfg* cfg, const fsvit_tensor* state_dict, int n_tensors, int dtype, fsvit_vit** out) {
  const bool bad = cfg && (cfg->num_heads < 1 || cfg->embed_dim < 8 || cfg->depth < 0 || cfg->patch_size < 1);
  return encoder_create(cfg, state_dict, n_tensors, dtype, out, bad, "bad ViT configuration", KIND_VIT, build_vit, vit_plan_bytes, vit_forward_chunk, SIZE_FMT_VIT);
}
extern "C" void fsvit_vit_destroy(fsvit_vit* h) { encoder_destroy(h); }
extern "C" int fsvit_vit_out_dim(const fsvit_vit* h) { return h ? h->out_dim : 0; }
extern "C" size_t fsvit_vit_workspace_bytes(const fsvit_vit* h, int chunk_images) { return encoder_workspace_bytes(h, chunk_images); }
extern "C" int fsvit_vit_forward(fsvit_vit* h, const float* x, int n_img, int img_h, int img_w, float* feat, void* ws,
                                 size_t ws_bytes, void* stream) {
  return encoder_forward(h, x, n_img, img_h, img_w, feat, ws, ws_bytes, stream);
}

// ==================================================================================== LV-ViT encoder
// meta_tuning_sun_m/models/lvvit.py:277-318, :413-546 (factory lvvit_micro_80, :583).  The stem is the Visformer ConvBlock at stem_channels
// (conv1 s2 | conv2 | conv3 + downsample identity, eval BatchNorm folded, LeakyReLU(0.1), MaxPool2d(2)) followed by a 4 x 4 / stride 4 Conv2d
// projection to embed_dim; cls token + pos_embed; pre-LN blocks with skip_lam; features = norm(x)[:, 0].
// Stem (EvalStem): im2col27 + a K = 32 GEMM for conv1; conv2 and conv3 (+ downsample as the tail K slice over the same im2col rows + LeakyReLU +
// MaxPool2d) on the dedicated conv3x3_halo instantiation in bf16 / f16 at 96 channels (STEM_HALO_NHWC), on conv_gemm_v2 otherwise (a 96-channel map is
// no power of two: the tap is found per K chunk by division); the projection is the same implicit GEMM as a 4 x 4 / stride 4 conv over the pooled
// NHWC map of a slice, writing token rows 1..np of every image with bias + pos_embed[1:].
struct fsvit_lvvit : EngineBase {
  fsvit_lvvit_cfg cfg;
  int C0 = 0, D = 0, H1 = 0, npw = 0, np = 0, S = 0, hd = 0, hdp = 0, hid = 0;
  EvalStem stem;
  Layer pe;
  float *pos_patch = nullptr, *cls_pos0 = nullptr, *ng = nullptr, *nb = nullptr;
  std::vector<VitBlock> blocks;
  float* map_out = nullptr;    // fsvit_lvvit_forward_map: where the next chunk's patch rows [Bc][S - 1][D] go (advanced chunk by chunk); null: cls feature only
};

namespace {

int build_lvvit(fsvit_lvvit* h, const SD& sd) {
  const fsvit_lvvit_cfg& cf = h->cfg;
  const int kch = 64 / h->es;
  const int C0 = cf.stem_channels, D = cf.embed_dim, heads = cf.num_heads;
  if (cf.img_size % 16) return fail(FSVIT_ERR_ARG, "img_size %d must be a multiple of 16", cf.img_size);
  if (C0 % 32) return fail(FSVIT_ERR_ARG, "stem_channels %d must be a multiple of 32", C0);
  if (D % heads || D % 32) return fail(FSVIT_ERR_ARG, "unsupported LV-ViT geometry");
  if (!(cf.skip_lam > 0.0f)) return fail(FSVIT_ERR_ARG, "skip_lam must be positive");
  h->C0 = C0; h->D = h->out_dim = D;
  h->H1 = cf.img_size / 4; h->npw = h->H1 / 4; h->np = h->npw * h->npw; h->S = h->np + 1;
  h->hd = D / heads; h->hdp = round_up(h->hd, kch); h->hid = (int)(D * cf.mlp_ratio);
  if (h->hid % 32) return fail(FSVIT_ERR_ARG, "hidden width must be a multiple of 32");
  if (h->S > (h->es == 4 ? 208 : 224)) return fail(FSVIT_ERR_ARG, "attention supports at most %d tokens", h->es == 4 ? 208 : 224);
  {   // ---- stem (no position table, no weight-rounding correction, conv1 always im2col27 + GEMM, every route sliced) and the 4 x 4 projection
    const float* wp = sd.get("patch_embed.proj.weight", {D, C0, 4, 4});
    const float* bp = sd.get("patch_embed.proj.bias", {D});
    if (!wp || !bp) return FSVIT_ERR_KEY;
    RC_TRY(pack_stem(h, sd, "patch_embed.", C0, C0, cf.img_size, cf.bn_eps, nullptr, nullptr, false, stem_slice_images(), &h->stem));
    std::vector<double> bias(bp, bp + D);
    RC_TRY(pack_layer(h, &h->pe, wp, D, C0, 4, 4, 1, nullptr, nullptr, bias, true, nullptr, 0, nullptr, 0));   // K = (ky, kx, c): 16 taps of C0
  }
  {
    const float* cls = sd.get("cls_token", {1, 1, D});
    const float* pos = sd.get("pos_embed", {1, h->S, D});
    const float* g = sd.get("norm.weight", {D});
    const float* bt = sd.get("norm.bias", {D});
    if (!cls || !pos || !g || !bt) return FSVIT_ERR_KEY;
    RC_TRY(upload_token_consts(h, cls, pos, g, bt));
  }
  return pack_vit_blocks(h, sd, cf.depth, D, heads, h->hd, h->hdp, h->hid, h->S, false, 1.0 / (double)cf.skip_lam, &h->blocks);
}

// Workspace of a chunk of Bc images: the token rows, then ONE region shared by the stem scratch of a slice (im2col rows, conv1 / conv2 maps and
// the pooled map) and the block scratch of the whole chunk.
struct LvvitPlan { void* tokens; StemScratch stem; void *xn, *qkv, *ctx, *hid; };

LvvitPlan lvvit_layout(const fsvit_lvvit* h, size_t Bc, Arena& a) {
  LvvitPlan p;
  const size_t es = h->es, heads = h->cfg.num_heads;
  p.tokens = a.take(Bc * h->S * h->D * es);
  const size_t scratch0 = a.mark();
  p.stem = stem_scratch(h->stem, es, Bc, true, a);
  a.rewind(scratch0);
  p.xn = a.take(Bc * h->S * h->D * es);
  p.qkv = a.take(Bc * h->S * 3 * heads * h->hdp * es);
  p.ctx = a.take(Bc * h->S * heads * h->hdp * es);
  p.hid = a.take(Bc * h->S * h->hid * es);
  return p;
}

size_t lvvit_plan_bytes(const EngineBase* h, size_t Bc) { return layout_bytes(lvvit_layout, h, Bc); }

int lvvit_forward_chunk(EngineBase* hb, const float* x, int Bc, float* feat, unsigned char* ws, bool first, hipStream_t st) {
  fsvit_lvvit* h = static_cast<fsvit_lvvit*>(hb);
  Arena arena = chunk_arena(ws);
  const LvvitPlan pl = lvvit_layout(h, Bc, arena);
  const int kdt = h->dtype, dt = kd(kdt), D = h->D, S = h->S, C0 = h->C0, heads = h->cfg.num_heads;
  const size_t es = h->es;
  void* tokens = pl.tokens;
  h->prof_last = nullptr;
  // stem: every slice pools into the slice's own map, which the 4 x 4 projection turns into the token rows of its images
  RC_TRY(stem_forward(h, h->stem, pl.stem, ImageSrc{x, nullptr, Bc, (size_t)3 * h->stem.img * h->stem.img}, Bc, st, [&](int) { return pl.stem.pooled; },
                      [&](int g0, int n, void* p1) {
    if (g0 == 0) RC_TRY(tap(h, "stem", p1, (size_t)n * h->H1 * h->H1 * C0 * es, first, st));
    ConvGemmParams pp = conv_params(h->pe, p1, (unsigned char*)tokens + (size_t)g0 * S * D * es, n, h->H1, h->H1, C0, C0, 4, 4, 4, 0, D, ACT_NONE, nullptr, 0,
                                    h->pos_patch);
    pp.y_rpi = S; pp.y_row0 = 1;                                 // patch token i of image b -> row b*S + 1 + i
    return run_gemm(h, st, "patch_embed.proj", h->pe, pp, D, 16.0 * C0);
  }));
  RC_TRY(timed(h, st, "cls_token", KID_PATCHIFY, 0.0, [&]() { return K(launch_cls_pos)(h->cls_pos0, tokens, Bc, S, D, dt, st); }));
  RC_TRY(tap(h, "embed", tokens, (size_t)Bc * S * D * es, first, st));
  RC_TRY(vit_blocks_forward(h, h->blocks, tokens, pl.xn, pl.qkv, pl.ctx, pl.hid, Bc, S, D, heads, h->hd, h->hdp, h->hid,
                            h->cfg.ln_eps, first, st));
  if (h->map_out) {
    float* map = h->map_out;
    h->map_out += (size_t)Bc * (S - 1) * D;
    RC_TRY(timed(h, st, "norm.map", KID_LN, 0.0, [&]() { return K(launch_final_ln_map)(tokens, h->ng, h->nb, feat, map, Bc, S, D, h->cfg.ln_eps, dt, st); }));
    return 0;
  }
  RC_TRY(timed(h, st, "norm.cls", KID_LN, 0.0, [&]() { return K(launch_final_ln_cls)(tokens, h->ng, h->nb, feat, Bc, S, D, h->cfg.ln_eps, dt, st); }));
  return 0;
}

}  // namespace

extern "C" int fsvit_lvvit_create(const fsvit_lvvit_cfg* cfg, const fsvit_tensor* state_dict, int n_tensors, int dtype, fsvit_lvvit** out) {
  const bool bad = cfg && (cfg->num_heads < 1 || cfg->embed_dim < 32 || cfg->depth < 0 || cfg->stem_channels < 32);
  return encoder_create(cfg, state_dict, n_tensors, dtype, out, bad, "bad LV-ViT configuration", KIND_LVVIT, build_lvvit, lvvit_plan_bytes, lvvit_forward_chunk,
                        SIZE_FMT_VIT);
}
extern "C" void fsvit_lvvit_destroy(fsvit_lvvit* h) { encoder_destroy(h); }
extern "C" int fsvit_lvvit_out_dim(const fsvit_lvvit* h) { return h ? h->out_dim : 0; }
extern "C" size_t fsvit_lvvit_workspace_bytes(const fsvit_lvvit* h, int chunk_images) { return encoder_workspace_bytes(h, chunk_images); }
extern "C" int fsvit_lvvit_forward(fsvit_lvvit* h, const float* x, int n_img, int img_h, int img_w, float* feat, void* ws,
                                   size_t ws_bytes, void* stream) {
  return encoder_forward(h, x, n_img, img_h, img_w, feat, ws, ws_bytes, stream);
}
extern "C" int fsvit_lvvit_forward_map(fsvit_lvvit* h, const float* x, int n_img, int img_h, int img_w, float* feat, float* tokens, void* ws, size_t ws_bytes,
                                       void* stream) {
  if (h && n_img <= 0) return 0;
  if (!h || !tokens) return fail(FSVIT_ERR_ARG, "null argument");
  h->map_out = tokens;                   // every chunk writes its images' rows and moves this on
  const int rc = encoder_forward(h, x, n_img, img_h, img_w, feat, ws, ws_bytes, stream);
  h->map_out = nullptr;
  return rc;
}
