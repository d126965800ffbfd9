"""Float64 references of the fused inference row kernels (mlp_rows.hip, qkv_attn.hip, stem.hip), one pair per operator entry point.

Every function takes float64 tensors that the caller has ALREADY rounded to the storage type (bf16 or fp16), and comes in two forms:

* `NAME_exact(...)`: the operator's mathematics with no intermediate rounding - erf GELU, LayerNorm with the population variance and the given eps,
  softmax(scale q k^T) v.
* `NAME_points(..., dtype)` -> Points(pre, out, acc): the same with the kernel's own rounding points applied (round to `dtype`, back to float64), taken from
  the kernel sources:
    - proj prologue of mlp_rows_kernel: x1 = T(x + Wp ctx [+ bp]) is what the Mlp (and the residual) continue from;
    - mr_layernorm_rows: the normalised row T((x - mean) rstd) is the GEMM operand;
    - mlp_pack_kernel stores T(W1 / 8) and T(8 W2) (exact in bf16; in fp16 W1 / 8 is subnormal below 2^-11), the kernel carries the hidden map at 1/8
      scale: hp = T(GELU(z) / 8);
    - the GELU itself: bf16 build = the gelu_tab look-up, T(gelu_erf(z') / 8) on the bf16-rounded pre-activation z' = 8 T(z / 8) with |z'| held to the
      table's range [2^-10, 32); fp16 build = gelu_sig (x sigmoid(x poly(x^2)), coefficients of fsvit_common.h) on the unrounded pre-activation;
    - attention (qkv_attn_kernel, qkv_attn_rows_kernel, vit_attn_rows_kernel): q, k, v = T(W x + b); the scores stay fp32; the un-normalised
      probabilities exp(scale (s - max)) are rounded to T as the operand of P V while their row sum is taken from the unrounded values; the output is
      T((P V) / sum);
    - every operator: the stored output, `out` = T(`pre`).
  `acc` is the fp32 accumulation allowance of the LAST accumulation chain of the operator, K 2^-24 sum |terms| with K the chain's length, from the
  reference's own operands.
  `sig` (attention only, else None) is the standard deviation of `pre - exact` PER ELEMENT, from first-order propagation of the rounding points above
  taken as independent errors of variance (u |value|)^2 / 3 (a rounding error is uniform within half an ulp <= u |value|).  The rounding effect of the
  attention operators is not one population: d out_c / d s_j = scale p_j (v_jc - out_c), so a query with a large |q| or a peaked softmax over unlike
  values carries a several times larger error than the case's RMS, and a cap of 6 RMS does not hold for it while 6 of its own deviation does.

Padded head dims (zero weight rows, zero bias) come out exactly 0 in both forms.  tests/test_rows_ops_ref_cpu.py proves the exact forms against
torch.nn.functional and holds the points forms inside the gates of tests/test_gpu_rows_ops.py; that file holds the kernels to both.
"""
import collections
import math

import torch
import torch.nn.functional as F

from .train_ops_oracle import gelu_sig, rounder

Points = collections.namedtuple('Points', 'pre out acc sig', defaults=(None,))
EPS24 = 2.0 ** -24


def half_ulp(dtype):
    """u: half an ulp, relative (2^-11 for fp16, 2^-8 for bf16; 2^-24 for the fp32 rows of the stand-alone attention kernels)"""
    return {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}[dtype]


def gelu_erf(z):
    return 0.5 * z * (1.0 + torch.erf(z * math.sqrt(0.5)))


def layernorm(x, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps)


def _hidden_points(z, rnd, dtype):
    """pre-activation z (float64, what the fp32 accumulator holds times 8) -> the hidden map GEMM2 multiplies, 8 T(GELU / 8)"""
    if dtype == torch.bfloat16:      # gelu_tab: the bf16 code of z / 8 indexes a table of T(gelu_erf(z) / 8); magnitudes below 2^-10 share the first entry
        zr = 8.0 * rnd(z / 8.0)
        zr = torch.where(zr.abs() < 2.0 ** -10, torch.where(zr < 0, -1.0, 1.0).double() * 2.0 ** -10, zr)
        zr = zr.clamp(-31.875, 31.875)
        return 8.0 * rnd(gelu_erf(zr) / 8.0)
    return 8.0 * rnd(gelu_sig(z) / 8.0)


# ---------------------------------------------------------------------------------------------------------------- mlp_rows / proj_mlp_rows / vit_block_tail
def _mlp_exact(x, w1, b1, w2, b2, ctx, wp, bp, ln_eps):
    x1 = x if ctx is None else x + ctx @ wp.t() + (0.0 if bp is None else bp)
    h = gelu_erf((x1 if ln_eps is None else layernorm(x1, ln_eps)) @ w1.t() + b1)
    return x1 + h @ w2.t() + (0.0 if b2 is None else b2)


def _mlp_points(x, w1, b1, w2, b2, ctx, wp, bp, ln_eps, dtype):
    rnd = rounder(dtype)
    x1 = x if ctx is None else rnd(x + ctx @ wp.t() + (0.0 if bp is None else bp))
    xn = x1 if ln_eps is None else rnd(layernorm(x1, ln_eps))
    w1p, w2p = 8.0 * rnd(w1 / 8.0), rnd(8.0 * w2) / 8.0
    h = _hidden_points(xn @ w1p.t() + b1, rnd, dtype)
    pre = x1 + h @ w2p.t() + (0.0 if b2 is None else b2)
    acc = w1.shape[0] * EPS24 * (h.abs() @ w2p.abs().t() + x1.abs() + (0.0 if b2 is None else b2.abs()))
    return Points(pre, rnd(pre), acc)


def mlp_rows_exact(x, w1, b1, w2, b2=None):
    """y = x + W2 GELU(W1 x + b1) + b2"""
    return _mlp_exact(x, w1, b1, w2, b2, None, None, None, None)


def mlp_rows_points(x, w1, b1, w2, b2, dtype):
    return _mlp_points(x, w1, b1, w2, b2, None, None, None, None, dtype)


def proj_mlp_rows_exact(x, ctx, wp, w1, b1, w2, b2=None):
    """x1 = x + Wp ctx; y = x1 + W2 GELU(W1 x1 + b1) + b2"""
    return _mlp_exact(x, w1, b1, w2, b2, ctx, wp, None, None)


def proj_mlp_rows_points(x, ctx, wp, w1, b1, w2, b2, dtype):
    return _mlp_points(x, w1, b1, w2, b2, ctx, wp, None, None, dtype)


def vit_block_tail_exact(x, ctx, wp, bp, w1, b1, w2, b2, eps):
    """x1 = x + bp + Wp ctx; y = x1 + b2 + W2 GELU(W1 LN(x1) + b1), LN without affine"""
    return _mlp_exact(x, w1, b1, w2, b2, ctx, wp, bp, eps)


def vit_block_tail_points(x, ctx, wp, bp, w1, b1, w2, b2, eps, dtype):
    return _mlp_points(x, w1, b1, w2, b2, ctx, wp, bp, eps, dtype)


# ---------------------------------------------------------------------------------------------------------------- ln_linear_rows / patch_embed2x2 / stem_conv1
def ln_linear_rows_exact(x, w, b, eps=None):
    """y = b + W LN(x) (eps None: no LayerNorm, the C = 512 geometry)"""
    return (x if eps is None else layernorm(x, eps)) @ w.t() + (0.0 if b is None else b)


def ln_linear_rows_points(x, w, b, eps, dtype):
    rnd = rounder(dtype)
    xn = x if eps is None else rnd(layernorm(x, eps))
    pre = xn @ w.t() + (0.0 if b is None else b)
    acc = x.shape[-1] * EPS24 * (xn.abs() @ w.abs().t() + (0.0 if b is None else b.abs()))
    return Points(pre, rnd(pre), acc)


def patch_rows(x):
    """x NHWC [B, H, H, Ci] -> the rows of the 2 x 2 / stride-2 patches [B (H/2)^2, 4 Ci], k = (ky, kx, c)"""
    B, H, _, Ci = x.shape
    return x.reshape(B, H // 2, 2, H // 2, 2, Ci).permute(0, 1, 3, 2, 4, 5).reshape(B * (H // 2) ** 2, 4 * Ci)


def patch_embed2x2_exact(x, w, bias, pos):
    """x NHWC, w [N, 4 Ci] in (ky, kx, c) order, pos [(H/2)^2, N] -> y [B (H/2)^2, N] = bias + W patch + pos"""
    B = x.shape[0]
    return patch_rows(x) @ w.t() + (0.0 if bias is None else bias) + pos.repeat(B, 1)


def patch_embed2x2_points(x, w, bias, pos, dtype):
    rnd = rounder(dtype)
    pre = patch_embed2x2_exact(x, w, bias, pos)
    acc = w.shape[1] * EPS24 * (patch_rows(x).abs() @ w.abs().t() + (0.0 if bias is None else bias.abs()) + pos.abs().repeat(x.shape[0], 1))
    return Points(pre, rnd(pre), acc)


def im2col27(x):
    """x NCHW [B, 3, H, W] -> the rows of the 3 x 3 / stride-2 / pad-1 patches [B (H/2) (W/2), 27], k = (ky 3 + kx) 3 + c"""
    B, _, H, W = x.shape
    n = (H // 2) * (W // 2)
    return F.unfold(x, 3, padding=1, stride=2).view(B, 3, 9, n).permute(0, 3, 2, 1).reshape(B * n, 27)


def stem_conv1_exact(x, w, bias):
    """x NCHW (values of the storage type), w [64, 27] in (ky, kx, c) order -> c1 rows [B 1600, 64] = LeakyReLU_0.1(bias + W patch)"""
    return F.leaky_relu(im2col27(x) @ w.t() + (0.0 if bias is None else bias), 0.1)


def stem_conv1_points(x, w, bias, dtype):
    rnd = rounder(dtype)
    pre = stem_conv1_exact(x, w, bias)
    acc = 32 * EPS24 * (im2col27(x).abs() @ w.abs().t() + (0.0 if bias is None else bias.abs()))
    return Points(pre, rnd(pre), acc)


# ---------------------------------------------------------------------------------------------------------------- qkv + attention
def _split_heads(qkv, B, S, heads, hdp):
    qkv = qkv.reshape(B, S, 3, heads, hdp)
    return [qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3)]        # [B, heads, S, hdp]


def _attn_exact(x, w, bias, B, S, heads, hdp, scale, eps):
    xn = x if eps is None else layernorm(x, eps)
    q, k, v = _split_heads(xn @ w.t() + (0.0 if bias is None else bias), B, S, heads, hdp)
    p = (q @ k.transpose(-1, -2) * scale).softmax(-1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B * S, heads * hdp)


def _attn_points(x, w, bias, B, S, heads, hdp, scale, eps, dtype):
    rnd = rounder(dtype)
    xn = x if eps is None else rnd(layernorm(x, eps))
    q, k, v = _split_heads(rnd(xn @ w.t() + (0.0 if bias is None else bias)), B, S, heads, hdp)
    s = q @ k.transpose(-1, -2)
    e = torch.exp((s - s.max(-1, keepdim=True).values) * scale)
    l = e.sum(-1, keepdim=True)
    er = rnd(e)
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(B * S, heads * hdp)
    pre = flat((er @ v) / l)
    acc = S * EPS24 * flat((er @ v.abs()) / l)
    # per-element variance of the propagated rounding errors, in units of u^2 / 3: the variances of q, k, v (own rounding + the normalised row's through W) ...
    var = rnd(xn @ w.t() + (0.0 if bias is None else bias)) ** 2 + (0.0 if eps is None else (xn ** 2) @ (w ** 2).t())
    vq, vk, vv = _split_heads(var, B, S, heads, hdp)
    p, o = e / l, (e / l) @ v
    # ... of q through the scores: d out_c = scale sum_d dq_d G_cd, G_cd = sum_j p_j (v_jc - out_c) k_jd
    G = (p @ (v.unsqueeze(-1) * k.unsqueeze(-2)).flatten(-2)).unflatten(-1, (hdp, hdp)) - o.unsqueeze(-1) * (p @ k).unsqueeze(-2)
    t_q = scale ** 2 * (G ** 2 * vq.unsqueeze(-2)).sum(-1)
    # ... of k: scale^2 sum_j p_j^2 (v_jc - out_c)^2 sum_d q_d^2 var(k_jd)
    a = p ** 2 * ((q ** 2) @ vk.transpose(-1, -2))
    t_k = scale ** 2 * (a @ v ** 2 - 2.0 * o * (a @ v) + o ** 2 * a.sum(-1, keepdim=True))
    # ... of v, and of the rounded probabilities (their sum is taken unrounded): sum_j p_j^2 (var(v_jc) + v_jc^2)
    t_vp = p ** 2 @ (vv + v ** 2)
    sig = half_ulp(dtype) / math.sqrt(3.0) * flat((t_q + t_k + t_vp).clamp(min=0.0).sqrt())
    return Points(pre, rnd(pre), acc, sig)


def qkv_attention_exact(x, w, bias, B, S, heads, hdp, scale):
    """x [B S, C], w [3 heads hdp, C] (rows (q | k | v, head, channel), padded channels zero) -> ctx [B S, heads hdp]"""
    return _attn_exact(x, w, bias, B, S, heads, hdp, scale, None)


def qkv_attention_points(x, w, bias, B, S, heads, hdp, scale, dtype):
    return _attn_points(x, w, bias, B, S, heads, hdp, scale, None, dtype)


def vit_ln_qkv_attention_exact(x, w, bias, B, S, heads, hdp, scale, eps):
    """the same on LN(x) (no affine)"""
    return _attn_exact(x, w, bias, B, S, heads, hdp, scale, eps)


def vit_ln_qkv_attention_points(x, w, bias, B, S, heads, hdp, scale, eps, dtype):
    return _attn_points(x, w, bias, B, S, heads, hdp, scale, eps, dtype)
