"""Float64 references of the stand-alone attention kernels: attention.hip (forward: attention_v2_kernel, the generic attention_kernel) and
attention_bwd.hip (backward: the bf16 MFMA kernel, the exact-fp32 MFMA kernels, the FMA fallbacks).

Layout, as the kernels': qkv [B S, 3 heads hdp] with row = (q | k | v, head, channel), every head padded from hd to hdp channels with ZEROS;
ctx / dctx [B S, heads hdp]; dqkv as qkv = (dQ | dK | dV).  Every function takes float64 tensors the caller has already rounded to the storage type.

* forward_exact / backward_exact: the mathematics, no intermediate rounding:
    P = softmax(scale q k^T), ctx = P v;   dV = P^T dO, dP = dO V^T, D = rowsum(P o dP), dS = scale P o (dP - D), dQ = dS K, dK = dS^T Q.
* forward_points(..., kind) / backward_points(..., kind) -> Points(pre, out, acc, sig): the same with the roundings the kernel code shows.
    forward 'v2' (16-bit attention_v2_kernel): scores fp32; the UN-normalised e = exp(s - max) is rounded to the storage type as the MFMA operand of
        e V, the row sum is taken from the unrounded e; out = T((e V) / sum).
    forward 'v1' (16-bit attention_kernel): the NORMALISED p = e / sum is rounded to the storage type in LDS; out = T(p V).
    forward 'x2' (attention_v2_kernel<f32x2l>, fp32 storage): K, V (at staging), q and the un-normalised e (in registers) are each replaced by
        hi + lo, two limbs of the 16-bit type (x2_split of fsvit_common.h: bf16 hi = the upper 16 bits, lo = RNE(x - hi); fp16 hi = RTZ(x),
        lo = RTZ(x - hi)); all four limb products are accumulated, so every product is (hi + lo)(hi' + lo') in fp32.  The arithmetic between the
        splits is evaluated in float32 (torch on the CPU), not float64: the fp32 roundings are of the limbs' own size.
    forward / backward 'f32' (fp32 storage) and backward 'fma' (attention_bwd_kernel<bf16>): no intermediate rounding.
    backward 'mfma' (attention_bwd_mfma_kernel, bf16): S and dP are exact products accumulated in fp32; P and D stay fp32; dS is rounded to bf16 as
        the operand of BOTH dQ = dS K and dK = dS^T Q; P is rounded to bf16 as the operand of dV = P^T dO; outputs rounded.
  acc: the deterministic first-order fp32 allowance of the whole operator (fp32_allowance_* below) - every fp32 dot product, the hardware exp2 / rcp,
  propagated through the softmax, D and the output products.  It is the whole bound of the fp32-storage kernels and the `acc` term of the 16-bit gates.
  sig: the standard deviation of (pre - exact) PER ELEMENT, first-order, the roundings above taken as independent with second moment (u |value|)^2 / 3:
    forward 16-bit:  sig(ctx_ic) = u / sqrt 3 * sqrt(sum_j p_ij^2 v_jc^2)
    forward x2:      the same with u2 = u16^2 (bf16: 2^-16, fp16 RTZ: 2^-20) plus the splits of q and k through the scores,
                     d ctx_ic = scale sum_j p_ij (v_jc - ctx_ic) ds_ij, and of v
    backward mfma:   sig(dQ_id) = u / sqrt 3 * sqrt(sum_j dS_ij^2 k_jd^2),  sig(dK_jd) = ... sqrt(sum_i dS_ij^2 q_id^2),  sig(dV_jd) = ... sqrt(sum_i p_ij^2 dO_id^2)
Pad channels come out exactly 0 in every form.  tests/test_attention_ref_cpu.py proves the exact forms against torch.softmax / autograd in float64 and
holds every points form inside the gates of tests/attention_cases.py.
"""
import math

import torch

from .rows_ops_oracle import Points, half_ulp
from .train_ops_oracle import rounder

U = 2.0 ** -24          # half an ulp of fp32, relative
E20 = 2.0 ** -20        # the allowance tests/test_gpu_train_ops.py (test_elementwise) gives the hardware exp2 / rcp and expf


def sum_tol(abs_terms_sum, depth):
    """tests/test_gpu_train_ops.py sum_tol: an fp32 chain of `depth` terms, 4 / sqrt(depth) of its worst case"""
    return 4.0 * math.sqrt(depth) * U * abs_terms_sum


def _dot_allow(abs_terms_sum, depth):
    """an fp32 dot product: the accumulation chain + the rounding of each fp32 x fp32 product (exact for 16-bit operands; kept for all)"""
    return sum_tol(abs_terms_sum, depth) + U * abs_terms_sum


def split_heads(qkv, B, S, heads, hdp):
    """[B S, 3 heads hdp] -> q, k, v [B, heads, S, hdp]"""
    t = qkv.reshape(B, S, 3, heads, hdp)
    return [t[:, :, i].permute(0, 2, 1, 3) for i in range(3)]


def heads_of(ctx, B, S, heads, hdp):
    """[B S, heads hdp] -> [B, heads, S, hdp]"""
    return ctx.reshape(B, S, heads, hdp).permute(0, 2, 1, 3)


def flat(t):
    """[B, heads, S, hdp] -> [B S, heads hdp]"""
    B, heads, S, hdp = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * S, heads * hdp)


def flat3(dq, dk, dv):
    """three [B, heads, S, hdp] -> [B S, 3 heads hdp]"""
    B, heads, S, hdp = dq.shape
    return torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(B * S, 3 * heads * hdp)


def _softmax(q, k, scale):
    s = q @ k.transpose(-1, -2) * scale
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    return s, m, e, l


# ------------------------------------------------------------------------------------------------------------------------------- exact forms
def forward_exact(qkv, B, S, heads, hdp, scale):
    q, k, v = split_heads(qkv, B, S, heads, hdp)
    _, _, e, l = _softmax(q, k, scale)
    return flat((e / l) @ v)


def _backward(q, k, v, do, scale, rnd_ds=None, rnd_p=None):
    _, _, e, l = _softmax(q, k, scale)
    p = e / l
    dp = do @ v.transpose(-1, -2)
    D = (p * dp).sum(-1, keepdim=True)
    ds = scale * p * (dp - D)
    dsr = ds if rnd_ds is None else rnd_ds(ds)
    pr = p if rnd_p is None else rnd_p(p)
    return dsr @ k, dsr.transpose(-1, -2) @ q, pr.transpose(-1, -2) @ do, p, dp, D, ds


def backward_exact(qkv, dctx, B, S, heads, hdp, scale):
    q, k, v = split_heads(qkv, B, S, heads, hdp)
    dq, dk, dv = _backward(q, k, v, heads_of(dctx, B, S, heads, hdp), scale)[:3]
    return flat3(dq, dk, dv)


# ------------------------------------------------------------------------------------------------------------------------------- fp32 allowances
def _rel_e(q, k, s, m, scale, hdp):
    """bound of the relative error of e_ij = exp(s_ij - m_i) as the kernels form it: the fp32 score (dot product, the scale multiply, the subtraction
    of the row maximum - whose own error is common to the row and cancels in e / sum) and the exponential"""
    a_s = scale * _dot_allow(q.abs() @ k.abs().transpose(-1, -2), hdp) + 2.0 * U * (s.abs() + m.abs())
    return a_s + E20


def _gamma(S):
    """relative error of 1 / sum beyond that of its terms: the chain of S positive terms, the reciprocal, the multiply"""
    return 4.0 * math.sqrt(S) * U + E20 + 2.0 * U


def fp32_allowance_forward(qkv, B, S, heads, hdp, scale):
    """|ctx_kernel - ctx_exact| <= this (first order), for a kernel that rounds nothing but fp32 arithmetic.  d ctx_ic = sum_j p_ij eps_ij (v_jc - ctx_ic)
    + gamma ctx_ic, |eps_ij| <= rel_e_ij; the product p v is a chain over the keys (padded to at most S + 31)."""
    q, k, v = split_heads(qkv, B, S, heads, hdp)
    s, m, e, l = _softmax(q, k, scale)
    p = e / l
    o = p @ v
    w = p * _rel_e(q, k, s, m, scale, hdp)
    a = torch.stack([torch.stack([(w[b, h].unsqueeze(-1) * (v[b, h].unsqueeze(0) - o[b, h].unsqueeze(1)).abs()).sum(1) for h in range(heads)]) for b in range(B)])
    return flat(a + _gamma(S) * o.abs() + _dot_allow(p @ v.abs(), S + 31) + 2.0 * U * o.abs())


def fp32_allowance_backward(qkv, dctx, B, S, heads, hdp, scale):
    """|dqkv_kernel - dqkv_exact| <= this (first order).  With ap_ij >= |dp_ij| (softmax: p_ij (eps_ij - sum_j' p_ij' eps_ij' + gamma)):
         a_dP = dot(|dO| |v|),  a_D = sum_j (ap |dP| + p a_dP) + dot(sum_j p |dP|),  a_dS = scale (ap |dP - D| + p (a_dP + a_D)) + 3 u |dS|,
         a_dQ = a_dS |K| + dot(|dS| |K|),  a_dK = a_dS^T |Q| + dot(|dS|^T |Q|),  a_dV = ap^T |dO| + dot(p^T |dO|)."""
    q, k, v = split_heads(qkv, B, S, heads, hdp)
    do = heads_of(dctx, B, S, heads, hdp)
    s, m, e, l = _softmax(q, k, scale)
    _, _, _, p, dp, D, ds = _backward(q, k, v, do, scale)
    re = _rel_e(q, k, s, m, scale, hdp)
    ap = p * (re + (p * re).sum(-1, keepdim=True) + _gamma(S))
    a_dp = _dot_allow(do.abs() @ v.abs().transpose(-1, -2), hdp)
    pdp = (p * dp.abs()).sum(-1, keepdim=True)
    a_D = (ap * dp.abs() + p * a_dp).sum(-1, keepdim=True) + _dot_allow(pdp, S + 15)
    a_ds = scale * (ap * (dp - D).abs() + p * (a_dp + a_D + U * (dp.abs() + D.abs()))) + 3.0 * U * ds.abs()
    T = lambda t: t.transpose(-1, -2)
    a_dq = a_ds @ k.abs() + _dot_allow(ds.abs() @ k.abs(), S + 15)
    a_dk = T(a_ds) @ q.abs() + _dot_allow(T(ds.abs()) @ q.abs(), S + 15)
    a_dv = T(ap) @ do.abs() + _dot_allow(T(p) @ do.abs(), S + 15)
    return flat3(a_dq, a_dk, a_dv)


# ------------------------------------------------------------------------------------------------------------------------------- the two-limb split
def _rtz(x, bits, emin):
    """x (float64) truncated toward zero to `bits` significand bits, exponent floor emin (fp16: 11 bits, quantum 2^-24 below 2^-14)"""
    _, ex = torch.frexp(x)                                            # |x| in [2^(ex-1), 2^ex)
    quantum = torch.ldexp(torch.ones_like(x), (ex.clamp(min=emin + 1) - bits).to(torch.int32))
    return torch.trunc(x / quantum) * quantum


def x2(x, dtype):
    """hi + lo of x2_split (fsvit_common.h) on the fp32 value of x"""
    x = x.float()
    if dtype == torch.bfloat16:
        hi = (x.contiguous().view(torch.int32) & -65536).view(torch.float32)
        lo = (x - hi).to(torch.bfloat16).float()
        return (hi.double() + lo.double())
    xd = x.double()
    hi = _rtz(xd, 11, -14)
    return hi + _rtz(xd - hi, 11, -14)


def x2_unit(dtype):
    """u2: bound of |x - (hi + lo)| / |x| (bf16: lo is within 2^-7 |x| and rounded to nearest, 2^-9 of itself; fp16: both limbs truncated, 2^-10 each)"""
    return 2.0 ** -16 if dtype == torch.bfloat16 else 2.0 ** -20


# ------------------------------------------------------------------------------------------------------------------------------- points forms
def forward_points(qkv, B, S, heads, hdp, scale, kind, dtype, order='natural'):
    """kind 'v2' | 'v1' (dtype = the 16-bit storage type), 'x2' (dtype = the limb type, fp32 storage; order: the key order of its float32
    evaluation, 'natural' | 'reversed'), 'f32'"""
    q, k, v = split_heads(qkv, B, S, heads, hdp)
    acc = fp32_allowance_forward(qkv, B, S, heads, hdp, scale)
    if kind == 'f32':
        pre = forward_exact(qkv, B, S, heads, hdp, scale)
        return Points(pre, pre.float().double(), acc)
    if kind == 'x2':
        # the limb errors (fp16: 2^-20) are of the size of the fp32 roundings between them (a score of magnitude 60 rounds by 2^-19 of e; a chain of S
        # accumulations by 2^-24 sqrt S), so the form is EVALUATED IN FLOAT32, keys in `order`: with the arithmetic in float64 a float32 torch evaluation
        # of these very formulas sat at 1.16 .. 1.52 of gate 2 (tests/test_attention_ref_cpu.py) - the reference alone missed its gate
        q2, k2, v2 = x2(q, dtype).float(), x2(k, dtype).float(), x2(v, dtype).float()
        if order == 'reversed':
            k2, v2 = k2.flip(-2), v2.flip(-2)
        sc = (q2 @ k2.transpose(-1, -2)) * torch.tensor(scale, dtype=torch.float32)
        e = torch.exp(sc - sc.max(-1, keepdim=True).values)
        inv = 1.0 / e.sum(-1, keepdim=True)
        pre = flat((x2(e.double(), dtype).float() @ v2) * inv).double()
        # first-order deviation: the splits of e and v directly, those of q and k through the scores
        _, _, e0, l0 = _softmax(q, k, scale)
        p = e0 / l0
        o = p @ v
        t_vp = 2.0 * (p ** 2 @ v ** 2)
        a = p ** 2 * 2.0 * ((q ** 2) @ (k ** 2).transpose(-1, -2))     # var(s_ij) / (scale u2)^2 * 3 = sum_d q_d^2 k_jd^2 (q's split) + the same (k's)
        t_s = scale ** 2 * (a @ v ** 2 - 2.0 * o * (a @ v) + o ** 2 * a.sum(-1, keepdim=True))
        sig = x2_unit(dtype) / math.sqrt(3.0) * flat((t_vp + t_s).clamp(min=0.0).sqrt())
        return Points(pre, pre.float().double(), acc, sig)
    rnd = rounder(dtype)
    _, _, e, l = _softmax(q, k, scale)
    p = e / l
    pre = flat((rnd(e) @ v) / l) if kind == 'v2' else flat(rnd(p) @ v)
    sig = half_ulp(dtype) / math.sqrt(3.0) * flat((p ** 2 @ v ** 2).sqrt())
    return Points(pre, rnd(pre), acc, sig)


def backward_points(qkv, dctx, B, S, heads, hdp, scale, kind, dtype):
    """kind 'mfma' | 'fma' (dtype torch.bfloat16), 'f32'"""
    q, k, v = split_heads(qkv, B, S, heads, hdp)
    do = heads_of(dctx, B, S, heads, hdp)
    acc = fp32_allowance_backward(qkv, dctx, B, S, heads, hdp, scale)
    if kind in ('f32', 'fma'):
        pre = backward_exact(qkv, dctx, B, S, heads, hdp, scale)
        return Points(pre, pre.float().double() if kind == 'f32' else rounder(dtype)(pre), acc)
    rnd = rounder(dtype)
    dq, dk, dv, p, _, _, ds = _backward(q, k, v, do, scale, rnd, rnd)
    pre = flat3(dq, dk, dv)
    T = lambda t: t.transpose(-1, -2)
    sig = half_ulp(dtype) / math.sqrt(3.0) * flat3((ds ** 2 @ k ** 2).sqrt(), (T(ds ** 2) @ q ** 2).sqrt(), (T(p ** 2) @ do ** 2).sqrt())
    return Points(pre, rnd(pre), acc, sig)
