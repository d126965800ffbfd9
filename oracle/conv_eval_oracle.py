"""Float64 references of the kernels every evaluation runs first: the single-GEMM conv kernels (conv3x3_halo.hip, conv_gemm_v2.hip, gemm256.hip) with
their eval epilogues, and the fused stage-1 block (stage1_w4.hip, stage1_ring.hip).  Written from the mathematics and from the kernel headers of this
repository; every function takes float64 tensors that the caller has ALREADY rounded to the storage type.

Single-GEMM kernels (one output = one dot product + an epilogue, no stored intermediate):
  conv_pre(...)      -> (z, sabs): the pre-activation  z = sum_k x_k w_k [+ tail] + bias  and  sabs = sum_k |x_k w_k|  (the quantity the accumulation
                        bound of an element is taken from; the tail slice included)
  conv_epilogue(...) -> y:  (+ res if res_first); act; (+ res otherwise); 2 x 2 max-pool; + pos      (conv_gemm.h)

Stage-1 block, y = x + W3 GELU(W2 *g8 GELU(W1 x + b1)):
  stage1_exact(...)            no intermediate rounding, erf GELU
  stage1_points(..., dtype)    -> Points(pre, out, acc): the same with the rounding points of stage1_w4.hip's header and of fsvit_common.h:
      * W1 / 8 rounded to the storage type (exact in bf16, subnormal in fp16 below 2^-11); b1 / 8 (fp32) as the 16-bit pair hi + lo that rides as one
        more k step; the accumulators hold z / 8;
      * bf16: gelu_tab - the bf16 code of z / 8 indexes a table of T(gelu_erf(z) / 8): 15 binades x 128 codes per sign, |z| in [2^-10, 32); smaller
        magnitudes share the first entry, larger ones the last (z = 31.875), the sign is kept.  gelu_table(z) is that function;
      * fp16: no table - gelu_sig on the unrounded z, h / 8 stored in fp16 (subnormals included);
      * h1 / 8 and h2 / 8 are rounded where they are stored; everything else fp32; the residual enters conv3's accumulators in fp32;
      * out = T(pre);  acc = K 2^-24 sum |terms| of conv3's chain (K = 256 + the residual).
"""
import math

import torch
import torch.nn.functional as F

from .rows_ops_oracle import EPS24, Points
from .train_ops_oracle import gelu_sig, rounder

TAB_LO, TAB_HI = 2.0 ** -10, 31.875        # |z| of the table's first and last entry (gelu_tab: TLO = 2^-13 on z / 8, 15 binades x 128 codes)
TAB_CODES = 15 * 128


def gelu_erf(z):
    """the erf GELU as z Phi(z) with Phi = erfc(-z / sqrt 2) / 2: accurate in RELATIVE terms on the negative tail too, where 1 + erf(z / sqrt 2) cancels
    (float64 loses every digit below z = -8.3; the table of the bf16 build has entries down to z = -31.875)"""
    return 0.5 * z * torch.special.erfc(-z * math.sqrt(0.5))


# ---------------------------------------------------------------------------------------------------------------- single-GEMM kernels
def conv_pre(x, w, bias=None, stride=1, pad=0, groups=1, x2=None, w2=None):
    """x NCHW, w [O, Ig, KH, KW]; tail: x2 [B OH OW, K2] rows in (b, oy, ox) order, w2 [O, K2] -> (z, sabs) NCHW"""
    z = F.conv2d(x, w, None, stride=stride, padding=pad, groups=groups)
    s = F.conv2d(x.abs(), w.abs(), None, stride=stride, padding=pad, groups=groups)
    if x2 is not None:
        B, O, OH, OW = z.shape
        z = z + (x2 @ w2.t()).reshape(B, OH, OW, O).permute(0, 3, 1, 2)
        s = s + (x2.abs() @ w2.abs().t()).reshape(B, OH, OW, O).permute(0, 3, 1, 2)
    if bias is not None:
        z = z + bias.view(1, -1, 1, 1)
    return z, s


def act_fn(act, kind='sig'):
    """act 0 none, 1 GELU (kind 'sig': gelu_sig of the 16-bit builds, 'erf': the exact form of fp32 storage), 2 LeakyReLU(0.1)"""
    if act == 1:
        return gelu_sig if kind == 'sig' else gelu_erf
    if act == 2:
        return lambda t: F.leaky_relu(t, 0.1)
    return lambda t: t


def conv_epilogue(z, act=0, kind='sig', res=None, res_first=False, pool2=False, pos=None):
    """z NCHW pre-activation (bias included) -> y NCHW; pos [OH OW, O] of the (pooled) output pixels"""
    if res is not None and res_first:
        z = z + res
    y = act_fn(act, kind)(z)
    if res is not None and not res_first:
        y = y + res
    if pool2:
        y = F.max_pool2d(y, 2)
    if pos is not None:
        y = y + pos.t().reshape(1, y.shape[1], y.shape[2], y.shape[3])
    return y


# ---------------------------------------------------------------------------------------------------------------- the GELU table of the bf16 build
def gelu_table(z):
    """what a gelu_tab look-up returns for the pre-activation z (float64), times 8: 8 T(gelu_erf(z') / 8), z' = the bf16 rounding of z (of z / 8: the
    same code) held to the table's range with its sign"""
    rnd = rounder(torch.bfloat16)
    zr = 8.0 * rnd(z / 8.0)
    sign = torch.where(torch.signbit(zr), -1.0, 1.0).double()
    zr = sign * zr.abs().clamp(TAB_LO, TAB_HI)
    return 8.0 * rnd(gelu_erf(zr) / 8.0)


def table_values():
    """-> (z, value): the 2 x 1920 pre-activations the table has an entry for and the float64 value gelu_erf(z) / 8 each entry is the bf16 rounding of"""
    mant = 1.0 + torch.arange(128, dtype=torch.float64) / 128.0
    mag = (torch.exp2(torch.arange(-10, 5, dtype=torch.float64))[:, None] * mant[None, :]).reshape(-1)
    z = torch.cat([-mag.flip(0), mag])
    return z, gelu_erf(z) / 8.0


def near_rounding_boundary(v, dtype, rel):
    """True where the float64 value v lies within rel |v| of a rounding boundary of `dtype` (the midpoint of two neighbouring representable values):
    there a correctly rounded result of a slightly different evaluation may be the neighbour"""
    rnd = rounder(dtype)
    d = rel * v.abs()
    return (rnd(v + d) != rnd(v - d))


# ---------------------------------------------------------------------------------------------------------------- stage-1 block
def _conv2_g8(h, w2, B, H, W):
    """h [B H W, 256] rows, w2 [256, 32, 3, 3] -> grouped 3 x 3 conv rows [B H W, 256]"""
    m = h.reshape(B, H, W, 256).permute(0, 3, 1, 2)
    return F.conv2d(m, w2, None, padding=1, groups=8).permute(0, 2, 3, 1).reshape(B * H * W, 256)


def stage1_exact(x, w1, b1, w2, w3, B, H, W):
    """x rows [B H W, 128], w1 [256, 128], b1 [256], w2 [256, 32, 3, 3], w3 [128, 256] -> y rows"""
    h1 = gelu_erf(x @ w1.t() + b1)
    h2 = gelu_erf(_conv2_g8(h1, w2, B, H, W))
    return x + h2 @ w3.t()


def _hidden(z, dtype, table):
    if table:
        return gelu_table(z)
    return 8.0 * rounder(dtype)(gelu_sig(z) / 8.0)


def stage1_points(x, w1, b1, w2, w3, B, H, W, dtype, table=None):
    """table: the GELUs are gelu_tab look-ups (default: the bf16 build of stage1_w4.hip); False with bf16 is the 16-wave kernel of stage1_ring.hip, which
    keeps gelu_sig on the fp32 pre-activation"""
    table = dtype == torch.bfloat16 if table is None else table
    rnd = rounder(dtype)
    w1p = 8.0 * rnd(w1 / 8.0)
    b8 = (b1 / 8.0).float().double()                    # b1 * 0.125f in fp32 (exact), then hi + lo
    hi = rnd(b8)
    b1p = 8.0 * (hi + rnd((b8 - hi).float().double()))
    h1 = _hidden(x @ w1p.t() + b1p, dtype, table)
    h2 = _hidden(_conv2_g8(h1, w2, B, H, W), dtype, table)
    pre = x + h2 @ w3.t()
    acc = 257 * EPS24 * (h2.abs() @ w3.abs().t() + x.abs())
    return Points(pre, rnd(pre), acc)
