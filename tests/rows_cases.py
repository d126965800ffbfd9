"""Cases, inputs, checked subsets and gates of the fused row operators, shared by test_rows_ops_ref_cpu.py (the references alone, no GPU) and
test_gpu_rows_ops.py (the kernels against them).

Gates (none of their constants comes from a kernel run).  For a case let A = NAME_exact on the checked rows, P = NAME_points (P.pre before, P.out after
the output rounding), u = half an ulp of the storage type (relative), sigma = RMS(P.pre - A) over the checked elements = the size of the
intermediate-rounding effect as the reference itself measures it:
  1. per element  |got - A| <= u |A| + 6 sigma + acc,  acc = K 2^-24 sum |terms| of the last fp32 accumulation chain (oracle/rows_ops_oracle.py);
     6 sigma caps a sum of ~1000 independent rounding errors over at most ~1e6 checked elements.  Where the reference gives a per-element deviation
     (P.sig, the attention operators: the rounding effect there depends on the query's |q| and on how peaked its softmax is, so the case's RMS is not
     the deviation of every element - with sigma alone the REFERENCE missed the gate by up to 1.5 x) the element's sigma is max(sigma, P.sig);
  2. mean         mean |got - A| <= 1.25 mean |P.out - A|: a kernel that rounds where the reference says it rounds is statistically P; the margin is
     for roundings that flip because the fp32 accumulation order differs.
The float64 references are formed for a subset of rows (images): the first tile, the last (partial) tile, 32 rows on each side of the first row a
workgroup reaches only on its second tile, and 256 rows drawn with a fixed seed; the GPU tests cover the rest with bit-exact checks.
"""
import math
import os
import re
import zlib

import torch

from oracle import rows_ops_oracle as ro

DTYPES = {'f16': torch.float16, 'bf16': torch.bfloat16}
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'few-shot-vit_amd', 'csrc')
with open(os.path.join(_CSRC, 'mlp_rows.hip')) as _f:
    LGR_OCC = int(re.search(r'^#define LGR_OCC (\d+)', _f.read(), re.M).group(1))      # workgroups per CU of ln_gemm_rows_kernel: its grid cap is 256 LGR_OCC
LN_EPS = 1e-6
GEMM_ROWS_WRAP = 256 * LGR_OCC * 128      # first row a workgroup of ln_gemm_rows reaches only on its second tile


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) % (2 ** 31))


def weight(g, N, K, dtype):
    """randn / sqrt(K) with 1 % of the entries at magnitudes in [2^-14, 2^-11) (below 2^-11 the fp16 W1 / 8 of mlp_pack_kernel is subnormal), rounded to
    the storage type"""
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    tiny = torch.rand(N, K, generator=g) < 0.01
    mag = torch.exp2(-14.0 + 3.0 * torch.rand(N, K, generator=g)).clamp(max=2.0 ** -11 * (1 - 2.0 ** -10))
    w = torch.where(tiny, torch.where(w < 0, -mag, mag), w)
    return w.to(dtype)


def _pad_heads(w, heads, hd, hdp):
    """[3 heads hd, ...] -> [3 heads hdp, ...] with zero rows past hd"""
    out = torch.zeros(3, heads, hdp, *w.shape[1:], dtype=w.dtype)
    out[:, :, :hd] = w.reshape(3, heads, hd, *w.shape[1:])
    return out.reshape(3 * heads * hdp, *w.shape[1:])


def rows_subset(M, BM, wrap):
    """first tile, last tile, 32 rows each side of `wrap` (if the case reaches it), 256 seeded rows"""
    idx = [torch.arange(0, min(BM, M)), torch.arange((M - 1) // BM * BM, M)]
    if wrap is not None and wrap < M:
        idx.append(torch.arange(wrap - 32, min(wrap + 32, M)))
    idx.append(torch.randint(0, M, (256,), generator=_gen('rows', M, BM)))
    return torch.unique(torch.cat(idx))


def images_subset(B, S, per_tile, wrap):
    """the same in whole images of S tokens, per_tile images per workgroup tile"""
    n = -(-32 // S)
    idx = [torch.arange(0, min(per_tile, B)), torch.arange((B - 1) // per_tile * per_tile, B)]
    if wrap is not None and wrap < B:
        idx.append(torch.arange(max(wrap - n, 0), min(wrap + n, B)))
    idx.append(torch.randint(0, B, (-(-256 // S),), generator=_gen('images', B, S)))
    return torch.unique(torch.cat(idx))


def _image_rows(imgs, S):
    return (imgs[:, None] * S + torch.arange(S)[None, :]).reshape(-1)


# --------------------------------------------------------------------------------------------------------------------------- the cases of each operator
# an entry: (id, params).  `wrap`: first row (image) of the second-walk tiles, None where the grid covers the case in one tile per workgroup
def _mlp_cases():
    out = []
    for C, hid, BM in ((256, 1024, 256), (512, 2048, 128)):
        for M in (37, BM + 1, 256 * BM + BM + 3):
            for variant in ('b2', 'nob2', 'inplace'):
                out.append((f'C{C}-M{M}-{variant}', dict(C=C, hid=hid, BM=BM, M=M, variant=variant, wrap=256 * BM)))
    return out


def _proj_cases():
    return [(f'C{C}-M{M}', dict(C=C, KC=KC, hid=4 * C, BM=BM, M=M, wrap=256 * BM))
            for C, KC, BM in ((256, 288, 256), (512, 576, 128)) for M in (BM + 1, 256 * BM + 3)]


def _tail_cases():
    return [(f'hid{hid}-M{M}-{variant}', dict(C=384, KC=384, hid=hid, BM=128, M=M, variant=variant, wrap=256 * 128))
            for hid in (1536, 1152) for M in (197, 256 * 128 + 131) for variant in ('out', 'inplace')]


def _lnlin_cases():
    return [('C384-M197-N1152', dict(C=384, M=197, N=1152, bias=True, ln=True)),
            (f'C384-M{GEMM_ROWS_WRAP + 6}-N96', dict(C=384, M=GEMM_ROWS_WRAP + 6, N=96, bias=True, ln=True)),
            ('C512-M245-N1728-bias', dict(C=512, M=245, N=1728, bias=True, ln=False)),
            ('C512-M131-N96-nobias', dict(C=512, M=131, N=96, bias=False, ln=False))]


def _patch_cases():
    return [(f'B{B}-H{H}-N{N}', dict(B=B, H=H, N=N, Ci=128)) for B, H, N in ((3, 20, 256), (5, 6, 96))]


def _qkv_cases():
    out = []
    for C, hd, hdp, per, cap, shapes in ((256, 42, 48, 2, 256, ((3, 100), (5, 37), (2, 112), (4, 1), (259, 97))),
                                        (512, 85, 96, 4, 512, ((3, 25), (9, 32), (5, 1), (2053, 25)))):
        for B, S in shapes:
            for bias in (True, False):
                out.append((f'C{C}-B{B}-S{S}-{"bias" if bias else "nobias"}',
                            dict(C=C, heads=6, hd=hd, hdp=hdp, B=B, S=S, bias=bias, per=per, wrap=per * cap, ln=False)))
    return out


def _vit_cases():
    return [(f'B{B}-S{S}', dict(C=384, heads=6, hd=64, hdp=64, B=B, S=S, bias=True, per=1, wrap=256, ln=True))
            for B, S in ((3, 197), (1, 33), (2, 1), (2, 256), (258, 33))]


CASES = {'mlp_rows': _mlp_cases(), 'proj_mlp_rows': _proj_cases(), 'vit_block_tail': _tail_cases(), 'ln_linear_rows': _lnlin_cases(),
         'patch_embed2x2': _patch_cases(), 'qkv_attention': _qkv_cases(), 'vit_ln_qkv_attention': _vit_cases(), 'stem_conv1': [('B5', dict(B=5))]}


def params_of(op, cid):
    return dict(CASES[op])[cid]


def ids(op, cpu=False):
    """case ids of an operator; cpu: without the variants that share another case's reference (in place = the same mathematics)"""
    return [cid for cid, p in CASES[op] if not (cpu and p.get('variant') == 'inplace')]


# --------------------------------------------------------------------------------------------------------------------------- inputs (storage-typed, CPU)
def inputs(op, p, dtype):
    """every tensor the operator reads, already in the storage type (biases / pos / the stem's image fp32)"""
    key = {k: v for k, v in p.items() if k != 'variant'}
    g = _gen(op, sorted(key.items()))
    t = {}
    if op in ('mlp_rows', 'proj_mlp_rows', 'vit_block_tail'):
        M, C, hid = p['M'], p['C'], p['hid']
        x = torch.randn(M, C, generator=g)
        t['x'] = (x * 2.0 + 0.5 if op == 'vit_block_tail' else x).to(dtype)
        if op != 'mlp_rows':
            t['ctx'] = torch.randn(M, p['KC'], generator=g).to(dtype)
            t['wp'] = weight(g, C, p['KC'], dtype)
        if op == 'vit_block_tail':
            t['bp'] = torch.randn(C, generator=g) * 0.3
        t['w1'], t['b1'] = weight(g, hid, C, dtype), torch.randn(hid, generator=g) * 0.3
        t['w2'], t['b2'] = weight(g, C, hid, dtype), torch.randn(C, generator=g) * 0.3
        if p.get('variant') == 'nob2':
            t['b2'] = None
    elif op == 'ln_linear_rows':
        x = torch.randn(p['M'], p['C'], generator=g)
        if p['ln']:
            x = x * 2.0 + 0.5
            x[5], x[6] = 0.75, 0.0      # constant rows: variance 0, the LayerNorm lives on eps alone (the zero row: 0 x rsqrt(0) is NaN without it)
        t['x'], t['w'] = x.to(dtype), weight(g, p['N'], p['C'], dtype)
        t['b'] = torch.randn(p['N'], generator=g) * 0.3 if p['bias'] else None
    elif op == 'patch_embed2x2':
        t['x'] = torch.randn(p['B'], p['H'], p['H'], p['Ci'], generator=g).to(dtype)
        t['w'], t['bias'] = weight(g, p['N'], 4 * p['Ci'], dtype), torch.randn(p['N'], generator=g) * 0.3
        t['pos'] = torch.randn((p['H'] // 2) ** 2, p['N'], generator=g) * 0.5
    elif op in ('qkv_attention', 'vit_ln_qkv_attention'):
        B, S, C, heads, hd, hdp = p['B'], p['S'], p['C'], p['heads'], p['hd'], p['hdp']
        x = torch.randn(B * S, C, generator=g)
        if p['ln']:
            x = x * 2.0 + 0.5
            x[0], x[1] = 0.75, 0.0      # constant rows, as for ln_linear_rows
        t['x'] = x.to(dtype)
        t['w'] = _pad_heads(weight(g, 3 * heads * hd, C, dtype), heads, hd, hdp)
        t['b'] = _pad_heads(torch.randn(3 * heads * hd, generator=g) * 0.3, heads, hd, hdp) if p['bias'] else None
    elif op == 'stem_conv1':
        t['x'] = torch.randn(p['B'], 3, 80, 80, generator=g).to(dtype).float()       # the fp32 image, values of the storage type
        w = torch.zeros(64, 64)
        w[:, :27] = weight(g, 64, 27, dtype).float()
        t['w'], t['b'] = w.to(dtype), torch.randn(64, generator=g) * 0.2
    else:
        raise KeyError(op)
    return t


def wrap_of(op, p):
    """first row (image) that a workgroup reaches only on its second tile, or None if the case stays below it"""
    if op == 'ln_linear_rows':
        return GEMM_ROWS_WRAP if p['M'] > GEMM_ROWS_WRAP else None
    if op in ('mlp_rows', 'proj_mlp_rows', 'vit_block_tail'):
        return p['wrap'] if p['M'] > p['wrap'] else None
    if op in ('qkv_attention', 'vit_ln_qkv_attention'):
        return p['wrap'] if p['B'] > p['wrap'] else None
    return None


def checked(op, p):
    """-> (rows, imgs): indices of the checked output rows; imgs (the whole images they make up) for the attention operators, else None"""
    if op in ('mlp_rows', 'proj_mlp_rows', 'vit_block_tail'):
        return rows_subset(p['M'], p['BM'], p['wrap']), None
    if op == 'ln_linear_rows':
        return rows_subset(p['M'], 128, GEMM_ROWS_WRAP), None
    if op == 'patch_embed2x2':
        return torch.arange(p['B'] * (p['H'] // 2) ** 2), None
    if op == 'stem_conv1':
        return torch.arange(p['B'] * 1600), None
    imgs = images_subset(p['B'], p['S'], p['per'], p['wrap'])
    return _image_rows(imgs, p['S']), imgs


def _d(t):
    return None if t is None else t.double()


def reference(op, p, t, dtype):
    """-> (rows, A, P) on the checked rows"""
    rows, imgs = checked(op, p)
    if op == 'mlp_rows':
        a = (_d(t['x'][rows]), _d(t['w1']), _d(t['b1']), _d(t['w2']), _d(t['b2']))
        return rows, ro.mlp_rows_exact(*a), ro.mlp_rows_points(*a, dtype)
    if op == 'proj_mlp_rows':
        a = (_d(t['x'][rows]), _d(t['ctx'][rows]), _d(t['wp']), _d(t['w1']), _d(t['b1']), _d(t['w2']), _d(t['b2']))
        return rows, ro.proj_mlp_rows_exact(*a), ro.proj_mlp_rows_points(*a, dtype)
    if op == 'vit_block_tail':
        a = (_d(t['x'][rows]), _d(t['ctx'][rows]), _d(t['wp']), _d(t['bp']), _d(t['w1']), _d(t['b1']), _d(t['w2']), _d(t['b2']), LN_EPS)
        return rows, ro.vit_block_tail_exact(*a), ro.vit_block_tail_points(*a, dtype)
    if op == 'ln_linear_rows':
        a = (_d(t['x'][rows]), _d(t['w']), _d(t['b']), LN_EPS if p['ln'] else None)
        return rows, ro.ln_linear_rows_exact(*a), ro.ln_linear_rows_points(*a, dtype)
    if op == 'patch_embed2x2':
        a = (_d(t['x']), _d(t['w']), _d(t['bias']), _d(t['pos']))
        return rows, ro.patch_embed2x2_exact(*a), ro.patch_embed2x2_points(*a, dtype)
    if op == 'stem_conv1':
        a = (_d(t['x']), _d(t['w'][:, :27]), _d(t['b']))
        return rows, ro.stem_conv1_exact(*a), ro.stem_conv1_points(*a, dtype)
    a = (_d(t['x'][rows]), _d(t['w']), _d(t['b']), len(imgs), p['S'], p['heads'], p['hdp'], p['hd'] ** -0.5)
    if op == 'qkv_attention':
        return rows, ro.qkv_attention_exact(*a), ro.qkv_attention_points(*a, dtype)
    return rows, ro.vit_ln_qkv_attention_exact(*a, LN_EPS), ro.vit_ln_qkv_attention_points(*a, LN_EPS, dtype)


# --------------------------------------------------------------------------------------------------------------------------- the gates
def gate(got, A, P, dtype):
    """got: float64 values to hold against A (the kernel's output rows, or P.out for the reference-alone test) -> dict(worst = max err / bound of gate 1,
    ratio = mean |got - A| / mean |P.out - A| of gate 2, sigma)"""
    u = ro.half_ulp(dtype)
    sigma = float((P.pre - A).pow(2).mean().sqrt())
    bound = u * A.abs() + 6.0 * (sigma if P.sig is None else P.sig.clamp(min=sigma)) + P.acc
    err = (got - A).abs()
    worst = float(torch.where(bound > 0, err / bound, torch.where(err > 0, math.inf, 0.0).double()).max())
    ref_mean = float((P.out - A).abs().mean())
    ratio = float(err.mean()) / ref_mean if ref_mean > 0 else (0.0 if float(err.mean()) == 0 else math.inf)
    return dict(worst=worst, ratio=ratio, sigma=sigma)
