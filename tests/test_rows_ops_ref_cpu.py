"""The float64 references of the fused row operators (oracle/rows_ops_oracle.py), proved without a GPU:

* every NAME_exact equals the same operator written with torch.nn.functional in float64 (F.gelu, F.layer_norm, F.linear, F.conv2d,
  F.scaled_dot_product_attention-style softmax);
* every NAME_points stays inside the gates that tests/test_gpu_rows_ops.py holds the kernels to - gate 1 for EVERY checked element of EVERY case and
  both storage types, gate 2 trivially (ratio 1) - so a kernel that rounds exactly where the reference says it rounds passes, and the bound is not
  something only a lucky kernel meets;
* the sigmoid-form GELU the fp16 build's points use is within its documented 2.6e-5 of the erf form, and the gelu_tab model of the bf16 build
  within one bf16 rounding of it.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import rows_cases as rc
from oracle import rows_ops_oracle as ro
from oracle.train_ops_oracle import gelu_sig

OPS = list(rc.CASES)


def _small(op):
    """the operator's smallest case, fp16 inputs, as float64"""
    cid = {'mlp_rows': 'C256-M37-b2', 'proj_mlp_rows': 'C256-M257', 'vit_block_tail': 'hid1152-M197-out', 'ln_linear_rows': 'C384-M197-N1152',
           'patch_embed2x2': 'B5-H6-N96', 'qkv_attention': 'C256-B5-S37-bias', 'vit_ln_qkv_attention': 'B1-S33', 'stem_conv1': 'B5'}[op]
    p = rc.params_of(op, cid)
    return p, {k: rc._d(v) for k, v in rc.inputs(op, p, torch.float16).items()}


def _close(a, b):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max()))


def test_exact_mlp_family_equals_functional():
    p, t = _small('mlp_rows')
    _close(ro.mlp_rows_exact(t['x'], t['w1'], t['b1'], t['w2'], t['b2']),
           t['x'] + F.linear(F.gelu(F.linear(t['x'], t['w1'], t['b1'])), t['w2'], t['b2']))
    _close(ro.mlp_rows_exact(t['x'], t['w1'], t['b1'], t['w2'], None), t['x'] + F.linear(F.gelu(F.linear(t['x'], t['w1'], t['b1'])), t['w2']))
    p, t = _small('proj_mlp_rows')
    x1 = t['x'] + F.linear(t['ctx'], t['wp'])
    _close(ro.proj_mlp_rows_exact(t['x'], t['ctx'], t['wp'], t['w1'], t['b1'], t['w2'], t['b2']),
           x1 + F.linear(F.gelu(F.linear(x1, t['w1'], t['b1'])), t['w2'], t['b2']))
    p, t = _small('vit_block_tail')
    x1 = t['x'] + F.linear(t['ctx'], t['wp'], t['bp'])
    _close(ro.vit_block_tail_exact(t['x'], t['ctx'], t['wp'], t['bp'], t['w1'], t['b1'], t['w2'], t['b2'], rc.LN_EPS),
           x1 + F.linear(F.gelu(F.linear(F.layer_norm(x1, (384,), eps=rc.LN_EPS), t['w1'], t['b1'])), t['w2'], t['b2']))


def test_exact_linear_family_equals_functional():
    p, t = _small('ln_linear_rows')
    _close(ro.ln_linear_rows_exact(t['x'], t['w'], t['b'], rc.LN_EPS), F.linear(F.layer_norm(t['x'], (384,), eps=rc.LN_EPS), t['w'], t['b']))
    _close(ro.ln_linear_rows_exact(t['x'], t['w'], None, None), F.linear(t['x'], t['w']))
    p, t = _small('patch_embed2x2')
    N, H, Ci = p['N'], p['H'], p['Ci']
    conv = F.conv2d(t['x'].permute(0, 3, 1, 2), t['w'].reshape(N, 2, 2, Ci).permute(0, 3, 1, 2), t['bias'], stride=2)
    conv = conv + t['pos'].t().reshape(1, N, H // 2, H // 2)
    _close(ro.patch_embed2x2_exact(t['x'], t['w'], t['bias'], t['pos']), conv.permute(0, 2, 3, 1).reshape(-1, N))
    p, t = _small('stem_conv1')
    w = t['w'][:, :27]
    conv = F.leaky_relu(F.conv2d(t['x'], w.reshape(64, 3, 3, 3).permute(0, 3, 1, 2), t['b'], stride=2, padding=1), 0.1)
    _close(ro.stem_conv1_exact(t['x'], w, t['b']), conv.permute(0, 2, 3, 1).reshape(-1, 64))


@pytest.mark.parametrize('op', ['qkv_attention', 'vit_ln_qkv_attention'])
def test_exact_attention_equals_functional(op):
    p, t = _small(op)
    B, S, heads, hdp, hd = p['B'], p['S'], p['heads'], p['hdp'], p['hd']
    x = F.layer_norm(t['x'], (p['C'],), eps=rc.LN_EPS) if p['ln'] else t['x']
    qkv = F.linear(x, t['w'], t['b']).reshape(B, S, 3, heads, hdp).permute(2, 0, 3, 1, 4)
    ref = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2], scale=hd ** -0.5).permute(0, 2, 1, 3).reshape(B * S, heads * hdp)
    a = (t['x'], t['w'], t['b'], B, S, heads, hdp, hd ** -0.5)
    got = ro.vit_ln_qkv_attention_exact(*a, rc.LN_EPS) if p['ln'] else ro.qkv_attention_exact(*a)
    _close(got, ref)
    pts = ro.vit_ln_qkv_attention_points(*a, rc.LN_EPS, torch.float16) if p['ln'] else ro.qkv_attention_points(*a, torch.float16)
    for v in (got, pts.pre, pts.out):
        assert float(v.reshape(B * S, heads, hdp)[..., hd:].abs().max() if hdp > hd else 0.0) == 0.0      # padded head dims exactly 0


def test_gelu_forms():
    z = torch.linspace(-12.0, 12.0, 200001, dtype=torch.float64)
    assert float((gelu_sig(z) - F.gelu(z)).abs().max()) <= 2.7e-5                         # fsvit_common.h: max |gelu_sig - gelu_erf| = 2.6e-5
    _close(ro.gelu_erf(z), F.gelu(z))
    rnd = ro.rounder(torch.bfloat16)
    h = ro._hidden_points(z, rnd, torch.bfloat16)
    zr = 8.0 * rnd(z / 8.0)
    big = zr.abs() >= 2.0 ** -10
    assert float((h - rnd(F.gelu(zr)))[big].abs().max()) == 0.0                           # the table entry IS bf16(gelu_erf(bf16(z)))
    assert float(h[~big].abs().max()) <= 2.0 ** -10                                      # below the table: the first entry


@pytest.mark.parametrize('dt', list(rc.DTYPES))
@pytest.mark.parametrize('op,cid', [(op, cid) for op in OPS for cid in rc.ids(op, cpu=True)])
def test_points_stay_inside_the_gates(op, cid, dt):
    dtype = rc.DTYPES[dt]
    p = rc.params_of(op, cid)
    rows, A, P = rc.reference(op, p, rc.inputs(op, p, dtype), dtype)
    assert A.shape == P.out.shape and A.shape[0] == len(rows)
    assert bool(torch.isfinite(A).all()) and bool(torch.isfinite(P.pre).all())
    assert float((P.out - ro.rounder(dtype)(P.pre)).abs().max()) == 0.0
    g = rc.gate(P.out, A, P, dtype)
    print(f'{op} {cid} {dt}: points worst err/bound {g["worst"]:.3f}, sigma {g["sigma"]:.3e}, rows {len(rows)}')
    assert g['worst'] <= 1.0, (op, cid, dt, g)
    assert math.isclose(g['ratio'], 1.0)
