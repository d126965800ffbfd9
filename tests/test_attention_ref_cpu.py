"""The references, gates and route table of the stand-alone attention kernels (oracle/attention_oracle.py, tests/attention_cases.py), without a GPU:

* forward_exact / backward_exact equal torch.softmax and torch autograd in float64;
* the route entries (host only) return, for every case of the table, the kernel the table names; the table reaches EVERY instantiation behind
  launch_attention and launch_attention_bwd and every refusal - a dispatch change that orphans a kernel fails here;
* for every case and EVERY element the reference alone sits inside the gate the GPU test holds the kernel to: the points form (16-bit storage; two-limb:
  evaluated in float32, and its reversed key order held to both gates against the natural one), or a float32 torch evaluation of the same formulas in
  two key orders, natural and reversed (fp32 storage).  Prints the worst err / bound per case;
* fp16 / f16x2 inputs and results stay far from 65504.
"""
import math

import pytest
import torch

import attention_cases as ac
from oracle import attention_oracle as ao


def _close(a, b):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize('cid', ['bf16-S100-hd42to64-peaked', 'bf16-S17-hd21to32', 'f32-S113-hd56to64-offset', 'bf16-S100-hd42to64-B1h1'])
def test_exact_forms_equal_torch(cid):
    p = ac.params_of('backward', cid)
    B, S, heads, hd, hdp = p['B'], p['S'], p['heads'], p['hd'], p['hdp']
    t = {k: v.double() for k, v in ac.inputs('backward', p).items()}
    qkv = t['qkv'].clone().requires_grad_(True)
    q, k, v = [qkv.reshape(B, S, 3, heads, hdp)[:, :, i].permute(0, 2, 1, 3) for i in range(3)]
    ctx = (torch.softmax(q @ k.transpose(-1, -2) * ac.scale_of(p), -1) @ v).permute(0, 2, 1, 3).reshape(B * S, heads * hdp)
    _close(ao.forward_exact(t['qkv'], B, S, heads, hdp, ac.scale_of(p)), ctx.detach())
    ctx.backward(t['dctx'])
    got = ao.backward_exact(t['qkv'], t['dctx'], B, S, heads, hdp, ac.scale_of(p))
    _close(got, qkv.grad)
    if hdp > hd:                                                      # pad channels exactly 0
        assert float(got.reshape(B * S, 3 * heads, hdp)[..., hd:].abs().max()) == 0.0


def test_route_table_reaches_every_kernel():
    from fewshot_vit_amd import _lib
    lib = _lib.load()
    seen = {'forward': set(), 'backward': set()}
    for op in ac.CASES:
        for cid, p in ac.CASES[op]:
            if op == 'forward':
                r = lib.fsvit_op_attention_route(p['S'], p['hdp'], ac.CODE[p['dt']])
            else:
                r = lib.fsvit_op_attention_bwd_route(p['S'], p['hd'], p['hdp'], ac.CODE[p['dt']])
            assert r == p['route'], (op, cid, r, p['route'])
            seen[op].add((p['dt'], r))
    missing = [x for x in ac.FWD_INSTANCES if x not in seen['forward']] + [x for x in ac.BWD_INSTANCES if x not in seen['backward']]
    assert not missing, missing
    assert {r for _, r in seen['forward'] if r >= 0} == {r for _, r in ac.FWD_INSTANCES}          # and nothing the lists do not know
    assert {r for _, r in seen['backward'] if r >= 0} == {r for _, r in ac.BWD_INSTANCES}
    # refusals of the route entries themselves
    for dtype in (-1, 5, 17):
        assert lib.fsvit_op_attention_route(25, 32, dtype) == -1
    for dtype in (-1, 2, 3, 4, 17):
        assert lib.fsvit_op_attention_bwd_route(25, 21, 32, dtype) == -1
    for S, hd, hdp in ((0, 21, 32), (25, 0, 32), (25, 33, 32)):
        assert lib.fsvit_op_attention_bwd_route(S, hd, hdp, 1) == -1 and lib.fsvit_op_attention_bwd_route(S, hd, hdp, 0) == -1
    for S, hdp in ((0, 32), (25, 0), (25, 8), (-3, 64)):
        for dtype in range(5):
            assert lib.fsvit_op_attention_route(S, hdp, dtype) == -1


def _eval32(op, p, t, reverse):
    """the exact formulas evaluated in float32 by torch, keys in natural or reversed order"""
    B, S, heads, hdp = p['B'], p['S'], p['heads'], p['hdp']
    q, k, v = [x.float() for x in ao.split_heads(t['qkv'], B, S, heads, hdp)]
    if reverse:
        k, v = k.flip(-2), v.flip(-2)
    scale = float(ac.scale_of(p))
    if op == 'forward':
        _, _, e, l = ao._softmax(q, k, scale)
        return ao.flat((e / l) @ v).double()
    dq, dk, dv = ao._backward(q, k, v, ao.heads_of(t['dctx'], B, S, heads, hdp).float(), scale)[:3]
    if reverse:
        dk, dv = dk.flip(-2), dv.flip(-2)
    return ao.flat3(dq, dk, dv).double()


@pytest.mark.parametrize('op,cid', [(op, cid) for op in ac.CASES for cid in ac.ids(op)])
def test_reference_stays_inside_its_gate(op, cid):
    p = ac.params_of(op, cid)
    t = {k: v.double() for k, v in ac.inputs(op, p).items()}
    A, P = ac.reference(op, cid)
    assert bool(torch.isfinite(A).all()) and bool(torch.isfinite(P.pre).all()) and bool(torch.isfinite(P.acc).all())
    if p['dt'] in ('f16', 'f16x2'):
        assert max(float(x.abs().max()) for x in t.values()) < 1024.0 and float(A.abs().max()) < 1024.0
    if p['hdp'] > p['hd']:
        for x in (A, P.pre, P.out):
            assert float(x.reshape(x.shape[0], -1, p['hdp'])[..., p['hd']:].abs().max()) == 0.0
    if ac.kind_of(op, p) == 'f32':
        worst = max(ac.gate(op, p, _eval32(op, p, t, rev), A, P)['worst'] for rev in (False, True))
        print(f'{op} {cid}: float32 torch (two key orders) worst err/bound {worst:.3f}')
    elif ac.kind_of(op, p) == 'x2':      # the two-limb form is evaluated in float32: its other key order against both gates
        B, S, heads, hdp = p['B'], p['S'], p['heads'], p['hdp']
        other = ao.forward_points(t['qkv'], B, S, heads, hdp, ac.scale_of(p), 'x2', ac.points_dtype(p), order='reversed')
        g = ac.gate(op, p, other.out, A, P)
        worst = max(g['worst'], ac.gate(op, p, P.out, A, P)['worst'])
        print(f'{op} {cid} (x2): points worst err/bound {worst:.3f}, reversed key order mean ratio {g["ratio"]:.4f}')
        assert g['ratio'] <= 1.25, (op, cid, g)
    else:
        g = ac.gate(op, p, P.out, A, P)
        worst = g['worst']
        print(f'{op} {cid} ({ac.kind_of(op, p)}): points worst err/bound {worst:.3f}')
        assert math.isclose(g['ratio'], 1.0) or (g['ratio'] == 0.0 and bool((P.out == A).all()))      # (S = 1: ctx = v, nothing to round)
    assert worst <= 1.0, (op, cid, worst)


def test_regimes_are_what_they_claim():
    """peaked (q x 4 at 100 keys): the median row maximum of P is above 0.5 and every twentieth row or more is nearly one-hot (max P > 0.9);
    offset: the raw scaled scores pass +-60; zero_row: a uniform row of P and a key of score 0"""
    for regime, cid in (('peaked', 'bf16-S100-hd42to64-peaked'), ('offset', 'bf16-S100-hd42to64-offset'), ('zero_row', 'bf16-S100-hd42to64-zero_row')):
        p = ac.params_of('backward', cid)
        t = ac.inputs('backward', p)
        q, k, _ = ao.split_heads(t['qkv'].double(), p['B'], p['S'], p['heads'], p['hdp'])
        s = q @ k.transpose(-1, -2) * ac.scale_of(p)
        P = s.softmax(-1)
        if regime == 'peaked':
            assert float(P.max(-1).values.median()) > 0.5 and float((P.max(-1).values > 0.9).double().mean()) > 0.05
        elif regime == 'offset':
            assert float(s.max()) > 60.0 and float(s.min()) < -60.0
        else:
            assert float((P[:, :, 1] - 1.0 / p['S']).abs().max()) < 1e-15 and float(s[:, :, :, p['S'] - 2].abs().max()) == 0.0
