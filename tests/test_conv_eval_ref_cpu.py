"""The references of tests/conv_eval_cases.py (oracle/conv_eval_oracle.py), proved without a GPU:

* the row-chunk-planar converters are inverse to each other, place every element where the formula of conv_gemm.h puts it, and are a permutation;
* conv_pre / conv_epilogue equal torch.nn.functional in float64, and every reference - halo, the rows of CASES, y_rpi, the second walks, the STATS
  layers, the C1F inputs - has the shape of its case's output (the large halo cases: their inputs; they share the small ones' reference code);
* stage1_exact equals the block written with torch.nn.functional; stage1_points stays inside gate 1 of rows_cases.gate against stage1_exact for EVERY
  case and both storage types (the condition under which the GPU test may use the gate), gate 2 trivially;
* the GELU table model: an entry IS the bf16 rounding of gelu_erf / 8 at the entry's pre-activation, both saturating ends keep the sign; the entries
  whose float64 value lies within 2^-20 |value| of a bf16 rounding boundary (where the kernel's fp32 evaluation may round to the neighbour) are
  counted and must be fewer than 1 % of the table;
* the sweep's input reaches every table code of both signs, and at least four codes beyond each end, at BOTH GELU call sites.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_eval_cases as cc
from oracle import conv_eval_oracle as co
from test_gpu_ops import CASES, X2_CASES

DTS16 = ['bf16', 'f16']


def _close(a, b):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max()))


def test_planar_converters_round_trip():
    for B, H, W, C in ((1, 8, 40, 64), (3, 16, 40, 128), (2, 8, 40, 96)):
        x = torch.arange(B * H * W * C, dtype=torch.float32).reshape(B, H, W, C)
        p = cc.to_planar(x)
        assert p.shape == (x.numel(),) and torch.equal(torch.sort(p).values, x.reshape(-1))          # a permutation
        assert torch.equal(cc.from_planar(p, B, H, W, C), x)
        assert torch.equal(cc.to_planar(cc.from_planar(x.reshape(-1), B, H, W, C)), x.reshape(-1))
        # the formula, element by element on a few: a 16-byte chunk of 8 channels is contiguous along a row
        for b, r, c, ch in ((0, 0, 0, 0), (B - 1, H - 1, W - 1, C - 1), (0, 3, 17, 41), (B - 1, 5, 39, 8)):
            assert float(p[((b * H + r) * (C // 8) + ch // 8) * W * 8 + c * 8 + ch % 8]) == float(x[b, r, c, ch])
        assert torch.equal(p.reshape(B, H, C // 8, W, 8), x.reshape(B, H, W, C // 8, 8).permute(0, 1, 3, 2, 4))


def test_conv_reference_equals_functional():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 16, 8, 12, generator=g, dtype=torch.float64)
    w = torch.randn(24, 8, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(24, generator=g, dtype=torch.float64)
    x2 = torch.randn(2 * 8 * 12, 5, generator=g, dtype=torch.float64)
    w2 = torch.randn(24, 5, generator=g, dtype=torch.float64)
    pos = torch.randn(4 * 6, 24, generator=g, dtype=torch.float64)
    z, s = co.conv_pre(x, w, b, 1, 1, 2, x2, w2)
    tail = (x2 @ w2.t()).reshape(2, 8, 12, 24).permute(0, 3, 1, 2)
    _close(z, F.conv2d(x, w, b, padding=1, groups=2) + tail)
    assert bool((s >= (z - b.view(1, -1, 1, 1)).abs() - 1e-12).all())
    _close(co.conv_epilogue(z, act=2, pool2=True, pos=pos), F.max_pool2d(F.leaky_relu(z, 0.1), 2) + pos.t().reshape(1, 24, 4, 6))
    _close(co.conv_epilogue(z, act=1, kind='erf', res=z * 0.5), F.gelu(z) + z * 0.5)
    _close(co.conv_epilogue(z, act=2, res=z * 0.5, res_first=True), F.leaky_relu(1.5 * z, 0.1))


@pytest.mark.parametrize('cid', [c for c, _ in cc.HALO_CASES + cc.HALO_STATS_CASES])
def test_halo_reference_shapes(cid):
    p = dict(cc.HALO_CASES + cc.HALO_STATS_CASES)[cid]
    t = cc.halo_inputs(p, 'f16')
    C, act, tail = cc.HALO_KINDS[p['kind']]
    B, H = p['B'], p['H']
    N = t['N']
    assert N == (96 if C == 96 else 128) and t['w'].shape == (N, C, 3, 3)
    assert t['x'].shape == (B, H, 40, C) and t['wp'].shape == (128, 9 * (128 if C == 96 else C) + (64 if tail else 0))
    sub, src = t['sub'], t['src']
    assert len(sub) <= 10 and torch.equal(src[sub], sub) and bool(torch.isin(src, sub).all())
    assert torch.equal(t['x'], t['x'][src])                                     # every image is a copy of its twin
    if B * (H // 8) > cc.HALO_GRID:                                               # the images of the second-walk tiles are reference images
        assert bool(torch.isin(torch.arange(cc.HALO_GRID, B * (H // 8)) // (H // 8), sub).all())
    if B > 8:
        return                                                                    # (the large cases share the small ones' reference code)
    ref, a, pre = cc.halo_reference(p, t, 'f16')
    n = len(sub)
    assert ref.shape == ((n, H // 2, 20, N) if tail else (n, H, 40, N)) and a.shape == ref.shape and pre[0].shape == (n, H, 40, N)
    assert bool(torch.isfinite(ref).all()) and bool((a > 0).all())


def _out_hw(case):
    B, H, W, Cin, O, KH, s, p = case[1:9]
    return (H + 2 * p - KH) // s + 1, (W + 2 * p - KH) // s + 1


@pytest.mark.parametrize('case', CASES + [cc.Y_RPI_CASE], ids=[c[0] for c in CASES] + ['y_rpi'])
def test_conv_case_reference_shapes(case):
    """every row of CASES (and the y_rpi case): the reference and its allowance have the shape of the case's output"""
    t = cc.conv_case_inputs(case, 'f16')
    ref, a = cc.case_reference(case, t, 'f16')
    assert ref.shape == (case[1], case[5]) + _out_hw(case) and a.shape == ref.shape
    assert bool(torch.isfinite(ref).all()) and bool((a > 0).all())
    if case[0] in X2_CASES:
        t = cc.conv_case_inputs(case, 'f32', 'bf16x2')
        ref2, a2 = cc.case_reference(case, t, 'f32', 'bf16x2')
        assert ref2.shape == ref.shape and bool((a2 > 0).all())


def test_grouped_walk_reference_shape():
    case = cc.GROUPED_WALK_CASE
    t = cc.conv_case_inputs(case, 'bf16')
    sub = torch.cat([torch.arange(2), torch.arange(case[1] - 4, case[1])])
    ref, a = cc.case_reference(case, t, 'bf16', images=sub)
    assert ref.shape == (6, 256, 20, 20) and a.shape == ref.shape
    assert 8 * -(-case[1] * 400 // 128) > 768                                   # more (group, m-tile) items than the 128 x 32 configuration's 768 workgroups


@pytest.mark.parametrize('name', list(cc.WALK_CASES) + list(cc.V2_STATS_CASES))
def test_rows_reference_shapes(name):
    """the second-walk and STATS GEMM cases: reference rows = rows_subset (the last tile, which is the second walk, included), every other row a copy"""
    c = cc.WALK_CASES.get(name) or cc.V2_STATS_CASES[name]
    M, N, K, BM = c['M'], c['N'], c['K'], c.get('BM', 128)
    t = cc.gemm_rows_inputs(M, N, K, 'bf16', BM, (M - 1) // BM * BM, name)
    sub, src = t['sub'], t['src']
    assert t['x'].shape == (M, K) and t['w'].shape == (N, K) and torch.equal(t['x'], t['x'][src]) and torch.equal(src[sub], sub)
    assert bool(torch.isin(torch.arange((M - 1) // BM * BM, M), sub).all()) and bool(torch.isin(torch.arange(min(BM, M)), sub).all())
    ref, a = cc.rows_reference(t, 'bf16', act=1)
    assert ref.shape == (len(sub), N) and a.shape == ref.shape and bool((a > 0).all())
    if name in cc.V2_STATS_CASES:       # conv_gemm_v2's persistent grid of the 128 x 64 statistics configuration, restated: one partial row per workgroup
        items = -(-M // 128) * (N // 64)
        assert c['rows'] == (512 if items >= 512 else -(-items // 8) * 8)


@pytest.mark.parametrize('cid', [c for c, _ in cc.C1F_CASES])
def test_c1f_input_shapes(cid):
    p = dict(cc.C1F_CASES)[cid]
    t = cc.c1f_inputs(p, 'bf16')
    B = p['B']
    assert t['img'].shape == (B, 3, 80, 80) and t['img'].dtype == torch.float32 and t['w1'].shape == (64, 64) and t['wp'].shape == (128, 576)
    assert torch.equal(t['img'], t['img'][t['src']]) and float(t['w1'][:, 27:].abs().max()) == 0.0
    if B * 5 > cc.HALO_GRID:
        assert bool(torch.isin(torch.arange(cc.HALO_GRID, B * 5) // 5, t['sub']).all())


def test_stage1_exact_equals_functional():
    p = dict(cc.STAGE1_CASES)['B3-H7']
    t = cc.stage1_inputs(p, 'f16')
    A, P = cc.stage1_reference(p, t, 'f16')
    x = t['x'].double().reshape(3, 7, 7, 128).permute(0, 3, 1, 2)
    h1 = F.gelu(F.conv2d(x, t['w1'].double().reshape(256, 128, 1, 1), t['b1'].double()))
    h2 = F.gelu(F.conv2d(h1, cc.stage1_w2_conv(t['w2'].double()), padding=1, groups=8))
    y = x + F.conv2d(h2, t['w3'].double().reshape(128, 256, 1, 1))
    _close(A, y.permute(0, 2, 3, 1).reshape(-1, 128))
    assert cc.stage1_pack_w2(t['w2'], torch.float16).shape == (256, 320)


@pytest.mark.parametrize('dt', DTS16)
@pytest.mark.parametrize('cid', [c for c, _ in cc.STAGE1_CASES])
def test_stage1_points_stay_inside_the_gates(cid, dt):
    p = dict(cc.STAGE1_CASES)[cid]
    A, P = cc.stage1_reference(p, cc.stage1_inputs(p, dt), dt)
    assert A.shape == (p['B'] * p['H'] ** 2, 128) and P.out.shape == A.shape
    assert bool(torch.isfinite(A).all()) and bool(torch.isfinite(P.pre).all())
    g = cc.gate(P.out, A, P, cc.DTYPES[dt])
    print(f'stage1 {cid} {dt}: points worst err/bound {g["worst"]:.3f}, sigma {g["sigma"]:.3e}')
    assert g['worst'] <= 1.0, (cid, dt, g)
    assert math.isclose(g['ratio'], 1.0)


def test_gelu_table_model():
    z, v = co.table_values()
    assert z.shape == (2 * co.TAB_CODES,) and float(z.abs().min()) == co.TAB_LO and float(z.abs().max()) == co.TAB_HI
    rnd = co.rounder(torch.bfloat16)
    assert torch.equal(co.gelu_table(z), 8.0 * rnd(v))                                       # an entry IS T(gelu_erf(z) / 8)
    assert torch.equal(rnd(z / 8.0), z / 8.0)                                                # ... at a bf16 code of z / 8
    lo, hi = co.gelu_table(torch.tensor([co.TAB_LO, -co.TAB_LO], dtype=torch.float64)), co.gelu_table(torch.tensor([co.TAB_HI, -co.TAB_HI], dtype=torch.float64))
    small = torch.tensor([0.0, 2.0 ** -11, 2.0 ** -10 * (1 - 2.0 ** -8), 1e-30], dtype=torch.float64)
    big = torch.tensor([32.0, 33.0, 48.0, 1e30], dtype=torch.float64)
    assert bool((co.gelu_table(small) == lo[0]).all()) and bool((co.gelu_table(-small[1:]) == lo[1]).all())      # the first entry, the sign kept
    assert bool((co.gelu_table(big) == hi[0]).all()) and bool((co.gelu_table(-big) == hi[1]).all())              # the last entry, no wrap
    assert float(hi[0]) == co.TAB_HI and float(lo[1]) < 0.0 <= -float(hi[1])
    flips = int(co.near_rounding_boundary(v, torch.bfloat16, cc.E20).sum())
    print(f'gelu table: {flips} of {v.numel()} entries lie within 2^-20 |value| of a bf16 rounding boundary')
    assert flips < 0.01 * v.numel()


def test_sweep_reaches_every_code_at_both_call_sites():
    t = cc.sweep_inputs('bf16')
    for v in t.values():                                                                      # every operand is exact in both storage types
        assert torch.equal(v.float(), v.to(torch.float16).float()) or v.dtype == torch.float32
    z1, z2 = cc.sweep_codes(t)
    want, _ = co.table_values()
    beyond = torch.cat([s * torch.exp2(torch.tensor(float(e), dtype=torch.float64)) * (1.0 + torch.arange(128, dtype=torch.float64) / 128.0)
                        for e in (-11, 5) for s in (1.0, -1.0)])
    for name, zz in (('first', z1), ('second', z2)):
        seen = torch.unique(zz)
        assert bool(torch.isin(want, seen).all()), name
        n_beyond = int(torch.isin(beyond, seen).sum())
        print(f'{name} GELU: all {want.numel()} table codes reached, {n_beyond} codes beyond the ends')
        assert bool(torch.isin(beyond, seen).all()), name
