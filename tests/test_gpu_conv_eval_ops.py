"""The kernels every evaluation runs first - conv3x3_halo.hip, conv_gemm_v2.hip, gemm256.hip with their eval epilogues, stem.hip's planar conv1 and the
stage-1 block (stage1_w4.hip both instantiations, stage1_ring.hip) - against the float64 references of oracle/conv_eval_oracle.py, through
fsvit_op_conv_eval / fsvit_op_stem_conv1 / fsvit_op_stage1_block_eval.  Cases, inputs, references and bounds: tests/conv_eval_cases.py (its docstring
states every bound; tests/test_conv_eval_ref_cpu.py proves the references without a GPU).  No bound is computed from a kernel's output.

Single-GEMM kernels: every element within stored_tol(ref, dt, a) of float64; every copy of a reference image (row) bit-equal to its twin; no NaN prefill
survives; the route the dispatcher took is asserted.  Each test prints `worst err / bound` and, in 16-bit storage, the worst `(err - half ulp) / a`
(how the ARITHMETIC sits in its allowance: the rounding of the stored value itself takes the half ulp on any correct kernel).
Stage-1 block: gate 1 (per element) and gate 2 (mean) of rows_cases.gate; prescaled == unscaled, bit for bit; a pixel's value does not depend on its
position in a chunk or a launch, bit for bit; the GELU table entry by entry.
"""
import math

import pytest
import torch

import conv_eval_cases as cc
from conv_eval_cases import E20, U, check, q, stored_tol, sum_tol
from oracle import conv_eval_oracle as co
from test_gpu_ops import CASES, X2_CASES, pack_w

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTS16 = ['bf16', 'f16']
ROUTE_HALO, ROUTE_G256, ROUTE_V2, ROUTE_GCONV_X2 = 0, 1, 2, 3


def _ops():
    from fewshot_vit_amd.engine import ops
    return ops


def held(name, got, ref, dt, a):
    """check(got, ref, stored_tol(ref, dt, a)); printed only: the worst (err - half ulp) / a of 16-bit storage"""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), name + ': not finite (a prefilled element survived?)'
    a = a if torch.is_tensor(a) else torch.full_like(ref, float(a))
    a = a.expand_as(ref)
    if dt != 'f32':
        over = ((got - ref).abs() - cc.half_ulp(ref, dt, a)) / a.clamp_min(1e-300)
        print(f'      beyond the half ulp of {dt}: worst (err - half ulp) / a = {max(float(over.max()), 0.0):.3f}')
    check(name, got, ref, stored_tol(ref, dt, a))


def same_bits(a, b):
    if a.dtype == torch.float32:
        return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    return a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


def nan_like(shape, dtype):
    return torch.full(shape, float('nan'), dtype=dtype, device=DEV)


# ------------------------------------------------------------------------------------------------------------------------------ conv3x3_halo
def run_halo(p, t, dt, stats_buf=None, c1f=None):
    """one fsvit_op_conv_eval launch of a halo case on the device tensors -> (y NHWC on the device, route, stats rows)"""
    dtype = cc.DTYPES[dt]
    B, H, C, N, tail = p['B'], p['H'], t['C'], t['N'], t['tail']
    oh, ow = (H // 2, 20) if tail else (H, 40)
    y = nan_like((B * oh * ow * N,), dtype)
    f = dict(w=t['wp_d'], bias=t['bias_d'], B=B, H=H, W=40, Cin=C, x_cstride=C, KH=3, KW=3, stride=1, pad=1, N=N, y_cstride=N, Kw=t['wp_d'].shape[1], groups=1,
             act=t['act'], x_planar=int(p['xl'] == 'p'), y_planar=int(p['yl'] == 'p'), w_cpad=128 if C == 96 else 0)
    if c1f is None:
        f['x'] = t['xp_d'] if p['xl'] == 'p' else t['x_d']
    else:
        f.update(c1f)
    if tail:
        f.update(x2=t['x2_d'], x2_cstride=32, K2=32, pool2=1, pos=t.get('pos_d'))
    if stats_buf is not None:
        f['stats'] = stats_buf
    route, rows = _ops().conv_eval(y, **f)
    torch.cuda.synchronize()
    y = cc.from_planar(y, B, oh, ow, N) if p['yl'] == 'p' else y.reshape(B, oh, ow, N)
    return y, route, rows


def halo_device(p, t, dt):
    for k in ('x', 'wp', 'bias', 'x2', 'pos'):
        if k in t:
            t[k + '_d'] = t[k].to(DEV)
    if p['xl'] == 'p':
        t['xp_d'] = cc.to_planar(t['x_d'])
    return t


_HALO_REF = {}


def halo_ref(p, t, dt):
    """the float64 reference of a case: formed once, shared by its layouts and tests, never changed"""
    key = (p['kind'], p['B'], p['H'], dt)
    if key not in _HALO_REF:
        _HALO_REF[key] = cc.halo_reference(p, t, dt)
    return _HALO_REF[key]


@pytest.mark.parametrize('dt', DTS16)
@pytest.mark.parametrize('cid', [c for c, _ in cc.HALO_CASES])
def test_halo(cid, dt):
    p = dict(cc.HALO_CASES)[cid]
    t = halo_device(p, cc.halo_inputs(p, dt), dt)
    y, route, _ = run_halo(p, t, dt)
    assert route == ROUTE_HALO
    assert same_bits(y, y[t['src'].to(DEV)]), 'a copy of a reference image differs from its twin: the value depends on the position in the launch'
    assert same_bits(run_halo(p, t, dt)[0], y)
    ref, a, _ = halo_ref(p, t, dt)
    print(f'\n  halo {cid} {dt}')
    held('y', y[t['sub'].to(DEV)], ref, dt, a)


@pytest.mark.parametrize('dt', DTS16)
@pytest.mark.parametrize('cid', [c for c, _ in cc.HALO_STATS_CASES])
def test_halo_stats(cid, dt):
    """the STATS epilogue of conv3x3_halo_kernel<64 | 128, false, true>: y as in test_halo; the column sums of the partial rows against float64 sum y and
    sum y^2 of the UNROUNDED reference map"""
    p = dict(cc.HALO_STATS_CASES)[cid]
    t = halo_device(p, cc.halo_inputs(p, dt), dt)
    C, B = t['N'], p['B']
    n_rows = min(B, 256)
    bufs = []
    for _ in range(2):
        st = nan_like((n_rows + 2, 2, C), torch.float32)
        y, route, rows = run_halo(p, t, dt, stats_buf=st)
        assert route == ROUTE_HALO and rows == n_rows
        assert bool(torch.isnan(st[rows:]).all()), 'rows behind the partial rows were written'
        assert bool(torch.isfinite(st[:rows]).all()), 'a NaN prefill survived in a partial row'
        bufs.append(st[:rows].clone())
    assert same_bits(bufs[0], bufs[1])
    ref, a, _ = halo_ref(p, t, dt)
    print(f'\n  halo stats {cid} {dt}')
    held('y', y[t['sub'].to(DEV)], ref, dt, a)
    stats_check(bufs[0], ref.reshape(-1, C), a.reshape(-1, C), torch.bincount(t['src'], minlength=B)[t['sub']].repeat_interleave(p['H'] * 40), B * p['H'] * 40)


def stats_check(partial, ref, a, count, n_rows):
    """partial [rows][2][C] fp32; ref / a [n, C] the unrounded reference rows and their allowances, count [n] how many rows of the launch equal each"""
    got = partial.double().sum(0).cpu()
    cnt = count.double()[:, None]
    s1, s1a, s2 = (cnt * ref).sum(0), (cnt * ref.abs()).sum(0), (cnt * ref * ref).sum(0)
    check('sum y', got[0], s1, sum_tol(s1a, n_rows) + (cnt * a).sum(0))
    check('sum y^2', got[1], s2, sum_tol(s2, n_rows) + 2.0 * (cnt * ref.abs() * a).sum(0))


# ------------------------------------------------------------------------------------------------------------------------------ C1F, planar stem_conv1
@pytest.mark.parametrize('dt', DTS16)
def test_stem_conv1_planar_is_a_permutation(dt):
    """c1_planar = 1: the planar c1 is a bit-exact permutation of the NHWC c1 (which test_gpu_rows_ops.test_stem_conv1 holds to float64), same patch rows"""
    import rows_cases as rc
    ops = _ops()
    d = {k: (None if v is None else v.to(DEV)) for k, v in rc.inputs('stem_conv1', rc.params_of('stem_conv1', 'B5'), cc.DTYPES[dt]).items()}
    pat, c1 = ops.stem_conv1(d['x'], d['w'], d['b'])
    pat_p, c1_p = ops.stem_conv1(d['x'], d['w'], d['b'], c1_planar=True)
    torch.cuda.synchronize()
    assert same_bits(pat, pat_p)
    assert same_bits(cc.from_planar(c1_p, 5, 40, 40, 64), c1.reshape(5, 40, 40, 64))
    assert same_bits(c1_p.reshape(-1), cc.to_planar(c1.reshape(5, 40, 40, 64)))


@pytest.mark.parametrize('dt', DTS16)
@pytest.mark.parametrize('cid', [c for c, _ in cc.C1F_CASES])
def test_c1f_equals_parent_chain(cid, dt):
    """conv2 with conv1 built on-chip (STEM_PLANAR_C1F, as the engine sets it: planar in and out) == stem_conv1 (planar) -> halo conv2 (planar), bit for
    bit, c2 and the patch rows; the parent chain itself is held to float64 by test_halo / test_stem_conv1.  Copies of an image equal their twin."""
    ops = _ops()
    p = dict(cc.C1F_CASES)[cid]
    B, split = p['B'], p['split']
    t = {k: (v.to(DEV) if torch.is_tensor(v) and k not in ('sub', 'src') else v) for k, v in cc.c1f_inputs(p, dt).items()}
    pat, c1p = ops.stem_conv1(t['img'], t['w1'], t['b1'], c1_planar=True)
    hp = dict(kind='conv2', B=B, H=40, xl='p', yl='p')
    ht = dict(C=64, N=128, act=2, tail=False, wp_d=t['wp'], bias_d=t['bias'], xp_d=c1p)
    c2, route, _ = run_halo(hp, ht, dt)
    assert route == ROUTE_HALO
    pat_f = nan_like(tuple(pat.shape), pat.dtype)
    raw2 = t['img'][split:] if split < B else None
    c2_f, route, _ = run_halo(hp, ht, dt, c1f=dict(c1f_raw=t['img'][:split].contiguous(), c1f_raw2=raw2.contiguous() if raw2 is not None else None, c1f_split=split,
                                                   c1f_patches=pat_f, c1f_w=t['w1'], c1f_kw=t['w1'].shape[1], c1f_bias=t['b1']))
    assert route == ROUTE_HALO
    assert same_bits(pat_f, pat)
    assert same_bits(c2_f, c2)
    assert same_bits(c2_f, c2_f[t['src'].to(DEV)])


# ------------------------------------------------------------------------------------------------------------------------------ conv_gemm_v2 / gemm256
def run_conv(case, t, dt, numerics=None, **extra):
    """a CASES row through fsvit_op_conv_eval -> (y NCHW float64 on the CPU, route)"""
    ops = _ops()
    name, B, H, W, Cin, O, KH, s, p, groups, act, use_res, res_first, use_bias, use_pos = case
    dtype = cc.DTYPES[dt]
    OH, OW = (H + 2 * p - KH) // s + 1, (W + 2 * p - KH) // s + 1
    wd = pack_w(t['w'], groups, dtype)
    wd = ops.x2_limbs(wd, numerics).to(DEV) if numerics else wd.to(DEV)
    nhwc = lambda v: None if v is None else v.permute(0, 2, 3, 1).contiguous().to(DEV)
    y = nan_like((B, OH, OW, O), dtype)
    route, _ = ops.conv_eval(y, numerics=numerics, x=nhwc(t['x']), w=wd, bias=None if t['bias'] is None else t['bias'].to(DEV), res=nhwc(t['res']),
                             pos=None if t['pos'] is None else t['pos'].to(DEV), B=B, H=H, W=W, Cin=Cin // groups, x_cstride=Cin, KH=KH, KW=KH, stride=s, pad=p,
                             N=O // groups, y_cstride=O, Kw=wd.shape[-1], groups=groups, act=act, res_first=res_first, **extra)
    torch.cuda.synchronize()
    return y, route


# (the 16-bit gemm256 takes a layer from 190 flop per streamed byte: these three rows of CASES sit below that and run on conv_gemm_v2; two-limb: all of g256_*)
G256_BELOW_GATE = ('g256_fc2_res', 'g256_proj_k384', 'g256_k128')


def conv_case_route(case, dt):
    name = case[0]
    if name.startswith('halo_') and dt in DTS16:
        return ROUTE_HALO
    if name.startswith('g256_') and dt != 'f32' and name not in G256_BELOW_GATE:
        return ROUTE_G256
    return ROUTE_V2


def conv_case_check(case, dt, numerics=None):
    t = cc.conv_case_inputs(case, dt, numerics)
    name, B, H, W, Cin, O, KH, s, p, groups, act, use_res, res_first = case[:13]
    y, route = run_conv(case, t, dt, numerics)
    ref, a = cc.case_reference(case, t, dt, numerics)
    print(f'\n  conv {name} {numerics or dt}: route {route}')
    held('y', y.permute(0, 3, 1, 2), ref, dt, a)
    return route


@pytest.mark.parametrize('dt', ['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_conv_cases(case, dt):
    """every row of CASES of test_gpu_ops.py, per element against float64"""
    assert conv_case_check(case, dt) == conv_case_route(case, dt)


@pytest.mark.parametrize('numerics', ['bf16x2', 'f16x2'])
@pytest.mark.parametrize('case', [c for c in CASES if c[0] in X2_CASES], ids=[c[0] for c in CASES if c[0] in X2_CASES])
def test_conv_cases_two_limb(case, numerics):
    """the two-limb modes: unrounded fp32 operands, the operand-precision gate of test_conv_gemm_two_limb per element on the element's sum |products|"""
    route = conv_case_check(case, 'f32', numerics)
    assert route == (ROUTE_GCONV_X2 if case[0].startswith('3x3_grouped') else ROUTE_G256 if case[0].startswith('g256_') else ROUTE_V2)


WALK_PARAMS = [(n, m) for n in cc.WALK_CASES for m in (('f32', 'bf16', 'f16', 'bf16x2') if n.startswith('v2') else ('bf16', 'f16', 'bf16x2'))]


@pytest.mark.parametrize('name,mode', WALK_PARAMS, ids=[f'{n}-{m}' for n, m in WALK_PARAMS])
def test_second_walk_rows(name, mode):
    """plain [M][K] x [N][K] layers one tile longer than the persistent grid: the reference rows (first tile, last tile = the second walk, 32 rows each side
    of it, 256 seeded rows) per element against float64, every other row bit-equal to the reference row it is a copy of"""
    ops = _ops()
    c = cc.WALK_CASES[name]
    M, N, K, BM = c['M'], c['N'], c['K'], c['BM']
    numerics = mode if mode.endswith('x2') else None
    dt = 'f32' if numerics else mode
    dtype = cc.DTYPES[dt]
    t = cc.gemm_rows_inputs(M, N, K, dt, BM, (M - 1) // BM * BM, name, numerics)
    bke = 32 if dt == 'f32' else 64
    kw = -(-K // bke) * bke
    wp = torch.zeros(N, kw)
    wp[:, :K] = t['w']
    wd = ops.x2_limbs(wp, numerics).to(DEV) if numerics else wp.to(dtype).to(DEV)
    y = nan_like((M, N), dtype)
    route, _ = ops.conv_eval(y, numerics=numerics, x=t['x'].to(DEV), w=wd, bias=t['bias'].to(DEV), B=M, H=1, W=1, Cin=K, x_cstride=K, KH=1, KW=1, stride=1, pad=0,
                             N=N, y_cstride=N, Kw=kw, groups=1, act=1 if name.startswith('g256') else 0, res_first=0)
    torch.cuda.synchronize()
    want = ROUTE_V2 if name.startswith('v2') or (name == 'g256_k128' and not numerics) else ROUTE_G256
    assert route == want, (route, want)
    assert same_bits(y, y[t['src'].to(DEV)]), 'a copy of a reference row differs from its twin'
    sub = t['sub']
    ref, a = cc.rows_reference(t, dt, act=1 if name.startswith('g256') else 0, numerics=numerics)
    print(f'\n  second walk {name} {mode}: route {route}, {len(sub)} reference rows of {M}')
    held('y', y[sub.to(DEV)], ref, dt, a)


@pytest.mark.parametrize('dt', ['f32', 'bf16', 'f16'])
def test_second_walk_grouped3x3(dt):
    """grouped 3 x 3 (8 groups of 32 -> 32, the 128 x 32 tile at three workgroups per CU): 31 images of 20 x 20 = 97 m-tiles, 8 x 97 = 776 items on 768
    workgroups.  Reference images: the first two and the last four (the eight items of the second walk lie in the last 1024 rows); the rest are copies"""
    case = cc.GROUPED_WALK_CASE
    B = case[1]
    t = cc.conv_case_inputs(case, dt)
    sub = torch.cat([torch.arange(2), torch.arange(B - 4, B)])
    src = cc.twins(B, sub)
    t['x'] = t['x'][src]
    y, route = run_conv(case, t, dt)
    assert route == ROUTE_V2
    assert same_bits(y, y[src.to(DEV)])
    ref, a = cc.case_reference(case, t, dt, images=sub)
    print(f'\n  grouped 3x3 second walk {dt}')
    held('y', y[sub.to(DEV)].permute(0, 3, 1, 2), ref, dt, a)


@pytest.mark.parametrize('dt', ['f32', 'bf16', 'f16'])
def test_y_rpi_rows_behind_a_cls_token(dt):
    """y_rpi = S, y_row0 = 1: the 16 patch rows of each of 3 images go behind the image's cls row, which must come back untouched"""
    case = cc.Y_RPI_CASE
    S, sentinel = cc.Y_RPI_S, 24576.0
    t = cc.conv_case_inputs(case, dt)
    ops = _ops()
    dtype = cc.DTYPES[dt]
    wd = pack_w(t['w'], 1, dtype).to(DEV)
    y = torch.full((3 * S + 1, 96), sentinel, dtype=dtype, device=DEV)
    route, _ = ops.conv_eval(y, x=t['x'].permute(0, 2, 3, 1).contiguous().to(DEV), w=wd, bias=t['bias'].to(DEV), pos=t['pos'].to(DEV), B=3, H=4, W=4, Cin=64,
                             x_cstride=64, KH=1, KW=1, stride=1, pad=0, N=96, y_cstride=96, Kw=wd.shape[-1], groups=1, act=0, res_first=0, y_rpi=S, y_row0=1)
    torch.cuda.synchronize()
    assert route == ROUTE_V2
    rows = y[:3 * S].reshape(3, S, 96)
    assert bool((rows[:, 0] == sentinel).all()) and bool((y[3 * S:] == sentinel).all()), 'a cls row or the row behind the buffer was written'
    ref, a = cc.case_reference(case, t, dt)
    print(f'\n  y_rpi {dt}')
    held('y', rows[:, 1:].reshape(3, 4, 4, 96).permute(0, 3, 1, 2), ref, dt, a)


@pytest.mark.parametrize('dt', ['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('B,OH,OW,C', [(3, 4, 3, 128), (2, 5, 20, 96)])
def test_maxpool2_pos(B, OH, OW, C, dt):
    """its only inexact step is one fp32 add and one rounding: stored_tol(ref, dt, u (|max| + |pos|))"""
    g = cc._gen('maxpool', B, OH, OW, C)
    x = torch.randn(B, 2 * OH, 2 * OW, C, generator=g).to(cc.DTYPES[dt])
    pos = torch.randn(OH * OW, C, generator=g) * 0.5
    got = _ops().maxpool2_pos(x.to(DEV), pos.to(DEV))
    torch.cuda.synchronize()
    mx = torch.nn.functional.max_pool2d(x.double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    ref = mx + pos.double().reshape(1, OH, OW, C)
    print(f'\n  maxpool2_pos {(B, OH, OW, C)} {dt}')
    held('y', got, ref, dt, U * (mx.abs() + pos.double().abs().reshape(1, OH, OW, C)))


@pytest.mark.parametrize('dt', DTS16)
@pytest.mark.parametrize('name', list(cc.V2_STATS_CASES))
def test_v2_stats(name, dt):
    """conv_gemm_v2_kernel<., 128, 64, 2, 2, 2, true>: y per element, the partial rows' column sums against float64, idle workgroups' rows exactly zero"""
    ops = _ops()
    c = cc.V2_STATS_CASES[name]
    M, N, K = c['M'], c['N'], c['K']
    dtype = cc.DTYPES[dt]
    t = cc.gemm_rows_inputs(M, N, K, dt, 128, (M - 1) // 128 * 128, name)
    wd = t['w'].to(dtype).to(DEV)
    f = dict(x=t['x'].to(DEV), w=wd, bias=t['bias'].to(DEV), B=M, H=1, W=1, Cin=K, x_cstride=K, KH=1, KW=1, stride=1, pad=0, N=N, y_cstride=N, Kw=K, groups=1, act=0)
    bufs = []
    for _ in range(2):
        st = nan_like((c['rows'] + 2, 2, N), torch.float32)
        y = nan_like((M, N), dtype)
        route, rows = ops.conv_eval(y, stats=st, **f)
        torch.cuda.synchronize()
        assert route == ROUTE_V2 and rows == c['rows']
        assert bool(torch.isnan(st[rows:]).all()) and bool(torch.isfinite(st[:rows]).all()), 'a NaN prefill survived, or rows behind the partial rows were written'
        bufs.append(st[:rows].clone())
    assert same_bits(bufs[0], bufs[1])
    zero_rows = int((bufs[0].abs().amax((1, 2)) == 0).sum())
    assert zero_rows == c['idle'], f'{zero_rows} all-zero partial rows, {c["idle"]} idle workgroups'
    assert same_bits(y, y[t['src'].to(DEV)])
    sub = t['sub']
    ref, a = cc.rows_reference(t, dt)
    print(f'\n  v2 stats {name} {dt}')
    held('y', y[sub.to(DEV)], ref, dt, a)
    stats_check(bufs[0], ref, a, torch.bincount(t['src'], minlength=M)[sub], M)


def test_v2_stats_refused_where_the_grid_mixes_n_tiles():
    """N = 128, M = 389: 4 x 2 items on a grid of 8 - a workgroup's items would not share an n-tile, conv_stats_rows is 0 and the entry refuses the layer"""
    ops = _ops()
    x, w = torch.zeros(389, 64, device=DEV, dtype=torch.bfloat16), torch.zeros(128, 64, device=DEV, dtype=torch.bfloat16)
    y, st = nan_like((389, 128), torch.bfloat16), nan_like((8, 2, 128), torch.float32)
    with pytest.raises(ValueError, match='no statistics epilogue'):
        ops.conv_eval(y, stats=st, x=x, w=w, B=389, H=1, W=1, Cin=64, x_cstride=64, KH=1, KW=1, stride=1, pad=0, N=128, y_cstride=128, Kw=64, groups=1, act=0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(st).all())


# ------------------------------------------------------------------------------------------------------------------------------ stage-1 block
def stage1_device(t, dt):
    dtype = cc.DTYPES[dt]
    return dict(x=t['x'].to(DEV), w1=t['w1'].to(DEV), b1=t['b1'].to(DEV), w2=cc.stage1_pack_w2(t['w2'], dtype).to(DEV), w3=t['w3'].to(DEV))


def stage1_launch(d, B, H, prescaled, x=None):
    x = d['x'] if x is None else x
    y = _ops().stage1_block_eval(x.reshape(B, H, H, 128), d['w1'], d['b1'], d['w2'], d['w3'], prescaled)
    torch.cuda.synchronize()
    return y.reshape(B * H * H, 128)


@pytest.mark.parametrize('dt', DTS16)
@pytest.mark.parametrize('cid', [c for c, _ in cc.STAGE1_CASES])
def test_stage1_block(cid, dt):
    """stage1_w4_kernel<true, true> (the instantiation the engine runs) and <true, false>: bit-equal to each other (8 x W3 is exact), repeatable, and
    inside both gates against the float64 block"""
    p = dict(cc.STAGE1_CASES)[cid]
    B, H = p['B'], p['H']
    t = cc.stage1_inputs(p, dt)
    d = stage1_device(t, dt)
    y1, y0 = stage1_launch(d, B, H, True), stage1_launch(d, B, H, False)
    assert bool(torch.isfinite(y1).all())
    assert same_bits(y1, y0), 'prescaled (8 x W3) and unscaled conv3 differ: the header claims the prescale is exact'
    assert same_bits(stage1_launch(d, B, H, True), y1)
    A, P = cc.stage1_reference(p, t, dt)
    g = cc.gate(y1.double().cpu(), A, P, cc.DTYPES[dt])
    print(f'stage1 {cid} {dt}: worst err/bound {g["worst"]:.3f}, mean ratio {g["ratio"]:.4f}, sigma {g["sigma"]:.3e}')
    assert g['worst'] <= 1.0, (cid, dt, g)
    assert g['ratio'] <= 1.25, (cid, dt, g)


@pytest.mark.parametrize('B', [1, 5])
def test_stage1_ring16(B):
    """the 16-wave kernel of stage1_ring.hip (fsvit_stage1_block, bf16, 20 x 20): the same gates, its points without the GELU table"""
    p = dict(cc.STAGE1_CASES)[f'B{B}-H20']
    t = cc.stage1_inputs(p, 'bf16')
    d = stage1_device(t, 'bf16')
    y = _ops().stage1_block(d['x'].reshape(B, 20, 20, 128), d['w1'], d['b1'], d['w2'], d['w3'])
    torch.cuda.synchronize()
    A, P = cc.stage1_reference(p, t, 'bf16', table=False)
    g = cc.gate(y.reshape(-1, 128).double().cpu(), A, P, torch.bfloat16)
    print(f'stage1 ring16 B{B}: worst err/bound {g["worst"]:.3f}, mean ratio {g["ratio"]:.4f}')
    assert g['worst'] <= 1.0 and g['ratio'] <= 1.25, g


@pytest.mark.parametrize('dt', DTS16)
@pytest.mark.parametrize('B,H', [(7, 10), (42, 20)])
def test_stage1_position_independence(B, H, dt):
    """one image copied B times: every copy's output equals the B = 1 launch, bit for bit (7 x 100 pixels: every copy starts at another phase of the
    64-pixel chunks; 42 x 400: 263 chunks, two per workgroup)"""
    p = dict(cc.STAGE1_CASES)['B5-H10' if H == 10 else 'B5-H20']
    t = cc.stage1_inputs(p, dt)
    d = stage1_device(t, dt)
    one = d['x'][:H * H].contiguous()
    for prescaled in (True, False):
        y1 = stage1_launch(d, 1, H, prescaled, one)
        yB = stage1_launch(d, B, H, prescaled, one.repeat(B, 1).contiguous())
        assert same_bits(yB.reshape(B, H * H, 128), y1.reshape(1, H * H, 128).expand(B, -1, -1).contiguous()), (B, H, dt, prescaled)


# ------------------------------------------------------------------------------------------------------------------------------ the GELU table, entry by entry
def _bf16_step(v, n):
    """float64 values of bf16 numbers moved by n codes (away from zero for n > 0)"""
    c = v.to(torch.bfloat16).view(torch.int16).to(torch.int32)
    return (c + n).to(torch.int16).view(torch.bfloat16).double()


def _table_flip(z):
    """True where the table entry a pre-activation z reads lies within 2^-20 |value| of a bf16 rounding boundary"""
    rnd = co.rounder(torch.bfloat16)
    zr = 8.0 * rnd(z / 8.0)
    zr = torch.where(torch.signbit(zr), -1.0, 1.0).double() * zr.abs().clamp(co.TAB_LO, co.TAB_HI)
    return co.near_rounding_boundary(co.gelu_erf(zr) / 8.0, torch.bfloat16, E20)


@pytest.mark.parametrize('prescaled', [True, False])
def test_gelu_table_sweep_bf16(prescaled):
    """every table code of both signs, and 128 codes beyond each end, at both GELU call sites (cases: sweep_inputs): each output IS a table value, so it
    must equal the oracle's table EXACTLY unless an entry on its way lies within 2^-20 |value| of a bf16 rounding boundary: a second-GELU flip entry may
    come out one ulp beside the oracle's; a first-GELU flip entry may be one code beside it, and the output then has to EQUAL the oracle's composition
    from that neighbouring code - one code in total.
    One allowance beyond the issue's rule, from the number formats: the kernel fills its table in fp32, and an entry below the smallest NORMAL fp32
    number (8 x 2^-126 at the output: z < -13, |GELU| < 1e-37) has no 2^-24 relative precision left - fp32 subnormals carry fewer bits, or are flushed -
    so the 2^-20 rule cannot classify it: such an output may be the oracle's rounded subnormal or zero."""
    t = cc.sweep_inputs('bf16')
    d = stage1_device(t, 'bf16')
    y = stage1_launch(d, 1, 16, prescaled).double().cpu()
    z1, z2 = cc.sweep_codes(t)
    w2, w3 = cc.stage1_w2_conv(t['w2'].double()), t['w3'].double()
    flip1 = _table_flip(z1)
    cand = []
    for n in (0, 1, -1):          # the first GELU's entry as the oracle has it, and one code beside it
        h1 = co.gelu_table(z1)
        h1 = h1 if n == 0 else 8.0 * _bf16_step(h1 / 8.0, n)
        zz = co._conv2_g8(h1, w2, 1, 16, 16)
        cand.append((co.gelu_table(zz) @ w3.t(), _table_flip(zz).double() @ w3.t().abs() > 0))
    dirty1 = co._conv2_g8(flip1.double(), w2.abs(), 1, 16, 16) @ w3.t().abs() > 0      # routed from a flip entry of the first GELU
    used = w3.abs().sum(1) > 0
    n_bad, n_soft = 0, 0
    ulp = lambda v: 2.0 * cc.half_ulp(v, 'bf16', 0.0)
    ok0 = torch.where(cand[0][1], (y - cand[0][0]).abs() <= ulp(cand[0][0]), y == cand[0][0])
    ok_any = ok0.clone()
    for c, _ in cand[1:]:
        ok_any |= y == c
    tiny = cand[0][0].abs() < 8.0 * 2.0 ** -126
    ok0 |= tiny & (y == 0.0)
    ok_any |= tiny & (y == 0.0)
    ok = torch.where(dirty1, ok_any, ok0)[:, used]
    n_soft = int((dirty1 | cand[0][1])[:, used].sum())
    n_bad = int((~ok).sum())
    print(f'gelu table sweep bf16 (prescaled {prescaled}): {int(used.sum()) * 256} outputs, {n_soft} on a flip entry, {n_bad} mismatches')
    assert float(y[:, ~used][:, 1:].abs().max()) == 0.0 and torch.equal(y[:, 0], t['x'][:, 0].double())      # unrouted channels: x itself
    if n_bad:
        bad = (~torch.where(dirty1, ok_any, ok0)) & used[None, :]
        i = bad.nonzero()[:: max(1, n_bad // 8)][:8]
        print('  first mismatches (pixel, channel, got, want):', [(int(a), int(b), float(y[a, b]), float(cand[0][0][a, b])) for a, b in i])
    assert n_bad == 0


def test_gelu_table_sweep_f16():
    """the same inputs in the fp16 build (no table: gelu_sig by VALU; the two call sites are separately slotted), every (binade, sign) of both sites:
      * second GELU (hidden blocks 1 / 3, positive pixels): its pre-activation is exact, |h / 8 - gelu_sig(z) / 8| <= t(z);
      * first GELU (blocks 0 / 2: positive / negative pixels) through the second: with z2 = s 8 gelu_sig(z1) / 8 (s = the power-of-two rescale),
        |y / 8 - gelu_sig(z2) / 8| <= L0 |s| t(z1) + t(z2) - the first site's allowance carried through the slope of the second; where z2 lies in
        [8, 32) the second GELU is the identity in fp16 and the element is ALSO held directly, |y / (8 s) - gelu_sig(z1) / 8| <= t(z1).
    t(z) = stored_tol(ref, 'f16', 2^-20 (1 + |z|)) on the stored h / 8, half an ulp no smaller than 2^-25 (fp16 subnormals)."""
    from oracle.train_ops_oracle import gelu_sig
    from test_gpu_train_conv_ops import lipschitz
    L0 = lipschitz('sig')[0]
    t = cc.sweep_inputs('f16')
    d = stage1_device(t, 'f16')
    y = stage1_launch(d, 1, 16, True).double().cpu()
    assert same_bits(stage1_launch(d, 1, 16, False), stage1_launch(d, 1, 16, True))
    m = 1.0 + torch.arange(128, dtype=torch.float64) / 128.0

    def tol8(z):
        ref8, a8 = gelu_sig(z) / 8.0, E20 * (1.0 + z.abs()) / 8.0
        return ref8, torch.maximum(cc.half_ulp(ref8, 'f16', a8), torch.tensor(2.0 ** -25, dtype=torch.float64)) + a8

    worst, checked, direct = 0.0, 0, 0
    for j, e in enumerate(cc.SWEEP_BINADES):
        k = 4 - min(max(e, -10), 4)
        for blk, rows, sign, scale in ((0, slice(0, 128), 1.0, 2.0 ** k), (2, slice(128, 256), -1.0, -2.0 ** k), (1, slice(0, 128), 1.0, 1.0),
                                       (3, slice(0, 128), -1.0, 1.0)):
            z = sign * m * 2.0 ** e
            got8 = y[rows, 1 + 32 * blk + j] / 8.0
            ref8, t1 = tol8(z)
            if blk in (1, 3):
                r = (got8 - ref8).abs() / t1
            else:
                z2 = scale * 8.0 * ref8
                ref2, t2 = tol8(z2)
                r = (got8 - ref2).abs() / (L0 * abs(scale) * t1 + t2)
                through = (z2 >= 8.0) & (z2 < 32.0)
                if bool(through.any()):
                    r = torch.maximum(r, torch.where(through, (got8 / scale - ref8).abs() / t1, torch.zeros_like(r)))
                    direct += int(through.sum())
            worst = max(worst, float(r.max()))
            checked += 1
            assert bool((r <= 1.0).all()), (e, blk, float(r.max()))
    assert checked == 4 * len(cc.SWEEP_BINADES) and direct >= 15 * 128      # every (binade, block); the positive half of the table's 15 binades held directly
    print(f'gelu sweep f16: {checked} (binade, block) pairs, {direct} elements also held directly, worst err/bound {worst:.3f}')


# ------------------------------------------------------------------------------------------------------------------------------ refusals
def test_rejections_conv_eval():
    """fsvit_op_conv_eval / fsvit_op_stage1_block_eval / fsvit_op_stem_conv1 refuse what the kernels would misread (ValueError = FSVIT_ERR_ARG) and leave a
    NaN-filled output untouched"""
    ops = _ops()
    bf = torch.bfloat16
    x64 = torch.zeros(1, 40, 40, 64, device=DEV, dtype=bf)          # (every buffer holds the largest geometry below: a refusal that failed would stay in bounds)
    w64 = torch.zeros(128, 640, device=DEV, dtype=bf)
    y = nan_like((1, 40, 40, 128), bf)
    base = dict(x=x64, w=w64, B=1, H=8, W=40, Cin=64, x_cstride=64, KH=3, KW=3, stride=1, pad=1, N=128, y_cstride=128, Kw=576, groups=1, act=2)
    route, rows = ops.conv_eval(y, **base)
    assert route == ROUTE_HALO and rows == 0
    y.fill_(float('nan'))
    st = nan_like((256, 2, 128), torch.float32)
    raw = torch.zeros(1, 3, 80, 80, device=DEV)
    c1f = dict(c1f_raw=raw, c1f_patches=torch.zeros(1600, 32, device=DEV, dtype=bf), c1f_w=torch.zeros(64, 64, device=DEV, dtype=bf), c1f_kw=64,
               c1f_bias=torch.zeros(64, device=DEV), c1f_split=1)
    bad = [
        dict(base, W=36, x_planar=1),                                  # planar on a map conv3x3_halo does not take (conv_gemm_v2 would read it as NHWC)
        dict(base, H=12, y_planar=1),                                  # H % 8
        dict(base, w_cpad=128),                                        # the 128-channel image on a 64-channel layer
        dict(base, w_cpad=64),
        dict(base, stats=st),                                          # stats behind an activation
        dict(base, act=0, stats=st, y_planar=1),                       # stats with a planar output
        dict(base, x_planar=1, y_planar=1, **c1f),                     # C1F at H = 8 (H = 40 only)
        dict(base, H=40, x_planar=0, y_planar=1, **c1f),               # C1F without the planar input flag
        dict(base, H=40, x_planar=1, y_planar=1, **dict(c1f, c1f_kw=16)),
        dict(base, H=40, x_planar=1, y_planar=1, **dict(c1f, c1f_split=0)),      # images past the split without c1f_raw2
        dict(base, act=3),                                             # ACT_MUL is a training epilogue
        dict(base, x2=x64, x2_cstride=32, K2=32),                      # a tail operand without its K slice in the weights
        dict(base, pool2=1, H=8, res=y),                               # pool2 with a residual
        dict(base, y_rpi=100, y_row0=1),                               # y_rpi smaller than the rows it has to hold
        dict(base, Kw=512),                                            # weight rows shorter than K
        dict(base, x=None),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            ops.conv_eval(y, **f)
        torch.cuda.synchronize()
        assert bool(torch.isnan(y).all()) and bool(torch.isnan(st).all()), i
    with pytest.raises(ValueError):
        ops.conv_eval(nan_like((1, 40, 40, 128), torch.float32), **dict(base, x=x64.float(), w=torch.zeros(128, 640, device=DEV), x_planar=1))      # planar in fp32 storage
    xs = torch.zeros(2, 10, 10, 128, device=DEV, dtype=bf)
    w1, b1, w2, w3 = torch.zeros(256, 128, device=DEV, dtype=bf), torch.zeros(256, device=DEV), torch.zeros(256, 320, device=DEV, dtype=bf), torch.zeros(128, 256, device=DEV, dtype=bf)
    with pytest.raises(TypeError):
        ops.stage1_block_eval(xs.float(), w1, b1, w2, w3, True)
    with pytest.raises(TypeError):
        ops.stage1_block_eval(xs.half(), w1, b1, w2, w3, True)
    with pytest.raises(ValueError):
        ops.stage1_block_eval(torch.zeros(2, 21, 21, 128, device=DEV, dtype=bf), w1, b1, w2, w3, True)
    with pytest.raises(ValueError):
        ops.stage1_block_eval(torch.zeros(2, 10, 12, 128, device=DEV, dtype=bf), w1, b1, w2, w3, False)
    with pytest.raises(ValueError):
        ops.stem_conv1(torch.zeros(1, 3, 64, 64, device=DEV), torch.zeros(64, 64, device=DEV, dtype=bf), None, c1_planar=True)
    torch.cuda.synchronize()
