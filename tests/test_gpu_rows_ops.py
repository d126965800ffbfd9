"""The fused inference row kernels (mlp_rows.hip, qkv_attn.hip, stem.hip) in BOTH 16-bit builds - namespace fsvit (bf16) and fsvit_f16 (fp16, the VALU GELU
slots, the subnormal W1 / 8 of the pack) - against the float64 references of oracle/rows_ops_oracle.py, through the dtype-taking operator entries.

Every case asserts, in this order: the output is finite; padded head dims are exactly 0; 3 repeats are bit-identical; the rows of the tiles a workgroup
reaches only on its second walk equal, bit for bit, the same rows launched alone; gate 1 (per element) and gate 2 (mean) of tests/rows_cases.py on the
checked rows.  The gates' constants come from the number formats and the reference's own error (proved on the CPU by tests/test_rows_ops_ref_cpu.py),
none from a kernel run.  Each test prints `op, case, dtype, worst err/bound, mean ratio`.
"""
import pytest
import torch

import rows_cases as rc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CANARY = 24576.0        # exactly representable in both types; no output of these cases comes near it


def _dev(t):
    return {k: (None if v is None else v.to(DEV)) for k, v in t.items()}


def _launch(op, p, d, lo=0):
    """the operator on rows (images) lo .. of the device inputs d -> [rows, N] output"""
    from fewshot_vit_amd.engine import ops
    if op in ('mlp_rows', 'proj_mlp_rows', 'vit_block_tail'):
        x = d['x'][lo:]
        out = x.clone() if p.get('variant') == 'inplace' else None
        x = out if out is not None else x
        if op == 'mlp_rows':
            return ops.mlp_rows(x, d['w1'], d['b1'], d['w2'], d['b2'], out=out)
        if op == 'proj_mlp_rows':
            return ops.proj_mlp_rows(x, d['ctx'][lo:], d['wp'], d['w1'], d['b1'], d['w2'], d['b2'], out=out)
        return ops.vit_block_tail(x, d['ctx'][lo:], d['wp'], d['bp'], d['w1'], d['b1'], d['w2'], d['b2'], eps=rc.LN_EPS, out=out)
    if op == 'ln_linear_rows':
        # x and y sit inside larger buffers: 128 canary rows behind y must survive, 128 finite rows behind x keep a kernel that loses its row guard in bounds
        M, N = p['M'] - lo, p['N']
        xb = torch.zeros(M + 128, p['C'], dtype=d['x'].dtype, device=DEV)
        xb[:M] = d['x'][lo:]
        yb = torch.full((M + 128, N), CANARY, dtype=d['x'].dtype, device=DEV)
        y = ops.ln_linear_rows(xb[:M], d['w'], d['b'], eps=rc.LN_EPS, out=yb[:M])
        torch.cuda.synchronize()
        assert bool((yb[M:] == CANARY).all()), 'rows behind the output were written'
        return y
    if op == 'patch_embed2x2':
        return ops.patch_embed2x2(d['x'], d['w'], d['bias'], d['pos'])
    if op == 'stem_conv1':
        return ops.stem_conv1(d['x'], d['w'], d['b'])[1]
    S = p['S']
    a = (d['x'][lo * S:], d['w'], d['b'], p['B'] - lo, S, p['heads'], p['hdp'], p['hd'] ** -0.5)
    return ops.qkv_attention(*a) if op == 'qkv_attention' else ops.vit_ln_qkv_attention(*a, eps=rc.LN_EPS)


def _check(op, cid, dt):
    dtype = rc.DTYPES[dt]
    p = rc.params_of(op, cid)
    t = rc.inputs(op, p, dtype)
    d = _dev(t)
    got_d = _launch(op, p, d)
    torch.cuda.synchronize()
    assert got_d.dtype == dtype
    assert bool(torch.isfinite(got_d).all())
    if p.get('hdp', 0) > p.get('hd', 0):
        assert float(got_d.reshape(-1, p['heads'], p['hdp'])[..., p['hd']:].abs().max()) == 0.0       # padded head dims stay exactly 0
    for _ in range(2):
        assert torch.equal(_launch(op, p, d), got_d)
    wrap = rc.wrap_of(op, p)
    if wrap is not None:      # launch-size invariance: the second-walk tiles' rows, launched alone
        per_row = p['S'] if 'S' in p else 1
        assert torch.equal(_launch(op, p, d, lo=wrap), got_d[wrap * per_row:])
    rows, A, P = rc.reference(op, p, t, dtype)
    g = rc.gate(got_d[rows.to(DEV)].double().cpu(), A, P, dtype)
    print(f'{op} {cid} {dt}: worst err/bound {g["worst"]:.3f}, mean ratio {g["ratio"]:.4f}')
    assert g['worst'] <= 1.0, (op, cid, dt, g)
    assert g['ratio'] <= 1.25, (op, cid, dt, g)


def _cases(op):
    return pytest.mark.parametrize('cid', rc.ids(op))


dtypes = pytest.mark.parametrize('dt', list(rc.DTYPES))


@dtypes
@_cases('mlp_rows')
def test_mlp_rows(cid, dt):
    _check('mlp_rows', cid, dt)


@dtypes
@_cases('proj_mlp_rows')
def test_proj_mlp_rows(cid, dt):
    _check('proj_mlp_rows', cid, dt)


@dtypes
@_cases('vit_block_tail')
def test_vit_block_tail(cid, dt):
    _check('vit_block_tail', cid, dt)


@dtypes
@_cases('ln_linear_rows')
def test_ln_linear_rows(cid, dt):
    _check('ln_linear_rows', cid, dt)


@dtypes
@_cases('patch_embed2x2')
def test_patch_embed2x2(cid, dt):
    _check('patch_embed2x2', cid, dt)


@dtypes
@_cases('qkv_attention')
def test_qkv_attention(cid, dt):
    _check('qkv_attention', cid, dt)


@dtypes
@_cases('vit_ln_qkv_attention')
def test_vit_ln_qkv_attention(cid, dt):
    _check('vit_ln_qkv_attention', cid, dt)


@dtypes
def test_stem_conv1(dt):
    """both builds exist (stem_conv1_supported refuses only fp32 storage and other geometries): patch rows bit-identical to ops.im2col27, c1 to the gates"""
    from fewshot_vit_amd.engine import ops
    dtype = rc.DTYPES[dt]
    p = rc.params_of('stem_conv1', 'B5')
    d = _dev(rc.inputs('stem_conv1', p, dtype))
    patches, _ = ops.stem_conv1(d['x'], d['w'], d['b'])
    assert torch.equal(patches, ops.im2col27(d['x'], dtype))
    with pytest.raises(ValueError):          # the geometry it is not built for is refused, not run
        ops.stem_conv1(d['x'][:, :, :64, :64].contiguous(), d['w'], d['b'])
    _check('stem_conv1', 'B5', dt)


def test_row_ops_refuse_what_they_would_misread():
    """fp32 activations, and activations and weights of different 16-bit types, raise TypeError (the entries used to run the bf16 kernel on whatever bits
    they were handed); the C entries refuse any dtype but FSVIT_BF16 / FSVIT_F16."""
    from fewshot_vit_amd import _lib
    from fewshot_vit_amd.engine import _ptr, _stream_ptr, ops
    h, b = torch.float16, torch.bfloat16
    x = torch.randn(37, 256, device=DEV)
    w1, w2 = torch.randn(1024, 256, device=DEV) / 16, torch.randn(256, 1024, device=DEV) / 32
    b1 = torch.zeros(1024, device=DEV)
    with pytest.raises(TypeError):
        ops.mlp_rows(x.to(h), w1.to(b), b1, w2.to(b))
    with pytest.raises(TypeError):
        ops.mlp_rows(x.to(b), w1.to(b), b1, w2.to(h))
    with pytest.raises(TypeError):
        ops.mlp_rows(x, w1.to(b), b1, w2.to(b))
    with pytest.raises(TypeError):
        ops.mlp_rows(x, w1, b1, w2)
    ctx, wp = torch.randn(37, 288, device=DEV), torch.randn(256, 288, device=DEV) / 17
    with pytest.raises(TypeError):
        ops.proj_mlp_rows(x.to(h), ctx.to(b), wp.to(h), w1.to(h), b1, w2.to(h))
    x3, w3 = torch.randn(33, 384, device=DEV), torch.randn(1152, 384, device=DEV) / 20
    b3 = torch.zeros(1152, device=DEV)
    for bad in ((x3, w3.to(h)), (x3.to(h), w3.to(b)), (x3.to(b), w3)):
        with pytest.raises(TypeError):
            ops.ln_linear_rows(bad[0], bad[1], b3)
        with pytest.raises(TypeError):
            ops.vit_ln_qkv_attention(bad[0], bad[1], b3, 1, 33, 6, 64, 0.125)
    with pytest.raises(TypeError):
        ops.vit_block_tail(x3.to(h), x3.to(h), w3[:384].to(b), b3[:384], w3.to(h), b3, w3.t().contiguous().to(h), b3[:384])
    with pytest.raises(TypeError):
        ops.qkv_attention(x.to(h), torch.zeros(864, 256, device=DEV, dtype=b), None, 1, 37, 6, 48, 0.15)
    with pytest.raises(TypeError):
        ops.patch_embed2x2(torch.zeros(1, 4, 4, 128, device=DEV), torch.zeros(32, 512, device=DEV, dtype=h), None, torch.zeros(4, 32, device=DEV))
    with pytest.raises(TypeError):
        ops.stem_conv1(torch.zeros(1, 3, 80, 80, device=DEV), torch.zeros(64, 64, device=DEV), None)
    with pytest.raises(TypeError):
        ops.stem_conv1(torch.zeros(1, 3, 80, 80, device=DEV, dtype=h), torch.zeros(64, 64, device=DEV, dtype=h), None)
    lib = _lib.load()
    xh, w1h, w2h, y = x.to(h), w1.to(h), w2.to(h), torch.empty(37, 256, device=DEV, dtype=h)
    for dtype in (_lib.F32, _lib.BF16X2, _lib.F16X2, 17, -1):
        rc_ = lib.fsvit_mlp_rows_dt(_ptr(xh), _ptr(y), _ptr(w1h), 256, _ptr(b1), _ptr(w2h), 1024, None, 37, 256, 1024, dtype, _stream_ptr(x.device))
        assert rc_ == _lib.ERR_ARG, (dtype, rc_)
        rc_ = lib.fsvit_ln_linear_rows_dt(_ptr(x3), _ptr(y), _ptr(w3), 384, _ptr(b3), 33, 384, 1152, 1e-6, dtype, _stream_ptr(x.device))
        assert rc_ == _lib.ERR_ARG, (dtype, rc_)
