"""The stand-alone attention kernels - attention.hip (attention_v2_kernel in 5 element modes, the generic attention_kernel) and attention_bwd.hip (the bf16
MFMA kernel, the exact-fp32 MFMA kernels, the FMA fallbacks) - against the float64 references of oracle/attention_oracle.py, through ops.attention and
ops.attention_backward, over the table of tests/attention_cases.py: every instantiation behind both launchers, both sides of every dispatch threshold,
S = 1, exact multiples of 16, B = heads = 1, and the input regimes flat / peaked / offset / zero_row.

Every case asserts, in this order: the route entry names the kernel the table expects; the output is finite; pad channels hd .. hdp-1 of every output are
exactly 0; three launches are bit-identical; images 1 .. B-1 launched alone equal those rows of the full launch bit for bit; 8 canary rows behind the
output buffer are untouched; fp32 backward (the kernels mask by hd): a finite non-zero fill of the INPUT pad channels leaves the output bit-identical;
then the gates.

GATES (tests/attention_cases.py gate; no constant comes from a kernel run; tests/test_attention_ref_cpu.py holds the reference alone inside them for
every case and element).
 * 16-bit storage and two-limb: the two gates of tests/rows_cases.py, A = *_exact, P = *_points, dQ / dK / dV separately.
 * fp32 storage: |got - A| <= a + u |A|, u = 2^-24, a = the first-order allowance below, all from float64 quantities.  dot(t, n) = sum_tol(t, n) + u t
   (test_gpu_train_ops.py sum_tol = 4 sqrt(n) u t for a chain of n terms with sum |terms| = t; u t: the rounding of the fp32 products), E = 2^-20 (what
   test_elementwise allows the hardware exp2 / rcp and expf).
     score            a_s_ij  = scale dot(sum_d |q_id k_jd|, hdp) + 2 u (|s_ij| + |max_i|)          (the scale multiply, the subtraction of the maximum)
     exponential      r_ij    = a_s_ij + E                                                           relative error of e_ij; the maximum's own error cancels
     1 / sum          gamma   = 4 sqrt(S) u + E + 2 u                                                beyond the terms' errors
     softmax          ap_ij   = p_ij (r_ij + sum_j' p_ij' r_ij' + gamma)   >= |delta p_ij|
     forward          a_ctx   = sum_j p_ij r_ij |v_jc - ctx_ic| + gamma |ctx_ic| + dot(sum_j p_ij |v_jc|, S + 31) + 2 u |ctx_ic|
     dP               a_dP    = dot(sum_d |dO_id v_jd|, hdp)
     D                a_D     = sum_j (ap_ij |dP_ij| + p_ij a_dP_ij) + dot(sum_j p_ij |dP_ij|, S + 15)
     dS               a_dS    = scale (ap |dP - D| + p (a_dP + a_D + u (|dP| + |D|))) + 3 u |dS|
     dQ, dK, dV       a_dQ = a_dS |K| + dot(|dS| |K|, S + 15),  a_dK = a_dS^T |Q| + dot(|dS|^T |Q|, S + 15),  a_dV = ap^T |dO| + dot(p^T |dO|, S + 15)
   The same a is the `acc` term of the 16-bit gates.

Each test prints `op, case, dtype, route, worst err/bound, mean ratio`.
"""
import pytest
import torch

import attention_cases as ac

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CANARY = 24576.0        # exactly representable in every storage type; no output of these cases comes near it
NUMERICS = {'bf16x2': 'bf16x2', 'f16x2': 'f16x2'}


def _route(op, p):
    from fewshot_vit_amd import _lib
    lib = _lib.load()
    if op == 'forward':
        return lib.fsvit_op_attention_route(p['S'], p['hdp'], ac.CODE[p['dt']])
    return lib.fsvit_op_attention_bwd_route(p['S'], p['hd'], p['hdp'], ac.CODE[p['dt']])


def _launch(op, p, d, lo=0):
    """the operator on images lo .. of the device inputs; the output is the head of a larger buffer whose 8 tail rows are canaries"""
    from fewshot_vit_amd.engine import ops
    B, S, heads, hd, hdp = p['B'] - lo, p['S'], p['heads'], p['hd'], p['hdp']
    N = (1 if op == 'forward' else 3) * heads * hdp
    buf = torch.full((B * S + 8, N), CANARY, dtype=ac.TD[p['dt']], device=DEV)
    qkv = d['qkv'][lo * S:]
    if op == 'forward':
        out = ops.attention(qkv, B, S, heads, hdp, ac.scale_of(p), numerics=NUMERICS.get(p['dt']), out=buf[:B * S])
    else:
        out = ops.attention_backward(qkv, d['dctx'][lo * S:], B, S, heads, hd, hdp, ac.scale_of(p), out=buf[:B * S])
    torch.cuda.synchronize()
    assert bool((buf[B * S:] == CANARY).all()), 'rows behind the output were written'
    return out


def _check(op, cid):
    p = ac.params_of(op, cid)
    route = _route(op, p)
    assert route == p['route'], (op, cid, route)
    t = ac.inputs(op, p)
    d = {k: v.to(DEV) for k, v in t.items()}
    got_d = _launch(op, p, d)
    assert got_d.dtype == ac.TD[p['dt']]
    assert bool(torch.isfinite(got_d).all())
    if p['hdp'] > p['hd']:
        assert float(got_d.reshape(got_d.shape[0], -1, p['hdp'])[..., p['hd']:].abs().max()) == 0.0
    for _ in range(2):
        assert torch.equal(_launch(op, p, d), got_d)
    if p['B'] > 1:
        assert torch.equal(_launch(op, p, d, lo=1), got_d[p['S']:])
    if op == 'backward' and p['dt'] == 'f32' and p['hdp'] > p['hd']:
        f = {}
        for k, v in d.items():
            x = v.clone().reshape(v.shape[0], -1, p['hdp'])
            x[..., p['hd']:] = 3.25
            f[k] = x.reshape(v.shape)
        assert torch.equal(_launch(op, p, f), got_d), 'the input pad channels reached the output'
    A, P = ac.reference(op, cid)
    g = ac.gate(op, p, got_d.double().cpu(), A, P)
    ratio = '-' if g['ratio'] is None else f'{g["ratio"]:.4f}'
    print(f'{op} {cid} {p["dt"]} route {route}: worst err/bound {g["worst"]:.3f}, mean ratio {ratio}')
    assert g['worst'] <= 1.0, (op, cid, g)
    assert g['ratio'] is None or g['ratio'] <= 1.25, (op, cid, g)


@pytest.mark.parametrize('cid', ac.ids('forward'))
def test_attention_forward(cid):
    _check('forward', cid)


@pytest.mark.parametrize('cid', ac.ids('backward'))
def test_attention_backward(cid):
    _check('backward', cid)


def test_rejections_attention():
    """every refusal of fsvit.h returns FSVIT_ERR_ARG with a message and leaves a canary-filled output untouched; fp16 and mixed types raise TypeError"""
    from fewshot_vit_amd import _lib
    from fewshot_vit_amd.engine import _ptr, _stream_ptr, ops
    lib = _lib.load()
    st = _stream_ptr(torch.device(DEV))

    def refused(call, out):
        rc_ = call()
        torch.cuda.synchronize()
        assert rc_ == _lib.ERR_ARG, rc_
        assert lib.fsvit_last_error().decode() != ''
        assert bool((out == CANARY).all()), 'a refused call wrote its output'

    for op in ('forward', 'backward'):                                 # the table's refused shapes, through ops and through the C entries
        for cid in ac.ids(op, refused=True):
            p = ac.params_of(op, cid)
            B, S, heads, hd, hdp = p['B'], p['S'], p['heads'], p['hd'], p['hdp']
            d = {k: v.to(DEV) for k, v in ac.inputs(op, p).items()}
            N = (1 if op == 'forward' else 3) * heads * hdp
            out = torch.full((B * S, N), CANARY, dtype=ac.TD[p['dt']], device=DEV)
            with pytest.raises(ValueError):
                if op == 'forward':
                    ops.attention(d['qkv'], B, S, heads, hdp, ac.scale_of(p), numerics=NUMERICS.get(p['dt']), out=out)
                else:
                    ops.attention_backward(d['qkv'], d['dctx'], B, S, heads, hd, hdp, ac.scale_of(p), out=out)
            torch.cuda.synchronize()
            assert bool((out == CANARY).all()), (op, cid)
            if op == 'forward':
                refused(lambda: lib.fsvit_attention(_ptr(d['qkv']), _ptr(out), B, S, heads, hdp, 0.1, ac.CODE[p['dt']], st), out)
            else:
                refused(lambda: lib.fsvit_attention_backward(_ptr(d['qkv']), _ptr(d['dctx']), _ptr(out), B, S, heads, hd, hdp, 0.1, ac.CODE[p['dt']], st), out)
    # the argument checks of the C entries
    B, S, heads, hd, hdp = 2, 25, 3, 21, 32
    for dt, code in ((torch.float32, _lib.F32), (torch.bfloat16, _lib.BF16)):
        qkv = torch.zeros(B * S, 3 * heads * hdp, dtype=dt, device=DEV)
        dctx = torch.zeros(B * S, heads * hdp, dtype=dt, device=DEV)
        out = torch.full_like(qkv, CANARY)
        bwd = lambda B=B, S=S, heads=heads, hd=hd, hdp=hdp, code=code, q=qkv, o=out: lib.fsvit_attention_backward(_ptr(q), _ptr(dctx), _ptr(o), B, S, heads, hd, hdp, 0.2, code, st)
        for kw in (dict(B=-1), dict(S=0), dict(S=-4), dict(heads=0), dict(hd=0), dict(hd=33), dict(hdp=16), dict(code=_lib.F16), dict(code=_lib.BF16X2),
                   dict(code=_lib.F16X2), dict(code=17), dict(code=-1), dict(q=None), dict(o=None)):
            if 'o' in kw:
                assert bwd(**kw) == _lib.ERR_ARG
            else:
                refused(lambda: bwd(**kw), out)
        assert bwd(B=0) == 0                                             # nothing to do: no launch, no error
        torch.cuda.synchronize()
        assert bool((out == CANARY).all())
        ctx = torch.full_like(dctx, CANARY)
        fwd = lambda B=B, S=S, heads=heads, hdp=hdp, code=code, q=qkv: lib.fsvit_attention(_ptr(q), _ptr(ctx), B, S, heads, hdp, 0.2, code, st)
        for kw in (dict(B=-1), dict(S=0), dict(heads=0), dict(hdp=0), dict(hdp=24), dict(code=17), dict(code=-1), dict(q=None)):
            refused(lambda: fwd(**kw), ctx)
    # fp16 and mixed-type tensors into ops.attention_backward; fp32 rows are what the two-limb forward reads
    qf = torch.zeros(B * S, 3 * heads * hdp, device=DEV)
    df = torch.zeros(B * S, heads * hdp, device=DEV)
    for a, b in ((qf.half(), df.half()), (qf.bfloat16(), df), (qf, df.bfloat16()), (qf.bfloat16(), df.half())):
        with pytest.raises(TypeError):
            ops.attention_backward(a, b, B, S, heads, hd, hdp, 0.2)
    with pytest.raises(TypeError):
        ops.attention(qf.bfloat16(), B, S, heads, hdp, 0.2, numerics='bf16x2')
    with pytest.raises(ValueError):
        ops.attention(qf, B, S, heads, hdp, 0.2, numerics='bf16')
