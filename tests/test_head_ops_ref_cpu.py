"""The references and gates of the episode head, distillation losses and optimizers (oracle/head_ops_oracle.py, tests/head_cases.py), without a GPU:

* each float64 reference equals torch ops / autograd / torch.optim in float64 to 1e-11 relative (the clamp of F.normalize at a zero row included);
* for every case and EVERY output element a float32 torch evaluation of the same formulas, in two summation orders (natural, and with every reduced axis
  reversed), sits inside the gate the GPU test holds the kernels to.  Prints the worst err / bound per case - all at most 1;
* for every query of every head case the float64 top-2 logit margin exceeds twice the row's logit allowance, which is what makes the exact accuracy
  comparison of the GPU test legitimate (rows that tie by construction excepted: tests/head_cases.py exact_tie_rows);
* the numpy soft-label reference equals a torch.topk construction where no ties exist, and resolves a hand-written tie as documented.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_cases as hc
from oracle import head_ops_oracle as ho


def _close(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def _torch_head(fs, fq, temp, method):
    p = fs.mean(2)
    if method == 'cos':
        return temp * F.normalize(fq, dim=-1) @ F.normalize(p, dim=-1).transpose(1, 2)
    if method == 'dot':
        return temp * fq @ p.transpose(1, 2)
    return -temp * (fq[:, :, None] - p[:, None]).pow(2).sum(-1)


# ----------------------------------------------------------------------------------------------------------------- references against torch, float64
@pytest.mark.parametrize('cid', ['D60', 'way17-Q17', 'Q33', 'shuffle', 'zero'])
@pytest.mark.parametrize('method', hc.METHODS)
def test_head_reference_equals_torch(cid, method):
    t = hc.head_inputs(cid)
    E, way, Q = hc.HEAD[cid]['E'], hc.HEAD[cid]['way'], hc.HEAD[cid]['Q']
    fs, fq = t['fs'].double().requires_grad_(True), t['fq'].double().requires_grad_(True)
    temp = torch.tensor(hc.head_temp(method, hc.HEAD[cid]['D']), dtype=torch.float64, requires_grad=True)
    L = _torch_head(fs, fq, temp, method)
    r = hc.head_reference(cid, method)
    _close(r['logits'], L.detach())
    _close(r['nll'], F.cross_entropy(L.detach().reshape(-1, way), t['labels'], reduction='none').reshape(E, Q))
    _close(r['loss'], r['nll'].mean(1))
    Ld = L.detach().clone().requires_grad_(True)
    F.cross_entropy(Ld.reshape(-1, way), t['labels']).backward()
    _close(r['dlogits'], Ld.grad)
    if method != 'dot':
        for up in (1.0, 3.0):
            b = hc.head_bwd_reference(cid, method, up)
            gs, gq, gt = torch.autograd.grad((L * t['dl'].double()).sum() * up, (fs, fq, temp), retain_graph=True)
            _close(b['dshot'], gs)
            _close(b['dq'], gq)
            _close(b['dtemp'].sum(), gt)


def test_misc_references_equal_torch():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(7, 12, dtype=torch.float64, generator=g).requires_grad_(True)
    w = torch.randn(5, 12, dtype=torch.float64, generator=g).requires_grad_(True)
    b = torch.randn(5, dtype=torch.float64, generator=g).requires_grad_(True)
    dy = torch.randn(7, 5, dtype=torch.float64, generator=g)
    y = F.linear(x, w, b)
    _close(ho.linear(x.detach(), w.detach(), b.detach())[0], y.detach())
    y.backward(dy)
    r = ho.linear_backward(dy, x.detach(), w.detach())
    _close(r['dx'], x.grad), _close(r['dw'], w.grad), _close(r['db'], b.grad)
    # soft-target CE
    z = (3 * torch.randn(6, 13, dtype=torch.float64, generator=g) + 80).requires_grad_(True)
    t = torch.rand(6, 13, dtype=torch.float64, generator=g)
    row = torch.sum(-t * F.log_softmax(z, dim=-1), dim=-1)
    (row.sum() * 0.25).backward()
    r = ho.soft_target_ce(z.detach(), t, 0.25)
    _close(r['row'], row.detach()), _close(r['dz'], z.grad)
    # row_normalize, its backward from (y, inv) and from x with torch's clamp - a zero row included
    x = torch.randn(5, 9, dtype=torch.float64, generator=g)
    x[2] = 0.0
    x = x.requires_grad_(True)
    dy = torch.randn(5, 9, dtype=torch.float64, generator=g)
    yn = F.normalize(x, dim=-1)
    yn.backward(dy)
    r = ho.row_normalize(x.detach())
    _close(r['y'], yn.detach())
    assert float(r['inv'][2]) == 1e12 and float(r['y'][2].abs().max()) == 0.0
    _close(ho.row_normalize_backward(r['y'], r['inv'], dy)[0] / 1e12, x.grad / 1e12)
    _close(ho.normalize_backward(x.detach(), dy) / 1e12, x.grad / 1e12)
    # pool_affine
    x = torch.randn(2, 7, 8, dtype=torch.float64, generator=g)
    sc, sh = torch.randn(8, dtype=torch.float64, generator=g), torch.randn(8, dtype=torch.float64, generator=g)
    _close(ho.pool_affine(x, sc, sh)[0], x.mean(1) * sc + sh)


def test_optimizer_references_equal_torch():
    g = torch.Generator().manual_seed(6)
    for momentum, wd, _ in hc.SGD_HYPER[::2]:
        p = torch.randn(33, dtype=torch.float64, generator=g)
        q = p.clone().requires_grad_(True)
        opt = torch.optim.SGD([q], lr=ho.f32(0.05), momentum=ho.f32(momentum), weight_decay=ho.f32(wd))
        buf = torch.zeros_like(p)
        for step in range(3):
            gr = torch.randn(33, dtype=torch.float64, generator=g)
            q.grad = gr.clone()
            opt.step()
            r = ho.sgd(p, gr, buf, 0.05, momentum, wd, step == 0)
            p, buf = r['p'], r['buf']
            _close(p, q.detach())
    h = hc.ADAMW_HYPER
    p = torch.randn(33, dtype=torch.float64, generator=g)
    q = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([q], lr=ho.f32(h['lr']), betas=(ho.f32(h['beta1']), ho.f32(h['beta2'])), eps=ho.f32(h['eps']), weight_decay=ho.f32(h['wd']))
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in range(1, 5):
        gr = torch.randn(33, dtype=torch.float64, generator=g)
        q.grad = gr.clone()
        opt.step()
        r = ho.adamw(p, gr, m, v, h['lr'], h['beta1'], h['beta2'], h['eps'], h['wd'], step, round_bc=False)
        p, m, v = r['p'], r['m'], r['v']
        _close(p, q.detach())
    # the once-rounded bias corrections of the launcher move the update by at most 2 u relative
    r2 = ho.adamw(p, gr, m, v, h['lr'], h['beta1'], h['beta2'], h['eps'], h['wd'], 5)
    r1 = ho.adamw(p, gr, m, v, h['lr'], h['beta1'], h['beta2'], h['eps'], h['wd'], 5, round_bc=False)
    assert float(((r2['p'] - r1['p']).abs() / (r1['p'] - p * (1 - ho.f32(h['lr']) * ho.f32(h['wd']))).abs().clamp_min(1e-30)).max()) <= 2.5 * ho.U


def test_softlabel_reference():
    for case in hc.SOFTLABEL:
        B, T, C, k, bp = case
        lt = hc.softlabel_inputs(case, 'random')
        got = ho.token_softlabel(lt.numpy(), k, bp, 0.1)
        off, on = np.float32(0.1 / C), np.float32(1.0 - 0.1 + 0.1 / C)
        want = torch.full((B, T, C + 1), float(off))
        pos = torch.zeros(B, T, dtype=torch.bool)
        if T - bp > 0:
            pos.scatter_(1, lt.max(-1).values.topk(T - bp, dim=1).indices, True)
        top = lt.topk(k, dim=-1).indices
        for b in range(B):
            for t in range(T):
                if pos[b, t]:
                    want[b, t, top[b, t]] = float(on)
                else:
                    want[b, t, 1] = float(on)
        assert np.array_equal(got, want.reshape(B * T, C + 1).numpy()), case
    # a hand-written tie: tokens 0 and 2 share the largest maximum, T - bp = 1 -> token 0 is the positive one; inside it classes 1 and 3 tie for second
    lt = np.array([[[5, 2, 1, 2], [0, 4, 0, 0], [1, 5, 0, 0]]], dtype=np.float32)
    got = ho.token_softlabel(lt, 2, 2, 0.1)
    on, off = np.float32(0.9 + 0.1 / 4), np.float32(0.1 / 4)
    assert np.array_equal(got, np.array([[on, on, off, off, off], [off, on, off, off, off], [off, on, off, off, off]], dtype=np.float32))


# ----------------------------------------------------------------------------------------------------------------- float32 evaluations inside the gates
def _worst(name, pairs):
    w = max(pairs.values())
    print(f'{name}: worst err/bound {w:.3f}  (' + ', '.join(f'{k} {v:.3f}' for k, v in pairs.items()) + ')')
    assert w <= 1.0, (name, pairs)


@pytest.mark.parametrize('cid', hc.head_ids())
@pytest.mark.parametrize('method', hc.METHODS)
def test_head_f32_inside_gate(cid, method):
    p = hc.HEAD[cid]
    t = hc.head_inputs(cid)
    temp = hc.head_temp(method, p['D'])
    r = hc.head_reference(cid, method)
    # the margin that makes the accuracy comparison exact
    margin, a_row = r['margin'].clone(), r['a_row']
    for q in hc.exact_tie_rows(cid, method):
        assert float(r['logits'][:, q].abs().max()) == 0.0
        margin[:, q] = math.inf
    assert bool((margin > 2.0 * a_row).all()), (cid, method, float((margin - 2.0 * a_row).min()))
    out = {}
    for order in ('natural', 'reversed'):
        fs, fq = (t['fs'], t['fq']) if order == 'natural' else (t['fs'].flip(-1).flip(2), t['fq'].flip(-1))
        f = ho.head_forward(fs, fq, temp, method, t['labels'])
        for k in ('logits', 'nll', 'loss', 'dlogits'):
            out[f'{k}/{order[0]}'] = hc.ratio(f[k], r[k], r['a_' + k])
        assert torch.equal(f['count'], r['count'])
        if method != 'dot' and p['bwd']:
            for up in (1.0, 3.0):
                b = hc.head_bwd_reference(cid, method, up)
                f = ho.head_backward(fs, fq, t['dl'], temp, method, up)
                if order == 'reversed':
                    f['dshot'], f['dq'] = f['dshot'].flip(-1).flip(2), f['dq'].flip(-1)
                for k in ('dshot', 'dq', 'dtemp'):
                    out[f'{k}*{up:g}/{order[0]}'] = hc.ratio(f[k], b[k], b['a_' + k])
    _worst(f'head {cid} {method}', out)


@pytest.mark.parametrize('shape', hc.POOL_SHAPES)
@pytest.mark.parametrize('dt', list(hc.POOL_DTYPES))
def test_pool_affine_f32_inside_gate(shape, dt):
    x, sc, sh = hc.pool_inputs(shape, dt)
    A, a = ho.pool_affine(x.double(), sc.double(), sh.double())
    _worst(f'pool_affine {shape} {dt}', {'n': hc.ratio(ho.pool_affine(x.float(), sc, sh)[0], A, a),
                                         'r': hc.ratio(ho.pool_affine(x.float().flip(1), sc, sh)[0], A, a)})


@pytest.mark.parametrize('case', hc.LINEAR, ids=str)
def test_linear_f32_inside_gate(case):
    t = hc.linear_inputs(case)
    d = {k: (None if v is None else v.double()) for k, v in t.items()}
    y, a_y = ho.linear(d['x'], d['w'], d['b'])
    r = ho.linear_backward(d['dy'], d['x'], d['w'])
    out = {}
    for order in 'nr':
        fl = (lambda v, dim: v) if order == 'n' else (lambda v, dim: v.flip(dim))
        out['y/' + order] = hc.ratio(ho.linear(fl(t['x'], 1), fl(t['w'], 1), t['b'])[0], y, a_y)
        out['dx/' + order] = hc.ratio(ho.linear_backward(fl(t['dy'], 1), t['x'], fl(t['w'], 0))['dx'], r['dx'], r['a_dx'])
        f = ho.linear_backward(fl(t['dy'], 0), fl(t['x'], 0), t['w'])
        out['dw/' + order] = hc.ratio(f['dw'], r['dw'], r['a_dw'])
        out['db/' + order] = hc.ratio(f['db'], r['db'], r['a_db'])
    _worst(f'linear {case}', out)


def test_fma_emulation_and_weight_gradient_bits():
    """_fma32 rounds a * b + s once (checked against exact rational arithmetic); linear_dw_bits sits inside the float64 gate on both of its paths"""
    from fractions import Fraction
    g = np.random.default_rng(7)
    a, b = g.standard_normal(400).astype(np.float32), g.standard_normal(400).astype(np.float32)
    s = (-(a.astype(np.float64) * b) + g.standard_normal(400) * np.logspace(-12, 0, 400)).astype(np.float32)          # cancelling sums: the hard roundings
    got = ho._fma32(a, b, s)
    for i in range(400):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(s[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        assert abs(Fraction(float(got[i])) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact)), i
    for case in hc.LINEAR_BITS:
        t = hc.linear_inputs(case)
        dw, db = ho.linear_dw_bits(t['dy'].numpy(), t['x'].numpy())
        r = ho.linear_backward(t['dy'].double(), t['x'].double(), t['w'].double())
        _worst(f'linear_dw_bits {case}', {'dw': hc.ratio(torch.from_numpy(dw), r['dw'], r['a_dw']), 'db': hc.ratio(torch.from_numpy(db), r['db'], r['a_db'])})


@pytest.mark.parametrize('shape', hc.STCE_SHAPES, ids=str)
def test_soft_target_ce_f32_inside_gate(shape):
    out = {}
    for offset in hc.STCE_OFFSETS:
        for target in hc.STCE_TARGETS:
            z, t = hc.stce_inputs(shape, offset, target)
            gs = 1.0 / shape[0]
            r = ho.soft_target_ce(z.double(), t.double(), gs)
            for order in 'nr':
                f = ho.soft_target_ce(z if order == 'n' else z.flip(1), t if order == 'n' else t.flip(1), gs)
                out[f'row{offset:+g}{target[0]}/{order}'] = hc.ratio(f['row'], r['row'], r['a_row'])
                out[f'dz{offset:+g}{target[0]}/{order}'] = hc.ratio(f['dz'] if order == 'n' else f['dz'].flip(1), r['dz'], r['a_dz'])
    _worst(f'soft_target_ce {shape}', out)


@pytest.mark.parametrize('shape', hc.ROWNORM_SHAPES, ids=str)
@pytest.mark.parametrize('zero', (False, True))
def test_row_normalize_f32_inside_gate(shape, zero):
    x, dy = hc.rownorm_inputs(shape, zero)
    n = x.double().norm(dim=1)
    assert bool(((n >= 1e-6) | (n == 0)).all())
    r = ho.row_normalize(x.double())
    yk, ik = r['y'].float(), r['inv'].float()                    # what the backward is handed: the forward's outputs in fp32
    dx, a_dx = ho.row_normalize_backward(yk.double(), ik.double(), dy.double())
    out = {}
    for order in 'nr':
        fl = (lambda v: v) if order == 'n' else (lambda v: v.flip(1))
        f = ho.row_normalize(fl(x))
        out['y/' + order] = hc.ratio(fl(f['y']), r['y'], r['a_y'])
        out['inv/' + order] = hc.ratio(f['inv'], r['inv'], r['a_inv'])
        out['dx/' + order] = hc.ratio(fl(ho.row_normalize_backward(fl(yk), ik, fl(dy))[0]), dx, a_dx)
    if zero:
        z = shape[0] // 2
        assert float(r['y'][z].abs().max()) == 0.0 and float(r['inv'][z]) == 1e12 and np.float32(1e12) == ik[z].item()
        assert torch.equal(dx[z], dy[z].double() * float(ik[z]))
    _worst(f'row_normalize {shape} zero={zero}', out)


@pytest.mark.parametrize('n', hc.OPT_N)
def test_optimizers_f32_inside_gate(n):
    out = {}
    for momentum, wd, first in hc.SGD_HYPER:
        s = hc.opt_state(n, (momentum, wd, first))
        r = ho.sgd(s['p'].double(), s['g'].double(), s['buf'].double(), 0.05, momentum, wd, first)
        f = ho.sgd(s['p'], s['g'], s['buf'], 0.05, momentum, wd, first)
        out[f'sgd{momentum}/{wd}/{int(first)}'] = max(hc.ratio(f['p'], r['p'], r['a_p']), hc.ratio(f['buf'], r['buf'], r['a_buf']))
    h = hc.ADAMW_HYPER
    for step in hc.ADAMW_STEPS if n <= 257 else (1,):
        s = hc.adamw_state(n, step)
        a = (h['lr'], h['beta1'], h['beta2'], h['eps'], h['wd'], step)
        r = ho.adamw(s['p'].double(), s['g'].double(), s['m'].double(), s['v'].double(), *a)
        f = ho.adamw(s['p'], s['g'], s['m'], s['v'], *a)
        out[f'adamw@{step}'] = max(hc.ratio(f[k], r[k], r['a_' + k]) for k in 'pmv')
        z = s['zero_from']
        out[f'decay@{step}'] = hc.ratio(hc.f32_decay(s['p'][z:], h['lr'], h['wd']), r['p'][z:], r['a_p'][z:])      # g = m = v = 0: the decay alone
    _worst(f'optimizers n={n}', out)
