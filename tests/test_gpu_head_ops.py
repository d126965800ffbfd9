"""The kernels that produce the numbers users read - few-shot accuracy, the losses, the parameter updates: feat_out.hip (pool_affine), head.hip (proto_head
and its fused cross entropy, both head backwards), token_label.hip (linear forward / backward, token soft labels, soft-target CE, row_normalize) and the
SGD and AdamW updates of optim.hip - against the float64 references of oracle/head_ops_oracle.py, through the ops.* entry points, over the tables of
tests/head_cases.py (the edges each case reaches are written next to it there).

Every case asserts, in this order: the output is finite; three launches are bit-identical; PAD canary elements behind every output buffer are untouched
(the wrappers allocate their outputs themselves: _guard hands torch.empty / empty_like / full a canary-tailed buffer for the duration of the call); for
the per-episode / per-row kernels, episodes / rows 1 .. launched alone reproduce those outputs bit for bit (dlogits of the fused head carries 1 / (E Q)
and the batch means stats[0:2] / dtemp[E] sum over episodes: those are gated instead, the means as the fixed-order sums they document); after every
fused-CE launch ops._ticket(dev) is zero; then the gates.

GATES: |got - A| <= a + u |A|, u = 2^-24, A the float64 result from the fp32 inputs, a from float64 quantities only (oracle/head_ops_oracle.py; no constant
comes from a kernel run; tests/test_head_ops_ref_cpu.py holds a float32 evaluation in two summation orders inside them for every case and element).
sum_tol(t, n) = 4 sqrt(n) u t, dot(t, n) = sum_tol(t, n) + u t, E = 2^-20 per expf / logf / sqrtf / reciprocal or division, nD = ceil(D / 64) + 6 the
chain of a lane-strided wave reduction.  |.| of a vector or matrix is elementwise; "x^" is x / max(|x|, 1e-12).
  prototype p        a_p    = dot(sum_k |f_ck|, shot) / shot + u |p|
  inverse norm       r(x)   = (4 sqrt(nD) u + u + 2 sum_d |x_d| a_x_d / sum x^2) / 2 + 2 E      relative; zero row: 2 E (1 / 1e-12f is fp32(1e12) to 4e-9)
  p^                 a_p^   = a_p / |p| + |p^| (r(p) + u)
  cos logits         a_l    = T (sum_d |q^_d| a_p^_d + t (r(q) + u) + dot(t, nD)) + u |l|,  t = sum_d |q^_d p^_d|, T the temperature
  dot logits         a_l    = T (sum_d |q_d| a_p_d + dot(sum_d |q_d p_d|, nD)) + u |l|
  sqr logits         a_l    = T (sum_d 2 |df_d| (a_p_d + u |df_d|) + dot(sum_d df_d^2, nD)) + u |l|,  df = q - p
  per-query NLL      a_nll  = sum_c P_c a_l_c + a_l_label + r_se + E |log se| + u |lse| + u |nll|,  r_se = sum_c P_c (u |l_c - max| + E) + 4 sqrt(way) u
                     (not an output of its own: it is gated through the per-episode loss; at Q = 1 they are the same number)
  per-episode loss   a_loss = mean_q a_nll + dot(sum_q |nll|, Q) / Q + u |loss|
  dlogits            a_dl   = (P_c (a_l_c + sum_c' P_c' a_l_c') + P_c (u |l_c - max| + E + r_se + E + u) + u |P_c - 1hot|) / (E Q) + (E + u) |dl|
  cos backward       a_s    = sum_d |q^_d| a_p^_d + s_abs (r(q) + u) + dot(s_abs, nD)                    s_qc = <q^, p^_c>, T' = T * dloss
    dq^ = T' dl p^   a_g    = |T' dl| a_p^ + dot(G, way) + 3 u G,  G = |T' dl| |p^|;   <q^, dq^>: a_dot = sum_c |T' dl_c| a_s_c + dot(DA, way) + 3 u DA
    dq               a_dq   = (a_g + |q^| a_dot + |q^ <q^, dq^>| (r(q) + 2 u) + u |dq^ - q^ <q^, dq^>|) / |q| + |dq| (r(q) + u)   (zero row: 1 / |q| = 1e12)
    dtemp[e]         a_dt   = |dloss| (sum_qc |dl| a_s + dot(sum_qc |dl s|, ceil(Q / 16) way + 16)) + 2 u |dtemp|
    dp^              a_dp^  = |T'| (sum_q |dl q^_d| (r(q) + 2 u) + sum_tol(sum_q |dl q^_d|, Q)) + 2 u |dp^|;   <p^, dp^> as a dot over D with both allowances
    dshot            a      = ((a_dp^ + a_p^ |dot| + |p^| a_dot + u |p^ dot| + u |dp^ - p^ dot|) / |p| + |dp| (r(p) + 2 u)) / shot + u |dp| / shot
  sqr backward       a_dq   = 2 |T'| (sum_c |dl_c| (a_p + u |df|) + dot(sum_c |dl_c df|, way)) + 3 u |dq|;   dshot the same over q with chain Q, / shot, 4 u
    dtemp[e]         a_dt   = |dloss| (sum_qc |dl| (sum_d 2 |df| (a_p + u |df|) + dot(sum df^2, nD)) + dot(sum_qc |dl| |df|^2, ceil(Q / 4) way + 4)) + 2 u |dtemp|
  batch means        |got - mean_e got_e| <= sum_tol(sum_e |got_e|, E) / E + 2 u |mean|;  dtemp[E]: sum_tol(sum_e |dtemp_e|, E) + u |sum|
  pool_affine        a = |scale| (sum_tol(sum_p |x_p|, HW) / HW + (E + u) |mean|) + u |mean scale| + u |y|
  linear             y: dot(sum_k |x_k w_k|, 4 ceil(K / 256) + 6) + u |y|;  dx: dot(sum_n |dy_n w_nk|, N);  dw, db: dot / sum_tol over the rows with chain M below
                     256 rows and rows_per_slab + slabs from there;  accumulate_dx: A = prefill + dx
  soft-target CE     a_row = |st| a_lse + |lse| a_st + u |lse st| + a_tz + u |row|,  a_lse = r_se + E |log se| + u |lse|, a_st = sum_tol(sum |t|, nC),
                     a_tz = dot(sum |t z|, nC);  a_dz = |gs| (P |st| (u |z - max| + E + r_se + 2 E + u) + P a_st + u |P st - t|) + u |dz|
  row_normalize      a_y = |y| (r(x) + u), a_inv = inv r(x);  backward from the forward's fp32 (y, inv): a_dx = inv (|y| dot(sum |y dy|, nD) + u |y d| + u |dy - y d|) + u |dx|
  SGD                a_d = u |wd p| + u |d|, a_buf = a_d + u |mom buf| + u |buf'|, a_p = lr a_buf + u |lr buf'| + u |p'|
  AdamW              a_pi = |p| (u lr wd + u (1 - lr wd)) + u |pi|, a_m = 2 u (|b1 m| + |(1 - b1) g|) + u |m'|, a_v = u b2 v + 3 u (1 - b2) g^2 + u v',
                     a_sqrt = a_v / (2 sqrt v') + E sqrt v', a_den = rs a_sqrt + u rs sqrt v' + u den, a_q = a_m / den + |q| a_den / den + E |q|,
                     a_p = a_pi + (lr / bc1) a_q + |upd| (E + u) + u |p'|;  hyperparameters rounded to fp32, bc1 and rs = 1 / sqrt(bc2) formed in double, rounded once

Accuracy is compared exactly (acc[e] Q = the float64 count of first maxima equal to the label); the CPU test asserts the margin that makes it legitimate.
token_softlabel is compared with array_equal against numpy's stable argsort: torch.topk's tie order is unspecified, which is why the golden files (random
floats, compared against torch.topk) cannot cover the documented tie rule; the 'grid' inputs here are small integers with many ties.

Each test prints `op, case, worst err/bound`.
"""
import math

import numpy as np
import pytest
import torch

import head_cases as hc
import sgd_cases
from oracle import head_ops_oracle as ho

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CANARY = 24576.0
PAD = 64


def _ops():
    from fewshot_vit_amd.engine import ops
    return ops


class _Guard:
    """for the duration of `with`: torch.empty / empty_like / full return the head of a canary-filled buffer with PAD canary elements behind it"""

    def __enter__(self):
        self.bufs, self._orig = [], (torch.empty, torch.empty_like, torch.full)
        empty, _, full = self._orig

        def alloc(shape, dtype, device, fill=None):
            shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else tuple(shape)
            n = int(np.prod(shape)) if shape else 1
            buf = full((n + PAD,), CANARY, dtype=dtype or torch.float32, device=device)
            if fill is not None:
                buf[:n] = fill
            self.bufs.append((buf, n, fill is None))
            return buf[:n].view(shape)

        torch.empty = lambda *shape, dtype=None, device=None: alloc(shape, dtype, device)
        torch.empty_like = lambda x: alloc(x.shape, x.dtype, x.device)
        torch.full = lambda shape, v, dtype=None, device=None: alloc(shape, dtype, device, fill=v)
        return self

    def __exit__(self, *exc):
        torch.empty, torch.empty_like, torch.full = self._orig

    def check(self):
        torch.cuda.synchronize()
        for buf, n, _ in self.bufs:
            assert bool((buf[n:] == CANARY).all()), 'elements behind an output buffer were written'

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((buf == CANARY).all()) for buf, _, was_empty in self.bufs if was_empty)


def _g(fn):
    """run an ops call with guarded allocations; check the canaries; -> its result"""
    with _Guard() as gd:
        out = fn()
    gd.check()
    return out


def _bits(x):
    return x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x


def _same(a, b):
    """bit equality of two tensors or tuples of tensors (NaN equals the same NaN; None equals None)"""
    a, b = (a if isinstance(a, (tuple, list)) else (a,)), (b if isinstance(b, (tuple, list)) else (b,))
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and torch.equal(_bits(x), _bits(y))) for x, y in zip(a, b))


def _finite(*ts):
    for t in ts:
        assert bool(torch.isfinite(t).all())


def _report(name, pairs):
    w = max(pairs.values())
    print(f'{name}: worst err/bound {w:.3f}  (' + ', '.join(f'{k} {v:.3f}' for k, v in pairs.items()) + ')')
    assert w <= 1.0, (name, pairs)


def _ticket_zero():
    torch.cuda.synchronize()
    assert int(_ops()._ticket(torch.device(DEV, torch.cuda.current_device())).abs().sum()) == 0


# ----------------------------------------------------------------------------------------------------------------- head forward
def _head_dev(cid):
    t = hc.head_inputs(cid)
    return t, {k: t[k].to(DEV) for k in ('fs', 'fq', 'labels', 'dl')}


def _stats_gate(stats, E):
    """stats = {loss, acc, acc per episode .., loss per episode ..}: the two means as in-order sums of the per-episode values the kernel wrote"""
    s = stats.double().cpu()
    out = {}
    for name, mean, per in (('mean_loss', s[0], s[2 + E:]), ('mean_acc', s[1], s[2:2 + E])):
        A, a = ho.fixed_order_mean(per)
        out[name] = abs(float(mean) - A) / a if a > 0 else (0.0 if float(mean) == A else math.inf)
    return out


@pytest.mark.parametrize('cid', hc.head_ids())
@pytest.mark.parametrize('method', hc.METHODS)
def test_head_forward(cid, method):
    ops = _ops()
    p = hc.HEAD[cid]
    E, way, Q = p['E'], p['way'], p['Q']
    t, d = _head_dev(cid)
    temp = hc.head_temp(method, p['D'])
    lab = d['labels'] if t['explicit'] else None
    ce = lambda fs=d['fs'], fq=d['fq'], tv=temp, lb=lab: _g(lambda: ops.proto_head_ce(fs, fq, tv, lb, method))
    logits, dlogits, stats = ce()
    _ticket_zero()
    _finite(logits, dlogits, stats)
    for _ in range(2):
        assert _same(ce(), (logits, dlogits, stats))
        _ticket_zero()
    # both entry points and both temperature forms give the same bits; explicit make_nk_label labels equal the default
    tdev = torch.tensor(temp, dtype=torch.float32, device=DEV)
    assert _same(ce(tv=tdev), (logits, dlogits, stats))
    l2, acc2, loss2 = _g(lambda: ops.proto_head(d['fs'], d['fq'], temp, method))
    assert _same(_g(lambda: ops.proto_head(d['fs'], d['fq'], tdev, method)), (l2, acc2, loss2))
    assert torch.equal(l2, logits)
    if not t['explicit']:
        assert torch.equal(acc2, stats[2:2 + E]) and torch.equal(loss2, stats[2 + E:])
        assert _same(ce(lb=d['labels']), (logits, dlogits, stats))
    _ticket_zero()
    if E > 1:                                                                  # episodes 1 .. alone
        ls, _, ss = ce(fs=d['fs'][1:], fq=d['fq'][1:], lb=None if lab is None else lab[Q:])
        assert torch.equal(ls, logits[1:]) and torch.equal(ss[2:1 + E], stats[3:2 + E]) and torch.equal(ss[1 + E:], stats[3 + E:])
        l3, a3, s3 = _g(lambda: ops.proto_head(d['fs'][1:], d['fq'][1:], temp, method))
        assert _same((l3, a3, s3), (l2[1:], acc2[1:], loss2[1:]))
    r = hc.head_reference(cid, method)
    out = {'logits': hc.ratio(logits.cpu(), r['logits'], r['a_logits']), 'loss': hc.ratio(stats[2 + E:].cpu(), r['loss'], r['a_loss']),
           'dlogits': hc.ratio(dlogits.cpu(), r['dlogits'], r['a_dlogits'])}
    out.update(_stats_gate(stats, E))
    accq = stats[2:2 + E].double().cpu() * Q
    assert torch.equal(accq.round(), r['count']) and float((accq - r['count']).abs().max()) <= Q * hc.U, (accq, r['count'])
    if p['special'] == 'zero' and method == 'cos':                                # the eps clamp: exactly 0 for the zero query row and the zero class column
        assert float(logits[:, 1].abs().max()) == 0.0 and float(logits[:, :, 2].abs().max()) == 0.0
    _report(f'head_forward {cid} {method}', out)


@pytest.mark.parametrize('method', hc.METHODS)
def test_head_tie_takes_first_maximum(method):
    """classes 1 and 3 hold bit-identical shots: argmax must take class 1 (the first maximum, as torch.argmax), so the per-episode accuracy is exactly the
    number of queries labelled 1"""
    ops = _ops()
    t = hc.tie_inputs()
    fs, fq, lab = t['fs'].to(DEV), t['fq'].to(DEV), t['labels'].to(DEV)
    E, Q = fq.shape[:2]
    logits, _, stats = _g(lambda: ops.proto_head_ce(fs, fq, hc.head_temp(method, fq.shape[2]), lab, method))
    _ticket_zero()
    assert torch.equal(logits[:, :, 1], logits[:, :, 3])
    assert bool((logits.max(-1).values == logits[:, :, 1]).all()), 'the tied pair is not the maximum: the case tests nothing'
    assert torch.equal((stats[2:2 + E].double().cpu() * Q).round(), t['count']), stats


def test_head_lds_limit_refused():
    """(64 * 640 + 2) * 4 = 163 848 bytes of LDS: one step above 160 KB raises and leaves the outputs untouched (lds160k is the accepted side); the cosine
    backward of 40-way at D 512 needs 2 * 40 * 512 floats = 160 KB + and is refused the same way, while its 'sqr' form (80 KB) runs."""
    ops = _ops()
    p = hc.HEAD_FWD_REFUSED
    t = hc.head_inputs('refused-fwd', p)
    fs, fq = t['fs'].to(DEV), t['fq'].to(DEV)
    for call in (lambda: ops.proto_head_ce(fs, fq, 10.0, None, 'cos'), lambda: ops.proto_head(fs, fq, 10.0, 'sqr')):
        with _Guard() as gd:
            with pytest.raises((ValueError, RuntimeError)):
                call()
        gd.check()
        assert gd.untouched()
    _ticket_zero()
    t = hc.head_inputs('refused-bwd', hc.HEAD_BWD_REFUSED)
    fs, fq, dl = t['fs'].to(DEV), t['fq'].to(DEV), t['dl'].to(DEV)
    for call in (lambda: ops.proto_head_backward(fs, fq, dl, 10.0, 'cos'), lambda: ops.proto_head_ce_backward(fs, fq, dl, None, 10.0, 'cos')):
        with _Guard() as gd:
            with pytest.raises((ValueError, RuntimeError)):
                call()
        gd.check()
        assert gd.untouched()
    _ticket_zero()
    ds, dq, _ = _g(lambda: ops.proto_head_backward(fs, fq, dl, 0.01, 'sqr'))
    _finite(ds, dq)


# ----------------------------------------------------------------------------------------------------------------- head backward
@pytest.mark.parametrize('cid', hc.head_ids(bwd=True))
@pytest.mark.parametrize('method', ('cos', 'sqr'))
def test_head_backward(cid, method):
    ops = _ops()
    p = hc.HEAD[cid]
    E = p['E']
    t, d = _head_dev(cid)
    temp = hc.head_temp(method, p['D'])

    def ce_bwd(up, fs=d['fs'], fq=d['fq'], dl=d['dl'], tv=temp):
        dloss = None if up is None else torch.tensor([up], dtype=torch.float32, device=DEV)
        ds, dq, dt = _g(lambda: ops.proto_head_ce_backward(fs, fq, dl, dloss, tv, method))
        _ticket_zero()
        n = fs.shape[0]
        assert dt.data_ptr() == dt._base.data_ptr() + 4 * n
        return ds, dq, dt._base[:n + 1]                  # dtemp per episode and, behind them, their sum

    base = ce_bwd(None)
    _finite(*base)
    for _ in range(2):
        assert _same(ce_bwd(None), base)
    assert _same(ce_bwd(1.0), base)                                               # dloss = None is dloss = 1
    assert _same(ce_bwd(None, tv=torch.tensor(temp, dtype=torch.float32, device=DEV)), base)
    ds2, dq2, dts = _g(lambda: ops.proto_head_backward(d['fs'], d['fq'], d['dl'], temp, method))       # the unfused entry: the same kernel
    assert torch.equal(ds2, base[0]) and torch.equal(dq2, base[1])
    assert _same(_g(lambda: ops.proto_head_backward(d['fs'], d['fq'], d['dl'], torch.tensor(temp, dtype=torch.float32, device=DEV), method))[:2], (ds2, dq2))
    if E > 1:                                                                  # episodes 1 .. alone
        sub = ce_bwd(None, fs=d['fs'][1:], fq=d['fq'][1:], dl=d['dl'][1:])
        assert torch.equal(sub[0], base[0][1:]) and torch.equal(sub[1], base[1][1:]) and torch.equal(sub[2][:E - 1], base[2][1:E])
    out = {}
    for up in (1.0, 3.0):
        ds, dq, dt = base if up == 1.0 else ce_bwd(up)
        r = hc.head_bwd_reference(cid, method, up)
        out[f'dshot*{up:g}'] = hc.ratio(ds.cpu(), r['dshot'], r['a_dshot'])
        out[f'dq*{up:g}'] = hc.ratio(dq.cpu(), r['dq'], r['a_dq'])
        out[f'dtemp*{up:g}'] = hc.ratio(dt[:E].cpu(), r['dtemp'], r['a_dtemp'])
        A, a = ho.fixed_order_sum(dt[:E].cpu())
        out[f'dtemp_sum*{up:g}'] = abs(float(dt[E]) - A) / a if a > 0 else (0.0 if float(dt[E]) == A else math.inf)
        if up == 1.0:                                                             # the unfused entry sums dtemp with torch: any order
            tot = float(r['a_dtemp'].sum()) + ho.sum_tol(float(r['dtemp'].abs().sum()), E)
            out['dtemp_total'] = hc.ratio(dts.cpu(), r['dtemp'].sum(), tot)
    if p['special'] == 'zero':
        r = hc.head_bwd_reference(cid, method, 1.0)
        assert float(base[1][:, 3].abs().max()) == 0.0                             # a zero dlogits row: exactly no query gradient
        if method == 'cos':                                                       # the zero query row: dq = dq^ * 1e12 (the reference clamps as torch does)
            assert float(r['dq'][:, 1].abs().max()) > 1e9
    _report(f'head_backward {cid} {method}', out)


def test_head_wrappers_normalise_their_inputs():
    """feat_shot as a permuted view, feat_query and dlogits as strided slices, a float64 device temperature: all four wrappers give the bits of the
    contiguous fp32 copies (they used to hand data_ptr() of whatever they were given to the kernels)"""
    ops = _ops()
    t, d = _head_dev('shuffle')
    E, way, shot, D = d['fs'].shape
    fs_nc = d['fs'].permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    fq_nc = torch.stack((d['fq'], d['fq'] + 1.0), dim=2).reshape(E, -1, D)[:, ::2]
    dl_nc = torch.stack((d['dl'], d['dl'] - 1.0), dim=3)[..., 0]
    assert not fs_nc.is_contiguous() and not fq_nc.is_contiguous() and not dl_nc.is_contiguous()
    assert torch.equal(fs_nc, d['fs']) and torch.equal(fq_nc, d['fq']) and torch.equal(dl_nc, d['dl'])
    dloss = torch.tensor([3.0], dtype=torch.float32, device=DEV)
    for method in ('cos', 'sqr'):
        temp = hc.head_temp(method, D)
        t64 = torch.tensor(temp, dtype=torch.float64, device=DEV)
        for tv in (temp, t64):
            assert _same(_g(lambda: ops.proto_head(fs_nc, fq_nc, tv, method)), _g(lambda: ops.proto_head(d['fs'], d['fq'], temp, method)))
            assert _same(_g(lambda: ops.proto_head_ce(fs_nc, fq_nc, tv, d['labels'], method)), _g(lambda: ops.proto_head_ce(d['fs'], d['fq'], temp, d['labels'], method)))
            assert _same(_g(lambda: ops.proto_head_backward(fs_nc, fq_nc, dl_nc, tv, method)), _g(lambda: ops.proto_head_backward(d['fs'], d['fq'], d['dl'], temp, method)))
            got = _g(lambda: ops.proto_head_ce_backward(fs_nc, fq_nc, dl_nc, dloss, tv, method))
            assert all(x.is_contiguous() for x in got[:2])
            assert _same(got, _g(lambda: ops.proto_head_ce_backward(d['fs'], d['fq'], d['dl'], dloss, temp, method)))
        # bf16 features: read as their fp32 values
        want = _g(lambda: ops.proto_head_ce_backward(d['fs'].bfloat16().float(), d['fq'].bfloat16().float(), d['dl'], dloss, temp, method))
        assert _same(_g(lambda: ops.proto_head_ce_backward(d['fs'].bfloat16(), d['fq'].bfloat16(), d['dl'], dloss, temp, method)), want)
    _ticket_zero()


def test_head_backward_refuses_empty_dimensions():
    """way, shot or Q = 0 through every backward entry: FSVIT_ERR_ARG and untouched outputs (shot = 0 used to divide by it)"""
    from fewshot_vit_amd import _lib
    from fewshot_vit_amd.engine import _ptr, _stream_ptr
    ops, lib = _ops(), _lib.load()
    st = _stream_ptr(torch.device(DEV))
    E, way, shot, Q, D = 2, 5, 2, 5, 64
    fs, fq, dl = torch.randn(E, way, shot, D, device=DEV), torch.randn(E, Q, D, device=DEV), torch.randn(E, Q, way, device=DEV)
    tdev = torch.tensor([10.0], device=DEV)
    ds, dq, dt = torch.full_like(fs, CANARY), torch.full_like(fq, CANARY), torch.full((E + 1,), CANARY, device=DEV)
    tk = ops._ticket(torch.device(DEV, torch.cuda.current_device()))
    for kw in (dict(way=0), dict(shot=0), dict(Q=0), dict(way=-1), dict(D=0)):
        a = dict(way=way, shot=shot, Q=Q, D=D)
        a.update(kw)
        dims = (E, a['way'], a['shot'], a['Q'], a['D'])
        rcs = [lib.fsvit_proto_head_backward(_ptr(fs), _ptr(fq), _ptr(dl), *dims, 10.0, _ptr(ds), _ptr(dq), _ptr(dt), st),
               lib.fsvit_proto_head_backward_sqr(_ptr(fs), _ptr(fq), _ptr(dl), *dims, 10.0, _ptr(ds), _ptr(dq), _ptr(dt), st),
               lib.fsvit_proto_head_backward_devtemp(_ptr(fs), _ptr(fq), _ptr(dl), *dims, _ptr(tdev), _lib.HEAD_COS, _ptr(ds), _ptr(dq), _ptr(dt), st),
               lib.fsvit_proto_head_backward_devtemp(_ptr(fs), _ptr(fq), _ptr(dl), *dims, _ptr(tdev), _lib.HEAD_SQR, _ptr(ds), _ptr(dq), _ptr(dt), st),
               lib.fsvit_proto_head_ce_backward(_ptr(fs), _ptr(fq), _ptr(dl), None, *dims, 10.0, None, _lib.HEAD_COS, _ptr(ds), _ptr(dq), _ptr(dt), tk.data_ptr() + 4, st),
               lib.fsvit_proto_head_ce_backward(_ptr(fs), _ptr(fq), _ptr(dl), None, *dims, 10.0, None, _lib.HEAD_SQR, _ptr(ds), _ptr(dq), _ptr(dt), tk.data_ptr() + 4, st)]
        torch.cuda.synchronize()
        assert rcs == [_lib.ERR_ARG] * 6, (kw, rcs)
        assert lib.fsvit_last_error().decode() != ''
        assert bool((ds == CANARY).all()) and bool((dq == CANARY).all()) and bool((dt == CANARY).all()), kw
    _ticket_zero()
    for shape_s, shape_q, shape_l in (((E, 0, shot, D), (E, Q, D), (E, Q, 0)), ((E, way, 0, D), (E, Q, D), (E, Q, way)), ((E, way, shot, D), (E, 0, D), (E, 0, way))):
        a, b, c = torch.zeros(shape_s, device=DEV), torch.zeros(shape_q, device=DEV), torch.zeros(shape_l, device=DEV)
        for method in ('cos', 'sqr'):
            with pytest.raises(ValueError):
                ops.proto_head_backward(a, b, c, 10.0, method)
            with pytest.raises(ValueError):
                ops.proto_head_backward(a, b, c, tdev, method)
            with pytest.raises(ValueError):
                ops.proto_head_ce_backward(a, b, c, None, 10.0, method)
    _ticket_zero()


# ----------------------------------------------------------------------------------------------------------------- pool_affine
@pytest.mark.parametrize('shape', hc.POOL_SHAPES, ids=str)
@pytest.mark.parametrize('dt', list(hc.POOL_DTYPES))
def test_pool_affine(shape, dt):
    ops = _ops()
    x, sc, sh = hc.pool_inputs(shape, dt)
    xd, scd, shd = x.to(DEV), sc.to(DEV), sh.to(DEV)
    got = _g(lambda: ops.pool_affine(xd, scd, shd))
    _finite(got)
    for _ in range(2):
        assert torch.equal(_g(lambda: ops.pool_affine(xd, scd, shd)), got)
    if shape[0] > 1:
        assert torch.equal(_g(lambda: ops.pool_affine(xd[1:], scd, shd)), got[1:])
    A, a = ho.pool_affine(x.double(), sc.double(), sh.double())
    _report(f'pool_affine {shape} {dt}', {'feat': hc.ratio(got.cpu(), A, a)})


def test_pool_affine_refusals():
    from fewshot_vit_amd import _lib
    from fewshot_vit_amd.engine import _ptr, _stream_ptr
    ops, lib = _ops(), _lib.load()
    sc = torch.ones(8, device=DEV)
    out = torch.full((2, 8), CANARY, device=DEV)
    x = torch.ones(2, 4, 8, device=DEV)
    for HW, C in ((0, 8), (-1, 8), (4, 6), (4, 0)):                                 # HW = 0 used to divide by it
        assert lib.fsvit_pool_affine(_ptr(x), _ptr(sc), _ptr(sc), _ptr(out), 2, HW, C, _lib.F32, _stream_ptr(torch.device(DEV))) == _lib.ERR_ARG, (HW, C)
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    with pytest.raises(ValueError):
        ops.pool_affine(torch.ones(2, 0, 8, device=DEV), sc, sc)
    with pytest.raises(ValueError):
        ops.pool_affine(torch.ones(2, 4, 6, device=DEV), sc[:6], sc[:6])


# ----------------------------------------------------------------------------------------------------------------- linear
@pytest.mark.parametrize('case', hc.LINEAR, ids=str)
def test_linear(case):
    ops = _ops()
    M, N, K, bias = case
    t = hc.linear_inputs(case)
    d = {k: (None if v is None else v.to(DEV)) for k, v in t.items()}
    fwd = lambda x=d['x']: _g(lambda: ops.linear(x, d['w'], d['b']))
    bwd = lambda dy=d['dy'], x=d['x'], **kw: _g(lambda: ops.linear_backward(dy, x, d['w'], **kw))
    y, (dx, dw, db) = fwd(), bwd()
    _finite(y, dx, dw, db)
    for _ in range(2):
        assert torch.equal(fwd(), y) and _same(bwd(), (dx, dw, db))
    if M > 1:                                                                  # rows 1 .. alone: y and dx are per row
        assert torch.equal(fwd(d['x'][1:]), y[1:]) and torch.equal(bwd(d['dy'][1:], d['x'][1:], need_dw=False)[0], dx[1:])
    # the need_* switches change nothing in what is still computed
    assert _same(bwd(need_dw=False), (dx, None, None)) and _same(bwd(need_dx=False), (None, dw, db)) and _same(bwd(need_db=False), (dx, dw, None))
    if case in hc.LINEAR_BITS:                            # the documented summation order, bit for bit: serial below 256 rows, slabs from 256
        dwb, dbb = ho.linear_dw_bits(t['dy'].numpy(), t['x'].numpy())
        assert np.array_equal(dw.cpu().numpy(), dwb) and np.array_equal(db.cpu().numpy(), dbb), 'dw / db do not have the bits of the documented order'
    D = {k: (None if v is None else v.double()) for k, v in t.items()}
    A, a = ho.linear(D['x'], D['w'], D['b'])
    r = ho.linear_backward(D['dy'], D['x'], D['w'])
    _report(f'linear {case}', {'y': hc.ratio(y.cpu(), A, a), 'dx': hc.ratio(dx.cpu(), r['dx'], r['a_dx']), 'dw': hc.ratio(dw.cpu(), r['dw'], r['a_dw']),
                               'db': hc.ratio(db.cpu(), r['db'], r['a_db'])})


@pytest.mark.parametrize('case', [(5, 3, 512, False), (3, 257, 1028, False), (257, 65, 4, True)], ids=str)
def test_linear_backward_accumulate_dx(case):
    """accumulate_dx = 1 of fsvit_linear_backward (public in fsvit.h, no caller in the package): dx prefilled, the result gated against prefill + reference"""
    from fewshot_vit_amd import _lib
    from fewshot_vit_amd.engine import _ptr, _stream_ptr
    lib = _lib.load()
    M, N, K, _ = case
    t = hc.linear_inputs(case)
    dy, w = t['dy'].to(DEV), t['w'].to(DEV)

    def run():
        buf = torch.full((M * K + PAD,), CANARY, device=DEV)
        buf[:M * K] = t['dx0'].to(DEV).reshape(-1)
        _lib.check(lib.fsvit_linear_backward(_ptr(dy), None, _ptr(w), _ptr(buf), 1, None, None, M, N, K, _stream_ptr(torch.device(DEV))))
        torch.cuda.synchronize()
        assert bool((buf[M * K:] == CANARY).all())
        return buf[:M * K].view(M, K)

    got = run()
    _finite(got)
    assert torch.equal(run(), got) and torch.equal(run(), got)
    r = ho.linear_backward(t['dy'].double(), t['x'].double(), t['w'].double())
    _report(f'linear accumulate_dx {case}', {'dx': hc.ratio(got.cpu(), t['dx0'].double() + r['dx'], r['a_dx'])})


def test_linear_refusals():
    ops = _ops()
    x, w = torch.ones(3, 6, device=DEV), torch.ones(2, 6, device=DEV)
    with _Guard() as gd:
        with pytest.raises(ValueError):                                           # K % 4 != 0: the forward loads four columns at a time
            ops.linear(x, w)
    assert gd.untouched()


# ----------------------------------------------------------------------------------------------------------------- token soft labels
@pytest.mark.parametrize('case', hc.SOFTLABEL, ids=str)
@pytest.mark.parametrize('kind', ('random', 'grid'))
def test_token_softlabel(case, kind):
    ops = _ops()
    B, T, C, k, bp = case
    lt = hc.softlabel_inputs(case, kind)
    ld = lt.to(DEV)
    for smoothing in (0.1, 0.3):
        got = _g(lambda: ops.token_softlabel(ld, k, bp, smoothing))
        for _ in range(2):
            assert torch.equal(_g(lambda: ops.token_softlabel(ld, k, bp, smoothing)), got)
        if B > 1:
            assert torch.equal(_g(lambda: ops.token_softlabel(ld[1:], k, bp, smoothing)), got[T:])
        want = ho.token_softlabel(lt.numpy(), k, bp, smoothing)
        assert set(np.unique(got.cpu().numpy())) <= {np.float32(smoothing / C), np.float32(1.0 - smoothing + smoothing / C)}
        assert np.array_equal(got.cpu().numpy(), want), (case, kind, int((got.cpu().numpy() != want).sum()))
    print(f'token_softlabel {case} {kind}: equal')


def test_token_softlabel_refusals():
    ops = _ops()
    for B, T, C, k, bp in hc.SOFTLABEL_REFUSED:
        with _Guard() as gd:
            with pytest.raises(ValueError):
                ops.token_softlabel(torch.zeros(B, T, C, device=DEV), k, bp)
        assert gd.untouched()


# ----------------------------------------------------------------------------------------------------------------- soft-target CE
@pytest.mark.parametrize('shape', hc.STCE_SHAPES, ids=str)
def test_soft_target_ce(shape):
    ops = _ops()
    R, C = shape
    out = {}
    for offset in hc.STCE_OFFSETS:
        for target in hc.STCE_TARGETS:
            z, t = hc.stce_inputs(shape, offset, target)
            zd, td = z.to(DEV), t.to(DEV)
            gs = 1.0 / R
            row, dz = _g(lambda: ops.soft_target_ce(zd, td, gs))
            _finite(row, dz)
            for _ in range(2):
                assert _same(_g(lambda: ops.soft_target_ce(zd, td, gs)), (row, dz))
            row0, dz0 = _g(lambda: ops.soft_target_ce(zd, td, None))                 # no gradient asked for: the same losses
            assert dz0 is None and torch.equal(row0, row)
            if R > 1:
                assert _same(_g(lambda: ops.soft_target_ce(zd[1:], td[1:], gs)), (row[1:], dz[1:]))
            r = ho.soft_target_ce(z.double(), t.double(), ho.f32(gs))
            out[f'row{offset:+g}{target[0]}'] = hc.ratio(row.cpu(), r['row'], r['a_row'])
            out[f'dz{offset:+g}{target[0]}'] = hc.ratio(dz.cpu(), r['dz'], r['a_dz'])
    _report(f'soft_target_ce {shape}', out)


# ----------------------------------------------------------------------------------------------------------------- row_normalize
@pytest.mark.parametrize('shape', hc.ROWNORM_SHAPES, ids=str)
@pytest.mark.parametrize('zero', (False, True))
def test_row_normalize(shape, zero):
    ops = _ops()
    R, D = shape
    x, dy = hc.rownorm_inputs(shape, zero)
    xd = x.to(DEV)
    y, inv = _g(lambda: ops.row_normalize(xd))
    _finite(y, inv)
    for _ in range(2):
        assert _same(_g(lambda: ops.row_normalize(xd)), (y, inv))
    if R > 1:
        assert _same(_g(lambda: ops.row_normalize(xd[1:])), (y[1:], inv[1:]))
    r = ho.row_normalize(x.double())
    out = {'y': hc.ratio(y.cpu(), r['y'], r['a_y']), 'inv': hc.ratio(inv.cpu(), r['inv'], r['a_inv'])}
    # the backward from the reference's forward outputs in fp32 (what the forward kernel is gated to)
    yk, ik, dyd = r['y'].float().to(DEV), r['inv'].float().to(DEV), dy.to(DEV)
    dx = _g(lambda: ops.row_normalize_backward(yk, ik, dyd))
    _finite(dx)
    for _ in range(2):
        assert torch.equal(_g(lambda: ops.row_normalize_backward(yk, ik, dyd)), dx)
    if R > 1:
        assert torch.equal(_g(lambda: ops.row_normalize_backward(yk[1:], ik[1:], dyd[1:])), dx[1:])
    A, a = ho.row_normalize_backward(yk.double().cpu(), ik.double().cpu(), dy.double())
    out['dx'] = hc.ratio(dx.cpu(), A, a)
    if zero:                                                                   # the eps clamp: y exactly 0, inv exactly fp32(1e12), dx = dy * 1e12
        z = R // 2
        assert float(y[z].abs().max()) == 0.0 and float(inv[z]) == float(np.float32(1e12))
        out['dx_zero_row'] = hc.ratio(dx[z].cpu(), dy[z].double() * 1e12, 2.0 * ho.E * dy[z].double().abs() * 1e12)
    _report(f'row_normalize {shape} zero={zero}', out)


# ----------------------------------------------------------------------------------------------------------------- optimizers
def _tail(t):
    """a device copy of t as the head of a canary-tailed buffer -> (view, whole buffer)"""
    buf = torch.full((t.numel() + PAD,), CANARY, device=DEV)
    buf[:t.numel()] = t.to(DEV)
    return buf[:t.numel()], buf


def _tails_ok(*bufs):
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[-PAD:] == CANARY).all()), 'elements behind a parameter / state buffer were written'


@pytest.mark.parametrize('n', hc.OPT_N)
def test_sgd_step(n):
    ops = _ops()
    out = {}
    for momentum, wd, first in hc.SGD_HYPER:
        s = hc.opt_state(n, (momentum, wd, first))
        runs = []
        for _ in range(3):
            (p, pb), (b, bb), g = _tail(s['p']), _tail(s['buf']), s['g'].to(DEV)
            ops.sgd_step(p, g, b, 0.05, momentum, wd, first)
            _tails_ok(pb, bb)
            runs.append((p, b))
        _finite(*runs[0])
        assert _same(runs[1], runs[0]) and _same(runs[2], runs[0])
        r = ho.sgd(s['p'].double(), s['g'].double(), s['buf'].double(), 0.05, momentum, wd, first)
        out[f'm{momentum}/wd{wd}/{int(first)}'] = max(hc.ratio(runs[0][0].cpu(), r['p'], r['a_p']), hc.ratio(runs[0][1].cpu(), r['buf'], r['a_buf']))
    _report(f'sgd_step n={n}', out)


@pytest.mark.parametrize('n', hc.OPT_N)
def test_adamw_step(n):
    ops = _ops()
    h = hc.ADAMW_HYPER
    out = {}
    for step in hc.ADAMW_STEPS if n <= 257 else (1,):
        s = hc.adamw_state(n, step)
        a = (h['lr'], h['beta1'], h['beta2'], h['eps'], h['wd'], step)
        runs = []
        for _ in range(3):
            (p, pb), (m, mb), (v, vb), g = _tail(s['p']), _tail(s['m']), _tail(s['v']), s['g'].to(DEV)
            ops.adamw_step(p, g, m, v, *a)
            _tails_ok(pb, mb, vb)
            runs.append((p, m, v))
        _finite(*runs[0])
        assert _same(runs[1], runs[0]) and _same(runs[2], runs[0])
        r = ho.adamw(s['p'].double(), s['g'].double(), s['m'].double(), s['v'].double(), *a)
        out[f'step{step}'] = max(hc.ratio(x.cpu(), r[k], r['a_' + k]) for x, k in zip(runs[0], 'pmv'))
        z = s['zero_from']                                                         # g = m = v = 0: exactly the decay
        assert torch.equal(runs[0][0][z:].cpu(), hc.f32_decay(s['p'][z:], h['lr'], h['wd']))
        assert float(runs[0][1][z:].abs().max()) == 0.0 and float(runs[0][2][z:].abs().max()) == 0.0
    _report(f'adamw_step n={n}', out)


def _multi_state(kind):
    states = [hc.adamw_state(n, 2) if kind == 'adamw' else hc.opt_state(n, ('multi', i)) for i, n in enumerate(hc.MULTI_LENGTHS)]
    keys = ('p', 'm', 'v') if kind == 'adamw' else ('p', 'buf')
    tails = [{k: _tail(s[k]) for k in keys} for s in states]
    return states, tails, [s['g'].to(DEV) for s in states]


@pytest.mark.parametrize('kind', ('sgd', 'adamw'))
def test_multi_tensor_step_and_table_cache(kind):
    """lengths [1, 257, 131 077, 4] in one launch (the grid is sized by the longest: the short ones leave whole blocks idle, the long one strides) equal
    the single-tensor kernel bit for bit; call 2 with the same tensors re-uses the device table; call 3 with one gradient replaced by a new tensor uses
    the new pointer and leaves the old gradient's buffer alone."""
    ops = _ops()
    h = hc.ADAMW_HYPER
    dev = torch.device(DEV, torch.cuda.current_device())
    keys = ('p', 'm', 'v') if kind == 'adamw' else ('p', 'buf')

    def single(t, g, step):
        if kind == 'adamw':
            ops.adamw_step(t['p'][0], g, t['m'][0], t['v'][0], h['lr'], h['beta1'], h['beta2'], h['eps'], h['wd'], step)
        else:
            ops.sgd_step(t['p'][0], g, t['buf'][0], 0.05, 0.9, 5e-4, step == 1)

    def multi(ts, gs, step):
        if kind == 'adamw':
            return ops.adamw_step_multi([t['p'][0] for t in ts], gs, [t['m'][0] for t in ts], [t['v'][0] for t in ts], h['lr'], h['beta1'], h['beta2'], h['eps'],
                                        h['wd'], step)
        return ops.sgd_step_multi([t['p'][0] for t in ts], gs, [t['buf'][0] for t in ts], 0.05, 0.9, 5e-4, step == 1)

    def agree(a, b):
        _tails_ok(*[t[k][1] for t in a + b for k in keys])
        for x, y in zip(a, b):
            for k in keys:
                assert torch.equal(x[k][0], y[k][0]), k

    _, one, grads = _multi_state(kind)
    _, many, _ = _multi_state(kind)
    grads = [g.clone() for g in grads]                     # addresses of their own: nothing else may alias them while the table is cached
    # call 1
    for t, g in zip(one, grads):
        single(t, g, 1)
    table1 = multi(many, grads, 1)
    agree(one, many)
    _finite(*[t[k][0] for t in many for k in keys])
    ptr1 = table1.data_ptr()
    # call 2: the same tensors - the same table object, no re-upload
    for t, g in zip(one, grads):
        single(t, g, 2)
    table2 = multi(many, grads, 2)
    assert table2 is table1 and table2.data_ptr() == ptr1
    agree(one, many)
    # call 3: a new gradient tensor of the same length in slot 2
    old = grads[2]
    old_bits = old.clone()
    new = (old * 0.5 + 0.25).contiguous()
    assert new.data_ptr() != old.data_ptr()
    grads3 = grads[:2] + [new] + grads[3:]
    for t, g in zip(one, grads3):
        single(t, g, 3)
    table3 = multi(many, grads3, 3)
    assert table3 is not table1
    agree(one, many)
    assert torch.equal(old, old_bits)
    # and the result of the three steps against float64 for the longest tensor's last step is what test_sgd_step / test_adamw_step gate: here the
    # multi kernel inherits those gates through bit equality
    print(f'{kind}_step_multi lengths {hc.MULTI_LENGTHS}: equal to the single-tensor kernel over 3 steps, table cached / re-uploaded')


GS_CAP = 32768 * 256                   # gs_grid: one thread per element up to here, the grid-stride loop of a single-tensor kernel strides beyond


@pytest.mark.parametrize('kind', ('sgd', 'nesterov', 'adamw'))
def test_single_tensor_step_past_the_grid_cap(kind):
    """n = 32768 * 256 + 5, the smallest length at which a single-tensor launch strides: the single kernel equals the multi kernel (a one-row table,
    256 blocks striding 32 769 times) bit for bit on every output, nothing is written behind the buffers, and the last 261 elements - the last block
    and the 5 elements only the second stride reaches - are inside the float64 gates of test_sgd_step / test_adamw_step / test_gpu_sgd_nesterov.py.
    Inputs are drawn on the device (AdamW: the state after one update, update number 2)."""
    ops = _ops()
    h = hc.ADAMW_HYPER
    n, last = GS_CAP + 5, 261
    gen = torch.Generator(device=DEV)
    gen.manual_seed(8388613)
    draw = lambda scale: scale * torch.randn(n, generator=gen, device=DEV)
    src = dict(p=draw(1.0), g=draw(0.1))
    if kind == 'adamw':
        g0 = draw(0.1)
        src.update(m=(1.0 - h['beta1']) * g0, v=(1.0 - h['beta2']) * g0 * g0)
        keys, a = ('p', 'm', 'v'), (h['lr'], h['beta1'], h['beta2'], h['eps'], h['wd'], 2)
        single, multi = ops.adamw_step, ops.adamw_step_multi
    else:
        src.update(buf=draw(0.1))
        keys, a = ('p', 'buf'), (0.05, 0.9, 5e-4, False)
        single, multi = (ops.sgd_step, ops.sgd_step_multi) if kind == 'sgd' else (ops.sgd_nesterov_step, ops.sgd_nesterov_step_multi)
    one, many = {k: _tail(src[k]) for k in keys}, {k: _tail(src[k]) for k in keys}
    single(one['p'][0], src['g'], *[one[k][0] for k in keys[1:]], *a)
    multi([many['p'][0]], [src['g']], *[[many[k][0]] for k in keys[1:]], *a)
    _tails_ok(*[t[k][1] for t in (one, many) for k in keys])
    for k in keys:
        assert torch.equal(one[k][0], many[k][0]), k
    _finite(*[one[k][0] for k in keys])
    x = {k: v[n - last:].cpu().double() for k, v in src.items()}
    ref = {'sgd': ho.sgd, 'nesterov': sgd_cases.sgd_nesterov, 'adamw': ho.adamw}[kind]
    r = ref(x['p'], x['g'], *[x[k] for k in keys[1:]], *a)
    _report(f'{kind}_step n={n}, last {last}', {k: hc.ratio(one[k][0][n - last:].cpu(), r[k], r['a_' + k]) for k in keys})
