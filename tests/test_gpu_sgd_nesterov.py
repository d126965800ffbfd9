"""The Nesterov SGD kernels of optim.hip (fsvit_sgd_nesterov_step, fsvit_sgd_nesterov_step_multi) and FsvitSGD(nesterov=True) against the
float64 restatement and allowance of tests/sgd_cases.py (proven on the CPU against torch.optim.SGD by test_sgd_nesterov_ref_cpu.py).  Each case asserts:
canary elements behind every parameter / state buffer are untouched; three launches are bit-identical; |got - A| <= a + u |A| for p and buf."""
import pytest
import torch

import head_cases as hc
import sgd_cases as sc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CANARY = 24576.0
PAD = 64


def _ops():
    from fewshot_vit_amd.engine import ops
    return ops


def _tail(t):
    """a device copy of t as the head of a canary-tailed buffer -> (view, whole buffer)"""
    buf = torch.full((t.numel() + PAD,), CANARY, device=DEV)
    buf[:t.numel()] = t.to(DEV)
    return buf[:t.numel()], buf


def _tails_ok(*bufs):
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[-PAD:] == CANARY).all()), 'elements behind a parameter / state buffer were written'


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize('n', hc.OPT_N)
def test_sgd_nesterov_step(n):
    ops = _ops()
    for momentum, wd, first in sc.HYPER:
        s = sc.state(n, (momentum, wd, first))
        runs = []
        for _ in range(3):
            (p, pb), (b, bb), g = _tail(s['p']), _tail(s['buf']), s['g'].to(DEV)
            ops.sgd_nesterov_step(p, g, b, sc.LR, momentum, wd, first)
            _tails_ok(pb, bb)
            runs.append((p, b))
            assert torch.equal(g.cpu(), s['g'])
        assert all(bool(torch.isfinite(x).all()) for x in runs[0])
        assert _same(runs[1], runs[0]) and _same(runs[2], runs[0])
        ratio = sc.worst(runs[0][0], runs[0][1], sc.reference(s, sc.LR, momentum, wd, first))
        print(f'sgd_nesterov_step n={n} m={momentum} wd={wd} first={first}: worst err / bound = {ratio:.3f}')
        assert ratio <= 1.0


def test_multi_equals_single_and_table_cache():
    """lengths [1, 257, 131 077, 4] in one launch equal the single-tensor kernel bit for bit over three steps; call 2 with the same tensors re-uses the
    device table; call 3 with one gradient replaced by a new tensor uses the new pointer and leaves the old gradient's buffer alone."""
    ops = _ops()

    def make():
        states = [sc.state(n, ('multi', i)) for i, n in enumerate(hc.MULTI_LENGTHS)]
        return [{k: _tail(s[k]) for k in ('p', 'buf')} for s in states], [s['g'].to(DEV).clone() for s in states]

    def agree(a, b):
        _tails_ok(*[t[k][1] for t in a + b for k in ('p', 'buf')])
        for x, y in zip(a, b):
            for k in ('p', 'buf'):
                assert torch.equal(x[k][0].view(torch.int32), y[k][0].view(torch.int32)), k

    def step(grads, k):
        for t, g in zip(one, grads):
            ops.sgd_nesterov_step(t['p'][0], g, t['buf'][0], sc.LR, 0.9, 5e-4, k == 1)
        table = ops.sgd_nesterov_step_multi([t['p'][0] for t in many], grads, [t['buf'][0] for t in many], sc.LR, 0.9, 5e-4, k == 1)
        agree(one, many)
        return table

    one, grads = make()
    many, _ = make()
    table1 = step(grads, 1)
    ptr1 = table1.data_ptr()
    table2 = step(grads, 2)
    assert table2 is table1 and table2.data_ptr() == ptr1
    old = grads[2]
    old_bits = old.clone()
    new = (old * 0.5 + 0.25).contiguous()
    assert new.data_ptr() != old.data_ptr()
    table3 = step(grads[:2] + [new] + grads[3:], 3)
    assert table3 is not table1
    assert torch.equal(old, old_bits)
    assert all(bool(torch.isfinite(t[k][0]).all()) for t in many for k in ('p', 'buf'))


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*shape, generator=g).to(DEV)) for shape in ((3, 5), (257,), (2, 3, 4, 5), (1,))]


def _grads(params, seed):
    g = torch.Generator().manual_seed(seed)
    for p in params:
        p.grad = (0.1 * torch.randn(*p.shape, generator=g)).to(DEV)


def test_fsvit_sgd_nesterov_first_and_later_step():
    """each step is gated from the GPU's own state before it; StepLR halves lr between the two"""
    from fewshot_vit_amd.utils import FsvitSGD
    params = _params(0)
    opt = FsvitSGD(params, lr=sc.LR, momentum=0.9, weight_decay=5e-4, nesterov=True)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    for k in (1, 2):
        lr = opt.param_groups[0]['lr']
        assert lr == sc.LR * 0.5 ** (k - 1)
        _grads(params, 10 + k)
        before = [dict(p=p.detach().cpu().clone().view(-1), g=p.grad.cpu().clone().view(-1),
                       buf=opt.state[p]['momentum_buffer'].cpu().clone().view(-1) if k > 1 else torch.zeros(p.numel())) for p in params]
        opt.step()
        sched.step()
        for p, s in zip(params, before):
            r = sc.reference(s, lr, 0.9, 5e-4, k == 1)
            ratio = sc.worst(p.detach().view(-1), opt.state[p]['momentum_buffer'].view(-1), r)
            print(f'FsvitSGD(nesterov) step {k} lr {lr} {tuple(p.shape)}: worst err / bound = {ratio:.3f}')
            assert ratio <= 1.0
            assert not torch.equal(p.detach().cpu().view(-1), s['p'])


def test_fsvit_sgd_default_path_is_unchanged():
    """nesterov=False runs the launches FsvitSGD ran before the keyword existed: bit-identical to ops.sgd_step_multi on the same state over two steps"""
    from fewshot_vit_amd.utils import FsvitSGD
    ops = _ops()
    a, b = _params(1), _params(1)
    opt = FsvitSGD(a, lr=sc.LR, momentum=0.9, weight_decay=5e-4)
    assert opt.param_groups[0]['nesterov'] is False
    bufs = [torch.empty_like(p) for p in b]
    for k in (1, 2):
        _grads(a, 20 + k)
        _grads(b, 20 + k)
        opt.step()
        ops.sgd_step_multi([p.data.view(-1) for p in b], [p.grad.view(-1) for p in b], [x.view(-1) for x in bufs], sc.LR, 0.9, 5e-4, k == 1)
        for p, q, x in zip(a, b, bufs):
            assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32))
            assert torch.equal(opt.state[p]['momentum_buffer'].view(torch.int32), x.view(torch.int32))


def test_nesterov_needs_a_momentum():
    from fewshot_vit_amd.utils import FsvitSGD
    with pytest.raises(ValueError):
        FsvitSGD(_params(2), lr=0.1, momentum=0, nesterov=True)
