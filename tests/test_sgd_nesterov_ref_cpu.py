"""The allowance of tests/sgd_cases.py proven where it can be run: fp32 torch.optim.SGD(nesterov=True) on the CPU stays inside it."""
import pytest
import torch

import head_cases as hc
import sgd_cases as sc


@pytest.mark.parametrize('n', hc.OPT_N)
def test_torch_fp32_nesterov_sgd_is_inside_the_budget(n):
    for momentum, wd, first in sc.HYPER:
        s = sc.state(n, (momentum, wd, first))
        p = torch.nn.Parameter(s['p'].clone())
        p.grad = s['g'].clone()
        opt = torch.optim.SGD([p], lr=sc.LR, momentum=momentum, weight_decay=wd, nesterov=True)
        if not first:
            opt.state[p]['momentum_buffer'] = s['buf'].clone()
        opt.step()
        r = sc.reference(s, sc.LR, momentum, wd, first)
        ratio = sc.worst(p.detach(), opt.state[p]['momentum_buffer'], r)
        print(f'torch SGD(nesterov) n={n} m={momentum} wd={wd} first={first}: worst err / bound = {ratio:.3f}')
        assert ratio <= 1.0
        assert not torch.equal(p.detach(), s['p'])


def test_the_restatement_differs_from_plain_momentum():
    """the Nesterov step is p - lr (d + m b), not p - lr b: the two references are apart by far more than either allowance"""
    from oracle import head_ops_oracle as ho
    s = sc.state(257, 'differs')
    a = sc.reference(s, sc.LR, 0.9, 5e-4, False)
    b = ho.sgd(s['p'].double(), s['g'].double(), s['buf'].double(), sc.LR, 0.9, 5e-4, False)
    assert torch.equal(a['buf'], b['buf'])
    assert float((a['p'] - b['p']).abs().median()) > 1e3 * float((a['a_p'] + b['a_p']).median())
