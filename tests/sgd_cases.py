"""float64 restatement of torch.optim.SGD(nesterov=True, dampening=0) and its first-order fp32 allowance, shared by test_sgd_nesterov_ref_cpu.py
(torch's own fp32 optimizer against it, no GPU) and test_gpu_sgd_nesterov.py (the kernels of optim.hip).  In the style of
oracle.head_ops_oracle.sgd; gate as tests/head_cases.py: |got - A| <= a + u |A|.

  d = g + wd p                         a_d   = u |wd p| + u |d|
  b = d (first step) | m buf + d       a_buf = a_d  |  a_d + u |m buf| + u |b|
  s = d + m b                          a_s   = a_d + |m| a_buf + u |m b| + u |s|
  p' = p - lr s                        a_p   = |lr| a_s + u |lr s| + u |p'|

u = 2^-24: every fp32 operation rounds its exact result by at most u times its magnitude, and the error already carried by an operand passes through
a sum unchanged and through a product scaled by the other factor.  A fused multiply-add rounds once where this counts twice, so it stays inside.  No
constant comes from a kernel run."""
import torch

import head_cases as hc
from oracle import head_ops_oracle as ho

U = ho.U
LR = 0.05
HYPER = [(m, wd, first) for m in (0.5, 0.9) for wd in (0.0, 5e-4) for first in (True, False)]


def sgd_nesterov(p, g, buf, lr, momentum, wd, first):
    """float64 tensors p, g, buf (buf is not read on the first step) -> dict(p, buf, a_p, a_buf)"""
    lr, momentum, wd = ho.f32(lr), ho.f32(momentum), ho.f32(wd)
    d = g + wd * p
    a_d = U * (wd * p).abs() + U * d.abs()
    if first:
        b, a_b = d, a_d
    else:
        b = momentum * buf + d
        a_b = a_d + U * (momentum * buf).abs() + U * b.abs()
    s = d + momentum * b
    a_s = a_d + abs(momentum) * a_b + U * (momentum * b).abs() + U * s.abs()
    pn = p - lr * s
    return dict(p=pn, buf=b, a_buf=a_b, a_p=abs(lr) * a_s + U * (lr * s).abs() + U * pn.abs())


def state(n, key):
    """fp32 p, g, buf of n elements, seeded by (n, key)"""
    return hc.opt_state(n, ('nesterov', key))


def reference(s, lr, momentum, wd, first):
    return sgd_nesterov(s['p'].double(), s['g'].double(), s['buf'].double(), lr, momentum, wd, first)


def worst(p, buf, r):
    """worst err / bound over p and buf against a reference dict"""
    return max(hc.ratio(torch.as_tensor(p).cpu(), r['p'], r['a_p']), hc.ratio(torch.as_tensor(buf).cpu(), r['buf'], r['a_buf']))
