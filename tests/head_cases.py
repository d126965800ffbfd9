"""Cases, input builders, references and gates of pool_affine (feat_out.hip), the episode head (head.hip), the distillation head (token_label.hip: linear,
soft labels, soft-target CE, row normalisation) and the SGD / AdamW updates (optim.hip), shared by test_head_ops_ref_cpu.py (the references alone,
no GPU) and test_gpu_head_ops.py (the kernels).  All inputs come from seeded generators and are rounded to fp32 (pool_affine: to its storage type) before the
float64 reference of oracle/head_ops_oracle.py sees them.

Gate (fp32 storage, the form of tests/attention_cases.py): |got - A| <= a + u |A|, u = 2^-24, A the float64 result from the fp32 inputs, a the first-order
allowance the oracle returns next to A.  No constant comes from a kernel run; the allowances are derived in the header of test_gpu_head_ops.py.

Head inputs lean every query towards the class of its label (class centres + noise), so that accuracy can be compared exactly: the CPU test asserts for
every query of every case that the float64 top-2 margin exceeds twice the row's logit allowance.
"""
import math
import zlib

import numpy as np
import torch

from oracle import head_ops_oracle as ho

U = ho.U
METHODS = ('cos', 'sqr', 'dot')


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) % (2 ** 31))


def ratio(got, A, a):
    """worst |got - A| / (a + u |A|) over the elements; an element with a zero bound must be exact"""
    got, A, a = (torch.as_tensor(x, dtype=torch.float64) for x in (got, A, a))
    bound = a + U * A.abs()
    err = (got - A).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).double())
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------------------------- episode head
# id -> dict(E, way, shot, Q, D, labels: None (make_nk_label) | 'mod' (q % way, explicit) | 'shuffle', special: None | 'zero')
def _h(E, way, shot, Q, D, labels=None, special=None, bwd=True):
    return dict(E=E, way=way, shot=shot, Q=Q, D=D, labels=labels, special=special, bwd=bwd)


HEAD = {
    # lane-strided loops over D: a partial wave, 64 - 4, exactly one pass, a 4-element tail, ten passes
    'D4': _h(2, 5, 1, 5, 4), 'D60': _h(2, 5, 1, 5, 60), 'D64': _h(2, 5, 1, 5, 64, bwd=False), 'D68': _h(2, 5, 1, 5, 68), 'D640': _h(2, 5, 1, 5, 640),
    # fewer / more classes than the 16 waves; 20-way at D 512: the cosine backward needs 82 KB of LDS
    'way1': _h(2, 1, 5, 3, 64), 'way17-Q17': _h(2, 17, 1, 17, 60), 'way20-D512': _h(2, 20, 5, 20, 512),
    # forward LDS above 64 KB (80 KB); the cosine backward of this shape needs 160 KB + and is refused (HEAD_BWD_REFUSED)
    'way40-D512': _h(1, 40, 1, 8, 512, labels='mod', bwd=False),
    # the largest accepted forward LDS: (63 * 650 + 2 * 5) * 4 = 163 840 bytes = 160 KB exactly
    'lds160k': _h(1, 63, 1, 5, 650, labels='mod', bwd=False),
    # the wave-strided query loop: one query, fewer than 16, two passes + 1
    'Q1': _h(3, 5, 5, 1, 64), 'Q15': _h(3, 5, 5, 15, 64), 'Q33': _h(3, 5, 5, 33, 64, labels='mod'),
    # many workgroups on the ticket
    'E70': _h(70, 5, 1, 5, 64),
    'shuffle': _h(3, 5, 5, 15, 60, labels='shuffle'),
    # one all-zero query row and one all-zero class: the eps clamp
    'zero': _h(2, 5, 5, 10, 60, special='zero'),
}
# one step above 160 KB: (64 * 640 + 2) * 4 = 163 848 bytes
HEAD_FWD_REFUSED = _h(1, 64, 1, 1, 640)
HEAD_BWD_REFUSED = _h(1, 40, 1, 8, 512)          # cosine backward: 2 * 40 * 512 floats alone are 160 KB


def exact_tie_rows(cid, method):
    """query rows whose logits are all the same bits by construction (the all-zero query scores exactly 0 against every class under 'cos' and 'dot'): the
    first maximum is class 0 in the kernel and in the reference; the margin assertion does not apply to them"""
    return [1] if HEAD[cid]['special'] == 'zero' and method in ('cos', 'dot') else []


def head_ids(bwd=False):
    return [k for k, p in HEAD.items() if p['bwd'] or not bwd]


def head_temp(method, D):
    return ho.f32(10.0 if method == 'cos' else 4.0 / D)


def head_labels(p):
    """-> int64 [E Q] (the labels the case is scored with) and whether they are passed explicitly"""
    E, way, Q = p['E'], p['way'], p['Q']
    if p['labels'] is None:
        return ho.make_nk_label(E, way, Q), False
    lab = (torch.arange(Q) % way).repeat(E)
    if p['labels'] == 'shuffle':
        lab = torch.randint(0, way, (E * Q,), generator=_gen('labels', sorted(p.items(), key=str)))
    return lab, True


def head_inputs(cid, p=None):
    """-> dict(fs [E,way,shot,D], fq [E,Q,D], labels int64 [E Q], explicit, dl [E,Q,way] (an upstream gradient for the backward)), fp32"""
    p = p or HEAD[cid]
    E, way, shot, Q, D = p['E'], p['way'], p['shot'], p['Q'], p['D']
    g = _gen('head', cid)
    lab, explicit = head_labels(p)
    centre = torch.randn(E, way, D, generator=g)
    fs = centre[:, :, None, :] + 0.5 * torch.randn(E, way, shot, D, generator=g)
    fq = centre[torch.arange(E)[:, None], lab.reshape(E, Q)] + 0.5 * torch.randn(E, Q, D, generator=g)
    dl = torch.randn(E, Q, way, generator=g) / (E * Q)
    if p['special'] == 'zero':
        fq[:, 1] = 0.0
        fs[:, 2] = 0.0
        dl[:, 3] = 0.0
    return dict(fs=fs.float(), fq=fq.float(), labels=lab, explicit=explicit, dl=dl.float())


def tie_inputs():
    """classes 1 and 3 share bit-identical shot features; queries sit on that shared prototype, labelled 1 (episode e: the first 2 + e of them) or 3.
    Both logits are the same bits in every method, so the first maximum is class 1: accuracy = (2 + e) / Q exactly."""
    E, way, shot, Q, D = 2, 5, 2, 6, 60
    g = _gen('tie')
    centre = 2.0 * torch.randn(E, way, D, generator=g)
    fs = centre[:, :, None, :] + 0.1 * torch.randn(E, way, shot, D, generator=g)
    fs[:, 3] = fs[:, 1]
    fq = fs[:, 1].mean(1)[:, None, :] + 0.05 * torch.randn(E, Q, D, generator=g)
    lab = torch.tensor([[1] * (2 + e) + [3] * (Q - 2 - e) for e in range(E)])
    return dict(fs=fs.float(), fq=fq.float(), labels=lab.reshape(-1), count=torch.tensor([2.0 + e for e in range(E)], dtype=torch.float64))


_REF = {}


def head_reference(cid, method):
    if ('hf', cid, method) not in _REF:
        t = head_inputs(cid)
        _REF[('hf', cid, method)] = ho.head_forward(t['fs'].double(), t['fq'].double(), head_temp(method, HEAD[cid]['D']), method, t['labels'])
    return _REF[('hf', cid, method)]


def head_bwd_reference(cid, method, up):
    if ('hb', cid, method, up) not in _REF:
        t = head_inputs(cid)
        _REF[('hb', cid, method, up)] = ho.head_backward(t['fs'].double(), t['fq'].double(), t['dl'].double(), head_temp(method, HEAD[cid]['D']), method, up)
    return _REF[('hb', cid, method, up)]


# ------------------------------------------------------------------------------------------------------------------------------- pool_affine
POOL_SHAPES = [(1, 1, 4), (3, 25, 512), (2, 49, 384), (2, 196, 1028)]           # C = 1028: C / 4 = 257 > 256 threads, the channel loop runs twice
POOL_DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}


def pool_inputs(shape, dt):
    B, HW, C = shape
    g = _gen('pool', shape, dt)
    x = (torch.randn(B, HW, C, generator=g) + 0.5).to(POOL_DTYPES[dt])
    return x, (1.0 + 0.5 * torch.randn(C, generator=g)).float(), torch.randn(C, generator=g).float()


# ------------------------------------------------------------------------------------------------------------------------------- linear
# (M, N, K, bias).  M: the serial weight-gradient path (1, 5, 255), the first split size (256: 8 slabs of 32), an uneven last slab (257), the 64-slab cap
# (2049: 63 slabs of 33).  N: 1, 3 (not a multiple of the split kernel's 4 outputs), 65, 257 (a second dy tile of 256 in the dx kernel).  K: 4, 512,
# 1028 (a second K pass of 1024 in the dx kernel, a second lane pass of 256 in the forward).
LINEAR = [(1, 1, 4, True), (5, 3, 512, False), (255, 3, 512, True), (256, 3, 512, True), (256, 1, 4, False), (257, 65, 4, True), (257, 3, 1028, False),
          (2049, 65, 512, True), (2049, 3, 4, True), (4, 257, 512, True), (3, 257, 1028, False), (7, 65, 1028, True)]
# the cases whose weight gradient is also compared bit for bit with an emulation of the documented summation order (oracle linear_dw_bits): both sides
# of the M >= 256 switch between the serial and the slab kernels
LINEAR_BITS = [c for c in LINEAR if c[0] in (5, 255, 256, 257)]


def linear_inputs(case):
    M, N, K, bias = case
    g = _gen('linear', case)
    x, w, dy = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(M, N, generator=g)
    return dict(x=x.float(), w=w.float(), b=torch.randn(N, generator=g).float() if bias else None, dy=dy.float(), dx0=torch.randn(M, K, generator=g).float())


# ------------------------------------------------------------------------------------------------------------------------------- token soft labels
# (B, T, C, k, bp)
SOFTLABEL = [(1, 1, 2, 1, 0), (1, 1, 2, 2, 1), (5, 25, 12, 3, 10), (5, 25, 12, 12, 0), (1, 25, 351, 3, 25), (5, 64, 12, 1, 10), (1, 64, 351, 3, 64),
             (5, 64, 2, 2, 0), (5, 25, 351, 351, 10), (1, 64, 12, 3, 63)]
SOFTLABEL_REFUSED = [(1, 65, 12, 3, 10), (1, 25, 12, 0, 10), (1, 25, 12, 13, 10), (1, 25, 12, 3, 26)]


def softlabel_inputs(case, kind):
    """kind 'random': floats without ties; 'grid': integers in [-2, 2] - many equal logits inside a token and equal per-token maxima across tokens"""
    B, T, C, k, bp = case
    g = _gen('softlabel', case, kind)
    if kind == 'grid':
        return torch.randint(-2, 3, (B, T, C), generator=g).float()
    return torch.randn(B, T, C, generator=g).float()


# ------------------------------------------------------------------------------------------------------------------------------- soft-target CE
STCE_SHAPES = [(1, 2), (5, 13), (6, 64), (7, 65), (8, 352), (5, 352), (1, 65)]
STCE_OFFSETS = (0.0, 80.0, -80.0)
STCE_TARGETS = ('soft', 'unnormalised', 'zero_row')


def stce_inputs(shape, offset, target):
    R, C = shape
    g = _gen('stce', shape, offset, target)
    z = (2.0 * torch.randn(R, C, generator=g) + offset).float()
    if target == 'unnormalised':
        t = torch.rand(R, C, generator=g)
    else:                                                    # the two-valued rows token_softlabel writes (k = min(3, C - 1) classes on)
        off, on = 0.1 / C, 1.0 - 0.1 + 0.1 / C
        t = torch.full((R, C), off)
        for r in range(R):
            t[r, torch.randperm(C, generator=g)[:min(3, C - 1)]] = on
        if target == 'zero_row':
            t[R // 2] = 0.0
    return z, t.float()


# ------------------------------------------------------------------------------------------------------------------------------- row_normalize
ROWNORM_SHAPES = [(1, 4), (5, 60), (8, 64), (5, 96), (8, 640), (1, 640), (5, 4)]


def rownorm_inputs(shape, zero):
    """rows of norm >= 1e-6 (asserted on the CPU) except, with `zero`, row R // 2, which is all zero"""
    R, D = shape
    g = _gen('rownorm', shape, zero)
    x = torch.randn(R, D, generator=g) * torch.logspace(-4, 2, R)[:, None]          # row scales from 1e-4 to 1e2
    dy = torch.randn(R, D, generator=g)
    if zero:
        x[R // 2] = 0.0
    return x.float(), dy.float()


# ------------------------------------------------------------------------------------------------------------------------------- optimizers
OPT_N = [1, 255, 256, 257, 131077]            # 131 077 = two grid strides of 65 536 + a tail of 5
MULTI_LENGTHS = [1, 257, 131077, 4]
SGD_HYPER = [(m, wd, first) for m in (0.0, 0.9) for wd in (0.0, 5e-4) for first in (True, False)]
ADAMW_HYPER = dict(lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.05)
ADAMW_STEPS = (1, 2, 1000)


def opt_state(n, key):
    g = _gen('opt', n, key)
    return dict(p=torch.randn(n, generator=g).float(), g=(0.1 * torch.randn(n, generator=g)).float(), buf=(0.1 * torch.randn(n, generator=g)).float())


def adamw_state(n, step):
    """(p, g, m, v) before update number `step`: a float64 AdamW trajectory of step - 1 updates under fresh gradients, rounded to fp32.
    The last max(n // 8, 1) elements of g, m, v are zero: there the update is the decay alone."""
    g_ = _gen('adamw', n, step)
    h = ADAMW_HYPER
    p = torch.randn(n, generator=g_, dtype=torch.float64)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    z = n - max(n // 8, 1)
    for s in range(1, step):
        g = 0.1 * torch.randn(n, generator=g_, dtype=torch.float64)
        g[z:] = 0.0
        r = ho.adamw(p, g, m, v, h['lr'], h['beta1'], h['beta2'], h['eps'], h['wd'], s)
        p, m, v = r['p'], r['m'], r['v']
    g = 0.1 * torch.randn(n, generator=g_, dtype=torch.float64)
    g[z:] = 0.0
    return dict(p=p.float(), g=g.float(), m=m.float(), v=v.float(), zero_from=z)


def f32_decay(p, lr, wd):
    """p * (1 - lr * wd) as the kernel rounds it: every operation in fp32"""
    lr, wd = np.float32(lr), np.float32(wd)
    c = np.float32(1.0) - lr * wd
    assert c == np.float32(1.0 - float(lr) * float(wd)), 'a fused 1 - lr * wd would round differently: choose other hyperparameters'
    return torch.from_numpy(p.numpy() * c)
