"""Shapes, the selection reference and the log-sum-exp allowance of proto_bank_topk (proto_bank.hip), shared by tests/test_gpu_proto_bank_topk.py and
tests/test_proto_bank_topk_cpu.py.  Inputs come from proto_bank_cases._gen.

Selection has no allowance: values / indices must be the first k entries of torch.sort(row, descending=True, stable=True) of the row that
ops.proto_bank_logits writes for the same device tensors, bit for bit, padded with (-inf, -1) beyond `way`.

Log-sum-exp: gate |lse - L| <= a + U |L|, L the float64 log-sum-exp of the fp32 logits ops.proto_bank_logits returned (the kernel sums exactly those
values), with U = 2^-24 and
    a = (4 sqrt(way) + ln(way) + 16) U + U |L|
  4 sqrt(n) U   the project's sum_tol form (oracle/head_ops_oracle.py) for a sum of n positive terms, relative to the sum: absolute in its logarithm
  ln(way) U     rounding the arguments l - max: each term moves by U |l - max| relative, the sum by the softmax-weighted mean of max - l, which is at
                most the entropy <= ln(way)
  16 U          expf / logf and the pair merges (16 lanes -> 4 tree levels per segment, then the serial fold over at most 64 segments re-scales by
                exp(m - m') - each a few U on a term of the sum)
No constant comes from a kernel run.  emulate_lse restates the kernel's chain in fp32 numpy (a thread's 4 classes per 64-class tile over the 16 tiles of a
1024-class segment, the 16-lane tree, the fold over segments); tests/test_proto_bank_topk_cpu.py holds it to the allowance for the shapes below."""
import math

import numpy as np
import torch

import proto_bank_cases as pc

U = pc.U
SEG = 1024
# (Q, way, D, k) -> the n_split values to run; n_seg = ceil(way / 1024)
SELECT_CASES = (
    (1, 1, 64, 1), (1, 1, 64, 5),                 # padding beyond way
    (75, 5, 512, 5),                              # k == way
    (130, 17, 128, 3),
    (65, 130, 384, 1), (65, 130, 384, 16), (65, 130, 384, 32),      # tails in both tile axes
    (3, 2100, 64, 8), (70, 4100, 64, 32),         # three and five segments
)
LSE_WAYS = (1, 5, 17, 130, 2100, 4100)
SPIKES = (0, 1023, 1024, 2047, 2048, 2099)        # way = 2100: a query equal to prototype b


def n_seg(way):
    return (way + SEG - 1) // SEG


def splits(way):
    """the n_split values of a case: the library's choice, one, two and one per segment"""
    return tuple(sorted({0, 1, min(2, n_seg(way)), n_seg(way)}))


def topk_reference(logits, k):
    """logits fp32 [Q,way] on the CPU -> (values [Q,k] fp32, indices [Q,k] int32): the head of the stable descending sort, (-inf, -1) beyond way"""
    logits = logits.cpu()
    Q, way = logits.shape
    v, i = torch.sort(logits, dim=-1, descending=True, stable=True)
    values = torch.full((Q, k), -float('inf'), dtype=torch.float32)
    indices = torch.full((Q, k), -1, dtype=torch.int32)
    n = min(k, way)
    values[:, :n] = v[:, :n]
    indices[:, :n] = i[:, :n].int()
    return values, indices


def lse_reference(logits):
    """float64 log-sum-exp of the fp32 rows over their entries other than -inf; -inf for a row without any"""
    l = logits.cpu().double()
    m = l.max(-1, keepdim=True).values
    ok = torch.isfinite(m.squeeze(-1))
    out = torch.full((l.shape[0],), -float('inf'), dtype=torch.float64)
    out[ok] = (m[ok].squeeze(-1) + torch.log(torch.exp(l[ok] - m[ok]).sum(-1)))
    return out


def lse_allowance(way, L):
    L = torch.as_tensor(L, dtype=torch.float64)
    return (4.0 * math.sqrt(way) + math.log(way) + 16.0) * U + U * L.abs()


def lse_ratio(got, L, way):
    """worst |got - L| / (a + U |L|); where L is -inf the result must be -inf"""
    got, L = torch.as_tensor(got, dtype=torch.float64).cpu(), torch.as_tensor(L, dtype=torch.float64)
    inf = torch.isinf(L)
    assert bool((got[inf] == L[inf]).all()), 'a row without a class does not give -inf'
    got, L = got[~inf], L[~inf]
    assert bool(torch.isfinite(got).all())
    r = (got - L).abs() / (lse_allowance(way, L) + U * L.abs())
    return float(r.max()) if r.numel() else 0.0


# ---- the kernel's chain in fp32
_f = np.float32


def _merge(m, s, om, os_):
    nm = np.maximum(m, om)
    ok = nm > -np.inf
    with np.errstate(invalid='ignore', over='ignore'):
        ns = (s * np.exp((m - nm).astype(_f)).astype(_f)).astype(_f) + (os_ * np.exp((om - nm).astype(_f)).astype(_f)).astype(_f)
    return np.where(ok, nm, m).astype(_f), np.where(ok, ns, s).astype(_f)


def emulate_lse(row):
    """row: fp32 [way] (empty classes as -inf) -> the fp32 log-sum-exp the kernel's order of operations gives"""
    row = np.asarray(row, dtype=_f)
    way = row.shape[0]
    M, S = _f(-np.inf), _f(0.0)
    for g in range(n_seg(way)):
        seg = np.full(SEG, -np.inf, dtype=_f)
        part = row[g * SEG:(g + 1) * SEG]
        seg[:part.shape[0]] = part
        tiles = seg.reshape(16, 16, 4)                                  # [tile][lane][j]
        m, s = np.full(16, -np.inf, dtype=_f), np.zeros(16, dtype=_f)
        for t in range(16):
            tm = tiles[t].max(-1)
            up = tm > m
            with np.errstate(invalid='ignore', over='ignore'):
                s = np.where(up, (s * np.exp((m - tm).astype(_f)).astype(_f)).astype(_f), s).astype(_f)
            m = np.where(up, tm, m).astype(_f)
            live = m > -np.inf
            for j in range(4):
                with np.errstate(invalid='ignore', over='ignore'):
                    add = np.exp((tiles[t][:, j] - m).astype(_f)).astype(_f)
                s = np.where(live, (s + add).astype(_f), s).astype(_f)
        for o in (1, 2, 4, 8):
            idx = np.arange(16) ^ o
            m, s = _merge(m, s, m[idx], s[idx])
        Mn, Sn = _merge(np.array([M]), np.array([S]), np.array([m[0]]), np.array([s[0]]))
        M, S = Mn[0], Sn[0]
    if M == -np.inf:
        return _f(-np.inf)
    return _f(M + np.log(S).astype(_f))
