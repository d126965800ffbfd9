"""Inputs, float64 references and fp32 allowances of the prototype-bank kernels (proto_bank.hip), shared by tests/test_gpu_proto_bank.py,
tests/test_gpu_sauc.py, tests/test_gpu_predict_cli.py and the CPU check of the seeds in tests/test_proto_bank_cpu.py.

The allowances are built from the helpers of oracle/head_ops_oracle.py (U = 2^-24, E = 2^-20, sum_tol(t, n) = 4 sqrt(n) U t, dot(t, n) = sum_tol + U t,
_inv_rel: the relative allowance of 1 / max(|x|, 1e-12) from a lane-strided sum of squares) and from float64 quantities only, as the head's are
(tests/test_gpu_head_ops.py): gate |got - A| <= a + U |A|.  What differs from the episode head is the summation chains, which follow this kernel:
  class sum          a_sum  = sum_tol(sum_k |f_k|, n_c)                      one chain over the n_c rows of the class, in index order (also across add calls)
  prototype          a_p    = a_sum / n_c + U |p|                            one correctly rounded division
  p^ ('cos')         a_p^   = a_p / |p| + |p^| (r(p) + U)                    r(p) = _inv_rel(p, a_p): lane-strided sum of squares, sqrtf, reciprocal
  cos logits         a_l    = T (sum_d |q^_d| a_p^_d + t (r(q) + U) + dot(t, D)) + U |l|     t = sum_d |q^_d p^_d|; the GEMM adds its D products in one
  dot logits         a_l    = T (sum_d |q_d| a_p_d + dot(t, D)) + U |l|                        serial fmaf chain (chain length D, not a wave reduction);
  sqr logits         a_l    = T (sum_d 2 |df_d| (a_p_d + U |df_d|) + dot(sum df^2, D)) + U |l|  the inverse query norm multiplies the finished dot
An empty class has a zero prototype and a zero allowance; its logit must be -inf.
The --sauc score is the cosine logit of the episode head at temperature 1 with a single class (wave reductions, chain ceil(D / 64) + 6): its reference
and allowance are ho.head_forward's own."""
import zlib

import torch

from oracle import head_ops_oracle as ho

U = ho.U
METHODS = ('cos', 'sqr', 'dot')

# (S, way, D): accumulate + finalize
BANK_SHAPES = ((1, 1, 64), (7, 3, 128), (37, 5, 512), (300, 130, 384))
# (Q, way, D): logits - tails in both tile axes (64 x 64 tiles) and one exact tile
LOGIT_SHAPES = ((1, 1, 64), (75, 5, 512), (130, 17, 128), (65, 130, 384), (64, 64, 512))
# (E, shot, Q, D) -> seed for which every untied positive / negative gap exceeds the allowance (asserted on the CPU: tests/test_proto_bank_cpu.py)
SAUC_CASES = {(1, 1, 2, 64): 0, (3, 1, 30, 512): 0, (2, 5, 30, 384): 0}


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) % (2 ** 31))


def ragged_labels(S, way, g):
    """int64 [S]: class 0 gets one row when S > way (and class `way - 1` none when way > 2), the rest are drawn: ragged sizes that include 0 and 1"""
    if S <= way:
        return torch.arange(S, dtype=torch.int64) % way
    hi = way - 1 if way > 2 else way
    lab = torch.randint(1 if way > 1 else 0, hi, (S,), generator=g)
    lab[S // 2] = 0
    return lab


def bank_inputs(S, way, D):
    g = _gen('bank', S, way, D)
    return dict(feat=torch.randn(S, D, generator=g), labels=ragged_labels(S, way, g))


def bank_reference(feat, labels, way, method):
    """feat fp32 [S,D], labels int64 [S] (entries outside [0, way) are left out) -> dict(sum, a_sum, count, empty, proto, a_proto), float64"""
    f = feat.double()
    D = f.shape[1]
    onehot = torch.zeros(f.shape[0], way, dtype=torch.float64)
    ok = (labels >= 0) & (labels < way)
    onehot[ok.nonzero().squeeze(1), labels[ok]] = 1.0
    count = onehot.sum(0)
    s = onehot.t() @ f
    a_s = 4.0 * count.sqrt()[:, None] * U * (onehot.t() @ f.abs())             # sum_tol(sum |f|, n_c) per class
    n = count.clamp_min(1.0)[:, None]
    p = s / n
    a_p = a_s / n + U * p.abs()
    if method == 'cos':
        ph, pinv = ho.normalize(p)
        a_p = a_p * pinv + ph.abs() * (ho._inv_rel(p, a_p) + U)
        p = ph
    empty = count == 0
    p[empty] = 0.0
    a_p[empty] = 0.0
    return dict(sum=s, a_sum=a_s, count=count, empty=empty, proto=p, a_proto=a_p)


def logits_reference(query, proto, a_proto, empty, temp, method):
    """query fp32 [Q,D]; proto / a_proto float64 [way,D] (bank_reference, or an exact fp32 prototype with a_proto = 0) -> (logits, allowance) float64"""
    q = query.double()
    D = q.shape[1]
    temp = ho.f32(temp)
    if method == 'cos':
        qh, _ = ho.normalize(q)
        L = temp * qh @ proto.t()
        T = qh.abs() @ proto.abs().t()
        a = abs(temp) * (qh.abs() @ a_proto.t() + T * (ho._inv_rel(q) + U) + ho.dot(T, D)) + U * L.abs()
    elif method == 'dot':
        L = temp * q @ proto.t()
        T = q.abs() @ proto.abs().t()
        a = abs(temp) * (q.abs() @ a_proto.t() + ho.dot(T, D)) + U * L.abs()
    else:
        df = q[:, None, :] - proto[None, :, :]
        T = df.pow(2).sum(-1)
        L = -temp * T
        a = abs(temp) * ((2.0 * df.abs() * (a_proto[None] + U * df.abs())).sum(-1) + ho.dot(T, D)) + U * L.abs()
    L[:, empty] = -float('inf')
    a[:, empty] = 0.0
    return L, a


def ratio(got, A, a):
    """worst |got - A| / (a + U |A|); where the reference is -inf the result must be -inf"""
    got, A, a = (torch.as_tensor(x, dtype=torch.float64) for x in (got, A, a))
    inf = torch.isinf(A)
    assert bool((got[inf] == A[inf]).all()), 'an empty class does not score -inf'
    got, A, a = got[~inf], A[~inf], a[~inf]
    bound = a + U * A.abs()
    err = (got - A).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float('inf'), 0.0).double())
    return float(r.max()) if r.numel() else 0.0


def head_temp(method, D):
    return ho.f32(10.0 if method == 'cos' else 4.0 / D)


# ------------------------------------------------------------------------------------------------------------------------------- --sauc
def sauc_inputs(E, shot, Q, D, seed):
    """feat_shot [E,shot,D], feat_query [E,Q,D] fp32; with Q >= 4 the first two negative rows are copies of the first two positive rows: two tied pairs
    per episode whose scores are bit-identical on any arithmetic that treats rows alike"""
    g = torch.Generator().manual_seed(seed * 7919 + zlib.crc32(repr((E, shot, Q, D)).encode()) % 10007)
    fs, fq = torch.randn(E, shot, D, generator=g), torch.randn(E, Q, D, generator=g)
    k = Q // 2
    n_dup = 2 if k > 1 else 0
    fq[:, k:k + n_dup] = fq[:, :n_dup]
    return fs, fq, n_dup


def sauc_reference(fs, fq, n_dup):
    """-> (score float64 [E,Q], auc [E] by sklearn.metrics.roc_auc_score, ok: every positive / negative pair other than the constructed ties is further
    apart than the two scores' fp32 allowances, so the fp32 order of every pair is the float64 order)"""
    from sklearn.metrics import roc_auc_score
    E, Q = fq.shape[:2]
    k = Q // 2
    r = ho.head_forward(fs.double()[:, None], fq.double(), 1.0, 'cos')
    s, a = r['logits'][..., 0], r['a_logits'][..., 0] + U * r['logits'][..., 0].abs()
    gap = (s[:, :k, None] - s[:, None, k:]).abs()
    need = a[:, :k, None] + a[:, None, k:]
    tied = torch.zeros(k, k, dtype=torch.bool)
    for i in range(n_dup):
        tied[i, i] = True
    ok = bool((gap[:, ~tied] > need[:, ~tied]).all()) and bool((gap[:, tied] == 0).all())
    auc = torch.tensor([roc_auc_score([1] * k + [0] * k, s[e].numpy()) for e in range(E)], dtype=torch.float64)
    return s, auc, ok
