"""proto_bank_topk (proto_bank.hip) through ops.proto_bank_topk / PrototypeBank.topk / MetaBaseline.predict_topk / predict --topk.
Selection is held bit for bit to the stable descending sort of what ops.proto_bank_logits writes for the same device tensors (existing, separately
tested code); the log-sum-exp to the float64 sum of those fp32 logits under the allowance derived in tests/proto_bank_topk_cases.py.  No constant comes
from a kernel run.  Each gated test prints `name: worst err/bound`."""
import csv
import os

import numpy as np
import pytest
import torch

import proto_bank_cases as pc
import proto_bank_topk_cases as tc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TINY = dict(img_size=80, init_channels=8, embed_dim=64, depth=[1, 1, 1], num_heads=6, mlp_ratio=4., group=8)
CLASSES = ('ant', 'bee', 'cat')
INF = float('inf')


def _ops():
    from fewshot_vit_amd.engine import ops
    return ops


def _bank(*a, **k):
    from fewshot_vit_amd.models.proto_bank import PrototypeBank
    return PrototypeBank(*a, **k)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return all((x is None and y is None) or torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _inputs(Q, way, D, method, hole=None):
    """query, prototypes and the empty flags as tests/test_gpu_proto_bank.py's _logit_inputs makes them: the class `hole` (default: the last one) is empty
    wherever way > 1"""
    g = pc._gen('logits', Q, way, D)
    q, p = torch.randn(Q, D, generator=g), torch.randn(way, D, generator=g)
    if method == 'cos':
        p = torch.nn.functional.normalize(p, dim=-1)
    empty = torch.zeros(way, dtype=torch.int32)
    if way > 1:
        hole = way - 1 if hole is None else hole
        empty[hole] = 1
        p[hole] = 0.0
    return q, p, empty


_REF = {}


def _reference(Q, way, D, method):
    """device inputs and the existing kernel's (logits, pred) for them, computed once per shape and left unchanged"""
    key = (Q, way, D, method)
    if key not in _REF:
        q, p, e = (t.to(DEV) for t in _inputs(Q, way, D, method))
        temp = pc.head_temp(method, D)
        logits, pred = _ops().proto_bank_logits(q, p, e, temp, method)
        _REF[key] = (q, p, e, temp, logits.cpu(), pred.cpu())
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------------------- 1. selection
@pytest.mark.parametrize('case', tc.SELECT_CASES, ids=lambda c: 'x'.join(map(str, c)))
@pytest.mark.parametrize('method', pc.METHODS)
def test_selection_is_exact(case, method):
    ops = _ops()
    Q, way, D, k = case
    q, p, e, temp, logits, pred = _reference(Q, way, D, method)
    if way > 1:
        assert bool(torch.isneginf(logits[:, way - 1]).all())
    want_v, want_i = tc.topk_reference(logits, k)
    runs = []
    for ns in tc.splits(way):
        v, i, lse = (t.cpu() for t in ops.proto_bank_topk(q, p, e, temp, method, k, ns))
        assert v.dtype == torch.float32 and i.dtype == torch.int32 and tuple(v.shape) == tuple(i.shape) == (Q, k) and tuple(lse.shape) == (Q,)
        assert torch.equal(i, want_i), f'n_split {ns}: indices are not the head of the stable sort'
        assert torch.equal(_bits(v), _bits(want_v)), f'n_split {ns}: values are not the bits of proto_bank_logits'
        assert torch.equal(i[:, 0], pred), f'n_split {ns}: rank 0 is not the existing kernel\'s pred'
        assert not bool(torch.isnan(lse).any())
        runs.append((v, i, lse))
    assert all(_same(runs[0], r) for r in runs[1:]), 'the result depends on n_split'
    dv = tuple(t.cpu() for t in ops.proto_bank_topk(q, p, e, torch.tensor(temp, dtype=torch.float32, device=DEV), method, k))
    assert _same(runs[0], dv), 'temperature by value and from the device differ'
    v3, i3, l3 = ops.proto_bank_topk(q, p, e, temp, method, k, want_lse=False)
    assert l3 is None and _same(runs[0][:2], (v3.cpu(), i3.cpu()))


# ------------------------------------------------------------------------------------------------------------------------------- 2. ties
@pytest.mark.parametrize('method', pc.METHODS)
def test_ties_take_the_lower_class(method):
    """prototype rows 3 = 70 (two tiles apart) = 1030 (another segment, and another split from n_split 2 on) and 5 = 6 (one thread's columns); every query
    is a copy of row 3 or row 5, so the tied classes are the row maximum"""
    ops = _ops()
    Q, way, D = 70, 2100, 128
    g = pc._gen('topk-tie')
    p = torch.nn.functional.normalize(torch.randn(way, D, generator=g), dim=-1)
    p[70], p[1030], p[6] = p[3], p[3], p[5]
    h = Q // 2
    q = torch.cat([p[3].expand(h, D), p[5].expand(Q - h, D)]).contiguous()
    if method == 'dot':
        q = q * 4.0
    qd, pd = q.to(DEV), p.to(DEV)
    logits = ops.proto_bank_logits(qd, pd, None, 10.0, method)[0].cpu()
    assert torch.equal(_bits(logits[:, 3]), _bits(logits[:, 70])) and torch.equal(_bits(logits[:, 3]), _bits(logits[:, 1030]))
    assert torch.equal(_bits(logits[:, 5]), _bits(logits[:, 6]))
    top = logits.max(-1).values
    assert bool((logits[:h, 3] == top[:h]).all()) and bool((logits[h:, 5] == top[h:]).all()), 'the tied classes are not the maximum: the case tests nothing'
    want_v, want_i = tc.topk_reference(logits, 4)
    for ns in tc.splits(way):
        v, i, _ = (t.cpu() for t in ops.proto_bank_topk(qd, pd, None, 10.0, method, 4, ns))
        assert bool((i[:h, :3] == torch.tensor([3, 70, 1030], dtype=torch.int32)).all()), ns
        assert bool((i[h:, :2] == torch.tensor([5, 6], dtype=torch.int32)).all()), ns
        assert torch.equal(i, want_i) and torch.equal(_bits(v), _bits(want_v)), ns


# ---------------------------------------------------------------------------------------------------------------------- 3. empty classes
def test_empty_classes_follow_in_index_order():
    ops = _ops()
    Q, way, D, k = 9, 130, 64, 8
    q, p, _ = _inputs(Q, way, D, 'cos')
    keep = (7, 64, 129)
    empty = torch.ones(way, dtype=torch.int32)
    empty[list(keep)] = 0
    p[empty.bool()] = 0.0
    p[129] = torch.nn.functional.normalize(torch.ones(D), dim=0)
    qd, pd, ed = q.to(DEV), p.to(DEV), empty.to(DEV)
    logits = ops.proto_bank_logits(qd, pd, ed, 10.0, 'cos')[0].cpu()
    v, i, lse = (t.cpu() for t in ops.proto_bank_topk(qd, pd, ed, 10.0, 'cos', k))
    want_v, want_i = tc.topk_reference(logits, k)
    assert torch.equal(i, want_i) and torch.equal(_bits(v), _bits(want_v))
    assert bool(torch.isfinite(v[:, :3]).all()) and bool(torch.isneginf(v[:, 3:]).all())
    assert all(sorted(r) == list(keep) for r in i[:, :3].tolist())
    assert bool((i[:, 3:] == torch.tensor([0, 1, 2, 3, 4], dtype=torch.int32)).all()), 'empty classes: index order after every finite entry'
    r = tc.lse_ratio(lse, tc.lse_reference(logits), way)
    print(f'empty classes: lse worst err/bound {r:.3f}')
    assert r <= 1.0
    # no class has an example
    none = torch.ones(way, dtype=torch.int32, device=DEV)
    v, i, lse = (t.cpu() for t in ops.proto_bank_topk(qd, torch.zeros_like(pd), none, 10.0, 'cos', k))
    assert bool(torch.isneginf(v).all()) and bool(torch.isneginf(lse).all())
    assert bool((i == torch.arange(k, dtype=torch.int32)).all())
    bank = _bank(5, D, 'cos', DEV)
    for kk in (3, 8):
        c, l, pr = (t.cpu() for t in bank.topk(qd, kk, 10.0))
        assert c.dtype == torch.int64 and c[0].tolist() == ([0, 1, 2, 3, 4] + [-1] * kk)[:kk]
        assert bool(torch.isneginf(l).all()) and bool((pr == 0).all()) and not bool(torch.isnan(pr).any())


# ----------------------------------------------------------------------------------------------------------------------- 4. log-sum-exp
def _lse_inputs(way, D, method):
    """70 queries; a class in the middle is empty; for way = 2100 the first rows are spikes: query = prototype b at the edges of the segments"""
    Q = 70
    q, p, e = _inputs(Q, way, D, method, hole=way // 2)
    spikes = tc.SPIKES if way == 2100 else ()
    for r, b in enumerate(spikes):
        q[r] = p[b]
    return q, p, e, spikes


@pytest.mark.parametrize('way', tc.LSE_WAYS)
@pytest.mark.parametrize('method', pc.METHODS)
def test_log_sum_exp(way, method):
    ops = _ops()
    D = 64
    q, p, e, spikes = _lse_inputs(way, D, method)
    temp = pc.head_temp(method, D)
    qd, pd, ed = q.to(DEV), p.to(DEV), e.to(DEV)
    logits = ops.proto_bank_logits(qd, pd, ed, temp, method)[0].cpu()
    L = tc.lse_reference(logits)
    runs = [ops.proto_bank_topk(qd, pd, ed, temp, method, 5, ns)[2].cpu() for ns in tc.splits(way)]
    assert all(torch.equal(_bits(runs[0]), _bits(r)) for r in runs[1:]), 'lse depends on n_split'
    for row in (0, 37, 69):                                  # a row scored alone: the same bits as inside the batch of 70
        alone = ops.proto_bank_topk(qd[row:row + 1], pd, ed, temp, method, 5)[2].cpu()
        assert torch.equal(_bits(alone), _bits(runs[0][row:row + 1])), f'row {row}: lse depends on the other rows of the launch'
    for r, b in enumerate(spikes):                           # losing class b would move L by many allowances
        less = logits[r:r + 1].clone()
        less[0, b] = -INF
        moved = float((L[r] - tc.lse_reference(less)[0]).abs())
        assert moved > 100.0 * float(tc.lse_allowance(way, L[r]) + tc.U * L[r].abs()), (b, moved)
    ratio = tc.lse_ratio(runs[0], L, way)
    print(f'lse {way}x{D} {method}: worst err/bound {ratio:.3f}')
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------------------ 5. refusals, no-ops
def test_refusals():
    from fewshot_vit_amd import _lib
    ops = _ops()
    lib = _lib.load()
    D, Q, way, K = 64, 4, 3, 2
    q, p = torch.randn(Q, D, device=DEV), torch.randn(way, D, device=DEV)
    e = torch.zeros(way, dtype=torch.int32, device=DEV)
    v = torch.full((Q, K), 7.0, device=DEV)
    i = torch.full((Q, K), 7, dtype=torch.int32, device=DEV)
    lse = torch.full((Q,), 7.0, device=DEV)
    need = lib.fsvit_proto_bank_topk_workspace_bytes(Q, way, K, 1)
    assert need == (Q * K * 2 + Q * 2) * 4 == lib.fsvit_proto_bank_topk_workspace_bytes(Q, way, K, 0)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device=DEV)
    big = torch.randn(2100, D, device=DEV)
    P = lambda t: None if t is None else t.data_ptr()
    f = lib.fsvit_proto_bank_topk

    def call(query=P(q), proto=P(p), Q_=Q, way_=way, D_=D, temp=1.0, method=0, K_=K, ns=0, values=P(v), indices=P(i), w=P(ws), wb=need + 64):
        return f(query, proto, P(e), Q_, way_, D_, temp, None, method, K_, ns, values, indices, P(lse), w, wb, None)

    rcs = {
        'null query': call(query=None), 'null proto': call(proto=None), 'null values': call(values=None), 'null indices': call(indices=None),
        'way 0': call(way_=0), 'way 65537': call(way_=65537), 'D 6': call(D_=6), 'D 0': call(D_=0), 'D 8196': call(D_=8196),
        'misaligned query': call(query=P(q) + 4, Q_=3), 'misaligned proto': call(proto=P(p) + 4, way_=2),
        'temp inf': call(temp=INF), 'temp nan': call(temp=float('nan')), 'method 3': call(method=3), 'method -1': call(method=-1), 'Q -1': call(Q_=-1),
        'K 0': call(K_=0), 'K 33': call(K_=33), 'n_split -1': call(ns=-1), 'n_split 2 of 1': call(ns=2),
        'n_split 4 of 3': call(proto=P(big), way_=2100, ns=4, wb=0),
        'null workspace': call(w=None), 'small workspace': call(wb=need - 4), 'no workspace': call(wb=0),
    }
    assert all(rc == _lib.ERR_ARG for rc in rcs.values()), rcs
    assert lib.fsvit_last_error().decode()
    torch.cuda.synchronize()
    assert bool((v == 7.0).all()) and bool((i == 7).all()) and bool((lse == 7.0).all()), 'a refused call wrote an output'
    # the successful no-op, also without a workspace; then the same call for real
    assert call(Q_=0) == 0 and call(Q_=0, w=None, wb=0) == 0
    torch.cuda.synchronize()
    assert bool((v == 7.0).all()) and bool((i == 7).all()) and bool((lse == 7.0).all())
    assert call(wb=need) == 0
    torch.cuda.synchronize()
    assert not bool((i == 7).any())
    v0, i0, l0 = ops.proto_bank_topk(q[:0], p, e, 1.0, 'cos', K)
    assert tuple(v0.shape) == (0, K) and tuple(i0.shape) == (0, K) and tuple(l0.shape) == (0,)
    # the wrappers: the same refusals as exceptions; host tensors
    for bad in (lambda: ops.proto_bank_topk(q, p, e, INF, 'cos', K), lambda: ops.proto_bank_topk(q[:, :6], p[:, :6], e, 1.0, 'cos', K),
                lambda: ops.proto_bank_topk(q, p, e, 1.0, 'cos', 0), lambda: ops.proto_bank_topk(q, p, e, 1.0, 'cos', 33),
                lambda: ops.proto_bank_topk(q, p, e, 1.0, 'cos', K, n_split=2), lambda: ops.proto_bank_topk(q, p, e, 1.0, 'cos', K, n_split=-1),
                lambda: ops.proto_bank_topk(q, p, e[:2], 1.0, 'cos', K), lambda: ops.proto_bank_topk(q, p[:, :32], e, 1.0, 'cos', K),
                lambda: _bank(way, D, 'cos', DEV).topk(q, 0), lambda: _bank(way, D, 'cos', DEV).topk(q, 33)):
        with pytest.raises(ValueError):
            bad()
    for host in (lambda: ops.proto_bank_topk(q.cpu(), p, e, 1.0, 'cos', K), lambda: ops.proto_bank_topk(q, p.cpu(), e, 1.0, 'cos', K),
                 lambda: ops.proto_bank_topk(q, p, e.cpu(), 1.0, 'cos', K), lambda: _bank(way, D, 'cos', DEV).topk(q.cpu(), K)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            host()


# ------------------------------------------------------------------------------------------------------- 6. through the model and the CLI
def _model():
    from fewshot_vit_amd import models
    from fewshot_vit_amd.models.visformer import Visformer
    models.register('tiny_visformer_topk')(lambda **a: Visformer(**TINY, **a))
    torch.manual_seed(0)
    return models.make('meta-baseline', encoder='tiny_visformer_topk', encoder_args={'numerics': 'parity'}).cuda().eval()


def test_predict_topk_is_the_sorted_predict():
    model = _model()
    way, shot, Qn, k = 5, 2, 15, 2
    g = torch.Generator().manual_seed(11)
    x_shot = torch.randn(way * shot, 3, 80, 80, generator=g).cuda()
    x_query = torch.randn(Qn, 3, 80, 80, generator=g).cuda()
    y = torch.arange(way).repeat_interleave(shot).cuda()
    with torch.no_grad():
        bank = model.fit(x_shot, y)
        logits = model.predict(bank, x_query).cpu()
        c, l, pr = (t.cpu() for t in model.predict_topk(bank, x_query, k))
    want_v, want_i = tc.topk_reference(logits, k)
    assert c.dtype == torch.int64 and torch.equal(c, want_i.long()) and torch.equal(_bits(l), _bits(want_v))
    # prob = exp(logit - lse): against the float64 softmax of the fp32 logits; relative error of exp = the absolute error of its argument
    soft = torch.softmax(logits.double(), -1).gather(1, c)
    L = tc.lse_reference(logits)
    a = (tc.lse_allowance(way, L) + tc.U * L.abs() + tc.U * (l.double() - L[:, None]).abs().max(-1).values + 4.0 * tc.U)[:, None]
    ratio = float(((pr.double() - soft).abs() / (soft * a)).max())
    print(f'predict_topk: prob worst err/bound {ratio:.3f}')
    assert ratio <= 1.0
    assert bool((pr.double().sum(-1) <= 1.0 + way * tc.U).all())
    with pytest.raises(RuntimeError, match='eval-mode'):
        model.train().predict_topk(bank, x_query, k)
    model.eval()
    with pytest.raises(ValueError):
        model.predict_topk(bank, x_query, 33)


def _png(path, rng, cls, size):
    from PIL import Image
    base = np.zeros((size[1], size[0], 3))
    base[..., cls] = 160.0
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.clip(base + rng.normal(40.0, 30.0, base.shape), 0, 255).astype(np.uint8)).save(path)


def _tree(root):
    rng = np.random.default_rng(5)
    for c, (name, n) in enumerate(zip(CLASSES, (1, 2, 4))):
        for i in range(n):
            _png(os.path.join(root, 'support', name, f's{i}.png'), rng, c, (96 + 8 * i, 100))
    for i in range(5):
        _png(os.path.join(root, 'query_labelled', CLASSES[i % 3], f'q{i}.png'), rng, i % 3, (92, 92))


def _checkpoint(path):
    from fewshot_vit_amd import models
    from fewshot_vit_amd.models.visformer import Visformer
    models.register('tiny_visformer_topk_cli')(lambda **a: Visformer(**TINY, **a))
    torch.manual_seed(3)
    m = models.make('meta-baseline', encoder='tiny_visformer_topk_cli', encoder_args={})
    torch.save({'model': 'meta-baseline', 'model_args': {'encoder': 'tiny_visformer_topk_cli', 'encoder_args': {}}, 'model_sd': m.state_dict()}, path)


def test_predict_cli_topk(tmp_path, capsys):
    from fewshot_vit_amd import predict
    root = str(tmp_path)
    _tree(root)
    ck, out_f, old_f = (os.path.join(root, n) for n in ('ck.pth', 'top.csv', 'full.csv'))
    _checkpoint(ck)
    common = ['--load', ck, '--support', os.path.join(root, 'support'), '--query', os.path.join(root, 'query_labelled'), '--numerics', 'parity']
    res = predict.main(common + ['--out', out_f, '--topk', '2'])
    assert 'accuracy:' in capsys.readouterr().out
    assert 'logits' not in res and tuple(res['topk_classes'].shape) == tuple(res['topk_logits'].shape) == tuple(res['topk_prob'].shape) == (5, 2)
    rows = list(csv.reader(open(out_f)))
    assert rows[0] == ['file', 'pred_class', 'pred_name', 'class_0', 'name_0', 'logit_0', 'prob_0', 'class_1', 'name_1', 'logit_1', 'prob_1']
    assert len(rows) == 1 + 5 and [r[0] for r in rows[1:]] == res['files']
    for r, cs in zip(rows[1:], res['topk_classes'].tolist()):
        assert [int(r[1]), int(r[3]), int(r[7])] == [cs[0], cs[0], cs[1]]
        assert [r[2], r[4], r[8]] == [CLASSES[cs[0]], CLASSES[cs[0]], CLASSES[cs[1]]]
    got_l = torch.tensor([[float(r[5]), float(r[9])] for r in rows[1:]], dtype=torch.float64)
    got_p = torch.tensor([[float(r[6]), float(r[10])] for r in rows[1:]], dtype=torch.float64)
    assert torch.equal(got_l.float(), res['topk_logits']) and torch.equal(got_p.float(), res['topk_prob']), 'the CSV does not round-trip'
    assert torch.equal(res['pred'], res['topk_classes'][:, 0])
    truth = [CLASSES.index(os.path.basename(os.path.dirname(p))) for p in res['files']]
    assert res['acc'] == pytest.approx(float(np.mean(np.array(truth) == res['pred'].numpy())))
    # without --topk: the old header, the full logits, and the same prediction
    old = predict.main(common + ['--out', old_f])
    rows = list(csv.reader(open(old_f)))
    assert rows[0] == ['file', 'pred_class', 'logit_0', 'logit_1', 'logit_2'] and 'topk_classes' not in old
    assert torch.equal(old['pred'], res['pred']) and [int(r[1]) for r in rows[1:]] == res['pred'].tolist()
    want_v, want_i = tc.topk_reference(old['logits'], 2)
    assert torch.equal(res['topk_classes'], want_i.long()) and torch.equal(_bits(res['topk_logits']), _bits(want_v))
