"""The prototype bank (proto_bank.hip) through ops.proto_bank_* / PrototypeBank / MetaBaseline.fit + predict against float64 references of the fp32 inputs.
Gates: |got - A| <= a + U |A| with the allowances derived in the header of tests/proto_bank_cases.py from the helpers of oracle/head_ops_oracle.py; no
constant comes from a kernel run.  Each gated test prints `name: worst err/bound`."""
import numpy as np
import pytest
import torch

import proto_bank_cases as pc
from oracle import head_ops_oracle as ho

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TINY = dict(img_size=80, init_channels=8, embed_dim=64, depth=[1, 1, 1], num_heads=6, mlp_ratio=4., group=8)      # the TINY config of tests/test_gpu_emd.py


def _ops():
    from fewshot_vit_amd.engine import ops
    return ops


def _bank(*a, **k):
    from fewshot_vit_amd.models.proto_bank import PrototypeBank
    return PrototypeBank(*a, **k)


def _report(name, pairs):
    w = max(pairs.values())
    print(f'{name}: worst err/bound {w:.3f}  (' + ', '.join(f'{k} {v:.3f}' for k, v in pairs.items()) + ')')
    assert w <= 1.0, (name, pairs)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _state(way, D):
    return (torch.zeros(way, D, dtype=torch.float32, device=DEV), torch.zeros(way, dtype=torch.int32, device=DEV),
            torch.zeros(1, dtype=torch.int32, device=DEV))


def _run_bank(feat, labels, way, method, splits=(None,)):
    """accumulate (one call per split of the rows) + finalize -> (sum, count, invalid, proto, empty)"""
    ops = _ops()
    s, c, inv = _state(way, feat.shape[1])
    lo = 0
    for hi in splits:
        ops.proto_bank_accumulate(feat[lo:hi], labels[lo:hi], s, c, inv)
        lo = hi
    proto, empty = ops.proto_bank_finalize(s, c, method)
    return s, c, inv, proto, empty


def _gate_bank(name, out, r):
    s, c, inv, proto, empty = out
    assert torch.equal(c.cpu().double(), r['count']), 'counts are exact'
    assert torch.equal(empty.cpu().bool(), r['empty']) and int(inv) == 0
    assert bool((proto[empty.bool()] == 0).all())
    _report(name, {'sum': pc.ratio(s.cpu(), r['sum'], r['a_sum']), 'proto': pc.ratio(proto.cpu(), r['proto'], r['a_proto'])})


@pytest.mark.parametrize('S,way,D', pc.BANK_SHAPES)
@pytest.mark.parametrize('method', ('cos', 'sqr'))
@pytest.mark.parametrize('ldt', (torch.int64, torch.int32))
def test_accumulate_finalize(S, way, D, method, ldt):
    t = pc.bank_inputs(S, way, D)
    sizes = torch.bincount(t['labels'], minlength=way)
    if S > way:
        assert 0 in sizes.tolist() and 1 in sizes.tolist(), 'the case must hold an empty class and a class of one'
    feat, labels = t['feat'].to(DEV), t['labels'].to(DEV, ldt)
    out = _run_bank(feat, labels, way, method)
    again = _run_bank(feat, labels, way, method)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(out, again)), 'two runs differ'
    _gate_bank(f'bank {S}x{way}x{D} {method} {ldt}', out, pc.bank_reference(t['feat'], t['labels'], way, method))


@pytest.mark.parametrize('S,way,D', pc.BANK_SHAPES[1:])
def test_incremental_add(S, way, D):
    """two calls over a split of the rows: the same gate, and - the class chains being the same - the bits of one call"""
    t = pc.bank_inputs(S, way, D)
    feat, labels = t['feat'].to(DEV), t['labels'].to(DEV)
    one = _run_bank(feat, labels, way, 'cos')
    two = _run_bank(feat, labels, way, 'cos', splits=(S // 3 + 1, None))
    _gate_bank(f'incremental {S}x{way}x{D}', two, pc.bank_reference(t['feat'], t['labels'], way, 'cos'))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(one, two))


def test_invalid_labels_are_counted_and_left_out():
    way, D = 5, 128
    t = pc.bank_inputs(37, way, D)
    bank = _bank(way, D, 'cos', DEV).add(t['feat'].to(DEV), t['labels'].to(DEV))
    bank.check()
    s0, c0 = bank.sum.clone(), bank.counts.clone()
    bad = torch.tensor([-1, way], dtype=torch.int64, device=DEV)
    bank.add(torch.randn(2, D).to(DEV), bad)
    assert torch.equal(_bits(bank.sum), _bits(s0)) and torch.equal(bank.counts, c0)
    assert int(bank.invalid) == 2
    with pytest.raises(ValueError, match='2 support label'):
        bank.check()
    bank.add(torch.randn(1, D).to(DEV), torch.tensor([way + 7], dtype=torch.int32, device=DEV))
    assert int(bank.invalid) == 3 and torch.equal(bank.counts, c0)


def _logit_inputs(Q, way, D, method):
    g = pc._gen('logits', Q, way, D)
    q, p = torch.randn(Q, D, generator=g), torch.randn(way, D, generator=g)
    if method == 'cos':
        p = torch.nn.functional.normalize(p, dim=-1)          # any fp32 rows are a valid input; these look like finalize's
    empty = torch.zeros(way, dtype=torch.int32)
    if way > 1:
        empty[way - 1] = 1
        p[way - 1] = 0.0
    return q, p, empty


@pytest.mark.parametrize('Q,way,D', pc.LOGIT_SHAPES)
@pytest.mark.parametrize('method', pc.METHODS)
def test_logits(Q, way, D, method):
    ops = _ops()
    q, p, empty = _logit_inputs(Q, way, D, method)
    temp = pc.head_temp(method, D)
    qd, pd, ed = q.to(DEV), p.to(DEV), empty.to(DEV)
    logits, pred = ops.proto_bank_logits(qd, pd, ed, temp, method)
    l2, p2 = ops.proto_bank_logits(qd, pd, ed, torch.tensor(temp, dtype=torch.float32, device=DEV), method)
    assert torch.equal(_bits(logits), _bits(l2)) and torch.equal(pred, p2), 'temperature by value and from the device differ'
    l3, p3 = ops.proto_bank_logits(qd, pd, ed, temp, method, want_pred=False)
    assert p3 is None and torch.equal(_bits(logits), _bits(l3))
    assert pred.dtype == torch.int32 and torch.equal(pred.long(), logits.argmax(-1)), 'pred is the arg-max of the logits it came with'
    if way > 1:
        assert bool(torch.isneginf(logits[:, way - 1]).all()) and int((pred == way - 1).sum()) == 0
    assert bool(torch.isfinite(logits[:, :max(way - 1, 1)]).all())
    A, a = pc.logits_reference(q, p.double(), torch.zeros(way, D, dtype=torch.float64), empty.bool(), temp, method)
    _report(f'logits {Q}x{way}x{D} {method}', {'logits': pc.ratio(logits.cpu(), A, a)})


@pytest.mark.parametrize('method', pc.METHODS)
def test_logits_tie_takes_the_lower_index(method):
    """prototype rows 3 and 70 (two class tiles apart) and 5 and 6 (one thread's columns) are bit-identical, and every query is a copy of one of them,
    so the tied pair is the row maximum for 'cos' and 'sqr': the lower index wins"""
    ops = _ops()
    Q, way, D = 70, 130, 128
    g = pc._gen('tie')
    p = torch.nn.functional.normalize(torch.randn(way, D, generator=g), dim=-1)
    p[70], p[6] = p[3], p[5]
    q = torch.cat([p[3].expand(Q // 2, D), p[5].expand(Q - Q // 2, D)]).contiguous()
    if method == 'dot':
        q = q * 4.0
    logits, pred = ops.proto_bank_logits(q.to(DEV), p.to(DEV), None, 10.0, method)
    assert torch.equal(logits[:, 3], logits[:, 70]) and torch.equal(logits[:, 5], logits[:, 6])
    want = torch.cat([torch.full((Q // 2,), 3), torch.full((Q - Q // 2,), 5)])
    assert bool((logits.max(-1).values.cpu() == logits.cpu().gather(1, want[:, None]).squeeze(1)).all()), 'the tied pair is not the maximum: the case tests nothing'
    assert torch.equal(pred.cpu().long(), want)


def test_refusals():
    from fewshot_vit_amd import _lib
    ops = _ops()
    lib = _lib.load()
    D = 64
    q, p = torch.randn(4, D, device=DEV), torch.randn(3, D, device=DEV)
    e = torch.zeros(3, dtype=torch.int32, device=DEV)
    s, c, inv = _state(3, D)
    out = torch.full((4, 3), 7.0, device=DEV)
    auc = torch.full((2,), 7.0, device=DEV)
    fs, fq = torch.randn(2, 1, D, device=DEV), torch.randn(2, 4, D, device=DEV)
    lab = torch.zeros(4, dtype=torch.int64, device=DEV)
    P = lambda t: None if t is None else t.data_ptr()
    inf = float('inf')
    rcs = {
        'logits null query': lib.fsvit_proto_bank_logits(None, P(p), P(e), 4, 3, D, 1.0, None, 0, P(out), None, None),
        'logits null out': lib.fsvit_proto_bank_logits(P(q), P(p), P(e), 4, 3, D, 1.0, None, 0, None, None, None),
        'logits way 0': lib.fsvit_proto_bank_logits(P(q), P(p), P(e), 4, 0, D, 1.0, None, 0, P(out), None, None),
        'logits temp inf': lib.fsvit_proto_bank_logits(P(q), P(p), P(e), 4, 3, D, inf, None, 0, P(out), None, None),
        'logits temp nan': lib.fsvit_proto_bank_logits(P(q), P(p), P(e), 4, 3, D, float('nan'), None, 0, P(out), None, None),
        'logits D 6': lib.fsvit_proto_bank_logits(P(q), P(p), P(e), 4, 3, 6, 1.0, None, 0, P(out), None, None),
        'logits D 8196': lib.fsvit_proto_bank_logits(P(q), P(p), P(e), 4, 3, 8196, 1.0, None, 0, P(out), None, None),
        'logits misaligned': lib.fsvit_proto_bank_logits(P(q) + 4, P(p), P(e), 3, 3, D, 1.0, None, 0, P(out), None, None),
        'logits method 3': lib.fsvit_proto_bank_logits(P(q), P(p), P(e), 4, 3, D, 1.0, None, 3, P(out), None, None),
        'logits Q -1': lib.fsvit_proto_bank_logits(P(q), P(p), P(e), -1, 3, D, 1.0, None, 0, P(out), None, None),
        'accumulate null': lib.fsvit_proto_bank_accumulate(P(q), None, 1, 4, 3, D, P(s), P(c), P(inv), None),
        'accumulate way 0': lib.fsvit_proto_bank_accumulate(P(q), P(lab), 1, 4, 0, D, P(s), P(c), P(inv), None),
        'accumulate way 65537': lib.fsvit_proto_bank_accumulate(P(q), P(lab), 1, 4, 65537, D, P(s), P(c), P(inv), None),
        'finalize null': lib.fsvit_proto_bank_finalize(P(s), None, 3, D, 0, P(p), P(e), None),
        'finalize D 0': lib.fsvit_proto_bank_finalize(P(s), P(c), 3, 0, 0, P(p), P(e), None),
        'auc null': lib.fsvit_proto_auc(P(fs), None, 2, 1, 4, D, P(auc), None, None),
        'auc odd Q': lib.fsvit_proto_auc(P(fs), P(fq), 2, 1, 3, D, P(auc), None, None),
        'auc Q 4098': lib.fsvit_proto_auc(P(fs), P(fq), 2, 1, 4098, D, P(auc), None, None),
        'auc shot 0': lib.fsvit_proto_auc(P(fs), P(fq), 2, 0, 4, D, P(auc), None, None),
    }
    assert all(rc == _lib.ERR_ARG for rc in rcs.values()), rcs
    assert lib.fsvit_last_error().decode()
    # the successful no-ops
    assert lib.fsvit_proto_bank_accumulate(P(q), P(lab), 1, 0, 3, D, P(s), P(c), P(inv), None) == 0
    assert lib.fsvit_proto_bank_logits(P(q), P(p), P(e), 0, 3, D, 1.0, None, 0, P(out), None, None) == 0
    assert lib.fsvit_proto_auc(P(fs), P(fq), 0, 1, 4, D, P(auc), None, None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((auc == 7.0).all()) and int(c.sum()) == 0 and int(inv) == 0 and float(s.abs().sum()) == 0.0
    # the wrappers: the same refusals as exceptions; host tensors
    with pytest.raises(ValueError):
        ops.proto_bank_logits(q, p, e, inf, 'cos')
    with pytest.raises(ValueError):
        ops.proto_bank_logits(q[:, :6], p[:, :6], e, 1.0, 'cos')
    for call in (lambda: ops.proto_bank_logits(q.cpu(), p, e, 1.0), lambda: ops.proto_bank_accumulate(q.cpu(), lab, s, c, inv),
                 lambda: ops.proto_bank_finalize(s.cpu(), c), lambda: ops.proto_auc(fs.cpu(), fq), lambda: _bank(3, D, 'cos', 'cpu'),
                 lambda: _bank(3, D, 'cos', DEV).add(q.cpu(), lab.cpu()), lambda: _bank(3, D, 'cos', DEV).predict(q.cpu())):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()


# ----------------------------------------------------------------------------------------------------------------- through the model
def _model():
    from fewshot_vit_amd import models
    from fewshot_vit_amd.models.visformer import Visformer
    models.register('tiny_visformer_bank')(lambda **a: Visformer(**TINY, **a))
    torch.manual_seed(0)
    return models.make('meta-baseline', encoder='tiny_visformer_bank', encoder_args={'numerics': 'parity'}).cuda().eval()


def test_rectangular_episode_equals_the_head():
    """2 episodes, 5-way 2-shot, 3 queries per class: fit + predict per episode and model(x_shot, x_query) are each held to the float64 head on the
    engine's own fp32 features - the bank under the gate of its chains, the episode head under ho.head_forward's"""
    model = _model()
    E, way, shot, Qn = 2, 5, 2, 15
    g = torch.Generator().manual_seed(11)
    x_shot = torch.randn(E, way, shot, 3, 80, 80, generator=g).cuda()
    x_query = torch.randn(E, Qn, 3, 80, 80, generator=g).cuda()
    temp = float(model.temp.detach())
    engine = model.encoder.engine()
    with torch.no_grad():
        f_shot = engine.forward(x_shot.view(-1, 3, 80, 80)).view(E, way, shot, -1).cpu()
        f_query = engine.forward(x_query.view(-1, 3, 80, 80)).view(E, Qn, -1).cpu()
        got_head = model(x_shot, x_query).cpu()
        y = torch.arange(way).repeat_interleave(shot).cuda()
        got_bank = torch.stack([model.predict(model.fit(x_shot[e].reshape(-1, 3, 80, 80), y), x_query[e]) for e in range(E)]).cpu()
    r = ho.head_forward(f_shot.double(), f_query.double(), temp, 'cos')
    out = {'head': pc.ratio(got_head, r['logits'], r['a_logits'])}
    for e in range(E):
        b = pc.bank_reference(f_shot[e].reshape(way * shot, -1), y.cpu(), way, 'cos')
        A, a = pc.logits_reference(f_query[e], b['proto'], b['a_proto'], b['empty'], temp, 'cos')
        assert float((A - r['logits'][e]).abs().max()) < 1e-12, 'the two float64 references disagree'
        out[f'bank{e}'] = pc.ratio(got_bank[e], A, a)
    _report('rectangular equivalence', out)
    with pytest.raises(RuntimeError, match='eval-mode'):
        model.train().fit(x_shot[0].reshape(-1, 3, 80, 80), y)


def test_state_dict_round_trip():
    way, D = 5, 128
    g = pc._gen('state')
    f1, f2 = torch.randn(20, D, generator=g).to(DEV), torch.randn(9, D, generator=g).to(DEV)
    y1, y2 = torch.randint(0, way, (20,), generator=g).to(DEV), torch.randint(0, way, (9,), generator=g).to(DEV)
    whole = _bank(way, D, 'sqr', DEV).add(f1, y1).add(f2, y2)
    sd = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in _bank(way, D, 'sqr', DEV).add(f1, y1).state_dict().items()}
    assert set(sd) == {'sum', 'count', 'method'}
    from fewshot_vit_amd.models.proto_bank import PrototypeBank
    back = PrototypeBank.from_state_dict(sd, DEV)
    assert back.method == 'sqr' and torch.equal(back.counts.cpu(), torch.bincount(y1.cpu(), minlength=way).int())
    back.add(f2, y2)
    # the same chain per class (f1's rows, then f2's): bit-exact
    assert torch.equal(_bits(back.sum), _bits(whole.sum)) and torch.equal(back.counts, whole.counts)
    assert torch.equal(_bits(back.prototypes()), _bits(whole.prototypes()))
    q = torch.randn(7, D, generator=g).to(DEV)
    (pa, la), (pb, lb) = back.predict(q, 0.5), whole.predict(q, 0.5)
    assert torch.equal(pa, pb) and torch.equal(_bits(la), _bits(lb)) and pa.dtype == torch.int64
    other = _bank(way, D, 'cos', DEV)
    other.load_state_dict(sd)
    assert other.method == 'sqr'
    with pytest.raises(ValueError):
        _bank(way + 1, D, 'sqr', DEV).load_state_dict(sd)
