"""The DeepEMD head over a token-map table (fsvit_emd_table_prep / fsvit_emd_head_gather behind ops.emd_table_prep / ops.emd_head_gather,
feature_table.TokenTable, eval_deepemd -feature_cache, train_deepemd -eval_feature_cache).

The table route promises the bits of the dense route, so the reference of every comparison is the dense `ops.emd_head_forward` (or the dense driver)
on the same maps and the test is `torch.equal` / `==`, no tolerance.  The float64 oracle (tests/emd_cases.py) bounds the gather head by the 1e-4 that
tests/test_gpu_emd.py derives for the dense head.  The invalid-slot test checks a guard that refuses before it reads: every address any launch here
forms lies inside the table."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import emd_cases as ec

pytestmark = pytest.mark.gpu
T = 12.5
SHAPES = [(2, 3, 4, 25, 64), (1, 5, 6, 13, 512), (1, 2, 2, 1, 64), (3, 2, 5, 32, 64)]          # (E, P, Q, N, C)
TINY = dict(img_size=80, init_channels=8, embed_dim=64, depth=[1, 1, 1], num_heads=6, mlp_ratio=4., group=8)       # the encoder of test_gpu_emd.py
ENCODER = 'tiny_visformer_emd'


def _ops():
    from fewshot_vit_amd.engine import ops
    return ops


_tables = {}


def _table(shape):
    """A prepared table with twice as many slots as one launch of `shape` uses: (tok, xhat, pooled) on the GPU; built once per shape, never modified."""
    if shape not in _tables:
        E, P, Q, N, Cc = shape
        n_slots = 2 * E * (P + Q)
        tok = ec.token_case(1, n_slots, 1, N, Cc, seed=100 + N)[0][0].float().cuda().contiguous()
        xhat, pooled = torch.full_like(tok, float('nan')), torch.full((n_slots, Cc), float('nan'), device='cuda')
        _ops().emd_table_prep(tok, xhat, pooled)
        _tables[shape] = (tok, xhat, pooled)
    return _tables[shape]


def _slot_patterns(shape):
    """name -> (proto_slots [E,P], query_slots [E,Q]) int64 on the host"""
    E, P, Q, N, Cc = shape
    n_slots = 2 * E * (P + Q)
    g = torch.Generator().manual_seed(N * 1000 + Cc)
    rand_p, rand_q = torch.randint(0, n_slots, (E, P), generator=g), torch.randint(0, n_slots, (E, Q), generator=g)
    rand_q[E - 1, 0] = rand_q[0, 0]                    # a repeat across episodes (inside the episode when E = 1)
    rand_p[E - 1, P - 1] = rand_p[0, 0]
    shared_p, shared_q = rand_p.clone(), rand_q.clone()
    shared_q[0, Q - 1] = shared_p[0, 0]                # one image as prototype and as query of the same episode
    desc = torch.arange(E * (P + Q) - 1, -1, -1)
    return {'random': (rand_p, rand_q), 'shared': (shared_p, shared_q), 'descending': (desc[:E * P].view(E, P), desc[E * P:].view(E, Q))}


def _dense(tok, ps, qs):
    logits, _, status = _ops().emd_head_forward(tok[ps.cuda().long()], tok[qs.cuda().long()], T, want_flow=False)
    return logits, status


def _gather(table, ps, qs, invalid=None, dtype=torch.int32, **kw):
    invalid = torch.zeros(1, dtype=torch.int32, device='cuda') if invalid is None else invalid
    out = _ops().emd_head_gather(*table, qs.to(dtype).cuda(), T, invalid, proto_slots=None if ps is None else ps.to(dtype).cuda(), **kw)
    return (*out, invalid)


# ---------------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize('shape', SHAPES)
def test_gather_equals_the_dense_head(shape):
    table = _table(shape)
    for name, (ps, qs) in _slot_patterns(shape).items():
        ref_logits, ref_status = _dense(table[0], ps, qs)
        for dtype in (torch.int32, torch.int64):
            logits, status, invalid = _gather(table, ps, qs, dtype=dtype)
            assert logits.shape == ref_logits.shape and status.dtype == torch.int32
            assert torch.equal(logits, ref_logits) and torch.equal(status, ref_status), (name, dtype)
            assert int(status.sum()) == 0 and int(invalid) == 0 and bool(torch.isfinite(logits).all())
        if name == 'shared':
            assert abs(logits[0, shape[2] - 1, 0].item() - T) <= 1e-4            # an image against itself: the logit is the temperature


@pytest.mark.parametrize('shape', SHAPES)
def test_gather_matches_the_float64_oracle(shape):
    table = _table(shape)
    ps, qs = _slot_patterns(shape)['random']
    tok = table[0].cpu().double()
    ref = ec.head_oracle(tok[ps], tok[qs], T)[0]
    logits, status, _ = _gather(table, ps, qs)
    err = (logits.cpu().double() - ref).abs().max().item()
    print(f'emd_head_gather {shape}: max |logit - oracle| = {err:.3e}')
    assert int(status.sum()) == 0 and err <= 1e-4


@pytest.mark.parametrize('shape', SHAPES)
def test_dense_prototype_form(shape):
    E, P, Q, N, Cc = shape
    table = _table(shape)
    _, qs = _slot_patterns(shape)['random']
    proto = ec.token_case(E, P, 1, N, Cc, seed=7 + N)[0].float().cuda()              # maps that are in no table
    ref_logits, _, ref_status = _ops().emd_head_forward(proto, table[0][qs.cuda()], T, want_flow=False)
    for dtype in (torch.int32, torch.int64):
        logits, status, invalid = _gather(table, None, qs, dtype=dtype, proto_tok=proto)
        assert torch.equal(logits, ref_logits) and torch.equal(status, ref_status) and int(invalid) == 0 and int(status.sum()) == 0


def test_table_prep_is_launch_independent():
    for shape in SHAPES:
        tok, xhat, pooled = _table(shape)
        n = tok.shape[0]
        for chunk in (1, 3):
            xh, pl = torch.full_like(xhat, float('nan')), torch.full_like(pooled, float('nan'))
            for lo in range(0, n, chunk):                              # every chunk is its own launch, at its own row offset
                _ops().emd_table_prep(tok[lo:lo + chunk], xh[lo:lo + chunk], pl[lo:lo + chunk])
            assert torch.equal(xh, xhat) and torch.equal(pl, pooled), (shape, chunk)
        # ... and they are the nodes the dense head prepares: unit vectors with zero channel mean, and the token mean of the map
        assert (xhat.double().norm(dim=-1) - 1).abs().max().item() <= 1e-5 and xhat.double().mean(dim=-1).abs().max().item() <= 1e-6
        assert (pooled.double() - tok.double().mean(dim=1)).abs().max().item() <= 1e-5


@pytest.mark.parametrize('side', ['proto', 'query'])
def test_invalid_slots_are_refused_before_any_read(side):
    shape = SHAPES[0]
    E, P, Q, N, Cc = shape
    table = _table(shape)
    n_slots = table[0].shape[0]
    ps, qs = (t.clone() for t in _slot_patterns(shape)['random'])
    ref_logits, _ = _dense(table[0], ps, qs)
    bad = torch.zeros(E, Q, P, dtype=torch.bool)
    if side == 'proto':
        ps[0, 1], ps[1, 2] = -1, n_slots
        bad[0, :, 1] = bad[1, :, 2] = True
    else:
        qs[0, 2], qs[1, 0] = -1, n_slots
        bad[0, 2, :] = bad[1, 0, :] = True
    for dtype in (torch.int32, torch.int64):
        logits, status, invalid = _gather(table, ps, qs, dtype=dtype)
        assert int(invalid) == 2
        assert torch.equal(torch.isnan(logits).cpu(), bad) and int(status.sum()) == 0
        assert torch.equal(logits.cpu()[~bad], ref_logits.cpu()[~bad])
        good_p, good_q = _slot_patterns(shape)['random']
        again, _, _ = _gather(table, good_p, good_q, invalid=invalid, dtype=dtype)   # a following valid launch: finite, the count stays
        assert torch.equal(again, ref_logits) and int(invalid) == 2
    if side == 'query':                                                             # the dense-prototype form guards its query side the same way
        proto = table[0][:E * P].view(E, P, N, Cc).contiguous()
        logits, status, invalid = _gather(table, None, qs, proto_tok=proto)
        assert int(invalid) == 2 and torch.equal(torch.isnan(logits).cpu(), bad) and int(status.sum()) == 0


def test_argument_refusals_launch_nothing():
    from fewshot_vit_amd import _lib
    lib = _lib.load()
    E, P, Q, N, Cc = 1, 2, 2, 5, 64
    z = lambda *s: torch.zeros(*s, device='cuda')
    tok, xhat, pooled = z(8, N, Cc), z(8, N, Cc), z(8, Cc)
    qs, ps = torch.zeros(E, Q, dtype=torch.int32, device='cuda'), torch.zeros(E, P, dtype=torch.int32, device='cuda')
    proto = z(E, P, N, Cc)
    logits, status = torch.full((E, Q, P), 7.0, device='cuda'), torch.full((E, Q, P), 7, dtype=torch.int32, device='cuda')
    invalid = torch.zeros(1, dtype=torch.int32, device='cuda')
    need = lib.fsvit_emd_head_gather_workspace_bytes(E, P, N, Cc)
    assert need == (E * P) * (N * Cc + Cc + N) * 4
    assert lib.fsvit_emd_head_gather_workspace_bytes(E, P, 33, Cc) == 0 and lib.fsvit_emd_head_gather_workspace_bytes(E, P, N, 96) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(ps_=ps, proto_=None, N_=N, C_=Cc, ws_bytes=need):
        rc = lib.fsvit_emd_head_gather(p(tok), p(xhat), p(pooled), 8, p(qs), p(ps_), 0, p(proto_), E, P, Q, N_, C_, T, p(logits), p(status), p(invalid), p(ws),
                                       ws_bytes, None)
        return rc, lib.fsvit_last_error().decode()

    for kw, code, word in ((dict(ps_=ps, proto_=proto), _lib.ERR_ARG, 'exactly one'), (dict(ps_=None, proto_=None), _lib.ERR_ARG, 'exactly one'),
                           (dict(N_=33), _lib.ERR_ARG, 'N must be'), (dict(C_=96), _lib.ERR_ARG, 'multiple of 64'),
                           (dict(ps_=None, proto_=proto, ws_bytes=need - 1), _lib.ERR_WORKSPACE, 'workspace')):
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
    assert lib.fsvit_emd_table_prep(p(tok), 8, 33, Cc, p(xhat), p(pooled), None) == _lib.ERR_ARG
    assert lib.fsvit_emd_table_prep(p(tok), 8, N, 96, p(xhat), p(pooled), None) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((logits == 7.0).all()) and bool((status == 7).all()) and int(invalid) == 0 and bool((xhat == 0).all())      # nothing ran
    rc, msg = call(ps_=None, proto_=proto)                                           # the same call with a workspace that is long enough
    assert rc == 0, msg
    ops = _ops()
    with pytest.raises(ValueError, match='exactly one'):
        ops.emd_head_gather(tok, xhat, pooled, qs, T, invalid)
    with pytest.raises(ValueError, match='exactly one'):
        ops.emd_head_gather(tok, xhat, pooled, qs, T, invalid, proto_slots=ps, proto_tok=proto)
    with pytest.raises(ValueError, match='not finite'):
        ops.emd_head_gather(tok, xhat, pooled, qs, float('inf'), invalid, proto_slots=ps)
    with pytest.raises(ValueError, match='int32 / int64'):
        ops.emd_head_gather(tok, xhat, pooled, qs.float(), T, invalid, proto_slots=ps)


# ---------------------------------------------------------------- 2. TokenTable over a fake encoder
def _tiny_model(**kw):
    from fewshot_vit_amd import models
    from fewshot_vit_amd.models.visformer import Visformer
    models.register(ENCODER)(lambda **a: Visformer(**TINY, **a))
    torch.manual_seed(0)
    return models.make('deepemd', encoder=ENCODER, encoder_args={'numerics': 'parity'}, **kw)


def _fake_table(stored, chunk):
    from fewshot_vit_amd.feature_table import TokenTable
    calls = []

    def encode_fn(index):
        calls.append(index.clone())
        return stored[index.cuda()]

    return TokenTable(encode_fn, stored.shape[0], 'cuda', chunk_images=chunk), calls


def test_token_table_encodes_once_and_does_not_depend_on_the_request_order():
    way, n_query, N, Cc = 2, 2, 13, 64
    stored = ec.token_case(1, 30, 1, N, Cc, seed=5)[0][0].float().cuda()
    model = _tiny_model(sfc_update_step=2, sfc_bs=3, sfc_lr=0.1).eval()
    g = torch.Generator().manual_seed(3)
    for shot in (1, 2):
        per = way * (shot + n_query)
        episodes = [torch.randperm(30, generator=g)[:per] for _ in range(4)]
        episodes[2][1] = episodes[0][0]                             # one image in two episodes
        a, calls_a = _fake_table(stored, 4)
        b, calls_b = _fake_table(stored, 5)
        b.ensure(torch.arange(29, -1, -1))                          # b sees every image first, in another order and other chunks: other slots
        assert [len(c) for c in calls_b] == [5] * 6
        out = {}
        for name, table in (('a', a), ('b', b), ('dense', None)):
            model.sfc_generator = torch.Generator().manual_seed(11)
            rows = []
            for pair in (episodes[:2], episodes[2:]):               # two launches of two episodes
                idx = torch.cat(pair)
                if table is not None:
                    rows.append(table.logits(idx, way, shot, n_query, model))
                    continue
                maps = stored[idx.cuda()].view(2, way, shot + n_query, N, Cc)
                proto = maps[:, :, 0] if shot == 1 else model.get_sfc(maps[:, :, :shot], generator=model.sfc_generator)
                rows.append(model.emd_forward(proto.contiguous(), maps[:, :, shot:].reshape(2, way * n_query, N, Cc)))
            out[name] = torch.cat(rows)
        model.check_status()
        a.check()
        b.check()
        assert out['a'].shape == (4, way * n_query, way)
        assert torch.equal(out['a'], out['dense']) and torch.equal(out['b'], out['dense']), shot
        seen = torch.cat(episodes).unique()
        encoded = torch.cat(calls_a)
        assert a.n_encoded == len(seen) == len(encoded) and torch.equal(encoded.sort().values, seen)           # each image once
        assert all(1 <= len(c) <= 4 and torch.equal(c, c.sort().values) for c in calls_a)                      # chunked, ascending
        assert a.n_requests == 4 * per and b.n_encoded == 30 and b.n_requests == 30 + 4 * per and len(calls_b) == 6
        assert not torch.equal(a.ensure(episodes[0]), b.ensure(episodes[0]))                                   # the two tables do hold other slots


# ---------------------------------------------------------------- 3. the drivers
@pytest.fixture(scope='module')
def checkpoint(tmp_path_factory):
    m = _tiny_model()
    path = os.path.join(tmp_path_factory.mktemp('emd_table'), 'tiny.pth')
    torch.save({'params': m.state_dict()}, path)
    return path


ROUTES = {'fcn-1shot': ['-shot', '1'], 'fcn-5shot': ['-shot', '5', '-sfc_update_step', '3'], 'fcn-5shot-fused': ['-shot', '5', '-sfc_update_step', '3', '-sfc_fused'],
          'grid-1shot': ['-shot', '1', '-deepemd', 'grid']}


@pytest.mark.parametrize('route', list(ROUTES))
def test_eval_driver_with_the_cache_equals_the_driver_without(route, checkpoint, monkeypatch):
    from fewshot_vit_amd import eval_deepemd
    _tiny_model()                                                   # registers the encoder
    stream = []

    class Recording(eval_deepemd.CategoriesSampler):
        def __iter__(self):
            for idx in super().__iter__():
                stream.append(idx.clone())
                yield idx

    monkeypatch.setattr(eval_deepemd, 'CategoriesSampler', Recording)
    argv = ['-encoder', ENCODER, '-numerics', 'parity', '-model_dir', checkpoint, '-dataset', 'synthetic-images', '-dataset_args',
            '{split: test, n_classes: 8, n_per_class: 24}', '-way', '3', '-query', '2', '-test_episode', '5', '-episodes_per_launch', '2', '-sfc_lr', '0.1',
            *ROUTES[route]]
    runs = {}
    for name, extra in (('off', []), ('on', ['-feature_cache'])):
        del stream[:]
        accs, lines = [], []
        res = eval_deepemd.evaluate(eval_deepemd.parse_args(argv + extra), log=lines.append, collect=accs)
        runs[name] = (res, accs, lines, torch.cat(stream))
    (off, acc_off, lines_off, stream_off), (on, acc_on, lines_on, stream_on) = runs['off'], runs['on']
    assert set(off) == {'acc', 'ci', 'n'} and set(on) == {'acc', 'ci', 'n', 'n_encoded', 'n_requests'}
    assert torch.equal(stream_off, stream_on)                       # the same episodes
    assert on['acc'] == off['acc'] and on['ci'] == off['ci'] and on['n'] == off['n'] == 5
    assert acc_on == acc_off and len(acc_on) == 5 and lines_on == lines_off
    assert on['n_requests'] == stream_on.numel() == 5 * 3 * (int(ROUTES[route][1]) + 2)
    assert on['n_encoded'] == stream_on.unique().numel() < on['n_requests']


def test_eval_driver_on_the_default_encoder_in_bf16():
    """the configuration tools/bench_emd_cache.py measures (Visformer, bf16, fcn 1-shot), small"""
    from fewshot_vit_amd import eval_deepemd
    argv = ['-numerics', 'bf16', '-dataset', 'synthetic-images', '-dataset_args', '{split: test, n_classes: 8, n_per_class: 24}', '-way', '3', '-query', '2',
            '-test_episode', '5', '-episodes_per_launch', '2']
    acc_off, acc_on = [], []
    off = eval_deepemd.evaluate(eval_deepemd.parse_args(argv), log=lambda s: None, collect=acc_off)
    on = eval_deepemd.evaluate(eval_deepemd.parse_args(argv + ['-feature_cache']), log=lambda s: None, collect=acc_on)
    assert acc_on == acc_off and (on['acc'], on['ci'], on['n']) == (off['acc'], off['ci'], off['n'])
    assert on['n_encoded'] <= on['n_requests'] == 5 * 3 * 3


@pytest.mark.parametrize('mode', ['fcn', 'grid'])
def test_train_driver_validates_from_the_table_with_the_same_figures(mode, checkpoint, tmp_path):
    from fewshot_vit_amd import train_deepemd
    _tiny_model()
    argv = ['-dataset', 'synthetic-images', '-dataset_args', '{n_classes: 4, n_per_class: 6}', '-encoder', ENCODER, '-numerics', 'parity', '-pretrain_dir',
            checkpoint, '-way', '2', '-shot', '1', '-query', '2', '-max_epoch', '2', '-val_frequency', '2', '-bs', '2', '-val_episode', '3', '-test_episode', '4',
            '-step_size', '1', '-episodes_per_launch', '2', '-lr', '0.01', '-seed', '3', '-deepemd', mode, '-save_all'] + (['-patch_list', '2'] if mode == 'grid' else [])
    logs = {}
    for name, extra in (('plain', []), ('cache', ['-eval_feature_cache'])):
        lines = []
        out = train_deepemd.run(train_deepemd.parse_args(argv + ['-save_root', str(tmp_path / name)] + extra), log=lines.append)
        logs[name] = (out, torch.load(os.path.join(out['save_path'], 'trlog'), weights_only=False), lines)
    (plain, tr_plain, lines_plain), (cache, tr_cache, lines_cache) = logs['plain'], logs['cache']
    assert set(plain) == {'max_acc', 'max_acc_epoch', 'test_acc', 'test_ci', 'save_path'} and set(cache) == set(plain) | {'eval_cache'}
    assert tr_cache['train_loss'] == tr_plain['train_loss']         # the training step is untouched (and reproducible: what follows compares like with like)
    assert tr_cache['val_loss'] == tr_plain['val_loss'] and tr_cache['val_acc'] == tr_plain['val_acc'] and len(tr_cache['val_loss']) == 2
    assert (cache['test_acc'], cache['test_ci'], cache['max_acc'], cache['max_acc_epoch']) == (plain['test_acc'], plain['test_ci'], plain['max_acc'], plain['max_acc_epoch'])
    assert [l for l in lines_cache if l.startswith(('epo ', 'Test Acc'))] == [l for l in lines_plain if l.startswith(('epo ', 'Test Acc'))]
    # every pass starts from an empty table: after two validation passes over the fixed three episodes the counters are those of one pass
    counters = cache['eval_cache']
    assert counters['val']['n_requests'] == 3 * 2 * 3 and counters['test']['n_requests'] == 4 * 2 * 3
    assert 1 <= counters['val']['n_encoded'] <= 18 and 1 <= counters['test']['n_encoded'] <= 24           # (the splits hold 24 images)
    # the figures of the cached run are those of the plain evaluation of its own saved weights (whatever the training did)
    args = train_deepemd.parse_args(argv)
    model = train_deepemd.build_model(args)
    model.load_state_dict(torch.load(os.path.join(cache['save_path'], 'epoch-1.pth'))['params'])
    dev = torch.device('cuda', torch.cuda.current_device())
    vl, va = train_deepemd.evaluate(model.to(dev), train_deepemd.make_dataset(args, 'val'), args, args.val_episode, dev, seed=args.seed)
    assert vl == tr_cache['val_loss'][0] and float(va.mean()) == tr_cache['val_acc'][0]
