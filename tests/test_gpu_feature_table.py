"""The episode head over gathered rows (fsvit_proto_head_gather) and the drivers' feature cache on the MI355X: the operator gives the bits of
ops.proto_head on the gathered copy, an index outside the table never becomes an address, and eval_cached.evaluate / train_meta report the same
numbers with the cache as without it while encoding every image once."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (E, way, shot, n_query, D, N): the evaluation's two geometries, a tiny one, the LDS limit (way 79 at D 512), a one-slot table
CASES = [(3, 5, 1, 15, 512, 40), (2, 5, 5, 15, 512, 64), (1, 2, 3, 1, 64, 7), (1, 79, 1, 1, 512, 80), (4, 5, 1, 15, 512, 1)]
METHODS = ('cos', 'sqr', 'dot')


def _temp(method, D):
    return 10.0 if method == 'cos' else 4.0 / D


def _inputs(case):
    E, way, shot, n_query, D, N = case
    g = torch.Generator().manual_seed(1000 * E + 10 * way + shot + D + N)
    table = torch.randn(N, D, generator=g)
    idx = torch.randint(0, N, (E, way, shot + n_query), generator=g)       # far more entries than slots: shared between and within episodes
    if E > 1:
        idx[1, 0] = idx[0, 0]                                              # a whole class of episode 0 again in episode 1
    return table.to(DEV), idx


def _gather(table, idx, shot, temp, method, dtype=torch.int64):
    from fewshot_vit_amd.engine import ops
    invalid = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = ops.proto_head_gather(table, idx.to(DEV, dtype), shot, temp, invalid, method)
    return out, invalid


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'E{}-way{}-shot{}-q{}-D{}-N{}'.format(*c))
def test_gather_head_equals_head_on_the_gathered_copy(case):
    from fewshot_vit_amd.engine import ops
    E, way, shot, n_query, D, N = case
    table, idx = _inputs(case)
    rows = table[idx.to(DEV)]                                              # [E, way, shot + n_query, D]
    fs = rows[:, :, :shot].contiguous()
    fq = rows[:, :, shot:].reshape(E, way * n_query, D).contiguous()
    for method in METHODS:
        temp = _temp(method, D)
        want = ops.proto_head(fs, fq, temp, method)
        assert bool(torch.isfinite(want[0]).all())
        for dtype in (torch.int32, torch.int64):
            got, invalid = _gather(table, idx, shot, temp, method, dtype)
            assert _same(got, want), (method, dtype)
            assert int(invalid) == 0
        got, _ = _gather(table, idx, shot, torch.tensor(temp, dtype=torch.float32, device=DEV), method)      # the temperature read on the device
        assert _same(got, want), method
    if E > 1:                                                              # an episode's outputs do not depend on the launch it sits in
        got, _ = _gather(table, idx[1:], shot, _temp('cos', D), 'cos')
        assert _same(got, [w[1:] for w in ops.proto_head(fs, fq, _temp('cos', D), 'cos')])


def test_invalid_index_poisons_its_episode_only():
    from fewshot_vit_amd.feature_table import FeatureTable
    case = CASES[0]
    E, way, shot, n_query, D, N = case
    table, idx = _inputs(case)
    bad = idx.clone()
    bad[1, 2, 0] = -1                                                      # a shot
    bad[1, 4, 7] = N                                                       # a query
    for method in METHODS:
        for dtype in (torch.int32, torch.int64):
            clean, _ = _gather(table, idx, shot, _temp(method, D), method, dtype)
            got, invalid = _gather(table, bad, shot, _temp(method, D), method, dtype)
            for g, c in zip(got, clean):
                assert torch.equal(g[0], c[0]) and torch.equal(g[2], c[2])
                assert bool(torch.isnan(g[1]).all())
            assert int(invalid) == 2
    ft = FeatureTable(lambda index: table[index.to(DEV)], N, D, DEV)
    ft.episodes(torch.arange(N).repeat(6)[:E * way * (shot + n_query)].view(E, -1), way, shot, n_query, 10.0)
    ft.check()                                                             # every slot in range: silent
    ft.n_encoded = N - 1                                                   # the head now sees a table one slot shorter than the slots in use
    ft.episodes(torch.arange(N).repeat(6)[:E * way * (shot + n_query)].view(E, -1), way, shot, n_query, 10.0)
    with pytest.raises(ValueError, match='outside'):
        ft.check()


def test_refusals_launch_nothing():
    from fewshot_vit_amd import _lib
    from fewshot_vit_amd.engine import _ptr, ops
    inv = torch.zeros(1, dtype=torch.int32, device=DEV)
    table = torch.randn(8, 512, device=DEV)
    temp = 10.0
    with pytest.raises(ValueError, match='LDS'):                           # way 80 at D 512: 160 KiB of prototypes alone
        ops.proto_head_gather(table, torch.zeros(1, 80, 2, dtype=torch.int64, device=DEV), 1, temp, inv)
    with pytest.raises(ValueError, match='shot = 0'):
        ops.proto_head_gather(table, torch.zeros(1, 5, 4, dtype=torch.int64, device=DEV), 0, temp, inv)
    with pytest.raises(ValueError):                                        # no query left
        ops.proto_head_gather(table, torch.zeros(1, 5, 4, dtype=torch.int64, device=DEV), 4, temp, inv)
    with pytest.raises(ValueError):                                        # N = 0
        ops.proto_head_gather(table[:0], torch.zeros(1, 5, 4, dtype=torch.int64, device=DEV), 1, temp, inv)
    with pytest.raises(ValueError, match='int32 / int64'):
        ops.proto_head_gather(table, torch.zeros(1, 5, 4, device=DEV), 1, temp, inv)
    lib = _lib.load()
    idx = torch.zeros(1, 5, 4, dtype=torch.int64, device=DEV)
    logits = torch.full((1, 15, 5), 7.0, device=DEV)
    args = lambda t, n, i, lg, iv: (_ptr(t), n, 512, _ptr(i), 1, 1, 5, 1, 3, temp, None, _lib.HEAD_COS, _ptr(lg), None, None, _ptr(iv), None)
    for what, a in {'table': args(None, 8, idx, logits, inv), 'idx': args(table, 8, None, logits, inv), 'logits': args(table, 8, idx, None, inv),
                    'invalid': args(table, 8, idx, logits, None), 'N': args(table, 0, idx, logits, inv)}.items():
        assert lib.fsvit_proto_head_gather(*a) == _lib.ERR_ARG, what
        assert b'fsvit_proto_head_gather' in lib.fsvit_last_error()
    assert lib.fsvit_proto_head_gather(_ptr(table), 8, 512, _ptr(idx), 1, 0, 5, 1, 3, temp, None, _lib.HEAD_COS, _ptr(logits), None, None, _ptr(inv), None) == 0
    torch.cuda.synchronize()
    assert bool((logits == 7.0).all()) and int(inv) == 0                   # nothing ran
    acc = ops.proto_head_gather(table, idx, 1, temp, inv)[1]               # acc / loss may be NULL, a good call still goes through
    assert lib.fsvit_proto_head_gather(*args(table, 8, idx, logits, inv)) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(acc).all())


# ---- the evaluation driver
_IMAGES = dict(split='test', n_classes=8, n_per_class=24, seed=3)


def _eval_config(encoder, tmp_path):
    """the evaluate() config of an 8-class x 24-image split behind `encoder`"""
    if encoder == 'deit_nano_patch6_84':                                   # an 84 x 84 registry ViT: finished float images, a stored checkpoint
        from fewshot_vit_amd import models, synthetic
        m = models.make('meta-baseline', encoder=encoder, encoder_args={})
        sd = synthetic.procedural_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
        path = os.path.join(str(tmp_path), 'deit.pth')
        torch.save({'model': 'meta-baseline', 'model_args': {'encoder': encoder, 'encoder_args': {}}, 'model_sd': sd}, path)
        return {'dataset': 'synthetic-episodes', 'dataset_args': dict(_IMAGES, image_size=84, noise=1.0), 'load': path}
    return {'dataset': 'synthetic-images', 'dataset_args': dict(_IMAGES), 'synthetic_checkpoint': encoder}


def _stream_unique(config, shot, ep_per_batch, n_batch):
    from fewshot_vit_amd import datasets
    from fewshot_vit_amd.datasets.samplers import CategoriesSampler
    label = datasets.make(config['dataset'], **config['dataset_args']).label
    np.random.seed(12345)
    return len(torch.cat(list(CategoriesSampler(label, n_batch, 5, shot + 15, ep_per_batch=ep_per_batch))).unique())


@pytest.mark.parametrize('encoder,shot,ep_per_batch,numerics', [
    ('visformer_micro_80', 1, 1, 'bf16'), ('visformer_micro_80', 5, 2, 'bf16'), ('visformer_micro_80', 1, 2, 'parity'), ('visformer_micro_80', 5, 1, 'parity'),
    ('deit_nano_patch6_84', 1, 2, 'bf16'), ('deit_nano_patch6_84', 5, 1, 'parity'), ('lvvit_micro_80', 5, 1, 'bf16'), ('lvvit_micro_80', 1, 2, 'parity')])
def test_evaluate_with_the_cache_reports_the_same_numbers(tmp_path, encoder, shot, ep_per_batch, numerics):
    from fewshot_vit_amd import eval_cached
    config = _eval_config(encoder, tmp_path)
    kw = dict(shot=shot, n_batch=12, ep_per_batch=ep_per_batch, launch_batches=5, numerics=numerics, log=lambda *_: None, collect_pred=True)
    a = eval_cached.evaluate(config, feature_cache=False, **kw)       # = test_few_shot.evaluate, plus the two counters
    b = eval_cached.evaluate(config, feature_cache=True, **kw)
    assert set(a) == set(b) and set(a['phase_seconds']) == set(b['phase_seconds']) and a['launch_batches'] == b['launch_batches'] == 5
    for k in ('va_lst', 'acc', 'loss', 'ci', 'last_label', 'n'):
        assert a[k] == b[k], k
    assert torch.equal(a['pred'], b['pred'])
    assert len(a['va_lst']) == 12 and np.isfinite(a['va_lst']).all() and np.isfinite(a['loss'])
    requested = 12 * ep_per_batch * 5 * (shot + 15)
    assert a['images_requested'] == b['images_requested'] == a['images_encoded'] == requested
    assert b['images_encoded'] == _stream_unique(config, shot, ep_per_batch, 12) <= 192


def test_cached_driver_follows_test_few_shot_through_the_ramp_and_two_epochs(tmp_path):
    """eval_cached.evaluate runs episodic.evaluate's loop with the table route: the 32-batch first launch, the launch grouping after it, the averagers
    and va_lst kept across epochs and the result dict are held to test_few_shot.evaluate (the dense route), value for value."""
    from fewshot_vit_amd import eval_cached, test_few_shot
    config = _eval_config('visformer_micro_80', tmp_path)
    logs_a, logs_b = [], []
    kw = dict(shot=1, n_batch=40, launch_batches=36, test_epochs=2, numerics='bf16', collect_pred=True)
    a = test_few_shot.evaluate(config, log=logs_a.append, **kw)
    b = eval_cached.evaluate(config, feature_cache=True, log=logs_b.append, **kw)
    assert set(b) - set(a) == {'images_requested', 'images_encoded'} and set(a['phase_seconds']) == set(b['phase_seconds'])
    for k in ('va_lst', 'acc', 'loss', 'ci', 'last_label', 'n', 'launch_batches'):
        assert a[k] == b[k], k
    assert torch.equal(a['pred'], b['pred']) and len(a['va_lst']) == 80
    assert logs_a == logs_b and len(logs_a) == 3                           # num params, then one line per epoch, the same text
    assert b['images_requested'] == 2 * 40 * 5 * 16 and b['images_encoded'] <= 192

# ---- train_meta
def _epoch_lines(config, tmp_path, name):
    from fewshot_vit_amd import train_meta
    lines = []
    trlog = train_meta.main(config, name=name, device=torch.device('cuda', 0), log=lines.append, save_root=str(tmp_path))
    return trlog, lines


def test_train_meta_eval_loops_with_the_cache(tmp_path):
    ds = dict(n_classes=8, n_per_class=24)
    config = dict(train_dataset='synthetic-episodes', train_dataset_args=dict(split='train', n_per_class=20, n_classes=8, noise=1.0, seed=1),
                  tval_dataset='synthetic-images', tval_dataset_args=dict(split='test', seed=0, **ds),
                  val_dataset='synthetic-images', val_dataset_args=dict(split='val', seed=2, **ds),
                  model='meta-baseline', model_args=dict(encoder='visformer_micro_80', encoder_args=dict(drop_path_rate=0.1, numerics='bf16')),
                  synthetic_checkpoint='visformer_micro_80', n_train_way=5, n_train_shot=1, n_train_query=3, n_way=5, n_shot=1, n_query=15,
                  train_batches=2, eval_batches=3, ep_per_batch=2, max_epoch=2, optimizer='sgd', optimizer_args=dict(lr=0.01, weight_decay=5e-4))
    plain, lines_plain = _epoch_lines(dict(config), tmp_path, 'plain')
    cached, lines = _epoch_lines(dict(config, eval_feature_cache=True), tmp_path, 'cached')
    for k in ('tvl', 'tva', 'vl', 'va'):
        assert plain[k] == cached[k], k
    assert len(plain['tvl']) == 2 and all(np.isfinite(plain[k]).all() for k in plain)
    assert not any('feature cache' in l for l in lines_plain)
    counts = {}
    for l in lines:
        m = re.match(r'epoch (\d+), (\w+) feature cache: (\d+) images encoded for (\d+) requested', str(l))
        if m:
            counts[int(m.group(1)), m.group(2)] = (int(m.group(3)), int(m.group(4)))
    assert sorted(counts) == [(1, 'tval'), (1, 'val'), (2, 'tval'), (2, 'val')]
    for (epoch, nm), (encoded, requested) in counts.items():
        assert requested == 3 * 4 * 5 * 16                                 # eval_batches x 4 episodes x 5-way x (1 + 15): this epoch's alone
        assert 0 < encoded <= 8 * 24
        assert (encoded, requested) == counts[1, nm]                       # the table was emptied: epoch 2 encodes the same stream again
