"""The feature-table switch of the --sauc, distillation and classifier evaluations on the MI355X: eval_sauc.evaluate, train_classifier's fs-eval block and
offline.py's validation / fs-eval report with the switch what they report without it, while every image an evaluation touches is encoded once.

Datasets: the fs-eval block and --sauc draw up to 5 + 15 images per class, so their splits are 6 classes x 24 images; offline's validation split is
6 x 12."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
TINY = dict(img_size=80, init_channels=8, embed_dim=64, depth=[1, 1, 1], num_heads=6, mlp_ratio=4., group=8)       # the encoder of test_gpu_emd.py
ENCODER = 'tiny_visformer_tables'
D = 128                                                                    # its pooled feature
B_LOGIT = 2 * (D + 8) * 2.0 ** -24 * 10                                    # see test_offline_with_the_cache_against_the_torch_route


def _register():
    from fewshot_vit_amd import models
    from fewshot_vit_amd.models.visformer import Visformer
    models.register(ENCODER)(lambda **a: Visformer(**TINY, **a))


def _quiet(*_):
    pass


# ---- eval_sauc
def _sauc_config(tmp_path):
    """a 6-class x 24-image split behind a stored meta-baseline over the tiny encoder (default initialisation, seed 0)"""
    from fewshot_vit_amd import models
    _register()
    torch.manual_seed(0)
    m = models.make('meta-baseline', encoder=ENCODER, encoder_args={})
    path = os.path.join(str(tmp_path), 'tiny.pth')
    torch.save({'model': 'meta-baseline', 'model_args': {'encoder': ENCODER, 'encoder_args': {}}, 'model_sd': m.state_dict()}, path)
    return {'dataset': 'synthetic-images', 'dataset_args': dict(split='test', n_classes=6, n_per_class=24, seed=3), 'load': path}


@pytest.mark.parametrize('shot,ep_per_batch', [(1, 1), (5, 2)])
def test_eval_sauc_with_the_cache_reports_the_same_numbers(tmp_path, shot, ep_per_batch):
    from fewshot_vit_amd import datasets, eval_sauc
    from fewshot_vit_amd.datasets.samplers import CategoriesSampler
    config = _sauc_config(tmp_path)
    n_batch = 6
    kw = dict(shot=shot, n_batch=n_batch, ep_per_batch=ep_per_batch, launch_batches=4, numerics='parity', sauc=True, log=_quiet)      # two flushes: 4 + 2
    a = eval_sauc.evaluate(config, feature_cache=False, **kw)
    b = eval_sauc.evaluate(config, feature_cache=True, **kw)
    assert set(a) == set(b) and set(a['phase_seconds']) == set(b['phase_seconds']) and a['launch_batches'] == b['launch_batches'] == 4
    for k in ('va_lst', 'acc', 'ci', 'n', 'last_label'):
        assert a[k] == b[k], k
    assert len(a['va_lst']) == n_batch * ep_per_batch and np.isfinite(a['va_lst']).all() and a['loss'] == b['loss']
    label = datasets.make(config['dataset'], **config['dataset_args']).label
    np.random.seed(12345)                                                  # the stream evaluate() draws
    idx = torch.stack(list(CategoriesSampler(label, n_batch, 2, shot + 15, ep_per_batch=ep_per_batch))).view(-1, 2, shot + 15)
    used = torch.cat([idx[:, 0, :shot].reshape(-1), idx[:, :, shot:].reshape(-1)])
    assert a['images_requested'] == a['images_encoded'] == b['images_requested'] == used.numel() == n_batch * ep_per_batch * (shot + 30)
    assert b['images_encoded'] == len(used.unique()) < b['images_requested']
    print(f'sauc shot {shot}: {b["images_encoded"]} images encoded for {b["images_requested"]} requested, auc {b["va_lst"]}')


def test_eval_sauc_routes_agree_through_the_ramp_and_two_epochs():
    """Both AUC routes of episodic.evaluate on the 8-class x 24-image split behind visformer_micro_80 in bf16: 40 batches at launch_batches=36 are a
    32-batch first launch and one of 8, twice; the averagers and va_lst run on across the epochs.  The table encodes no image twice (<= 192); the dense
    route encodes per episode the shot of class 0 and the 2 x 15 queries."""
    from fewshot_vit_amd import eval_sauc
    config = {'dataset': 'synthetic-images', 'dataset_args': dict(split='test', n_classes=8, n_per_class=24, seed=3), 'synthetic_checkpoint': 'visformer_micro_80'}
    logs_a, logs_b = [], []
    kw = dict(shot=1, n_batch=40, launch_batches=36, test_epochs=2, numerics='bf16', sauc=True)
    a = eval_sauc.evaluate(config, feature_cache=False, log=logs_a.append, **kw)
    b = eval_sauc.evaluate(config, feature_cache=True, log=logs_b.append, **kw)
    print(f'sauc ramp: acc {a["acc"]} +- {a["ci"]}, encoded {b["images_encoded"]} of {b["images_requested"]} requested, dense {a["images_requested"]}')
    assert set(a) == set(b)
    for k in ('va_lst', 'acc', 'ci', 'loss', 'n', 'last_label', 'launch_batches'):
        assert a[k] == b[k], k
    assert logs_a == logs_b and len(logs_a) == 3                           # num params, then one line per epoch, the same text
    assert len(a['va_lst']) == 80 and np.isfinite(a['va_lst']).all()
    assert b['images_encoded'] <= 192
    assert a['images_requested'] == 2 * 40 * (1 + 2 * 15)


def test_eval_sauc_without_sauc_takes_the_cached_episode_driver(tmp_path):
    from fewshot_vit_amd import eval_cached, eval_sauc
    config = _sauc_config(tmp_path)
    kw = dict(shot=1, n_batch=3, launch_batches=2, numerics='parity', log=_quiet)
    a = eval_cached.evaluate(config, feature_cache=True, **kw)
    b = eval_sauc.evaluate(config, sauc=False, feature_cache=True, **kw)
    assert set(a) == set(b)
    for k in ('va_lst', 'acc', 'loss', 'ci', 'n', 'last_label', 'images_requested', 'images_encoded'):
        assert a[k] == b[k], k
    assert b['images_encoded'] < b['images_requested'] == 3 * 5 * 16


# ---- train_classifier
_TRAIN = dict(train_dataset='synthetic-episodes', train_dataset_args=dict(split='train', n_classes=6, n_per_class=12, noise=1.0, seed=1),
              batch_size=16, train_batches=2, max_epoch=2, optimizer='adamw', optimizer_args=dict(lr=5e-4, weight_decay=0.05, warmup_lr=1e-6, warmup=1))
_FS = dict(fs_dataset='synthetic-episodes', fs_dataset_args=dict(split='test', n_classes=6, n_per_class=24, noise=1.0, seed=0), fs_batches=3)
_ENC = dict(encoder=ENCODER, encoder_args=dict(drop_path_rate=0.1, numerics='parity'), classifier='linear-classifier', classifier_args=dict(n_classes=6))


def _counts(lines, what):
    out = {}
    for l in lines:
        m = re.match(r'epoch (\d+), ' + what + r' feature cache: (\d+) images encoded for (\d+) requested', str(l))
        if m:
            out[int(m.group(1))] = (int(m.group(2)), int(m.group(3)))
    return out


def test_train_classifier_fs_eval_with_the_cache(tmp_path):
    from fewshot_vit_amd import train_classifier
    _register()
    config = dict(_TRAIN, **_FS, eval_fs_epoch=1, model='classifier', model_args=_ENC,
                  val_dataset='synthetic-episodes', val_dataset_args=dict(split='train', n_classes=6, n_per_class=4, noise=1.0, seed=1))
    logs = {}
    for name, cache in (('plain', False), ('cached', True)):
        torch.manual_seed(0)
        lines = []
        logs[name] = (train_classifier.main(dict(config, eval_feature_cache=cache), name=name, device=DEV, log=lines.append, save_root=str(tmp_path)), lines)
    plain, cached = logs['plain'][0], logs['cached'][0]
    assert set(plain) == set(cached) == {'tl', 'ta', 'vl', 'va', 'fsa-1', 'fsa-5'}
    for k in plain:
        assert plain[k] == cached[k], k                                    # epoch 2 agrees only if the table was emptied after epoch 1's steps
        assert len(plain[k]) == 2 and np.isfinite(plain[k]).all()
    assert not _counts(logs['plain'][1], 'fs')
    counts = _counts(logs['cached'][1], 'fs')
    assert sorted(counts) == [1, 2]
    for encoded, requested in counts.values():
        assert requested == 3 * 4 * 5 * (16 + 20) and 0 < encoded <= 6 * 24   # both shot settings fill one table
    print('train_classifier fsa-1 / fsa-5:', plain['fsa-1'], plain['fsa-5'], 'encoded / requested:', counts)


# ---- offline.py
def _offline_config(**kw):
    return dict(_TRAIN, val_dataset='synthetic-episodes', val_dataset_args=dict(split='val', n_classes=6, n_per_class=12, noise=1.0, seed=2),
                model='token-label', model_args=_ENC, n_way=5, n_shot=1, n_query=3, ep_per_batch=2, eval_batches=3, tl_soft_k=3, bg_token_num=10, **kw)


def _offline(config, tmp_path, name, seed=0):
    from fewshot_vit_amd import offline
    _register()
    torch.manual_seed(seed)
    lines = []
    return offline.main(config, name=name, device=DEV, log=lines.append, save_root=str(tmp_path)), lines


def test_offline_fs_eval_block_without_the_cache(tmp_path):
    trlog, lines = _offline(_offline_config(), tmp_path, 'nofs')
    assert list(trlog) == ['tl', 'ta', 'vl', 'va'] and all(len(v) == 2 for v in trlog.values())
    assert not any('fs ' in str(l) or 'feature cache' in str(l) for l in lines if str(l).startswith('epoch'))
    trlog, lines = _offline(_offline_config(**_FS, eval_fs_epoch=2), tmp_path, 'fs')
    assert set(trlog) == {'tl', 'ta', 'vl', 'va', 'fsa-1', 'fsa-5'} and len(trlog['tl']) == len(trlog['va']) == 2
    assert len(trlog['fsa-1']) == len(trlog['fsa-5']) == 1                 # one entry per evaluated epoch: epoch 2 alone
    assert 0.0 <= trlog['fsa-1'][0] <= 1.0 and 0.0 <= trlog['fsa-5'][0] <= 1.0
    epoch_lines = [str(l) for l in lines if re.match(r'epoch \d+, train', str(l))]
    assert len(epoch_lines) == 2 and ', fs 1:' not in epoch_lines[0]
    assert re.search(r'val [\d.]+\|[\d.]+, fs 1: {:.4f} 5: {:.4f}, '.format(trlog['fsa-1'][0], trlog['fsa-5'][0]), epoch_lines[1])


def test_offline_table_logits_are_the_head_on_the_models_pooled_feature():
    """offline.table_eval_logits - the helper the driver's table route calls for every evaluation - against ops.proto_head ('cos', temperature 10.0) on
    `model(x)[2]` of the gathered images, batch by batch"""
    from fewshot_vit_amd import datasets, models, offline
    from fewshot_vit_amd.datasets.samplers import CategoriesSampler
    from fewshot_vit_amd.engine import ops
    from fewshot_vit_amd.feature_table import FeatureTable
    _register()
    torch.manual_seed(0)
    model = models.make('token-label', **dict(_ENC, encoder_args=dict(_ENC['encoder_args'], return_map=True))).to(DEV).eval()
    dataset = datasets.make('synthetic-episodes', split='test', n_classes=6, n_per_class=24, noise=1.0, seed=0)
    for shot, n_query, ep in ((1, 15, 2), (5, 15, 4)):
        sampler = CategoriesSampler(dataset.label, 3, 5, shot + n_query, ep_per_batch=ep)
        table = FeatureTable.for_dataset(model, dataset)
        np.random.seed(0)
        got = offline.table_eval_logits(table, sampler, 5, shot, n_query)
        assert got.shape == (3, ep * 5 * n_query, 5) and table.n_encoded < table.n_requests == 3 * ep * 5 * (shot + n_query)
        np.random.seed(0)
        for g, idx in enumerate(sampler):
            x = torch.stack([dataset[int(i)][0] for i in idx]).to(DEV)
            with torch.no_grad():
                feat = model(x)[2].view(ep, 5, shot + n_query, D)
            want = ops.proto_head(feat[:, :, :shot].contiguous(), feat[:, :, shot:].reshape(ep, 5 * n_query, D).contiguous(), 10.0, 'cos')[0]
            assert torch.equal(got[g], want.view(-1, 5)), (shot, g)


def test_offline_with_the_cache_against_the_torch_route(tmp_path, monkeypatch):
    """Two epochs with validation and the fs-eval block, switch off and on, from the same seed.  The bound is derived, not measured: both routes evaluate
    10 <q^, p^> on the same fp32 features, each within (D + 8) 2^-24 10 of the exact value (unit vectors: sum |a_i b_i| <= 1; the 8 covers the mean and
    the two normalisations), so logits differ by at most b = 2 (D + 8) 2^-24 10 = 1.6e-4 at D = 128; cross-entropy is 1-Lipschitz in the sup norm of the
    logits, so |d vl| <= b; accuracy can differ only on queries whose two largest logits on the table route lie within 2 b of each other - their share
    bounds |d va| and |d fsa-*|, and is capped at 1 % (a cap on the data, not a measurement: seed 3 of the model initialisation leaves at most 4 of 900
    queries of any evaluation that close; seed 0 leaves 3 of the 90 validation queries of epoch 1)."""
    from fewshot_vit_amd import offline
    seen = []
    inner = offline.table_eval_logits

    def recording(table, sampler, n_way, n_shot, n_query):
        logits = inner(table, sampler, n_way, n_shot, n_query)
        seen.append((n_shot, n_query, logits.detach().cpu()))
        return logits

    config = _offline_config(**_FS, eval_fs_epoch=1)
    plain, lines_plain = _offline(config, tmp_path, 'plain', seed=3)
    monkeypatch.setattr(offline, 'table_eval_logits', recording)
    cached, lines = _offline(dict(config, eval_feature_cache=True), tmp_path, 'cached', seed=3)
    assert len(seen) == 2 * 3                                              # per epoch: validation, fs 1-shot, fs 5-shot - the driver went through the helper
    assert plain['tl'] == cached['tl'] and plain['ta'] == cached['ta']    # the same training run
    assert set(plain) == set(cached) and all(len(cached[k]) == 2 and np.isfinite(cached[k]).all() for k in cached)
    for epoch in range(2):
        for j, key in enumerate(('va', 'fsa-1', 'fsa-5')):
            n_shot, n_query, logits = seen[3 * epoch + j]
            assert (n_shot, n_query) == ((1, 3), (1, 15), (5, 15))[j]
            top2 = logits.reshape(-1, 5).topk(2, dim=1).values
            share = float((top2[:, 0] - top2[:, 1] <= 2 * B_LOGIT).double().mean())
            d_acc = abs(plain[key][epoch] - cached[key][epoch])
            print(f'offline epoch {epoch + 1} {key}: |d acc| {d_acc:.3e}, near-tie share {share:.3e}' +
                  (f', |d vl| {abs(plain["vl"][epoch] - cached["vl"][epoch]):.3e} (bound {B_LOGIT:.3e})' if key == 'va' else ''))
            assert share < 0.01
            assert d_acc <= share + 1e-12
        assert abs(plain['vl'][epoch] - cached['vl'][epoch]) <= B_LOGIT
    assert not _counts(lines_plain, 'val') and not _counts(lines_plain, 'fs')
    val, fsc = _counts(lines, 'val'), _counts(lines, 'fs')
    assert sorted(val) == sorted(fsc) == [1, 2]
    for epoch in (1, 2):
        assert val[epoch][1] == 3 * 2 * 5 * 4 and 0 < val[epoch][0] <= 6 * 12
        assert fsc[epoch][1] == 3 * 4 * 5 * (16 + 20) and 0 < fsc[epoch][0] <= 6 * 24
        assert val[epoch] == val[1] and fsc[epoch] == fsc[1]               # emptied every epoch: the same stream is encoded again


def test_offline_refuses_the_cache_over_a_random_augment(tmp_path):
    config = _offline_config(eval_feature_cache=True)
    config.update(val_dataset='synthetic-images', val_dataset_args=dict(split='val', n_classes=6, n_per_class=12, seed=2, augment='resize'))
    with pytest.raises(ValueError, match='no single feature per image'):
        _offline(config, tmp_path, 'refused')
