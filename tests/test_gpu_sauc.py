"""`--sauc` (meta_tuning_sun_m/test_few_shot.py:42-45,95-112): ops.proto_auc against sklearn.metrics.roc_auc_score on float64 scores of the fp32 features,
and eval_sauc.evaluate(..., sauc=True) against ops.proto_auc on the same episode stream."""
import os

import numpy as np
import pytest
import torch
import yaml

import proto_bank_cases as pc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(REPO, 'few-shot-vit_amd', 'configs', 'test_synthetic.yaml')


def _ops():
    from fewshot_vit_amd.engine import ops
    return ops


@pytest.mark.parametrize('case', sorted(pc.SAUC_CASES))
def test_proto_auc_matches_roc_auc_score(case):
    """The inputs hold two constructed ties per episode (Q >= 4) and, asserted here first on the float64 side, every other positive / negative pair is
    further apart than the fp32 allowance of its two scores; then the pair counts agree and the AUC, a count over k^2, matches to 2 * 2^-24.
    The scores themselves are gated like the head's cosine logits at temperature 1 (ho.head_forward)."""
    E, shot, Q, D = case
    fs, fq, n_dup = pc.sauc_inputs(E, shot, Q, D, pc.SAUC_CASES[case])
    s, auc, ok = pc.sauc_reference(fs, fq, n_dup)
    assert ok, 'the seed leaves a pair closer than the fp32 dot-product allowance: choose another (tests/test_proto_bank_cpu.py checks them)'
    got, score = _ops().proto_auc(fs.cuda(), fq.cuda(), want_score=True)
    again = _ops().proto_auc(fs.cuda(), fq.cuda())
    assert torch.equal(got, again)
    k = Q // 2
    for i in range(n_dup):
        assert torch.equal(score[:, i], score[:, k + i]), 'copied rows must score bit-identically'
    from oracle import head_ops_oracle as ho
    r = ho.head_forward(fs.double()[:, None], fq.double(), 1.0, 'cos')
    worst = pc.ratio(score.cpu(), s, r['a_logits'][..., 0])
    err = float((got.cpu().double() - auc).abs().max())
    print(f'proto_auc {case}: score err/bound {worst:.3f}, |auc - sklearn| {err:.3e}, auc {got.tolist()}')
    assert worst <= 1.0
    assert err <= 2.0 * 2.0 ** -24


def _stream(config, n_way, shot, n_query, n_batch):
    """the episode stream evaluate() draws, with the seeds it sets"""
    from fewshot_vit_amd import datasets, parallel, test_few_shot
    from fewshot_vit_amd.datasets.samplers import CategoriesSampler
    test_few_shot.fix_random_seeds(12345)
    dataset = datasets.make(config['dataset'], **config['dataset_args'])
    sampler = CategoriesSampler(dataset.label, n_batch, n_way, shot + n_query, ep_per_batch=1, rank=0, world_size=1, shard=parallel.sampler_shard(1))
    np.random.seed(12345)
    return dataset, [idx for idx in sampler]


def test_evaluate_sauc():
    from fewshot_vit_amd import eval_sauc, test_few_shot, utils
    config = yaml.load(open(CONFIG), Loader=yaml.FullLoader)
    n_batch, shot, n_query = 4, 1, 15
    out = eval_sauc.evaluate(config, shot=shot, n_batch=n_batch, sauc=True, log=lambda *_: None)
    va = out['va_lst']
    assert len(va) == n_batch and out['n'] == n_batch and all(0.0 <= v <= 1.0 for v in va)
    assert out['acc'] == pytest.approx(float(np.mean(va)), abs=1e-12)
    assert out['loss'] == utils.Averager().item()
    # the same episodes through engine.forward + ops.proto_auc
    dataset, stream = _stream(config, 2, shot, n_query, n_batch)
    idx = torch.stack(stream).view(n_batch, 2, shot + n_query)
    model = test_few_shot.build_model(config).cuda().eval()
    engine = model.encoder.engine()
    f_shot = engine.forward(dataset.gather(idx[:, 0, :shot].reshape(-1))).view(n_batch, shot, -1)
    f_query = engine.forward(dataset.gather(idx[:, :, shot:].reshape(-1))).view(n_batch, 2 * n_query, -1)
    want = _ops().proto_auc(f_shot, f_query).double().cpu().tolist()
    print('sauc per episode:', va)
    assert va == want


def test_evaluate_without_sauc_is_the_episode_head():
    """sauc=False hands over to test_few_shot.evaluate, which is left as it was: `acc`, `loss` and `va_lst` are the per-batch accuracy and loss of
    engine.meta_baseline_forward over the same stream"""
    from fewshot_vit_amd import eval_sauc, test_few_shot
    config = yaml.load(open(CONFIG), Loader=yaml.FullLoader)
    n_batch, shot, n_query = 4, 1, 15
    out = eval_sauc.evaluate(config, shot=shot, n_batch=n_batch, sauc=False, log=lambda *_: None)
    assert {'acc', 'ci', 'loss', 'n', 'last_label', 'va_lst'} <= set(out) and len(out['va_lst']) == n_batch
    dataset, stream = _stream(config, 5, shot, n_query, n_batch)
    idx = torch.stack(stream).view(n_batch, 5, shot + n_query)
    data = dataset.gather(torch.cat([idx[:, :, :shot].reshape(-1), idx[:, :, shot:].reshape(-1)]))
    n_s = n_batch * 5 * shot
    model = test_few_shot.build_model(config).cuda().eval()
    logits, acc, loss = model.encoder.engine().meta_baseline_forward(data[:n_s].view(n_batch, 5, shot, *data.shape[1:]),
                                                                      data[n_s:].view(n_batch, 5 * n_query, *data.shape[1:]),
                                                                      float(model.temp.detach()), model.method, want_stats=True)
    assert out['va_lst'] == acc.double().cpu().tolist()
    assert out['acc'] == pytest.approx(float(acc.double().mean()), abs=1e-12)
    assert out['loss'] == pytest.approx(float(loss.double().mean()), abs=1e-12)
    # the two drivers must not drift apart: the sauc dict carries every key of the plain one
    s = eval_sauc.evaluate(config, shot=shot, n_batch=2, sauc=True, log=lambda *_: None)
    assert set(s) == set(out) and set(s['phase_seconds']) == set(out['phase_seconds'])
    with pytest.raises(ValueError, match='collect_pred'):
        eval_sauc.evaluate(config, shot=shot, n_batch=2, sauc=True, collect_pred=True)
