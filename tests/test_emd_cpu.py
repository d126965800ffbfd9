"""DeepEMD head without a GPU: known answers of the float64 oracle (tests/emd_cases.py), the C-ABI declarations of the four entries, the
registry name and the refusals of models/deepemd.py."""
import os
import re

import numpy as np
import pytest
import torch

import emd_cases as ec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('fsvit_emd_head_forward', 'fsvit_emd_head_backward', 'fsvit_emd_head_workspace_bytes', 'fsvit_op_emd_solve')
TINY = dict(img_size=80, init_channels=8, embed_dim=64, depth=[1, 1, 1], num_heads=6, mlp_ratio=4., group=8)


def test_query_equal_to_proto_scores_the_temperature():
    shot, query = ec.token_case(1, 2, 2, 25, 64, seed=3, shared_image=True)
    logits, flows = ec.head_oracle(shot, query, 12.5)
    assert abs(logits[0, 1, 0].item() - 12.5) <= 1e-9            # identical maps: cost 0 on the diagonal, w1 == w2, all mass stays
    assert (flows[0, 1, 0] - torch.diag(torch.diagonal(flows[0, 1, 0]))).abs().max().item() <= 1e-9
    assert (logits[0, 0] < 12.5 - 1e-3).all()


def test_token_permutation_of_one_image_leaves_the_logit_unchanged():
    shot, query = ec.token_case(1, 2, 2, 13, 64, seed=4)
    ref, _ = ec.head_oracle(shot, query, 12.5)
    perm = torch.randperm(13, generator=torch.Generator().manual_seed(0))
    got_q, _ = ec.head_oracle(shot, query[:, :, perm], 12.5)
    shot_p = shot.clone()
    shot_p[0, 1] = shot[0, 1, perm]
    got_p, _ = ec.head_oracle(shot_p, query, 12.5)
    assert (got_q - ref).abs().max().item() <= 1e-9 and (got_p - ref).abs().max().item() <= 1e-9


@pytest.mark.parametrize('cost,w1,w2,optimum,flow', [
    # the diagonal is cheaper: x = F00 as large as it gets, min(w1[0], w2[0])
    ([[0.0, 1.0], [1.0, 0.0]], [1.5, 0.5], [1.0, 1.0], 0.5, [[1.0, 0.5], [0.0, 0.5]]),
    # the anti-diagonal is cheaper: F00 as small as it gets, max(0, w1[0] - w2[1]) = 0.25
    ([[1.0, 0.25], [0.5, 2.0]], [1.25, 0.75], [1.0, 1.0], 0.25 * 1.0 + 1.0 * 0.25 + 0.75 * 0.5, [[0.25, 1.0], [0.75, 0.0]]),
    # c00 + c11 == c01 + c10: every feasible flow is optimal, the optimum is still unique
    ([[0.5, 1.0], [1.0, 1.5]], [0.5, 1.5], [1.0, 1.0], 0.5 * 0.5 + 0.5 * 1.0 + 1.0 * 1.5, None),
])
def test_two_node_problems_solved_by_hand(cost, w1, w2, optimum, flow):
    got, f = ec.solve_transport(np.array(cost), np.array(w1), np.array(w2))
    assert abs(got - optimum) <= 1e-9
    assert np.abs(f.sum(1) - w1).max() <= 1e-9 and np.abs(f.sum(0) - w2).max() <= 1e-9 and f.min() >= -1e-12
    if flow is not None:
        assert np.abs(f - np.array(flow)).max() <= 1e-9


def test_logit_is_temperature_times_one_minus_mean_cost():
    shot, query = ec.token_case(1, 1, 1, 13, 64, seed=5)
    logits, flows = ec.head_oracle(shot, query, 12.5)
    S = ec.similarity_map(ec.centre(shot[0]), ec.centre(query[0]))[0, 0]
    cost = ((1.0 - S) * flows[0, 0, 0]).sum().item()
    assert abs(logits.item() - 12.5 / 13 * (13 - cost)) <= 1e-9


def test_solver_cases_cover_every_kind_with_equal_sums():
    for N in (1, 2, 13, 25, 32):
        kinds, cost, w1, w2 = ec.solver_cases(N)
        assert set(kinds) == set(ec.SOLVER_KINDS) and cost.shape == (32, N, N) and cost.dtype == np.float32
        assert cost.min() >= 0.0 and cost.max() <= 2.0
        assert np.abs(w1.astype(np.float64).sum(1) - N).max() <= N * 2.0 ** -23 and np.abs(w2.astype(np.float64).sum(1) - N).max() <= N * 2.0 ** -23


def test_c_abi_declares_the_four_entries():
    from fewshot_vit_amd import _lib
    header = open(os.path.join(REPO, 'include', 'fsvit.h')).read()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES, name
        assert re.search(r'\b(int|size_t)\s+%s\s*\(' % name, header), name
    assert len(_lib.SIGNATURES['fsvit_emd_head_forward'][1]) == 14
    assert len(_lib.SIGNATURES['fsvit_op_emd_solve'][1]) == 8


def test_deepemd_is_registered_with_the_reference_state_dict_keys():
    from fewshot_vit_amd import models
    from fewshot_vit_amd.models.visformer import Visformer
    assert 'deepemd' in models.models
    models.register('tiny_visformer_emd_cpu')(lambda **kw: Visformer(**TINY, **kw))
    m = models.models['deepemd'](encoder='tiny_visformer_emd_cpu', encoder_args={})
    assert m.encoder.return_map and m.temperature == 12.5
    assert all(k.startswith('encoder.') for k in m.state_dict())          # a SUN-D checkpoint's `params`
    assert set(m.state_dict()) == {'encoder.' + k for k in Visformer(**TINY).state_dict()}


@pytest.mark.parametrize('kwargs', [dict(feature_pyramid=[2, 3]), dict(metric='l2'), dict(solver='qpth'), dict(form='QP'), dict(form='L2')])
def test_refusals_raise_not_implemented(kwargs):
    from fewshot_vit_amd import models
    with pytest.raises(NotImplementedError):
        models.models['deepemd'](encoder='tiny_visformer_emd_cpu_unbuilt', encoder_args={}, **kwargs)


def test_more_than_32_nodes_is_refused():
    from fewshot_vit_amd import models
    from fewshot_vit_amd.models.visformer import Visformer
    models.register('tiny_visformer_emd_cpu')(lambda **kw: Visformer(**TINY, **kw))
    m = models.models['deepemd'](encoder='tiny_visformer_emd_cpu', encoder_args={}, deepemd='grid')
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 2, 1, 33, 3, 80, 80), torch.zeros(1, 2, 33, 3, 80, 80))


def test_status_check_raises_on_a_filled_status_tensor():
    from fewshot_vit_amd.models.deepemd import check_status_count
    check_status_count(torch.zeros(2, 3, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='loop bound'):
        check_status_count(torch.tensor([0, 1, 0], dtype=torch.int32))
