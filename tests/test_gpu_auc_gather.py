"""The --sauc reduction over rows of a feature table (fsvit_proto_auc_gather) on the MI355X: the bits of ops.proto_auc on the gathered copy of the same
rows, exact tie counting, a slot outside the table never becomes an address, and a refused call launches nothing."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (E, shot, n_query, D, N): the smallest geometry (most lanes idle at D = 4), the evaluation's two, and a ragged last pass of the four-wave query loop
# over a table so short that slots repeat within and across episodes
CASES = [(1, 1, 1, 4, 3), (3, 1, 15, 512, 40), (2, 5, 15, 384, 64), (2, 3, 17, 64, 9)]


def _ops():
    from fewshot_vit_amd.engine import ops
    return ops


def _inputs(case):
    E, shot, n_query, D, N = case
    g = torch.Generator().manual_seed(1000 * E + 100 * shot + n_query + D + N)
    table = torch.randn(N, D, generator=g)
    shot_slots = torch.randint(0, N, (E, shot), generator=g)
    query_slots = torch.randint(0, N, (E, 2 * n_query), generator=g)
    return table.to(DEV), shot_slots, query_slots


def _gather(table, shot_slots, query_slots, dtype=torch.int64, invalid=None):
    invalid = torch.zeros(1, dtype=torch.int32, device=DEV) if invalid is None else invalid
    auc, score = _ops().proto_auc_gather(table, shot_slots.to(DEV, dtype), query_slots.to(DEV, dtype), invalid, want_score=True)
    return auc, score, invalid


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'E{}-shot{}-q{}-D{}-N{}'.format(*c))
def test_gather_auc_equals_auc_on_the_gathered_copy(case):
    table, shot_slots, query_slots = _inputs(case)
    want_auc, want_score = _ops().proto_auc(table[shot_slots.to(DEV)].contiguous(), table[query_slots.to(DEV)].contiguous(), want_score=True)
    assert bool(torch.isfinite(want_auc).all()) and bool(torch.isfinite(want_score).all())
    for dtype in (torch.int32, torch.int64):
        auc, score, invalid = _gather(table, shot_slots, query_slots, dtype)
        assert torch.equal(auc, want_auc) and torch.equal(score, want_score), dtype
        assert int(invalid) == 0
    inv = torch.zeros(1, dtype=torch.int32, device=DEV)                    # without the score output: the same auc
    assert torch.equal(_ops().proto_auc_gather(table, shot_slots.to(DEV), query_slots.to(DEV), inv), want_auc) and int(inv) == 0


def test_ties_count_half():
    """rows 0 and 1 of the table are the same vector and sit on both sides: the pair count is an integer ratio with denominator 2 k^2 <= 2^24, exact"""
    from sklearn.metrics import roc_auc_score
    k, D, N = 6, 64, 12
    g = torch.Generator().manual_seed(7)
    table = torch.randn(N, D, generator=g)
    table[1] = table[0]
    shot_slots = torch.tensor([[2, 3]])
    query_slots = torch.tensor([[0, 4, 5, 0, 6, 1, 1, 7, 8, 0, 9, 10]])    # positives 0, 0, 1 - negatives 1, 0: six tied pairs
    auc, score, invalid = _gather(table.to(DEV), shot_slots, query_slots)
    s = score[0].cpu().numpy()
    assert s[0] == s[3] == s[5] == s[6] == s[9]
    want = roc_auc_score(np.array([1] * k + [0] * k), s.astype(np.float64))
    print(f'ties: auc {float(auc[0])!r}, sklearn on the returned scores {want!r}')
    assert float(auc[0]) == float(np.float32(want)) and abs(float(auc[0]) - want) <= 2.0 ** -24
    assert int(invalid) == 0


def test_invalid_slot_poisons_its_episode_only():
    E, shot, n_query, D, N = 4, 2, 5, 128, 20
    table, shot_slots, query_slots = _inputs((E, shot, n_query, D, N))
    bad_shot, bad_query = shot_slots.clone(), query_slots.clone()
    bad_query[1, 3] = -1
    bad_shot[3, 1] = N
    for dtype in (torch.int32, torch.int64):
        clean_auc, clean_score, _ = _gather(table, shot_slots, query_slots, dtype)
        auc, score, invalid = _gather(table, bad_shot, bad_query, dtype)
        for e in (0, 2):
            assert torch.equal(auc[e], clean_auc[e]) and torch.equal(score[e], clean_score[e])
        for e in (1, 3):
            assert bool(torch.isnan(auc[e])) and bool(torch.isnan(score[e]).all())
        assert int(invalid) == 2
        bad_query2 = bad_query.clone()
        bad_query2[1, 0] = N + 5                                           # three bad entries now; the count accumulates across calls
        auc2, _, invalid = _gather(table, bad_shot, bad_query2, dtype, invalid)
        assert int(invalid) == 2 + 3 and torch.equal(auc2[0], clean_auc[0])


def test_refusals_launch_nothing():
    from fewshot_vit_amd import _lib
    from fewshot_vit_amd.engine import _ptr
    lib = _lib.load()
    D = 64
    table = torch.randn(8, D, device=DEV)
    big = torch.zeros(8, 8200, device=DEV)
    shot_slots = torch.zeros(2, 1, dtype=torch.int64, device=DEV)
    query_slots = torch.zeros(2, 4098, dtype=torch.int64, device=DEV)
    auc = torch.full((2,), 7.0, device=DEV)
    score = torch.full((2, 4098), 7.0, device=DEV)
    inv = torch.zeros(1, dtype=torch.int32, device=DEV)
    P = _ptr
    call = lambda t, N, d, Q: lib.fsvit_proto_auc_gather(t, N, d, P(shot_slots), P(query_slots), 1, 2, 1, Q, P(auc), P(score), P(inv), None)
    refused = {'Q odd': call(P(table), 8, D, 3), 'Q 4098': call(P(table), 8, D, 4098), 'N 0': call(P(table), 0, D, 4),
               'D 8200': call(P(big), 8, 8200, 4), 'D 0': call(P(table), 8, 0, 4), 'null table': call(None, 8, D, 4)}
    for what, rc in refused.items():
        assert rc == _lib.ERR_ARG, what
        assert b'fsvit_proto_auc_gather' in lib.fsvit_last_error()
    assert lib.fsvit_proto_auc_gather(P(table), 8, D, P(shot_slots), P(query_slots), 1, 0, 1, 4, P(auc), P(score), P(inv), None) == 0      # E == 0: a no-op
    torch.cuda.synchronize()
    assert bool((auc == 7.0).all()) and bool((score == 7.0).all()) and int(inv) == 0      # nothing ran
    ops = _ops()
    with pytest.raises(ValueError, match='int32 / int64'):
        ops.proto_auc_gather(table, shot_slots.float(), query_slots, inv)
    with pytest.raises(ValueError, match='int32 / int64'):
        ops.proto_auc_gather(table, shot_slots.int(), query_slots, inv)    # two dtypes
    with pytest.raises(ValueError, match='invalid'):
        ops.proto_auc_gather(table, shot_slots, query_slots[:, :4], inv.long())
    with pytest.raises(ValueError):
        ops.proto_auc_gather(table, shot_slots, query_slots[:, :3], inv)   # Q odd through the wrapper
    got = ops.proto_auc_gather(table, shot_slots, query_slots[:, :4], inv) # a good call still goes through (score may be NULL)
    assert bool(torch.isfinite(got).all()) and int(inv) == 0
