"""Host side of the fused SFC fine-tune: the mini-batch table builder (models.deepemd.sfc_step_table) against the loop order of DeepEMD.get_sfc, and
the stability screen of the cases the GPU tests run (tests/emd_sfc_cases.py)."""
import pytest
import torch

import emd_sfc_cases as sc


def _table(perms, bs):
    from fewshot_vit_amd.models.deepemd import sfc_step_table
    return sfc_step_table(perms, bs)


def _loop_order(perms, bs):
    """The mini-batches as get_sfc's loops visit them: for every update step k, for j in range(0, n, bs): perm[:, j:j + bs]."""
    steps, E, n = perms.shape
    return [perms[k][:, j:j + bs] for k in range(steps) for j in range(0, n, bs)]


@pytest.mark.parametrize('steps,E,n,bs', [(3, 2, 10, 4), (2, 1, 6, 4), (1, 3, 4, 8), (2, 2, 4, 1), (1, 1, 25, 4), (2, 2, 8, 4)])
def test_step_table_follows_the_loop_order_of_get_sfc(steps, E, n, bs):
    g = torch.Generator().manual_seed(steps * 100 + n)
    perms = torch.stack([torch.stack([torch.randperm(n, generator=g) for _ in range(E)]) for _ in range(steps)])
    table = _table(perms, bs)
    per = -(-n // bs)
    assert table.shape == (steps * per, E, bs) and table.dtype == torch.int32 and table.device.type == 'cpu' and table.is_contiguous()
    batches = _loop_order(perms, bs)
    assert len(batches) == table.shape[0]
    for row, ids in zip(table, batches):
        b = ids.shape[1]
        assert torch.equal(row[:, :b].long(), ids)
        assert (row[:, b:] == -1).all()                  # the empty slots of a partial batch (every row when bs > n)
    assert int(table.min()) >= -1 and int(table.max()) == n - 1
    # every support image once per update step and episode
    for k in range(steps):
        seen = table[k * per:(k + 1) * per].permute(1, 0, 2).reshape(E, -1)
        assert torch.equal(seen[seen >= 0].reshape(E, n).sort(dim=1).values, torch.arange(n, dtype=torch.int32).expand(E, n))


def test_step_table_takes_one_shared_permutation_per_step():
    perms = torch.tensor([[[2, 0, 1]], [[1, 2, 0]]])
    assert _table(perms, 2).tolist() == [[[2, 0]], [[1, -1]], [[1, 2]], [[0, -1]]]


@pytest.mark.parametrize('name,seed', sc.CASES)
def test_cases_are_stable_under_float32_rounding_of_their_inputs(name, seed):
    dev = sc.screen(name, seed)
    c, maps, perms, ref = sc.sfc_case(name, seed)
    moved = ((ref - maps.mean(dim=2)).abs().max() / ref.abs().max()).item()
    print(f'SFC case {name} seed {seed}: oracle on unrounded vs rounded inputs {dev:.2e} of the largest entry; the fine-tune moves it by {moved:.2e}')
    assert dev <= 1e-5
    assert moved > 0.0
