"""episodic.py without a GPU: the launch grouping, the two reductions and the image gather the evaluation drivers share."""
import numpy as np
import pytest
import scipy.stats
import torch


def _stream(n):
    return [torch.tensor([10 * i, 10 * i + 1]) for i in range(n)]


def _evaluate_ramp(launch_batches):
    return [n for n in (32,) if n < launch_batches]             # the rule evaluate() passes


@pytest.mark.parametrize('n,launch_batches,ramp,sizes', [
    (40, 36, None, [32, 8]), (12, 5, None, [5, 5, 2]), (70, 32, None, [32, 32, 6]), (0, 36, None, []), (0, 1, None, []), (7, 3, (), [3, 3, 1]),
    (64, 32, None, [32, 32]), (33, 64, None, [32, 1]), (10, 4, (1, 2), [1, 2, 4, 3])])
def test_launch_groups_known_answers(n, launch_batches, ramp, sizes):
    from fewshot_vit_amd.episodic import launch_groups
    stream = _stream(n)
    ramp = _evaluate_ramp(launch_batches) if ramp is None else ramp
    before = list(ramp)
    groups = list(launch_groups(iter(stream), launch_batches, ramp))
    assert [len(g) for g in groups] == sizes
    flat = [idx for g in groups for idx in g]
    assert len(flat) == n and all(a is b for a, b in zip(flat, stream))      # the sampler's stream, in order, nothing copied
    assert list(ramp) == before                                              # the caller's ramp is not consumed: every epoch starts with it


def test_launch_groups_default_has_no_ramp_and_runs_a_launch_before_the_next_draw():
    from fewshot_vit_amd.episodic import launch_groups
    drawn = []

    def sampler():
        for idx in _stream(5):
            drawn.append(idx)
            yield idx

    seen = []
    for group in launch_groups(sampler(), 2):
        seen.append((len(group), len(drawn)))
    assert seen == [(2, 2), (2, 4), (1, 5)]


def _ci(va):
    a = np.array(va, dtype=np.float64)
    return float(scipy.stats.sem(a) * scipy.stats.t.ppf(0.975, len(a) - 1))


def test_reduce_batches_over_two_epochs():
    from fewshot_vit_amd import episodic, utils
    items = 2 * 5 * 16
    e1 = np.array([[0.5, 1.25], [0.75, 0.5], [1.0, 0.125]])     # [n_batch, (acc, loss)]
    e2 = np.array([[0.25, 2.0], [0.625, 0.75], [0.875, 1.5]])
    aves_va, aves_vl, va_lst = utils.Averager(), utils.Averager(), []
    episodic.reduce_batches(e1, aves_va, aves_vl, va_lst, items)
    assert va_lst == [0.5, 0.75, 1.0] and aves_va.item() == 0.75 and aves_vl.item() == 0.625
    assert float(utils.mean_confidence_interval(va_lst)) == pytest.approx(_ci([0.5, 0.75, 1.0]), rel=1e-12)
    episodic.reduce_batches(e2, aves_va, aves_vl, va_lst, items)                 # the second epoch extends the same lists
    acc = [0.5, 0.75, 1.0, 0.25, 0.625, 0.875]
    loss = [1.25, 0.5, 0.125, 2.0, 0.75, 1.5]
    assert va_lst == acc and len(va_lst) == 6
    assert aves_va.item() == sum(a * items for a in acc) / (6 * items) and aves_vl.item() == sum(l * items for l in loss) / (6 * items)
    assert aves_va.n == aves_vl.n == 6 * items
    assert float(utils.mean_confidence_interval(va_lst)) == pytest.approx(_ci(acc), rel=1e-12)


def test_reduce_episodes_over_two_epochs():
    from fewshot_vit_amd import episodic, utils
    items = 2 * 2 * 16
    e1 = np.array([[0.5, 1.0], [0.75, 0.25], [1.0, 0.625]])     # [n_batch, ep_per_batch] AUCs
    e2 = np.array([[0.125, 0.875], [0.375, 1.0], [0.5, 0.5]])
    aves_va, aves_vl, va_lst = utils.Averager(), utils.Averager(), []
    episodic.reduce_episodes(e1, aves_va, aves_vl, va_lst, items)
    first = [0.5, 1.0, 0.75, 0.25, 1.0, 0.625]                  # per episode, batch-major
    assert va_lst == first and aves_va.item() == sum(first) / 6
    episodic.reduce_episodes(e2, aves_va, aves_vl, va_lst, items)
    both = first + [0.125, 0.875, 0.375, 1.0, 0.5, 0.5]
    assert va_lst == both and len(va_lst) == 12
    assert aves_va.item() == sum(a * items for a in both) / (12 * items) and aves_va.n == 12 * items
    assert aves_vl.n == 0 and aves_vl.item() == utils.Averager().item()          # the loss averager is never fed under --sauc
    assert float(utils.mean_confidence_interval(va_lst)) == pytest.approx(_ci(both), rel=1e-12)


class _Host:
    """image i is the constant i; (image, label) items as the datasets return them"""
    label = [0, 0, 1, 1, 2, 2]

    def __init__(self):
        self.items = []

    def __getitem__(self, i):
        assert isinstance(i, int)
        self.items.append(i)
        return torch.full((3, 2, 2), float(i)), self.label[i]


class _Resident(_Host):
    def gather(self, index):
        self.gathers = getattr(self, 'gathers', []) + [index]
        return torch.stack([torch.full((3, 2, 2), float(i) + 0.5) for i in index])


def test_gather_images_with_and_without_gather():
    from fewshot_vit_amd.episodic import gather_images
    index = torch.tensor([4, 1, 1, 5])
    host = _Host()
    x = gather_images(host, index, torch.device('cpu'))
    assert x.shape == (4, 3, 2, 2) and x[:, 0, 0, 0].tolist() == [4.0, 1.0, 1.0, 5.0] and host.items == [4, 1, 1, 5]
    resident = _Resident()
    y = gather_images(resident, index, torch.device('cpu'))
    assert y[:, 0, 0, 0].tolist() == [4.5, 1.5, 1.5, 5.5] and not resident.items          # the dataset's own gather, no per-item access
    assert len(resident.gathers) == 1 and resident.gathers[0] is index


def test_head_temp_forms():
    from fewshot_vit_amd.episodic import head_temp

    class M:
        pass

    m = M()
    m.temp = torch.nn.Parameter(torch.tensor(12.5))
    assert head_temp(m) == 12.5 and type(head_temp(m)) is float
    t = head_temp(m, on_device=True)
    assert isinstance(t, torch.Tensor) and not t.requires_grad and t.data_ptr() == m.temp.data_ptr()
    m.temp = 10
    assert head_temp(m) == 10.0 and type(head_temp(m)) is float and type(head_temp(m, on_device=True)) is float


def test_the_drivers_share_the_helpers_and_one_command_line():
    from fewshot_vit_amd import episodic, eval_sauc, test_few_shot, train_meta
    assert test_few_shot.fix_random_seeds is train_meta.fix_random_seeds is episodic.fix_random_seeds
    assert test_few_shot.build_model is episodic.build_model and test_few_shot.default_launch_batches is episodic.default_launch_batches
    flags = lambda p: sorted(s for a in p._actions for s in a.option_strings)
    plain, both = episodic.make_parser(), eval_sauc.make_parser()
    assert set(flags(both)) - set(flags(plain)) == {'--sauc', '--feature-cache'}
    args = both.parse_args([])
    assert (args.shot, args.test_epochs, args.episodes, args.ep_per_batch, args.launch_batches, args.numerics, args.sauc, args.feature_cache) == \
        (1, 1, 2000, 1, None, None, False, False)
    assert args.config == './configs/test_few_shot.yaml' and args.gpu is None
