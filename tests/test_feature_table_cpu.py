"""Host-side checks of the feature table (no GPU): the gather head is declared in fsvit.h and bound with the same argument list, FeatureTable's
bookkeeping encodes every image once whatever the requests look like, and for_dataset refuses what has no single feature per image."""
import ctypes as C
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gather_head_is_declared_and_bound():
    from fewshot_vit_amd import _lib
    from fewshot_vit_amd.engine import ops
    header = open(os.path.join(REPO, 'include', 'fsvit.h')).read()
    m = re.search(r'\bint\s+fsvit_proto_head_gather\s*\(([^;]*?)\)\s*;', header, re.S)
    assert m
    want = []
    for p in m.group(1).split(','):
        p = re.sub(r'/\*.*?\*/', '', p, flags=re.S).strip()
        want.append(C.c_void_p if '*' in p else {'int': C.c_int, 'float': C.c_float}[p.split()[-2]])
    res, args = _lib.SIGNATURES['fsvit_proto_head_gather']
    assert res is C.c_int and args == want and len(args) == 17
    assert hasattr(_lib.load(), 'fsvit_proto_head_gather')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.proto_head_gather(torch.zeros(4, 8), torch.zeros(1, 2, 2, dtype=torch.int64), 1, 10.0, torch.zeros(1, dtype=torch.int32))


def _fake_table(n_images=20, dim=6, chunk=4):
    from fewshot_vit_amd.feature_table import FeatureTable
    calls = []

    def encode_fn(index):
        calls.append(index.clone())
        return index[:, None].float() * torch.ones(dim)

    return FeatureTable(encode_fn, n_images, dim, 'cpu', chunk_images=chunk), calls


def test_ensure_encodes_every_image_once():
    table, calls = _fake_table()
    requests = [torch.tensor([[7, 3, 7], [15, 3, 0]]),              # repeats inside one request, out of order, 2-d
                torch.tensor([19, 18, 7, 2, 11, 12, 13, 3, 1, 0]),  # overlaps the first; 7 new images: two chunks
                torch.tensor([15, 4, 4, 19])]                       # one new image
    for r in requests:
        slots = table.ensure(r)
        assert slots.shape == r.shape and slots.dtype == torch.int32
        assert int(slots.min()) >= 0 and int(slots.max()) < table.n_encoded
        assert torch.equal(table.feat[slots.reshape(-1).long()], r.reshape(-1)[:, None].float() * torch.ones(table.dim))      # the right rows
    unique = sorted(set(torch.cat([r.reshape(-1) for r in requests]).tolist()))
    encoded = torch.cat(calls).tolist()
    assert sorted(encoded) == unique and len(encoded) == len(unique)                    # exactly once each
    assert all(1 <= len(c) <= 4 and c.dtype == torch.int64 and torch.equal(c, c.sort().values) for c in calls)
    assert [c.tolist() for c in calls] == [[0, 3, 7, 15], [1, 2, 11, 12], [13, 18, 19], [4]]
    assert table.n_encoded == len(unique) == 12 and table.n_requests == 6 + 10 + 4
    assert sorted(table.slot_of[table.slot_of >= 0].tolist()) == list(range(12))        # slots are dense, in encode order
    assert table.slot_of[0] == 0 and table.slot_of[15] == 3 and table.slot_of[4] == 11
    n_calls = len(calls)
    table.ensure(torch.tensor(unique))                                                  # nothing new: no call
    assert len(calls) == n_calls and table.n_encoded == 12
    table.reset()
    assert table.n_encoded == 0 and table.n_requests == 0 and bool((table.slot_of == -1).all())
    assert table.ensure(torch.tensor([5, 5])).tolist() == [0, 0] and calls[-1].tolist() == [5] and table.n_encoded == 1


def test_ensure_refusals():
    table, calls = _fake_table()
    for bad in ([-1], [20], [3, 25]):
        with pytest.raises(IndexError):
            table.ensure(torch.tensor(bad))
    assert not calls and table.n_encoded == 0
    assert table.ensure(torch.zeros(0, dtype=torch.int64)).shape == (0,)
    from fewshot_vit_amd.feature_table import FeatureTable
    wrong = FeatureTable(lambda index: torch.zeros(len(index), 5), 8, 6, 'cpu')
    with pytest.raises(ValueError, match='encode_fn returned'):
        wrong.ensure(torch.tensor([1, 2]))
    with pytest.raises(ValueError):
        FeatureTable(lambda index: None, 0, 6, 'cpu')
    with pytest.raises(ValueError, match='whole number'):
        table.episodes(torch.arange(7), 2, 1, 2, 10.0)


def test_for_dataset_refusals():
    from fewshot_vit_amd import datasets, models
    from fewshot_vit_amd.feature_table import FeatureTable
    model = models.make('meta-baseline', encoder='visformer_micro_80', encoder_args={}).cpu()
    small = dict(split='test', n_classes=2, n_per_class=2, device='cpu')
    with pytest.raises(ValueError, match='no single feature per image'):
        FeatureTable.for_dataset(model.eval(), datasets.make('synthetic-images', augment='resize', **small))
    for patches in ('grid', 'sampling'):
        with pytest.raises(ValueError, match='no single feature per image'):
            FeatureTable.for_dataset(model.eval(), datasets.make('synthetic-images', patches=patches, **small))
    with pytest.raises(ValueError, match='train mode'):
        FeatureTable.for_dataset(model.train(), datasets.make('synthetic-images', **small))


def test_driver_lists_the_switch_and_keeps_the_evaluate_surface(capsys):
    import inspect
    from fewshot_vit_amd import eval_cached, test_few_shot
    with pytest.raises(SystemExit) as e:
        eval_cached.main(['--help'])
    text = capsys.readouterr().out
    assert e.value.code == 0
    for flag in ('--feature-cache', '--config', '--shot', '--test-epochs', '--gpu', '--episodes', '--ep-per-batch', '--launch-batches', '--numerics'):
        assert flag in text, flag
    mine, theirs = inspect.signature(eval_cached.evaluate).parameters, inspect.signature(test_few_shot.evaluate).parameters
    assert mine['feature_cache'].default is False                    # off unless asked for
    assert [(k, p.default) for k, p in mine.items() if k != 'feature_cache'] == [(k, p.default) for k, p in theirs.items()]
