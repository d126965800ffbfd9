"""Host-side checks of the DeepEMD token-map table (no GPU): the two C entries are declared in fsvit.h and bound with the same argument lists,
TokenTable's bookkeeping encodes every image once whatever the requests look like, for_dataset refuses what has no single node set per image, and
both driver flags are off unless asked for."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {'int': C.c_int, 'float': C.c_float, 'size_t': C.c_size_t}


@pytest.mark.parametrize('name,restype,n_args', [('fsvit_emd_table_prep', 'int', 7), ('fsvit_emd_head_gather_workspace_bytes', 'size_t', 4),
                                                 ('fsvit_emd_head_gather', 'int', 20)])
def test_entries_are_declared_and_bound(name, restype, n_args):
    from fewshot_vit_amd import _lib
    header = open(os.path.join(REPO, 'include', 'fsvit.h')).read()
    m = re.search(r'\b%s\s+%s\s*\(([^;]*?)\)\s*;' % (restype, name), header, re.S)
    assert m, name
    want = []
    for p in m.group(1).split(','):
        p = re.sub(r'/\*.*?\*/', '', p, flags=re.S).strip()
        want.append(C.c_void_p if '*' in p else C_TYPES[p.split()[-2]])
    res, args = _lib.SIGNATURES[name]
    assert res is C_TYPES[restype] and args == want and len(args) == n_args
    assert hasattr(_lib.load(), name)


def test_wrappers_have_no_cpu_fallback():
    from fewshot_vit_amd.engine import ops
    tok, xhat, pooled = torch.zeros(4, 5, 64), torch.zeros(4, 5, 64), torch.zeros(4, 64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.emd_table_prep(tok, xhat, pooled)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.emd_head_gather(tok, xhat, pooled, torch.zeros(1, 2, dtype=torch.int32), 12.5, torch.zeros(1, dtype=torch.int32),
                            proto_slots=torch.zeros(1, 2, dtype=torch.int32))


def _fake_table(n_images=20, N=3, dim=4, chunk=4):
    """encode_fn: node n of image i is the constant i + n / 10; the stubbed prep writes xhat = -tok, pooled = the token mean"""
    from fewshot_vit_amd.feature_table import TokenTable
    calls, preps = [], []

    def encode_fn(index):
        calls.append(index.clone())
        return (index[:, None, None].float() + torch.arange(N)[None, :, None] / 10) * torch.ones(dim)

    def prep_fn(tok, xhat, pooled):
        preps.append(tok.shape[0])
        xhat.copy_(-tok)
        pooled.copy_(tok.mean(dim=1))

    return TokenTable(encode_fn, n_images, 'cpu', chunk_images=chunk, prep_fn=prep_fn), calls, preps


def test_ensure_encodes_and_prepares_every_image_once():
    table, calls, preps = _fake_table()
    assert table.tok is None and table.n_encoded == 0
    requests = [torch.tensor([[7, 3, 7], [15, 3, 0]]),              # repeats inside one request, out of order, 2-d
                torch.tensor([19, 18, 7, 2, 11, 12, 13, 3, 1, 0]),  # overlaps the first; 7 new images: two chunks
                torch.tensor([15, 4, 4, 19])]                       # one new image
    for r in requests:
        slots = table.ensure(r)
        assert slots.shape == r.shape and slots.dtype == torch.int32
        assert int(slots.min()) >= 0 and int(slots.max()) < table.n_encoded
        rows = table.tok[slots.reshape(-1).long()]
        assert torch.equal(rows[:, 0, 0], r.reshape(-1).float()) and torch.equal(rows[:, 2, 3], r.reshape(-1).float() + 0.2)      # the right rows
        assert torch.equal(table.xhat[slots.reshape(-1).long()], -rows) and torch.equal(table.pooled[slots.reshape(-1).long()], rows.mean(dim=1))
    assert table.tok.shape == (20, 3, 4) and table.xhat.shape == (20, 3, 4) and table.pooled.shape == (20, 4)
    unique = sorted(set(torch.cat([r.reshape(-1) for r in requests]).tolist()))
    encoded = torch.cat(calls).tolist()
    assert sorted(encoded) == unique and len(encoded) == len(unique)                    # exactly once each
    assert [c.tolist() for c in calls] == [[0, 3, 7, 15], [1, 2, 11, 12], [13, 18, 19], [4]]      # ascending, at most four per call
    assert all(c.dtype == torch.int64 for c in calls) and preps == [4, 4, 3, 1]         # one prep per appended chunk
    assert table.n_encoded == len(unique) == 12 and table.n_requests == 6 + 10 + 4
    assert sorted(table.slot_of[table.slot_of >= 0].tolist()) == list(range(12))        # slots are dense, in encode order
    assert table.slot_of[0] == 0 and table.slot_of[15] == 3 and table.slot_of[4] == 11
    table.ensure(torch.tensor(unique))                                                  # nothing new: no call
    assert len(calls) == 4 and len(preps) == 4 and table.n_encoded == 12
    table.reset()
    assert table.n_encoded == 0 and table.n_requests == 0 and bool((table.slot_of == -1).all())
    assert table.ensure(torch.tensor([5, 5])).tolist() == [0, 0] and calls[-1].tolist() == [5] and table.n_encoded == 1
    assert torch.equal(table.tok[0, :, 0], 5 + torch.arange(3) / 10)


def test_ensure_refusals():
    from fewshot_vit_amd.feature_table import FeatureTable, TokenTable
    table, calls, _ = _fake_table()
    for bad in ([-1], [20], [3, 25]):
        with pytest.raises(IndexError):
            table.ensure(torch.tensor(bad))
    assert not calls and table.n_encoded == 0
    assert table.ensure(torch.zeros(0, dtype=torch.int64)).shape == (0,)
    with pytest.raises(ValueError, match='encode_fn returned'):
        TokenTable(lambda index: torch.zeros(len(index), 5), 8, 'cpu', prep_fn=lambda *a: None).ensure(torch.tensor([1, 2]))
    table.ensure(torch.tensor([1]))
    table.encode_fn = lambda index: torch.zeros(len(index), 4, 4)                       # another node count than the table holds
    with pytest.raises(ValueError, match='encode_fn returned'):
        table.ensure(torch.tensor([2]))
    with pytest.raises(ValueError):
        TokenTable(lambda index: None, 0, 'cpu')
    with pytest.raises(ValueError, match='whole number'):
        table.logits(torch.arange(7), 2, 1, 2, None)
    assert issubclass(TokenTable, FeatureTable.__mro__[1]) and FeatureTable.ensure is TokenTable.ensure      # one copy of the bookkeeping


def test_for_dataset_refusals():
    from fewshot_vit_amd import datasets, models
    from fewshot_vit_amd.feature_table import TokenTable
    small = dict(split='test', n_classes=2, n_per_class=2, device='cpu')
    make = lambda mode: models.make('deepemd', encoder='visformer_micro_80', encoder_args={}, deepemd=mode).cpu()
    fcn, grid, sampling = make('fcn'), make('grid'), make('sampling')
    with pytest.raises(ValueError, match='train mode'):
        TokenTable.for_dataset(fcn.train(), datasets.make('synthetic-images', **small))
    with pytest.raises(ValueError, match='no single node set per image'):
        TokenTable.for_dataset(sampling.eval(), datasets.make('synthetic-images', patches='sampling', **small))
    with pytest.raises(ValueError, match='no single node set per image'):
        TokenTable.for_dataset(grid.eval(), datasets.make('synthetic-images', patches='grid', patch_train=True, **small))
    with pytest.raises(ValueError, match='no single node set per image'):
        TokenTable.for_dataset(fcn.eval(), datasets.make('synthetic-images', augment='resize', **small))
    # a loader the model's mode does not read
    with pytest.raises(ValueError, match='no single node set per image'):
        TokenTable.for_dataset(fcn.eval(), datasets.make('synthetic-images', patches='grid', **small))
    with pytest.raises(ValueError, match='no single node set per image'):
        TokenTable.for_dataset(grid.eval(), datasets.make('synthetic-images', **small))


def test_drivers_refuse_the_sampling_loader_before_any_gpu_call(monkeypatch):
    from fewshot_vit_amd import eval_deepemd, train_deepemd
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: pytest.fail('a GPU call'))
    with pytest.raises(ValueError, match='sampling'):
        eval_deepemd.main(['-feature_cache', '-deepemd', 'sampling', '-dataset', 'synthetic-images'])
    with pytest.raises(ValueError, match='sampling'):
        train_deepemd.main(['-eval_feature_cache', '-deepemd', 'sampling'])


def test_flags_default_to_off_and_the_evaluate_surfaces_stay():
    from fewshot_vit_amd import eval_deepemd, train_deepemd
    assert eval_deepemd.parse_args([]).feature_cache is False and eval_deepemd.parse_args(['-feature_cache']).feature_cache is True
    assert train_deepemd.parse_args([]).eval_feature_cache is False and train_deepemd.parse_args(['-eval_feature_cache']).eval_feature_cache is True
    ev = inspect.signature(eval_deepemd.evaluate).parameters
    assert list(ev) == ['args', 'log', 'collect'] and ev['log'].default is print and ev['collect'].default is None
    tr = inspect.signature(train_deepemd.evaluate).parameters
    assert list(tr) == ['model', 'dataset', 'args', 'n_episode', 'device', 'seed', 'table'] and tr['seed'].default is None and tr['table'].default is None
