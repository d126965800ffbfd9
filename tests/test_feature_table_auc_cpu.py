"""Host-side checks of FeatureTable.auc (no GPU): the gather reduction is declared in fsvit.h and bound with the same argument list, the table hands it
the slots of class 0's shots and of all queries in the reference's order, and only those images go through the encoder."""
import ctypes as C
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gather_auc_is_declared_and_bound():
    from fewshot_vit_amd import _lib
    from fewshot_vit_amd.engine import ops
    header = open(os.path.join(REPO, 'include', 'fsvit.h')).read()
    m = re.search(r'\bint\s+fsvit_proto_auc_gather\s*\(([^;]*?)\)\s*;', header, re.S)
    assert m
    want = []
    for p in m.group(1).split(','):
        p = re.sub(r'/\*.*?\*/', '', p, flags=re.S).strip()
        want.append(C.c_void_p if '*' in p else {'int': C.c_int, 'float': C.c_float}[p.split()[-2]])
    res, args = _lib.SIGNATURES['fsvit_proto_auc_gather']
    assert res is C.c_int and args == want and len(args) == 13
    assert hasattr(_lib.load(), 'fsvit_proto_auc_gather')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.proto_auc_gather(torch.zeros(4, 8), torch.zeros(1, 1, dtype=torch.int64), torch.zeros(1, 2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))


def _fake_table(monkeypatch, n_images=40, dim=3, chunk=4):
    from fewshot_vit_amd import engine
    from fewshot_vit_amd.feature_table import FeatureTable
    calls, launches = [], []

    def encode_fn(index):
        calls.append(index.clone())
        return index[:, None].float() * torch.ones(dim)

    def proto_auc_gather(table, shot_slots, query_slots, invalid, want_score=False):
        launches.append((table.clone(), shot_slots.clone(), query_slots.clone(), invalid))
        return torch.zeros(shot_slots.shape[0])

    monkeypatch.setattr(engine.ops, 'proto_auc_gather', staticmethod(proto_auc_gather))
    return FeatureTable(encode_fn, n_images, dim, 'cpu', chunk_images=chunk), calls, launches


def test_auc_passes_the_reference_order_and_skips_the_shots_of_class_1(monkeypatch):
    table, calls, launches = _fake_table(monkeypatch)
    shot, n_query = 2, 3
    # two batches of two 2-way episodes, class-major, the first `shot` of a class its shots; images 30..37 are shots of class 1 only
    ep = lambda c0, c1: c0 + c1
    idx = torch.tensor([ep([5, 1, 9, 8, 5], [30, 31, 2, 9, 0]) + ep([1, 3, 4, 4, 6], [32, 33, 7, 5, 11]),
                        ep([9, 5, 12, 13, 1], [34, 35, 14, 2, 3]) + ep([0, 2, 15, 16, 17], [36, 37, 18, 19, 5])])
    out = table.auc(idx, shot, n_query)
    assert out.shape == (4,) and len(launches) == 1
    feat, shot_slots, query_slots, invalid = launches[0]
    assert invalid is table.invalid and feat.shape == (table.n_encoded, 3)
    assert shot_slots.shape == (4, shot) and query_slots.shape == (4, 2 * n_query) and shot_slots.dtype == query_slots.dtype == torch.int32
    image_of = lambda slots: feat[slots.long(), 0].long().tolist()          # the stub's feature of image i is i
    assert image_of(shot_slots) == [[5, 1], [1, 3], [9, 5], [0, 2]]         # the shots of class 0
    assert image_of(query_slots) == [[9, 8, 5, 2, 9, 0], [4, 4, 6, 7, 5, 11], [12, 13, 1, 14, 2, 3], [15, 16, 17, 18, 19, 5]]      # positives first
    used = sorted(set(range(20)) - {10})
    encoded = torch.cat(calls).tolist()
    assert encoded == used                                                  # once each, ascending; none of 30..37
    assert all(1 <= len(c) <= 4 for c in calls)
    assert table.n_encoded == len(used) == 19 and table.n_requests == 4 * (shot + 2 * n_query)
    assert bool((table.slot_of[30:38] == -1).all())
    n_calls = len(calls)
    table.auc(idx[:1], shot, n_query)                                       # nothing new: no encoder call, one more launch
    assert len(calls) == n_calls and len(launches) == 2 and table.n_requests == 6 * (shot + 2 * n_query)


def test_auc_refuses_a_ragged_index(monkeypatch):
    table, calls, launches = _fake_table(monkeypatch)
    with pytest.raises(ValueError, match='whole number'):
        table.auc(torch.arange(2 * (1 + 15) + 1), 1, 15)
    with pytest.raises(ValueError, match='whole number'):
        table.auc(torch.arange(32), 2, 15)
    assert not calls and not launches and table.n_encoded == 0 and table.n_requests == 0


def test_drivers_list_the_switch(capsys):
    import inspect
    from fewshot_vit_amd import eval_sauc
    with pytest.raises(SystemExit) as e:
        eval_sauc.main(['--help'])
    assert e.value.code == 0 and '--feature-cache' in capsys.readouterr().out
    assert inspect.signature(eval_sauc.evaluate).parameters['feature_cache'].default is False      # off unless asked for
