"""Host-side checks of the prototype bank's top-k surface (no GPU): the ctypes signatures mirror fsvit.h, `--topk` is a documented flag, there is no CPU
path, k is checked before anything else, the stable-sort reference of tests/proto_bank_topk_cases.py is a stable sort, and the fp32 restatement of the
kernel's log-sum-exp chain stays inside the allowance the GPU test gates with."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import proto_bank_cases as pc
import proto_bank_topk_cases as tc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_decl(header, name):
    """(result, parameter list) of `name` in fsvit.h as ctypes types: pointers -> c_void_p, int / float / size_t by value"""
    types = {'int': C.c_int, 'float': C.c_float, 'size_t': C.c_size_t}
    m = re.search(r'\b(int|size_t)\s+' + name + r'\s*\(([^;]*?)\)\s*;', header, re.S)
    assert m, name
    out = []
    for p in m.group(2).split(','):
        p = re.sub(r'/\*.*?\*/', '', p, flags=re.S).strip()
        out.append(C.c_void_p if '*' in p else types[p.split()[-2]])
    return types[m.group(1)], out


def test_signatures_match_the_header():
    from fewshot_vit_amd import _lib
    header = open(os.path.join(REPO, 'include', 'fsvit.h')).read()
    for name in ('fsvit_proto_bank_topk_workspace_bytes', 'fsvit_proto_bank_topk'):
        assert _lib.SIGNATURES[name] == _c_decl(header, name), name
        assert hasattr(_lib.load(), name)
    assert _lib.SIGNATURES['fsvit_proto_bank_topk_workspace_bytes'] == (C.c_size_t, [C.c_int] * 4)
    assert len(_lib.SIGNATURES['fsvit_proto_bank_topk'][1]) == 17


def test_workspace_bytes_on_the_host():
    """the size entry touches no device: explicit n_split, and 0 bytes for what the call would refuse"""
    from fewshot_vit_amd import _lib
    lib = _lib.load()
    f = lib.fsvit_proto_bank_topk_workspace_bytes
    assert f(70, 4100, 32, 5) == (5 * 70 * 32 * 2 + 70 * 5 * 2) * 4
    assert f(1, 1, 1, 1) == (2 + 2) * 4
    assert f(0, 5, 5, 1) == 0
    for bad in ((4, 5, 0, 1), (4, 5, 33, 1), (4, 5, 5, 2), (4, 5, 5, -1), (4, 0, 5, 1), (4, 65537, 5, 1), (-1, 5, 5, 1), (4, 2100, 5, 4)):
        assert f(*bad) == 0, bad


def test_cli_help_lists_topk(capsys):
    from fewshot_vit_amd import predict
    with pytest.raises(SystemExit) as e:
        predict.main(['--help'])
    assert e.value.code == 0
    assert '--topk' in capsys.readouterr().out
    for k in ('0', '33'):
        with pytest.raises(SystemExit):
            predict.main(['--load', 'x.pth', '--support', 'x', '--topk', k])


def test_no_cpu_fallback_and_k_range():
    from fewshot_vit_amd import models
    from fewshot_vit_amd.engine import ops
    from fewshot_vit_amd.models.proto_bank import PrototypeBank
    f, p, e = torch.zeros(4, 64), torch.zeros(3, 64), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.proto_bank_topk(f, p, e, 1.0, 'cos', 2)
    m = models.make('meta-baseline', encoder='visformer_micro_80', encoder_args={}).eval()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.predict_topk(None, torch.zeros(2, 3, 80, 80), 2)
    with pytest.raises(RuntimeError, match='eval-mode'):
        m.train().predict_topk(None, torch.zeros(2, 3, 80, 80), 2)
    m.eval()
    bank = object.__new__(PrototypeBank)                     # a bank cannot be made on the host: topk must refuse before it looks at its state
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        bank.topk(f, 2)
    for k in (0, 33, -1, 2.0, True, None):                   # the argument alone decides: before any device check
        with pytest.raises(ValueError):
            ops.proto_bank_topk(f, p, e, 1.0, 'cos', k)
        with pytest.raises(ValueError):
            bank.topk(f, k)
        with pytest.raises(ValueError):
            m.predict_topk(None, torch.zeros(2, 3, 80, 80), k)
    with pytest.raises(ValueError):
        ops.proto_bank_topk(f, p, e, 1.0, 'cos', 2, n_split=-1)


def test_reference_is_a_stable_descending_sort():
    inf = float('inf')
    rows = torch.tensor([[1.0, 3.0, 3.0, -inf, 2.0, 3.0, -inf, 1.0],
                         [-inf, -inf, -inf, -inf, -inf, -inf, -inf, -inf],
                         [0.0, -0.0, 5.0, 5.0, -1.0, 0.0, 7.0, 7.0]])
    for k in (1, 3, 8, 11):
        v, i = tc.topk_reference(rows, k)
        for r in range(rows.shape[0]):
            order = sorted(range(rows.shape[1]), key=lambda c: (-rows[r, c].item(), c))      # Python's sort: larger value first, then the lower index
            want_i = (order + [-1] * k)[:k]
            want_v = [rows[r, c].item() if c >= 0 else -inf for c in want_i]
            assert i[r].tolist() == want_i and v[r].tolist() == want_v, (k, r)
        assert v.dtype == torch.float32 and i.dtype == torch.int32
    assert tc.topk_reference(rows, 3)[1][0].tolist() == [1, 2, 5]
    assert tc.topk_reference(rows, 8)[1][0].tolist() == [1, 2, 5, 4, 0, 7, 3, 6], 'empty classes follow every finite entry, in index order'
    assert tc.splits(4100) == (0, 1, 2, 5) and tc.splits(2100) == (0, 1, 2, 3) and tc.splits(130) == (0, 1)


def _rows(way):
    g = pc._gen('lse-emulation', way)
    n = torch.randn(way, generator=g)
    asc = torch.sort(n).values
    wide = (torch.rand(way, generator=g) * 160.0 - 80.0)
    holes = n.clone()
    holes[::3] = -float('inf')
    return {'normal': n * 4.0, 'ascending': asc * 4.0, 'descending': asc.flip(0) * 4.0, 'wide': wide, 'holes': holes}


@pytest.mark.parametrize('way', tc.LSE_WAYS)
def test_lse_chain_in_fp32_stays_inside_the_allowance(way):
    worst = {}
    for name, row in _rows(way).items():
        L = tc.lse_reference(row[None])
        got = tc.emulate_lse(row.numpy())
        worst[name] = tc.lse_ratio(torch.tensor([float(got)]), L, way)
    print(f'lse emulation way {way}: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    # what the gate can see: one dropped class of a near-uniform row moves L by many allowances
    if way > 1:
        row = torch.zeros(way)
        full, less = tc.lse_reference(row[None]), tc.lse_reference(row[None, 1:])
        assert float((full - less).abs() / (tc.lse_allowance(way, full) + tc.U * full.abs())) > 10.0
    none = np.full(way, -np.inf, dtype=np.float32)
    assert tc.emulate_lse(none) == -np.inf
