"""Host-side checks of the prototype bank surface (no GPU): no CPU path anywhere, the CLIs list their new flags, the ctypes signatures mirror fsvit.h,
and the seeds of the --sauc cases of tests/test_gpu_sauc.py keep every untied score pair further apart than the fp32 allowance."""
import ctypes as C
import os
import re

import pytest
import torch

import proto_bank_cases as pc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_cpu_fallback():
    from fewshot_vit_amd import models
    from fewshot_vit_amd.engine import ops
    from fewshot_vit_amd.models.proto_bank import PrototypeBank
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        PrototypeBank(3, 64, 'cos', device='cpu')
    with pytest.raises(ValueError):
        PrototypeBank(3, 64, 'l2', device='cpu')
    f, y = torch.zeros(4, 64), torch.zeros(4, dtype=torch.int64)
    s, c, inv = torch.zeros(3, 64), torch.zeros(3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    for call in (lambda: ops.proto_bank_accumulate(f, y, s, c, inv), lambda: ops.proto_bank_finalize(s, c), lambda: ops.proto_bank_logits(f, s, c, 1.0),
                 lambda: ops.proto_auc(f.view(1, 4, 64), f.view(1, 4, 64))):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    m = models.make('meta-baseline', encoder='visformer_micro_80', encoder_args={}).eval()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.fit(torch.zeros(2, 3, 80, 80), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.predict(None, torch.zeros(2, 3, 80, 80))
    with pytest.raises(RuntimeError, match='eval-mode'):
        m.train().fit(torch.zeros(2, 3, 80, 80), torch.zeros(2, dtype=torch.int64))


def test_cli_help_lists_the_new_flags(capsys):
    from fewshot_vit_amd import eval_sauc, predict
    with pytest.raises(SystemExit) as e:
        predict.main(['--help'])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for flag in ('--load', '--support', '--query', '--method', '--numerics', '--out', '--save-bank', '--load-bank'):
        assert flag in text, flag
    with pytest.raises(SystemExit) as e:
        eval_sauc.main(['--help'])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for flag in ('--sauc', '--config', '--shot', '--test-epochs', '--gpu'):      # the reference driver's flags (test_few_shot.py:120-127)
        assert flag in text, flag
    with pytest.raises(SystemExit):                          # neither a support folder nor a stored bank
        predict.main(['--load', 'x.pth'])


def _c_args(header, name):
    """the parameter list of `name` in fsvit.h as ctypes types: pointers -> c_void_p, int / float / size_t by value"""
    m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', header, re.S)
    assert m, name
    out = []
    for p in m.group(1).split(','):
        p = re.sub(r'/\*.*?\*/', '', p, flags=re.S).strip()
        out.append(C.c_void_p if '*' in p else {'int': C.c_int, 'float': C.c_float, 'size_t': C.c_size_t}[p.split()[-2]])
    return out


def test_signatures_match_the_header():
    from fewshot_vit_amd import _lib
    header = open(os.path.join(REPO, 'include', 'fsvit.h')).read()
    for name in ('fsvit_proto_bank_accumulate', 'fsvit_proto_bank_finalize', 'fsvit_proto_bank_logits', 'fsvit_proto_auc'):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == _c_args(header, name), name
        assert hasattr(_lib.load(), name)
    assert len(_lib.SIGNATURES['fsvit_proto_bank_logits'][1]) == 12


@pytest.mark.parametrize('case', sorted(pc.SAUC_CASES))
def test_sauc_seeds_keep_untied_pairs_apart(case):
    E, shot, Q, D = case
    fs, fq, n_dup = pc.sauc_inputs(E, shot, Q, D, pc.SAUC_CASES[case])
    s, auc, ok = pc.sauc_reference(fs, fq, n_dup)
    assert ok
    assert bool(((auc >= 0) & (auc <= 1)).all())
    k = Q // 2
    pairs = (s[:, :k, None] > s[:, None, k:]).double() + 0.5 * (s[:, :k, None] == s[:, None, k:]).double()      # the identity the kernel counts by
    assert float((pairs.sum((1, 2)) / (k * k) - auc).abs().max()) < 1e-15


def test_references_agree_with_the_head_oracle():
    """a rectangular support set through bank_reference + logits_reference is the episode head's float64 result"""
    from oracle import head_ops_oracle as ho
    g = pc._gen('agree')
    fs, fq = torch.randn(1, 4, 3, 64, generator=g), torch.randn(1, 8, 64, generator=g)
    y = torch.arange(4).repeat_interleave(3)
    for method in pc.METHODS:
        b = pc.bank_reference(fs.view(12, 64), y, 4, method)
        A, a = pc.logits_reference(fq[0], b['proto'], b['a_proto'], b['empty'], 2.5, method)
        r = ho.head_forward(fs.double(), fq.double(), 2.5, method)
        assert float((A - r['logits'][0]).abs().max()) < 1e-12 and bool((a > 0).all())
