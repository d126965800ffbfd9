"""Sizing pass of the two trainer handles, without a device: `fsvit_*_trainer_workspace_bytes` walks forward + backward with dry arenas, launches
nothing and reads only the names of the parameter table, so it runs on a CPU-only box.

The byte counts below are constants taken from a run of the library built at commit afb0c5c ("Delete retired-switch dead code; share the
encoder-handle plumbing"), the parent of the change that gave both trainers one `TrainerBase` and one step driver.  They pin that the shared driver
sizes exactly what the two copied drivers sized; they are not to be regenerated from the code under test."""
import ctypes as C

import pytest

from fewshot_vit_amd import _lib

FAKE = 4096          # the sizing pass never dereferences a parameter


def _model(kind, drop_path_rate=0.0):
    if kind == 'visformer':      # the `tiny_visformer` geometry of test_boundary_cpu.py
        from fewshot_vit_amd.models.visformer import Visformer
        return Visformer(img_size=80, init_channels=8, embed_dim=64, depth=[1, 1, 1], num_heads=6, mlp_ratio=4., group=8, drop_path_rate=drop_path_rate)
    from fewshot_vit_amd.models import deit
    return deit.deit_nano_patch6_84(drop_path_rate=drop_path_rate)


def _trainer(kind, numerics):
    from fewshot_vit_amd import engine
    cls = engine.VisformerTrainer if kind == 'visformer' else engine.VitTrainer
    return cls(_model(kind).cfg, numerics=numerics)


def _table(kind, drop=()):
    names = [k.encode() for k in _model(kind).state_dict() if not k.endswith('num_batches_tracked') and k not in drop]
    arr = (_lib.Param * len(names))()
    for i, k in enumerate(names):
        arr[i].name, arr[i].data, arr[i].grad, arr[i].numel = k, FAKE, None, 1
    return arr, names


def _workspace_bytes(kind, numerics, n_img, rate, drop=()):
    tr = _trainer(kind, numerics)
    arr, names = _table(kind, drop)
    fn = tr.lib.fsvit_visformer_trainer_workspace_bytes if kind == 'visformer' else tr.lib.fsvit_vit_trainer_workspace_bytes
    return fn(tr.h, arr, len(names), n_img, C.c_float(rate))


# (model, numerics, n_img, drop_path_rate) -> save + tmp bytes, from the library of commit afb0c5c
WORKSPACE_BYTES = {
    ('visformer', 'bf16', 2, 0.0): 10193408,
    ('visformer', 'bf16', 2, 0.5): 10193664,
    ('visformer', 'bf16', 7, 0.0): 29595392,
    ('visformer', 'bf16', 7, 0.5): 29595648,
    ('visformer', 'bf16x2', 2, 0.0): 16060928,
    ('visformer', 'bf16x2', 2, 0.5): 16061184,
    ('visformer', 'bf16x2', 7, 0.0): 47232512,
    ('visformer', 'bf16x2', 7, 0.5): 47232768,
    ('visformer', 'parity', 2, 0.0): 14950912,
    ('visformer', 'parity', 2, 0.5): 14951168,
    ('visformer', 'parity', 7, 0.0): 42121728,
    ('visformer', 'parity', 7, 0.5): 42121984,
    ('deit', 'bf16', 2, 0.0): 282803712,
    ('deit', 'bf16', 2, 0.5): 282803968,
    ('deit', 'bf16', 7, 0.0): 620574976,
    ('deit', 'bf16', 7, 0.5): 620575744,
    ('deit', 'bf16x2', 2, 0.0): 348389376,
    ('deit', 'bf16x2', 2, 0.5): 348389632,
    ('deit', 'bf16x2', 7, 0.0): 779714048,
    ('deit', 'bf16x2', 7, 0.5): 779714816,
    ('deit', 'parity', 2, 0.0): 167767040,
    ('deit', 'parity', 2, 0.5): 167767296,
    ('deit', 'parity', 7, 0.0): 389259776,
    ('deit', 'parity', 7, 0.5): 389260544,
}


@pytest.mark.parametrize('case', sorted(WORKSPACE_BYTES), ids=lambda c: '-'.join(str(v) for v in c))
def test_trainer_workspace_bytes_are_the_recorded_ones(case):
    got = _workspace_bytes(*case)
    print('workspace_bytes%r = %d (recorded %d)' % (case, got, WORKSPACE_BYTES[case]))
    assert got == WORKSPACE_BYTES[case]


def test_workspace_table_covers_the_grid():
    assert set(WORKSPACE_BYTES) == {(k, n, b, r) for k in ('visformer', 'deit') for n in ('bf16', 'bf16x2', 'parity') for b in (2, 7) for r in (0.0, 0.5)}


@pytest.mark.parametrize('kind,missing', [('visformer', 'stage2.0.norm2.bn.running_var'), ('visformer', 'patch_embed3.proj.weight'),
                                          ('deit', 'blocks.3.attn.proj.bias'), ('deit', 'norm.weight')])
def test_workspace_bytes_names_a_missing_parameter(kind, missing):
    """A table that lacks one parameter sizes to 0 and leaves the message engine.py looks for ('missing') with the parameter's name."""
    assert _workspace_bytes(kind, 'bf16', 2, 0.0, drop=(missing,)) == 0
    assert _lib.load().fsvit_last_error().decode() == 'missing parameter: ' + missing


@pytest.mark.parametrize('kind', ['visformer', 'deit'])
def test_workspace_bytes_of_nothing_is_zero(kind):
    tr = _trainer(kind, 'bf16')
    arr, names = _table(kind)
    fn = tr.lib.fsvit_visformer_trainer_workspace_bytes if kind == 'visformer' else tr.lib.fsvit_vit_trainer_workspace_bytes
    assert fn(tr.h, arr, len(names), 0, 0.0) == 0
    assert fn(tr.h, None, 0, 2, 0.0) == 0
    assert fn(None, arr, len(names), 2, 0.0) == 0
