"""LV-ViT training, the parts that need no GPU: the reference golden of one train-mode step (tests/golden/lvvit_train_step.npz) means what the GPU
test assumes - a plain-torch fp32 restatement of the step, replaying the recorded DropPath masks, reproduces it -, the C ABI's new names agree
between the header, the ctypes table and the library, and the DropPath keep list is get_dpr's."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
NEW_ABI = ['fsvit_lvvit_trainer_create', 'fsvit_lvvit_trainer_destroy', 'fsvit_lvvit_trainer_droppath_calls', 'fsvit_lvvit_trainer_workspace_bytes',
           'fsvit_lvvit_trainer_set_freeze_bn', 'fsvit_lvvit_train_forward', 'fsvit_lvvit_train_backward']


@pytest.fixture(scope='module')
def golden():
    sys.path.insert(0, GOLDEN)
    import make_lvvit_train_golden as mk
    z = np.load(os.path.join(GOLDEN, 'lvvit_train_step.npz'))
    return {k: z[k] for k in z.files}, mk


def test_golden_has_the_reference_state_dict_table(golden):
    z, _ = golden
    ref = np.load(os.path.join(GOLDEN, 'lvvit.npz'))
    assert len(z['keys']) == 118 and list(z['keys']) == list(ref['keys'])
    assert z['x'].shape == (4, 3, 80, 80) and z['masks'].shape == (14, 4) and z['bn.feat'].shape == (4, 384)
    assert os.path.getsize(os.path.join(GOLDEN, 'lvvit_train_step.npz')) < 1 << 20
    for rec in ('bn', 'frozen'):
        assert sum(k.startswith(rec + '.gnorm.') for k in z) == 106 and sum(k.startswith(rec + '.buf.') for k in z) == 12
    # frozen BatchNorm leaves its buffers alone; batch statistics move them and count the step
    assert int(z['bn.buf.patch_embed.bn1.num_batches_tracked']) == int(z['frozen.buf.patch_embed.bn1.num_batches_tracked']) + 1
    assert np.abs(z['bn.buf.patch_embed.bn2.running_mean'] - z['frozen.buf.patch_embed.bn2.running_mean']).max() > 1e-4


def _forward(p, bufs, x, masks, frozen, depth=8, heads=6, skip_lam=2.0, rate=0.5):
    """lvvit.py:277-317 (stem), :134-155 (blocks), :529-546, restated on a dict of tensors; `bufs` is updated as nn.BatchNorm2d would."""
    def bn(t, name):
        return F.batch_norm(t, bufs[name + '.running_mean'], bufs[name + '.running_var'], p[name + '.weight'], p[name + '.bias'],
                            training=not frozen, momentum=0.1, eps=1e-5)
    pe = 'patch_embed.'
    y = F.leaky_relu(bn(F.conv2d(x, p[pe + 'conv1.weight'], stride=2, padding=1), pe + 'bn1'), 0.1)
    y = F.leaky_relu(bn(F.conv2d(y, p[pe + 'conv2.weight'], padding=1), pe + 'bn2'), 0.1)
    y = bn(F.conv2d(y, p[pe + 'conv3.weight'], padding=1), pe + 'bn3')
    y = y + bn(F.conv2d(x, p[pe + 'downsample.0.weight'], stride=2, padding=1), pe + 'downsample.1')
    y = F.max_pool2d(F.leaky_relu(y, 0.1), 2)
    y = F.conv2d(y, p[pe + 'proj.weight'], p[pe + 'proj.bias'], stride=4)
    B, D = y.shape[0], y.shape[1]
    t = torch.cat([p['cls_token'].expand(B, -1, -1), y.flatten(2).transpose(1, 2)], dim=1) + p['pos_embed']
    dpr = torch.linspace(0, rate, depth).tolist()
    call = 0

    def drop(v, r):
        nonlocal call
        if r == 0.0:
            return v
        mk = masks[call].view(B, 1, 1)
        call += 1
        return v.div(1 - r) * mk
    hd = D // heads
    for i in range(depth):
        b = f'blocks.{i}.'
        h = F.layer_norm(t, (D,), p[b + 'norm1.weight'], p[b + 'norm1.bias'], 1e-5)
        qkv = F.linear(h, p[b + 'attn.qkv.weight']).reshape(B, -1, 3, heads, hd).permute(2, 0, 3, 1, 4)
        a = ((qkv[0] * hd ** -0.5) @ qkv[1].transpose(-2, -1)).softmax(dim=-1)
        h = F.linear((a @ qkv[2]).transpose(1, 2).reshape(B, -1, heads * hd), p[b + 'attn.proj.weight'], p[b + 'attn.proj.bias'])
        t = t + drop(h, dpr[i]) / skip_lam
        h = F.layer_norm(t, (D,), p[b + 'norm2.weight'], p[b + 'norm2.bias'], 1e-5)
        h = F.linear(F.gelu(F.linear(h, p[b + 'mlp.fc1.weight'], p[b + 'mlp.fc1.bias'])), p[b + 'mlp.fc2.weight'], p[b + 'mlp.fc2.bias'])
        t = t + drop(h, dpr[i]) / skip_lam
    assert call == masks.shape[0]
    return F.layer_norm(t, (D,), p['norm.weight'], p['norm.bias'], 1e-5)[:, 0]


@pytest.mark.parametrize('rec', ['bn', 'frozen'])
def test_plain_torch_restatement_reproduces_the_golden(golden, rec):
    z, mk = golden
    from fewshot_vit_amd import models
    m = models.make('lvvit_micro_80')
    sd, _ = mk.perturbed_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    names = {k for k, _ in m.named_parameters()}
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k in names}
    bufs = {k: v.clone() for k, v in sd.items() if k not in names}
    feat = _forward(p, bufs, torch.from_numpy(z['x']), torch.from_numpy(z['masks']), rec == 'frozen')
    (feat * torch.from_numpy(z['w'])).sum().backward()
    assert np.abs(feat.detach().numpy() - z[rec + '.feat']).max() <= 1e-5
    for k, ref in z.items():
        if k.startswith(rec + '.buf.') and not k.endswith('num_batches_tracked'):
            assert np.abs(bufs[k[len(rec) + 5:]].numpy() - ref).max() <= 1e-6, k
        elif k.startswith(rec + '.gnorm.'):
            name = k[len(rec) + 7:]
            assert abs(float(p[name].grad.double().norm()) - float(ref)) <= 1e-5 * max(1.0, float(ref)), k
        elif k.startswith(rec + '.grad.'):
            name = k[len(rec) + 6:]
            g = p[name].grad.contiguous()
            stride = mk.STRIDE if name.startswith('patch_embed.conv') else mk.STRIDE_BLOCKS
            got = (g if g.numel() <= mk.FULL_MAX else g.view(-1)[::stride]).numpy()
            assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), k


def test_header_signatures_and_exports_agree():
    from fewshot_vit_amd import _lib
    header = open(os.path.join(HERE, '..', 'include', 'fsvit.h')).read()
    lib = _lib.load()
    for name in NEW_ABI:
        assert re.search(r'\b%s\(' % name, header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    # the trainer entries take what the Visformer / ViT ones take
    assert _lib.SIGNATURES['fsvit_lvvit_train_forward'][1] == _lib.SIGNATURES['fsvit_vit_train_forward'][1]
    assert _lib.SIGNATURES['fsvit_lvvit_train_backward'][1] == _lib.SIGNATURES['fsvit_vit_train_backward'][1]
    assert _lib.SIGNATURES['fsvit_lvvit_trainer_set_freeze_bn'][1] == _lib.SIGNATURES['fsvit_visformer_trainer_set_freeze_bn'][1]


def test_droppath_keep_list_is_get_dpr():
    """get_dpr(0.5, 8, 'linear') (lvvit.py:401-404) = linspace(0, 0.5, 8): block 0 has no DropPath, the other seven call it twice."""
    from fewshot_vit_amd.engine import LvvitTrainer
    t = LvvitTrainer.__new__(LvvitTrainer)
    t.cfg = dict(depth=8)
    keep = t.droppath_keep(0.5)
    dpr = [x.item() for x in torch.linspace(0, 0.5, 8)]
    assert keep == [1.0 - r for r in dpr[1:] for _ in range(2)] and len(keep) == 14
    assert t.droppath_keep(0.0) == []
    from fewshot_vit_amd import models
    assert models.make('lvvit_micro_80').drop_path_rate == 0.5 and models.make('lvvit_micro_80', drop_path_rate=0.1).drop_path_rate == 0.1
