"""CPU checks of the LV-ViT encoder `lvvit_micro_80` (meta_tuning_sun_m/models/lvvit.py:583): registry and state-dict contract against the
reference's key table (tests/golden/lvvit.npz, make_lvvit_golden.py), checkpoint round trips through `models.load` in the reference's
schemas, a plain-torch fp32 restatement of the eval forward that reproduces the reference's features, and the refusals (no CPU fallback,
no training)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lvvit.npz')


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def golden_shapes(g):
    return {k: tuple(int(d) for d in s.split(',') if d) for k, s in zip(g['keys'].tolist(), g['shapes'].tolist())}


def procedural_sd(shapes):
    from fewshot_vit_amd import synthetic
    return synthetic.procedural_state_dict(shapes)


def lvvit_forward(sd, x, taps=None, depth=8, heads=6, skip_lam=2.0, eps=1e-5):
    """fp32 restatement of LV_ViT.forward in eval mode (lvvit.py:277-318 ConvBlock, :140-155 Block, :529-546): `sd` encoder-relative."""
    def bn(t, p):
        return F.batch_norm(t, sd[p + '.running_mean'], sd[p + '.running_var'], sd[p + '.weight'], sd[p + '.bias'], False, 0.0, 1e-5)

    def lrelu(t):
        return F.leaky_relu(t, 0.1)

    pe = 'patch_embed.'
    o = lrelu(bn(F.conv2d(x, sd[pe + 'conv1.weight'], stride=2, padding=1), pe + 'bn1'))
    o = lrelu(bn(F.conv2d(o, sd[pe + 'conv2.weight'], padding=1), pe + 'bn2'))
    o = bn(F.conv2d(o, sd[pe + 'conv3.weight'], padding=1), pe + 'bn3')
    o = lrelu(o + bn(F.conv2d(x, sd[pe + 'downsample.0.weight'], stride=2, padding=1), pe + 'downsample.1'))
    o = F.max_pool2d(o, 2)
    if taps is not None:
        taps['stem'] = o
    t = F.conv2d(o, sd[pe + 'proj.weight'], sd[pe + 'proj.bias'], stride=4).flatten(2).transpose(1, 2)
    B, D = t.shape[0], t.shape[2]
    t = torch.cat([sd['cls_token'].expand(B, -1, -1), t], dim=1) + sd['pos_embed']
    if taps is not None:
        taps['embed'] = t
    N, hd = t.shape[1], D // heads
    for i in range(depth):
        p = f'blocks.{i}.'
        h = F.layer_norm(t, (D,), sd[p + 'norm1.weight'], sd[p + 'norm1.bias'], eps)
        q, k, v = F.linear(h, sd[p + 'attn.qkv.weight']).reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
        a = ((q * hd ** -0.5) @ k.transpose(-2, -1)).softmax(dim=-1)
        c = (a @ v).transpose(1, 2).reshape(B, N, heads * hd)
        t = t + F.linear(c, sd[p + 'attn.proj.weight'], sd[p + 'attn.proj.bias']) / skip_lam
        h = F.layer_norm(t, (D,), sd[p + 'norm2.weight'], sd[p + 'norm2.bias'], eps)
        t = t + F.linear(F.gelu(F.linear(h, sd[p + 'mlp.fc1.weight'], sd[p + 'mlp.fc1.bias'])), sd[p + 'mlp.fc2.weight'], sd[p + 'mlp.fc2.bias']) / skip_lam
        if taps is not None:
            taps[f'blocks.{i}'] = t
    return F.layer_norm(t, (D,), sd['norm.weight'], sd['norm.bias'], eps)[:, 0]


def test_registry_and_state_dict_match_the_reference():
    from fewshot_vit_amd import models
    g = golden()
    assert 'lvvit_micro_80' in models.models
    enc = models.make('lvvit_micro_80').cpu()
    sd = enc.state_dict()
    ref = golden_shapes(g)
    assert len(ref) == 118
    assert list(sd.keys()) == list(ref.keys())
    assert {k: tuple(v.shape) for k, v in sd.items()} == ref
    assert ref['patch_embed.conv1.weight'] == (96, 3, 3, 3) and ref['patch_embed.proj.weight'] == (384, 96, 4, 4)
    assert ref['blocks.0.attn.qkv.weight'] == (1152, 384) and 'blocks.0.attn.qkv.bias' not in ref
    assert enc.out_dim == 384 and enc.cfg['ln_eps'] == 1e-5 and enc.cfg['skip_lam'] == 2.0
    enc2 = models.make('lvvit_micro_80', numerics='bf16x2')
    assert enc2.numerics == 'bf16x2'


def test_torch_restatement_reproduces_reference_features():
    g = golden()
    sd = procedural_sd(golden_shapes(g))
    x = torch.randn(4, 3, 80, 80, generator=torch.Generator().manual_seed(5))
    taps = {}
    with torch.no_grad():
        feat = lvvit_forward(sd, x, taps)
    assert (feat - torch.from_numpy(g['feat'])).abs().max().item() <= 1e-5
    assert (taps['stem'][:1] - torch.from_numpy(g['tap.stem'])).abs().max().item() <= 1e-5
    for k in ('embed', 'blocks.3', 'blocks.7'):
        assert (taps[k][:2] - torch.from_numpy(g['tap.' + k])).abs().max().item() <= 1e-4, k


def test_reference_schema_checkpoints_load(tmp_path):
    from fewshot_vit_amd import models
    from fewshot_vit_amd.test_few_shot import build_model
    g = golden()
    enc_sd = procedural_sd(golden_shapes(g))
    mb_sv = {'model': 'meta-baseline', 'model_args': {'encoder': 'lvvit_micro_80', 'encoder_args': {}},
             'model_sd': dict({'encoder.' + k: v for k, v in enc_sd.items()}, temp=torch.tensor(10.0))}
    mb = models.load(mb_sv).cpu()
    assert type(mb.encoder).__name__ == 'LvVit'
    for k, v in enc_sd.items():
        assert torch.equal(mb.encoder.state_dict()[k], v), k
    # sun_train_teacher schema: classifier(encoder=lvvit_micro_80, classifier=linear-classifier); its encoder evaluated inside meta-baseline
    cls_sv = {'model': 'classifier',
              'model_args': {'encoder': 'lvvit_micro_80', 'encoder_args': {}, 'classifier': 'linear-classifier', 'classifier_args': {'n_classes': 64}},
              'model_sd': dict({'encoder.' + k: v for k, v in enc_sd.items()},
                               **{'classifier.linear.weight': torch.zeros(64, 384), 'classifier.linear.bias': torch.zeros(64)})}
    path = tmp_path / 'teacher.pth'
    torch.save(cls_sv, path)
    model = build_model({'load_encoder': str(path)})
    assert type(model).__name__ == 'MetaBaseline' and type(model.encoder).__name__ == 'LvVit'
    for k, v in enc_sd.items():
        assert torch.equal(model.encoder.state_dict()[k].cpu(), v), k


def test_synthetic_checkpoint_needs_no_calibration():
    from fewshot_vit_amd.test_few_shot import build_model
    model = build_model({'synthetic_checkpoint': 'lvvit_micro_80'}, numerics='bf16')
    assert type(model.encoder).__name__ == 'LvVit' and model.encoder.numerics == 'bf16'


def test_cpu_eval_refuses_and_training_is_not_built():
    from fewshot_vit_amd import models
    enc = models.make('lvvit_micro_80').cpu().eval()
    x = torch.zeros(2, 3, 80, 80)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        enc(x)
    mb = models.make('meta-baseline', encoder='lvvit_micro_80').cpu().eval()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        mb(torch.zeros(1, 5, 1, 3, 80, 80), torch.zeros(1, 5, 3, 80, 80))
    enc.train()
    with pytest.raises(NotImplementedError, match='LV-ViT'):
        enc(x)
    mb.train()
    with pytest.raises(NotImplementedError, match='LV-ViT'):
        mb(torch.zeros(1, 5, 1, 3, 80, 80), torch.zeros(1, 5, 3, 80, 80))
    with pytest.raises(NotImplementedError, match='img_size must be 80'):
        models.make('lvvit_micro_80', img_size=84)
    with pytest.raises(TypeError):
        models.make('lvvit_micro_80', mlp_ratoi=3.0)                     # unknown keyword: refused, not dropped
    assert models.make('lvvit_micro_80', drop_path_rate=0.5, mix_token=True, return_dense=True).out_dim == 384   # the reference's training-only keywords
