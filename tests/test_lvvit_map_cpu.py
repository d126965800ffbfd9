"""CPU checks of the (token map, cls) output of `lvvit_micro_80` (sun_meta_training/models/lvvit.py:529-552) against tests/golden/lvvit_map.npz
(make_lvvit_map_golden.py): the plain-torch restatement reproduces both outputs, the cls feature is the one of lvvit.npz, the encoder and the
`token-label` model over it construct with the reference's state-dict keys, the CPU refusals keep their types, and the two LV-ViT configs load."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from test_lvvit_cpu import golden as lvvit_golden, golden_shapes, lvvit_forward, procedural_sd

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'lvvit_map.npz')
CONFIGS = os.path.join(os.path.dirname(HERE), 'few-shot-vit_amd', 'configs')


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_torch_restatement_reproduces_reference_map_and_cls():
    g, gl = golden(), lvvit_golden()
    sd = procedural_sd(golden_shapes(gl))
    x = torch.randn(4, 3, 80, 80, generator=torch.Generator().manual_seed(5))
    taps = {}
    with torch.no_grad():
        lvvit_forward(sd, x, taps)
        rows = F.layer_norm(taps['blocks.7'], (384,), sd['norm.weight'], sd['norm.bias'], 1e-5)
    fmap = rows[:, 1:].permute(0, 2, 1).reshape(4, 384, 5, 5)
    assert g['map'].shape == (4, 384, 5, 5) and g['cls'].shape == (4, 384)
    assert (fmap - torch.from_numpy(g['map'])).abs().max().item() <= 1e-5
    assert (rows[:, 0] - torch.from_numpy(g['cls'])).abs().max().item() <= 1e-5


def test_cls_is_the_feature_of_the_cls_only_golden():
    assert np.array_equal(golden()['cls'], lvvit_golden()['feat'])


def test_construction_and_token_label_keys():
    from fewshot_vit_amd import models
    g = golden()
    enc = models.make('lvvit_micro_80', return_map=True)
    assert enc.return_map and enc.out_dim == 384
    m = models.make('token-label', encoder='lvvit_micro_80', encoder_args={'return_map': True}, classifier='linear-classifier',
                    classifier_args={'n_classes': 64})
    assert list(m.state_dict().keys()) == g['tl.keys'].tolist()
    assert tuple(m.classifier_local.linear.weight.shape) == (65, 384) and tuple(m.classifier.linear.weight.shape) == (64, 384)


def test_no_cpu_path():
    from fewshot_vit_amd import models
    enc = models.make('lvvit_micro_80', return_map=True).cpu().eval()
    x = torch.zeros(2, 3, 80, 80)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        enc(x)
    enc.train()
    with pytest.raises(NotImplementedError, match='LV-ViT'):
        enc(x)


@pytest.mark.parametrize('name,model', [('offline_lvvit_synthetic.yaml', 'token-label'), ('train_classifier_lvvit_synthetic.yaml', 'classifier')])
def test_lvvit_configs_load_and_build(name, model):
    from fewshot_vit_amd import models
    config = yaml.load(open(os.path.join(CONFIGS, name)), Loader=yaml.FullLoader)
    assert config['model'] == model and config['model_args']['encoder'] == 'lvvit_micro_80'
    assert config['model_args']['encoder_args'] == {'drop_path_rate': 0.1} and config['synthetic_checkpoint'] == 'lvvit_micro_80'
    m = models.make(config['model'], **config['model_args'])
    assert type(m.encoder).__name__ == 'LvVit' and m.encoder.drop_path_rate == 0.1
