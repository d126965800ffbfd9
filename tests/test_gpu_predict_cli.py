"""python -m fewshot_vit_amd.predict on a tmp tree of PNGs: three classes with 1, 2 and 4 support images, five query images, a tiny registered Visformer
saved with the project's checkpoint schema."""
import csv
import os

import numpy as np
import pytest
import torch

import proto_bank_cases as pc

pytestmark = pytest.mark.gpu
TINY = dict(img_size=80, init_channels=8, embed_dim=64, depth=[1, 1, 1], num_heads=6, mlp_ratio=4., group=8)
CLASSES = ('ant', 'bee', 'cat')


def _png(path, rng, cls, size):
    from PIL import Image
    base = np.zeros((size[1], size[0], 3))
    base[..., cls] = 160.0                                   # a colour per class under noise
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.clip(base + rng.normal(40.0, 30.0, base.shape), 0, 255).astype(np.uint8)).save(path)


def _tree(root):
    rng = np.random.default_rng(5)
    for c, (name, n) in enumerate(zip(CLASSES, (1, 2, 4))):
        for i in range(n):
            _png(os.path.join(root, 'support', name, f's{i}.png'), rng, c, (96 + 8 * i, 100))
    for c, (name, n) in enumerate(zip(CLASSES, (2, 0, 3))):
        for i in range(n):
            _png(os.path.join(root, 'more', name, f'm{i}.png'), rng, c, (90, 90))
    for i in range(5):
        _png(os.path.join(root, 'query', f'q{i}.png'), rng, i % 3, (120, 92))
        _png(os.path.join(root, 'query_labelled', CLASSES[i % 3], f'q{i}.png'), rng, i % 3, (92, 92))


def _checkpoint(path):
    from fewshot_vit_amd import models
    from fewshot_vit_amd.models.visformer import Visformer
    models.register('tiny_visformer_cli')(lambda **a: Visformer(**TINY, **a))
    torch.manual_seed(3)
    m = models.make('meta-baseline', encoder='tiny_visformer_cli', encoder_args={})
    torch.save({'model': 'meta-baseline', 'model_args': {'encoder': 'tiny_visformer_cli', 'encoder_args': {}}, 'model_sd': m.state_dict()}, path)


def test_predict_cli(tmp_path, capsys):
    from fewshot_vit_amd import predict
    root = str(tmp_path)
    _tree(root)
    ck, bank_f, out_f = (os.path.join(root, n) for n in ('ck.pth', 'bank.pt', 'preds.csv'))
    _checkpoint(ck)
    res = predict.main(['--load', ck, '--support', os.path.join(root, 'support'), '--query', os.path.join(root, 'query'), '--numerics', 'parity',
                        '--out', out_f, '--save-bank', bank_f])
    assert res['classes'] == list(CLASSES) and res['bank'].counts.tolist() == [1, 2, 4]
    rows = list(csv.reader(open(out_f)))
    assert rows[0] == ['file', 'pred_class', 'logit_0', 'logit_1', 'logit_2'] and len(rows) == 1 + 5
    assert [os.path.basename(r[0]) for r in rows[1:]] == [f'q{i}.png' for i in range(5)]
    # the float64 head on the model's own features of the same transformed images
    model = predict.load_model(ck, numerics='parity').cuda().eval()
    sup, lab = predict.list_labelled(os.path.join(root, 'support'), list(CLASSES))
    assert lab == [0, 1, 1, 2, 2, 2, 2]
    f_sup = predict.encode_files(model, sup, 80, 91, 'cuda').cpu()
    f_q = predict.encode_files(model, [r[0] for r in rows[1:]], 80, 91, 'cuda').cpu()
    b = pc.bank_reference(f_sup, torch.tensor(lab), 3, 'cos')
    A, a = pc.logits_reference(f_q, b['proto'], b['a_proto'], b['empty'], float(model.temp.detach()), 'cos')
    got = torch.tensor([[float(v) for v in r[2:]] for r in rows[1:]], dtype=torch.float64)
    assert torch.equal(got.float(), res['logits']), 'the CSV does not round-trip the logits'
    worst = pc.ratio(got, A, a)
    top2 = A.topk(2, -1).values
    print(f'predict: logits err/bound {worst:.3f}, float64 margins {(top2[:, 0] - top2[:, 1]).tolist()}')
    assert worst <= 1.0
    assert bool(((top2[:, 0] - top2[:, 1]) > 2.0 * a.max(-1).values).all()), 'a float64 arg-max is closer than the allowance: the comparison tests nothing'
    assert [int(r[1]) for r in rows[1:]] == A.argmax(-1).tolist() == res['pred'].tolist()

    # a stored bank extended with more/ (no 'bee' images there): counts 1 + 2, 2 + 0, 4 + 3; labelled queries print the accuracy
    capsys.readouterr()
    res2 = predict.main(['--load', ck, '--load-bank', bank_f, '--support', os.path.join(root, 'more'), '--query', os.path.join(root, 'query_labelled'),
                         '--numerics', 'parity'])
    assert res2['bank'].counts.tolist() == [3, 2, 7]
    assert 'accuracy:' in capsys.readouterr().out and 0.0 <= res2['acc'] <= 1.0
    truth = [CLASSES.index(os.path.basename(os.path.dirname(p))) for p in res2['files']]
    assert res2['acc'] == pytest.approx(float(np.mean(np.array(truth) == res2['pred'].numpy())))
    # the reloaded bank alone reproduces the first run's logits bit for bit
    res3 = predict.main(['--load', ck, '--load-bank', bank_f, '--query', os.path.join(root, 'query'), '--numerics', 'parity'])
    assert torch.equal(res3['logits'], res['logits'])
    with pytest.raises(ValueError, match='not one of'):
        os.makedirs(os.path.join(root, 'other', 'dog'))
        predict.main(['--load', ck, '--load-bank', bank_f, '--support', os.path.join(root, 'other')])
