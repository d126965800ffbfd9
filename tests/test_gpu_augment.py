"""Train-time augmentation `augment: resize` through the C-ABI (fsvit_image_transform_rrc_gather): RandomResizedCrop(80) + RandomHorizontalFlip +
ToTensor + Normalize on the GPU, bit-exact against Pillow's own vectors (tests/golden/transform_rrc_pil.npz) and against the Pillow-pinned oracle
resize of the cropped array: the uint8 resize is integer work on coefficient tables the kernel computes in fp64 per box, the normalisation is two
correctly-rounded fp32 operations."""
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _normalise(u8):
    """uint8 [80, 80, 3] -> float32 [3, 80, 80]: ToTensor + Normalize as test_gpu_transform.py computes them."""
    from oracle import transform_oracle as to
    t = u8.astype(np.float32) / np.float32(255)
    return np.ascontiguousarray(((t - to.MEAN) / to.STD).transpose(2, 0, 1))


def _oracle(img, box, flip):
    """The reference transform restated: crop, Pillow BILINEAR resize to 80 x 80, mirror, ToTensor, Normalize."""
    from oracle import transform_oracle as to
    i, j, h, w = (int(v) for v in box)
    r = to.pil_resize_bilinear(img[i:i + h, j:j + w], 80, 80)
    return _normalise(r[:, ::-1] if flip else r)


@pytest.fixture(scope='module')
def sources(golden_dir):
    z = np.load(os.path.join(golden_dir, 'transform_rrc_pil.npz'))
    return z, [np.load(os.path.join(golden_dir, 'transform_pil.npz'))['images'], z['src32'][None], z['src60x100'][None]]


def _run(images, index, boxes, flips):
    from fewshot_vit_amd.datasets.transforms import DeviceRandomResizedCrop
    dev = torch.device('cuda', 0)
    tf = DeviceRandomResizedCrop(images.shape[1:3], 80, dev)
    out = tf(torch.from_numpy(images).to(dev), torch.as_tensor(index), boxes=torch.as_tensor(np.asarray(boxes, np.int32)),
             flips=torch.as_tensor(np.asarray(flips, np.uint8)))
    assert tuple(out.shape) == (len(index), 3, 80, 80) and out.dtype == torch.float32
    return out.cpu().numpy()


def test_fixture_cases_bit_exact_vs_pillow(sources):
    z, tables = sources
    src, box, flip, gold = z['case_source'], z['case_box'], z['case_flip'], z['out']
    for table, sel in ((0, src < 4), (1, src == 4), (2, src == 5)):       # all cases of one source table in one call
        index = src[sel] if table == 0 else np.zeros(int(sel.sum()), np.int64)
        assert len(index) > len(set(index.tolist()))                      # a repeated index among them
        out = _run(tables[table], index, box[sel], flip[sel])
        for k, g in enumerate(gold[sel]):
            assert np.array_equal(out[k], _normalise(g)), (table, box[sel][k].tolist(), int(flip[sel][k]))


def _sweep_84():
    cases, n = [], 0
    for k in range(1, 85):
        for h, w in ((k, k), (k, 85 - k)):
            top, left = ((0, 0), (0, 84 - w), (84 - h, 0), (84 - h, 84 - w))[(n // 2) % 4]
            cases.append(((top, left, h, w), n % 2))
            n += 1
    return cases


def _sweep_60x100():
    cases = [((0, (0, 100 - w)[w % 2], 60, w), (w // 2) % 2) for w in range(1, 101)]
    return cases + [(((0, 60 - h)[h % 2], 0, h, 100), (h // 2) % 2) for h in range(1, 61)]


@pytest.mark.parametrize('table,image,cases', [(0, 3, _sweep_84()), (2, 0, _sweep_60x100())], ids=['84x84', '60x100'])
def test_every_box_size_bit_exact_vs_oracle(sources, table, image, cases):
    """Every crop width and height a source admits: each gives its own scale, and one contracted multiply-add or one re-associated sum in the
    kernel's fp64 table arithmetic moves int(center - support + 0.5) or a 22-bit tap at scales such as 0.6 or 1.2."""
    imgs = sources[1][table]
    out = _run(imgs, np.full(len(cases), image), [c[0] for c in cases], [c[1] for c in cases])
    bad = [(box, flip) for k, (box, flip) in enumerate(cases) if not np.array_equal(out[k], _oracle(imgs[image], box, flip))]
    assert not bad, (len(bad), bad[:8])


def test_sweep_on_the_32x32_source_bit_exact_vs_oracle(sources):
    img = sources[1][1]
    cases = [((k % 2 * (32 - k), (k // 2) % 2 * (32 - k), k, k), k % 2) for k in range(1, 33)]
    cases += [((0, 0, k, 33 - k), (k // 2) % 2) for k in range(1, 33)]
    out = _run(img, np.zeros(len(cases), np.int64), [c[0] for c in cases], [c[1] for c in cases])
    bad = [(box, flip) for k, (box, flip) in enumerate(cases) if not np.array_equal(out[k], _oracle(img[0], box, flip))]
    assert not bad, (len(bad), bad[:8])


def _mini_pickle(path, n_cls, per, seed):
    rng = np.random.default_rng(seed)
    mu = rng.integers(0, 256, size=(n_cls, 1, 84, 84, 3))
    data = np.clip(mu + rng.normal(0, 60, size=(n_cls, per, 84, 84, 3)), 0, 255).astype(np.uint8).reshape(-1, 84, 84, 3)
    with open(os.path.join(str(path), 'miniImageNet_category_split_train_phase_train.pickle'), 'wb') as f:
        pickle.dump({'data': data, 'labels': [64 + i // per for i in range(n_cls * per)]}, f)
    return data


def test_dataset_gather_draws_boxes_reproducibly(tmp_path):
    from fewshot_vit_amd import datasets
    from oracle import transform_oracle as to
    data = _mini_pickle(tmp_path, 3, 4, 9)
    make = lambda: datasets.make('mini-imagenet', root_path=str(tmp_path), split='train', augment='resize')
    a, b = make(), make()
    idx = torch.tensor([5, 0, 11, 5, 7, 2])
    a.transform.manual_seed(21)
    b.transform.manual_seed(21)
    xa = a.gather(idx).cpu().numpy()
    boxes, flips = a.transform.boxes.clone(), a.transform.flips.clone()
    assert tuple(boxes.shape) == (6, 4) and tuple(flips.shape) == (6,)
    assert np.array_equal(xa, b.gather(idx).cpu().numpy())                               # same seed, same batch
    b.transform.manual_seed(22)
    assert not np.array_equal(xa, b.gather(idx).cpu().numpy())                           # another seed, another batch
    for k, i in enumerate(idx.tolist()):                                                 # the boxes and flips the transform reports
        assert np.array_equal(xa[k], _oracle(data[i], boxes[k].tolist(), bool(flips[k]))), (k, boxes[k].tolist())
    a.transform.manual_seed(33)                                                          # __getitem__ goes through self.transform
    x3, y3 = a[3]
    assert y3 == 0 and tuple(a.transform.boxes.shape) == (1, 4)
    assert np.array_equal(x3.cpu().numpy(), _oracle(data[3], a.transform.boxes[0].tolist(), bool(a.transform.flips[0])))
    a.transform = a.default_transform                                                    # the augmentation switched off: Resize(80)
    xd = a.gather(idx).cpu().numpy()
    assert np.array_equal(xd, np.stack([to.eval_transform(data[i], 80, 80) for i in idx.tolist()]))
    assert np.array_equal(a[3][0].cpu().numpy(), to.eval_transform(data[3], 80, 80))


def test_train_classifier_runs_the_reference_augment_args(tmp_path, monkeypatch):
    """`train_dataset_args: {split: train, augment: resize}` through the supervised driver: one augmented epoch and the `epoch_ex` epoch under
    the default transform; the same seed gives the same run."""
    from fewshot_vit_amd import train_classifier
    from oracle import transform_oracle as to
    data = _mini_pickle(tmp_path, 6, 20, 5)
    config = dict(train_dataset='mini-imagenet', train_dataset_args=dict(root_path=str(tmp_path), split='train', augment='resize'),
                  model='classifier', model_args=dict(encoder='visformer_micro_80', encoder_args=dict(drop_path_rate=0.0),
                                                      classifier='linear-classifier', classifier_args=dict(n_classes=6)),
                  synthetic_checkpoint='visformer_micro_80', batch_size=16, train_batches=2, max_epoch=1, epoch_ex=True, optimizer='adamw', seed=7,
                  optimizer_args=dict(lr=5e-4, weight_decay=0.05, warmup_lr=1e-6, warmup=1))
    seen = []
    inner = train_classifier._gather

    def recording_gather(dataset, idx, device):
        x, y = inner(dataset, idx, device)
        seen.append((idx.tolist(), x.cpu().numpy(), y.tolist()))
        return x, y
    monkeypatch.setattr(train_classifier, '_gather', recording_gather)
    logs = []
    for run in ('a', 'b'):
        torch.manual_seed(99)
        logs.append(train_classifier.main(config, name=run, device=torch.device('cuda', 0), log=lambda *_: None, save_root=str(tmp_path)))
    assert len(logs[0]['tl']) == 2 and np.isfinite(logs[0]['tl']).all()
    assert logs[0] == logs[1]
    assert len(seen) == 8                                                                # 2 runs x (1 + 1 epochs) x 2 batches
    for k, (idx, x, y) in enumerate(seen[:4]):
        plain = np.stack([to.eval_transform(data[i], 80, 80) for i in idx])
        assert x.shape == (16, 3, 80, 80) and y == [i // 20 for i in idx]
        if k < 2:
            assert not np.array_equal(x, plain)                                          # the augmented epoch
        else:
            assert np.array_equal(x, plain)                                              # epoch_ex: the default transform
        assert np.array_equal(x, seen[4 + k][1]) and idx == seen[4 + k][0]               # the second run saw the same data
