"""RandAugment on the GPU (fsvit_image_rand_augment) through the C-ABI and the two pipelines built on it, bit-exact against the numpy restatement
tests/randaug_ref.py, which tests/test_randaug_cpu.py pins to Pillow: every operation is integer work or uncontracted IEEE float64 / float32
arithmetic, so no tolerance appears; only the erase noise of the last stage is skipped (its box is compared for finiteness).  Every launch has at
most 32 images; views are 80 x 80, the kernel's only size."""
import ctypes as C
import glob
import os
import pickle

import numpy as np
import pytest
import torch

import augment_ref as A
import randaug_ref as R
from fewshot_vit_amd.datasets import transforms as T

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
NONE = np.zeros(T.RA_OP_COLS, np.int32)
SPECIAL = ('stripes', 'constant', 'narrow', 'bright')


@pytest.fixture(scope='module')
def sources():
    return R.sources()


def _run(views, slots, table, fill=None):
    """views uint8 [B, 80, 80, 3] numpy -> the batch after the launch, and the restatement's."""
    assert len(slots) <= 32 and len(views) <= 32
    tf = T.DeviceStrongWeakPair((84, 84), 80, DEV)
    if fill is not None:
        tf.fill[:] = fill
    slots, table = torch.as_tensor(np.asarray(slots, np.int32)), torch.as_tensor(np.asarray(table, np.int32).reshape(len(slots), T.RA_COLS))
    dev = torch.from_numpy(np.ascontiguousarray(views)).to(DEV)
    out = tf.rand_augment(dev, slots, table)
    assert out is dev                                                   # in place
    return out.cpu().numpy(), R.rand_augment(views, slots.numpy(), table.numpy(), tuple(tf.fill))


def _mismatches(got, ref):
    return [(k, int((got[k] != ref[k]).sum())) for k in range(len(ref)) if not np.array_equal(got[k], ref[k])]


@pytest.mark.parametrize('name', T.RAND_INCREASING_OPS)
def test_each_operation_alone_is_bit_exact(sources, name):
    """Both signs and m in {0, 9, 10} on the four special sources: 24 images, the operation in the first slot or the second."""
    views, rows = [], []
    for key in SPECIAL:
        for m in (0, 9, 10):
            for neg in (False, True):
                op = T.rand_augment_op(name, m, neg)
                views.append(sources[key])
                rows.append(np.concatenate([op, NONE] if len(rows) % 2 == 0 else [NONE, op]))
    views = np.stack(views)
    got, ref = _run(views, np.arange(len(rows)), rows)
    assert not _mismatches(got, ref), _mismatches(got, ref)
    assert sum(not np.array_equal(ref[k], views[k]) for k in range(len(rows))) >= 4         # the operation does something


PAIRS = [(a, b) for a in range(15) for b in range(15)]


@pytest.mark.parametrize('chunk', range(0, 225, 32))
def test_all_ordered_operation_pairs_on_the_stripes(sources, chunk):
    pairs = PAIRS[chunk:chunk + 32]
    rows = [np.concatenate([T.rand_augment_op(T.RAND_INCREASING_OPS[a], 9, (a + b) % 2 == 0), T.rand_augment_op(T.RAND_INCREASING_OPS[b], 8.6, b % 2 == 0)])
            for a, b in pairs]
    views = np.repeat(sources['stripes'][None], len(pairs), 0)
    got, ref = _run(views, np.arange(len(pairs)), rows)
    bad = _mismatches(got, ref)
    assert not bad, [(pairs[k], n) for k, n in bad]
    if chunk == 0:                                                      # the order matters: (a, b) is not (b, a)
        row = rows[PAIRS.index((1, 3))]                                 # Equalize, then Rotate: the fill colour is not in the histogram
        swapped = R.apply_op(R.apply_op(sources['stripes'], row[T.RA_OP_COLS:]), row[:T.RA_OP_COLS])
        assert not np.array_equal(R.apply_row(sources['stripes'], row), swapped)


def test_only_the_listed_images_are_touched(sources):
    rng = np.random.default_rng(4)
    views = rng.integers(0, 256, size=(32, 80, 80, 3), dtype=np.uint8)
    views[5], views[31] = sources['stripes'], sources['narrow']
    slots = [0, 5, 6, 17, 18, 30, 31]
    names = ('Rotate', 'Equalize', 'SharpnessIncreasing', 'Invert', 'ShearY', 'AutoContrast', 'TranslateXRel', 'ColorIncreasing')
    rows = [np.concatenate([T.rand_augment_op(names[k], 9, k % 2 == 0), T.rand_augment_op(names[k + 1], 9.5, k % 2 == 1)]) for k in range(7)]
    got, ref = _run(views, slots, rows)
    rest = [k for k in range(32) if k not in slots]
    assert np.array_equal(got[rest], views[rest])                       # 25 views byte-identical
    assert not _mismatches(got, ref)
    assert all(not np.array_equal(got[k], views[k]) for k in slots)


def test_empty_list_and_single_image(sources):
    views = np.stack([sources['noise'], sources['stripes']])
    got, _ = _run(views, [], np.zeros((0, T.RA_COLS), np.int32))
    assert np.array_equal(got, views)                                   # n_slots = 0: nothing launched, nothing changed
    row = np.concatenate([T.rand_augment_op('Equalize', 9, False), T.rand_augment_op('Rotate', 10, True)])       # the corners end as the fill
    got, ref = _run(views[:1], [0], [row], fill=(1, 2, 254))            # B = 1, and another fill colour
    assert np.array_equal(got, ref) and (got[0, 0, 0] == (1, 2, 254)).all() and not np.array_equal(got, views[:1])


def test_argument_errors():
    from fewshot_vit_amd import _lib
    from fewshot_vit_amd.engine import _ptr
    lib = _lib.load()
    tf = T.DeviceStrongWeakPair((84, 84), 80, DEV)
    v = torch.zeros(2, 80, 80, 3, dtype=torch.uint8, device=DEV)
    slots = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    tab = torch.zeros(2, T.RA_COLS, dtype=torch.int32, device=DEV)
    call = lambda views, B, H, W, s, n, t, cols, fill: _lib.check(lib.fsvit_image_rand_augment(views, B, H, W, s, n, t, cols, fill, None))
    good = (_ptr(v), 2, 80, 80, _ptr(slots), 2, _ptr(tab), T.RA_COLS, tf.fill)
    call(*good)
    for pos, value in ((0, None), (8, None), (4, None), (6, None), (2, 64), (3, 84), (7, T.RA_COLS - 1), (1, -1), (5, 3), (5, -1), (0, C.c_void_p(v.data_ptr() + 8))):
        args = list(good)
        args[pos] = value
        with pytest.raises(ValueError):
            call(*args)
    call(_ptr(v), 2, 80, 80, None, 0, None, T.RA_COLS, tf.fill)         # nothing listed: the two arrays may be empty
    torch.cuda.synchronize()
    assert not v.any()
    with pytest.raises(ValueError):
        tf.rand_augment(torch.zeros(2, 64, 64, 3, dtype=torch.uint8, device=DEV), slots.cpu(), tab.cpu())


# ---------------------------------------------------------------- the two pipelines, the datasets and the drivers
def _mini_pickles(path, n_cls, per, seed):
    rng = np.random.default_rng(seed)
    mu = rng.integers(0, 256, size=(n_cls, 1, 84, 84, 3))
    data = np.clip(mu + rng.normal(0, 60, size=(n_cls, per, 84, 84, 3)), 0, 255).astype(np.uint8).reshape(-1, 84, 84, 3)
    for tag in ('train_phase_train', 'val'):
        with open(os.path.join(str(path), f'miniImageNet_category_split_{tag}.pickle'), 'wb') as f:
            pickle.dump({'data': data, 'labels': [64 + i // per for i in range(n_cls * per)]}, f)
    return data


def _clone(params):
    return {k: (tuple(t.clone() for t in v) if isinstance(v, tuple) else v.clone() if torch.is_tensor(v) else v) for k, v in params.items()}


def test_view_pair_with_the_weak_views_randaugment():
    rng = np.random.default_rng(8)
    data = rng.integers(0, 256, size=(6, 84, 84, 3), dtype=np.uint8)
    data[1, :, 30:60] = np.where((np.arange(30) // 2 % 2)[None, :, None] == 0, 255, 0)
    images = torch.from_numpy(data).to(DEV)
    idx = [1, 0, 5, 1, 3, 2, 4, 1, 0, 3, 2, 5, 1, 4, 0, 2]
    tf = T.DeviceStrongWeakPair((84, 84), 80, DEV, seed=31, weak_randaug=1.0)
    strong, weak = (x.cpu().numpy() for x in tf(images, torch.tensor(idx)))
    params = _clone(tf.params)
    slots, table = params['randaug']
    assert 8 <= slots.numel() <= 16 and len(set(table.view(-1, T.RA_OP_COLS)[:, T.RA_CODE].tolist())) >= 5
    views = R.weak_views(data, idx, params)
    plain = R.weak_views(data, idx, {k: v for k, v in params.items() if k != 'randaug'})
    assert sum(not np.array_equal(views[k], plain[k]) for k in slots.tolist()) >= slots.numel() // 2
    for k in range(len(idx)):
        ref_s, ref_w, mask = A.pair(views[k], params['table'][k].numpy())
        assert np.array_equal(weak[k], ref_w), k                        # the weak view carries the RandAugment
        assert np.array_equal(strong[k][:, ~mask], ref_s[:, ~mask]), k  # and the strong view is made from it
    again = tf(images, torch.tensor(idx), params=params)                # replay from the reported params: erase noise included
    assert np.array_equal(again[0].cpu().numpy(), strong) and np.array_equal(again[1].cpu().numpy(), weak)
    off = T.DeviceStrongWeakPair((84, 84), 80, DEV, seed=31)(images, torch.tensor(idx))
    assert np.array_equal(off[1].cpu().numpy(), np.stack([A.normalise(v) for v in plain]))              # the default is the two-launch pair


def test_randaug_crop_through_mini_imagenet(tmp_path):
    from fewshot_vit_amd import datasets
    from oracle import transform_oracle as to
    data = _mini_pickles(tmp_path, 3, 4, 9)
    make = lambda: datasets.make('mini-imagenet', root_path=str(tmp_path), split='train', augment='randaug')
    a, b = make(), make()
    idx = [5, 0, 11, 5, 7, 2, 3, 3, 9, 1, 10, 4, 6, 8, 0, 11]
    a.transform.manual_seed(21)
    b.transform.manual_seed(21)
    x = a.gather(torch.tensor(idx)).cpu().numpy()
    params = _clone(a.transform.params)
    assert x.shape == (16, 3, 80, 80) and x.dtype == np.float32 and np.isfinite(x).all()
    assert not params['table'][:, T.SW_STRONG].any() and (params['table'][:, T.SW_ERASE + 2] > 0).sum() >= 1 and params['randaug'][0].numel() >= 8
    views = R.weak_views(data, idx, params)
    for k in range(len(idx)):
        mask = A.erase_mask(params['table'][k].numpy())
        assert np.array_equal(x[k][:, ~mask], A.normalise(views[k])[:, ~mask]), k
    assert np.array_equal(b.gather(torch.tensor(idx)).cpu().numpy(), x)                                 # same seed, same batch
    assert np.array_equal(b.transform(b.device_images(), torch.tensor(idx), params=params).cpu().numpy(), x)      # replay
    x3, y3 = a[3]
    assert y3 == 0 and tuple(x3.shape) == (3, 80, 80)
    a.transform = a.default_transform                                   # the augmentation switched off: Resize(80)
    assert np.array_equal(a.gather(torch.tensor(idx[:3])).cpu().numpy(), np.stack([to.eval_transform(data[i], 80, 80) for i in idx[:3]]))


def _moved(tmp_path):
    """The checkpoint the driver left against the synthetic weights it started from: how many encoder tensors differ."""
    from fewshot_vit_amd import synthetic
    path, = glob.glob(os.path.join(str(tmp_path), '**', 'epoch-last.pth'), recursive=True)
    sd = torch.load(path, map_location='cpu')['model_sd']
    enc = {k: v for k, v in sd.items() if k.startswith('encoder.')}
    start = synthetic.synthetic_checkpoint_sd({k: tuple(v.shape) for k, v in enc.items()}, calib='visformer_micro_80')
    assert all(bool(torch.isfinite(v.float()).all()) for v in enc.values())
    return sum(not torch.equal(enc[k].float(), start[k].float()) for k in enc if enc[k].dtype.is_floating_point and enc[k].dim() > 1), len(enc)


def test_train_classifier_steps_on_randaug(tmp_path, monkeypatch):
    from fewshot_vit_amd import train_classifier
    _mini_pickles(tmp_path, 6, 12, 5)
    config = dict(train_dataset='mini-imagenet', train_dataset_args=dict(root_path=str(tmp_path), split='train', augment='randaug'),
                  model='classifier', model_args=dict(encoder='visformer_micro_80', encoder_args=dict(drop_path_rate=0.0),
                                                      classifier='linear-classifier', classifier_args=dict(n_classes=6)),
                  synthetic_checkpoint='visformer_micro_80', batch_size=16, train_batches=2, max_epoch=1, optimizer='adamw', seed=7,
                  optimizer_args=dict(lr=5e-4, weight_decay=0.05, warmup_lr=1e-6, warmup=1))
    seen = []
    inner = train_classifier._gather

    def gather(dataset, idx, device):
        x, y = inner(dataset, idx, device)
        seen.append((isinstance(dataset.transform, T.DeviceRandAugCrop), x.cpu().numpy(), y.tolist(), idx.tolist()))
        return x, y
    monkeypatch.setattr(train_classifier, '_gather', gather)
    trlog = train_classifier.main(config, name='ra', device=DEV, log=lambda *_: None, save_root=str(tmp_path))
    assert len(trlog['tl']) == 1 and np.isfinite(trlog['tl']).all()
    assert len(seen) == 2
    for augmented, x, y, idx in seen:
        assert augmented and x.shape == (16, 3, 80, 80) and np.isfinite(x).all() and y == [i // 12 for i in idx]
    moved, total = _moved(tmp_path)
    assert moved > 0 and total > 0, (moved, total)


def test_offline_distills_with_the_weak_views_randaugment(tmp_path, monkeypatch):
    from fewshot_vit_amd import offline
    _mini_pickles(tmp_path, 6, 12, 5)
    config = dict(train_dataset='mini-imagenet',
                  train_dataset_args=dict(root_path=str(tmp_path), split='train', augment='strongweak', weak_randaug=0.2),
                  val_dataset='mini-imagenet', val_dataset_args=dict(root_path=str(tmp_path), split='val'),
                  model='token-label', model_args=dict(encoder='visformer_micro_80', encoder_args=dict(drop_path_rate=0.0),
                                                       classifier='linear-classifier', classifier_args=dict(n_classes=6)),
                  synthetic_checkpoint='visformer_micro_80', batch_size=16, train_batches=2, eval_batches=1, max_epoch=1, seed=3,
                  n_way=5, n_shot=1, n_query=2, ep_per_batch=1, tl_soft_k=3, bg_token_num=10, optimizer='adamw',
                  optimizer_args=dict(lr=5e-4, weight_decay=0.05, warmup_lr=1e-6, warmup=1))
    seen, losses, moved = [], [], []
    inner_gather, inner_step = offline._gather, offline.distill_step

    def gather(dataset, idx, device):
        out = inner_gather(dataset, idx, device)
        tf = getattr(dataset, 'transform', None)
        if isinstance(tf, T.DeviceStrongWeakPair):
            seen.append((tf.weak_randaug, 'randaug' in tf.params, out[0].cpu().numpy(), out[1].cpu().numpy()))
        return out

    def step(model, *a, **kw):
        before = [p.detach().clone() for p in model.parameters()]
        out = inner_step(model, *a, **kw)
        losses.append(float(out[0]))
        moved.append(sum(not torch.equal(b, p.detach()) for b, p in zip(before, model.parameters())))
        return out
    monkeypatch.setattr(offline, '_gather', gather)
    monkeypatch.setattr(offline, 'distill_step', step)
    trlog = offline.main(config, name='ra', device=DEV, log=lambda *_: None, save_root=str(tmp_path))
    assert len(losses) == 2 and np.isfinite(losses).all() and np.isfinite(trlog['tl']).all()
    assert len(seen) == 2
    for p, drawn, strong, weak in seen:
        assert p == 0.2 and drawn and strong.shape == weak.shape == (16, 3, 80, 80) and np.isfinite(strong).all() and np.isfinite(weak).all()
    assert len(moved) == 2 and min(moved) > 0, moved                    # every step moves parameters
