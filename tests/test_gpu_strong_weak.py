"""The distillation phase's strong / weak view pair through the C-ABI (fsvit_image_transform_rrc_u8 + fsvit_image_strong_weak), bit-exact against
the numpy restatement tests/augment_ref.py, which tests/test_strong_weak_cpu.py pins to Pillow: the byte stages are integer work plus one fp32
multiply and one fp32 add per blend, the normalisation two correctly rounded fp32 operations.  Only the erase noise is statistical.  Every launch
has at most 32 images."""
import itertools
import os
import pickle

import numpy as np
import pytest
import torch

import augment_ref as R
from fewshot_vit_amd.datasets import transforms as T

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


@pytest.fixture(scope='module')
def sources(golden_dir):
    """84 x 84 noise with a band of saturating 2-pixel stripes (bicubic overshoot beyond 0..255 on both sides), and a 32 x 32 one."""
    rng = np.random.default_rng(7)
    s84 = rng.integers(0, 256, size=(84, 84, 3), dtype=np.uint8)
    s84[:, 30:60] = np.where((np.arange(30) // 2 % 2)[None, :, None] == 0, 255, 0)
    s32 = rng.integers(0, 256, size=(32, 32, 3), dtype=np.uint8)
    s32[10:20] = np.where((np.arange(10) % 2)[:, None, None] == 0, 255, 0)
    return {'84': s84[None], '32': s32[None], 'base': np.load(os.path.join(golden_dir, 'transform_pil.npz'))['images']}


def _crop_u8(images, index, boxes, flips, filter):
    tf = T.DeviceStrongWeakPair(images.shape[1:3], 80, DEV)
    out = tf.crop_u8(torch.from_numpy(images).to(DEV), torch.as_tensor(index), torch.as_tensor(np.asarray(boxes, np.int32)),
                     torch.as_tensor(np.asarray(flips, np.uint8)), filter)
    assert tuple(out.shape) == (len(index), 80, 80, 3) and out.dtype == torch.uint8
    return out.cpu().numpy()


def _sweep_84():
    cases, n = [], 0
    for k in range(1, 85):
        for h, w in ((k, k), (k, 85 - k)):
            top, left = ((0, 0), (0, 84 - w), (84 - h, 0), (84 - h, 84 - w))[(n // 2) % 4]
            cases.append(((top, left, h, w), n % 2))
            n += 1
    return cases


def _sweep_32():
    cases = [((k % 2 * (32 - k), (k // 2) % 2 * (32 - k), k, k), k % 2) for k in range(1, 33)]
    return cases + [((0, 0, k, 33 - k), (k // 2) % 2) for k in range(1, 33)]


SWEEPS = [('84', _sweep_84()[i:i + 28]) for i in range(0, 168, 28)] + [('32', _sweep_32()[i:i + 32]) for i in range(0, 64, 32)]


@pytest.mark.parametrize('chunk', range(len(SWEEPS)), ids=[f'{s}-{k}' for k, (s, _) in enumerate(SWEEPS)])
def test_rrc_u8_bicubic_bit_exact_at_every_box_size(sources, chunk):
    """Every crop width and height of the 84 x 84 and the 32 x 32 source (each its own scale and tap count), on stripes that drive the negative-tap
    overshoot into clip8."""
    src, cases = SWEEPS[chunk]
    imgs = sources[src]
    out = _crop_u8(imgs, np.zeros(len(cases), np.int64), [c[0] for c in cases], [c[1] for c in cases], 'bicubic')
    ref = [R.weak_view(imgs[0], box, flip) for box, flip in cases]
    bad = [(box, flip) for k, (box, flip) in enumerate(cases) if not np.array_equal(out[k], ref[k])]
    assert not bad, (len(bad), bad[:8])
    if chunk in (2, 6):                                   # mid-size boxes over the stripes: the clip is exercised, and bicubic is not bilinear
        assert sum(int((r == 0).sum() + (r == 255).sum()) for r in ref) > 1000
        assert any(not np.array_equal(ref[k], R.weak_view(imgs[0], box, flip, filter='bilinear')) for k, (box, flip) in enumerate(cases))


def test_rrc_u8_bilinear_is_the_existing_kernel_denormalised(sources):
    """The shared kernel body did not move: the bytes of the bilinear u8 epilogue, normalised, are fsvit_image_transform_rrc_gather's output."""
    imgs = sources['base']
    g = torch.Generator().manual_seed(5)
    boxes = T.random_resized_crop_boxes(32, 84, 84, g)
    boxes[:4] = torch.tensor([[0, 0, 84, 84], [83, 83, 1, 1], [2, 3, 50, 80], [4, 10, 80, 40]], dtype=torch.int32)
    flips = torch.rand(32, generator=g) < 0.5
    index = torch.arange(32) % 4
    u8 = _crop_u8(imgs, index, boxes, flips, 'bilinear')
    ref = T.DeviceRandomResizedCrop((84, 84), 80, DEV)(torch.from_numpy(imgs).to(DEV), index, boxes=boxes, flips=flips).cpu().numpy()
    for k in range(32):
        assert np.array_equal(R.normalise(u8[k]), ref[k]), (k, boxes[k].tolist())
        assert np.array_equal(u8[k], R.weak_view(imgs[index[k]], boxes[k].tolist(), bool(flips[k]), filter='bilinear')), k


# ---------------------------------------------------------------- the colour stage
@pytest.fixture(scope='module')
def views(sources):
    """uint8 80 x 80 x 3 views: 0 noise, 1 smooth ramp + noise, 2 saturating stripes, 3 uniform (77, 130, 201), 4 all 0, 5 all 255, 6 dark noise."""
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:80, 0:80]
    smooth = np.clip(np.stack([yy * 3, xx * 3, (yy + xx) * 1.5], -1) + rng.normal(0, 20, (80, 80, 3)), 0, 255).astype(np.uint8)
    stripes = np.where(((xx // 5 + yy // 7) % 2)[..., None] == 0, [255, 0, 255], [0, 255, 10]).astype(np.uint8)
    uniform = np.broadcast_to(np.array([77, 130, 201], np.uint8), (80, 80, 3)).copy()
    return np.stack([rng.integers(0, 256, size=(80, 80, 3), dtype=np.uint8), smooth, stripes, uniform, np.zeros((80, 80, 3), np.uint8),
                     np.full((80, 80, 3), 255, np.uint8), rng.integers(0, 40, size=(80, 80, 3), dtype=np.uint8)])


def _pair(view_batch, rows, seed=0, mean=T.IMAGENET_MEAN, std=T.IMAGENET_STD):
    tf = T.DeviceStrongWeakPair((84, 84), 80, DEV, mean=mean, std=std)
    assert len(rows) <= 32
    table = torch.from_numpy(np.stack(rows).astype(np.int32))
    strong, weak = tf.strong_weak(torch.from_numpy(np.ascontiguousarray(view_batch)).to(DEV), table, seed)
    assert tuple(strong.shape) == tuple(weak.shape) == (len(rows), 3, 80, 80) and strong.dtype == weak.dtype == torch.float32
    return strong.cpu().numpy(), weak.cpu().numpy()


def _check_exact(view_batch, rows, seed=0, **norm):
    strong, weak = _pair(view_batch, rows, seed, **norm)
    for k, row in enumerate(rows):
        ref_s, ref_w, mask = R.pair(view_batch[k], row, **norm)
        assert np.array_equal(weak[k], ref_w), k
        assert np.array_equal(strong[k][:, ~mask], ref_s[:, ~mask]), (k, np.asarray(row).tolist())
    return strong, weak


LO, HI = 1.4142134, 1.4142135                             # the float32 radii on either side of the box-radius step (test_strong_weak_cpu.py)
ONE = (1.0, 1.0, 1.0)


def _cases_single():
    """Each operation alone, at a factor below 1 (truncating branch) and above 1 (clamped branch); each blur radius class; each flag."""
    rows, src = [], []
    for op in range(3):
        for f in (0.6, 0.73, 1.0, 1.21, 1.4):
            factors = list(ONE)
            factors[op] = f
            rows.append(R.make_row(1, (op, (op + 1) % 3, (op + 2) % 3), factors))
            src.append(len(rows) % 3)
    for radius in (0.1, 0.58, 1.0, LO, HI, 1.7, 2.0):
        rows.append(R.make_row(1, (0, 1, 2), ONE, radius))
        src.append(len(rows) % 3)
    rows += [R.make_row(1, (0, 1, 2), ONE, None, 1, 0), R.make_row(1, (0, 1, 2), ONE, None, 0, 1), R.make_row(1, (0, 1, 2), ONE, None, 1, 1)]
    return rows, src + [0, 1, 2]


def _cases_orders():
    """All 6 orders with every flag on (strong, blur, solarize, gray), at r = 0 and at r = 1, on noise and on the stripes: 24 rows; then each order
    once more with gray off, where the three channels still tell the orders apart: 6 rows."""
    rows, src = [], []
    for order in itertools.permutations(range(3)):
        for radius, factors in ((0.9, (1.3, 0.7, 1.25)), (1.9, (0.65, 1.35, 0.8))):
            for s in (0, 2):
                rows.append(R.make_row(1, order, factors, radius, 1, 1))
                src.append(s)
    for k, order in enumerate(itertools.permutations(range(3))):
        rows.append(R.make_row(1, order, (1.3, 0.7, 1.25), (0.9, 1.9)[k % 2], 1, 0))
        src.append((0, 2)[k // 2 % 2])
    assert all(r[T.SW_STRONG] and r[T.SW_BLUR] and r[T.SW_SOLARIZE] and r[T.SW_GRAY] for r in rows[:24])
    assert {tuple(r[T.SW_ORDER:T.SW_ORDER + 3]) for r in rows[:24]} == set(itertools.permutations(range(3)))
    return rows, src


def _cases_flat():
    """Uniform (the contrast mean equals every pixel's luma), all-0, all-255 and dark views under every operation."""
    rows, src = [], []
    for s in (3, 4, 5, 6):
        for order, factors, radius, sol, gray in (((0, 1, 2), (1.4, 1.4, 1.4), None, 0, 0), ((1, 2, 0), (0.6, 0.6, 0.6), 1.5, 0, 0),
                                                  ((2, 0, 1), (1.0, 1.37, 0.61), 0.3, 1, 0), ((1, 0, 2), (0.99, 1.01, 1.4), 2.0, 1, 1),
                                                  ((2, 1, 0), (1.0, 0.0, 1.0), None, 0, 0)):
            rows.append(R.make_row(1, order, factors, radius, sol, gray))
            src.append(s)
    return rows, src


def _cases_strong_off():
    """Strong flag off: every other column set, none applied."""
    rows = [R.make_row(0, order, (1.4, 0.6, 1.3), 1.8, 1, 1) for order in itertools.permutations(range(3))]
    return rows, [0, 1, 2, 3, 5, 6]


@pytest.mark.parametrize('cases', [_cases_single, _cases_orders, _cases_flat, _cases_strong_off], ids=['single', 'orders', 'flat', 'strong-off'])
def test_strong_weak_bit_exact_against_the_restatement(views, cases):
    rows, src = cases()
    batch = views[src]
    strong, weak = _check_exact(batch, rows)
    if cases is _cases_strong_off:
        assert np.array_equal(strong, weak)
    elif cases is not _cases_flat:                        # (an all-0 or all-255 view survives most operations unchanged)
        assert sum(not np.array_equal(strong[k], weak[k]) for k in range(len(rows))) >= len(rows) // 2


def test_strong_weak_with_the_cifar_statistics_and_drawn_rows(views):
    from fewshot_vit_amd.datasets.folder_datasets import CIFAR_MEAN, CIFAR_STD
    table = T.strong_weak_table(32, torch.Generator().manual_seed(12)).numpy()
    assert table[:, T.SW_STRONG].sum() >= 8 and (table[:, T.SW_ERASE + 2] > 0).sum() >= 3
    _check_exact(views[np.arange(32) % 7], list(table), mean=CIFAR_MEAN, std=CIFAR_STD, seed=5)


def test_erase_is_unit_normal_noise_keyed_by_the_seed(views):
    box = (13, 9, 40, 60)                                 # 40 x 60 x 3 channels: n = 7200 values
    rows = [R.make_row(1, (1, 0, 2), (1.2, 0.8, 1.1), 1.2, 0, 0, erase=box), R.make_row(0, erase=box), R.make_row(0, erase=(0, 0, 79, 79)),
            R.make_row(1, (1, 0, 2), (1.2, 0.8, 1.1), 1.2, 0, 0), R.make_row(0, erase=(79, 79, 1, 1)), R.make_row(0, erase=box)]
    batch = views[[0, 1, 2, 0, 1, 1]]
    strong, weak = _check_exact(batch, rows, seed=1234)                           # outside every box: the un-erased reference, bit for bit
    assert np.array_equal(strong[0][:, ~R.erase_mask(rows[0])], strong[3][:, ~R.erase_mask(rows[0])])
    n = 7200
    for k in (0, 1, 5):
        z = strong[k][:, R.erase_mask(rows[k])].astype(np.float64)
        assert z.size == n
        print(f'erase[{k}]: mean {z.mean():+.4f} (bound {5 / np.sqrt(n):.4f}), var {z.var():.4f} (1 +- {5 * np.sqrt(2 / n):.4f})')
        assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1.0) <= 5 * np.sqrt(2.0 / n)
    assert not np.array_equal(strong[1][:, R.erase_mask(rows[1])], strong[5][:, R.erase_mask(rows[5])])      # the image slot is part of the key
    z = strong[1][:, R.erase_mask(rows[1])]
    assert abs(np.corrcoef(z[0], z[1])[0, 1]) < 5 / np.sqrt(2400) and abs(np.corrcoef(z[0][:-1], z[0][1:])[0, 1]) < 5 / np.sqrt(2400)
    again, _ = _pair(batch, rows, seed=1234)
    assert np.array_equal(again, strong)                                           # same seed: the same batch
    other, _ = _pair(batch, rows, seed=1235)
    m = R.erase_mask(rows[1])
    assert not np.array_equal(other[1][:, m], strong[1][:, m]) and np.array_equal(other[1][:, ~m], strong[1][:, ~m])
    big, _ = _pair(batch, rows, seed=(1 << 63) + 1234)                             # the high seed word is part of the key too
    assert not np.array_equal(big[1][:, m], strong[1][:, m])


def test_argument_errors():
    tf = T.DeviceStrongWeakPair((84, 84), 80, DEV)
    from fewshot_vit_amd import _lib
    from fewshot_vit_amd.engine import _ptr
    lib = _lib.load()
    v = torch.zeros(1, 64, 64, 3, dtype=torch.uint8, device=DEV)
    tab = torch.from_numpy(R.make_row()[None]).to(DEV)
    out = torch.empty(2, 1, 3, 80, 80, device=DEV)
    for H, W, cols in ((64, 64, T.SW_COLS), (80, 84, T.SW_COLS), (80, 80, T.SW_COLS - 1)):
        with pytest.raises(ValueError):
            _lib.check(lib.fsvit_image_strong_weak(_ptr(v), 1, H, W, _ptr(tab), cols, tf.mean, tf.std, 0, _ptr(out[0]), _ptr(out[1]), None))
    with pytest.raises(ValueError):
        tf.strong_weak(v, tab.cpu())
    with pytest.raises(ValueError):
        _lib.check(lib.fsvit_image_transform_rrc_u8(_ptr(v), 64, 64, _ptr(tab), 1, _ptr(tab), _ptr(v), 80, 80, 2, _ptr(v), None))


# ---------------------------------------------------------------- datasets and the distillation driver
def _mini_pickles(path, n_cls, per, seed):
    rng = np.random.default_rng(seed)
    mu = rng.integers(0, 256, size=(n_cls, 1, 84, 84, 3))
    data = np.clip(mu + rng.normal(0, 60, size=(n_cls, per, 84, 84, 3)), 0, 255).astype(np.uint8).reshape(-1, 84, 84, 3)
    for tag in ('train_phase_train', 'val'):
        with open(os.path.join(str(path), f'miniImageNet_category_split_{tag}.pickle'), 'wb') as f:
            pickle.dump({'data': data, 'labels': [64 + i // per for i in range(n_cls * per)]}, f)
    return data


def _check_pair_against_params(strong, weak, data, idx, params, **norm):
    for k, i in enumerate(idx):
        view = R.weak_view(data[i], params['boxes'][k].tolist(), bool(params['flips'][k]))
        ref_s, ref_w, mask = R.pair(view, params['table'][k].numpy(), **norm)
        assert np.array_equal(weak[k], ref_w), k
        assert np.array_equal(strong[k][:, ~mask], ref_s[:, ~mask]), k


def test_dataset_gather_pair_is_reproducible_and_reports_its_params(tmp_path):
    from fewshot_vit_amd import datasets
    from oracle import transform_oracle as to
    data = _mini_pickles(tmp_path, 3, 4, 9)
    make = lambda **kw: datasets.make('mini-imagenet', root_path=str(tmp_path), split='train', **kw)
    a, b = make(augment='strongweak'), make(augment='strongweak')
    idx = torch.tensor([5, 0, 11, 5, 7, 2, 3, 3, 9, 1, 10, 4])
    a.transform.manual_seed(21)
    b.transform.manual_seed(21)
    sa, wa = (x.cpu().numpy() for x in a.gather_pair(idx))
    params = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in a.transform.params.items()}
    assert tuple(params['boxes'].shape) == (12, 4) and tuple(params['flips'].shape) == (12,) and tuple(params['table'].shape) == (12, T.SW_COLS)
    sb, wb = (x.cpu().numpy() for x in b.gather_pair(idx))
    assert np.array_equal(sa, sb) and np.array_equal(wa, wb)                             # same seed, same batch - erase noise included
    sc, wc = (x.cpu().numpy() for x in b.gather_pair(idx))
    assert not np.array_equal(wa, wc) and not np.array_equal(sa, sc)                     # the stream moves on
    sr, wr = (x.cpu().numpy() for x in b.transform(b.device_images(), idx, params=params))
    assert np.array_equal(sa, sr) and np.array_equal(wa, wr)                             # replay from the reported params
    _check_pair_against_params(sa, wa, data, idx.tolist(), params)
    a.transform.manual_seed(33)
    s3, w3, y3 = a[3]
    assert y3 == 0 and tuple(a.transform.params['boxes'].shape) == (1, 4)
    _check_pair_against_params(s3[None].cpu().numpy(), w3[None].cpu().numpy(), data, [3], a.transform.params)
    plain = make()                                                                       # augment=None is unchanged
    assert not hasattr(plain, 'gather_pair')
    assert np.array_equal(plain.gather(idx[:3]).cpu().numpy(), np.stack([to.eval_transform(data[i], 88, 80) for i in idx[:3].tolist()]))
    x, y = plain[3]
    assert y == 0 and np.array_equal(x.cpu().numpy(), to.eval_transform(data[3], 88, 80))


def test_cifar_fs_strongweak_on_32_pixel_sources(tmp_path):
    from PIL import Image
    from fewshot_vit_amd import datasets
    from fewshot_vit_amd.datasets.folder_datasets import CIFAR_MEAN, CIFAR_STD
    rng = np.random.default_rng(2)
    data = rng.integers(0, 256, size=(6, 32, 32, 3), dtype=np.uint8)
    for k, img in enumerate(data):
        os.makedirs(tmp_path / 'meta-train' / f'c{k // 3}', exist_ok=True)
        Image.fromarray(img).save(tmp_path / 'meta-train' / f'c{k // 3}' / f'{k % 3}.png')
    ds = datasets.make('cifar-fs', root_path=str(tmp_path), split='train', augment='strongweak')
    ds.transform.manual_seed(4)
    idx = [5, 0, 3, 3, 1, 2, 4, 0]
    strong, weak = (x.cpu().numpy() for x in ds.gather_pair(torch.tensor(idx)))
    _check_pair_against_params(strong, weak, data, idx, ds.transform.params, mean=CIFAR_MEAN, std=CIFAR_STD)


def test_offline_distills_on_the_view_pair(tmp_path, monkeypatch):
    """Two distill_step iterations of the driver through `_gather` on a `strongweak` dataset: finite losses, and the teacher's batch is not the
    student's."""
    from fewshot_vit_amd import offline
    _mini_pickles(tmp_path, 6, 12, 5)
    config = dict(train_dataset='mini-imagenet', train_dataset_args=dict(root_path=str(tmp_path), split='train', augment='strongweak'),
                  val_dataset='mini-imagenet', val_dataset_args=dict(root_path=str(tmp_path), split='val'),
                  model='token-label', model_args=dict(encoder='visformer_micro_80', encoder_args=dict(drop_path_rate=0.0),
                                                       classifier='linear-classifier', classifier_args=dict(n_classes=6)),
                  synthetic_checkpoint='visformer_micro_80', batch_size=16, train_batches=2, eval_batches=1, max_epoch=1, seed=3,
                  n_way=5, n_shot=1, n_query=2, ep_per_batch=1, tl_soft_k=3, bg_token_num=10, optimizer='adamw',
                  optimizer_args=dict(lr=5e-4, weight_decay=0.05, warmup_lr=1e-6, warmup=1))
    seen, losses = [], []
    inner_gather, inner_step = offline._gather, offline.distill_step

    def gather(dataset, idx, device):
        out = inner_gather(dataset, idx, device)
        seen.append((hasattr(dataset, 'gather_pair'), out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].tolist(), idx.tolist()))
        return out

    def step(*a, **kw):
        out = inner_step(*a, **kw)
        losses.append(float(out[0]))
        return out
    monkeypatch.setattr(offline, '_gather', gather)
    monkeypatch.setattr(offline, 'distill_step', step)
    trlog = offline.main(config, name='sw', device=DEV, log=lambda *_: None, save_root=str(tmp_path))
    assert len(losses) == 2 and np.isfinite(losses).all() and np.isfinite(trlog['tl']).all()
    assert len(seen) == 2
    for paired, strong, weak, label, idx in seen:
        assert paired and strong.shape == weak.shape == (16, 3, 80, 80) and label == [i // 12 for i in idx]
        assert np.isfinite(strong).all() and not np.array_equal(strong, weak)
    assert not np.array_equal(seen[0][2], seen[1][2])
