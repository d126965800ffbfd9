"""CPU checks of the distillation phase's strong / weak view pair (sun_meta_training/datasets/mini_imagenet.py:91-124, :194-204): the numpy
restatement the GPU tests compare the kernels with (tests/augment_ref.py) equals live Pillow and the committed Pillow vectors
(tests/golden/strong_weak_pil.npz) bit for bit, the host-side parameter draw follows the reference's distributions, and the datasets accept
`augment='strongweak'` without a GPU."""
import itertools
import math
import os
import pickle

import numpy as np
import pytest
import torch

import augment_ref as R
from fewshot_vit_amd.datasets import transforms as T


@pytest.fixture(scope='module')
def images():
    """Four 80 x 80 x 3 views: uniform noise, smooth + noise, saturating stripes, and a dark low-contrast one."""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:80, 0:80]
    smooth = np.clip(np.stack([yy * 3, xx * 3, (yy + xx) * 1.5], -1) + rng.normal(0, 20, (80, 80, 3)), 0, 255).astype(np.uint8)
    stripes = np.where(((xx // 5 + yy // 7) % 2)[..., None] == 0, [255, 0, 255], [0, 255, 10]).astype(np.uint8)
    dark = rng.integers(0, 40, size=(80, 80, 3), dtype=np.uint8)
    return [rng.integers(0, 256, size=(80, 80, 3), dtype=np.uint8), smooth, stripes, dark]


def _f32_neighbours_of_the_radius_step():
    """The two adjacent float32 radii between which Pillow's integer box radius steps from 0 to 1 (12 * rho^2 / 3 + 1 = 9: rho = sqrt 2)."""
    lo, hi = np.float32(1.0), np.float32(2.0)
    assert T.gaussian_blur_box(lo)[0] == 0 and T.gaussian_blur_box(hi)[0] == 1
    while np.nextafter(lo, np.float32(3)) < hi:
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        if T.gaussian_blur_box(mid)[0] == 0:
            lo = mid
        else:
            hi = mid
    return float(lo), float(hi)


def test_radius_step_is_at_sqrt2():
    lo, hi = _f32_neighbours_of_the_radius_step()
    assert abs(lo - math.sqrt(2.0)) < 2.5e-7 and abs(hi - math.sqrt(2.0)) < 2.5e-7          # within two float32 steps (1.2e-7 each) of sqrt 2
    assert np.nextafter(np.float32(lo), np.float32(3)) == np.float32(hi)
    r, ww, fw = T.gaussian_blur_box([0.1, 0.58, lo, hi, 2.0])
    assert r.tolist() == [0, 0, 0, 1, 1]
    assert bool(((2 * r + 1) * ww + 2 * fw <= (1 << 24)).all()) and bool((fw >= 0).all()) and bool((ww >= 1).all())


# ---------------------------------------------------------------- the restatement against live Pillow
try:
    from PIL import Image, ImageEnhance, ImageFilter, ImageOps
except ImportError:                                                   # the golden tests below still run
    Image = None
needs_pillow = pytest.mark.skipif(Image is None, reason='Pillow is not installed: tests/golden/strong_weak_pil.npz pins the restatement instead')

FACTORS = [0.6, 1.0, 1.4, 0.0, 0.73, 0.999, 1.21, float(np.float32(0.6)), float(np.float32(1.4))]


@needs_pillow
@pytest.mark.parametrize('op', [T.OP_BRIGHTNESS, T.OP_CONTRAST, T.OP_SATURATION], ids=['brightness', 'contrast', 'saturation'])
def test_colour_operations_equal_pillow(images, op):
    enhance = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)[op]
    for k, img in enumerate(images):
        for f in FACTORS:
            assert np.array_equal(R.COLOUR_OPS[op](img, f), np.asarray(enhance(Image.fromarray(img)).enhance(f))), (k, f)


@needs_pillow
def test_blur_equals_pillow(images):
    lo, hi = _f32_neighbours_of_the_radius_step()
    for k, img in enumerate(images):
        for radius in (0.1, 0.58, 1.0, lo, hi, 1.7, 2.0):
            assert np.array_equal(R.gaussian_blur(img, radius), np.asarray(Image.fromarray(img).filter(ImageFilter.GaussianBlur(radius)))), (k, radius)


@needs_pillow
def test_solarize_and_grayscale_equal_pillow(images):
    for img in images:
        im = Image.fromarray(img)
        assert np.array_equal(R.solarize(img), np.asarray(ImageOps.solarize(im)))
        L = np.asarray(im.convert('L'))
        assert np.array_equal(R.luma(img), L) and np.array_equal(R.grayscale(img), np.dstack([L, L, L]))


@needs_pillow
def test_bicubic_crop_resize_equals_pillow_at_every_width():
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, size=(84, 84, 3), dtype=np.uint8)
    src[:, 40:60] = np.where((np.arange(20) // 2 % 2)[None, :, None] == 0, 255, 0)          # saturating stripes: overshoot beyond 0..255
    clipped = 0
    for w in range(1, 85):                                            # every crop width once, the height running the other way
        h = 85 - w
        box = ((0, 84 - h)[w % 2], (0, 84 - w)[(w // 2) % 2], h, w)
        ref = np.asarray(Image.fromarray(src).crop((box[1], box[0], box[1] + w, box[0] + h)).resize((80, 80), Image.BICUBIC))
        got = R.weak_view(src, box, 0)
        assert np.array_equal(got, ref), box
        clipped += int((got == 0).sum() + (got == 255).sum())
    assert clipped > 1000
    src32 = rng.integers(0, 256, size=(32, 32, 3), dtype=np.uint8)
    for w in range(1, 33):
        box = (0, 32 - w, 33 - w, w)
        ref = np.asarray(Image.fromarray(src32).crop((box[1], 0, 32, box[2])).resize((80, 80), Image.BICUBIC).transpose(Image.FLIP_LEFT_RIGHT))
        assert np.array_equal(R.weak_view(src32, box, 1), ref), box


def test_bilinear_tables_are_unchanged():
    from oracle import transform_oracle as to
    for n in (1, 5, 32, 79, 80, 84, 100, 200):
        for a, b in zip(T.pil_bilinear_tables(n, 80), to.bilinear_coeffs(n, 80)):
            assert np.array_equal(a, b), n
        for a, b in zip(T.pil_bilinear_tables(n, 80), T.pil_resample_tables(n, 80, 'bilinear')):
            assert np.array_equal(a, b), n
    xmin, cnt, coef = T.pil_resample_tables(84, 80, 'bicubic')
    assert coef.shape == (80, 7) and int(coef.min()) < 0 and bool((coef.sum(1) - (1 << 22)).__abs__().max() <= 4)


# ---------------------------------------------------------------- the restatement against the committed Pillow vectors
def test_restatement_equals_the_committed_pillow_vectors(golden_dir):
    path = os.path.join(golden_dir, 'strong_weak_pil.npz')
    z = np.load(path)
    base = np.load(os.path.join(golden_dir, 'transform_pil.npz'))['images']
    assert 10 <= len(z['weak']) <= 16 and os.path.getsize(path) < 256 * 1024
    assert set(map(tuple, z['case_order'].tolist())) == set(itertools.permutations(range(3)))
    for k in range(len(z['weak'])):
        radius = float(z['case_radius'][k])
        row = R.make_row(1, z['case_order'][k], z['case_factors'][k], radius if radius else None, int(z['case_solarize'][k]), int(z['case_gray'][k]))
        weak = R.weak_view(base[z['case_source'][k]], z['case_box'][k], int(z['case_flip'][k]))
        assert np.array_equal(weak, z['weak'][k]), k
        assert np.array_equal(R.strong_u8(weak, row), z['strong'][k]), k
        off = row.copy()
        off[T.SW_STRONG] = 0
        assert R.strong_u8(weak, off) is weak


# ---------------------------------------------------------------- the parameter draw
def _within_5_sigma(count, n, p):
    return abs(count - n * p) <= 5.0 * math.sqrt(n * p * (1.0 - p))           # binomial standard deviation


def test_parameter_draw_follows_the_reference_distribution():
    n = 60000
    tab = T.strong_weak_table(n, torch.Generator().manual_seed(3))
    assert tab.dtype == torch.int32 and tuple(tab.shape) == (n, T.SW_COLS) and tab.is_contiguous()
    assert torch.equal(tab, T.strong_weak_table(n, torch.Generator().manual_seed(3)))
    assert not torch.equal(tab, T.strong_weak_table(n, torch.Generator().manual_seed(4)))
    assert T._checked_table(n, tab, 80) is not None                   # every drawn row passes the host validation
    order = tab[:, T.SW_ORDER:T.SW_ORDER + 3].tolist()
    counts = {p: 0 for p in itertools.permutations(range(3))}
    for o in order:
        counts[tuple(o)] += 1                                          # KeyError if a row is no permutation
    for p, c in counts.items():
        assert _within_5_sigma(c, n, 1.0 / 6.0), (p, c)
    for col, p in ((T.SW_STRONG, 0.5), (T.SW_BLUR, 0.5), (T.SW_SOLARIZE, 0.5), (T.SW_GRAY, 0.2)):
        flag = tab[:, col]
        assert bool(((flag == 0) | (flag == 1)).all())
        assert _within_5_sigma(int(flag.sum()), n, p), (col, int(flag.sum()))
    f = tab[:, T.SW_FACTOR:T.SW_FACTOR + 3].contiguous().view(torch.float32)
    assert float(f.min()) >= 0.6 and float(f.max()) <= 1.4 and float(f.min()) < 0.601 and float(f.max()) > 1.399
    assert bool((f.mean(0) - 1.0).abs().max() < 5 * 0.8 / math.sqrt(12 * n))                 # U(0.6, 1.4): sigma = 0.8 / sqrt 12
    r, ww, fw = (tab[:, c].long() for c in (T.SW_R, T.SW_WW, T.SW_FW))
    assert set(r.tolist()) == {0, 1}
    assert _within_5_sigma(int(r.sum()), n, (2.0 - math.sqrt(2.0)) / 1.9)                   # radius U(0.1, 2): r = 1 from sqrt 2
    assert bool((fw == ((1 << 24) - (2 * r + 1) * ww) // 2).all()) and bool((fw >= 0).all())
    top, left, h, w = tab[:, T.SW_ERASE:T.SW_ERASE + 4].long().unbind(1)
    on = h > 0
    assert _within_5_sigma(int(on.sum()), n, 0.25), int(on.sum())     # every attempt set holds an accepted one at these ranges, or nearly: see below
    assert bool(((h == 0) == (w == 0)).all()) and bool((tab[~on][:, T.SW_ERASE:] == 0).all())
    h, w, top, left = h[on], w[on], top[on], left[on]
    assert bool(((h < 80) & (w < 80) & (top >= 0) & (left >= 0) & (top + h <= 80) & (left + w <= 80)).all())
    area, ratio = (h * w).double(), h.double() / w.double()
    assert float(area.min()) < 0.03 * 6400 and float(area.max()) > 0.3 * 6400 and bool((area <= (math.sqrt(6400 / 3.) + 1) ** 2 * 1.2).all())
    assert float(ratio.min()) < 0.4 and float(ratio.max()) > 2.5
    assert int(top.min()) == 0 and int(left.min()) == 0 and int((top + h).max()) == 80 and int((left + w).max()) == 80


def test_erase_boxes_are_refused_only_when_ten_attempts_fail():
    """P(one attempt has h >= 80 or w >= 80) needs area * ratio >= 6400 with area <= 6400 / 3 and ratio <= 1 / 0.3: under 2 % per attempt, so ten
    failures in a row are below 1e-17 and the erase rate is the apply probability."""
    box = T.random_erase_boxes(20000, 80, 80, torch.Generator().manual_seed(0), prob=1.0)
    assert bool((box[:, 2] > 0).all())
    assert bool((T.random_erase_boxes(100, 80, 80, torch.Generator().manual_seed(0), prob=0.0) == 0).all())


def test_explicit_parameters_are_validated_on_the_host():
    tf = T.DeviceStrongWeakPair((84, 84), 80, 'cpu')
    images = torch.zeros(2, 84, 84, 3, dtype=torch.uint8)              # a CPU tensor: a call that got past the checks raises RuntimeError
    index = torch.tensor([0, 1])
    good = tf.draw(2)

    def with_cell(col, value):
        p = dict(good, table=good['table'].clone())
        p['table'][1, col] = value
        return p
    bad = [with_cell(T.SW_STRONG, 2), with_cell(T.SW_ORDER, 3), with_cell(T.SW_ORDER + 1, int(good['table'][1, T.SW_ORDER])),
           with_cell(T.SW_FACTOR, int(np.float32(-0.5).view(np.int32))), with_cell(T.SW_FACTOR + 2, int(np.float32(np.nan).view(np.int32))),
           with_cell(T.SW_R, 4), with_cell(T.SW_WW, 0), with_cell(T.SW_FW, int(good['table'][1, T.SW_FW]) + 1), with_cell(T.SW_GRAY, -1),
           dict(good, table=good['table'][:1]), dict(good, table=good['table'].long()), dict(good, table=good['table'][:, :-1]),
           dict(good, boxes=torch.tensor([[0, 0, 84, 84], [1, 0, 84, 84]])), dict(good, seed=-1)]
    for col, vals in ((T.SW_ERASE, (70, 0, 20, 5)), (T.SW_ERASE, (0, 0, 0, 5)), (T.SW_ERASE, (0, -1, 5, 5)), (T.SW_ERASE, (0, 0, 5, 81))):
        p = dict(good, table=good['table'].clone())
        p['table'][0, col:col + 4] = torch.tensor(vals, dtype=torch.int32)
        bad.append(p)
    for p in bad:
        with pytest.raises(ValueError):
            tf(images, index, params=p)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        tf(images, index, params=good)
    views = torch.zeros(2, 80, 80, 3, dtype=torch.uint8)
    for seed in (-1, 1 << 64):                                         # the helper checks its seed like the call does
        with pytest.raises(ValueError):
            tf.strong_weak(views, good['table'], seed)
    with pytest.raises(ValueError):
        tf.crop_u8(images, index, torch.tensor([[0, 0, 84, 84], [1, 0, 84, 84]]), good['flips'])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        tf.strong_weak(views, good['table'], (1 << 64) - 1)
    with pytest.raises(NotImplementedError):
        T.DeviceStrongWeakPair((84, 84), 64, 'cpu')


def test_datasets_accept_strongweak_without_a_gpu(tmp_path):
    from fewshot_vit_amd import datasets
    rng = np.random.default_rng(0)
    data = rng.integers(0, 256, size=(12, 84, 84, 3), dtype=np.uint8)
    labels = [i // 3 for i in range(12)]
    with open(tmp_path / 'miniImageNet_category_split_train_phase_train.pickle', 'wb') as f:
        pickle.dump({'data': data, 'labels': labels}, f)
    np.savez(tmp_path / 'train_images.npz', images=data)
    with open(tmp_path / 'train_labels.pkl', 'wb') as f:
        pickle.dump({'labels': labels}, f)
    for name in ('mini-imagenet', 'tiered-imagenet'):
        ds = datasets.make(name, root_path=str(tmp_path), device='cpu', split='train', augment='strongweak')
        assert isinstance(ds.transform, T.DeviceStrongWeakPair) and (ds.transform.H, ds.transform.W, ds.transform.out) == (84, 84, 80)
        assert isinstance(ds.default_transform, T.DeviceTransform) and hasattr(ds, 'gather_pair')
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            ds.gather_pair(torch.tensor([0, 1]))
        plain = datasets.make(name, root_path=str(tmp_path), device='cpu', split='train')
        assert isinstance(plain.transform, T.DeviceTransform) and not hasattr(plain, 'gather_pair')
        assert ds.transform.strong_prob == 0.5                         # the reference's constructor default; the argument is forwarded
        assert datasets.make(name, root_path=str(tmp_path), device='cpu', split='train', augment='strongweak', strong_prob=0.8).transform.strong_prob == 0.8
        pair, ds.transform = ds.transform, ds.default_transform        # gather_pair follows a replaced transform, both ways
        assert not hasattr(ds, 'gather_pair')
        ds.transform = pair
        assert hasattr(ds, 'gather_pair')
    tab = datasets.make('mini-imagenet', root_path=str(tmp_path), device='cpu', split='train', augment='strongweak', strong_prob=0.8).transform.draw(20000)['table']
    assert _within_5_sigma(int(tab[:, T.SW_STRONG].sum()), 20000, 0.8)


@needs_pillow
def test_cifar_fs_accepts_strongweak_without_a_gpu(tmp_path):
    from fewshot_vit_amd import datasets
    from fewshot_vit_amd.datasets.folder_datasets import CIFAR_MEAN
    rng = np.random.default_rng(0)
    for c in range(2):
        os.makedirs(tmp_path / 'meta-train' / f'c{c}')
        for k in range(3):
            Image.fromarray(rng.integers(0, 256, size=(32, 32, 3), dtype=np.uint8)).save(tmp_path / 'meta-train' / f'c{c}' / f'{k}.png')
    sw = datasets.make('cifar-fs', root_path=str(tmp_path), device='cpu', split='train', augment='strongweak')
    assert isinstance(sw.transform, T.DeviceStrongWeakPair) and (sw.transform.H, sw.transform.W) == (32, 32)
    assert list(sw.transform.mean) == pytest.approx(list(CIFAR_MEAN)) and sw.transform.strong_prob == 0.5 and hasattr(sw, 'gather_pair')
    assert datasets.make('cifar-fs', root_path=str(tmp_path), device='cpu', split='train', augment='strongweak', strong_prob=0.25).transform.strong_prob == 0.25
    for aug in ('resize', 'cropaug'):                                   # 'resize' on cifar-fs stays refused (tests/test_folder_datasets_cpu.py holds it)
        with pytest.raises(NotImplementedError):
            datasets.make('cifar-fs', root_path=str(tmp_path), device='cpu', split='train', augment=aug)
