"""CPU checks of RandAugment on the GPU data path (the weak view's RandomApply([RandAugment], p = 0.2) of the distillation phase and the
classifier phase's timm pipeline): the numpy restatement the GPU tests compare the kernel with (tests/randaug_ref.py) equals live Pillow and the
committed Pillow vectors (tests/golden/randaug_pil.npz) bit for bit, the host-side draw follows timm's published distribution, every refusal of
the host validation, and the datasets accept `augment='randaug'` / `weak_randaug` without a GPU.  No tolerance anywhere: the operations are
integer or uncontracted IEEE arithmetic."""
import math
import os
import pickle

import numpy as np
import pytest
import torch

import randaug_ref as R
from fewshot_vit_amd.datasets import transforms as T

try:
    from PIL import Image
except ImportError:                                                   # the golden test below still runs
    Image = None
needs_pillow = pytest.mark.skipif(Image is None, reason='Pillow is not installed: tests/golden/randaug_pil.npz pins the restatement instead')

MAGNITUDES = (0, 4.3, 9, 10)


@pytest.fixture(scope='module')
def sources():
    return R.sources()


def _op(name, m, neg, size=80):
    return T.rand_augment_op(name, m, neg, size)


# ---------------------------------------------------------------- the restatement against live Pillow
@needs_pillow
@pytest.mark.parametrize('name', T.RAND_INCREASING_OPS)
def test_every_operation_equals_pillow(sources, name):
    """Each operation at m in {0, 4.3, 9, 10} and both signs, on every source (Posterize reaches 0 bits at m = 10, Rotate is a no-op at m = 0)."""
    changed = 0
    for key, img in sources.items():
        for m in MAGNITUDES:
            for neg in (False, True):
                got, ref = R.apply_op(img, _op(name, m, neg)), R.timm_op_pil(img, name, m, neg)
                assert np.array_equal(got, ref), (key, m, neg, int((got != ref).sum()))
                changed += not np.array_equal(got, img)
    assert changed >= 8, changed                                       # the operation does something


@needs_pillow
def test_rotation_and_fractional_translation_equal_pillow(sources):
    img = sources['stripes']
    for deg in (17.3, -27.0, 30.0, -0.5, 3.0, 360.0, 0.0):
        coef = T.rotate_matrix(deg, 80, 80)
        ref = np.asarray(Image.fromarray(img).rotate(deg, resample=Image.BICUBIC, fillcolor=T.RA_FILL))
        got = img if coef is None else R.affine(img, coef, T.RA_FILL)
        assert (coef is None) == (deg % 360 == 0) and np.array_equal(got, ref), deg
    for coef in ((1, 0, 12.37, 0, 1, 0), (1, 0, 0, 0, 1, -30.61), (1, 0.17, -3.3, -0.08, 1, 4.9), (1, 0, 0.5, 0, 1, 0.5), (1, 0, -79.4, 0, 1, 79.4)):
        ref = np.asarray(Image.fromarray(img).transform((80, 80), Image.AFFINE, coef, Image.BICUBIC, fillcolor=T.RA_FILL))
        assert np.array_equal(R.affine(img, coef, T.RA_FILL), ref), coef


@needs_pillow
def test_bicubic_overshoot_reaches_both_clamps_on_the_stripes(sources):
    img = sources['stripes']
    band = np.zeros((80, 80), bool)
    band[20:60, 32:56] = True                                          # well inside the band of 0 / 255 stripes
    for name, m, neg in (('Rotate', 9, False), ('ShearX', 10, True), ('TranslateXRel', 4.3, False)):
        got = R.apply_op(img, _op(name, m, neg))
        assert np.array_equal(got, R.timm_op_pil(img, name, m, neg))
        assert (got == 0).any() and (got == 255).any()
    coef = (1, 0, 0.5, 0, 1, 0)                                        # half a pixel: every band pixel sits between a 0 and a 255 or inside a pair
    v = R.affine(img, coef, T.RA_FILL)[band]
    assert (v == 0).any() and (v == 255).any() and ((v > 0) & (v < 255)).any()


@needs_pillow
def test_histogram_operations_on_their_edge_cases(sources):
    from PIL import ImageOps
    const, narrow, bright = sources['constant'], sources['narrow'], sources['bright']
    for name in ('AutoContrast', 'Equalize'):                          # a constant image: left as it is
        assert np.array_equal(R.apply_op(const, _op(name, 9, False)), const)
        assert np.array_equal(R.timm_op_pil(const, name, 9, False), const)
    luts = [R.equalize_table_unclamped(np.bincount(narrow[..., c].ravel(), minlength=256)) for c in range(3)]
    assert all(int(l.max()) > 255 for l in luts), [int(l.max()) for l in luts]      # Pillow clamps; a uint8 wrap would be wrong
    got = R.equalize(narrow)
    assert np.array_equal(got, np.asarray(ImageOps.equalize(Image.fromarray(narrow)))) and int(got.max()) == 255
    assert [int((bright[..., c] == 255).sum()) for c in range(3)] == [6300] * 3
    assert R.equalize_table_unclamped(np.bincount(bright[..., 0].ravel(), minlength=256)) is None                # step == 0
    assert np.array_equal(R.equalize(bright), bright) and np.array_equal(np.asarray(ImageOps.equalize(Image.fromarray(bright))), bright)
    assert not np.array_equal(R.autocontrast(narrow), narrow)
    zero_bits = _op('PosterizeIncreasing', 10, False)
    assert zero_bits[T.RA_CODE] == T.RA_POSTERIZE and zero_bits[T.RA_ARG] == 0
    assert not R.apply_op(narrow, zero_bits).any() and not R.timm_op_pil(narrow, 'PosterizeIncreasing', 10, False).any()


# ---------------------------------------------------------------- the restatement against the committed Pillow vectors
def test_restatement_equals_the_committed_pillow_vectors(golden_dir):
    path = os.path.join(golden_dir, 'randaug_pil.npz')
    assert os.path.getsize(path) < 512 * 1024
    z = np.load(path)
    src, out = z['sources'], z['outputs']
    size = src.shape[1]
    n_signed = len(T.RA_SIGNED)
    assert out.shape[:2] == (2, len(T.RAND_INCREASING_OPS) + n_signed + 4)
    singles = [(int(o[0]), bool(g[0])) for o, g in zip(z['case_op'], z['case_negate']) if o[1] < 0]
    assert sorted(singles) == sorted([(k, False) for k in range(15)] + [(k, True) for k, n in enumerate(T.RAND_INCREASING_OPS) if n in T.RA_SIGNED])
    assert int((z['case_op'][:, 1] >= 0).sum()) == 4
    for s in range(2):
        for k in range(out.shape[1]):
            img = src[s]
            for j in range(2):
                if z['case_op'][k, j] >= 0:
                    img = R.apply_op(img, T.rand_augment_op(T.RAND_INCREASING_OPS[z['case_op'][k, j]], float(z['case_magnitude'][k, j]),
                                                            bool(z['case_negate'][k, j]), size))
            assert np.array_equal(img, out[s, k]), (s, k, z['case_op'][k].tolist())


# ---------------------------------------------------------------- the draw
def _within_5_sigma(count, n, p):
    return abs(count - n * p) <= 5.0 * math.sqrt(n * p * (1.0 - p))           # binomial standard deviation


def test_draw_follows_timms_distribution():
    n = 20000
    for apply_prob in (0.2, 1.0):
        d = T.rand_augment_draw(n, torch.Generator().manual_seed(5), apply_prob)
        assert _within_5_sigma(int(d['apply'].sum()), n, apply_prob) if apply_prob < 1 else bool(d['apply'].all())
    op, on, neg, raw, mag = d['op'], d['on'], d['negate'], d['raw'], d['magnitude']
    assert tuple(op.shape) == tuple(on.shape) == tuple(neg.shape) == tuple(raw.shape) == (n, 2)
    for layer in range(2):
        counts = torch.bincount(op[:, layer], minlength=15)
        assert counts.numel() == 15
        for k in range(15):
            assert _within_5_sigma(int(counts[k]), n, 1.0 / 15.0), (layer, k, int(counts[k]))
        assert _within_5_sigma(int(on[:, layer].sum()), n, 0.5) and _within_5_sigma(int(neg[:, layer].sum()), n, 0.5)
    assert _within_5_sigma(int((op[:, 0] == op[:, 1]).sum()), n, 1.0 / 15.0)            # with replacement
    assert _within_5_sigma(int((on[:, 0] & on[:, 1]).sum()), n, 0.25)                   # each operation on its own coin
    r = raw.flatten().double()                                                          # 2n draws of N(9, 0.5)
    assert abs(float(r.mean()) - 9.0) <= 5 * 0.5 / math.sqrt(2 * n)
    assert abs(float(r.var()) - 0.25) <= 5 * 0.25 * math.sqrt(2.0 / (2 * n))            # sd of a normal sample variance: sigma^2 sqrt(2 / N)
    assert float(mag.min()) >= 0.0 and float(mag.max()) == 10.0 and torch.equal(mag, raw.clamp(0, 10))
    assert _within_5_sigma(int((mag == 10.0).sum()), 2 * n, 0.5 * math.erfc(2.0 / math.sqrt(2.0)))               # P(N(9, 0.5) > 10) = P(Z > 2)
    wide = T.rand_augment_draw(2000, torch.Generator().manual_seed(1), 1.0, magnitude=1, magnitude_std=3)
    assert float(wide['magnitude'].min()) == 0.0 and float(wide['magnitude'].max()) == 10.0 and float(wide['raw'].min()) < 0


def test_table_is_the_draw_mapped_through_timms_levels():
    n = 20000
    slots, table = T.rand_augment_table(n, torch.Generator().manual_seed(5), 1.0)
    d = T.rand_augment_draw(n, torch.Generator().manual_seed(5), 1.0)
    again = T.rand_augment_table(n, torch.Generator().manual_seed(5), 1.0)
    assert torch.equal(slots, again[0]) and torch.equal(table, again[1])
    assert slots.dtype == table.dtype == torch.int32 and tuple(table.shape) == (slots.numel(), T.RA_COLS)
    assert torch.equal(slots.long(), d['on'].any(1).nonzero()[:, 0])                    # the images with at least one applied operation
    assert _within_5_sigma(slots.numel(), n, 0.75)
    assert T._checked_randaug(n, slots, table) is not None                              # every drawn row passes the host validation
    ops = table.view(-1, T.RA_OP_COLS).numpy()
    on = d['on'][slots.long()].flatten().numpy()
    assert bool((ops[~on] == 0).all()) and np.array_equal(ops[:, T.RA_CODE] != T.RA_NONE, on)      # N(9, 0.5) never draws the Rotate no-op m = 0
    name = np.asarray(T.RAND_INCREASING_OPS)[d['op'][slots.long()].flatten().numpy()]
    mag, neg = d['magnitude'][slots.long()].flatten().numpy(), d['negate'][slots.long()].flatten().numpy()
    for k in np.flatnonzero(on)[:3000]:
        assert np.array_equal(ops[k], T.rand_augment_op(name[k], mag[k], neg[k])), (k, name[k])
    factor = ops[:, T.RA_ARG].copy().view(np.float32)[on & np.isin(ops[:, T.RA_CODE], (T.RA_COLOR, T.RA_CONTRAST, T.RA_BRIGHTNESS, T.RA_SHARPNESS))]
    assert float(factor.min()) == np.float32(0.1) and 1.8 < float(factor.max()) <= 1.9
    few, _ = T.rand_augment_table(n, torch.Generator().manual_seed(6), 0.2)
    assert _within_5_sigma(few.numel(), n, 0.2 * 0.75)
    none = T.rand_augment_table(64, torch.Generator().manual_seed(6), 0.0)
    assert none[0].numel() == 0 and tuple(none[1].shape) == (0, T.RA_COLS)


def test_level_maps():
    f = lambda op: float(op[T.RA_ARG:T.RA_ARG + 1].view(np.float32)[0])
    c = lambda op: op[T.RA_COEF:T.RA_COEF + 12].view(np.float64).tolist()
    assert T.RA_FILL == (124, 116, 104) and T.fill_colour((0.5071, 0.4866, 0.4409)) == (129, 124, 112)
    assert [int(_op('PosterizeIncreasing', m, False)[T.RA_ARG]) for m in (0, 4.3, 9, 10)] == [4, 3, 1, 0]
    assert [int(_op('SolarizeIncreasing', m, False)[T.RA_ARG]) for m in (0, 4.3, 9, 10)] == [256, 146, 26, 0]
    assert [int(_op('SolarizeAdd', m, False)[T.RA_ARG]) for m in (0, 4.3, 9, 10)] == [0, 47, 99, 110]
    assert f(_op('ColorIncreasing', 9, False)) == np.float32(1.81) and f(_op('SharpnessIncreasing', 10, True)) == np.float32(0.1)
    assert f(_op('ContrastIncreasing', 0, True)) == 1.0 and f(_op('BrightnessIncreasing', 4.3, True)) == np.float32(1 - 0.43 * 0.9)
    assert c(_op('ShearX', 10, True)) == [1, -0.3, 0, 0, 1, 0] and c(_op('ShearY', 10, False)) == [1, 0, 0, 0.3, 1, 0]
    assert c(_op('TranslateXRel', 10, False)) == [1, 0, 36.0, 0, 1, 0] and c(_op('TranslateYRel', 5, True)) == [1, 0, 0, 0, 1, -0.225 * 80]
    assert _op('Rotate', 0, True)[T.RA_CODE] == T.RA_NONE and _op('Rotate', 9, True)[T.RA_CODE] == T.RA_AFFINE
    assert c(_op('Rotate', 9, True)) == list(T.rotate_matrix(-27.0, 80, 80))
    with pytest.raises(ValueError):
        T.rand_augment_op('Hue', 9)
    with pytest.raises(NotImplementedError):
        T.rand_augment_table(4, torch.Generator(), 1.0, num_layers=3)


# ---------------------------------------------------------------- host validation
def test_explicit_randaug_parameters_are_validated_on_the_host():
    tf = T.DeviceStrongWeakPair((84, 84), 80, 'cpu', weak_randaug=1.0)
    images = torch.zeros(4, 84, 84, 3, dtype=torch.uint8)              # a CPU tensor: a call that got past the checks raises RuntimeError
    index = torch.arange(4)
    good = tf.draw(4)
    row = lambda *ops: torch.from_numpy(np.concatenate(ops))[None]
    slots = torch.tensor([1, 3], dtype=torch.int32)
    table = torch.cat([row(_op('Rotate', 9, False), _op('Equalize', 9, False)), row(_op('PosterizeIncreasing', 9, False), _op('ColorIncreasing', 9, True))])
    good['randaug'] = (slots, table)

    sol = torch.cat([table[:1], row(_op('SolarizeIncreasing', 0, False), _op('SolarizeAdd', 9, False))])

    def with_cell(r, col, value, base=table):
        t = base.clone()
        t[r, col] = value
        return dict(good, randaug=(slots, t))
    f32 = lambda v: int(np.float32(v).view(np.int32))
    hi_word = lambda v: int(np.asarray([v], np.float64).view(np.int32)[1])
    bad = [with_cell(0, T.RA_CODE, 12), with_cell(0, T.RA_CODE, -1), with_cell(0, T.RA_COEF + 1, hi_word(np.nan)),
           with_cell(0, T.RA_COEF + 11, hi_word(np.inf)), with_cell(1, T.RA_ARG, 9), with_cell(1, T.RA_ARG, -1),
           with_cell(1, T.RA_OP_COLS + T.RA_ARG, f32(-0.5)), with_cell(1, T.RA_OP_COLS + T.RA_ARG, f32(np.nan)),
           with_cell(1, T.RA_OP_COLS + T.RA_ARG, f32(np.inf)), with_cell(1, T.RA_ARG, 257, sol), with_cell(1, T.RA_ARG, -1, sol),
           with_cell(1, T.RA_OP_COLS + T.RA_ARG, 256, sol), with_cell(1, T.RA_OP_COLS + T.RA_ARG, -1, sol),
           dict(good, randaug=(slots, table[:1])), dict(good, randaug=(slots, table.long())), dict(good, randaug=(slots, table[:, :-1])),
           dict(good, randaug=(slots.long(), table)), dict(good, randaug=(slots[None], table)),
           dict(good, randaug=(torch.tensor([3, 1], dtype=torch.int32), table)), dict(good, randaug=(torch.tensor([1, 1], dtype=torch.int32), table)),
           dict(good, randaug=(torch.tensor([1, 4], dtype=torch.int32), table)), dict(good, randaug=(torch.tensor([-1, 2], dtype=torch.int32), table))]
    for k, p in enumerate(bad):
        with pytest.raises(ValueError):
            tf(images, index, params=p)
            pytest.fail(f'case {k} was accepted')
    for p in (good, dict(good, randaug=(slots[:0], table[:0])), with_cell(1, T.RA_ARG, 0), with_cell(1, T.RA_ARG, 8), with_cell(0, 0, 0, sol)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            tf(images, index, params=p)
    views = torch.zeros(4, 80, 80, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        tf.rand_augment(views, torch.tensor([1, 4], dtype=torch.int32), table)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        tf.rand_augment(views, slots, table)
    with pytest.raises(ValueError):
        T.DeviceStrongWeakPair((84, 84), 80, 'cpu', weak_randaug=1.5)
    crop = T.DeviceRandAugCrop((84, 84), 80, 'cpu')
    with pytest.raises(ValueError):
        crop(images, index, params={k: v for k, v in crop.draw(4).items() if k != 'randaug'})
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        crop(images, index)
    with pytest.raises(NotImplementedError):
        T.DeviceRandAugCrop((84, 84), 64, 'cpu')


def test_weak_randaug_zero_leaves_the_stream_unchanged():
    plain, zero = T.DeviceStrongWeakPair((84, 84), 80, 'cpu', seed=9), T.DeviceStrongWeakPair((84, 84), 80, 'cpu', seed=9, weak_randaug=0.0)
    on = T.DeviceStrongWeakPair((84, 84), 80, 'cpu', seed=9, weak_randaug=0.2)
    for _ in range(2):                                                 # the second draw too: nothing extra was consumed
        a, b = plain.draw(64), zero.draw(64)
        assert list(a) == list(b) == ['boxes', 'flips', 'table', 'seed']
        assert all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in a)
    c = on.draw(64)
    first = T.DeviceStrongWeakPair((84, 84), 80, 'cpu', seed=9).draw(64)
    assert list(c) == ['boxes', 'flips', 'table', 'seed', 'randaug']   # drawn after the others: they are the ones a plain pair draws
    assert all(torch.equal(c[k], first[k]) if torch.is_tensor(c[k]) else c[k] == first[k] for k in first)
    crop = T.DeviceRandAugCrop((84, 84), 80, 'cpu', seed=9).draw(64)
    assert not crop['table'][:, T.SW_STRONG].any() and torch.equal(crop['boxes'], first['boxes'])
    assert _within_5_sigma(crop['randaug'][0].numel(), 64, 0.75)


# ---------------------------------------------------------------- datasets
def _write_splits(tmp_path):
    rng = np.random.default_rng(0)
    data = rng.integers(0, 256, size=(12, 84, 84, 3), dtype=np.uint8)
    labels = [i // 3 for i in range(12)]
    with open(tmp_path / 'miniImageNet_category_split_train_phase_train.pickle', 'wb') as f:
        pickle.dump({'data': data, 'labels': labels}, f)
    np.savez(tmp_path / 'train_images.npz', images=data)
    with open(tmp_path / 'train_labels.pkl', 'wb') as f:
        pickle.dump({'labels': labels}, f)


def _check_dataset(datasets, name, root, in_hw):
    ds = datasets.make(name, root_path=root, device='cpu', split='train', augment='randaug')
    assert isinstance(ds.transform, T.DeviceRandAugCrop) and (ds.transform.H, ds.transform.W, ds.transform.out) == in_hw + (80,)
    assert isinstance(ds.default_transform, T.DeviceTransform) and (ds.default_transform.RH, ds.default_transform.crop) == (80, 80)
    assert not hasattr(ds, 'gather_pair')                              # one view, not a pair
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ds.gather(torch.tensor([0, 1]))
    sw = datasets.make(name, root_path=root, device='cpu', split='train', augment='strongweak')
    assert sw.transform.weak_randaug == 0.0 and 'randaug' not in sw.transform.draw(8)
    sw = datasets.make(name, root_path=root, device='cpu', split='train', augment='strongweak', weak_randaug=0.2, strong_prob=0.8)
    assert sw.transform.weak_randaug == 0.2 and sw.transform.strong_prob == 0.8 and hasattr(sw, 'gather_pair')
    assert _within_5_sigma(sw.transform.draw(20000)['randaug'][0].numel(), 20000, 0.2 * 0.75)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        sw.gather_pair(torch.tensor([0, 1]))
    with pytest.raises(NotImplementedError):
        datasets.make(name, root_path=root, device='cpu', split='train', augment='cropaug')
    return ds


def test_pickle_datasets_accept_randaug_without_a_gpu(tmp_path):
    from fewshot_vit_amd import datasets
    _write_splits(tmp_path)
    for name in ('mini-imagenet', 'tiered-imagenet'):
        ds = _check_dataset(datasets, name, str(tmp_path), (84, 84))
        assert tuple(ds.transform.fill) == T.RA_FILL


@needs_pillow
def test_cifar_fs_accepts_randaug_without_a_gpu(tmp_path):
    from fewshot_vit_amd import datasets
    from fewshot_vit_amd.datasets.folder_datasets import CIFAR_MEAN
    rng = np.random.default_rng(0)
    for c in range(2):
        os.makedirs(tmp_path / 'meta-train' / f'c{c}')
        for k in range(3):
            Image.fromarray(rng.integers(0, 256, size=(32, 32, 3), dtype=np.uint8)).save(tmp_path / 'meta-train' / f'c{c}' / f'{k}.png')
    ds = _check_dataset(datasets, 'cifar-fs', str(tmp_path), (32, 32))
    assert list(ds.transform.mean) == pytest.approx(list(CIFAR_MEAN)) and tuple(ds.transform.fill) == (129, 124, 112)
