"""The host side of the SUN-D patch loaders (datasets/transforms.py: grid_boxes, DevicePatchGrid.draw, DevicePatchSampler.draw) and the
'synthetic-images' dataset, without a GPU.  tests/golden/patch_grid_pil.npz holds the reference's own get_grid_location outputs and Pillow's
patches (tests/golden/make_patch_grid_golden.py)."""
import os

import numpy as np
import pytest
import torch

from fewshot_vit_amd import datasets
from fewshot_vit_amd.datasets import transforms as T
from oracle import transform_oracle as to


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'patch_grid_pil.npz'))


@pytest.fixture(scope='module')
def sources(golden_dir):
    return [np.load(os.path.join(golden_dir, 'transform_pil.npz'))['images'], np.load(os.path.join(golden_dir, 'transform_rrc_pil.npz'))['src60x100']]


def test_grid_locations_equal_the_reference(golden):
    assert len(golden['loc_case']) == 3 * 2 * 6
    for (size, n), ratio, out in zip(golden['loc_case'], golden['loc_ratio'], golden['loc_out']):
        assert T.grid_location(int(size), float(ratio), int(n)) == [tuple(int(v) for v in c) for c in out[:n]], (size, n, ratio)
        # grid_boxes: the same extents once per axis, rows outer and columns inner
        boxes = T.grid_boxes(int(size), int(size), float(ratio), int(n))
        want = [(t, l, b - t, r - l) for t, b in out[:n].tolist() for l, r in out[:n].tolist()]
        assert boxes == want
    # a non-square image takes the width's extents for the columns and the height's for the rows
    assert T.grid_boxes(60, 100, 2.0, 2) == [(t, l, b - t, r - l) for t, b in T.grid_location(60, 2.0, 2) for l, r in T.grid_location(100, 2.0, 2)]


def test_grid_extents_of_the_84_pixel_source():
    assert T.grid_location(84, 2, 2) == [(0, 63), (21, 84)]
    assert T.grid_location(84, 2, 3) == [(0, 42), (14, 70), (42, 84)]


def test_eval_patch_order_and_count(golden):
    g = T.DevicePatchGrid((84, 84), 80, 'cpu')
    assert g.n_patch == 13
    boxes, flips = g.draw(3)
    assert boxes.shape == (39, 4) and boxes.dtype == torch.int32 and flips.shape == (39,) and not bool(flips.any())
    for b in range(3):
        assert np.array_equal(boxes[13 * b:13 * (b + 1)].numpy(), golden['eval_box'])
    assert T.DevicePatchGrid((84, 84), 80, 'cpu', patch_list=(2,)).n_patch == 4
    assert T.DevicePatchGrid((84, 84), 80, 'cpu', patch_list=(3, 2, 1)).n_patch == 14


def test_train_grid_draw():
    g = T.DevicePatchGrid((84, 84), 80, 'cpu', train=True, seed=5)
    boxes, flips = g.draw(64)
    again = T.DevicePatchGrid((84, 84), 80, 'cpu', train=True, seed=5).draw(64)
    assert torch.equal(boxes, again[0]) and torch.equal(flips, again[1])
    assert boxes.shape == (64 * 13, 4) and flips.shape == (64 * 13,)
    b = boxes.view(64, 13, 4).long()
    assert bool((b[..., 0] >= 0).all() and (b[..., 1] >= 0).all() and (b[..., 2] > 0).all() and (b[..., 3] > 0).all())
    assert bool((b[..., 0] + b[..., 2] <= 84).all() and (b[..., 1] + b[..., 3] <= 84).all())
    # one ratio per (image, level): the first cell of a level is (0, 0, raw // 2 + enl // 2, the same) with enl = int(84 / n * ratio), ratio in [1, 3)
    for lo, n in ((0, 2), (4, 3)):
        side = b[:, lo, 2]
        raw = 84 // n
        assert bool((side >= raw // 2 + raw // 2).all() and (side <= raw // 2 + int(84 / n * 3) // 2).all())
        assert side.unique().numel() > 8                          # ... and it varies from image to image
    assert not torch.equal(b[:, 0, 2] * 2, b[:, 4, 2] * 3)        # the two levels of an image draw their own ratios
    assert 0.4 < flips.float().mean().item() < 0.6                # flips: per patch, probability 0.5
    assert flips.view(64, 13).float().mean(dim=1).unique().numel() > 3


def test_golden_patches_are_what_the_oracle_resize_gives(golden, sources):
    """pins the fixture to oracle.transform_oracle.pil_resize_bilinear, which the GPU tests of the crop kernel lean on"""
    src = sources[0][int(golden['eval_source'])]
    for (i, j, h, w), out in zip(golden['eval_box'].tolist(), golden['eval_out']):
        assert np.array_equal(to.pil_resize_bilinear(src[i:i + h, j:j + w], 80, 80), out)
    train_sources = [sources[0][1], sources[1]]
    for s, (i, j, h, w), flip, out in zip(golden['train_source'], golden['train_box'].tolist(), golden['train_flip'], golden['train_out']):
        r = to.pil_resize_bilinear(train_sources[int(s)][i:i + h, j:j + w], 80, 80)
        assert np.array_equal(r[:, ::-1] if flip else r, out)
    # and the recorded train boxes are grid_boxes at the recorded ratio, level and cell
    for s, level, ratio, (row, col), box in zip(golden['train_source'], golden['train_level'], golden['train_ratio'], golden['train_cell'], golden['train_box']):
        H, W = train_sources[int(s)].shape[:2]
        assert T.grid_boxes(H, W, float(ratio), int(level))[int(row) * int(level) + int(col)] == tuple(box.tolist())


def test_sampler_boxes():
    B, P = 6, 9
    s = T.DevicePatchSampler((60, 100), 80, 'cpu', num_patch=P, seed=3)
    boxes, flips = s.draw(B)
    again = T.DevicePatchSampler((60, 100), 80, 'cpu', num_patch=P, seed=3).draw(B)
    other = T.DevicePatchSampler((60, 100), 80, 'cpu', num_patch=P, seed=4).draw(B)
    assert boxes.shape == (B * P, 4) and boxes.dtype == torch.int32 and flips.shape == (B * P,)
    assert torch.equal(boxes, again[0]) and torch.equal(flips, again[1]) and not torch.equal(boxes, other[0])
    i, j, h, w = boxes.long().unbind(1)
    assert bool((i >= 0).all() and (j >= 0).all() and (h > 0).all() and (w > 0).all() and (i + h <= 60).all() and (j + w <= 100).all())
    for b in boxes.view(B, P, 4):                                   # the P copies of one image get their own boxes
        assert len({tuple(r.tolist()) for r in b}) > 1


def test_synthetic_images_dataset():
    assert 'synthetic-images' in datasets.datasets
    kw = dict(n_classes=3, n_per_class=4, device='cpu')
    a, b = datasets.make('synthetic-images', split='val', **kw), datasets.make('synthetic-images', split='val', **kw)
    assert a.images.dtype == torch.uint8 and tuple(a.images.shape) == (12, 84, 84, 3) and torch.equal(a.images, b.images)
    assert a.label == [0] * 4 + [1] * 4 + [2] * 4 and a.n_classes == 3 and len(a) == 12
    assert not torch.equal(a.images, datasets.make('synthetic-images', split='val', seed=1, **kw).images)
    seeds = [set(datasets.make('synthetic-images', split=s, **kw).class_seeds) for s in ('train', 'val', 'test')]
    assert not (seeds[0] & seeds[1]) and not (seeds[0] & seeds[2]) and not (seeds[1] & seeds[2])
    x = a.images.float()
    within = (x[:4] - x[:4].mean(0)).abs().mean().item()
    across = (x[:4].mean(0) - x[4:8].mean(0)).abs().mean().item()
    assert across > within                                          # class-structured: the class means differ by more than the noise
    # prefix property: image i of class c does not depend on how many classes there are
    assert torch.equal(datasets.make('synthetic-images', split='val', n_classes=2, n_per_class=4, device='cpu').images, a.images[:8])


def test_dataset_patch_keywords():
    kw = dict(n_classes=2, n_per_class=2, device='cpu')
    assert isinstance(datasets.make('synthetic-images', patches='grid', **kw).transform, T.DevicePatchGrid)
    s = datasets.make('synthetic-images', patches='sampling', num_patch=5, mean=T.SUND_MEAN, std=T.SUND_STD, **kw)
    assert isinstance(s.transform, T.DevicePatchSampler) and s.transform.n_patch == 5
    assert [round(v * 255, 1) for v in s.mean] == [125.3, 123.0, 113.9]
    g = datasets.make('synthetic-images', patches='grid', patch_list=(2,), patch_ratio=1.5, patch_train=True, **kw).transform
    assert g.patch_list == (2,) and g.patch_ratio == 1.5 and g.train
    plain = datasets.make('synthetic-images', **kw)
    assert isinstance(plain.transform, T.DeviceTransform) and (plain.transform.RH, plain.transform.RW) == (88, 88)
    assert (datasets.make('synthetic-images', resize=[92, 92], **kw).transform.RH) == 92
    for augment in ('strongweak', 'randaug'):
        with pytest.raises(ValueError):
            datasets.make('synthetic-images', patches='grid', augment=augment, **kw)
    with pytest.raises(ValueError):
        datasets.make('synthetic-images', patches='pyramid', **kw)
