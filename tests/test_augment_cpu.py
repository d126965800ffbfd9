"""CPU checks of the train-time augmentation `augment: resize` (sun_train_teacher/datasets/mini_imagenet.py:57-63): the host-side box sampler
restates the distribution of torchvision's RandomResizedCrop.get_params, the image datasets accept the reference's
`train_dataset_args: {split: train, augment: resize}` without a GPU, the committed Pillow vectors (tests/golden/transform_rrc_pil.npz) equal the
oracle's resize of the cropped array, and explicit boxes are validated on the host."""
import os
import pickle

import numpy as np
import pytest
import torch

from oracle import transform_oracle as to


def _boxes(n, H, W, seed, **kw):
    from fewshot_vit_amd.datasets.transforms import random_resized_crop_boxes
    return random_resized_crop_boxes(n, H, W, torch.Generator().manual_seed(seed), **kw)


@pytest.mark.parametrize('H,W', [(84, 84), (60, 100)])
def test_drawn_boxes_follow_the_reference_distribution(H, W):
    b = _boxes(20000, H, W, 3)
    assert b.dtype == torch.int32 and tuple(b.shape) == (20000, 4)
    i, j, h, w = (x.double() for x in b.long().unbind(1))
    assert bool(((h >= 1) & (w >= 1) & (i >= 0) & (j >= 0) & (i + h <= H) & (j + w <= W)).all())
    # w = round(sqrt(area * r)), h = round(sqrt(area / r)) with area in [0.08, 1] * H * W and r in [3/4, 4/3]: each side is within 0.5 of its real value
    lo_a, hi_a = (w - 0.5).clamp(min=0) * (h - 0.5).clamp(min=0), (w + 0.5) * (h + 0.5)
    assert bool((hi_a >= 0.08 * H * W).all()) and bool((lo_a <= 1.0 * H * W).all())
    assert bool(((w + 0.5) / (h - 0.5).clamp(min=1e-9) >= 3. / 4.).all()) and bool(((w - 0.5) / (h + 0.5) <= 4. / 3.).all())
    # the draws cover the range (a 60 x 100 image admits at most 0.8 of its area at a ratio <= 4/3): small and large crops, both extremes of the
    # ratio, every corner of the offsets
    frac = (h * w) / (H * W)
    assert float(frac.min()) < 0.1 and float(frac.max()) > 0.75 and float((w / h).min()) < 0.8 and float((w / h).max()) > 1.25
    assert int(i.min()) == 0 and int(j.min()) == 0 and int((i + h).max()) == H and int((j + w).max()) == W
    assert torch.equal(b, _boxes(20000, H, W, 3))
    assert not torch.equal(b, _boxes(20000, H, W, 4))


def test_fallback_is_the_centre_crop_at_the_clamped_ratio():
    # 10 x 1000: every attempt has h = sqrt(area / r) >= sqrt(800 / (4/3)) = 24.5 > 10 -> fallback, W/H > 4/3: h = H, w = round(h * 4/3)
    assert _boxes(5, 10, 1000, 0).tolist() == [[0, (1000 - 13) // 2, 10, 13]] * 5
    # 1000 x 10: W/H < 3/4: w = W, h = round(w / (3/4))
    assert _boxes(5, 1000, 10, 0).tolist() == [[(1000 - 13) // 2, 0, 13, 10]] * 5
    # a scale above 1 never fits either; the ratio of a square image is inside [3/4, 4/3]: the whole image
    assert _boxes(3, 84, 84, 0, scale=(2.0, 3.0)).tolist() == [[0, 0, 84, 84]] * 3


def test_image_datasets_accept_the_reference_train_dataset_args(tmp_path):
    from fewshot_vit_amd import datasets
    from fewshot_vit_amd.datasets.transforms import DeviceRandomResizedCrop, DeviceTransform
    rng = np.random.default_rng(0)
    data = rng.integers(0, 256, size=(12, 84, 84, 3), dtype=np.uint8)
    labels = [i // 3 for i in range(12)]
    with open(tmp_path / 'miniImageNet_category_split_train_phase_train.pickle', 'wb') as f:
        pickle.dump({'data': data, 'labels': labels}, f)
    np.savez(tmp_path / 'train_images.npz', images=data)
    with open(tmp_path / 'train_labels.pkl', 'wb') as f:
        pickle.dump({'labels': labels}, f)
    args = {'split': 'train', 'augment': 'resize'}                     # train_classifier_mini.yaml / train_classifier_tiered.yaml, verbatim
    for name in ('mini-imagenet', 'tiered-imagenet'):
        ds = datasets.make(name, root_path=str(tmp_path), device='cpu', **args)
        assert isinstance(ds.transform, DeviceRandomResizedCrop) and (ds.transform.H, ds.transform.W, ds.transform.out) == (84, 84, 80)
        assert isinstance(ds.default_transform, DeviceTransform)
        assert (ds.default_transform.RH, ds.default_transform.RW, ds.default_transform.crop) == (80, 80, 80)      # Resize(80), no crop
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            ds.gather(torch.tensor([0, 1]))
        plain = datasets.make(name, root_path=str(tmp_path), device='cpu', split='train')
        assert plain.transform is plain.default_transform and isinstance(plain.transform, DeviceTransform)
        assert (plain.transform.RH, plain.transform.RW) == plain.resize and plain.transform.crop == plain.crop
    dt = datasets.make('tiered-imagenet', root_path=str(tmp_path), device='cpu', split='train', augment='test')
    assert dt.transform is dt.default_transform and isinstance(dt.transform, DeviceTransform)
    for name, aug in (('mini-imagenet', 'cropaug'), ('mini-imagenet', 'test'), ('tiered-imagenet', 'crop'), ('tiered-imagenet', 'cropaug')):
        with pytest.raises(NotImplementedError):
            datasets.make(name, root_path=str(tmp_path), device='cpu', split='train', augment=aug)


def test_fixture_equals_pillow_and_the_oracle(golden_dir):
    z = np.load(os.path.join(golden_dir, 'transform_rrc_pil.npz'))
    sources = list(np.load(os.path.join(golden_dir, 'transform_pil.npz'))['images']) + [z['src32'], z['src60x100']]
    assert len(z['out']) <= 20 and os.path.getsize(os.path.join(golden_dir, 'transform_rrc_pil.npz')) < 512 * 1024
    assert set(z['case_flip'].tolist()) == {0, 1}
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for s, (i, j, h, w), flip, gold in zip(z['case_source'], z['case_box'].tolist(), z['case_flip'], z['out']):
        img = sources[s]
        ref = to.pil_resize_bilinear(img[i:i + h, j:j + w], 80, 80)
        assert np.array_equal(ref[:, ::-1] if flip else ref, gold), (s, i, j, h, w, flip)
        if Image is not None:
            im = Image.fromarray(img).crop((j, i, j + w, i + h)).resize((80, 80), Image.BILINEAR)
            if flip:
                im = im.transpose(Image.FLIP_LEFT_RIGHT)
            assert np.array_equal(np.asarray(im), gold), (s, i, j, h, w, flip)


def test_explicit_boxes_are_validated_on_the_host():
    from fewshot_vit_amd.datasets.transforms import DeviceRandomResizedCrop
    tf = DeviceRandomResizedCrop((84, 84), 80, 'cpu')
    images = torch.zeros(2, 84, 84, 3, dtype=torch.uint8)               # a CPU tensor: a call that got past the check would raise RuntimeError
    index = torch.tensor([0, 1])
    flips = torch.tensor([False, True])
    for bad in ([[0, 0, 84, 84], [1, 0, 84, 84]], [[0, 0, 84, 84], [0, 5, 10, 80]], [[0, 0, 0, 5], [0, 0, 5, 5]], [[0, 0, 5, -1], [0, 0, 5, 5]],
                [[-1, 0, 5, 5], [0, 0, 5, 5]], [[0, 0, 84, 84]], [[0, 0, 84], [0, 0, 84]]):
        with pytest.raises(ValueError):
            tf(images, index, boxes=torch.tensor(bad, dtype=torch.int32), flips=flips)
    with pytest.raises(ValueError):
        tf(images, index, boxes=torch.tensor([[0, 0, 84, 84]] * 2, dtype=torch.int32), flips=torch.tensor([True]))
    with pytest.raises(RuntimeError, match='no CPU fallback'):          # a valid box reaches the device check
        tf(images, index, boxes=torch.tensor([[0, 0, 84, 84], [83, 83, 1, 1]], dtype=torch.int32), flips=flips)
