"""'mini-imagenet' / 'tiered-imagenet' with the reference's file formats and constructor surface
(test_phase/datasets/mini_imagenet.py:27-44, tiered_imagenet.py:13-50), MI355X-first: the whole split is uploaded ONCE as a
uint8 [N,84,84,3] tensor (mini test split 254 MB; all 60 000 images 1.27 GB of the 288 GB) and episodes are gathered +
transformed on the GPU by index (`gather`, fsvit_image_transform_gather) instead of 8 DataLoader workers running PIL.
`self.transform` is what `gather` / `__getitem__` apply.  `augment=None` is the eval transform.  `augment='resize'` is the supervised phase's
train-time augmentation (sun_train_teacher/datasets/mini_imagenet.py:50-63, tiered_imagenet.py:68-81): RandomResizedCrop(80) +
RandomHorizontalFlip on the GPU (fsvit_image_transform_rrc_gather), with `default_transform` = that phase's Resize(80) + ToTensor +
Normalize; `ds.transform = ds.default_transform` switches the augmentation off.  `augment='strongweak'` (our name: the reference keys it on
`split == 'train'`, sun_meta_training/datasets/mini_imagenet.py:160-163, :194-204) is the distillation phase's view pair on the GPU
(transforms.DeviceStrongWeakPair: fsvit_image_transform_rrc_u8 + fsvit_image_strong_weak): `gather_pair(index)` -> (strong, weak),
`__getitem__` -> (strong, weak, label), `strong_prob` (default 0.5) as in the reference's constructor; `weak_randaug` (default 0.0: off; the
reference's value is 0.2) is the probability of the weak view's RandomApply([RandAugment], p), a third launch (fsvit_image_rand_augment) between
the two.  `augment='randaug'` is the reference's `cropaug` pipeline under our own name (timm's create_transform: bicubic RandomResizedCrop + flip
-> RandAugment 'rand-m9-mstd0.5-inc1' -> Normalize -> RandomErasing(0.25, 'pixel'); transforms.DeviceRandAugCrop), with the `default_transform` of
`'resize'`; the RandAugment draw restates timm's published algorithm and is not pinned against timm, so the name `'cropaug'` itself stays
refused, as does `'crop'` (padded RandomCrop).

`patches='grid' | 'sampling'` (default None) are the SUN-D loaders (meta_tuning_sun_d/Models/dataloader/miniimagenet/{grid,sampling}): `gather` then
returns [len, P, 3, 80, 80] and `__getitem__` [P, 3, 80, 80] (transforms.DevicePatchGrid with `patch_list`, `patch_ratio`, `patch_train`;
transforms.DevicePatchSampler with `num_patch`).  `mean` / `std` override the normalisation statistics (default: ImageNet's; SUN-D's csv loaders
use transforms.SUND_MEAN / SUND_STD) and `resize` the eval transform's Resize (SUN-D `fcn`: Resize([92, 92]) -> CenterCrop(80)).

'synthetic-images' is a deterministic class-structured uint8 table behind the same class, for machines without the pickles."""
import os
import pickle

import numpy as np
import torch

from .datasets import register
from .transforms import (IMAGENET_MEAN, IMAGENET_STD, DevicePatchGrid, DevicePatchSampler, DeviceRandAugCrop, DeviceRandomResizedCrop,
                         DeviceStrongWeakPair, DeviceTransform)


class _DeviceImageDataset:
    resize, crop = (88, 88), 80

    def _finish(self, data: np.ndarray, label, device, augment=None, strong_prob=0.5, weak_randaug=0.0, patches=None, patch_list=(2, 3),
                patch_ratio=2.0, num_patch=9, patch_train=False, mean=None, std=None, resize=None):
        if patches not in (None, 'grid', 'sampling'):
            raise ValueError(f"patches={patches!r}: None, 'grid' or 'sampling'")
        if patches is not None and augment in ('strongweak', 'randaug'):
            raise ValueError(f'patches={patches!r} cannot be combined with augment={augment!r}')
        if mean is not None:
            self.mean = tuple(float(v) for v in mean)
        if std is not None:
            self.std = tuple(float(v) for v in std)
        if resize is not None:
            self.resize = (int(resize), int(resize)) if isinstance(resize, int) else tuple(int(v) for v in resize)
        if data.dtype != np.uint8 or data.ndim != 4 or data.shape[-1] != 3:
            raise ValueError('expected uint8 images [N,H,W,3]')
        min_label = min(label)
        self.label = [int(x) - int(min_label) for x in label]
        self.n_classes = max(self.label) + 1
        self.device = torch.device(device if device is not None else ('cuda' if torch.cuda.is_available() else 'cpu'))
        self.images = torch.from_numpy(np.ascontiguousarray(data))
        self._on_device = None
        in_hw, norm = tuple(self.images.shape[1:3]), dict(mean=getattr(self, 'mean', IMAGENET_MEAN), std=getattr(self, 'std', IMAGENET_STD))
        if augment == 'resize':
            self.default_transform = DeviceTransform(in_hw, (self.crop, self.crop), self.crop, self.device, **norm)     # Resize(80)
            self.transform = DeviceRandomResizedCrop(in_hw, self.crop, self.device, **norm)
        elif augment == 'strongweak':
            self.default_transform = DeviceTransform(in_hw, (self.crop, self.crop), self.crop, self.device, **norm)     # Resize(80)
            self.transform = DeviceStrongWeakPair(in_hw, self.crop, self.device, strong_prob=strong_prob, weak_randaug=weak_randaug, **norm)
        elif augment == 'randaug':
            self.default_transform = DeviceTransform(in_hw, (self.crop, self.crop), self.crop, self.device, **norm)     # Resize(80)
            self.transform = DeviceRandAugCrop(in_hw, self.crop, self.device, **norm)
        else:
            self.default_transform = self.transform = DeviceTransform(in_hw, self.resize, self.crop, self.device, **norm)
        if patches == 'grid':
            self.transform = DevicePatchGrid(in_hw, self.crop, self.device, patch_list=patch_list, patch_ratio=patch_ratio, train=patch_train, **norm)
        elif patches == 'sampling':
            self.transform = DevicePatchSampler(in_hw, self.crop, self.device, num_patch=num_patch, **norm)

    def __len__(self):
        return len(self.label)

    def device_images(self):
        if self._on_device is None:
            if self.device.type != 'cuda':
                raise RuntimeError('fsvit: the dataset transform runs on an MI355X (no CPU fallback)')
            self._on_device = self.images.to(self.device)
        return self._on_device

    def gather(self, index) -> torch.Tensor:
        """index: LongTensor of dataset indices (one sampler batch) -> float32 [len, 3, 80, 80] on the GPU ([len, P, 3, 80, 80] with patches)."""
        out = self.transform(self.device_images(), torch.as_tensor(index))
        return out[0] if isinstance(out, tuple) else out   # under 'strongweak': the strong view

    @property
    def gather_pair(self):
        """`gather_pair(index)` -> (strong, weak), float32 [len, 3, 80, 80] each on the GPU: one launch pair for the batch.  The attribute exists
        exactly while `self.transform` is the view-pair transform (`hasattr` is how the distillation driver asks), so it follows a replaced
        `ds.transform` both ways."""
        if not isinstance(self.transform, DeviceStrongWeakPair):
            raise AttributeError("gather_pair: dataset.transform is not the 'strongweak' view pair")
        return self._gather_pair

    def _gather_pair(self, index):
        return self.transform(self.device_images(), torch.as_tensor(index))

    def __getitem__(self, i):
        if isinstance(self.transform, DeviceStrongWeakPair):
            strong, weak = self._gather_pair(torch.tensor([int(i)]))
            return strong[0], weak[0], self.label[i]
        return self.gather(torch.tensor([int(i)]))[0], self.label[i]


@register('mini-imagenet')
class MiniImageNet(_DeviceImageDataset):
    resize, crop = (88, 88), 80                         # Resize((88, 88)) -> CenterCrop(80), mini_imagenet.py:49-52

    def __init__(self, root_path, split='train', augment=None, device=None, strong_prob=0.5, weak_randaug=0.0, patches=None, patch_list=(2, 3),
                 patch_ratio=2.0, num_patch=9, patch_train=False, mean=None, std=None, resize=None, **kwargs):
        if augment not in (None, 'resize', 'strongweak', 'randaug'):
            raise NotImplementedError("fsvit: augment=None, 'resize', 'strongweak' and 'randaug' are built ('crop' / 'cropaug' are not)")
        split_tag = 'train_phase_train' if split == 'train' else split
        with open(os.path.join(root_path, 'miniImageNet_category_split_{}.pickle'.format(split_tag)), 'rb') as f:
            pack = pickle.load(f, encoding='latin1')
        self._finish(np.asarray(pack['data']), pack['labels'], device, augment, strong_prob, weak_randaug, patches, patch_list, patch_ratio, num_patch,
                     patch_train, mean, std, resize)


@register('tiered-imagenet')
class TieredImageNet(_DeviceImageDataset):
    resize, crop = (80, 80), 80                         # Resize(80) on square images, tiered_imagenet.py:53-57

    def __init__(self, root_path, split='train', mini=False, augment=None, device=None, strong_prob=0.5, weak_randaug=0.0, patches=None,
                 patch_list=(2, 3), patch_ratio=2.0, num_patch=9, patch_train=False, mean=None, std=None, resize=None, **kwargs):
        if augment not in (None, 'test', 'resize', 'strongweak', 'randaug'):       # 'test' = the un-augmented transform, tiered_imagenet.py:90-91
            raise NotImplementedError("fsvit: augment=None, 'test', 'resize', 'strongweak' and 'randaug' are built ('crop' / 'cropaug' are not)")
        data = np.load(os.path.join(root_path, '{}_images.npz'.format(split)), allow_pickle=True)['images']
        data = data[:, :, :, ::-1]                      # BGR -> RGB, tiered_imagenet.py:21
        with open(os.path.join(root_path, '{}_labels.pkl'.format(split)), 'rb') as f:
            label = pickle.load(f)['labels']
        if mini:                                        # tiered_imagenet.py:33-50
            min_label = min(label)
            label = [x - min_label for x in label]
            np.random.seed(0)
            c = np.random.choice(max(label) + 1, 64, replace=False).tolist()
            cnt = {x: 0 for x in c}
            ind = {x: i for i, x in enumerate(c)}
            keep, label_ = [], []
            for i in range(len(data)):
                y = int(label[i])
                if y in cnt and cnt[y] < 600:
                    keep.append(i)
                    label_.append(ind[y])
                    cnt[y] += 1
            data, label = data[keep], label_
        self._finish(np.ascontiguousarray(data), label, device, augment, strong_prob, weak_randaug, patches, patch_list, patch_ratio, num_patch,
                     patch_train, mean, std, resize)


@register('synthetic-images')
class SyntheticImages(_DeviceImageDataset):
    """A stand-in for a miniImageNet split as RAW images: a uint8 [n_classes * n_per_class, 84, 84, 3] table, image i of class c =
    clip(128 + 40 mu_c + noise eps_i), fixed by (seed, split, index), behind the transforms of 'mini-imagenet' - the patch modes crop raw
    images, which 'synthetic-episodes' (finished float images) cannot offer.  The splits carry disjoint class seeds."""
    resize, crop = (88, 88), 80
    SPLIT_OFFSET = {'train': 0, 'train_phase_train': 0, 'val': 1, 'test': 2}

    def __init__(self, root_path=None, split='test', n_classes=20, n_per_class=30, image_size=84, noise=20.0, seed=0, augment=None, device=None,
                 strong_prob=0.5, weak_randaug=0.0, patches=None, patch_list=(2, 3), patch_ratio=2.0, num_patch=9, patch_train=False, mean=None,
                 std=None, resize=None, **kwargs):
        if augment not in (None, 'resize', 'strongweak', 'randaug'):
            raise NotImplementedError("fsvit: augment=None, 'resize', 'strongweak' and 'randaug' are built ('crop' / 'cropaug' are not)")
        if split not in self.SPLIT_OFFSET:
            raise ValueError(split)
        self.class_seeds = [(int(seed) * 3 + self.SPLIT_OFFSET[split]) * 100003 + c for c in range(n_classes)]      # disjoint across the splits of a seed
        data = np.empty((n_classes * n_per_class, image_size, image_size, 3), dtype=np.uint8)
        for c, cs in enumerate(self.class_seeds):
            rng = np.random.Generator(np.random.PCG64(cs))
            mu = rng.standard_normal((image_size, image_size, 3))
            eps = rng.standard_normal((n_per_class, image_size, image_size, 3))
            data[c * n_per_class:(c + 1) * n_per_class] = np.clip(np.rint(128.0 + 40.0 * mu[None] + float(noise) * eps), 0, 255).astype(np.uint8)
        self._finish(data, np.repeat(np.arange(n_classes), n_per_class).tolist(), device, augment, strong_prob, weak_randaug, patches, patch_list,
                     patch_ratio, num_patch, patch_train, mean, std, resize)
