"""The SUN-D patch loaders on the GPU (datasets/transforms.py: DevicePatchGrid, DevicePatchSampler; the `patches` keyword of the image datasets)
against Pillow's own bytes (tests/golden/patch_grid_pil.npz), compared after ToTensor + Normalize as tests/test_gpu_augment.py compares, bit for bit."""
import os
import pickle

import numpy as np
import pytest
import torch

import emd_cases as ec

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
TINY = dict(img_size=80, init_channels=8, embed_dim=64, depth=[1, 1, 1], num_heads=6, mlp_ratio=4., group=8)       # the encoder of test_gpu_emd.py


def _normalise(u8, mean=None, std=None):
    """uint8 [80, 80, 3] -> float32 [3, 80, 80]: ToTensor + Normalize as test_gpu_augment.py computes them"""
    from oracle import transform_oracle as to
    mean = to.MEAN if mean is None else np.array(mean, dtype=np.float32)
    std = to.STD if std is None else np.array(std, dtype=np.float32)
    t = u8.astype(np.float32) / np.float32(255)
    return np.ascontiguousarray(((t - mean) / std).transpose(2, 0, 1))


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'patch_grid_pil.npz'))


@pytest.fixture(scope='module')
def sources(golden_dir):
    return np.load(os.path.join(golden_dir, 'transform_pil.npz'))['images'], np.load(os.path.join(golden_dir, 'transform_rrc_pil.npz'))['src60x100']


def _same_bits(got, want):
    return np.array_equal(got.view(np.int32), want.view(np.int32))


def test_grid_eval_is_pillow_exact(golden, sources):
    from fewshot_vit_amd.datasets import transforms as T
    images = torch.from_numpy(sources[0]).to(DEV)
    src = int(golden['eval_source'])
    grid = T.DevicePatchGrid((84, 84), 80, DEV)
    out = grid(images, torch.tensor([src, 2, src]))
    assert out.shape == (3, 13, 3, 80, 80) and out.dtype == torch.float32
    assert np.array_equal(grid.boxes.view(3, 13, 4)[0].numpy(), golden['eval_box']) and not bool(grid.flips.any())
    got = out.cpu().numpy()
    for p in range(13):
        want = _normalise(golden['eval_out'][p])
        assert _same_bits(got[0, p], want) and _same_bits(got[2, p], want), p
    assert not np.array_equal(got[1], got[0])
    # mean / std override: the same bytes under the statistics of the reference's SUN-D loaders
    sund = T.DevicePatchGrid((84, 84), 80, DEV, mean=T.SUND_MEAN, std=T.SUND_STD)(images, torch.tensor([src])).cpu().numpy()
    for p in range(13):
        assert _same_bits(sund[0, p], _normalise(golden['eval_out'][p], T.SUND_MEAN, T.SUND_STD)), p
    assert not np.array_equal(sund[0], got[0])


def test_grid_train_cases_are_pillow_exact(golden, sources):
    """the 8 recorded train patches, boxes and flips passed in: 4 per source, through a one-level grid object (4 patches per image)"""
    from fewshot_vit_amd.datasets import transforms as T
    for s, images in enumerate((sources[0][1:2], sources[1][None])):
        sel = np.nonzero(golden['train_source'] == s)[0]
        assert len(sel) == 4
        images = torch.from_numpy(np.ascontiguousarray(images)).to(DEV)
        grid = T.DevicePatchGrid(tuple(images.shape[1:3]), 80, DEV, patch_list=(2,), train=True)
        out = grid(images, torch.tensor([0]), boxes=torch.from_numpy(golden['train_box'][sel]), flips=torch.from_numpy(golden['train_flip'][sel]))
        assert out.shape == (1, 4, 3, 80, 80)
        assert golden['train_flip'][sel].tolist() == grid.flips.int().tolist()
        for k, c in enumerate(sel):
            assert _same_bits(out[0, k].cpu().numpy(), _normalise(golden['train_out'][c])), int(c)


def test_grid_train_draw_is_seeded_and_kept(sources):
    from fewshot_vit_amd.datasets import transforms as T
    images = torch.from_numpy(sources[0]).to(DEV)
    index = torch.tensor([0, 1, 2, 3, 1])
    a = T.DevicePatchGrid((84, 84), 80, DEV, train=True, seed=7)
    out = a(images, index)
    boxes, flips = a.boxes.clone(), a.flips.clone()
    assert boxes.shape == (65, 4) and flips.shape == (65,) and bool(flips.any()) and not bool(flips.all())
    b = T.DevicePatchGrid((84, 84), 80, DEV, train=True, seed=7)
    assert torch.equal(b(images, index), out) and torch.equal(b.boxes, boxes) and torch.equal(b.flips, flips)
    assert not torch.equal(b(images, index), out)                                    # the generator moves on
    assert torch.equal(b.manual_seed(7)(images, index), out)
    assert torch.equal(T.DevicePatchGrid((84, 84), 80, DEV, train=True)(images, index, boxes=boxes, flips=flips), out)


def test_sampling_equals_the_random_resized_crop(sources):
    from fewshot_vit_amd.datasets import transforms as T
    images = torch.from_numpy(sources[0]).to(DEV)
    index, P = torch.tensor([3, 0, 3]), 9
    s = T.DevicePatchSampler((84, 84), 80, DEV, num_patch=P, seed=11)
    out = s(images, index)
    assert out.shape == (3, P, 3, 80, 80) and s.boxes.shape == (3 * P, 4) and s.flips.shape == (3 * P,)
    rrc = T.DeviceRandomResizedCrop((84, 84), 80, DEV)(images, index.repeat_interleave(P), boxes=s.boxes, flips=s.flips)
    assert torch.equal(out.view(-1, 3, 80, 80).view(torch.int32), rrc.view(torch.int32))
    again = T.DevicePatchSampler((84, 84), 80, DEV, num_patch=P, seed=11)
    assert torch.equal(again(images, index), out) and torch.equal(again.boxes, s.boxes) and torch.equal(again.flips, s.flips)
    assert torch.equal(T.DevicePatchSampler((84, 84), 80, DEV, num_patch=P)(images, index, boxes=s.boxes, flips=s.flips), out)
    assert len({tuple(r.tolist()) for r in s.boxes[:P]}) > 1


@pytest.fixture(scope='module')
def tiny_root(tmp_path_factory, sources):
    root = tmp_path_factory.mktemp('mini')
    rng = np.random.default_rng(0)
    data = np.concatenate([sources[0], rng.integers(0, 256, (8, 84, 84, 3), dtype=np.uint8)])          # 3 classes x 4 images
    with open(os.path.join(root, 'miniImageNet_category_split_test.pickle'), 'wb') as f:
        pickle.dump({'data': data, 'labels': [c for c in (7, 8, 9) for _ in range(4)]}, f)
    return str(root)


def test_dataset_gather_shapes_and_the_unchanged_default(tiny_root, golden):
    from fewshot_vit_amd import datasets
    from fewshot_vit_amd.datasets import transforms as T
    index = torch.tensor([0, 5, 11, 0, 2])
    plain = datasets.make('mini-imagenet', root_path=tiny_root, split='test', device=DEV)
    want = T.DeviceTransform((84, 84), (88, 88), 80, DEV)(plain.device_images(), index)            # today's gather: the transform alone
    assert torch.equal(plain.gather(index).view(torch.int32), want.view(torch.int32))
    assert torch.equal(datasets.make('mini-imagenet', root_path=tiny_root, split='test', device=DEV, patches=None).gather(index), want)
    grid = datasets.make('mini-imagenet', root_path=tiny_root, split='test', device=DEV, patches='grid')
    out = grid.gather(index)
    assert out.shape == (5, 13, 3, 80, 80)
    assert int(golden['eval_source']) == 0                                              # dataset image 0, gathered at positions 0 and 3
    got = out.cpu().numpy()
    for p in range(13):
        assert _same_bits(got[0, p], _normalise(golden['eval_out'][p])) and _same_bits(got[3, p], got[0, p]), p
    x, y = grid[5]
    assert x.shape == (13, 3, 80, 80) and y == 1
    samp = datasets.make('mini-imagenet', root_path=tiny_root, split='test', device=DEV, patches='sampling')
    assert samp.gather(index).shape == (5, 9, 3, 80, 80) and samp[0][0].shape == (9, 3, 80, 80)
    assert datasets.make('mini-imagenet', root_path=tiny_root, split='test', device=DEV, patches='sampling', num_patch=3).gather(index).shape == (5, 3, 3, 80, 80)
    fcn = datasets.make('mini-imagenet', root_path=tiny_root, split='test', device=DEV, resize=[92, 92])
    assert torch.equal(fcn.gather(index), T.DeviceTransform((84, 84), (92, 92), 80, DEV)(plain.device_images(), index))


def test_deepemd_grid_on_a_gathered_batch(tiny_root):
    """DeepEMD(deepemd='grid') over the tiny Visformer of test_gpu_emd.py on a gathered, split batch: the logits against emd_cases.head_oracle on the
    module's own nodes within that file's 1e-4 (13 nodes)"""
    from fewshot_vit_amd import datasets, models
    from fewshot_vit_amd.models.visformer import Visformer
    from fewshot_vit_amd.utils import few_shot as fs
    models.register('tiny_visformer_emd')(lambda **a: Visformer(**TINY, **a))
    torch.manual_seed(0)
    m = models.make('deepemd', encoder='tiny_visformer_emd', encoder_args={'numerics': 'parity'}, deepemd='grid').cuda().eval()
    ds = datasets.make('mini-imagenet', root_path=tiny_root, split='test', device=DEV, patches='grid')
    way, shot, query = 3, 1, 2
    index = torch.tensor([0, 1, 2, 4, 5, 6, 8, 9, 10])                                       # class-major: 3 classes x (1 shot + 2 queries)
    x_shot, x_query = fs.split_shot_query(ds.gather(index), way, shot, query)
    assert x_shot.shape == (1, 3, 1, 13, 3, 80, 80) and x_query.shape == (1, 6, 13, 3, 80, 80)
    with torch.no_grad():
        logits = m(x_shot, x_query)
        tok = m.encode(torch.cat([x_shot.reshape(-1, 13, 3, 80, 80), x_query.reshape(-1, 13, 3, 80, 80)]), True).cpu().double()
    m.check_status()
    ref = ec.head_oracle(tok[:3].reshape(1, 3, 13, -1), tok[3:].reshape(1, 6, 13, -1), m.temperature)[0]
    err = (logits.cpu().double() - ref).abs().max().item()
    print(f'DeepEMD grid on gathered patches (13 nodes): max |logit - oracle| = {err:.3e}')
    assert logits.shape == (1, 6, 3) and err <= 1e-4
