"""Driver smoke test of fewshot_vit_amd.train_deepemd (SUN-D meta-tuning) on the tiny Visformer of test_gpu_emd.py in `parity` numerics over three
tiny pickles: the loop runs for fcn / grid / sampling, the encoder moves, StepLR halves lr, the artifacts load into eval_deepemd, the fixed
validation set is reproduced, the 5-shot (SFC) path trains the encoder through the query side, and a NaN gradient is zeroed by the guard."""
import math
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TINY = dict(img_size=80, init_channels=8, embed_dim=64, depth=[1, 1, 1], num_heads=6, mlp_ratio=4., group=8)       # the encoder of test_gpu_emd.py
ENCODER = 'tiny_visformer_emd'
MODES = {'fcn': [], 'grid': ['-patch_list', '2'], 'sampling': ['-num_patch', '3']}


def _register():
    from fewshot_vit_amd import models
    from fewshot_vit_amd.models.visformer import Visformer
    models.register(ENCODER)(lambda **a: Visformer(**TINY, **a))


@pytest.fixture(scope='module')
def root(tmp_path_factory):
    """train 4 classes x 6, val / test 3 classes x 6: class-structured 84 x 84 uint8 images in the pickle format of 'mini-imagenet'"""
    d = tmp_path_factory.mktemp('sund')
    rng = np.random.default_rng(0)
    for split, n_cls in (('train_phase_train', 4), ('val', 3), ('test', 3)):
        mu = rng.normal(size=(n_cls, 1, 84, 84, 3))
        data = np.clip(128 + 50 * mu + 25 * rng.normal(size=(n_cls, 6, 84, 84, 3)), 0, 255).astype(np.uint8).reshape(-1, 84, 84, 3)
        with open(os.path.join(d, f'miniImageNet_category_split_{split}.pickle'), 'wb') as f:
            pickle.dump({'data': data, 'labels': [c for c in range(n_cls) for _ in range(6)]}, f)
    return str(d)


@pytest.fixture(scope='module')
def pretrained(tmp_path_factory):
    """a pre-trained encoder as a DataParallel meta-tuning checkpoint with a `temp` entry: what -pretrain_dir has to digest"""
    from fewshot_vit_amd import models
    _register()
    torch.manual_seed(0)
    m = models.make('deepemd', encoder=ENCODER, encoder_args={'numerics': 'parity'})
    sd = {'module.' + k: v.clone() for k, v in m.state_dict().items()}
    sd['module.temp'] = torch.tensor(10.0)
    path = os.path.join(tmp_path_factory.mktemp('pre'), 'max-va.pth')
    torch.save({'model_sd': sd}, path)
    return path, {k: v.clone() for k, v in m.state_dict().items()}


def _argv(root, pretrained, mode, save_root, extra=()):
    return ['-dataset', 'mini-imagenet', '-dataset_args', '{root_path: %s}' % root, '-encoder', ENCODER, '-numerics', 'parity', '-pretrain_dir', pretrained[0],
            '-way', '2', '-shot', '1', '-query', '2', '-max_epoch', '2', '-val_frequency', '2', '-bs', '2', '-val_episode', '3', '-test_episode', '3',
            '-step_size', '1', '-episodes_per_launch', '2', '-lr', '0.01', '-seed', '3', '-deepemd', mode, '-save_root', str(save_root), '-save_all',
            *MODES[mode], *extra]


@pytest.mark.parametrize('mode', list(MODES))
def test_driver_runs_and_its_artifacts_load(mode, root, pretrained, tmp_path):
    from fewshot_vit_amd import eval_deepemd, train_deepemd
    _register()
    argv = _argv(root, pretrained, mode, tmp_path)
    out = train_deepemd.main(argv)
    assert set(out) == {'max_acc', 'max_acc_epoch', 'test_acc', 'test_ci', 'save_path'}
    path = out['save_path']
    assert path == os.path.join(str(tmp_path), 'mini-imagenet', mode, '1shot-2way')
    assert sorted(os.listdir(path)) == ['epoch-1.pth', 'epoch-2.pth', 'max_acc.pth', 'optimizer_latest.pth', 'results.txt', 'trlog']
    trlog = torch.load(os.path.join(path, 'trlog'), weights_only=False)
    assert len(trlog['train_loss']) == 2 and all(math.isfinite(v) for k in ('train_loss', 'val_loss', 'train_acc', 'val_acc') for v in trlog[k])
    assert all(v > 0 for v in trlog['train_loss']) and trlog['grad_nan_zeroed'] == [0, 0]
    assert trlog['lr'] == [0.01, 0.005]                                                   # StepLR(step_size 1, gamma 0.5)
    assert out['max_acc'] == max(trlog['val_acc']) and 1 <= out['max_acc_epoch'] <= 2 and 0.0 <= out['test_acc'] <= 100.0 and math.isfinite(out['test_ci'])
    best = torch.load(os.path.join(path, 'max_acc.pth'))
    model = train_deepemd.build_model(train_deepemd.parse_args(argv))
    assert set(best) == {'params'} and list(best['params']) == list(model.state_dict())
    assert all(k.startswith('encoder.') for k in best['params'])
    for e in (1, 2):                                                                      # every encoder parameter has left its initial value
        sd = torch.load(os.path.join(path, f'epoch-{e}.pth'))['params']
        for k, _ in model.named_parameters():
            assert bool(torch.isfinite(sd[k]).all()) and not torch.equal(sd[k], pretrained[1][k]), (e, k)
    with open(os.path.join(path, 'results.txt')) as f:
        lines = f.read().splitlines()
    assert lines[0] == path and lines[-1] == 'Test Acc {:.4f} + {:.4f}'.format(out['test_acc'], out['test_ci'])
    # the checkpoint loads into the eval driver, which scores the same three test episodes
    res = eval_deepemd.main(['-encoder', ENCODER, '-numerics', 'parity', '-dataset', 'mini-imagenet', '-dataset_args', '{root_path: %s}' % root, '-set', 'test',
                             '-way', '2', '-shot', '1', '-query', '2', '-test_episode', '3', '-episodes_per_launch', '2', '-deepemd', mode,
                             '-model_dir', os.path.join(path, 'max_acc.pth'), *MODES[mode]])
    assert res['n'] == 3 and 0.0 <= res['acc'] <= 100.0
    # fixed validation set: the weights of epoch 1 give epoch 1's validation figures again
    args = train_deepemd.parse_args(argv)
    model.load_state_dict(torch.load(os.path.join(path, 'epoch-1.pth'))['params'])
    model = model.cuda()
    valset = train_deepemd.make_dataset(args, 'val')
    dev = torch.device('cuda', torch.cuda.current_device())
    for _ in range(2):
        vl, va = train_deepemd.evaluate(model, valset, args, args.val_episode, dev, seed=args.seed)
        assert len(va) == 3 and float(va.mean()) == trlog['val_acc'][0] and vl == trlog['val_loss'][0]


def test_a_second_run_keeps_what_is_in_the_save_directory(root, pretrained, tmp_path):
    """the save path is fixed by dataset / mode / shot / way: a later run overwrites its own files and removes nothing, an -extra_dir sub-run included"""
    from fewshot_vit_amd import train_deepemd
    _register()
    short = ['-max_epoch', '1']
    sub = train_deepemd.main(_argv(root, pretrained, 'fcn', tmp_path, short + ['-extra_dir', 'lr0.01']))['save_path']
    first = train_deepemd.main(_argv(root, pretrained, 'fcn', tmp_path, short))['save_path']
    assert sub == os.path.join(first, 'lr0.01')
    with open(os.path.join(first, 'notes.txt'), 'w') as f:
        f.write('kept')
    kept = sorted(os.listdir(sub))
    assert 'max_acc.pth' in kept and 'trlog' in kept
    again = train_deepemd.main(_argv(root, pretrained, 'fcn', tmp_path, short + ['-lr', '0.02']))['save_path']
    assert again == first and sorted(os.listdir(sub)) == kept
    with open(os.path.join(first, 'notes.txt')) as f:
        assert f.read() == 'kept'
    assert torch.load(os.path.join(first, 'trlog'), weights_only=False)['lr'] == [0.02]            # ... and the run's own files are the new ones


def test_fcn_uses_the_loaders_of_the_reference(root, pretrained, tmp_path):
    """fcn/mini_imagenet.py:36-53: RandomResizedCrop(80) + flip for the train split, Resize([92, 92]) -> CenterCrop(80) for val / test; keys given in
    -dataset_args win; the patch modes leave both alone"""
    from fewshot_vit_amd import train_deepemd
    from fewshot_vit_amd.datasets import transforms as T
    args = train_deepemd.parse_args(_argv(root, pretrained, 'fcn', tmp_path))
    train, val = train_deepemd.make_dataset(args, 'train', train=True), train_deepemd.make_dataset(args, 'val')
    assert isinstance(train.transform, T.DeviceRandomResizedCrop)
    assert isinstance(val.transform, T.DeviceTransform) and (val.transform.RH, val.transform.RW, val.transform.crop) == (92, 92, 80)
    index = torch.tensor([0, 7])
    want = T.DeviceTransform((84, 84), (92, 92), 80, val.device)(val.device_images(), index)
    assert torch.equal(val.gather(index), want)
    out = train.gather(index)
    assert out.shape == (2, 3, 80, 80) and train.transform.boxes.shape == (2, 4)
    args.dataset_args = dict(args.dataset_args, resize=[88, 88])
    assert train_deepemd.make_dataset(args, 'val').transform.RH == 88
    grid = train_deepemd.parse_args(_argv(root, pretrained, 'grid', tmp_path))
    assert isinstance(train_deepemd.make_dataset(grid, 'train', train=True).transform, T.DevicePatchGrid)
    assert train_deepemd.make_dataset(grid, 'val').default_transform.RH == 88


def test_eval_driver_seeds_the_sampled_patches_from_its_seed(root, pretrained, tmp_path, monkeypatch):
    from fewshot_vit_amd import datasets, eval_deepemd
    _register()
    made = []
    make = datasets.make
    monkeypatch.setattr(datasets, 'make', lambda *a, **k: made.append(make(*a, **k)) or made[-1])
    argv = ['-encoder', ENCODER, '-numerics', 'parity', '-dataset', 'mini-imagenet', '-dataset_args', '{root_path: %s}' % root, '-set', 'test', '-way', '2',
            '-shot', '1', '-query', '2', '-test_episode', '2', '-episodes_per_launch', '2', '-deepemd', 'sampling', '-num_patch', '3', '-model_dir', pretrained[0]]
    boxes = []
    for seed in ('5', '5', '6'):
        eval_deepemd.main(argv + ['-seed', seed])
        assert made[-1].transform.generator.initial_seed() == int(seed)
        boxes.append(made[-1].transform.boxes.clone())
    assert torch.equal(boxes[0], boxes[1]) and not torch.equal(boxes[0], boxes[2])


def test_five_shot_path_trains_the_encoder_through_the_queries(root, pretrained, tmp_path):
    from fewshot_vit_amd import train_deepemd
    _register()
    argv = _argv(root, pretrained, 'fcn', tmp_path, ['-shot', '2', '-sfc_update_step', '2', '-sfc_bs', '2', '-sfc_lr', '0.1', '-max_epoch', '1'])
    out = train_deepemd.main(argv)
    trlog = torch.load(os.path.join(out['save_path'], 'trlog'), weights_only=False)
    assert out['save_path'].endswith(os.path.join('fcn', '2shot-2way')) and math.isfinite(trlog['train_loss'][0]) and trlog['grad_nan_zeroed'] == [0]
    args = train_deepemd.parse_args(argv)
    dev = torch.device('cuda', torch.cuda.current_device())
    model = train_deepemd.build_model(args).to(dev).train()
    model.sfc_generator = torch.Generator().manual_seed(0)
    ds = train_deepemd.make_dataset(args, 'train', train=True)
    from fewshot_vit_amd.utils import few_shot as fs
    index = torch.tensor([0, 1, 2, 3, 6, 7, 8, 9])                                        # 2 classes x (2 shots + 2 queries)
    x_shot, x_query = fs.split_shot_query(ds.gather(index), 2, 2, 2)
    loss, acc = train_deepemd.task_backward(model, x_shot, x_query, fs.make_nk_label(2, 2).to(dev), 1)
    model.check_status()
    g = model.encoder.stem.conv1.weight.grad
    assert math.isfinite(float(loss)) and g is not None and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0.0


def test_nan_gradient_is_zeroed_and_that_tensor_moves_by_weight_decay_alone(root, pretrained, tmp_path):
    from fewshot_vit_amd import train_deepemd
    from fewshot_vit_amd.utils import few_shot as fs
    _register()
    args = train_deepemd.parse_args(_argv(root, pretrained, 'fcn', tmp_path))
    dev = torch.device('cuda', torch.cuda.current_device())
    model = train_deepemd.build_model(args).to(dev).train()
    optimizer, _ = train_deepemd.make_optimizer(model, args)
    ds = train_deepemd.make_dataset(args, 'train', train=True)
    x_shot, x_query = fs.split_shot_query(ds.gather(torch.tensor([0, 1, 2, 6, 7, 8])), 2, 1, 2)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    train_deepemd.task_backward(model, x_shot, x_query, fs.make_nk_label(2, 2).to(dev), 1)
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    victim = 'encoder.stage2.0.attn.qkv.weight'
    assert victim in grads and float(grads[victim].abs().sum()) > 0.0
    dict(model.named_parameters())[victim].grad.view(-1)[5] = math.nan
    zeroed = train_deepemd.guard_and_step(model, optimizer, True)
    model.check_status()
    assert zeroed.is_cuda and int(zeroed) == 1                                            # what an epoch sums into its log line
    lr, wd = args.lr, 0.0005
    for k, p in model.named_parameters():
        assert bool(torch.isfinite(p).all()), k
        g = torch.zeros_like(grads[k]) if k == victim else grads[k]
        # first Nesterov step: d = g + wd p, buf = d, p' = p - lr (1 + 0.9) d; float64 restatement, fp32 rounding far below the 1e-6 relative gate
        want = before[k].double() - lr * 1.9 * (g.double() + wd * before[k].double())
        err = (p.detach().double() - want).abs().max().item()
        assert err <= 1e-6 * max(1.0, want.abs().max().item()), (k, err)
        assert bool((p.grad == 0).all())                                                  # zero_grad after the step
    moved = (dict(model.named_parameters())[victim].detach() - before[victim]).abs().max().item()
    assert 0.0 < moved <= lr * 1.9 * wd * before[victim].abs().max().item() * (1 + 1e-5)
