#!/usr/bin/env python3
"""SUN-D meta-tuning driver: the loop of the reference's meta_tuning_sun_d/train_meta.py:95-277 on the HIP DeepEMD head (models/deepemd.py,
csrc/emd_head.hip), the HIP encoder trainer, the Nesterov SGD kernel and the on-device NaN-gradient guard (csrc/optim.hip).

  python -m fewshot_vit_amd.train_deepemd -dataset mini-imagenet -dataset_args '{root_path: ./materials/mini-imagenet}' -deepemd grid \\
      -pretrain_dir sun_m/max-va.pth -way 5 -shot 1 -query 15 -norm_stats sund

Flags and defaults are the reference's (train_meta.py:20-64).  One epoch = val_frequency * bs training tasks of ONE episode per forward (BatchNorm
statistics span one episode's images or patches, as in the reference), loss = CE / bs, backward, `utils.detect_grad_nan` after every backward,
`optimizer.step(); zero_grad()` every bs tasks; then a validation pass under `model.eval()`, `max_acc.pth` on `va >= max_acc`, `StepLR.step()`.
The optimizer is FsvitSGD(lr, momentum 0.9, weight_decay 5e-4, nesterov=True) (train_meta.py:115-116).  After the last epoch `max_acc.pth` is
reloaded and scored on the test split (`Test Acc m + pm`, compute_confidence_interval: 1.96 std / sqrt(n)).

`-deepemd` selects the data loader too: fcn -> whole images (on the raw-image datasets 'mini-imagenet', 'tiered-imagenet', 'synthetic-images' as
the reference's fcn loader: RandomResizedCrop(80) + flip for the train split, Resize([92, 92]) -> CenterCrop(80) for val / test; `augment` /
`resize` keys in `-dataset_args` win; other datasets keep their own transform); grid -> the patch pyramid, random ratios and flips for the train split only;
sampling -> random patches for every split.  Without `-random_val_task` the index stream, the patch generator and the SFC permutations of the
validation pass are re-seeded every epoch, so the validation set is fixed (the reference materialises its val loader once).
`-eval_feature_cache` (off by default; fcn and grid) runs the validation and test passes from a `feature_table.TokenTable` per split, emptied before
every pass because the weights have moved: every image a pass draws is encoded once, the figures are the same; the training step is untouched.

Differences from the reference: a single process on a single GPU (no DataParallel); datasets come through this package's `datasets.make`
(`-dataset`, `-dataset_args` a YAML dict; `-set` names the validation split) and episodes from this package's CategoriesSampler (class-major
batches; SUN-D's own `randperm` sampler stream is not reproduced); validation and test run `-episodes_per_launch` episodes per launch; the
zeroed-gradient count and the solver status are read from the device once per epoch; no tensorboard, no tqdm; `-backbone` / `-encoder` names a
registered encoder, `-numerics` its arithmetic, `-norm_stats` the normalisation statistics, `-save_root` replaces the literal `checkpoint`.
An existing save directory is kept (the reference's `ensure_path` removes nothing either): a run overwrites the files it writes and leaves the rest.
Without `-pretrain_dir` the encoder carries the procedural stand-in weights, as in eval_deepemd."""
import argparse
import os

import numpy as np
import torch
import torch.nn.functional as F
import yaml

from . import datasets, models, utils
from .datasets.samplers import CategoriesSampler
from .episodic import gather_images, launch_groups
from .eval_deepemd import parse_patch_list, patch_dataset_args
from .models.deepemd import load_encoder_params
from .utils import few_shot as fs


def compute_confidence_interval(data):
    """Models/utils.py:62-72: mean and 1.96 std / sqrt(n) of the per-episode accuracies."""
    a = 1.0 * np.array(data)
    return float(np.mean(a)), float(1.96 * (np.std(a) / np.sqrt(len(a))))


def build_model(args):
    model = models.make('deepemd', encoder=args.encoder, encoder_args={'numerics': args.numerics} if args.numerics else {},
                        temperature=args.temperature, metric=args.metric, norm=args.norm, deepemd=args.deepemd, solver=args.solver,
                        sfc_lr=args.sfc_lr, sfc_update_step=int(args.sfc_update_step), sfc_bs=args.sfc_bs)
    if args.pretrain_dir:
        return load_encoder_params(model, args.pretrain_dir)
    from . import synthetic
    model.load_state_dict(synthetic.synthetic_checkpoint_sd({k: tuple(v.shape) for k, v in model.state_dict().items()}, calib=args.encoder))
    return model


RAW_IMAGE_DATASETS = ('mini-imagenet', 'tiered-imagenet', 'synthetic-images')      # uint8 tables behind the `augment` / `resize` / `patches` keywords


def make_dataset(args, split, train=False):
    extra = patch_dataset_args(args, train=train)
    if extra and args.dataset == 'synthetic-episodes':
        raise ValueError("fsvit: 'synthetic-episodes' yields finished float images; the patch modes and -norm_stats need raw images ('synthetic-images')")
    kw = {**args.dataset_args, 'split': split, **extra}
    if args.deepemd == 'fcn' and args.dataset in RAW_IMAGE_DATASETS:
        # fcn/mini_imagenet.py:36-53: RandomResizedCrop(80) + flip for the train split, Resize([92, 92]) -> CenterCrop(80) for val / test
        # (keys given in -dataset_args win)
        if train:
            kw.setdefault('augment', 'resize')
        else:
            kw.setdefault('resize', [92, 92])
    return datasets.make(args.dataset, **kw)


def make_optimizer(model, args):
    optimizer = utils.FsvitSGD(model.parameters(), args.lr, momentum=0.9, weight_decay=0.0005, nesterov=True)
    return optimizer, torch.optim.lr_scheduler.StepLR(optimizer, step_size=args.step_size, gamma=args.gamma)


def _seed_dataset(dataset, seed):
    transform = getattr(dataset, 'transform', None)
    if hasattr(transform, 'manual_seed'):
        transform.manual_seed(seed)


def task_backward(model, x_shot, x_query, label, bs):
    """One training task: logits of one episode, loss = CE / bs accumulated into the gradients -> (loss / bs, accuracy), device scalars."""
    logits = model(x_shot, x_query).view(-1, x_shot.shape[1])
    total_loss = F.cross_entropy(logits, label) / bs
    total_loss.backward()
    return total_loss.detach(), (logits.detach().argmax(dim=1) == label).float().mean()


def guard_and_step(model, optimizer, step_now):
    """detect_grad_nan after every backward; the optimizer steps every bs tasks -> device scalar, the number of gradient tensors zeroed."""
    zeroed = utils.detect_grad_nan(model)
    if step_now:
        optimizer.step()
        optimizer.zero_grad(set_to_none=False)        # the gradients keep their addresses: neither pointer table is uploaded again
    return zeroed


def train_epoch(model, optimizer, dataset, args, epoch, device):
    """val_frequency * bs tasks -> (mean loss / bs, mean accuracy, gradient tensors zeroed by the guard); one host read at the end."""
    model.train()
    optimizer.zero_grad(set_to_none=False)
    np.random.seed(args.seed + epoch)
    sampler = CategoriesSampler(dataset.label, args.val_frequency * args.bs, args.way, args.shot + args.query)
    label = fs.make_nk_label(args.way, args.query).to(device)
    sums = torch.zeros(2, dtype=torch.float64, device=device)
    zeroed = torch.zeros((), dtype=torch.int64, device=device)
    n = 0
    for n, idx in enumerate(sampler, 1):
        x_shot, x_query = fs.split_shot_query(gather_images(dataset, idx, device), args.way, args.shot, args.query)
        loss, acc = task_backward(model, x_shot, x_query, label, args.bs)
        sums += torch.stack([loss, acc]).double()
        zeroed += guard_and_step(model, optimizer, n % args.bs == 0)
    model.check_status()
    tl, ta = (sums / max(n, 1)).tolist()
    return tl, ta, int(zeroed.item())


def evaluate(model, dataset, args, n_episode, device, seed=None, table=None):
    """n_episode episodes under model.eval(), episodes_per_launch per launch -> (mean loss, per-episode accuracies in [0, 1] as a numpy array).
    `seed` fixes the index stream, the dataset's patch generator and the SFC permutations.  `table` (a feature_table.TokenTable over `dataset`,
    -eval_feature_cache) is reset - the weights have changed since the last pass - and every image the pass draws is encoded once; same figures."""
    model.eval()
    if table is not None:
        table.reset()
    if seed is not None:
        np.random.seed(seed)
        _seed_dataset(dataset, seed)
        model.sfc_generator = torch.Generator().manual_seed(seed)
    sampler = CategoriesSampler(dataset.label, n_episode, args.way, args.shot + args.query)
    losses, accs = [], []
    for group in launch_groups(sampler, args.episodes_per_launch):
        G = len(group)
        idx = torch.stack(group).view(-1)
        label = fs.make_nk_label(args.way, args.query, ep_per_batch=G).to(device)
        with torch.no_grad():
            if table is not None:
                logits = table.logits(idx, args.way, args.shot, args.query, model).view(-1, args.way)
            else:
                x_shot, x_query = fs.split_shot_query(gather_images(dataset, idx, device), args.way, args.shot, args.query, ep_per_batch=G)
                logits = model(x_shot, x_query).view(-1, args.way)
        losses.append(F.cross_entropy(logits, label, reduction='none').view(G, -1).mean(dim=1))
        accs.append((logits.argmax(dim=1) == label).float().view(G, -1).mean(dim=1))
    model.check_status()
    if table is not None:
        table.check()
    return float(torch.cat(losses).double().mean().item()), torch.cat(accs).double().cpu().numpy()


def make_eval_table(model, dataset, args):
    """-eval_feature_cache: a token-map table over a val / test split (None without the flag); `evaluate` resets it before every pass."""
    if not getattr(args, 'eval_feature_cache', False):
        return None
    from .feature_table import TokenTable
    was_training = model.training
    try:
        return TokenTable.for_dataset(model.eval(), dataset)
    finally:
        model.train(was_training)


def save_path_of(args):
    path = os.path.join(args.save_root, args.dataset, args.deepemd, '%dshot-%dway' % (args.shot, args.way))
    return os.path.join(path, args.extra_dir) if args.extra_dir is not None else path


def run(args, log=print):
    if getattr(args, 'eval_feature_cache', False) and args.deepemd == 'sampling':
        raise ValueError('fsvit: -eval_feature_cache needs one node set per image; -deepemd sampling draws random patches at every visit (use fcn or grid)')
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    device = torch.device('cuda', torch.cuda.current_device())
    save_path = save_path_of(args)
    utils.ensure_path(save_path, remove=False)        # an earlier run's files stay until this run writes its own over them
    model = build_model(args).to(device)
    model.sfc_generator = torch.Generator().manual_seed(args.seed)
    trainset, valset = make_dataset(args, 'train', train=True), make_dataset(args, args.set)
    _seed_dataset(trainset, args.seed)
    _seed_dataset(valset, args.seed)
    val_table = make_eval_table(model, valset, args)
    if not args.random_val_task:
        log('fix val set for all epochs')
    optimizer, lr_scheduler = make_optimizer(model, args)

    def save_model(name):
        torch.save(dict(params=model.state_dict()), os.path.join(save_path, name + '.pth'))

    trlog = dict(args=vars(args), train_loss=[], val_loss=[], train_acc=[], val_acc=[], lr=[], grad_nan_zeroed=[], max_acc=0.0, max_acc_epoch=0)
    result_list = [save_path]
    timer = utils.Timer()
    for epoch in range(1, args.max_epoch + 1):
        timer.s()
        lr = optimizer.param_groups[0]['lr']
        tl, ta, zeroed = train_epoch(model, optimizer, trainset, args, epoch, device)
        vl, va = evaluate(model, valset, args, args.val_episode, device, seed=None if args.random_val_task else args.seed,
                          table=val_table)
        va = float(va.mean())
        log('epo {}, lr {:.6g}, train loss={:.4f} acc={:.4f}, val loss={:.4f} acc={:.4f}, nan-gradient tensors zeroed {}'.format(
            epoch, lr, tl, ta, vl, va, zeroed))
        if va >= trlog['max_acc']:
            log('*********A better model is found*********')
            trlog['max_acc'], trlog['max_acc_epoch'] = va, epoch
            save_model('max_acc')
        for k, v in (('train_loss', tl), ('train_acc', ta), ('val_loss', vl), ('val_acc', va), ('lr', lr), ('grad_nan_zeroed', zeroed)):
            trlog[k].append(v)
        result_list.append('epoch:%03d,training_loss:%.5f,training_acc:%.5f,val_loss:%.5f,val_acc:%.5f' % (epoch, tl, ta, vl, va))
        torch.save(trlog, os.path.join(save_path, 'trlog'))
        if args.save_all:
            save_model('epoch-%d' % epoch)
            torch.save(optimizer.state_dict(), os.path.join(save_path, 'optimizer_latest.pth'))
        log('best epoch {}, best val acc={:.4f}'.format(trlog['max_acc_epoch'], trlog['max_acc']))
        log('This epoch takes {}, still need {} to finish'.format(utils.time_str(timer.t()), utils.time_str(timer.t() * (args.max_epoch - epoch))))
        lr_scheduler.step()

    # Test phase (train_meta.py:237-277)
    testset = make_dataset(args, 'test')
    model.load_state_dict(torch.load(os.path.join(save_path, 'max_acc.pth'), map_location='cpu')['params'])
    test_table = make_eval_table(model, testset, args)
    _, acc = evaluate(model, testset, args, args.test_episode, device, seed=args.seed, table=test_table)
    m, pm = compute_confidence_interval(acc * 100.0)
    result_list.append('Val Best Epoch {},\nbest val Acc {:.4f}, \nbest est Acc {:.4f}'.format(trlog['max_acc_epoch'], trlog['max_acc'], m))
    result_list.append('Test Acc {:.4f} + {:.4f}'.format(m, pm))
    log(result_list[-2])
    log(result_list[-1])
    with open(os.path.join(save_path, 'results.txt'), 'w') as f:
        f.write('\n'.join(result_list) + '\n')
    out = dict(max_acc=trlog['max_acc'], max_acc_epoch=trlog['max_acc_epoch'], test_acc=m, test_ci=pm, save_path=save_path)
    if val_table is not None:                          # the counters of the last pass over each split (every pass starts from an empty table)
        out['eval_cache'] = {name: dict(n_encoded=t.n_encoded, n_requests=t.n_requests) for name, t in (('val', val_table), ('test', test_table))}
    return out


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('-dataset', default='synthetic-images')
    p.add_argument('-dataset_args', type=yaml.safe_load, default={})
    p.add_argument('-set', default='val', choices=['test', 'val'], help='the set used for validation')
    p.add_argument('-bs', type=int, default=1, help='batch size of tasks')
    p.add_argument('-max_epoch', type=int, default=100)
    p.add_argument('-lr', type=float, default=0.0005)
    p.add_argument('-temperature', type=float, default=12.5)
    p.add_argument('-step_size', type=int, default=10)
    p.add_argument('-gamma', type=float, default=0.5)
    p.add_argument('-val_frequency', type=int, default=50)
    p.add_argument('-random_val_task', action='store_true', help='random samples tasks for validation at each epoch')
    p.add_argument('-save_all', action='store_true', help='save models on each epoch')
    p.add_argument('-way', type=int, default=5)
    p.add_argument('-shot', type=int, default=1)
    p.add_argument('-query', type=int, default=15, help='number of query image per class')
    p.add_argument('-val_episode', type=int, default=2000)
    p.add_argument('-test_episode', type=int, default=2000)
    p.add_argument('-pretrain_dir', default=None)
    p.add_argument('-metric', default='cosine')
    p.add_argument('-norm', default='center')
    p.add_argument('-deepemd', default='sampling', choices=['fcn', 'grid', 'sampling'])
    p.add_argument('-num_patch', type=int, default=9)
    p.add_argument('-patch_list', type=parse_patch_list, default=[2, 3], help='the size of grids at every image-pyramid level')
    p.add_argument('-patch_ratio', type=float, default=2.0, help='scale the patch to incorporate context around the patch')
    p.add_argument('-solver', default='opencv')
    p.add_argument('-sfc_lr', type=float, default=0.1)
    p.add_argument('-sfc_update_step', type=float, default=100)
    p.add_argument('-sfc_bs', type=int, default=4)
    p.add_argument('-extra_dir', default=None)
    p.add_argument('-seed', type=int, default=12345)
    p.add_argument('-encoder', '-backbone', '--backbone', dest='encoder', default='visformer_micro_80')
    p.add_argument('-numerics', default=None, choices=[None, 'bf16', 'f16', 'bf16x2', 'f16x2', 'parity'])
    p.add_argument('-norm_stats', default='imagenet', choices=['imagenet', 'sund'])
    p.add_argument('-episodes_per_launch', type=int, default=16, help='validation / test episodes per launch (training runs one per forward)')
    p.add_argument('-eval_feature_cache', action='store_true',
                   help='validation / test: encode every image of a pass once into a token-map table (fcn, grid) - same figures')
    p.add_argument('-save_root', default='checkpoint')
    return p.parse_args(argv)


def main(argv=None):
    return run(parse_args(argv), log=utils.log)


if __name__ == '__main__':
    main()
