#!/usr/bin/env python3
"""SUN-D evaluation driver: the reference's meta_tuning_sun_d/eval.py on the HIP DeepEMD head (models/deepemd.py, csrc/emd_head.hip).

  python -m fewshot_vit_amd.eval_deepemd -way 5 -shot 1 -query 15 -test_episode 5000 -model_dir max_acc.pth
  python -m fewshot_vit_amd.eval_deepemd -shot 5 -test_episode 600 -sfc_lr 100 -sfc_update_step 100 -sfc_bs 4

Flags are the reference's (eval.py:18-50).  Differences: datasets come through this package's `datasets.make` (`-dataset`, default the synthetic
stand-in; `-dataset_args` a YAML dict), episodes are drawn by this package's CategoriesSampler (class-major batches; SUN-D's own `randperm` sampler
stream is not reproduced), `-episodes_per_launch` episodes go through the encoder and the head per launch - one episode's 375
transportation problems are fewer than the GPU's SIMDs -, and the solver's status is checked once per evaluation.  Without `-model_dir` the encoder
carries the procedural stand-in weights.  `-deepemd grid` / `sampling` build the dataset with the matching patch loader (`-patch_list`, `-patch_ratio`,
`-num_patch`; they need a dataset of raw images: 'mini-imagenet', 'tiered-imagenet', 'synthetic-images') and seed its generator from `-seed`; `-set`
overrides the split of `-dataset_args`; `-norm_stats sund` normalises with the statistics of the reference's SUN-D loaders.  `-deepemd fcn` keeps the
dataset's own eval transform: the reference's fcn loader (Resize([92, 92]) -> CenterCrop(80)), which train_deepemd applies to its val / test splits by
itself, is `-dataset_args '{..., resize: [92, 92]}'` here.  `-feature_cache` (off by default; fcn and grid) encodes every image once into a
`feature_table.TokenTable` and lets the head read its rows by slot number (fsvit_emd_head_gather): the same accuracies, bit for bit.  Reports the mean accuracy and its 95 % interval over episodes (eval.py:100-104)."""
import argparse

import numpy as np
import torch
import yaml

from . import datasets, models, utils
from .datasets.samplers import CategoriesSampler
from .episodic import gather_images, launch_groups
from .utils import few_shot as fs


def load_params(model, path):
    """load_model (Models/utils.py): the checkpoint's `model_sd` / `params` with the DataParallel prefix removed, encoder keys only."""
    from .models.deepemd import load_encoder_params
    return load_encoder_params(model, path)


def patch_dataset_args(args, train=False):
    """The dataset keywords of `-deepemd`: fcn -> whole images; grid -> the patch pyramid (random ratios / flips for the train split only);
    sampling -> random patches for every split.  `-norm_stats sund` selects the statistics of the reference's SUN-D loaders."""
    from .datasets.transforms import SUND_MEAN, SUND_STD
    kw = {}
    if args.deepemd == 'grid':
        kw.update(patches='grid', patch_list=tuple(args.patch_list), patch_ratio=args.patch_ratio, patch_train=bool(train))
    elif args.deepemd == 'sampling':
        kw.update(patches='sampling', num_patch=args.num_patch)
    if args.norm_stats == 'sund':
        kw.update(mean=SUND_MEAN, std=SUND_STD)
    return kw


def parse_patch_list(text):
    return [int(x) for x in str(text).split(',')]


def build_model(args):
    model = models.make('deepemd', encoder=args.encoder, encoder_args={'numerics': args.numerics} if args.numerics else {},
                        temperature=args.temperature, metric=args.metric, norm=args.norm, deepemd=args.deepemd, feature_pyramid=args.feature_pyramid,
                        solver=args.solver, sfc_lr=args.sfc_lr, sfc_update_step=int(args.sfc_update_step), sfc_bs=args.sfc_bs, sfc_fused=args.sfc_fused)
    if args.model_dir:
        return load_params(model, args.model_dir)
    from . import synthetic
    model.load_state_dict(synthetic.synthetic_checkpoint_sd({k: tuple(v.shape) for k, v in model.state_dict().items()}, calib=args.encoder))
    return model


def evaluate(args, log=print, collect=None):
    """-> dict(acc, ci, n).  `collect`, when a list, receives the per-episode accuracies (per cent, float64, in episode order).  With `-feature_cache`
    every image is encoded once into a feature_table.TokenTable and the head reads its rows through slot numbers - the same accuracies from
    `n_encoded` encoder passes instead of `n_requests` (both are then added to the dict)."""
    feature_cache = bool(getattr(args, 'feature_cache', False))
    if feature_cache and args.deepemd == 'sampling':
        raise ValueError('fsvit: -feature_cache needs one node set per image; -deepemd sampling draws random patches at every visit (use fcn or grid)')
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    device = torch.device('cuda', torch.cuda.current_device())
    gen = torch.Generator().manual_seed(args.seed)            # the SFC permutations (torch.randperm per step and episode)
    dataset_args = dict(args.dataset_args)
    if args.set is not None:
        dataset_args['split'] = args.set
    extra = patch_dataset_args(args)
    if extra and args.dataset == 'synthetic-episodes':
        raise ValueError("fsvit: 'synthetic-episodes' yields finished float images; the patch modes and -norm_stats need raw images ('synthetic-images')")
    dataset = datasets.make(args.dataset, **{**dataset_args, **extra})
    transform = getattr(dataset, 'transform', None)
    if hasattr(transform, 'manual_seed'):
        transform.manual_seed(args.seed)                      # -deepemd sampling: the random patches follow -seed, as the episodes do
    model = build_model(args).to(device).eval()
    model.sfc_generator = gen
    sampler = CategoriesSampler(dataset.label, args.test_episode, args.way, args.shot + args.query)
    label = fs.make_nk_label(args.way, args.query).to(device)
    accs = []
    table = None
    if feature_cache:
        from .feature_table import TokenTable
        table = TokenTable.for_dataset(model, dataset)

    for group in launch_groups(sampler, args.episodes_per_launch):
        idx = torch.stack(group).view(-1)
        with torch.no_grad():
            if table is not None:
                logits = table.logits(idx, args.way, args.shot, args.query, model)
            else:
                x_shot, x_query = fs.split_shot_query(gather_images(dataset, idx, device), args.way, args.shot, args.query, ep_per_batch=len(group))
                logits = model(x_shot, x_query)
        accs.append((logits.argmax(dim=-1) == label).float().mean(dim=1))
    model.check_status()                                     # the one synchronisation: raises if any transportation problem hit a loop bound
    if table is not None:
        table.check()
    acc = torch.cat(accs).double().cpu().numpy() * 100.0
    if collect is not None:
        collect.extend(acc.tolist())
    mean = float(acc.mean())
    ci = float(utils.mean_confidence_interval(acc)) if len(acc) > 1 else float('nan')
    log('test Acc {:.4f}'.format(mean))
    log('Test Acc {:.4f} + {:.4f}'.format(mean, ci))
    out = dict(acc=mean, ci=ci, n=len(acc))
    if table is not None:
        out.update(n_encoded=table.n_encoded, n_requests=table.n_requests)
    return out


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('-encoder', '--backbone', dest='encoder', default='visformer_micro_80')
    p.add_argument('-way', type=int, default=5)
    p.add_argument('-shot', type=int, default=1)
    p.add_argument('-query', type=int, default=15)
    p.add_argument('-dataset', default='synthetic-episodes')
    p.add_argument('-dataset_args', type=yaml.safe_load, default={'split': 'test', 'noise': 1.0, 'seed': 0})
    p.add_argument('-temperature', type=float, default=12.5)
    p.add_argument('-metric', default='cosine')
    p.add_argument('-norm', default='center')
    p.add_argument('-deepemd', default='fcn', choices=['fcn', 'grid', 'sampling'])
    p.add_argument('-feature_pyramid', default=None)
    p.add_argument('-num_patch', type=int, default=9)
    p.add_argument('-patch_list', type=parse_patch_list, default=[2, 3])
    p.add_argument('-patch_ratio', type=float, default=2.0)
    p.add_argument('-set', default=None, choices=[None, 'train', 'val', 'test'])
    p.add_argument('-norm_stats', default='imagenet', choices=['imagenet', 'sund'])
    p.add_argument('-solver', default='opencv')
    p.add_argument('-sfc_lr', type=float, default=100)
    p.add_argument('-sfc_update_step', type=float, default=100)
    p.add_argument('-sfc_bs', type=int, default=4)
    p.add_argument('-sfc_fused', action='store_true', help='5-shot: run the SFC fine-tune as one on-device loop per episode (emd_sfc_kernel)')
    p.add_argument('-test_episode', type=int, default=5000)
    p.add_argument('-model_dir', default=None)
    p.add_argument('-seed', type=int, default=1)
    p.add_argument('-numerics', default=None, choices=[None, 'bf16', 'f16', 'bf16x2', 'f16x2', 'parity'])
    p.add_argument('-episodes_per_launch', type=int, default=16)
    p.add_argument('-feature_cache', action='store_true',
                   help='encode every image once into a token-map table (fcn, grid); the head reads its rows by slot number - same accuracies')
    return p.parse_args(argv)


def main(argv=None):
    return evaluate(parse_args(argv), log=utils.log if hasattr(utils, 'log') else print)


if __name__ == '__main__':
    main()
