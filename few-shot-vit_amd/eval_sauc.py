#!/usr/bin/env python3
"""The reference's `test_few_shot.py --sauc` (test_phase/, meta_tuning_sun_m/test_few_shot.py:42-45,95-112, sun_meta_training/): 2-way episodes, the
queries scored against the single prototype of class 0 (`x_shot[:, 0]`) and reduced by ROC-AUC instead of soft-max.  Same CLI / YAML surface, episode
stream, seeds and launch batching as `test_few_shot.evaluate`, which this module calls when `sauc` is off; with it on, every flush is two encoder
passes and one `ops.proto_auc` launch - no per-episode host sync - and the multi-rank path exchanges the AUCs through the same
`parallel.gather_in_stream_order` call.

`--feature-cache` / `feature_cache=True` (off by default): a flush encodes only the images no earlier flush has seen into a
`feature_table.FeatureTable` and reduces over its rows (`FeatureTable.auc`, fsvit_proto_auc_gather) - the same `va_lst` from at most one encoder pass
per image of the split.  Without `--sauc` the switch is `eval_cached.evaluate`'s.

  python -m fewshot_vit_amd.eval_sauc --config few-shot-vit_amd/configs/test_synthetic.yaml --shot 1 --sauc [--feature-cache]"""
import argparse

import numpy as np
import torch
import yaml

from . import datasets, eval_cached, parallel, test_few_shot, utils
from .datasets.samplers import CategoriesSampler
from .engine import ops
from .feature_table import FeatureTable
from .utils import few_shot as fs


def evaluate(config, shot=1, test_epochs=1, n_batch=2000, ep_per_batch=1, launch_batches=None, numerics=None,
             rank=0, world=1, device=None, log=print, collect_pred=False, sauc=False, feature_cache=False):
    """sauc=False: `eval_cached.evaluate` - `test_few_shot.evaluate` itself with the cache off, plus the two image counters.  sauc=True: the same dict,
    where `va_lst` holds one AUC per EPISODE as the reference's loop appends them (:107-112), `acc` their mean, `ci` their 95 % interval and `loss` the
    untouched averager's value; out['images_requested'] / out['images_encoded'] are the images this rank's flushes read / pushed through the encoder
    (equal without the cache)."""
    if not sauc:                                            # (both drivers carry the same keys, whatever the switches)
        return eval_cached.evaluate(config, shot=shot, test_epochs=test_epochs, n_batch=n_batch, ep_per_batch=ep_per_batch, launch_batches=launch_batches,
                                    numerics=numerics, rank=rank, world=world, device=device, log=log, collect_pred=collect_pred,
                                    feature_cache=feature_cache)
    if collect_pred:
        raise ValueError('collect_pred: --sauc scores against one prototype, there is no per-query arg-max to collect')
    import time
    t_call = time.perf_counter()
    test_few_shot.fix_random_seeds(12345)
    dataset = datasets.make(config['dataset'], **config['dataset_args'])
    t_dataset = time.perf_counter()
    n_way, n_query = 2, 15                                  # (:42-46)
    sampler = CategoriesSampler(dataset.label, n_batch, n_way, shot + n_query, ep_per_batch=ep_per_batch,
                                rank=rank, world_size=world, shard=parallel.sampler_shard(world))
    device = device or torch.device('cuda', torch.cuda.current_device())
    model = test_few_shot.build_model(config, numerics).to(device).eval()
    if rank == 0:
        log('num params: {}'.format(utils.compute_n_params(model)))
    t_model = time.perf_counter()
    engine = model.encoder.engine()
    if launch_batches is None:
        launch_batches = test_few_shot.default_launch_batches(engine, ep_per_batch * n_way * (shot + n_query), engine.img_size, device)
    table = FeatureTable.for_dataset(model, dataset) if feature_cache else None
    n_dense = 0                                             # images the dense route's flushes encoded: the shots of class 0 and all queries

    np.random.seed(12345)                                  # fixes the episode stream (:76)
    out = None
    torch.cuda.synchronize(device)
    t_loop = time.perf_counter()
    aves_va, aves_vl, va_lst = utils.Averager(), utils.Averager(), []      # one pair of averagers and one va_lst across epochs (:72-77)
    for epoch in range(1, test_epochs + 1):
        aucs, pending, last_label = [], [], None

        def flush():
            nonlocal n_dense
            if not pending:
                return
            E = len(pending) * ep_per_batch
            if table is not None:                           # only the images no earlier flush has seen go through the encoder
                aucs.append(table.auc(torch.stack(list(pending)), shot, n_query).view(len(pending), ep_per_batch))
                pending.clear()
                return
            n_dense += E * (shot + n_way * n_query)
            if hasattr(dataset, 'gather'):                  # device-resident dataset: the shots of class 0, then all queries, in one gather
                idx = torch.stack(list(pending)).view(E, n_way, shot + n_query)
                data = dataset.gather(torch.cat([idx[:, 0, :shot].reshape(-1), idx[:, :, shot:].reshape(-1)]))
                x_shot, x_query = data[:E * shot], data[E * shot:]
            else:
                data = torch.stack([torch.stack([dataset[int(i)][0] for i in idx]) for idx in pending])
                data = data.view(E * n_way * (shot + n_query), *data.shape[2:]).to(device, non_blocking=True)
                x_shot, x_query = fs.split_shot_query(data, n_way, shot, n_query, ep_per_batch=E)
                x_shot, x_query = x_shot[:, 0].reshape(-1, *data.shape[1:]), x_query.reshape(-1, *data.shape[1:])      # x_shot[:, 0] (:96)
            f_shot = engine.forward(x_shot).view(E, shot, -1)
            f_query = engine.forward(x_query).view(E, n_way * n_query, -1)        # class-major: the first n_query queries are class 0, the positives
            aucs.append(ops.proto_auc(f_shot, f_query).view(len(pending), ep_per_batch))
            pending.clear()

        ramp = [n for n in (32,) if n < launch_batches]      # a small first launch, as test_few_shot.evaluate
        for idx in sampler:
            pending.append(idx)
            last_label = dataset.label[int(idx[-1])]
            if len(pending) == (ramp[0] if ramp else launch_batches):
                flush()
                if ramp:
                    ramp.pop(0)
        flush()
        if table is not None:
            table.check()                                    # raises if the reduction met a slot outside the table
        mine = torch.cat(aucs).double() if aucs else torch.zeros(0, ep_per_batch, dtype=torch.float64, device=device)
        allv = parallel.gather_in_stream_order(mine, n_batch, rank, world).cpu().numpy()     # the one exchange: [n_batch, ep_per_batch]
        per_batch_items = ep_per_batch * n_way * (shot + n_query)
        for a in allv.reshape(-1).tolist():                  # `aves['va'].add(acc, len(data)); va_lst.append(acc)` per episode (:111-112)
            aves_va.add(a, per_batch_items)
            va_lst.append(a)
        out = dict(acc=aves_va.item(), ci=float(utils.mean_confidence_interval(va_lst)) if len(va_lst) > 1 else float('nan'),
                   loss=aves_vl.item(), n=len(va_lst), last_label=last_label, va_lst=list(va_lst))
        out['loop_seconds'] = time.perf_counter() - t_loop      # the keys of test_few_shot.evaluate's dict, all of them
        out['launch_batches'] = launch_batches
        out['phase_seconds'] = {'dataset': t_dataset - t_call, 'model': t_model - t_dataset, 'engine': t_loop - t_model, 'loop': out['loop_seconds']}
        out['images_requested'], out['images_encoded'] = (table.n_requests, table.n_encoded) if table is not None else (n_dense, n_dense)
        if rank == 0:
            log('test epoch {}: acc={:.2f} +- {:.2f} (%), loss={:.4f} (@{})'.format(epoch, out['acc'] * 100, out['ci'] * 100, out['loss'], last_label))
    return out


def make_parser():
    parser = argparse.ArgumentParser(prog='python -m fewshot_vit_amd.eval_sauc')
    parser.add_argument('--config', default='./configs/test_few_shot.yaml')
    parser.add_argument('--shot', type=int, default=1)
    parser.add_argument('--test-epochs', type=int, default=1)
    parser.add_argument('--sauc', action='store_true', help='2-way episodes scored against the prototype of class 0, reduced by ROC-AUC (the reference flag)')
    parser.add_argument('--gpu', default=None, help='kept for CLI compatibility; use torchrun for multi-GPU')
    parser.add_argument('--episodes', type=int, default=2000, help='number of batches')
    parser.add_argument('--ep-per-batch', type=int, default=1)
    parser.add_argument('--launch-batches', type=int, default=None, help='reference batches per engine launch (default: one encoder chunk)')
    parser.add_argument('--numerics', default=None, choices=[None, 'bf16', 'f16', 'bf16x2', 'f16x2', 'parity'], help="default: FSVIT_NUMERICS or 'bf16'")
    parser.add_argument('--feature-cache', action='store_true',
                        help='encode every image once into a feature table and run the episodes over its rows (same numbers, fewer encoder passes)')
    return parser


def main(argv=None):
    args = make_parser().parse_args(argv)
    config = yaml.load(open(args.config, 'r'), Loader=yaml.FullLoader)
    if args.gpu is not None and ',' not in args.gpu:
        utils.set_gpu(args.gpu)
    rank, world, local = parallel.init_from_env()
    torch.cuda.set_device(local)
    evaluate(config, shot=args.shot, test_epochs=args.test_epochs, n_batch=args.episodes, ep_per_batch=args.ep_per_batch,
             launch_batches=args.launch_batches, numerics=args.numerics, rank=rank, world=world,
             device=torch.device('cuda', local), log=utils.log, sauc=args.sauc, feature_cache=args.feature_cache)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
