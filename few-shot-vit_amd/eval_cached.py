#!/usr/bin/env python3
"""Episodic few-shot evaluation from a feature table: `test_few_shot`'s CLI and `evaluate()` with one more switch, `--feature-cache` /
`feature_cache=True` (off by default: then this module calls `test_few_shot.evaluate`).

With the switch on, the sampler, the seeds, the ramp / launch grouping and the statistics exchange are those of `test_few_shot.evaluate`, but a launch
encodes only the images no earlier launch has seen, into a `feature_table.FeatureTable`, and the episode head reads its rows through the sampler's
index table (fsvit_proto_head_gather): the same `va_lst`, accuracy, CI and loss from 12 000 encoder passes instead of the 160 000 (1-shot) / 200 000
(5-shot) of the reference's 2000-episode protocol.  Multi-GPU: every rank keeps its own table and encodes what its own batches touch (an image two
ranks draw is encoded on both); the sharding and the one exchange stay as they are.

  python -m fewshot_vit_amd.eval_cached --config few-shot-vit_amd/configs/test_synthetic.yaml --shot 5 --feature-cache
"""
import argparse
import time

import numpy as np
import torch
import yaml

from . import datasets, parallel, test_few_shot, utils
from .datasets.samplers import CategoriesSampler
from .feature_table import FeatureTable


def evaluate(config, shot=1, test_epochs=1, n_batch=2000, ep_per_batch=1, launch_batches=None, numerics=None,
             rank=0, world=1, device=None, log=print, collect_pred=False, feature_cache=False):
    """The arguments and the result dict of `test_few_shot.evaluate`, plus out['images_requested'] / out['images_encoded']: the images this rank's batches
    named / pushed through the encoder (equal without the cache)."""
    n_way, n_query = 5, 15
    if not feature_cache:
        out = test_few_shot.evaluate(config, shot=shot, test_epochs=test_epochs, n_batch=n_batch, ep_per_batch=ep_per_batch, launch_batches=launch_batches,
                                     numerics=numerics, rank=rank, world=world, device=device, log=log, collect_pred=collect_pred)
        mine = len(range(rank, n_batch, world)) * test_epochs          # CategoriesSampler.__len__: both shard modes hand rank r the batches r::world
        out['images_requested'] = out['images_encoded'] = mine * ep_per_batch * n_way * (shot + n_query)
        return out
    t_call = time.perf_counter()
    test_few_shot.fix_random_seeds(12345)
    dataset = datasets.make(config['dataset'], **config['dataset_args'])
    t_dataset = time.perf_counter()
    sampler = CategoriesSampler(dataset.label, n_batch, n_way, shot + n_query, ep_per_batch=ep_per_batch,
                                rank=rank, world_size=world, shard=parallel.sampler_shard(world))
    device = device or torch.device('cuda', torch.cuda.current_device())
    model = test_few_shot.build_model(config, numerics).to(device).eval()
    if rank == 0:
        log('num params: {}'.format(utils.compute_n_params(model)))
    t_model = time.perf_counter()
    engine = model.encoder.engine()
    temp = float(model.temp.detach()) if isinstance(model.temp, torch.Tensor) else float(model.temp)
    if launch_batches is None:
        launch_batches = test_few_shot.default_launch_batches(engine, ep_per_batch * n_way * (shot + n_query), engine.img_size, device)
    table = FeatureTable.for_dataset(model, dataset)

    np.random.seed(12345)                                  # fixes the episode stream (test_few_shot.py:76)
    out = None
    torch.cuda.synchronize(device)
    t_loop = time.perf_counter()
    aves_va, aves_vl, va_lst = utils.Averager(), utils.Averager(), []      # one pair of averagers and one va_lst across epochs, as test_few_shot.evaluate
    for epoch in range(1, test_epochs + 1):
        accs, losses, last_label = [], [], None
        pending, preds = [], []

        def flush():
            if not pending:
                return
            G = len(pending)
            logits, acc, loss = table.episodes(torch.stack(list(pending)), n_way, shot, n_query, temp, model.method)
            if collect_pred:
                preds.append(logits.argmax(-1).to(torch.uint8).cpu())
            accs.append(acc.view(G, ep_per_batch).mean(dim=1))       # per reference batch
            losses.append(loss.view(G, ep_per_batch).mean(dim=1))
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
        table.check()                                        # raises if the head met a slot outside the table
        mine = torch.stack([torch.cat(accs), torch.cat(losses)], dim=1).double() if accs else torch.zeros(0, 2, dtype=torch.float64, device=device)
        allv = parallel.gather_in_stream_order(mine, n_batch, rank, world).cpu().numpy()     # the one exchange
        va_lst.extend(allv[:, 0].tolist())
        per_batch_items = ep_per_batch * n_way * (shot + n_query)
        for a, l in allv:
            aves_va.add(a, per_batch_items)
            aves_vl.add(l, per_batch_items)
        out = dict(acc=aves_va.item(), ci=float(utils.mean_confidence_interval(va_lst)) if len(va_lst) > 1 else float('nan'),
                   loss=aves_vl.item(), n=len(va_lst), last_label=last_label, va_lst=list(va_lst))
        if collect_pred:
            out['pred'] = torch.cat(preds) if preds else torch.zeros(0, n_way * n_query, dtype=torch.uint8)
        out['loop_seconds'] = time.perf_counter() - t_loop      # the keys of test_few_shot.evaluate's dict, all of them
        out['launch_batches'] = launch_batches
        out['phase_seconds'] = {'dataset': t_dataset - t_call, 'model': t_model - t_dataset, 'engine': t_loop - t_model, 'loop': out['loop_seconds']}
        out['images_requested'], out['images_encoded'] = table.n_requests, table.n_encoded
        if rank == 0:
            log('test epoch {}: acc={:.2f} +- {:.2f} (%), loss={:.4f} (@{})'.format(
                epoch, out['acc'] * 100, out['ci'] * 100, out['loss'], last_label))
    return out


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    parser.add_argument('--config', default='./configs/test_few_shot.yaml')
    parser.add_argument('--shot', type=int, default=1)
    parser.add_argument('--test-epochs', type=int, default=1)
    parser.add_argument('--gpu', default=None, help='kept for CLI compatibility; use torchrun for multi-GPU')
    parser.add_argument('--episodes', type=int, default=2000, help='number of batches (reference: 2000)')
    parser.add_argument('--ep-per-batch', type=int, default=1)
    parser.add_argument('--launch-batches', type=int, default=None, help='reference batches per launch (default: as test_few_shot)')
    parser.add_argument('--numerics', default=None, choices=[None, 'bf16', 'f16', 'bf16x2', 'f16x2', 'parity'])
    parser.add_argument('--feature-cache', action='store_true',
                        help='encode every image once into a feature table and run the episodes over its rows (same numbers, fewer encoder passes)')
    args = parser.parse_args(argv)
    config = yaml.load(open(args.config, 'r'), Loader=yaml.FullLoader)
    if args.gpu is not None and ',' not in args.gpu:
        utils.set_gpu(args.gpu)
    rank, world, local = parallel.init_from_env()
    torch.cuda.set_device(local)
    evaluate(config, shot=args.shot, test_epochs=args.test_epochs, n_batch=args.episodes, ep_per_batch=args.ep_per_batch,
             launch_batches=args.launch_batches, numerics=args.numerics, rank=rank, world=world,
             device=torch.device('cuda', local), log=utils.log, feature_cache=args.feature_cache)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
