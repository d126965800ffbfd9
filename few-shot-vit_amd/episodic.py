"""Episodic evaluation, once: the launch loop and the result path behind `test_few_shot.evaluate`, `eval_cached.evaluate` and `eval_sauc.evaluate`,
and the helpers the other drivers' evaluation blocks share.

`evaluate` is the reference's protocol (test_phase/test_few_shot.py:36-134): seeds 12345, `n_way`-way `shot`-shot episodes with 15 queries per class,
one pair of averagers and one `va_lst` across epochs, `acc +- 95 % CI`.  Many batches go through the HIP engine per launch (`launch_groups`), every
rank keeps its statistics on the device and exchanges them once per epoch (`parallel.gather_in_stream_order`).  What differs between the drivers is
a ROUTE - what one launch does with a group of index batches - and a REDUCTION - how the exchanged rows feed the averagers:

  route         head call                       images
  proto_dense   engine.meta_baseline_forward    shots-then-queries gather, x_shot / x_query are views of it
  proto_table   FeatureTable.episodes           table rows; only images no earlier launch has seen are encoded
  auc_dense     ops.proto_auc                   two encoder passes: the shots of class 0, all queries
  auc_table     FeatureTable.auc                table rows

  reduce_batches    one row (acc, loss) per batch; both averagers and va_lst are fed per batch
  reduce_episodes   one AUC per episode; va_lst and the accuracy averager are fed per episode, the loss averager stays untouched (--sauc)

A route is made once per call, `make(ctx) -> (launch, finish)`: `launch(group) -> (rows [len(group), k] on the device, pred or None)` and
`finish() -> (images requested, images encoded)` by this rank so far, called once per epoch after the last launch (the tables' one host read)."""
import argparse
import time
from types import SimpleNamespace

import numpy as np
import torch
import yaml

from . import datasets, parallel, utils
from .datasets.samplers import CategoriesSampler


def fix_random_seeds(seed=12345):
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)


def gather_images(dataset, index, device):
    """Images of these indices on the device: `dataset.gather` (device-resident dataset: gather + transform on the GPU), else `dataset[i][0]` stacked."""
    if hasattr(dataset, 'gather'):
        return dataset.gather(index)
    return torch.stack([dataset[int(i)][0] for i in index]).to(device, non_blocking=True)


def head_temp(model, on_device=False):
    """The temperature of a MetaBaseline as the head takes it: a host float, or with `on_device` the parameter itself (read by the kernel, no sync)."""
    if isinstance(model.temp, torch.Tensor):
        return model.temp.detach() if on_device else float(model.temp.detach())
    return float(model.temp)


def launch_groups(sampler, launch_batches, ramp=()):
    """The sampler's index batches in lists of `launch_batches`, in stream order; while `ramp` lasts the next list closes at ramp[0] batches instead.
    What is left at the end of the stream is one more list; an empty sampler yields nothing."""
    ramp, pending = list(ramp), []
    for idx in sampler:
        pending.append(idx)
        if len(pending) == (ramp[0] if ramp else launch_batches):
            yield pending                                   # the caller's flush: the launch runs before the next batch is drawn
            pending = []
            if ramp:
                ramp.pop(0)
    if pending:
        yield pending


def table_episode_logits(table, sampler, n_way, n_shot, n_query, temp, method):
    """The logits of one whole evaluation from a feature_table.FeatureTable: the sampler's epoch is drawn first (the draws do not depend on the encoder
    and the sampler is the loop's only consumer of np.random), the table encodes the images it has not seen, the head runs over all episodes in one
    launch, then `table.check()` -> [n_batches, ep_per_batch * n_way * n_query, n_way]; no batches: an empty [0, 0, n_way]."""
    batches = [idx for idx in sampler]
    if not batches:
        return torch.zeros(0, 0, n_way, device=table.device)
    idx = torch.stack(batches)
    logits, _, _ = table.episodes(idx, n_way, n_shot, n_query, temp, method)
    table.check()
    return logits.view(idx.shape[0], -1, n_way)


def build_model(config, numerics=None):
    """`load` / `load_encoder` handling of test_few_shot.py:56-63."""
    from . import models                                   # (models.meta_baseline imports head_temp from this module)
    if config.get('load') is None:
        model = models.make('meta-baseline', encoder=None)
    else:
        model = models.load(torch.load(config['load'], map_location='cpu'))
    if config.get('load_encoder') is not None:
        model.encoder = models.load(torch.load(config['load_encoder'], map_location='cpu')).encoder
    if config.get('synthetic_checkpoint'):            # offline stand-in: procedural weights + calibrated BN
        from . import synthetic
        model = models.make('meta-baseline', encoder=config['synthetic_checkpoint'], encoder_args={})
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        model.load_state_dict(synthetic.synthetic_checkpoint_sd(shapes, calib=config['synthetic_checkpoint']))
    if model.encoder is None:
        raise ValueError('config must provide load, load_encoder or synthetic_checkpoint')
    if numerics is not None:
        model.encoder.numerics = numerics
    return model


def default_launch_batches(engine, images_per_batch, img_size, device):
    """Reference batches (`ep_per_batch` episodes each) per engine launch when the caller does not say: one encoder chunk's worth of images (12 800
    for the Visformer: the size the persistent kernels are tuned and benched at), bounded so that the launch's fp32 input and its
    uint8 -> fp32 transform output stay within a quarter of the free device memory."""
    n_img = engine.chunk_images
    free = torch.cuda.mem_get_info(device)[0]
    n_img = min(n_img, max(images_per_batch, int(0.25 * free) // (3 * img_size * img_size * 4)))
    return max(1, n_img // images_per_batch)


# ---- routes: ctx carries dataset, model, engine, device, n_way, shot, n_query, ep_per_batch, collect_pred
def _proto_rows(ctx, G, logits, acc, loss):
    # per-query arg-max of every episode (agreement tests between numerics modes); acc / loss per reference batch
    pred = logits.argmax(-1).to(torch.uint8).cpu() if ctx.collect_pred else None
    return torch.stack([acc.view(G, ctx.ep_per_batch).mean(dim=1), loss.view(G, ctx.ep_per_batch).mean(dim=1)], dim=1), pred


def proto_dense(ctx):
    n_way, shot, n_query, temp = ctx.n_way, ctx.shot, ctx.n_query, head_temp(ctx.model)
    seen = [0]

    def launch(group):
        E = len(group) * ctx.ep_per_batch
        # the index list is permuted on the host so that the transform writes all shot images, then all query images: x_shot / x_query
        # are views of its output (fs.split_shot_query on the class-major batch would copy 1 GB per 128-episode launch)
        idx = torch.stack(group).view(E, n_way, shot + n_query)
        n_s = E * n_way * shot
        data = gather_images(ctx.dataset, torch.cat([idx[:, :, :shot].reshape(-1), idx[:, :, shot:].reshape(-1)]), ctx.device)
        seen[0] += data.shape[0]
        x_shot = data[:n_s].view(E, n_way, shot, *data.shape[1:])
        x_query = data[n_s:].view(E, n_way * n_query, *data.shape[1:])
        return _proto_rows(ctx, len(group), *ctx.engine.meta_baseline_forward(x_shot, x_query, temp, ctx.model.method, want_stats=True))

    return launch, lambda: (seen[0], seen[0])


def _table_route(ctx, rows):
    from .feature_table import FeatureTable
    table = FeatureTable.for_dataset(ctx.model, ctx.dataset)

    def finish():
        table.check()                                       # raises if a launch met a slot outside the table
        return table.n_requests, table.n_encoded

    return lambda group: rows(table, torch.stack(group), len(group)), finish


def proto_table(ctx):
    temp = head_temp(ctx.model)
    return _table_route(ctx, lambda table, idx, G: _proto_rows(ctx, G, *table.episodes(idx, ctx.n_way, ctx.shot, ctx.n_query, temp, ctx.model.method)))


def auc_dense(ctx):
    from .engine import ops
    n_way, shot, n_query = ctx.n_way, ctx.shot, ctx.n_query
    seen = [0]                                              # the shots of class 0 and all queries

    def launch(group):
        E = len(group) * ctx.ep_per_batch
        idx = torch.stack(group).view(E, n_way, shot + n_query)
        data = gather_images(ctx.dataset, torch.cat([idx[:, 0, :shot].reshape(-1), idx[:, :, shot:].reshape(-1)]), ctx.device)      # x_shot[:, 0] (:96)
        seen[0] += data.shape[0]
        f_shot = ctx.engine.forward(data[:E * shot]).view(E, shot, -1)
        f_query = ctx.engine.forward(data[E * shot:]).view(E, n_way * n_query, -1)       # class-major: the first n_query queries are class 0, the positives
        return ops.proto_auc(f_shot, f_query).view(len(group), ctx.ep_per_batch), None

    return launch, lambda: (seen[0], seen[0])


def auc_table(ctx):
    return _table_route(ctx, lambda table, idx, G: (table.auc(idx, ctx.shot, ctx.n_query).view(G, ctx.ep_per_batch), None))


# ---- reductions: the exchanged rows of one epoch into the averagers and va_lst, which live across epochs
def reduce_batches(allv, aves_va, aves_vl, va_lst, items):
    va_lst.extend(allv[:, 0].tolist())
    for a, l in allv:
        aves_va.add(a, items)
        aves_vl.add(l, items)


def reduce_episodes(allv, aves_va, aves_vl, va_lst, items):
    for a in allv.reshape(-1).tolist():                      # `aves['va'].add(acc, len(data)); va_lst.append(acc)` per episode (--sauc, :111-112)
        aves_va.add(a, items)
        va_lst.append(a)


def evaluate(config, n_way, make_route, reduce, shot=1, test_epochs=1, n_batch=2000, ep_per_batch=1, launch_batches=None, numerics=None,
             rank=0, world=1, device=None, log=print, collect_pred=False):
    """launch_batches: reference batches per engine launch; None (the default, also the CLI's) = `default_launch_batches` - the benched
    configuration (128 five-shot episodes of 100 images).  -> the result dict of the last epoch."""
    t_call = time.perf_counter()
    fix_random_seeds(12345)
    dataset = datasets.make(config['dataset'], **config['dataset_args'])
    t_dataset = time.perf_counter()
    n_query = 15
    per_batch_items = ep_per_batch * n_way * (shot + n_query)
    sampler = CategoriesSampler(dataset.label, n_batch, n_way, shot + n_query, ep_per_batch=ep_per_batch,
                                rank=rank, world_size=world, shard=parallel.sampler_shard(world))
    device = device or torch.device('cuda', torch.cuda.current_device())
    model = build_model(config, numerics).to(device).eval()
    if rank == 0:
        log('num params: {}'.format(utils.compute_n_params(model)))
    t_model = time.perf_counter()
    engine = model.encoder.engine()
    if launch_batches is None:
        launch_batches = default_launch_batches(engine, per_batch_items, engine.img_size, device)
    launch, finish = make_route(SimpleNamespace(dataset=dataset, model=model, engine=engine, device=device, n_way=n_way, shot=shot, n_query=n_query,
                                                ep_per_batch=ep_per_batch, collect_pred=collect_pred))
    width = 2 if reduce is reduce_batches else ep_per_batch    # columns of a batch's row

    np.random.seed(12345)                                  # fixes the episode stream (test_few_shot.py:76)
    out = None
    torch.cuda.synchronize(device)
    t_loop = time.perf_counter()
    # the reference keeps ONE pair of averagers and ONE va_lst across epochs (test_few_shot.py:73-74 sit outside the epoch loop), so the
    # accuracy / CI printed for epoch e covers every batch of epochs 1..e
    aves_va, aves_vl, va_lst = utils.Averager(), utils.Averager(), []
    for epoch in range(1, test_epochs + 1):
        rows, preds, last_label = [], [], None
        # the first launch is small so that the GPU starts while the host is still drawing the stream; from then on the sampler runs under the
        # previous launch.  (Round 5: with the native sampler a full launch of 128 episodes is 6 ms of host time, so one 32-episode step replaces the
        # 8 / 16 / 32 / 64 ramp of the 100-us-per-episode numpy sampler - small launches run the persistent kernels at half their efficiency.)
        for group in launch_groups(sampler, launch_batches, ramp=[n for n in (32,) if n < launch_batches]):
            last_label = dataset.label[int(group[-1][-1])]
            row, pred = launch(group)
            rows.append(row)
            preds.append(pred)
        images = finish()
        mine = torch.cat(rows).double() if rows else torch.zeros(0, width, dtype=torch.float64, device=device)
        allv = parallel.gather_in_stream_order(mine, n_batch, rank, world).cpu().numpy()     # the one exchange
        reduce(allv, aves_va, aves_vl, va_lst, per_batch_items)
        out = dict(acc=aves_va.item(), ci=float(utils.mean_confidence_interval(va_lst)) if len(va_lst) > 1 else float('nan'),
                   loss=aves_vl.item(), n=len(va_lst), last_label=last_label, va_lst=list(va_lst))
        if collect_pred:
            out['pred'] = torch.cat(preds) if preds else torch.zeros(0, n_way * n_query, dtype=torch.uint8)
        # sampler -> gather + transform -> encoder + head -> statistics exchange, everything after model / dataset construction (the gather above synchronised)
        out['loop_seconds'] = time.perf_counter() - t_loop
        out['launch_batches'] = launch_batches
        out['phase_seconds'] = {'dataset': t_dataset - t_call, 'model': t_model - t_dataset, 'engine': t_loop - t_model, 'loop': out['loop_seconds']}
        out['images_requested'], out['images_encoded'] = images
        if rank == 0:
            log('test epoch {}: acc={:.2f} +- {:.2f} (%), loss={:.4f} (@{})'.format(
                epoch, out['acc'] * 100, out['ci'] * 100, out['loss'], last_label))
    return out


# ---- the command line of the three drivers
def make_parser(sauc=False, feature_cache=False, **kw):
    parser = argparse.ArgumentParser(**kw)
    parser.add_argument('--config', default='./configs/test_few_shot.yaml')
    parser.add_argument('--shot', type=int, default=1)
    parser.add_argument('--test-epochs', type=int, default=1)
    if sauc:
        parser.add_argument('--sauc', action='store_true', help='2-way episodes scored against the prototype of class 0, reduced by ROC-AUC (the reference flag)')
    parser.add_argument('--gpu', default=None, help='kept for CLI compatibility; use torchrun for multi-GPU')
    parser.add_argument('--episodes', type=int, default=2000, help='number of batches (reference: 2000)')
    parser.add_argument('--ep-per-batch', type=int, default=1)
    parser.add_argument('--launch-batches', type=int, default=None, help='reference batches per engine launch (default: one encoder chunk, 12 800 images = 128 five-shot episodes)')
    parser.add_argument('--numerics', default=None, choices=[None, 'bf16', 'f16', 'bf16x2', 'f16x2', 'parity'],
                        help="default: FSVIT_NUMERICS or 'bf16' (throughput mode: logits within ~5e-2 of the reference's, 98.8 %% arg-max agreement). "
                             "'f16' runs at 0.93 x the rate with 7 x tighter logits (~8e-3, 99.85 %%) when the checkpoint's weights fit the fp16 range; "
                             "'bf16x2' / 'f16x2' meet the reference's logits within 1e-3 at 0.24 x the rate; 'parity' = exact fp32 (0.12 x)")
    if feature_cache:
        parser.add_argument('--feature-cache', action='store_true',
                            help='encode every image once into a feature table and run the episodes over its rows (same numbers, fewer encoder passes)')
    return parser


def run_cli(evaluate_fn, parser, argv=None):
    """Parse, join the process group torchrun set up, call `evaluate_fn` with the parser's switches (`--sauc`, `--feature-cache` where it has them)."""
    args = parser.parse_args(argv)
    config = yaml.load(open(args.config, 'r'), Loader=yaml.FullLoader)
    if args.gpu is not None and ',' not in args.gpu:
        utils.set_gpu(args.gpu)
    rank, world, local = parallel.init_from_env()
    torch.cuda.set_device(local)
    switches = {k: getattr(args, k) for k in ('sauc', 'feature_cache') if hasattr(args, k)}
    evaluate_fn(config, shot=args.shot, test_epochs=args.test_epochs, n_batch=args.episodes, ep_per_batch=args.ep_per_batch,
                launch_batches=args.launch_batches, numerics=args.numerics, rank=rank, world=world,
                device=torch.device('cuda', local), log=utils.log, **switches)
    if world > 1:
        torch.distributed.destroy_process_group()
