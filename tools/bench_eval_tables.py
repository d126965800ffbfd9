"""The evaluations that run inside the training phases, and --sauc, with and without the feature table on one MI355X, at the reference's protocol
(sun_meta_training/configs/offline_tl_visformer_k5_800epoch.yaml): the full visformer_micro_80 (procedural weights + shipped BN calibration, bf16) over
`synthetic-images` splits shaped like mini-imagenet's.

  val    offline.py's validation: 16 x 600 images, 200 batches of 16 five-way 1 + 15 episodes     offline.few_shot_eval / few_shot_eval_table
  fs     offline.py's fs-eval block: 20 x 600 images, 200 batches of 4 episodes at 1- and 5-shot  the same two functions, both shot settings, one table
  sauc   eval_sauc.evaluate(sauc=True): 20 x 600 images, 2000 two-way episodes, 1-shot            its `loop_seconds`

Every round runs A (switch off: the code the drivers run without it), A again and B (switch on, the table emptied first) in one process; val / fs are
timed with a synchronised wall clock around the evaluation only, seeded like the drivers.  Prints one JSON line per evaluation with the medians over the
rounds, the A / A-again spread B's lead is judged against, and B's `images_encoded` / `images_requested`.  A and B must report the same accuracy up to
the near-tie share DESIGN.md 4d derives (val / fs) or the same AUCs (sauc).
Usage: python tools/bench_eval_tables.py [--rounds 3] [--kinds val,fs,sauc] [--val-batches 200] [--fs-batches 200] [--episodes 2000] [--numerics bf16]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from fewshot_vit_amd import datasets, eval_sauc, models, offline, synthetic  # noqa: E402
from fewshot_vit_amd.datasets.samplers import CategoriesSampler            # noqa: E402
from fewshot_vit_amd.feature_table import FeatureTable                     # noqa: E402


def _timed(fn, device):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(device)
    return time.perf_counter() - t0, out


def _report(kind, args, a1, a2, b, extra):
    med = statistics.median
    A, A2, B = med(a1), med(a2), med(b)
    print(json.dumps(dict({'metric': 'evaluation_seconds', 'kind': kind, 'numerics': args.numerics, 'rounds': args.rounds, 'A': round(A, 4),
                           'A_again': round(A2, 4), 'B_feature_table': round(B, 4), 'AA_spread': round(max(abs(x - y) for x, y in zip(a1, a2)), 4),
                           'A_min_max': [round(min(a1 + a2), 4), round(max(a1 + a2), 4)], 'B_min_max': [round(min(b), 4), round(max(b), 4)],
                           'speedup': round(A / B, 2)}, **extra)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--kinds', default='val,fs,sauc')
    ap.add_argument('--val-batches', type=int, default=200)
    ap.add_argument('--fs-batches', type=int, default=200)
    ap.add_argument('--episodes', type=int, default=2000)
    ap.add_argument('--numerics', default='bf16')
    ap.add_argument('--per-class', type=int, default=600)
    args = ap.parse_args()
    kinds = args.kinds.split(',')
    if not torch.cuda.is_available():
        raise SystemExit('bench_eval_tables measures on an MI355X; no GPU is visible')
    device = torch.device('cuda', 0)
    made, make = {}, datasets.make

    def make_once(name, **kw):
        key = (name, repr(sorted(kw.items())))
        if key not in made:
            made[key] = make(name, **kw)
        return made[key]

    datasets.make = make_once                                   # the drivers look `make` up on this module
    val_args = dict(split='val', n_classes=16, n_per_class=args.per_class, seed=2)
    fs_args = dict(split='test', n_classes=20, n_per_class=args.per_class, seed=0)

    model = None
    if 'val' in kinds or 'fs' in kinds:                         # the distillation student, as offline.main builds it
        model = models.make('token-label', encoder='visformer_micro_80', encoder_args=dict(numerics=args.numerics, return_map=True),
                            classifier='linear-classifier', classifier_args=dict(n_classes=64)).to(device)
        shapes = {'encoder.' + k: tuple(v.shape) for k, v in model.encoder.state_dict().items()}
        esd = synthetic.synthetic_checkpoint_sd(shapes, calib='visformer_micro_80')
        model.encoder.load_state_dict({k[len('encoder.'):]: v for k, v in esd.items()})
        model.eval()

    def evaluation(dataset, settings, n_batches):
        """-> (run_a, run_b, table): one evaluation over `settings` = [(n_way, n_shot, n_query, ep_per_batch)], each seeded like the driver's"""
        samplers = [CategoriesSampler(dataset.label, n_batches, w, s + q, ep_per_batch=e) for w, s, q, e in settings]
        table = FeatureTable.for_dataset(model, dataset)

        def run_a():
            out = []
            for (w, s, q, e), sampler in zip(settings, samplers):
                np.random.seed(0)
                out.append(offline.few_shot_eval(model, dataset, sampler, w, s, q, e, device))
            return out

        def run_b():
            table.reset()                                       # what the driver does after an epoch's training steps
            out = []
            for (w, s, q, e), sampler in zip(settings, samplers):
                np.random.seed(0)
                out.append(offline.few_shot_eval_table(table, sampler, w, s, q, e))
            return out

        return run_a, run_b, table

    plans = []
    if 'val' in kinds:
        plans.append(('val', make_once('synthetic-images', **val_args), [(5, 1, 15, 16)], args.val_batches))
    if 'fs' in kinds:
        plans.append(('fs', make_once('synthetic-images', **fs_args), [(5, 1, 15, 4), (5, 5, 15, 4)], args.fs_batches))
    for kind, dataset, settings, n_batches in plans:
        warm_a, warm_b, _ = evaluation(dataset, settings, 2)    # warm-up at the timed batch shapes: the device copy of the split, kernel loading
        warm_a(), warm_b()
        run_a, run_b, table = evaluation(dataset, settings, n_batches)
        a1, a2, b, ra, rb = [], [], [], None, None
        for _ in range(args.rounds):
            (ta, ra), (ta2, ra2), (tb, rb) = _timed(run_a, device), _timed(run_a, device), _timed(run_b, device)
            assert ra == ra2, 'the switch-off route is not repeatable'
            a1.append(ta), a2.append(ta2), b.append(tb)
        _report(kind, args, a1, a2, b, {'batches': n_batches, 'settings': settings, 'images_requested': table.n_requests, 'images_encoded': table.n_encoded,
                                        'A_loss_acc': ra, 'B_loss_acc': rb})

    if 'sauc' in kinds:
        config = {'dataset': 'synthetic-images', 'dataset_args': fs_args, 'synthetic_checkpoint': 'visformer_micro_80'}
        run = lambda cache, n=args.episodes: eval_sauc.evaluate(config, shot=1, n_batch=n, numerics=args.numerics, log=lambda *_: None, sauc=True,
                                                                feature_cache=cache)
        run(False, 40), run(True, 40)                           # warm-up
        a1, a2, b, rc = [], [], [], None
        for _ in range(args.rounds):
            ra, ra2, rc = run(False), run(False), run(True)
            assert ra['va_lst'] == ra2['va_lst'] == rc['va_lst'], 'the table changed the AUCs'
            a1.append(ra['loop_seconds']), a2.append(ra2['loop_seconds']), b.append(rc['loop_seconds'])
        _report('sauc', args, a1, a2, b, {'episodes': args.episodes, 'images_requested': rc['images_requested'], 'images_encoded': rc['images_encoded'],
                                          'auc': round(rc['acc'], 6)})


if __name__ == '__main__':
    main()
