"""The reference's evaluation protocol with and without the feature cache on one MI355X: `eval_cached.evaluate` over a `synthetic-images` test split
of 20 classes x 600 images behind the full visformer_micro_80 (procedural weights + shipped BN calibration, bf16), 2000 batches, 1-shot and 5-shot.
Every round runs A (`feature_cache=False`), A again and B (`feature_cache=True`) in one process; the figure is `loop_seconds` (sampler -> ... ->
statistics exchange).  Prints one JSON line per shot with the medians over the rounds, the A / A-again spread B's lead is judged against, B's
`images_encoded`, and where B's time goes: the host time of drawing the same episode stream alone, and the encoder's share estimated from A's rate.
The split is built once and shared by all runs (evaluate() would rebuild the same 254 MB table per call); the accuracies of A and B must be equal.
Usage: python tools/bench_feature_cache.py [--rounds 5] [--episodes 2000] [--shots 1,5] [--numerics bf16]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from fewshot_vit_amd import datasets, eval_cached            # noqa: E402
from fewshot_vit_amd.datasets.samplers import CategoriesSampler  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--episodes', type=int, default=2000)
    ap.add_argument('--shots', default='1,5')
    ap.add_argument('--numerics', default='bf16')
    ap.add_argument('--classes', type=int, default=20)
    ap.add_argument('--per-class', type=int, default=600)
    args = ap.parse_args()
    config = {'dataset': 'synthetic-images', 'dataset_args': dict(split='test', n_classes=args.classes, n_per_class=args.per_class, seed=0),
              'synthetic_checkpoint': 'visformer_micro_80'}
    made, make = {}, datasets.make

    def make_once(name, **kw):
        key = (name, repr(sorted(kw.items())))
        if key not in made:
            made[key] = make(name, **kw)
        return made[key]

    datasets.make = make_once                                   # the drivers look `make` up on this module
    for shot in (int(s) for s in args.shots.split(',')):
        run = lambda cache: eval_cached.evaluate(config, shot=shot, n_batch=args.episodes, numerics=args.numerics, log=lambda *_: None, feature_cache=cache)
        run(False), run(True)                                   # warm-up: the split, the device copy of its images, kernel loading
        a1, a2, b, encoded, requested = [], [], [], None, None
        for _ in range(args.rounds):
            ra, rb, rc = run(False), run(False), run(True)
            assert ra['va_lst'] == rb['va_lst'] == rc['va_lst'], 'the cache changed the accuracies'
            a1.append(ra['loop_seconds']), a2.append(rb['loop_seconds']), b.append(rc['loop_seconds'])
            encoded, requested = rc['images_encoded'], rc['images_requested']
        label = make_once(config['dataset'], **config['dataset_args']).label
        draws = []
        for _ in range(args.rounds):                            # the host sampler alone, on the same stream
            np.random.seed(12345)
            t0 = time.perf_counter()
            for _idx in CategoriesSampler(label, args.episodes, 5, shot + 15):
                pass
            draws.append(time.perf_counter() - t0)
        med = statistics.median
        A, A2, B = med(a1), med(a2), med(b)
        print(json.dumps({'metric': 'evaluate_loop_seconds', 'shot': shot, 'episodes': args.episodes, 'numerics': args.numerics, 'rounds': args.rounds,
                          'A': round(A, 4), 'A_again': round(A2, 4), 'B_feature_cache': round(B, 4),
                          'AA_spread': round(max(abs(x - y) for x, y in zip(a1, a2)), 4), 'A_min_max': [round(min(a1 + a2), 4), round(max(a1 + a2), 4)],
                          'B_min_max': [round(min(b), 4), round(max(b), 4)], 'speedup': round(A / B, 2),
                          'images_requested': requested, 'images_encoded': encoded,
                          'B_sampler_seconds': round(med(draws), 4), 'B_encoder_seconds_at_A_rate': round(A * encoded / requested, 4)}), flush=True)


if __name__ == '__main__':
    main()
