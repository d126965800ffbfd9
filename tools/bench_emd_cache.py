"""The SUN-D evaluation protocol with and without the token-map table on one MI355X: `eval_deepemd.evaluate` (`-deepemd fcn`) over a
`synthetic-images` test split of 20 classes x 600 images behind the full visformer_micro_80 (procedural weights + shipped BN calibration, bf16):
5-way 1-shot with 2000 episodes, and 5-way 5-shot with 600 episodes with `-sfc_fused` on and off.  Every round runs A (`-feature_cache` off), A again
and B (`-feature_cache` on) in one process.  The figure is `loop_seconds`: a host clock from the first draw of the sampler (after a device
synchronise) to the return of evaluate(), which ends in the device reads of the solver status and the accuracies - the dataset, the model and the
packing of its weights are outside.  Prints one JSON line per configuration with the medians over the rounds, the A / A-again spread B's lead is judged
against, and B's `n_encoded` / `n_requests`.  The split is built once and shared by all runs; the per-episode accuracies of A and B must be equal.
Usage: python tools/bench_emd_cache.py [--rounds 5] [--configs 1shot,5shot,5shot-fused] [--episodes-1shot 2000] [--episodes-5shot 600]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from fewshot_vit_amd import datasets, eval_deepemd          # noqa: E402

CONFIGS = {'1shot': ['-shot', '1'], '5shot': ['-shot', '5'], '5shot-fused': ['-shot', '5', '-sfc_fused']}


class TimedSampler(eval_deepemd.CategoriesSampler):
    """the driver's sampler; notes when its first draw starts"""
    started = None

    def __iter__(self):
        torch.cuda.synchronize()
        TimedSampler.started = time.perf_counter()
        return super().__iter__()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--configs', default='1shot,5shot,5shot-fused')
    ap.add_argument('--episodes-1shot', type=int, default=2000)
    ap.add_argument('--episodes-5shot', type=int, default=600)
    ap.add_argument('--numerics', default='bf16')
    ap.add_argument('--classes', type=int, default=20)
    ap.add_argument('--per-class', type=int, default=600)
    ap.add_argument('--sfc-update-step', type=int, default=100)
    args = ap.parse_args()
    made, make = {}, datasets.make

    def make_once(name, **kw):
        key = (name, repr(sorted(kw.items())))
        if key not in made:
            made[key] = make(name, **kw)
        return made[key]

    datasets.make = make_once                                   # the driver looks `make` up on this module
    eval_deepemd.CategoriesSampler = TimedSampler
    for name in args.configs.split(','):
        episodes = args.episodes_1shot if name == '1shot' else args.episodes_5shot
        argv = ['-numerics', args.numerics, '-dataset', 'synthetic-images', '-dataset_args',
                '{split: test, n_classes: %d, n_per_class: %d, seed: 0}' % (args.classes, args.per_class), '-way', '5', '-query', '15', '-test_episode',
                str(episodes), '-sfc_update_step', str(args.sfc_update_step), *CONFIGS[name]]

        def run(cache):
            accs = []
            res = eval_deepemd.evaluate(eval_deepemd.parse_args(argv + (['-feature_cache'] if cache else [])), log=lambda *_: None, collect=accs)
            res['loop_seconds'] = time.perf_counter() - TimedSampler.started          # evaluate() has read the accuracies back: the device is idle
            res['accs'] = accs
            return res

        run(False), run(True)                                   # warm-up: the split, the device copy of its images, kernel loading
        a1, a2, b, encoded, requested = [], [], [], None, None
        for _ in range(args.rounds):
            ra, rb, rc = run(False), run(False), run(True)
            assert ra['accs'] == rb['accs'] == rc['accs'], 'the cache changed the accuracies'
            a1.append(ra['loop_seconds']), a2.append(rb['loop_seconds']), b.append(rc['loop_seconds'])
            encoded, requested = rc['n_encoded'], rc['n_requests']
        med = statistics.median
        A, A2, B = med(a1), med(a2), med(b)
        print(json.dumps({'metric': 'eval_deepemd_loop_seconds', 'config': name, 'episodes': episodes, 'numerics': args.numerics, 'rounds': args.rounds,
                          'sfc_update_step': args.sfc_update_step if name != '1shot' else None,
                          'A': round(A, 4), 'A_again': round(A2, 4), 'B_feature_cache': round(B, 4),
                          'AA_spread': round(max(abs(x - y) for x, y in zip(a1, a2)), 4), 'A_min_max': [round(min(a1 + a2), 4), round(max(a1 + a2), 4)],
                          'B_min_max': [round(min(b), 4), round(max(b), 4)], 'speedup': round(A / B, 3), 'acc': round(rc['acc'], 4),
                          'n_requests': requested, 'n_encoded': encoded}), flush=True)


if __name__ == '__main__':
    main()
