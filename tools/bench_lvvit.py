"""LV-ViT (`lvvit_micro_80`) eval throughput on one MI355X: 5-way 5-shot episodes (15 queries per class), EPISODES per launch
(128 x 100 = 12 800 images) through meta-baseline's one C-ABI call, procedural weights, bf16 by default.  Prints episodes/s, ms per launch,
the per-layer profile (fsvit_encoder_profile_begin / _end: HIP events around every launch of one profiled step) and the fraction of the
dense MFMA peak.  Usage: python tools/bench_lvvit.py [--numerics bf16] [--steps 10] [--warmup 3] [--episodes 128]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fewshot_vit_amd import models, synthetic     # noqa: E402

MFMA_PEAK_TFLOPS = {'bf16': 2500.0, 'f16': 2500.0, 'parity': 157.3, 'bf16x2': 625.0, 'f16x2': 625.0}    # as bench.py
GFLOP_PER_IMAGE = 1.199          # torch.utils.flop_counter on the reference model (stem 0.548, blocks 0.622, projection 0.030)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--numerics', default='bf16')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--episodes', type=int, default=128)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    way, shot, query, E = 5, 5, 15, args.episodes
    m = models.make('meta-baseline', encoder='lvvit_micro_80', encoder_args={'numerics': args.numerics})
    m.load_state_dict(synthetic.synthetic_checkpoint_sd({k: tuple(v.shape) for k, v in m.state_dict().items()}, calib='lvvit_micro_80'))
    m = m.to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(0)
    xs = torch.randn(E, way, shot, 3, 80, 80, device=dev, generator=g)
    xq = torch.randn(E, way * query, 3, 80, 80, device=dev, generator=g)
    with torch.no_grad():
        for _ in range(args.warmup):
            m(xs, xq)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            logits = m(xs, xq)
        torch.cuda.synchronize(dev)
        el = time.perf_counter() - t0
        eng = m.encoder.engine()
        eng.profile_begin()
        m(xs, xq)
        prof = eng.profile_end()
    assert torch.isfinite(logits).all()
    eps = E * args.steps / el
    ms = 1e3 * el / args.steps
    n_img = E * way * (shot + query)
    tflops = GFLOP_PER_IMAGE * n_img / (ms * 1e-3) / 1e3
    frac = tflops / MFMA_PEAK_TFLOPS[args.numerics]
    print(f'{"layer":28s} {"kernel":44s} {"launches":>8s} {"ms":>8s} {"TFLOP/s":>8s}')
    for r in prof:
        tf = r['flops'] / (r['ms'] * 1e-3) / 1e12 if r['ms'] > 0 else 0.0
        print(f'{r["layer"]:28s} {r["kernel"][:44]:44s} {r["launches"]:8d} {r["ms"]:8.3f} {tf:8.1f}')
    print(f'profiled step total {sum(r["ms"] for r in prof):.3f} ms')
    print(json.dumps({'metric': 'lvvit_micro_80_eval_episodes_per_s_5way_5shot', 'numerics': args.numerics, 'episodes_per_launch': E,
                      'value': round(eps, 1), 'unit': 'episodes/s', 'ms_per_launch': round(ms, 3), 'tflops': round(tflops, 1),
                      'mfma_peak_fraction': round(frac, 4), 'device': torch.cuda.get_device_name(dev)}))


if __name__ == '__main__':
    main()
