"""LV-ViT (`lvvit_micro_80`) eval throughput on one MI355X: 5-way 5-shot episodes (15 queries per class), EPISODES per launch
(128 x 100 = 12 800 images) through meta-baseline's one C-ABI call, procedural weights, bf16 by default.  Prints episodes/s, ms per launch,
the per-layer profile (fsvit_encoder_profile_begin / _end: HIP events around every launch of one profiled step) and the fraction of the
dense MFMA peak.  Usage: python tools/bench_lvvit.py [--numerics bf16] [--steps 10] [--warmup 3] [--episodes 128]

--mode train: one meta-tuning step (forward, cross-entropy, backward) of EPISODES 5-way 1-shot 3-query episodes (default 40 = 800 images) on the
HIP trainer, timed with HIP events.  Both weight-gradient routes of the dense 96 -> 96 stem layers are built in the same process (--routes: the
direct kernel under FSVIT_LVVIT_WGRAD=direct, the transposed split-K GEMM under =gemm) and their steps ALTERNATE; medians per route are printed.
--return-map: the same step with the encoder's (token map, cls) output and a loss on both (cross-entropy on the head + mean(map * w)): what the fused
final-norm backward and the fp32 map cost on top of the cls-only step (plus the three torch kernels of that extra loss term).

--mode distill: one offline.distill_step (student forward with both outputs, frozen teacher forward, soft labels, both losses, backward, AdamW) of
`token-label` over lvvit_micro_80 at --batch images (default 512, the reference's batch size), timed with HIP events."""
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


def train_step(args):
    import statistics
    import torch.nn.functional as F
    from fewshot_vit_amd.utils import few_shot as fs
    dev = torch.device('cuda', 0)
    way, shot, query, E = 5, 1, 3, args.episodes or 40
    g = torch.Generator(device=dev).manual_seed(0)
    xs = torch.randn(E, way, shot, 3, 80, 80, device=dev, generator=g)
    xq = torch.randn(E, way * query, 3, 80, 80, device=dev, generator=g)
    label = fs.make_nk_label(way, query, E).to(dev)
    n_shot = E * way * shot
    wtok = torch.randn(E * way * (shot + query), 5, 5, 384, device=dev, generator=g)

    def loss_of(m):
        if not args.return_map:
            return F.cross_entropy(m(xs, xq).view(-1, way), label)
        from fewshot_vit_amd.autograd import ProtoHeadFn
        fmap, feat = m.encoder(torch.cat([xs.reshape(-1, 3, 80, 80), xq.reshape(-1, 3, 80, 80)], dim=0))      # MetaBaseline._forward_train with the map kept
        logits = ProtoHeadFn.apply(feat[:n_shot].view(E, way, shot, -1), feat[n_shot:].view(E, way * query, -1),
                                   m.temp if isinstance(m.temp, torch.Tensor) else torch.tensor(float(m.temp)), m.method)
        return F.cross_entropy(logits.view(-1, way), label) + (fmap.permute(0, 2, 3, 1) * wtok).mean()      # (token-major, as token-label's heads read the map)

    routes = {}
    for route in args.routes.split(','):                    # the switch is read when the trainer handle is created (first train-mode forward)
        os.environ['FSVIT_LVVIT_WGRAD'] = route
        m = models.make('meta-baseline', encoder='lvvit_micro_80', encoder_args={'numerics': args.numerics, 'return_map': args.return_map})
        m.load_state_dict(synthetic.synthetic_checkpoint_sd({k: tuple(v.shape) for k, v in m.state_dict().items()}, calib='lvvit_micro_80'))
        m = m.to(dev).train()
        loss_of(m).backward()
        routes[route] = m
    os.environ.pop('FSVIT_LVVIT_WGRAD', None)

    def step(m):
        m.zero_grad(set_to_none=True)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        loss = loss_of(m)
        loss.backward()
        t1.record()
        t1.synchronize()
        assert torch.isfinite(loss)
        return t0.elapsed_time(t1)

    ms = {r: [] for r in routes}
    for i in range(args.warmup + args.steps):
        for r, m in routes.items():                        # A B A B ...
            t = step(m)
            if i >= args.warmup:
                ms[r].append(t)
    n_img = E * way * (shot + query)
    for r in routes:
        print(f'{r:7s} samples (ms): ' + ' '.join(f'{v:.2f}' for v in ms[r]))
    med = {r: statistics.median(v) for r, v in ms.items()}
    print(json.dumps({'metric': 'lvvit_micro_80_meta_tuning_step_ms', 'numerics': args.numerics, 'images': n_img, 'unit': 'ms', 'return_map': args.return_map,
                      **{f'wgrad96_{r}_route_ms': round(v, 3) for r, v in med.items()}, 'samples_per_route': args.steps, 'alternated': True,
                      'device': torch.cuda.get_device_name(dev)}))


def distill(args):
    import statistics
    from fewshot_vit_amd import offline
    from fewshot_vit_amd.models.classifier import FsvitAdamW, SoftTargetCrossEntropy
    dev = torch.device('cuda', 0)
    B, n_classes = args.batch, 64
    g = torch.Generator(device=dev).manual_seed(0)
    data = torch.randn(B, 3, 80, 80, device=dev, generator=g)
    weak = torch.randn(B, 3, 80, 80, device=dev, generator=g)
    label = torch.randint(0, n_classes, (B,), device=dev, generator=g)
    pair = []
    for _ in range(2):
        m = models.make('token-label', encoder='lvvit_micro_80', encoder_args={'numerics': args.numerics, 'return_map': True, 'drop_path_rate': 0.1},
                        classifier='linear-classifier', classifier_args={'n_classes': n_classes})
        esd = synthetic.synthetic_checkpoint_sd({'encoder.' + k: tuple(v.shape) for k, v in m.encoder.state_dict().items()}, calib='lvvit_micro_80')
        m.encoder.load_state_dict({k[len('encoder.'):]: v for k, v in esd.items()})
        pair.append(m.to(dev))
    model, teacher = pair[0].train(), pair[1].eval()
    opt = FsvitAdamW(model.parameters(), lr=5e-4 * B / 512, weight_decay=0.05)
    crit = SoftTargetCrossEntropy()
    ms = []
    for i in range(args.warmup + args.steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        loss, _ = offline.distill_step(model, teacher, opt, crit, data, weak, label)
        t1.record()
        t1.synchronize()
        assert torch.isfinite(loss)
        if i >= args.warmup:
            ms.append(t0.elapsed_time(t1))
    print('samples (ms): ' + ' '.join(f'{v:.2f}' for v in ms))
    print(json.dumps({'metric': 'lvvit_micro_80_distill_step_ms', 'numerics': args.numerics, 'images': B, 'unit': 'ms', 'value': round(statistics.median(ms), 3),
                      'min': round(min(ms), 3), 'max': round(max(ms), 3), 'samples': args.steps, 'device': torch.cuda.get_device_name(dev)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--numerics', default='bf16')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--episodes', type=int, default=None)
    ap.add_argument('--mode', choices=['eval', 'train', 'distill'], default='eval')
    ap.add_argument('--return-map', action='store_true', help='--mode train: the encoder returns (token map, cls) and the loss uses both')
    ap.add_argument('--batch', type=int, default=512, help='--mode distill: images per step')
    ap.add_argument('--routes', default='direct,gemm', help='--mode train: the weight-gradient routes to build and alternate (one name for a kernel trace)')
    args = ap.parse_args()
    if args.mode == 'train':
        return train_step(args)
    if args.mode == 'distill':
        return distill(args)
    if args.episodes is None:
        args.episodes = 128
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
