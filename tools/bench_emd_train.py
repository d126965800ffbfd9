"""SUN-D meta-tuning on one MI355X (fewshot_vit_amd.train_deepemd): one training task = forward (encoder + DeepEMD head) + cross entropy + backward +
NaN-gradient guard, and the optimizer step (Nesterov SGD), at 5-way 1-shot 15-query on 'synthetic-images' with visformer_micro_80 on the procedural
checkpoint, for -deepemd fcn (80 images per task), grid (80 x 13 = 1 040 patches) and sampling (80 x 9 = 720 patches), each in `bf16` and `parity`.
Also the guard + Nesterov launches alone over the real parameter table.  Prints one JSON line per figure.  The patch gather (host-drawn boxes + one
launch) is timed inside the task.  Every figure: --warmup untimed runs, then the median of --steps runs timed with HIP events; min / max reported.
The capability is new, so there is no parent-commit time: each task line carries, as a yardstick only, the per-image time of the SUN-M `train` leg of
DESIGN.md 5 (13.5 ... 13.8 ms per 800-image step of `bench.py --full`).  Nothing is gated on it.
Usage: python tools/bench_emd_train.py [--steps 10] [--warmup 3] [--numerics bf16,parity] [--modes fcn,grid,sampling]"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from fewshot_vit_amd import train_deepemd, utils    # noqa: E402
from fewshot_vit_amd.engine import ops              # noqa: E402
from fewshot_vit_amd.utils import few_shot as fs    # noqa: E402

WAY, SHOT, QUERY = 5, 1, 15
SUN_M_TRAIN_US_PER_IMAGE = (13.5e3 / 800, 13.8e3 / 800)          # DESIGN.md 5, `legs.train`: ms per step / 800 images


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--numerics', default='bf16,parity')
    ap.add_argument('--modes', default='fcn,grid,sampling')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    name = torch.cuda.get_device_name(dev)
    label = fs.make_nk_label(WAY, QUERY).to(dev)
    index = torch.cat([torch.arange(c * 30, c * 30 + SHOT + QUERY) for c in range(WAY)])          # class-major: 5 classes x (1 shot + 15 queries)
    for numerics in a.numerics.split(','):
        for mode in a.modes.split(','):
            args = train_deepemd.parse_args(['-dataset', 'synthetic-images', '-deepemd', mode, '-numerics', numerics, '-way', str(WAY), '-shot', str(SHOT),
                                             '-query', str(QUERY)])
            model = train_deepemd.build_model(args).to(dev).train()
            optimizer, _ = train_deepemd.make_optimizer(model, args)
            ds = train_deepemd.make_dataset(args, 'train', train=True)
            ds.device_images()
            zeroed = torch.zeros((), dtype=torch.int64, device=dev)

            def task():
                x_shot, x_query = fs.split_shot_query(ds.gather(index), WAY, SHOT, QUERY)
                train_deepemd.task_backward(model, x_shot, x_query, label, 1)
                zeroed.add_(utils.detect_grad_nan(model))

            def step():
                optimizer.step()

            task()
            optimizer.zero_grad(set_to_none=False)
            med, lo, hi = timed(task, a.warmup, a.steps)
            images = WAY * (SHOT + QUERY)
            patches = getattr(ds.transform, 'n_patch', 1)
            images *= patches
            s_med, s_lo, s_hi = timed(step, a.warmup, a.steps)
            model.check_status()
            assert int(zeroed) == 0 and all(bool(torch.isfinite(p).all()) for p in model.parameters())
            print(json.dumps({'metric': 'sund_train_task_ms', 'deepemd': mode, 'numerics': numerics, 'episode': f'{WAY}-way {SHOT}-shot {QUERY}-query',
                              'encoder_images_per_task': images, 'nodes': 25 if mode == 'fcn' else patches, 'value': round(med, 3), 'unit': 'ms',
                              'min_ms': round(lo, 3), 'max_ms': round(hi, 3), 'us_per_encoder_image': round(med * 1e3 / images, 2),
                              'optimizer_step_ms': round(s_med, 4), 'optimizer_step_min_ms': round(s_lo, 4), 'optimizer_step_max_ms': round(s_hi, 4),
                              'yardstick_sun_m_train_us_per_image': [round(v, 2) for v in SUN_M_TRAIN_US_PER_IMAGE], 'samples': a.steps, 'device': name}),
                  flush=True)
    # the guard and the Nesterov launch alone over the real parameter table (gradients in place from the last task)
    params = [p for p in model.parameters() if p.grad is not None]
    grads = [p.grad.view(-1) for p in params]
    data = [p.data.view(-1) for p in params]
    bufs = [torch.zeros_like(d) for d in data]
    n = sum(d.numel() for d in data)
    g_med, g_lo, g_hi = timed(lambda: ops.grad_nan_guard(grads), a.warmup, a.steps)
    o_med, o_lo, o_hi = timed(lambda: ops.sgd_nesterov_step_multi(data, grads, bufs, 0.0, 0.9, 5e-4, False), a.warmup, a.steps)
    print(json.dumps({'metric': 'sund_guard_and_nesterov_launch_ms', 'tensors': len(data), 'elements': n,
                      'grad_nan_guard_ms': round(g_med, 4), 'grad_nan_guard_min_ms': round(g_lo, 4), 'grad_nan_guard_max_ms': round(g_hi, 4),
                      'grad_nan_guard_GBps': round(n * 4 / (g_med * 1e-3) / 1e9, 1),
                      'sgd_nesterov_multi_ms': round(o_med, 4), 'sgd_nesterov_multi_min_ms': round(o_lo, 4), 'sgd_nesterov_multi_max_ms': round(o_hi, 4),
                      'sgd_nesterov_multi_GBps': round(n * 4 * 5 / (o_med * 1e-3) / 1e9, 1), 'samples': a.steps, 'device': name}), flush=True)


if __name__ == '__main__':
    main()
