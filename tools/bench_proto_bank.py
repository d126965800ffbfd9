"""Prototype bank (csrc/proto_bank.hip) on one MI355X: the share of a `MetaBaseline.predict` call that the logits kernel takes.
Prints one JSON line per figure:
  * proto_bank_logits at Q queries of D = 512 against `way` prototypes, per method, with the FMA rate it amounts to;
  * proto_bank_accumulate + finalize of a support set of --support rows into the same number of classes;
  * the encoder forward (visformer_micro_80, procedural checkpoint) of the same Q images, the other part of the predict call.
  * with --topk K: proto_bank_topk against the route over the full matrix (proto_bank_logits + torch.topk + torch.logsumexp) for the same answer, at
    (Q, way) = (8, 65536), (12800, 1024), (12800, 65536), (75, 5), D = 512, 'cos': the two routes alternate in one process, the full-matrix route runs
    twice per round (its run-to-run spread), and the line carries the bytes that route writes and re-reads for the logits.
Every figure: --warmup untimed runs, then the median of --steps runs timed with HIP events.
Usage: python tools/bench_proto_bank.py [--queries 12800] [--ways 64,1024] [--dim 512] [--support 5120] [--steps 20] [--warmup 3] [--numerics bf16] [--no-encoder]
       [--topk 5]"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from fewshot_vit_amd import models, synthetic     # noqa: E402
from fewshot_vit_amd.engine import ops            # noqa: E402


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


TOPK_SHAPES = ((8, 65536), (12800, 1024), (12800, 65536), (75, 5))


def timed_once(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def bench_topk(K, D, warmup, steps, dev, name):
    """Two routes to 'the K best classes of every row and the row's log-sum-exp', alternated in one process.  A: what the full matrix costs -
    proto_bank_logits, torch.topk, torch.logsumexp.  B: proto_bank_topk.  A runs twice back to back in every round: the difference is the run-to-run spread
    B's lead is judged against."""
    for Q, way in TOPK_SHAPES:
        g = torch.Generator().manual_seed(1)
        query = torch.randn(Q, D, generator=g).to(dev)
        proto = torch.nn.functional.normalize(torch.randn(way, D, generator=g), dim=-1).to(dev)
        empty = torch.zeros(way, dtype=torch.int32, device=dev)
        kk = min(K, way)

        def route_a():
            logits, _ = ops.proto_bank_logits(query, proto, empty, 10.0, 'cos', want_pred=False)
            return torch.topk(logits, kk, dim=-1), torch.logsumexp(logits, -1)

        def route_b():
            return ops.proto_bank_topk(query, proto, empty, 10.0, 'cos', K)

        for _ in range(warmup):
            route_a()
            route_b()
        a, a2, b = [], [], []
        for _ in range(steps):
            a.append(timed_once(route_a))
            a2.append(timed_once(route_a))
            b.append(timed_once(route_b))
        ma, ma2, mb = statistics.median(a), statistics.median(a2), statistics.median(b)
        spread = max(abs(ma - ma2), statistics.median(abs(x - y) for x, y in zip(a, a2)))
        print(json.dumps({'metric': 'proto_bank_topk_ms', 'K': K, 'Q': Q, 'way': way, 'D': D, 'method': 'cos', 'full_matrix_ms': round(ma, 4),
                          'full_matrix_again_ms': round(ma2, 4), 'spread_ms': round(spread, 4), 'topk_ms': round(mb, 4), 'topk_min_ms': round(min(b), 4),
                          'topk_max_ms': round(max(b), 4), 'speedup': round(ma / mb, 3), 'topk_faster_beyond_spread': bool(mb < min(ma, ma2) - spread),
                          'topk_slower_beyond_spread': bool(mb > max(ma, ma2) + spread), 'logits_bytes_written': Q * way * 4,
                          'logits_bytes_reread': 2 * Q * way * 4, 'samples': steps, 'device': name,
                          'note': 'full_matrix = proto_bank_logits + torch.topk + torch.logsumexp; both routes include their wrappers (allocation)'}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--topk', type=int, default=0, metavar='K', help='also time proto_bank_topk against the full-matrix route (D = 512, cos)')
    ap.add_argument('--queries', type=int, default=12800)
    ap.add_argument('--ways', default='64,1024')
    ap.add_argument('--dim', type=int, default=512)
    ap.add_argument('--support', type=int, default=5120)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--numerics', default='bf16')
    ap.add_argument('--no-encoder', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    name = torch.cuda.get_device_name(dev)
    Q, D = args.queries, args.dim
    g = torch.Generator().manual_seed(0)
    query = torch.randn(Q, D, generator=g).to(dev)
    for way in (int(w) for w in args.ways.split(',')):
        feat = torch.randn(args.support, D, generator=g).to(dev)
        labels = torch.randint(0, way, (args.support,), generator=g).to(dev)
        s = torch.zeros(way, D, dtype=torch.float32, device=dev)
        c = torch.zeros(way, dtype=torch.int32, device=dev)
        inv = torch.zeros(1, dtype=torch.int32, device=dev)
        med, lo, hi = timed(lambda: ops.proto_bank_accumulate(feat, labels, s, c, inv), args.warmup, args.steps)
        fmed, _, _ = timed(lambda: ops.proto_bank_finalize(s, c, 'cos'), args.warmup, args.steps)
        print(json.dumps({'metric': 'proto_bank_accumulate_ms', 'support': args.support, 'way': way, 'D': D, 'value': round(med, 4), 'min_ms': round(lo, 4),
                          'max_ms': round(hi, 4), 'finalize_ms': round(fmed, 4), 'samples': args.steps, 'device': name}))
        for method in ('cos', 'sqr'):
            proto, empty = ops.proto_bank_finalize(s, c, method)
            med, lo, hi = timed(lambda: ops.proto_bank_logits(query, proto, empty, 10.0, method), args.warmup, args.steps)
            print(json.dumps({'metric': 'proto_bank_logits_ms', 'method': method, 'Q': Q, 'way': way, 'D': D, 'value': round(med, 4), 'min_ms': round(lo, 4),
                              'max_ms': round(hi, 4), 'tfma_per_s': round(Q * way * D / (med * 1e-3) / 1e12, 2), 'samples': args.steps, 'device': name,
                              'note': 'includes the wrapper (output allocation); fma = one q * p (cos) or (q - p)^2 (sqr) term'}))
    if args.topk:
        bench_topk(args.topk, 512, args.warmup, args.steps, dev, name)
    if not args.no_encoder:
        m = models.make('meta-baseline', encoder='visformer_micro_80', encoder_args={'numerics': args.numerics})
        m.load_state_dict(synthetic.synthetic_checkpoint_sd({k: tuple(v.shape) for k, v in m.state_dict().items()}))
        engine = m.to(dev).eval().encoder.engine()
        x = torch.randn(Q, 3, 80, 80, generator=g).to(dev)
        out = torch.empty(Q, engine.out_dim, dtype=torch.float32, device=dev)
        med, lo, hi = timed(lambda: engine.forward(x, out=out), args.warmup, max(3, args.steps // 2))
        print(json.dumps({'metric': 'encoder_forward_ms', 'encoder': 'visformer_micro_80', 'numerics': args.numerics, 'images': Q, 'value': round(med, 3),
                          'min_ms': round(lo, 3), 'max_ms': round(hi, 3), 'device': name}))


if __name__ == '__main__':
    main()
