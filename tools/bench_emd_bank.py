"""DeepEMD over a labelled support set (csrc/emd_head.hip) on one MI355X: every class scored exactly against a shortlist re-ranked exactly.
Random class-structured token maps, no encoder: `--classes` class centres, a map = `--signal` (0.6) * centre + unit noise + a per-channel offset (the cases of
tests/emd_bank_cases.py), `--shots` support maps per class, `--queries` query maps, N = 25 tokens of C = 512 channels.  The queries are prepared once
(emd_table_prep), outside both timings.
  A: ops.emd_head_gather of every query against every class map (the dense route of TokenBank.logits): Q * classes transportation problems.  It uses
     no entry of the bank (class maps are formed with torch here), so `--dense-only` runs on a tree that lacks it.
  B: per M in --shortlists: ops.proto_bank_topk (the M best classes by the cosine of token means) + ops.emd_rerank: Q * M problems, ranked in the launch.
Per round A runs twice back to back (its run-to-run spread) and every B once; one JSON line per M with the medians, the share of queries whose dense
arg-max lies inside the shortlist, the top-1 agreement of B with A, and the accuracy of both against the labels the maps were drawn with.
Usage: python tools/bench_emd_bank.py [--classes 1024] [--queries 12800] [--shots 5] [--shortlists 8,16,32] [--steps 3] [--warmup 1] [--signal 0.6]
       [--dense-only]"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from fewshot_vit_amd.engine import ops            # noqa: E402

T = 12.5


def timed_once(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def draw(centre, offset, labels, g, signal, chunk=1024):
    out = torch.empty(labels.shape[0], *centre.shape[1:], device=centre.device)
    for i in range(0, labels.shape[0], chunk):
        lab = labels[i:i + chunk]
        out[i:i + chunk] = signal * centre[lab] + torch.randn(lab.shape[0], *centre.shape[1:], generator=g, device=centre.device) + offset
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--classes', type=int, default=1024)
    ap.add_argument('--queries', type=int, default=12800)
    ap.add_argument('--shots', type=int, default=5)
    ap.add_argument('--tokens', type=int, default=25)
    ap.add_argument('--channels', type=int, default=512)
    ap.add_argument('--shortlists', default='8,16,32')
    ap.add_argument('--signal', type=float, default=0.6, help='weight of the class centre under the unit noise: lower makes the classes harder to tell apart')
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--dense-only', action='store_true', help='time A alone (needs no entry of the bank)')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    name = torch.cuda.get_device_name(dev)
    n_cls, Q, N, C = args.classes, args.queries, args.tokens, args.channels
    g = torch.Generator(device=dev).manual_seed(0)
    centre = torch.randn(n_cls, N, C, generator=g, device=dev)
    offset = 0.5 * torch.randn(1, 1, C, generator=g, device=dev)
    sup_lab = torch.arange(n_cls, device=dev).repeat(args.shots)
    qry_lab = torch.randint(0, n_cls, (Q,), generator=g, device=dev)
    sup, qry = draw(centre, offset, sup_lab, g, args.signal), draw(centre, offset, qry_lab, g, args.signal)
    class_tok = torch.zeros(n_cls, N, C, device=dev).index_add_(0, sup_lab, sup) / args.shots
    xhat, pooled = torch.empty_like(qry), torch.empty(Q, C, device=dev)
    ops.emd_table_prep(qry, xhat, pooled)
    slots = torch.arange(Q, dtype=torch.int32, device=dev)[None]
    invalid = torch.zeros(1, dtype=torch.int32, device=dev)
    keep = {}

    def route_a():
        keep['dense'] = ops.emd_head_gather(qry, xhat, pooled, slots, T, invalid, proto_tok=class_tok[None])

    routes = {}
    if not args.dense_only:
        s, c, inv = torch.zeros(n_cls, N, C, device=dev), torch.zeros(n_cls, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        ops.emd_bank_accumulate(sup, sup_lab, s, c, inv)
        tok_c, xhat_c, pooled_c, proto, empty = ops.emd_bank_finalize(s, c)
        for M in (int(m) for m in args.shortlists.split(',')):
            def route_b(M=M):
                cand = ops.proto_bank_topk(pooled, proto, empty, 1.0, 'cos', k=M, want_lse=False)[1]
                keep[M] = (cand, ops.emd_rerank((qry, xhat, pooled), (tok_c, xhat_c, pooled_c, empty), cand, T, 1))
            routes[M] = route_b
    for _ in range(args.warmup):
        route_a()
        for fn in routes.values():
            fn()
    a, a2, b = [], [], {M: [] for M in routes}
    for _ in range(args.steps):
        a.append(timed_once(route_a))
        a2.append(timed_once(route_a))
        for M, fn in routes.items():
            b[M].append(timed_once(fn))
    ma, ma2 = statistics.median(a), statistics.median(a2)
    spread = max(abs(ma - ma2), statistics.median(abs(x - y) for x, y in zip(a, a2)))
    dense, status = keep['dense']
    best = dense[0].argmax(-1)
    base = {'Q': Q, 'classes': n_cls, 'shots': args.shots, 'signal': args.signal, 'N': N, 'C': C, 'dense_ms': round(ma, 2), 'dense_again_ms': round(ma2, 2), 'spread_ms': round(spread, 2),
            'dense_problems': Q * n_cls, 'dense_status': int(status.sum()), 'dense_accuracy': round(float((best == qry_lab).float().mean()), 4),
            'samples': args.steps, 'device': name}
    if args.dense_only:
        print(json.dumps({'metric': 'emd_bank_dense_ms', **base}))
    for M in routes:
        cand, (classes, values, prob, _, st, bad) = keep[M]
        mb = statistics.median(b[M])
        top1 = classes[:, 0].long()
        print(json.dumps({'metric': 'emd_bank_rerank_ms', 'M': M, 'rerank_ms': round(mb, 2), 'rerank_min_ms': round(min(b[M]), 2), 'rerank_max_ms': round(max(b[M]), 2),
                          'problems': Q * M, 'speedup': round(ma / mb, 2), 'rerank_faster_beyond_spread': bool(mb < min(ma, ma2) - spread),
                          'dense_argmax_in_shortlist': round(float((cand.long() == best[:, None]).any(-1).float().mean()), 4),
                          'top1_agreement': round(float((top1 == best).float().mean()), 4), 'rerank_accuracy': round(float((top1 == qry_lab).float().mean()), 4),
                          'rerank_status': int(st), 'rerank_invalid': int(bad), **base,
                          'note': 'rerank = proto_bank_topk (shortlist) + emd_rerank; both routes include their wrappers (allocation), neither the query preparation'}))


if __name__ == '__main__':
    main()
