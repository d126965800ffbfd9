"""DeepEMD head (csrc/emd_head.hip) on one MI355X: 5-way, 15 queries per class, 25-node token maps of visformer_micro_80 (C = 512) on the synthetic
episodes with the procedural checkpoint.  Prints one JSON line per figure:
  * episodes/s of the 1-shot head alone at E x 75 x 5 problems, next to the meta-baseline head on the pooled features of the same episodes and to the
    float64 HiGHS oracle's CPU time on a sample of the same problems (an oracle, not the reference's cv2.EMD);
  * episodes/s of the whole DeepEMD eval step (encoder + head);
  * episodes/s of the 5-shot SFC path at the reference's eval settings (sfc_lr 100, 100 update steps, mini-batches of 4) on the token maps;
  * with --sfc-fused, that 5-shot leg both ways in this process - the host loop and the on-device loop (DeepEMD.get_sfc(fused=True), emd_sfc_kernel) -
    at --sfc-episodes and at --sfc-episodes-large, and the arg-max agreement of the two routes' final logits on the same permutations (reported, not
    asserted: at sfc_lr 100 the two trajectories need not agree to rounding);
  * the histogram of augmenting paths per problem.
Every GPU figure: --warmup untimed runs, then the median of --steps runs timed with HIP events.
Usage: python tools/bench_emd.py [--episodes 1,16,64] [--steps 10] [--warmup 3] [--numerics bf16] [--sfc-episodes 16] [--sfc-steps 100] [--oracle-problems 40]
                                 [--sfc-fused [--sfc-episodes-large 64]]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from fewshot_vit_amd import models, synthetic     # noqa: E402
from fewshot_vit_amd.engine import ops            # noqa: E402
from fewshot_vit_amd.utils import few_shot as fs  # noqa: E402

WAY, QUERY, T = 5, 15, 12.5


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


def problems_of(shot_tok, query_tok):
    """cost and normalised weights of every (query, proto) pair in fp32 torch arithmetic (for the augmentation histogram and the oracle's timing)."""
    pooled_s, pooled_q = shot_tok.mean(2), query_tok.mean(2)
    w1 = torch.relu(torch.einsum('eqnc,epc->eqpn', query_tok, pooled_s)) + 1e-3
    w2 = torch.relu(torch.einsum('epnc,eqc->eqpn', shot_tok, pooled_q)) + 1e-3
    norm = lambda w: (torch.relu(w) + 1e-5) * (w.shape[-1] / (torch.relu(w) + 1e-5).sum(-1, keepdim=True))
    cen = lambda x: torch.nn.functional.normalize(x - x.mean(-1, keepdim=True), dim=-1, eps=1e-8)
    cost = 1.0 - torch.einsum('eqac,epbc->eqpab', cen(query_tok), cen(shot_tok))
    N = cost.shape[-1]
    return cost.reshape(-1, N, N), norm(w1).reshape(-1, N), norm(w2).reshape(-1, N)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--episodes', default='1,16,64')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--numerics', default='bf16')
    ap.add_argument('--sfc-episodes', type=int, default=16)
    ap.add_argument('--sfc-steps', type=int, default=100)
    ap.add_argument('--oracle-problems', type=int, default=40)
    ap.add_argument('--sfc-fused', action='store_true')
    ap.add_argument('--sfc-episodes-large', type=int, default=64)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    name = torch.cuda.get_device_name(dev)
    m = models.make('deepemd', encoder='visformer_micro_80', encoder_args={'numerics': args.numerics}, temperature=T,
                    sfc_lr=100., sfc_update_step=args.sfc_steps, sfc_bs=4)
    m.load_state_dict(synthetic.synthetic_checkpoint_sd({k: tuple(v.shape) for k, v in m.state_dict().items()}))
    m = m.to(dev).eval()
    sizes = [int(e) for e in args.episodes.split(',')]
    sfc_sizes = [args.sfc_episodes, args.sfc_episodes_large] if args.sfc_fused else [args.sfc_episodes]
    E_max = max(sizes + sfc_sizes)
    x5 = synthetic.synthetic_episodes(0, E_max, WAY, 5, QUERY).to(dev)
    xs5, xq = fs.split_shot_query(x5, WAY, 5, QUERY, ep_per_batch=E_max)
    with torch.no_grad():
        tok = m.encode(torch.cat([xs5.reshape(-1, 3, 80, 80), xq.reshape(-1, 3, 80, 80)]), False)
        _, feat = m.encoder(torch.cat([xs5[:, :, 0].reshape(-1, 3, 80, 80), xq.reshape(-1, 3, 80, 80)]))
    n5 = E_max * WAY * 5
    shot5_tok = tok[:n5].reshape(E_max, WAY, 5, *tok.shape[1:]).contiguous()
    query_tok = tok[n5:].reshape(E_max, WAY * QUERY, *tok.shape[1:]).contiguous()
    shot_tok = shot5_tok[:, :, 0].contiguous()
    feat_s, feat_q = feat[:E_max * WAY].reshape(E_max, WAY, 1, -1).contiguous(), feat[E_max * WAY:].reshape(E_max, WAY * QUERY, -1).contiguous()
    N, C = tok.shape[1:]

    # 1. the 1-shot head alone, the meta-baseline head on the same episodes
    for E in sizes:
        s, q = shot_tok[:E].contiguous(), query_tok[:E].contiguous()
        med, lo, hi = timed(lambda: ops.emd_head_forward(s, q, T, want_flow=False), args.warmup, args.steps)
        fsb, fqb = feat_s[:E].contiguous(), feat_q[:E].contiguous()
        mb, _, _ = timed(lambda: ops.proto_head(fsb, fqb, 10.0, 'cos'), args.warmup, args.steps)
        _, _, status = ops.emd_head_forward(s, q, T, want_flow=False)
        assert int(status.sum()) == 0
        print(json.dumps({'metric': 'emd_head_1shot_episodes_per_s', 'episodes_per_launch': E, 'problems': E * WAY * QUERY * WAY, 'nodes': N, 'C': C,
                          'value': round(E / (med * 1e-3), 1), 'unit': 'episodes/s', 'ms_per_launch': round(med, 4), 'min_ms': round(lo, 4), 'max_ms': round(hi, 4),
                          'meta_baseline_head_ms_per_launch': round(mb, 4), 'samples': args.steps, 'device': name}))

    # the HiGHS oracle on a sample of the same problems (CPU, float64) and the augmentation histogram of all of them
    cost, w1, w2 = problems_of(shot_tok[:sizes[-1]], query_tok[:sizes[-1]])
    _, status, n_aug = ops.emd_solve(cost, w1, w2, counts=True)
    assert int(status.sum()) == 0
    hist = torch.bincount(n_aug.cpu() // 10).tolist()
    print(json.dumps({'metric': 'emd_augmentations_per_problem', 'problems': int(n_aug.numel()), 'nodes': N, 'min': int(n_aug.min()), 'max': int(n_aug.max()),
                      'mean': round(float(n_aug.float().mean()), 1), 'histogram_bins_of_10': hist, 'bound': 8 * N}))
    if args.oracle_problems > 0:
        import emd_cases as ec
        k = min(args.oracle_problems, cost.shape[0])
        c64, a64, b64 = cost[:k].cpu().double().numpy(), w1[:k].cpu().double().numpy(), w2[:k].cpu().double().numpy()
        t0 = time.perf_counter()
        for i in range(k):
            ec.solve_transport(c64[i], a64[i], b64[i])
        per = (time.perf_counter() - t0) / k
        print(json.dumps({'metric': 'highs_oracle_cpu_ms_per_problem', 'value': round(per * 1e3, 3), 'problems_timed': k,
                          'ms_per_episode_of_375_problems': round(per * 1e3 * WAY * QUERY * WAY, 1), 'note': 'float64 HiGHS oracle on the CPU, not cv2.EMD'}))

    # 2. the whole DeepEMD eval step (encoder + head), 1-shot
    for E in sizes:
        xs1, xq1 = xs5[:E, :, :1].contiguous(), xq[:E].contiguous()
        with torch.no_grad():
            med, lo, hi = timed(lambda: m(xs1, xq1), args.warmup, args.steps)
        m.check_status()
        print(json.dumps({'metric': 'deepemd_eval_step_1shot_episodes_per_s', 'numerics': args.numerics, 'episodes_per_launch': E, 'value': round(E / (med * 1e-3), 1),
                          'unit': 'episodes/s', 'ms_per_launch': round(med, 3), 'min_ms': round(lo, 3), 'max_ms': round(hi, 3), 'samples': args.steps, 'device': name}))

    # 3. the 5-shot SFC path on the token maps: get_sfc (sfc_update_step x ceil(25 / 4) head forward + backward pairs, or the same mini-batch updates
    # in launches of the fused kernel) + the final head
    from fewshot_vit_amd.models.deepemd import SFC_CHUNK
    for E in sfc_sizes:
        s5, q = shot5_tok[:E].contiguous(), query_tok[:E].contiguous()
        final = {}
        for fused in ((False, True) if args.sfc_fused else (False,)):
            g = torch.Generator().manual_seed(0)
            med, lo, hi = timed(lambda: m.emd_forward(m.get_sfc(s5, generator=g, fused=fused), q), 1, max(3, args.steps // 3))
            m.check_status()
            rec = {'metric': 'deepemd_5shot_sfc_fused_episodes_per_s' if fused else 'deepemd_5shot_sfc_episodes_per_s', 'episodes_per_launch': E,
                   'sfc_update_step': args.sfc_steps, 'sfc_bs': 4, 'sfc_lr': 100.0, 'value': round(E / (med * 1e-3), 2), 'unit': 'episodes/s',
                   'ms_per_launch': round(med, 1), 'min_ms': round(lo, 1), 'max_ms': round(hi, 1), 'device': name}
            if fused:
                updates = args.sfc_steps * ((WAY * 5 + 3) // 4)
                launches = (updates + SFC_CHUNK - 1) // SFC_CHUNK
                rec.update({'updates_per_kernel_launch': SFC_CHUNK, 'kernel_launches': launches, 'ms_per_kernel_launch_at_most': round(med / launches, 1)})
            print(json.dumps(rec))
            if args.sfc_fused:
                final[fused] = m.emd_forward(m.get_sfc(s5, generator=torch.Generator().manual_seed(1), fused=fused), q)
                m.check_status()
        if args.sfc_fused:
            same = (final[True].argmax(-1) == final[False].argmax(-1)).float().mean().item()
            print(json.dumps({'metric': 'deepemd_5shot_sfc_fused_vs_unfused_argmax_agreement', 'episodes': E, 'queries': int(final[True].shape[0] * final[True].shape[1]),
                              'value': round(same, 4), 'max_abs_logit_difference': round((final[True] - final[False]).abs().max().item(), 4),
                              'note': 'same permutations on both routes; reported, not asserted'}))


if __name__ == '__main__':
    main()
