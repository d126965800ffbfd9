"""Case table of the fused SFC fine-tune tests (a helper, not a test module): the project's pinned get_sfc case (emd_cases.sfc_case) and four
shapes that take the fused kernel's other paths.  The input recipe is emd_cases.sfc_case's with generator seed 9000 + seed; the oracle is
emd_cases.sfc_oracle (float64, HiGHS).  Every case runs at temperature 12.5; B - E at sfc_lr 1.0 (0.1 moves the 32-node case by 1e-5 of its largest
entry, too close to fp32 resolution)."""
import functools

import torch

import emd_cases as ec

CFGS = {
    'A': dict(ec.SFC_CFG),                                                                     # the project's own pinned case, as it is
    'B': dict(E=2, way=5, shot=2, N=13, C=64, bs=4, steps=2, lr=1.0, temperature=12.5),         # 20 problems per step (> 16 waves), batches 4 / 4 / 2
    'C': dict(E=1, way=2, shot=3, N=25, C=128, bs=4, steps=2, lr=1.0, temperature=12.5),        # the 25-token map, partial batch 4 / 2
    'D': dict(E=1, way=2, shot=2, N=32, C=64, bs=8, steps=2, lr=1.0, temperature=12.5),         # N at its bound, bs > n
    'E': dict(E=1, way=2, shot=2, N=1, C=64, bs=1, steps=1, lr=1.0, temperature=12.5),          # one node, batches of one
}
# (case, seed) pairs the GPU tests run; the CPU test re-runs the stability screen of exactly these.  B's oracle takes a few seconds: one seed.
CASES = [('A', s) for s in ec.SFC_SEEDS] + [('B', 0), ('C', 0), ('C', 1), ('D', 0), ('D', 1), ('E', 0)]


def _inputs(c, seed):
    g = torch.Generator().manual_seed(9000 + seed)
    raw = torch.randn(c['E'], c['way'], c['shot'], c['N'], c['C'], generator=g, dtype=torch.float64) + \
        0.5 * torch.randn(1, 1, 1, 1, c['C'], generator=g, dtype=torch.float64)
    perms = torch.stack([torch.stack([torch.randperm(c['way'] * c['shot'], generator=g) for _ in range(c['E'])]) for _ in range(c['steps'])])
    return raw, perms


def _oracle(c, maps, perms):
    return torch.stack([ec.sfc_oracle(maps[e], perms[:, e], c['temperature'], c['lr'], c['steps'], c['bs']) for e in range(c['E'])])


@functools.lru_cache(maxsize=None)
def sfc_case(name, seed):
    """-> (cfg, shot_maps [E, way, shot, N, C] float64 holding float32 values, perms [steps, E, way * shot], oracle SFC [E, way, N, C]).  Computed once
    per process and shared: callers must not write into the tensors."""
    c = CFGS[name]
    if name == 'A':
        return (c,) + tuple(ec.sfc_case(seed))
    raw, perms = _inputs(c, seed)
    rounded = raw.float().double()
    return c, rounded, perms, _oracle(c, rounded, perms)


def screen(name, seed):
    """emd_cases.sfc_case's stability screen: the float64 oracle on the unrounded inputs against the one on their float32 rounding, as a fraction of
    the largest entry (the screen's bound is 1e-5)."""
    c = CFGS[name]
    if name == 'A':
        return 0.0 if ec.sfc_case(seed, screen=True) is not None else float('inf')
    raw, perms = _inputs(c, seed)
    ref = sfc_case(name, seed)[3]
    return ((_oracle(c, raw, perms) - ref).abs().max() / ref.abs().max()).item()
