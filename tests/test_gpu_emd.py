"""DeepEMD head on the GPU (csrc/emd_head.hip behind ops.emd_solve / ops.emd_head_forward / ops.emd_head_backward, autograd.EmdHeadFn and
models/deepemd.py) against the float64 oracle of tests/emd_cases.py (HiGHS in the place of cv2.EMD).

The bounds come from the number formats and from a float32 numpy prototype of the solver (largest gap to HiGHS 2.2e-6, bound ten times that), none
from what the kernels give.  Measured on an MI355X (DESIGN.md 4f has the table): solver max |sum c F - HiGHS optimum| 7.6e-6 (bound 2e-5), row / column
residual 6.3e-6 at N = 25 (bound 3.7e-5); head forward max |logit - oracle| 1.2e-6 (bound 1e-4; the project's logit criterion is 1e-3); backward 2.4e-7 of
the largest gradient (bound 1e-4); get_sfc 1.7e-7 of the largest entry (bound 1e-4).
"""
import numpy as np
import pytest
import torch

import emd_cases as ec

pytestmark = pytest.mark.gpu
T = 12.5
TINY = dict(img_size=80, init_channels=8, embed_dim=64, depth=[1, 1, 1], num_heads=6, mlp_ratio=4., group=8)


def _ops():
    from fewshot_vit_amd.engine import ops
    return ops


# ---------------------------------------------------------------- 1. the solver alone
@pytest.mark.parametrize('N', [1, 2, 13, 25, 32])
def test_solver_reaches_the_highs_optimum(N):
    kinds, cost, w1, w2 = ec.solver_cases(N)
    flow, status, n_aug = _ops().emd_solve(torch.from_numpy(cost).cuda(), torch.from_numpy(w1).cuda(), torch.from_numpy(w2).cuda(), counts=True)
    flow2, status2 = _ops().emd_solve(torch.from_numpy(cost).cuda(), torch.from_numpy(w1).cuda(), torch.from_numpy(w2).cuda())
    F = flow.cpu().numpy().astype(np.float64)
    assert np.array_equal(flow2.cpu().numpy(), flow.cpu().numpy()) and np.array_equal(status2.cpu().numpy(), status.cpu().numpy())
    worst = dict(gap=0.0, row=0.0, col=0.0)
    per_kind = {}
    for i, kind in enumerate(kinds):
        opt, _ = ec.solve_transport(cost[i], w1[i], w2[i])
        gap = abs(float((cost[i].astype(np.float64) * F[i]).sum()) - opt)
        row = np.abs(F[i].sum(1) - w1[i]).max()
        col = np.abs(F[i].sum(0) - w2[i]).max()
        per_kind[kind] = max(per_kind.get(kind, 0.0), gap)
        worst = dict(gap=max(worst['gap'], gap), row=max(worst['row'], row), col=max(worst['col'], col))
    print(f'emd_solve N={N}: max gap {worst["gap"]:.3e}, row residual {worst["row"]:.3e}, column residual {worst["col"]:.3e}, '
          f'augmentations max {int(n_aug.max())}, per kind ' + ', '.join(f'{k} {v:.1e}' for k, v in per_kind.items()))
    assert int(status.abs().sum()) == 0
    assert F.min() >= 0.0
    assert int(n_aug.max()) <= 8 * N
    resid = N * N * 2.0 ** -24            # worst-case fp32 rounding of N additions of values <= N
    assert worst['row'] <= resid and worst['col'] <= resid, worst
    assert worst['gap'] <= 2e-5, worst


# ---------------------------------------------------------------- 2. head forward
HEAD_CASES = [
    dict(shape=(2, 3, 4, 25, 64), seed=11),
    dict(shape=(1, 5, 6, 13, 512), seed=12),
    dict(shape=(1, 2, 2, 1, 64), seed=13),
    dict(shape=(2, 3, 4, 25, 64), seed=14, constant_token=True),
    dict(shape=(2, 3, 4, 25, 64), seed=15, shared_image=True),
]
_head_cache = {}


def _head_case(i):
    """(shot, query) float64 holding float32 values, oracle logits: computed once, shared by the forward and backward tests, never modified."""
    if i not in _head_cache:
        c = HEAD_CASES[i]
        shot, query = ec.token_case(*c['shape'], seed=c['seed'], constant_token=c.get('constant_token', False), shared_image=c.get('shared_image', False))
        _head_cache[i] = (shot, query, ec.head_oracle(shot, query, T)[0])
    return _head_cache[i]


@pytest.mark.parametrize('i', range(len(HEAD_CASES)))
def test_head_forward_matches_the_oracle(i):
    shot, query, ref = _head_case(i)
    logits, flow, status = _ops().emd_head_forward(shot.float().cuda(), query.float().cuda(), T)
    logits2, none, _ = _ops().emd_head_forward(shot.float().cuda(), query.float().cuda(), T, want_flow=False)
    err = (logits.cpu().double() - ref).abs().max().item()
    print(f'emd_head_forward {HEAD_CASES[i]}: max |logit - oracle| = {err:.3e}')
    assert int(status.abs().sum()) == 0 and none is None
    assert torch.isfinite(logits).all() and torch.equal(logits, logits2)
    assert err <= 1e-4
    E, P, Q, N, C = HEAD_CASES[i]['shape']
    f = flow.cpu().double()
    assert f.min().item() >= 0.0 and (f.sum((-1, -2)) - N).abs().max().item() <= N ** 3 * 2.0 ** -24 + N * 2.0 ** -21      # N rows of residual <= N^2 2^-24, and the fp32 scaling of the weights to sum N
    if HEAD_CASES[i].get('shared_image'):
        assert abs(logits[0, Q - 1, 0].item() - T) <= 1e-4


def test_head_refusals():
    ops = _ops()
    z = lambda *s: torch.zeros(*s, device='cuda')
    with pytest.raises(ValueError):
        ops.emd_head_forward(z(1, 2, 33, 64), z(1, 2, 33, 64), T)
    with pytest.raises(ValueError):
        ops.emd_head_forward(z(1, 2, 5, 96), z(1, 2, 5, 96), T)
    with pytest.raises(ValueError):
        ops.emd_head_forward(z(1, 2, 5, 64), z(1, 2, 5, 64), float('nan'))
    with pytest.raises(ValueError):
        ops.emd_solve(z(2, 33, 33), z(2, 33), z(2, 33))


# ---------------------------------------------------------------- 3. backward, with the GPU's own flows in the oracle
@pytest.mark.parametrize('i', [0, 1])
def test_head_backward_matches_float64_autograd(i):
    from fewshot_vit_amd.autograd import EmdHeadFn
    shot, query, _ = _head_case(i)
    s = shot.float().cuda().requires_grad_(True)
    q = query.float().cuda().requires_grad_(True)
    logits, status = EmdHeadFn.apply(s, q, T)
    dl = torch.randn(logits.shape, generator=torch.Generator().manual_seed(20 + i), dtype=torch.float64)
    (logits * dl.float().cuda()).sum().backward()
    flows = _ops().emd_head_forward(s, q, T)[1].cpu().double()            # deterministic: the flows the backward used
    sc, qc = shot.clone().requires_grad_(True), query.clone().requires_grad_(True)
    ref_logits, _ = ec.head_oracle(sc, qc, T, flows=flows)
    (ref_logits * dl).sum().backward()
    assert int(status.abs().sum()) == 0
    for name, got, ref in (('shot', s.grad, sc.grad), ('query', q.grad, qc.grad)):
        rel = (got.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
        print(f'emd_head_backward {HEAD_CASES[i]["shape"]} d{name}: max deviation / max |grad| = {rel:.3e}')
        assert torch.isfinite(got).all() and rel <= 1e-4


# ---------------------------------------------------------------- 4. the module
def _model(deepemd='fcn', **kw):
    from fewshot_vit_amd import models
    from fewshot_vit_amd.models.visformer import Visformer
    models.register('tiny_visformer_emd')(lambda **a: Visformer(**TINY, **a))
    torch.manual_seed(0)
    return models.make('deepemd', encoder='tiny_visformer_emd', encoder_args={'numerics': 'parity'}, deepemd=deepemd, **kw).cuda()


def _images(*shape, seed):
    return torch.randn(*shape, 3, 80, 80, generator=torch.Generator().manual_seed(seed)).cuda()


def _oracle_on_own_tokens(m, x_shot, x_query, patches):
    E, way, shot = x_shot.shape[:3]
    img = x_shot.shape[3:]
    with torch.no_grad():
        tok = m.encode(torch.cat([x_shot.reshape(-1, *img), x_query.reshape(-1, *img)]), patches).cpu().double()
    n = E * way * shot
    return ec.head_oracle(tok[:n].reshape(E, way, *tok.shape[1:]), tok[n:].reshape(E, -1, *tok.shape[1:]), m.temperature)[0]


def test_module_eval_matches_the_oracle_on_its_own_token_map():
    m = _model().eval()
    x_shot, x_query = _images(1, 2, 1, seed=1), _images(1, 3, seed=2)
    with torch.no_grad():
        logits = m(x_shot, x_query)
    m.check_status()
    ref = _oracle_on_own_tokens(m, x_shot, x_query, False)
    err = (logits.cpu().double() - ref).abs().max().item()
    print(f'DeepEMD eval (25 nodes, C = 128): max |logit - oracle| = {err:.3e}')
    assert logits.shape == (1, 3, 2) and err <= 1e-4


def test_module_grid_input_with_13_nodes():
    m = _model('grid').eval()
    x_shot, x_query = _images(1, 2, 1, 13, seed=3), _images(1, 2, 13, seed=4)
    with torch.no_grad():
        logits = m(x_shot, x_query)
    m.check_status()
    ref = _oracle_on_own_tokens(m, x_shot, x_query, True)
    err = (logits.cpu().double() - ref).abs().max().item()
    print(f'DeepEMD grid eval (13 nodes): max |logit - oracle| = {err:.3e}')
    assert logits.shape == (1, 2, 2) and err <= 1e-4


def test_module_train_matches_the_oracle_and_reaches_every_encoder_parameter():
    m = _model().train()
    x_shot, x_query = _images(1, 2, 1, seed=5), _images(1, 4, seed=6)
    ref = _oracle_on_own_tokens(m, x_shot, x_query, False)               # batch-statistics BatchNorm: the same batch gives the same map
    logits = m(x_shot, x_query)
    label = torch.tensor([0, 1, 0, 1], device='cuda')
    torch.nn.functional.cross_entropy(logits.view(-1, 2), label).backward()
    m.check_status()
    err = (logits.detach().cpu().double() - ref).abs().max().item()
    print(f'DeepEMD train (25 nodes, C = 128): max |logit - oracle| = {err:.3e}')
    assert err <= 1e-4
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert m.encoder.stem.conv1.weight.grad.abs().sum().item() > 0.0


# ---------------------------------------------------------------- 5. SFC
@pytest.mark.parametrize('seed', ec.SFC_SEEDS)
def test_sfc_matches_the_float64_oracle(seed):
    c = ec.SFC_CFG
    shot_maps, perms, ref = ec.sfc_case(seed)
    m = _model(temperature=c['temperature'], sfc_lr=c['lr'], sfc_update_step=c['steps'], sfc_bs=c['bs'])
    sfc = m.get_sfc(shot_maps.float().cuda(), perms=perms)
    m.check_status()
    rel = (sfc.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    moved = (ref - shot_maps.mean(dim=2)).abs().max().item() / ref.abs().max().item()
    print(f'get_sfc seed {seed}: max deviation / max |SFC| = {rel:.3e} (the fine-tune moved the tensor by {moved:.2e} of it)')
    assert sfc.shape == (c['E'], c['way'], c['N'], c['C']) and moved > 0.0
    assert rel <= 1e-4
    # at sfc_lr = 0.1 three steps move the tensor by less than that bound, so the update itself is held too: the fp32 tensor (entries up to ~4, half an
    # ulp 2.4e-7) is rounded once at the initial mean and once per mini-batch step (6 steps) - 1.7e-6 against an update of ~2.7e-4 is 6e-3; 2e-2 with the
    # 1e-4 of the gradients and the momentum arithmetic
    init = shot_maps.mean(dim=2)
    upd = ((sfc.cpu().double() - init) - (ref - init)).abs().max().item() / (ref - init).abs().max().item()
    print(f'get_sfc seed {seed}: deviation of the update / max |update| = {upd:.3e}')
    assert upd <= 2e-2


# ---------------------------------------------------------------- 6. status path (host side: a status tensor filled here, no kernel involved)
def test_nonzero_status_count_makes_the_check_raise():
    m = _model()
    m.add_status(torch.zeros(2, 3, 5, dtype=torch.int32, device='cuda'))
    m.check_status()
    bad = torch.zeros(2, 3, 5, dtype=torch.int32, device='cuda')
    bad[1, 2, 3] = 1
    m.add_status(torch.zeros(2, 3, 5, dtype=torch.int32, device='cuda'))
    m.add_status(bad)
    with pytest.raises(RuntimeError, match='loop bound'):
        m.check_status()
    m.check_status()                                                     # the count starts again after a check
