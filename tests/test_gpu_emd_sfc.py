"""The fused 5-shot SFC fine-tune on the GPU (emd_sfc_kernel in csrc/emd_head.hip behind ops.emd_sfc_steps and DeepEMD.get_sfc(fused=True)): against the
float64 oracle of tests/emd_cases.py on the cases of tests/emd_sfc_cases.py, against the unfused get_sfc on the same permutations, bit-identical under
chunking and repetition, at module level, and its refusals.

The bounds are the ones test_gpu_emd.test_sfc_matches_the_float64_oracle applies to the unfused path (1e-4 of the largest entry, 2e-2 of the largest
update) and the project's 1e-4 for head logits; none comes from what the kernel gives.  Measured on an MI355X: DESIGN.md 4f has the table.
"""
import ctypes

import pytest
import torch

import emd_sfc_cases as sc
from test_gpu_emd import _model

pytestmark = pytest.mark.gpu


def _ops():
    from fewshot_vit_amd.engine import ops
    return ops


def _head(c, **kw):
    return _model(temperature=c['temperature'], sfc_lr=c['lr'], sfc_update_step=c['steps'], sfc_bs=c['bs'], **kw)


# ---------------------------------------------------------------- 1. against the float64 oracle
@pytest.mark.parametrize('name,seed', sc.CASES)
def test_fused_sfc_matches_the_float64_oracle(name, seed):
    c, shot_maps, perms, ref = sc.sfc_case(name, seed)
    m = _head(c, sfc_fused=True)
    sfc = m.get_sfc(shot_maps.float().cuda(), perms=perms)
    count = int(m._status_count.item())
    m.check_status()
    init = shot_maps.mean(dim=2)
    got = sfc.cpu().double()
    rel = (got - ref).abs().max().item() / ref.abs().max().item()
    upd = ((got - init) - (ref - init)).abs().max().item() / (ref - init).abs().max().item()
    moved = (ref - init).abs().max().item() / ref.abs().max().item()
    print(f'fused get_sfc case {name} seed {seed}: max deviation / max |SFC| = {rel:.3e}, deviation of the update / max |update| = {upd:.3e} '
          f'(the fine-tune moved the tensor by {moved:.2e} of its largest entry), status count {count}')
    assert sfc.shape == (c['E'], c['way'], c['N'], c['C']) and torch.isfinite(sfc).all() and moved > 0.0
    assert rel <= 1e-4
    assert upd <= 2e-2
    assert count == 0


# ---------------------------------------------------------------- 2. against the unfused route on the same permutations
@pytest.mark.parametrize('name,seed', [('A', 0), ('B', 0), ('C', 0), ('D', 0), ('E', 0)])
def test_fused_sfc_matches_the_unfused_route(name, seed):
    c, shot_maps, perms, _ = sc.sfc_case(name, seed)
    m = _head(c)
    maps = shot_maps.float().cuda()
    unfused = m.get_sfc(maps, perms=perms)
    fused = m.get_sfc(maps, perms=perms, fused=True)
    m.check_status()
    rel = (fused - unfused).abs().max().item() / unfused.abs().max().item()
    print(f'fused vs unfused get_sfc case {name} seed {seed}: max deviation / max |SFC| = {rel:.3e}')
    assert fused.shape == unfused.shape and rel <= 1e-4


# ---------------------------------------------------------------- 3. chunking and determinism
def _run_table(c, shot_maps, perms, chunk):
    from fewshot_vit_amd.models.deepemd import sfc_step_table
    E, way, shot, N, C = shot_maps.shape
    maps = shot_maps.float().cuda()
    support = maps.permute(0, 2, 1, 3, 4).reshape(E, way * shot, N, C).contiguous()
    label = torch.arange(way).repeat(shot).cuda()
    table = sfc_step_table(perms, c['bs'])
    sfc, buf, count = maps.mean(dim=2).contiguous(), None, None
    for i in range(0, table.shape[0], chunk):
        sfc, buf, count = _ops().emd_sfc_steps(support, label, table[i:i + chunk], sfc, buf, count, temperature=c['temperature'], lr=c['lr'], first=i == 0)
    return sfc, buf, count


@pytest.mark.parametrize('name,seed', [('A', 0), ('B', 0)])
def test_chunked_and_repeated_runs_are_bit_identical(name, seed):
    c, shot_maps, perms, _ = sc.sfc_case(name, seed)
    whole = _run_table(c, shot_maps, perms, 1 << 20)
    single = _run_table(c, shot_maps, perms, 1)              # every launch after the first starts from the stored sfc and buf (first = 0)
    again = _run_table(c, shot_maps, perms, 1 << 20)
    assert whole[2].shape == (c['E'],) and int(whole[2].sum()) == 0
    for other in (single, again):
        assert torch.equal(whole[0], other[0]) and torch.equal(whole[1], other[1]) and torch.equal(whole[2], other[2])
    assert whole[1].abs().max().item() > 0.0
    # and through the module: get_sfc's own chunk loop
    m = _head(c, sfc_fused=True)
    maps = shot_maps.float().cuda()
    assert torch.equal(m.get_sfc(maps, perms=perms), whole[0])
    assert torch.equal(m.get_sfc(maps, perms=perms, chunk=1), whole[0])
    m.check_status()


# ---------------------------------------------------------------- 4. the module: 5-shot, grid input with 13 nodes
def test_module_5shot_grid_fused_matches_unfused():
    x_shot = torch.randn(1, 2, 5, 13, 3, 80, 80, generator=torch.Generator().manual_seed(11)).cuda()
    x_query = torch.randn(1, 2, 13, 3, 80, 80, generator=torch.Generator().manual_seed(12)).cuda()
    logits = {}
    for fused in (False, True):
        m = _model('grid', sfc_update_step=2, sfc_lr=1.0, sfc_fused=fused).eval()
        assert m.sfc_fused is fused
        m.sfc_generator = torch.Generator().manual_seed(5)
        with torch.no_grad():
            logits[fused] = m(x_shot, x_query)
        m.check_status()
    err = (logits[True] - logits[False]).abs().max().item()
    print(f'DeepEMD 5-shot grid (13 nodes, 2 SFC update steps at lr 1.0): max |logit fused - logit unfused| = {err:.3e}')
    assert logits[True].shape == (1, 2, 2) and torch.isfinite(logits[True]).all()
    assert err <= 1e-4


# ---------------------------------------------------------------- 5. refusals (nothing is launched by any of these)
def _c_call(E=1, way=2, n=4, bs=4, N=5, C=64, steps=1, null=None, short=False, temperature=12.5):
    from fewshot_vit_amd import _lib
    lib = _lib.load()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    z = lambda *s: torch.zeros(*s, device='cuda')
    # one episode's worth of zeros at the largest node count: a refused call reads none of it, the two no-ops launch nothing
    buffers = dict(support=z(max(n, 1), 32, 128), label=torch.zeros(max(n, 1), dtype=torch.int32, device='cuda'),
                   ids=torch.zeros(max(steps, 1), max(bs, 1), dtype=torch.int32, device='cuda'), sfc=z(max(way, 1), 32, 128), buf=z(max(way, 1), 32, 128),
                   count=torch.zeros(1, dtype=torch.int32, device='cuda'))
    need = lib.fsvit_emd_sfc_workspace_bytes(E, way, n, bs, N, C)
    ws = torch.zeros(max(need, 16), dtype=torch.uint8, device='cuda')
    p = {k: (None if k == null else ptr(v)) for k, v in buffers.items()}
    rc = lib.fsvit_emd_sfc_steps(p['support'], p['label'], p['ids'], steps, 1, E, way, n, bs, N, C, temperature, 1.0, 0.9, 0.9, p['sfc'], p['buf'], p['count'],
                                 None if null == 'workspace' else ptr(ws), (need - 4) if short else ws.numel(), None)
    return rc, need, lib.fsvit_last_error().decode()


def test_c_entry_refusals():
    from fewshot_vit_amd import _lib
    for kw in (dict(N=33), dict(N=0), dict(C=96), dict(C=0), dict(bs=0), dict(way=0), dict(n=0), dict(steps=-1), dict(E=65536),
               dict(temperature=float('nan')), dict(temperature=float('inf'))):
        rc, need, msg = _c_call(**kw)
        assert rc == _lib.ERR_ARG and 'fsvit_emd_sfc_steps' in msg, (kw, rc, msg)
        if 'steps' not in kw and 'temperature' not in kw:
            assert need == 0, kw
    for null in ('support', 'label', 'ids', 'sfc', 'buf', 'count', 'workspace'):
        rc, _, msg = _c_call(null=null)
        assert rc == _lib.ERR_ARG and 'null' in msg, (null, rc, msg)
    rc, need, msg = _c_call(short=True)
    assert need > 0 and rc == _lib.ERR_WORKSPACE and 'workspace' in msg, (rc, msg)
    assert _c_call(steps=0)[0] == 0 and _c_call(E=0)[0] == 0          # no-ops


def test_op_refuses_a_bad_step_table_before_any_launch():
    ops = _ops()
    E, way, n, bs, N, C = 1, 2, 4, 4, 5, 64
    support = torch.randn(E, n, N, C, device='cuda')
    label = torch.arange(way).repeat(2).cuda()
    start = torch.randn(E, way, N, C, device='cuda')
    for bad in (n, -2):
        sfc = start.clone()
        ids = torch.tensor([[[0, 1, 2, bad]]], dtype=torch.int32)
        with pytest.raises(ValueError):
            ops.emd_sfc_steps(support, label, ids, sfc, temperature=12.5, lr=1.0)
        assert torch.equal(sfc, start)
    with pytest.raises(ValueError):
        ops.emd_sfc_steps(support, label, torch.zeros(1, E, bs, dtype=torch.int32).cuda(), start.clone(), temperature=12.5, lr=1.0)      # a device table
    with pytest.raises(ValueError):
        ops.emd_sfc_steps(support, label, torch.zeros(1, E, bs, dtype=torch.int32), start.clone(), temperature=12.5, lr=1.0, first=False)   # no buf
    for shape in ((E, n, 33, 64), (E, n, 5, 96)):
        with pytest.raises(ValueError):
            ops.emd_sfc_steps(torch.zeros(*shape, device='cuda'), label, torch.zeros(1, E, bs, dtype=torch.int32),
                              torch.zeros(E, way, *shape[2:], device='cuda'), temperature=12.5, lr=1.0)
