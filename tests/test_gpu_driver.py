"""The episodic eval driver (reference test_few_shot.py surface) on one GPU."""
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config():
    return yaml.safe_load(open(os.path.join(REPO, 'few-shot-vit_amd', 'configs', 'test_synthetic.yaml')))


def test_driver_matches_oracle_and_is_launch_size_invariant():
    from fewshot_vit_amd import datasets, synthetic, test_few_shot
    from fewshot_vit_amd.datasets.samplers import CategoriesSampler
    from oracle import fewshot_oracle as fo
    from oracle import visformer_oracle as vo
    cfg = _config()
    logs = []
    a = test_few_shot.evaluate(cfg, shot=1, n_batch=6, launch_batches=4, numerics='bf16', log=logs.append)
    b = test_few_shot.evaluate(cfg, shot=1, n_batch=6, launch_batches=1, numerics='bf16', log=logs.append)
    assert a['va_lst'] == b['va_lst'] and a['n'] == 6            # batching per launch does not change any episode
    assert any(l.startswith('test epoch 1: acc=') for l in logs)
    # oracle on the first two episodes of the same seeded stream
    ds = datasets.make(cfg['dataset'], **cfg['dataset_args'])
    vcfg = vo.VisformerCfg()
    shapes = vo.state_dict_shapes(vcfg, prefix='encoder.')
    shapes['temp'] = ()
    sd = synthetic.synthetic_checkpoint_sd(shapes)
    np.random.seed(12345)
    label = fo.make_nk_label(5, 15, 1)
    for e, idx in enumerate(CategoriesSampler(ds.label, 2, 5, 16, 1)):
        x = torch.stack([ds[int(i)][0] for i in idx])
        xs, xq = fo.split_shot_query(x.numpy(), 5, 1, 15, 1)
        logits = vo.meta_baseline_forward(sd, torch.from_numpy(xs), torch.from_numpy(xq), vcfg)[0].numpy()
        assert a['va_lst'][e] == pytest.approx(fo.compute_acc(logits, label), abs=0.0401)   # <= 3 of 75 near-tie flips in bf16
    p = test_few_shot.evaluate(cfg, shot=1, n_batch=2, launch_batches=2, numerics='parity', log=logs.append)
    np.random.seed(12345)
    for e, idx in enumerate(CategoriesSampler(ds.label, 2, 5, 16, 1)):
        x = torch.stack([ds[int(i)][0] for i in idx])
        xs, xq = fo.split_shot_query(x.numpy(), 5, 1, 15, 1)
        logits = vo.meta_baseline_forward(sd, torch.from_numpy(xs), torch.from_numpy(xq), vcfg)[0].numpy()
        assert p['va_lst'][e] == pytest.approx(fo.compute_acc(logits, label), abs=1e-6)      # exact-fp32 mode: same arg-max


def test_accuracy_agreement_bf16_vs_parity_2000_episodes():
    """north_star: "reported 5-way accuracy within its own +-CI on identical episode seeds" (VERDICT r01 row g / weak #3).  The parity
    mode is pinned to the reference at 1e-3 in the logits, so it stands in for the reference here: the SAME 2000 seeded 5-way 5-shot
    episodes (CategoriesSampler stream, np.random.seed(12345)) through both numerics modes -
      * mean accuracies differ by less than the 95 % CI (in fact by far less),
      * per-query arg-max agreement >= 98 %,
      * no per-batch accuracy moves by more than 5 of 75 queries (measured: 4).
    Difficulty: noise 1.0 puts the accuracy at ~80 %, where the reference sits on miniImageNet (83.25 %) - 30 % of the
    queries then have a top-2 logit gap below 0.1 (tools/calib_noise.py), so bf16's 1e-2..6e-2 logit noise flips ~1.2 % of the
    arg-maxes, symmetrically (measured 98.8 % agreement, accuracies 80.46 vs 80.48 %).  99.5 % is reached at noise 0.85 (97 % accuracy)."""
    from fewshot_vit_amd import test_few_shot
    cfg = _config()
    cfg['dataset_args'] = dict(cfg['dataset_args'], noise=1.0)
    logs = []
    n = 2000
    a = test_few_shot.evaluate(cfg, shot=5, n_batch=n, launch_batches=64, numerics='bf16', log=logs.append, collect_pred=True)
    p = test_few_shot.evaluate(cfg, shot=5, n_batch=n, launch_batches=32, numerics='parity', log=logs.append, collect_pred=True)
    va, vp = np.array(a['va_lst']), np.array(p['va_lst'])
    assert len(va) == n and len(vp) == n
    agree = float((a['pred'] == p['pred']).float().mean())
    dmean = abs(a['acc'] - p['acc'])
    print(f"[agreement] bf16 acc {a['acc']:.4f} +- {a['ci']:.4f}, parity acc {p['acc']:.4f} +- {p['ci']:.4f}, |dmean| {dmean:.5f}, "
          f"argmax agreement {agree:.5f}, max per-batch |dacc| {np.abs(va - vp).max():.4f}")
    assert 0.6 < p['acc'] < 0.95                                         # the episodes are neither chance nor saturated
    assert dmean <= p['ci']
    assert agree >= 0.98
    assert np.abs(va - vp).max() <= 5.5 / 75.0


def test_accuracy_agreement_f16_vs_parity_2000_episodes():
    """The same gate for `--numerics f16` (the same-rate mode with 8 x tighter logits must be gated like the default): the same 2000
    seeded episodes through fp16 storage + MFMA and through exact fp32 - arg-max agreement >= 99.7 % (bench, 2048 episodes: 99.85 %), the mean
    accuracies closer than a fifth of the CI, no per-batch accuracy off by more than 2 of 75 queries."""
    from fewshot_vit_amd import test_few_shot
    cfg = _config()
    cfg['dataset_args'] = dict(cfg['dataset_args'], noise=1.0)
    logs = []
    n = 2000
    a = test_few_shot.evaluate(cfg, shot=5, n_batch=n, launch_batches=64, numerics='f16', log=logs.append, collect_pred=True)
    p = test_few_shot.evaluate(cfg, shot=5, n_batch=n, launch_batches=32, numerics='parity', log=logs.append, collect_pred=True)
    va, vp = np.array(a['va_lst']), np.array(p['va_lst'])
    agree = float((a['pred'] == p['pred']).float().mean())
    dmean = abs(a['acc'] - p['acc'])
    print(f"[agreement] f16 acc {a['acc']:.4f} +- {a['ci']:.4f}, parity acc {p['acc']:.4f} +- {p['ci']:.4f}, |dmean| {dmean:.5f}, "
          f"argmax agreement {agree:.5f}, max per-batch |dacc| {np.abs(va - vp).max():.4f}")
    assert 0.6 < p['acc'] < 0.95
    assert dmean <= 0.2 * p['ci']
    assert agree >= 0.997
    assert np.abs(va - vp).max() <= 2.5 / 75.0


def test_engine_logs_its_numerics_mode_once(capfd):
    """`models.make(...)` + the first engine build says which numerics mode it runs in and what that means for the logits (stderr, once per process and mode)."""
    from fewshot_vit_amd import engine as eng, models, synthetic
    eng._numerics_logged.clear()
    for _ in range(2):
        m = models.make('meta-baseline', encoder='visformer_micro_80', encoder_args={'numerics': 'bf16'})
        m.load_state_dict(synthetic.synthetic_checkpoint_sd({k: tuple(v.shape) for k, v in m.state_dict().items()}), strict=True)
        m.cuda().eval().encoder.engine()
    err = capfd.readouterr().err
    assert err.count("numerics mode 'bf16'") == 1 and '5e-2' in err and 'FSVIT_NUMERICS=f16' in err


def test_bench_rank_launcher_route_on_a_gpu_box():
    """`bench.py --gpus N` invoked plainly starts its ranks from a parent that never touches the GPU (device count by a throw-away child);
    `--via-launcher` sends the 1-GPU run down that same child-spawn route, so it runs once where GPUs exist."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--via-launcher', '--steps', '3', '--warmup', '1', '--episodes', '16',
                        '--chunk', '1600', '--full', '--no-modes', '--no-cpu-baseline', '--no-legs'], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line['n_gpus'] == 1 and line['steps'] == 3 and line['value'] > 0 and line['roofline']['kernel']
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '64', '--steps', '1'], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 2 and 'GPU(s) visible' in r.stderr


def test_bench_plain_run_dumps_its_last_step(tmp_path):
    """A plain `bench.py` times the headline only, and --dump-outputs writes what its last timed step returned; two runs with the same
    arguments see the same seeded episodes, so their outputs agree."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    dumps = []
    for run in range(2):
        d = tmp_path / ('run%d' % run)
        r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--episodes', '16',
                            '--chunk', '1600', '--dump-outputs', str(d)], capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line['steps'] == 3 and line['ms_per_step'] > 0 and line['value'] > 0 and line['unit'] == 'episodes/s' and line['dtype'] == 'bf16'
        assert line['config']['distinct_episode_batches'] == 3
        assert not {'roofline', 'kernels', 'modes', 'agreement', 'legs', 'cpu_baseline'} & set(line)
        out = {k: np.load(d / (k + '.npy')) for k in ('logits', 'accuracy', 'loss')}
        assert out['logits'].shape == (16, 75, 5) and out['accuracy'].shape == (16,) and out['loss'].shape == (16,)
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in out.values())
        label = np.repeat(np.arange(5), 15)
        assert np.allclose(out['accuracy'], (out['logits'].argmax(-1) == label).mean(-1), atol=1e-6)
        dumps.append(out)
    assert np.abs(dumps[0]['logits'] - dumps[1]['logits']).max() <= 1e-4


RCCL_CHILD = r'''
import os, sys
sys.path.insert(0, %r)
import torch
import torch.distributed as dist
from fewshot_vit_amd import parallel
os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=os.environ.get('MASTER_PORT', '29731'), WORLD_SIZE='1', RANK='0', LOCAL_RANK='0')
torch.cuda.set_device(0)
dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))      # backend "nccl" IS RCCL on ROCm
assert dist.get_backend() == 'nccl'
# the exchanges of the N > 1 paths, on a communicator of one rank: the flat gradient bucket (train_meta.py step), the fp64 statistics
# all-reduce and the all-gather of per-batch accuracies (test_few_shot.py)
m = torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.Linear(32, 8)).cuda()
bucket = parallel.GradBucket(m)                      # every .grad is a view of ONE flat buffer
m(torch.randn(16, 64, device='cuda')).square().mean().backward()
ref = bucket.flat.clone()
assert float(ref.abs().sum()) > 0
bucket.allreduce_mean()                              # (world 1: collects only)
dist.all_reduce(bucket.flat)                         # the collective allreduce_mean() issues for world > 1, on the bucket itself
torch.cuda.synchronize()
assert torch.equal(bucket.flat, ref) and all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(bucket.params, bucket.views))
s = torch.tensor([1.5, 2.5, 3.0], dtype=torch.float64, device='cuda')
dist.all_reduce(s)
assert s.tolist() == [1.5, 2.5, 3.0]
v = torch.arange(6, dtype=torch.float32, device='cuda')
out = [torch.empty_like(v)]
dist.all_gather(out, v)
assert torch.equal(out[0], v)
big = torch.ones(25 << 20, dtype=torch.bfloat16, device='cuda')       # a 50 MB bucket: the size of the Visformer-S gradient exchange
dist.all_reduce(big)
torch.cuda.synchronize()
assert float(big.float().sum()) == float(25 << 20)
dist.barrier()
dist.destroy_process_group()
print('rccl-ok')
''' % REPO


def test_rccl_communicator_runs_the_exchanges_of_the_multi_gpu_paths():
    """'RCCL has never run in this project'.  One-GPU boxes cannot measure scaling, but they can run the collectives: a child process
    (HSA_ENABLE_IPC_MODE_LEGACY=0 as exported on the pool) creates an RCCL communicator of one rank and runs the GradBucket all-reduce, the fp64
    statistics all-reduce, the accuracy all-gather and a 50 MB bf16 all-reduce through it."""
    import subprocess
    import sys
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, '-c', RCCL_CHILD], capture_output=True, text=True, timeout=600, env=env, cwd=REPO)
    assert r.returncode == 0 and 'rccl-ok' in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


@pytest.mark.parametrize('numerics,tol', [('parity', 1e-3), ('bf16x2', 1e-3), ('f16', 2e-2), ('bf16', 0.12)])
def test_reference_written_checkpoints_drop_in(golden_dir, monkeypatch, numerics, tol):
    """tests/golden/ref_ckpt_*.pth are the REFERENCE's own torch.save output (train_meta.py:241-257 schema, tiny Visformer; tests/golden/make_golden.py
    checkpoint_golden) and ref_ckpt_expected.npz the logits the reference computes from them.  `models.load` of the `meta-baseline` checkpoint, of the
    `classifier` one (test_phase/models/classifier.py:11-24), and the `load_encoder:` route of test_few_shot.py:55-63 must reproduce them: within 1e-3
    in the 1e-3-grade modes (the encoder_args in the file are the reference's - empty - so the mode comes from FSVIT_NUMERICS as for a drop-in user)."""
    from fewshot_vit_amd import models, synthetic
    from fewshot_vit_amd.utils import few_shot as fs
    from test_boundary_cpu import _register_tiny
    _register_tiny()
    monkeypatch.setenv('FSVIT_NUMERICS', numerics)
    z = np.load(os.path.join(golden_dir, 'ref_ckpt_expected.npz'))
    x = synthetic.synthetic_episodes(51, 1, 5, 1, 3)
    xs, xq = fs.split_shot_query(x, 5, 1, 3, 1)
    m = models.load(torch.load(os.path.join(golden_dir, 'ref_ckpt_meta_baseline.pth'), map_location='cpu', weights_only=False)).cuda().eval()
    with torch.no_grad():
        got = m(xs.cuda(), xq.cuda()).cpu().numpy()
    d_mb = np.abs(got - z['meta_baseline.logits']).max()
    cls = models.load(torch.load(os.path.join(golden_dir, 'ref_ckpt_classifier.pth'), map_location='cpu', weights_only=False)).cuda().eval()
    fresh = models.make('meta-baseline', encoder=None)
    fresh.encoder = cls.encoder
    fresh = fresh.cuda().eval()
    with torch.no_grad():
        got_le = fresh(xs.cuda(), xq.cuda()).cpu().numpy()
        got_cls = cls(x[:6].cuda()).float().cpu().numpy()
    d_le = np.abs(got_le - z['load_encoder.logits']).max()
    d_cls = np.abs(got_cls - z['classifier.logits']).max()
    print(f'[{numerics}] reference checkpoints: max|dlogit| meta-baseline {d_mb:.3e}, load_encoder {d_le:.3e}, classifier {d_cls:.3e}')
    assert d_mb <= tol and d_le <= tol and d_cls <= tol
    if numerics in ('parity', 'bf16x2'):
        assert (got.argmax(-1) == z['meta_baseline.logits'].argmax(-1)).all()
