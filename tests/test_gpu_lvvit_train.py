"""LV-ViT (lvvit_micro_80) on the HIP trainer: the reference's own train-mode step (tests/golden/lvvit_train_step.npz, made by
tests/golden/make_lvvit_train_golden.py) through the Python surface and the C ABI, the frozen-BatchNorm mean-of-episodes identity,
bit-reproducibility and a short meta-tuning loop."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

_CACHE = {}


def _golden(golden_dir):
    if 'z' not in _CACHE:
        sys.path.insert(0, golden_dir)
        import make_lvvit_train_golden as mk
        z = np.load(os.path.join(golden_dir, 'lvvit_train_step.npz'))
        _CACHE['z'], _CACHE['mk'] = {k: z[k] for k in z.files}, mk
    return _CACHE['z'], _CACHE['mk']


def _step(golden_dir, numerics, frozen, route='gemm'):
    """One step of the golden's inputs on the HIP trainer: (feat, grads, buffers), cached per (numerics, frozen, route) and left unchanged.
    route: the trainer is created under FSVIT_LVVIT_WGRAD=gemm | direct (conv2 / conv3 weight gradients on the transposed split-K GEMM, or on the
    direct kernel of wgrad3x3.hip)."""
    key = (numerics, frozen, route)
    if key in _CACHE:
        return _CACHE[key]
    os.environ['FSVIT_LVVIT_WGRAD'] = route
    try:
        return _step_run(golden_dir, numerics, frozen, key)
    finally:
        os.environ.pop('FSVIT_LVVIT_WGRAD', None)


def _step_run(golden_dir, numerics, frozen, key):
    from fewshot_vit_amd import models
    z, mk = _golden(golden_dir)
    m = models.make('lvvit_micro_80', numerics=numerics)
    assert m.drop_path_rate == 0.5                         # the reference factory's default (lvvit.py:585)
    sd, _ = mk.perturbed_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    if frozen:
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.eval()
    feat = m(torch.from_numpy(z['x']).cuda(), droppath_masks=torch.from_numpy(z['masks']).cuda())
    (feat * torch.from_numpy(z['w']).cuda()).sum().backward()
    torch.cuda.synchronize()
    out = (feat.detach().cpu(), {k: p.grad.detach().cpu() for k, p in m.named_parameters()}, {k: b.detach().cpu().clone() for k, b in m.named_buffers()})
    _CACHE[key] = out
    return out


def _sampled(mk, name, g):
    g = g.contiguous()
    stride = mk.STRIDE if name.startswith('patch_embed.conv') else mk.STRIDE_BLOCKS
    return (g if g.numel() <= mk.FULL_MAX else g.view(-1)[::stride]).numpy()


@pytest.mark.parametrize('rec', ['bn', 'frozen'])
def test_lvvit_train_step_vs_reference_golden(golden_dir, rec):
    """`parity` against the REFERENCE's LV_ViT.train() step (batch-statistics BatchNorm, and every BatchNorm in eval mode): feature, every BatchNorm
    buffer, every stored gradient elementwise and the norm of all 106 gradients.  Errors as in test_vit_train_step_vs_reference_golden: absolute
    over max(1, |reference|max)."""
    z, mk = _golden(golden_dir)
    feat, grads, bufs = _step(golden_dir, 'parity', rec == 'frozen')
    e_feat = float(np.abs(feat.numpy() - z[rec + '.feat']).max())
    e_buf = e_grad = e_norm = 0.0
    k_grad = k_norm = None
    n_grad = 0
    for k, ref in z.items():
        if k.startswith(rec + '.buf.'):
            name = k[len(rec) + 5:]
            if name.endswith('num_batches_tracked'):
                assert int(bufs[name]) == int(ref), name
            else:
                e_buf = max(e_buf, float(np.abs(bufs[name].numpy() - ref).max() / max(1.0, np.abs(ref).max())))
        elif k.startswith(rec + '.grad.'):
            name = k[len(rec) + 6:]
            e = float(np.abs(_sampled(mk, name, grads[name]) - ref).max() / max(1.0, np.abs(ref).max()))
            n_grad += 1
            if e > e_grad:
                e_grad, k_grad = e, name
        elif k.startswith(rec + '.gnorm.'):
            name = k[len(rec) + 7:]
            e = abs(float(grads[name].double().norm()) - float(ref)) / max(1.0, float(ref))
            if e > e_norm:
                e_norm, k_norm = e, name
    print(f'LV-ViT train step [{rec}] vs reference golden: feat {e_feat:.2e}, buffers {e_buf:.2e}, gradients {e_grad:.2e} ({k_grad}), '
          f'norms {e_norm:.2e} ({k_norm})')
    assert n_grad == 106
    # gates: the ViT golden step's 2e-5 (test_vit_train_step_vs_reference_golden) to start from, then 2 x the error measured on the MI355X
    assert e_feat <= 6.2e-6                                # measured 3.1e-6 / 2.9e-6 (2x)
    assert e_buf <= 1.5e-7                                 # measured 7.3e-8 / 0 (2x)
    assert e_grad <= 6.2e-6, k_grad                        # measured 3.1e-6 / 2.9e-6, patch_embed.conv2.weight (2x)
    assert e_norm <= 1.2e-6, k_norm                        # measured 3.6e-7 / 5.9e-7 (2x)


@pytest.mark.parametrize('numerics,gate_feat,gate_grad', [('bf16x2', 8.4e-5, 8.9e-3), ('bf16', 5.5e-2, 0.27)])
def test_lvvit_train_step_modes_vs_parity(golden_dir, numerics, gate_feat, gate_grad):
    """The same step in the two-limb and the 16-bit training mode against the `parity` result: feature (absolute) and every gradient
    (|difference| / |parity gradient|, in norms).  Gates = 2 x measured on the MI355X: bf16x2 feature 4.2e-5, gradients 4.4e-3 (patch_embed.bn2.bias);
    bf16 feature 2.7e-2, gradients 0.135 (patch_embed.bn1.bias: four images through batch-statistics BatchNorm with bf16 activations)."""
    feat_p, grads_p, _ = _step(golden_dir, 'parity', False)
    feat, grads, _ = _step(golden_dir, numerics, False)
    e_feat = float((feat - feat_p).abs().max())
    worst, worst_k = 0.0, None
    for k, g in grads_p.items():
        rel = float((grads[k] - g).norm() / g.norm().clamp_min(1e-6))
        if rel > worst:
            worst, worst_k = rel, k
    print(f'LV-ViT train step [{numerics}] vs parity: feat {e_feat:.2e}, worst gradient rel err {worst:.2e} ({worst_k})')
    assert e_feat <= gate_feat and worst <= gate_grad, (e_feat, worst, worst_k)


def _episodes(E, way=5, shot=1, query=1, seed=3):
    from fewshot_vit_amd import synthetic
    from fewshot_vit_amd.utils import few_shot as fs
    x = synthetic.synthetic_episodes(seed, E, way, shot, query)
    xs, xq = fs.split_shot_query(x, way, shot, query, E)
    return xs.cuda(), xq.cuda(), fs.make_nk_label(way, query, E).cuda()


def _meta_model(numerics):
    from fewshot_vit_amd import models, synthetic
    m = models.make('meta-baseline', encoder='lvvit_micro_80', encoder_args={'numerics': numerics})
    m.load_state_dict(synthetic.synthetic_checkpoint_sd({k: tuple(v.shape) for k, v in m.state_dict().items()}, calib='lvvit_micro_80'), strict=True)
    return m.cuda().train()


def test_frozen_bn_step_equals_mean_of_single_episode_steps():
    """With utils.freeze_bn and fixed DropPath masks every image is independent: the parameter gradients of a 2-episode MetaBaseline step
    (5-way 1-shot 1-query, 20 images) equal the mean of the two single-episode steps.  `parity`, at the gate of the Visformer test
    (test_full_size_800_image_step_equals_mean_of_single_episode_steps: 2e-5 relative in norms)."""
    from fewshot_vit_amd import utils
    E, way, shot, query = 2, 5, 1, 1
    m = _meta_model('parity')
    utils.freeze_bn(m)
    xs, xq, label = _episodes(E, way, shot, query)
    n_shot = E * way * shot
    keep = m.encoder.trainer().droppath_keep(0.5)
    assert len(keep) == m.encoder.trainer().n_droppath_calls(0.5) == 14
    g = torch.Generator().manual_seed(7)
    masks = torch.stack([(k + torch.rand(2 * n_shot, generator=g)).floor() for k in keep]).cuda()

    def run(xs_, xq_, label_, mk):
        m.encoder.draw_droppath_masks = lambda n, dev: mk
        m.zero_grad(set_to_none=True)
        loss = F.cross_entropy(m(xs_, xq_).view(-1, way), label_)
        loss.backward()
        torch.cuda.synchronize()
        return float(loss.detach()), {k: p.grad.detach().clone() for k, p in m.named_parameters()}

    loss_full, g_full = run(xs, xq, label, masks)
    assert np.isfinite(loss_full) and all(torch.isfinite(v).all() for v in g_full.values())
    per = way * shot
    acc = {k: torch.zeros_like(v) for k, v in g_full.items()}
    loss_sum = 0.0
    for e in range(E):
        mk = torch.cat([masks[:, e * per:(e + 1) * per], masks[:, n_shot + e * way * query:n_shot + (e + 1) * way * query]], dim=1).contiguous()
        l, ge = run(xs[e:e + 1], xq[e:e + 1], label[e * way * query:(e + 1) * way * query], mk)
        loss_sum += l
        for k in acc:
            acc[k] += ge[k] / E
    assert abs(loss_full - loss_sum / E) <= 1e-5 * max(1.0, abs(loss_full))
    worst, worst_k = 0.0, None
    for k, v in g_full.items():
        n = float(acc[k].norm())
        if n <= 1e-6:
            assert float(v.abs().max()) <= 1e-5, k
            continue
        rel = float((v - acc[k]).norm()) / n
        if rel > worst:
            worst, worst_k = rel, k
    print(f'LV-ViT 2-episode step vs mean of single-episode steps: worst gradient rel err {worst:.2e} ({worst_k})')
    assert worst <= 2e-5, (worst, worst_k)


@pytest.mark.parametrize('numerics', ['parity', 'bf16x2', 'bf16'])
def test_two_identical_steps_are_bit_identical(golden_dir, numerics):
    from fewshot_vit_amd import models
    z, mk = _golden(golden_dir)
    m = models.make('lvvit_micro_80', numerics=numerics)
    sd, _ = mk.perturbed_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    x, w, masks = torch.from_numpy(z['x']).cuda(), torch.from_numpy(z['w']).cuda(), torch.from_numpy(z['masks']).cuda()
    runs = []
    for _ in range(2):
        m.load_state_dict(sd, strict=True)                 # (the first step moved the BatchNorm running statistics)
        m = m.cuda().train()
        m.zero_grad(set_to_none=True)
        feat = m(x, droppath_masks=masks)
        (feat * w).sum().backward()
        torch.cuda.synchronize()
        runs.append((feat.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


def test_twelve_step_meta_tuning_lowers_the_loss():
    """train_meta.py:155-177 on synthetic episodes: SGD with the reference's optimizer args (lr 5e-4 is the YAML's; here the loop's own lr so that
    twelve steps move the loss), `parity` and `bf16` from the same start; the bf16 losses stay in a band around parity's."""
    from fewshot_vit_amd import utils
    xs, xq, label = _episodes(2, 5, 1, 3, seed=4)
    traj = {}
    for numerics in ('parity', 'bf16'):
        m = _meta_model(numerics)
        opt, _ = utils.make_optimizer(m.parameters(), 'sgd', lr=0.01, weight_decay=5e-4)
        torch.manual_seed(0)
        losses = []
        for _ in range(12):
            loss = F.cross_entropy(m(xs, xq).view(-1, 5), label)
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        traj[numerics] = losses
        assert all(np.isfinite(losses)), losses
    band = max(abs(a - b) for a, b in zip(traj['parity'], traj['bf16']))
    print('LV-ViT 12-step loss, parity:', ' '.join(f'{v:.4f}' for v in traj['parity']))
    print('LV-ViT 12-step loss, bf16:  ', ' '.join(f'{v:.4f}' for v in traj['bf16']), f'| worst |difference| {band:.3e}')
    for numerics in traj:
        assert min(traj[numerics][-3:]) < traj[numerics][0], (numerics, traj[numerics])
    assert band <= 1.3e-3, band                            # measured 6.4e-4 (2x)


# ---------------------------------------------------------------- the 96 -> 96 weight-gradient operator (wgrad3x3.hip, 3 x 3 job grid)
# B=1 8x8: exactly one 64-row chunk; B=2 6x10: 120 rows, a partial last chunk, W no multiple of 8; B=3 40x40: the stem's width, several row splits
WG96_SHAPES = [(1, 8, 8), (2, 6, 10), (3, 40, 40)]


def _wg96_inputs(shape):
    B, H, W = shape
    g = torch.Generator().manual_seed(23 + B + H)
    return torch.randn(B, 96, H, W, generator=g), torch.randn(B, 96, H, W, generator=g) * 0.1


@pytest.mark.parametrize('shape', WG96_SHAPES)
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_conv3x3_wgrad_96_direct_vs_torch(shape, dtype):
    """fsvit_conv3x3_wgrad at O = Ig = 96 vs torch.nn.grad.conv2d_weight in fp32 on the same 16-bit-rounded operands, at the gate of
    test_conv3x3_wgrad_direct_vs_torch (2e-4 * max(1, |dW|max)); corner tap separately; two calls bit-identical."""
    from fewshot_vit_amd.engine import ops
    x, dz = _wg96_inputs(shape)
    x, dz = x.to(dtype).float(), dz.to(dtype).float()
    ref = torch.nn.grad.conv2d_weight(x, (96, 96, 3, 3), dz, padding=1)
    args = (x.permute(0, 2, 3, 1).contiguous().to('cuda', dtype), dz.permute(0, 2, 3, 1).contiguous().to('cuda', dtype), 96, 96, 1)
    got = ops.conv3x3_wgrad(*args).cpu()
    err = (got - ref).abs().max().item()
    print(f'conv3x3_wgrad 96 {shape} {dtype}: max err {err:.3e} (max |dW| {ref.abs().max():.2f})')
    gate = 2e-4 * max(1.0, ref.abs().max().item())
    assert got.shape == ref.shape and err <= gate
    assert (got[:, :, 0, 0] - ref[:, :, 0, 0]).abs().max().item() <= gate
    assert torch.equal(got, ops.conv3x3_wgrad(*args).cpu())


@pytest.mark.parametrize('shape', WG96_SHAPES)
@pytest.mark.parametrize('limbs', ['bf16', 'f16'])
def test_conv3x3_wgrad_96_two_limb_vs_fp64(shape, limbs):
    """The two-limb form on fp32 activations vs fp64, at the gates of test_conv3x3_wgrad_two_limb_vs_fp64 (3e-5 / 2e-6 of the sum of |products|)."""
    from fewshot_vit_amd.engine import ops
    x, dz = _wg96_inputs(shape)
    ref = torch.nn.grad.conv2d_weight(x.double(), (96, 96, 3, 3), dz.double(), padding=1)
    scale = torch.nn.grad.conv2d_weight(x.double().abs(), (96, 96, 3, 3), dz.double().abs(), padding=1).max().item()
    args = (x.permute(0, 2, 3, 1).contiguous().cuda(), dz.permute(0, 2, 3, 1).contiguous().cuda(), 96, 96, 1, limbs)
    got = ops.conv3x3_wgrad(*args).cpu().double()
    err = (got - ref).abs().max().item()
    print(f'conv3x3_wgrad 96 two-limb {shape} {limbs}: max err {err:.3e} (sum |products| {scale:.1f})')
    gate = (3e-5 if limbs == 'bf16' else 2e-6) * scale
    assert err <= gate and (got[:, :, 0, 0] - ref[:, :, 0, 0]).abs().max().item() <= gate
    assert torch.equal(got, ops.conv3x3_wgrad(*args).cpu().double())


@pytest.mark.parametrize('numerics', ['bf16', 'bf16x2'])
def test_wgrad96_direct_and_gemm_routes_agree(golden_dir, numerics):
    """The golden step under FSVIT_LVVIT_WGRAD=gemm and =direct: the forward and every data gradient are the same launches, so the features are
    bit-identical and conv2 / conv3 weight gradients, compared in full, differ by fp32 summation order only - held to the 16-bit operator gate
    2e-4 * max(1, |dW|max) in both modes.  For bf16x2 this is not looser than the two-limb operator gate (3e-5 of the sum of |products|, which
    cannot be formed here: the trainer hands out neither the layers' inputs nor their output gradients): over M = 4 * 40 * 40 = 6400 mixed-sign
    products per element that sum is about sqrt(M) = 80 x |dW|, i.e. the two-limb gate is about 2.4e-3 |dW| against 2e-4 here; the two-limb gate
    itself is held per shape in test_conv3x3_wgrad_96_two_limb_vs_fp64."""
    feat_g, g_g, _ = _step(golden_dir, numerics, False)
    feat_d, g_d, _ = _step(golden_dir, numerics, False, route='direct')
    assert torch.equal(feat_d, feat_g)
    for k in ('patch_embed.conv2.weight', 'patch_embed.conv3.weight'):
        err = float((g_d[k] - g_g[k]).abs().max())
        print(f'LV-ViT [{numerics}] {k}: direct vs gemm route max |difference| {err:.3e} (max |dW| {float(g_g[k].abs().max()):.3f})')
        assert err <= 2e-4 * max(1.0, float(g_g[k].abs().max())), k
    for k in g_d:
        if k not in ('patch_embed.conv2.weight', 'patch_embed.conv3.weight'):
            assert torch.equal(g_d[k], g_g[k]), k


# ---------------------------------------------------------------- stem kernels at C = 96, M no multiple of the row tile
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_stem_kernels_at_96_channels_partial_row_tile(dt):
    """BatchNorm train forward / backward and the stem tail forward / backward at C = 96 with a row count that no row tile divides (203 = 7 x 29 rows for BatchNorm;
    3 x 10 x 14 = 420 rows for the tail): the checks, float64 references and bounds are those of
    test_gpu_train_ops.py, called at these cases."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_gpu_train_ops as tto
    tto.test_bn_train_forward((203, 96), dt, 'plain')
    tto.test_bn_train_forward((203, 96), dt, 'add_res_act')
    tto.test_bn_train_backward((203, 96), dt, 'plain')
    tto.test_bn_train_backward((203, 96), dt, 'act_acc_out2')
    tto.test_stem_tail((3, 5, 7, 96), 'res_bn_pos', dt)
    tto.test_stem_tail((3, 5, 7, 96), 'res', dt)


# ---------------------------------------------------------------- driver
def test_train_meta_driver_lvvit_one_epoch(tmp_path):
    """train_meta from a reference-style YAML with encoder: lvvit_micro_80 and freeze_bn: one epoch of 2 batches, a checkpoint in the reference's
    dict schema, read back by models.load and by evaluate()."""
    import yaml
    from fewshot_vit_amd import models, test_few_shot, train_meta
    text = """
train_dataset: synthetic-episodes
train_dataset_args: {split: train, n_classes: 12, n_per_class: 30, noise: 1.0, seed: 1}
tval_dataset: synthetic-episodes
tval_dataset_args: {split: test, n_classes: 6, n_per_class: 30, noise: 1.0, seed: 0}
val_dataset: synthetic-episodes
val_dataset_args: {split: val, n_classes: 6, n_per_class: 30, noise: 1.0, seed: 2}
model: meta-baseline
model_args:
    encoder: lvvit_micro_80
    encoder_args: {}
synthetic_checkpoint: lvvit_micro_80
freeze_bn: True
n_train_way: 5
n_train_shot: 1
n_train_query: 3
n_way: 5
n_shot: 1
n_query: 15
train_batches: 2
eval_batches: 1
ep_per_batch: 2
max_epoch: 1
optimizer: sgd
optimizer_args: {lr: 0.0005, weight_decay: 5.e-4, milestones: [20, 40]}
"""
    config = yaml.safe_load(text)
    lines = []
    trlog = train_meta.main(config, name='lv', device=torch.device('cuda', 0), log=lines.append, save_root=str(tmp_path))
    assert len(trlog['tl']) == 1 and all(np.isfinite(trlog[k]).all() for k in ('tl', 'ta', 'vl', 'va'))
    path = os.path.join(str(tmp_path), 'lv', 'epoch-last.pth')
    ck = torch.load(path, map_location='cpu')
    assert ck['model'] == 'meta-baseline' and ck['model_args']['encoder'] == 'lvvit_micro_80' and ck['training']['epoch'] == 1
    assert set(ck) >= {'model', 'model_args', 'model_sd', 'training'}
    m = models.load(ck)
    assert m.encoder.out_dim == 384
    out = test_few_shot.evaluate(dict(dataset='synthetic-episodes', dataset_args=dict(split='test', n_classes=6, n_per_class=30, noise=1.0, seed=0), load=path),
                                 shot=1, test_epochs=1, n_batch=2, ep_per_batch=2, log=lines.append)
    assert out is not None
