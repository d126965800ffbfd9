"""Parity of the HIP meta-tuning step (meta_tuning_sun_m/train_meta.py:161-177): train-mode
forward (batch-statistics BN, DropPath), loss.backward() and the SGD update, all through the C-ABI, against

  * the reference's own training step on the tiny Visformer (tests/golden/tiny_train_step.npz), and
  * torch.autograd of the oracle on visformer_micro_80 with the same seeded inputs and DropPath draws.

Tolerances: `parity` numerics (fp32 storage + exact fp32 MFMA) must reproduce every parameter gradient to 1e-3 of
its norm and the logits to the north_star 1e-3; the `bf16` throughput mode is bounded loosely and its measured
deviation printed."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TINY = dict(img_size=80, init_channels=8, embed_dim=64, depth=[2, 1, 2], num_heads=6, mlp_ratio=4., group=8)


def _cpu_masks(seed, rates, depth0, n_img):
    """The reference's DropPath draws from the CPU generator (visformer.py:93-95), in call order."""
    torch.manual_seed(seed)
    rows = []
    for b, r in enumerate(rates):
        if r > 0:
            for _ in range(1 if b < depth0 else 2):
                rows.append((1.0 - r + torch.rand((n_img, 1, 1, 1))).floor_().reshape(-1))
    return torch.stack(rows) if rows else None


def _make(encoder_kwargs, sd, numerics, drop_path_rate):
    from fewshot_vit_amd.models.meta_baseline import MetaBaseline
    from fewshot_vit_amd.models import register
    from fewshot_vit_amd.models.visformer import Visformer
    register('_test_visformer')(lambda **kw: Visformer(**encoder_kwargs, **kw))
    m = MetaBaseline('_test_visformer', encoder_args={'numerics': numerics, 'drop_path_rate': drop_path_rate})
    m.load_state_dict(sd, strict=True)
    return m.cuda().train()


def _layer_group(k):
    for tag in ('stem', 'stage1', 'patch_embed2', 'stage2', 'patch_embed3', 'stage3', 'pos_embed', 'norm'):
        if ('encoder.' + tag) in k or k.startswith(tag):
            return tag
    return 'other'


def _grad_check(named_grads, ref, rel_tol, what, noise_tol=1e-5, group_tol=None):
    worst = 0.0
    groups = {}
    for k, g in named_grads.items():
        r = ref[k]
        scale = float(r.norm())
        err = float((g.cpu() - r).norm())
        rel = err / (scale + 1e-12)
        if scale <= 1e-5:
            # analytically zero gradients (a per-channel constant in front of a train-mode BatchNorm: the PatchEmbed conv
            # bias, and the PatchEmbed norm's beta, which rides the residual stream into the next BatchNorm): both sides
            # hold rounding noise only
            assert float(g.abs().max()) <= noise_tol, f'{what}: grad of {k} should vanish, max {float(g.abs().max()):.3e}'
        else:
            worst = max(worst, rel)
            grp = _layer_group(k)
            groups[grp] = max(groups.get(grp, 0.0), rel)
            tol = rel_tol if group_tol is None else group_tol.get(grp, rel_tol)
            assert rel <= tol, f'{what}: grad of {k}: rel err {rel:.3e} (norm {scale:.3e}, gate {tol:.3e})'
    print(f'{what}: worst gradient rel err per layer group: ' + ', '.join(f'{g} {v:.2e}' for g, v in groups.items()))
    return worst


@pytest.mark.parametrize('numerics', ['parity', 'bf16', 'bf16x2'])
def test_tiny_train_step_vs_reference_golden(golden_dir, numerics):
    from fewshot_vit_amd import synthetic
    from fewshot_vit_amd.utils import few_shot as fs
    from oracle import visformer_oracle as vo
    z = np.load(os.path.join(golden_dir, 'tiny_train_step.npz'))
    cfg = vo.VisformerCfg(img_size=80, init_channels=8, embed_dim=64, depth=(2, 1, 2), num_heads=6, mlp_ratio=4.0, group=8)
    shapes = vo.state_dict_shapes(cfg, prefix='encoder.')
    shapes['temp'] = ()
    sd = synthetic.procedural_state_dict(shapes)
    for k in z.files:
        if k.startswith('bnpre.'):
            sd[k[len('bnpre.'):]] = torch.from_numpy(z[k])
    m = _make(TINY, sd, numerics, 0.5)
    x = synthetic.synthetic_episodes(33, 2, 3, 2, 2)
    xs, xq = fs.split_shot_query(x, 3, 2, 2, 2)
    label = torch.arange(3).repeat_interleave(2).repeat(2).cuda()
    rates = torch.linspace(0, 0.5, 5).tolist()
    masks = _cpu_masks(77, rates, 2, 24).cuda()
    m.encoder.draw_droppath_masks = lambda n, dev: masks
    logits = m(xs.cuda(), xq.cuda()).view(-1, 3)
    loss = torch.nn.functional.cross_entropy(logits, label)
    loss.backward()
    torch.cuda.synchronize()
    par = numerics in ('parity', 'bf16x2')       # the two-limb mode (fp32 storage, three-digit-grade GEMMs) is held to the parity gates
    dl = np.abs(logits.detach().cpu().numpy() - z['logits']).max()
    print(f'[{numerics}] tiny train step: |dloss| = {abs(float(loss) - float(z["loss"])):.3e}, max|dlogit| = {dl:.3e}')
    assert dl <= (1e-3 if par else 0.3)
    assert abs(float(loss) - float(z['loss'])) <= (1e-4 if par else 0.05)
    n, worst = 0, 0.0
    for k in z.files:
        if k.startswith('grad.'):
            name = k[5:]
            g = dict(m.named_parameters())[name].grad.flatten().cpu()
            got = g[::max(1, g.numel() // 256)][:256].numpy()
            scale = float(z['gradnorm.' + name])
            # bf16: 24 images through a 5-block net, gradient noise is large; bf16x2: two-limb GEMMs (16 mantissa bits per operand), measured 1.4e-3
            tol = {'parity': 1e-3, 'bf16x2': 4e-3, 'bf16': 0.3}[numerics] * scale + (1e-6 if par else 1e-3)
            e = np.abs(got - z[k]).max()
            worst = max(worst, e / (scale + 1e-12)) if scale > 1e-6 else worst
            assert e <= tol, (name, e, scale)
            if scale > 1e-5:             # (analytically zero gradients hold rounding noise only)
                assert abs(float(g.norm()) - scale) <= tol, name
            n += 1
        elif k.startswith('bn.'):
            got = m.state_dict()[k[3:]].cpu().numpy()
            np.testing.assert_allclose(got, z[k], rtol=1e-3 if par else 5e-2, atol=1e-4 if par else 2e-2, err_msg=k)
    assert n == 60
    print(f'[{numerics}] tiny train step: worst sampled grad error / grad norm = {worst:.3e}')


@pytest.mark.parametrize('numerics,drop,freeze', [('parity', 0.0, False), ('parity', 0.5, False), ('bf16', 0.5, False), ('parity', 0.5, True), ('bf16', 0.0, True),
                                                  ('bf16x2', 0.5, False), ('bf16x2', 0.0, True)])
def test_micro_train_step_vs_oracle_autograd(numerics, drop, freeze):
    """visformer_micro_80, 2 episodes x (5-way 1-shot + 10 queries) = 30 images: every gradient vs torch.autograd of the oracle.
    freeze: utils.freeze_bn after model.train() (train_meta.py:156-157) - running statistics normalise and stay untouched."""
    from fewshot_vit_amd import synthetic
    from fewshot_vit_amd.utils import few_shot as fs
    from oracle import visformer_oracle as vo
    cfg = vo.VisformerCfg()
    shapes = vo.state_dict_shapes(cfg, prefix='encoder.')
    shapes['temp'] = ()
    sd = synthetic.synthetic_checkpoint_sd(shapes)
    x = synthetic.synthetic_episodes(5, 2, 5, 1, 2)
    xs, xq = fs.split_shot_query(x, 5, 1, 2, 2)
    n_img = 30
    label = torch.arange(5).repeat_interleave(2).repeat(2)
    rates = torch.linspace(0, drop, 9).tolist()
    masks = _cpu_masks(123, rates, 4, n_img)
    # oracle (CPU fp32 autograd)
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))}
    full = {k: v.clone() for k, v in sd.items()}
    full.update(params)
    stats = {}
    ref_logits = vo.meta_baseline_forward(full, xs, xq, cfg, mode='train', drop_path_rate=drop,
                                          droppath_masks=list(masks) if masks is not None else None, stats_out=stats, freeze_bn=freeze).view(-1, 5)
    ref_loss = torch.nn.functional.cross_entropy(ref_logits, label)
    ref_loss.backward()
    ref_grads = {k: p.grad.detach() for k, p in params.items()}
    # HIP
    m = _make(dict(img_size=80, init_channels=64, embed_dim=256, depth=[4, 2, 3], num_heads=6, mlp_ratio=4., group=8), sd, numerics, drop)
    if freeze:
        from fewshot_vit_amd import utils
        utils.freeze_bn(m)
    if masks is not None:
        mc = masks.cuda()
        m.encoder.draw_droppath_masks = lambda n, dev: mc
    n0 = int(m.encoder.norm.bn.num_batches_tracked)
    logits = m(xs.cuda(), xq.cuda()).view(-1, 5)
    loss = torch.nn.functional.cross_entropy(logits, label.cuda())
    loss.backward()
    torch.cuda.synchronize()
    par = numerics in ('parity', 'bf16x2')
    dl = float((logits.detach().cpu() - ref_logits.detach()).abs().max())
    grads = {k: p.grad for k, p in m.named_parameters()}
    assert set(grads) == set(ref_grads)
    # parity: max-pool argmax / LeakyReLU sign decisions flip at rounding-level ties (6M stem activations), so the stem's
    # gradients carry a few discrete differences: 5e-3 of the norm; every other layer is at the 1e-5 level (printed)
    # bf16 gates per layer group = 1.5 x the measured worst (round 3: stem 1.4e-1 - 30 images through batch-statistics BatchNorm, max-pool /
    # LeakyReLU decisions on bf16 activations - every other group 2.3e-2 ... 5.0e-2, the temperature 7.8e-3)
    bf16_gates = {'stem': 0.22, 'stage1': 0.075, 'patch_embed2': 0.07, 'stage2': 0.07, 'patch_embed3': 0.065, 'stage3': 0.07, 'pos_embed': 0.065,
                  'norm': 0.065, 'other': 0.012}
    worst = _grad_check(grads, ref_grads, 5e-3 if par else 0.22, numerics, 1e-5 if par else 2e-3, None if par else bf16_gates)
    print(f'[{numerics} drop={drop} freeze_bn={freeze}] micro train step: max|dlogit| = {dl:.3e}, |dloss| = {abs(float(loss) - float(ref_loss)):.3e}, '
          f'worst grad rel err = {worst:.3e}')
    assert dl <= (1e-3 if par else 0.3)
    if freeze:                           # nothing may have been updated
        assert not stats
        for k, v in m.state_dict().items():
            if k.endswith(('running_mean', 'running_var')):
                assert torch.equal(v.cpu(), sd[k]), k
        assert int(m.encoder.norm.bn.num_batches_tracked) == n0
        return
    for k, v in stats.items():          # updated running statistics
        got = m.state_dict()['encoder.' + k].cpu()
        torch.testing.assert_close(got, v, rtol=1e-3 if par else 5e-2, atol=1e-4 if par else 2e-2, msg=k)
    assert int(m.encoder.norm.bn.num_batches_tracked) == n0 + 1


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('S,hd,hdp', [(100, 42, 48), (25, 85, 96), (25, 21, 32)])
def test_attention_backward_vs_torch(dtype, S, hd, hdp):
    from fewshot_vit_amd.engine import ops
    if dtype == torch.bfloat16 and hdp % 32:
        hdp = (hdp + 31) // 32 * 32
    B, heads = 3, 6
    g = torch.Generator().manual_seed(S * hd)
    qkv = torch.zeros(B, S, 3, heads, hdp)
    qkv[..., :hd] = torch.randn(B, S, 3, heads, hd, generator=g)
    dctx = torch.zeros(B, S, heads, hdp)
    dctx[..., :hd] = torch.randn(B, S, heads, hd, generator=g)
    qkv_d = qkv.to(dtype).cuda()
    dctx_d = dctx.to(dtype).cuda()
    scale = hd ** -0.5
    out = ops.attention_backward(qkv_d.view(B * S, -1), dctx_d.view(B * S, -1), B, S, heads, hd, hdp, scale)
    torch.cuda.synchronize()
    ref_in = qkv_d.float().cpu().requires_grad_(True)
    q, k, v = ref_in[:, :, 0].transpose(1, 2), ref_in[:, :, 1].transpose(1, 2), ref_in[:, :, 2].transpose(1, 2)   # [B,heads,S,hdp]
    p = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1)
    ctx = (p @ v).transpose(1, 2)                                                                              # [B,S,heads,hdp]
    ctx.backward(dctx_d.float().cpu())
    err = float((out.float().cpu().view_as(ref_in) - ref_in.grad).abs().max())
    ref_max = float(ref_in.grad.abs().max())
    print(f'attention_backward {dtype} S={S} hd={hd}: max err {err:.3e} (max |grad| {ref_max:.2f})')
    assert err <= (2e-4 if dtype == torch.float32 else 2e-2) * max(1.0, ref_max)
    if hdp > hd:
        assert float(out.float().view(B, S, 3, heads, hdp)[..., hd:].abs().max()) == 0.0     # padded head dims stay exact zeros


@pytest.mark.parametrize('S,hd', [(197, 64), (197, 56), (150, 32)])
def test_attention_backward_fp32_long_sequences(S, hd):
    """fp32 (`parity`) attention backward past the all-in-LDS limit: K / V resident, query blocks of 16, dK / dV accumulated in the output."""
    test_attention_backward_vs_torch(torch.float32, S, hd, hd)


@pytest.mark.parametrize('S,hd', [(197, 64), (197, 32), (130, 64)])
def test_attention_backward_vit_token_counts(S, hd):
    """The ViT shapes (196 patches + cls, deit.py:37-58) on the LDS-resident MFMA kernel: its A operands come from the row-major images through
    transposing reads, so four matrices of 224 keys fit (the round-1 kernel kept three transposed copies and stopped at 128 keys)."""
    test_attention_backward_vs_torch(torch.bfloat16, S, hd, hd)


def test_proto_head_backward_vs_torch():
    from fewshot_vit_amd.engine import ops
    E, way, shot, Q, D = 3, 5, 5, 15, 512
    g = torch.Generator().manual_seed(9)
    fs_ = torch.randn(E, way, shot, D, generator=g)
    fq = torch.randn(E, Q, D, generator=g)
    dl = torch.randn(E, Q, way, generator=g)
    a, b = fs_.clone().requires_grad_(True), fq.clone().requires_grad_(True)
    t = torch.tensor(10.0, requires_grad=True)
    proto = torch.nn.functional.normalize(a.mean(dim=-2), dim=-1)
    logits = torch.bmm(torch.nn.functional.normalize(b, dim=-1), proto.transpose(1, 2)) * t
    logits.backward(dl)
    ds, dq, dt = ops.proto_head_backward(fs_.cuda(), fq.cuda(), dl.cuda(), 10.0)
    torch.cuda.synchronize()
    assert float((ds.cpu() - a.grad).abs().max()) <= 1e-5 * float(a.grad.abs().max()) + 1e-7
    assert float((dq.cpu() - b.grad).abs().max()) <= 1e-5 * float(b.grad.abs().max()) + 1e-7
    assert abs(float(dt) - float(t.grad)) <= 1e-4 * abs(float(t.grad)) + 1e-6


def test_proto_head_sqr_backward_vs_torch():
    """method 'sqr' (meta_baseline.py:38-41): logits = -temp * |q - mean_shot|^2, forward and backward vs torch."""
    from fewshot_vit_amd.engine import ops
    E, way, shot, Q, D = 3, 5, 5, 15, 512
    g = torch.Generator().manual_seed(19)
    fs_ = torch.randn(E, way, shot, D, generator=g) * 0.1
    fq = torch.randn(E, Q, D, generator=g) * 0.1
    dl = torch.randn(E, Q, way, generator=g)
    a, b = fs_.clone().requires_grad_(True), fq.clone().requires_grad_(True)
    t = torch.tensor(2.0, requires_grad=True)
    proto = a.mean(dim=-2)
    logits = -(b.unsqueeze(2) - proto.unsqueeze(1)).pow(2).sum(dim=-1) * t
    logits.backward(dl)
    got, _, _ = ops.proto_head(fs_.cuda(), fq.cuda(), 2.0, 'sqr')
    assert float((got.cpu() - logits.detach()).abs().max()) <= 1e-4
    ds, dq, dt = ops.proto_head_backward(fs_.cuda(), fq.cuda(), dl.cuda(), 2.0, 'sqr')
    torch.cuda.synchronize()
    assert float((ds.cpu() - a.grad).abs().max()) <= 1e-5 * float(a.grad.abs().max()) + 1e-7
    assert float((dq.cpu() - b.grad).abs().max()) <= 1e-5 * float(b.grad.abs().max()) + 1e-7
    assert abs(float(dt) - float(t.grad)) <= 1e-4 * abs(float(t.grad)) + 1e-6


@pytest.mark.parametrize('method', ['cos', 'sqr'])
@pytest.mark.parametrize('labels', ['nk', 'shuffled'])
def test_fused_head_cross_entropy_vs_torch(method, labels):
    """fsvit_proto_head_ce / _backward (train_meta.py:167-169 in one launch each way): loss = F.cross_entropy(logits, label), acc = compute_acc, the
    gradients of 3 x loss w.r.t. both feature tensors and the temperature vs torch autograd; temperature on the device; bit-reproducible; tickets left at 0."""
    from fewshot_vit_amd.autograd import ProtoHeadCEFn
    from fewshot_vit_amd.engine import ops
    from fewshot_vit_amd.utils import few_shot as fs
    from fewshot_vit_amd import utils
    E, way, shot, Q, D = 4, 10, 5, 50, 512
    g = torch.Generator().manual_seed(29)
    sc = 1.0 if method == 'cos' else 0.1
    fs_ = torch.randn(E, way, shot, D, generator=g) * sc
    fq = torch.randn(E, Q, D, generator=g) * sc
    fq[:, :, :64] += fs_.mean(2).repeat_interleave(Q // way, dim=1)[:, :, :64] * 3            # queries lean towards their class: accuracy well off chance
    label = fs.make_nk_label(way, Q // way, E)
    if labels == 'shuffled':
        label = label[torch.randperm(label.numel(), generator=g)]
    a, b = fs_.clone().requires_grad_(True), fq.clone().requires_grad_(True)
    t = torch.tensor(10.0 if method == 'cos' else 2.0, requires_grad=True)
    if method == 'cos':
        proto = torch.nn.functional.normalize(a.mean(dim=-2), dim=-1)
        logits = torch.bmm(torch.nn.functional.normalize(b, dim=-1), proto.transpose(1, 2)) * t
    else:
        logits = -(b.unsqueeze(2) - a.mean(dim=-2).unsqueeze(1)).pow(2).sum(dim=-1) * t
    loss = torch.nn.functional.cross_entropy(logits.view(-1, way), label)
    (3.0 * loss).backward()
    acc = utils.compute_acc(logits.view(-1, way), label)

    def run():
        a2, b2 = fs_.cuda().requires_grad_(True), fq.cuda().requires_grad_(True)
        t2 = t.detach().cuda().requires_grad_(True)
        l2, acc2, lg2 = ProtoHeadCEFn.apply(a2, b2, t2, label.cuda() if labels == 'shuffled' else None, method)
        (3.0 * l2).backward()
        torch.cuda.synchronize()
        return l2.detach().cpu(), acc2.cpu(), lg2.cpu(), a2.grad.cpu(), b2.grad.cpu(), t2.grad.cpu()
    l2, acc2, lg2, da, db, dt = run()
    assert not acc2.requires_grad and not lg2.requires_grad
    assert float((lg2 - logits.detach()).abs().max()) <= 1e-4
    assert abs(float(l2) - float(loss)) <= 2e-6 * max(1.0, abs(float(loss))), (float(l2), float(loss))
    assert abs(float(acc2) - acc) <= 1e-6, (float(acc2), acc)
    assert labels == 'shuffled' or 0.15 < acc < 1.0            # (shuffled labels: chance level - the label tensor is what is being tested)
    assert float((da - a.grad).abs().max()) <= 1e-5 * float(a.grad.abs().max()) + 1e-8
    assert float((db - b.grad).abs().max()) <= 1e-5 * float(b.grad.abs().max()) + 1e-8
    assert abs(float(dt) - float(t.grad)) <= 1e-4 * abs(float(t.grad)) + 1e-7
    again = run()
    for x, y in zip((l2, acc2, lg2, da, db, dt), again):
        assert torch.equal(x, y)
    assert int(ops._ticket(torch.device('cuda', torch.cuda.current_device())).abs().sum()) == 0


def test_fused_head_flags_labels_outside_the_way_range_and_keeps_a_ticket_per_stream():
    """a label outside [0, way) - F.cross_entropy's ignore_index included - makes the fused head's loss NaN (the ATen path raises; a silent
    `logsumexp - 0` would train on garbage); two streams get two ticket pairs."""
    from fewshot_vit_amd.engine import ops
    E, way, shot, Q, D = 2, 5, 1, 10, 64
    g = torch.Generator().manual_seed(3)
    fs_, fq = torch.randn(E, way, shot, D, generator=g).cuda(), torch.randn(E, Q, D, generator=g).cuda()
    good = torch.arange(way).repeat_interleave(Q // way).repeat(E).cuda()
    _, _, st = ops.proto_head_ce(fs_, fq, 10.0, good)
    assert torch.isfinite(st).all()
    for bad_value in (-100, way):
        bad = good.clone()
        bad[Q + 3] = bad_value                                   # one query of the second episode
        _, _, st = ops.proto_head_ce(fs_, fq, 10.0, bad)
        torch.cuda.synchronize()
        assert torch.isnan(st[0]) and torch.isnan(st[2 + E + 1]) and torch.isfinite(st[2 + E + 0])      # batch loss, episode 1's loss; episode 0 untouched
    dev = torch.device('cuda', torch.cuda.current_device())
    t0 = ops._ticket(dev)
    with torch.cuda.stream(torch.cuda.Stream()):
        t1 = ops._ticket(dev)
        _, _, st = ops.proto_head_ce(fs_, fq, 10.0, good)
        torch.cuda.current_stream().synchronize()
        assert torch.isfinite(st).all()
    assert t0.data_ptr() != t1.data_ptr() and int(t0.abs().sum()) == 0 and int(t1.abs().sum()) == 0


def test_train_step_fused_head_equals_the_three_reference_lines():
    """train_meta.train_step through model.forward_loss (fused head + CE + accuracy) vs logits -> F.cross_entropy / compute_acc through ATen: same loss,
    accuracy and parameters after one parity-mode step."""
    import copy
    from fewshot_vit_amd import models, synthetic, train_meta, utils
    from fewshot_vit_amd.utils import few_shot as fs
    m0 = models.make('meta-baseline', encoder='visformer_micro_80', encoder_args={'drop_path_rate': 0.0, 'numerics': 'parity'})
    shapes = {k: tuple(v.shape) for k, v in m0.state_dict().items()}
    m0.load_state_dict(synthetic.synthetic_checkpoint_sd(shapes))
    E, way, shot, query = 2, 5, 1, 3
    x = synthetic.synthetic_episodes(3, E, way, shot, query).cuda()
    x_shot, x_query = fs.split_shot_query(x, way, shot, query, E)
    label = fs.make_nk_label(way, query, E).cuda()
    outs = []
    for fused in (True, False):
        m = copy.deepcopy(m0).cuda().train()
        opt, _ = utils.make_optimizer(m.parameters(), 'sgd', lr=0.01, weight_decay=5e-4)
        train_meta._FUSED_CE = fused
        try:
            loss, acc = train_meta.train_step(m, opt, x_shot, x_query, label, way)
        finally:
            train_meta._FUSED_CE = True
        outs.append((loss, acc, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}))
    (l0, a0, s0), (l1, a1, s1) = outs
    assert abs(l0 - l1) <= 2e-6 * max(1.0, abs(l1)) and abs(a0 - a1) <= 1e-6
    for k in s0:
        if s0[k].dtype.is_floating_point:
            assert float((s0[k] - s1[k]).abs().max()) <= 2e-6 * max(1e-3, float(s1[k].abs().max())), k


def test_sgd_step_matches_torch_optim():
    """torch.optim.SGD(momentum=0.9, weight_decay) semantics of utils.make_optimizer (utils/__init__.py:128-132)."""
    from fewshot_vit_amd.engine import ops
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(10007, generator=g)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.SGD([ref], lr=0.01, momentum=0.9, weight_decay=5e-4)
    p, buf = p0.clone().cuda(), torch.zeros(10007).cuda()
    for step in range(3):
        gr = torch.randn(10007, generator=g)
        ref.grad = gr.clone()
        opt.step()
        ops.sgd_step(p, gr.cuda(), buf, 0.01, 0.9, 5e-4, step == 0)
    torch.cuda.synchronize()
    assert float((p.cpu() - ref.detach()).abs().max()) <= 1e-6


def test_fsvit_sgd_multi_tensor_matches_torch_optim():
    """utils.FsvitSGD (one table-driven launch per param_group, fsvit_sgd_step_multi) vs torch.optim.SGD over ragged tensors, three steps,
    a tensor without gradient and one whose first gradient arrives late (its momentum buffer starts at that step)."""
    from fewshot_vit_amd import utils
    g = torch.Generator().manual_seed(5)
    shapes = [(33,), (128, 32, 3, 3), (1,), (1000, 7), (256,), (5, 5)]
    init = [torch.randn(*sh, generator=g) for sh in shapes]
    ref = [t.clone().requires_grad_(True) for t in init]
    mine = [t.clone().cuda().requires_grad_(True) for t in init]
    o_ref = torch.optim.SGD(ref, lr=0.02, momentum=0.9, weight_decay=5e-4)
    o_mine = utils.FsvitSGD(mine, lr=0.02, momentum=0.9, weight_decay=5e-4)
    for step in range(3):
        for k, (r, m) in enumerate(zip(ref, mine)):
            if k == 2 or (k == 4 and step == 0):
                r.grad = None; m.grad = None
                continue
            gr = torch.randn(*shapes[k], generator=g)
            r.grad = gr.clone(); m.grad = gr.cuda()
        o_ref.step(); o_mine.step()
    torch.cuda.synchronize()
    for r, m in zip(ref, mine):
        assert float((m.detach().cpu() - r.detach()).abs().max()) <= 1e-6


def test_training_loop_reduces_loss_and_eval_follows():
    """train_meta.py:155-177 shape: model.train(); loss.backward(); optimizer.step() repeated on one batch of episodes
    drives the loss down; the eval engine then repacks from the updated weights."""
    from fewshot_vit_amd import models, synthetic, utils
    from fewshot_vit_amd.utils import few_shot as fs
    m = models.make('meta-baseline', encoder='visformer_micro_80', encoder_args={'drop_path_rate': 0.1, 'numerics': 'bf16'}).cuda()
    opt, _ = utils.make_optimizer(m.parameters(), 'sgd', lr=0.01, weight_decay=5e-4)
    x = synthetic.synthetic_episodes(3, 2, 5, 1, 3).cuda()
    xs, xq = fs.split_shot_query(x, 5, 1, 3, 2)
    label = fs.make_nk_label(5, 3, 2).cuda()
    losses = []
    m.train()
    for it in range(6):
        logits = m(xs, xq).view(-1, 5)
        loss = torch.nn.functional.cross_entropy(logits, label)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print('losses', ['%.4f' % v for v in losses])
    assert all(np.isfinite(losses))
    assert losses[-1] < losses[0]
    m.eval()
    with torch.no_grad():
        lg = m(xs, xq)
    assert torch.isfinite(lg).all()


def test_eval_engine_follows_raw_pointer_weight_updates():
    """the HIP optimizer / trainer write through raw device pointers, which never bump torch's `_version`.  Sequence
    forward, eval, backward, step, eval (no train-mode forward between the two evals): the second eval must use freshly packed
    weights - compared with an engine built from a cloned state dict - and must differ from the first."""
    from fewshot_vit_amd import models, synthetic, utils
    from fewshot_vit_amd.engine import VisformerEngine
    from fewshot_vit_amd.utils import few_shot as fs
    m = models.make('meta-baseline', encoder='visformer_micro_80', encoder_args={'numerics': 'bf16'}).cuda()
    opt, _ = utils.make_optimizer(m.parameters(), 'sgd', lr=0.05, weight_decay=5e-4)
    x = synthetic.synthetic_episodes(5, 1, 5, 1, 3).cuda()
    xs, xq = fs.split_shot_query(x, 5, 1, 3, 1)
    label = fs.make_nk_label(5, 3, 1).cuda()
    m.train()
    loss = torch.nn.functional.cross_entropy(m(xs, xq).view(-1, 5), label)
    m.eval()
    with torch.no_grad():
        f0 = m.encoder(x).clone()
    opt.zero_grad()
    loss.backward()
    opt.step()                                   # raw-pointer update, no train-mode forward afterwards
    with torch.no_grad():
        f1 = m.encoder(x).clone()
    fresh = VisformerEngine(m.encoder.cfg, {k: v.detach().clone() for k, v in m.encoder.state_dict().items()}, numerics='bf16')
    f2 = fresh.forward(x)
    torch.cuda.synchronize()
    assert not torch.equal(f0, f1)
    assert torch.equal(f1, f2)


def test_second_forward_before_backward_raises():
    """one set of saved activations per trainer - a second train-mode forward invalidates the first graph loudly."""
    from fewshot_vit_amd import models, synthetic
    m = models.make('visformer_micro_80', numerics='parity').cuda().train()
    xa, xb = synthetic.synthetic_episodes(1, 1, 2, 1, 1).cuda(), synthetic.synthetic_episodes(2, 1, 2, 1, 1).cuda()
    fa = m(xa)
    fb = m(xb)
    with pytest.raises(RuntimeError, match='another train-mode forward'):
        fa.sum().backward()
    fb.sum().backward()                          # the latest forward is still valid
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    one = m(xa[:1])                              # B = 1: 25 values per channel at the last BatchNorm, valid in torch too
    assert one.shape == (1, 512) and torch.isfinite(one).all()


def test_train_meta_driver_one_epoch(tmp_path):
    """The train_meta.py surface end to end on a small schedule: train batches, tval/val episodes in eval mode, the
    reference's checkpoint schema (train_meta.py:241-257) readable by models.load, MultiStepLR stepping."""
    from fewshot_vit_amd import models, train_meta
    config = dict(train_dataset='synthetic-episodes', train_dataset_args=dict(split='train', n_classes=12, n_per_class=30, noise=1.0, seed=1),
                  tval_dataset='synthetic-episodes', tval_dataset_args=dict(split='test', n_classes=6, n_per_class=30, noise=1.0, seed=0),
                  val_dataset='synthetic-episodes', val_dataset_args=dict(split='val', n_classes=6, n_per_class=30, noise=1.0, seed=2),
                  model='meta-baseline', model_args=dict(encoder='visformer_micro_80', encoder_args=dict(drop_path_rate=0.5)),
                  synthetic_checkpoint='visformer_micro_80', n_train_way=5, n_train_shot=1, n_train_query=3, n_way=5, n_shot=1, n_query=15,
                  train_batches=3, eval_batches=2, ep_per_batch=2, max_epoch=2, optimizer='sgd',
                  optimizer_args=dict(lr=0.001, weight_decay=5e-4, gamma=0.5, milestones=[1]), save_epoch=1)
    lines = []
    trlog = train_meta.main(config, name='t', device=torch.device('cuda', 0), log=lines.append, save_root=str(tmp_path))
    assert len(trlog['tl']) == 2 and all(np.isfinite(trlog[k]).all() for k in trlog)
    assert any(l.startswith('epoch 2, train') for l in lines)
    for f in ('epoch-last.pth', 'epoch-1.pth', 'epoch-2.pth', 'max-va.pth', 'trlog.pth', 'config.yaml'):
        assert os.path.exists(os.path.join(str(tmp_path), 't', f)), f
    ck = torch.load(os.path.join(str(tmp_path), 't', 'epoch-last.pth'), map_location='cpu')
    assert ck['training']['epoch'] == 2 and ck['model'] == 'meta-baseline'
    assert ck['training']['optimizer_sd']['param_groups'][0]['lr'] == pytest.approx(0.0005)      # one milestone passed
    m = models.load(ck)
    assert m.encoder.out_dim == 512


def test_train_meta_warmup_driver(tmp_path):
    """train_meta_warmup.py surface: SGD + MultiStepLRScheduler(warmup_t=3, warmup_lr_init=1e-5, decay_rate=0.5) stepped with
    (epoch - 1): after epoch 3 the groups sit at _get_lr(2) = 1e-5 + 2/3 (lr - 1e-5)."""
    from fewshot_vit_amd import train_meta_warmup
    config = dict(train_dataset='synthetic-episodes', train_dataset_args=dict(split='train', n_classes=12, n_per_class=30, noise=1.0, seed=1),
                  val_dataset='synthetic-episodes', val_dataset_args=dict(split='val', n_classes=6, n_per_class=30, noise=1.0, seed=2),
                  model='meta-baseline', model_args=dict(encoder='visformer_micro_80', encoder_args=dict(drop_path_rate=0.5)),
                  synthetic_checkpoint='visformer_micro_80', n_train_way=5, n_train_shot=1, n_train_query=3, n_way=5, n_shot=1, n_query=15,
                  train_batches=2, eval_batches=1, ep_per_batch=2, max_epoch=3, optimizer='sgd',
                  optimizer_args=dict(lr=0.001, weight_decay=5e-4, milestones=[20, 40]))
    lines = []
    trlog = train_meta_warmup.main(config, name='w', device=torch.device('cuda', 0), log=lines.append, save_root=str(tmp_path))
    assert len(trlog['tl']) == 3 and all(np.isfinite(trlog[k]).all() for k in ('tl', 'ta', 'vl', 'va'))
    ck = torch.load(os.path.join(str(tmp_path), 'w', 'epoch-last.pth'), map_location='cpu')
    assert ck['training']['optimizer_sd']['param_groups'][0]['lr'] == pytest.approx(1e-5 + 2 * (1e-3 - 1e-5) / 3)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(3, 20, 20, 256, 32, 8), (2, 40, 40, 128, 64, 1), (2, 40, 40, 128, 128, 1), (5, 20, 20, 256, 32, 8), (1, 12, 16, 128, 64, 1)])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_conv3x3_wgrad_direct_vs_torch(shape, dtype):
    """fsvit_conv3x3_wgrad (transposing LDS reads, taps as addresses) vs torch's conv2d weight gradient on the same 16-bit-rounded operands
    (fp32 accumulation on both sides: only the summation order differs)."""
    from fewshot_vit_amd.engine import ops
    B, H, W, O, Ig, groups = shape
    g = torch.Generator().manual_seed(17 + B + O + Ig)
    x = torch.randn(B, groups * Ig, H, W, generator=g).to(dtype).float()
    dz = (torch.randn(B, O, H, W, generator=g) * 0.1).to(dtype).float()
    wref = torch.zeros(O, Ig, 3, 3, requires_grad=True)
    F.conv2d(x, wref, padding=1, groups=groups).backward(dz)
    got = ops.conv3x3_wgrad(x.permute(0, 2, 3, 1).contiguous().to('cuda', dtype), dz.permute(0, 2, 3, 1).contiguous().to('cuda', dtype), O, Ig, groups).cpu()
    ref = wref.grad
    err = (got - ref).abs().max().item()
    print(f'conv3x3_wgrad {shape} {dtype}: max err {err:.3e} (max |dW| {ref.abs().max():.2f})')
    assert err <= 2e-4 * max(1.0, ref.abs().max().item())
    # border structure: the tap that reads outside the image must contribute nothing (a wrong mask shows up on the corner taps first)
    assert (got[:, :, 0, 0] - ref[:, :, 0, 0]).abs().max().item() <= 2e-4 * max(1.0, ref.abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(3, 20, 20, 256, 32, 8), (2, 40, 40, 128, 64, 1), (2, 40, 40, 128, 128, 1), (5, 20, 20, 256, 32, 8), (1, 12, 16, 128, 64, 1), (2, 7, 9, 256, 32, 8)])
@pytest.mark.parametrize('limbs', ['bf16', 'f16'])
def test_conv3x3_wgrad_two_limb_vs_fp64(shape, limbs):
    """fsvit_conv3x3_wgrad on fp32 activations (FSVIT_BF16X2 / FSVIT_F16X2: limb rows at LDS staging, a tap = two rows per pixel) vs torch's conv2d
    weight gradient in fp64 on the unrounded operands; border taps included."""
    from fewshot_vit_amd.engine import ops
    B, H, W, O, Ig, groups = shape
    g = torch.Generator().manual_seed(19 + B + O + Ig + H)
    x = torch.randn(B, groups * Ig, H, W, generator=g)
    dz = torch.randn(B, O, H, W, generator=g) * 0.1
    wref = torch.zeros(O, Ig, 3, 3, requires_grad=True, dtype=torch.float64)
    F.conv2d(x.double(), wref, padding=1, groups=groups).backward(dz.double())
    wabs = torch.zeros(O, Ig, 3, 3, requires_grad=True, dtype=torch.float64)
    F.conv2d(x.double().abs(), wabs, padding=1, groups=groups).backward(dz.double().abs())
    scale = wabs.grad.max().item()                                                        # sum of |products|
    args = (x.permute(0, 2, 3, 1).contiguous().cuda(), dz.permute(0, 2, 3, 1).contiguous().cuda(), O, Ig, groups, limbs)
    got = ops.conv3x3_wgrad(*args).cpu().double()
    err = (got - wref.grad).abs().max().item()
    print(f'conv3x3_wgrad two-limb {shape} {limbs}: max err {err:.3e} (sum |products| {scale:.1f})')
    assert err <= (3e-5 if limbs == 'bf16' else 2e-6) * scale
    assert (got[:, :, 0, 0] - wref.grad[:, :, 0, 0]).abs().max().item() <= (3e-5 if limbs == 'bf16' else 2e-6) * scale
    assert torch.equal(got, ops.conv3x3_wgrad(*args).cpu().double())


def _wgrad1x1_splits(M, N, C):
    """Row splits (= partial slabs the finalize sums) of the 16-bit 1x1 weight-gradient launch: wgrad1x1_splits in csrc/wgrad3x3.hip at its default of
    128 workgroups - 64-row chunks, blocks of 256 along a dimension of >= 256 columns, else 128."""
    chunks = -(-M // 64)
    tiles = -(-N // (256 if N >= 256 else 128)) * -(-C // (256 if C >= 256 else 128))
    s = max(1, min(-(-128 // tiles), chunks))
    cpw = -(-chunks // s)
    return -(-chunks // cpw)


# (64, 8, 8): ONE split - the finalize's sum is a copy; (390, 8, 8): 7 splits - its four-slab loop runs once and the tail loop three times;
# (130, 8, 256): the 128 x 256 block (N < 256 <= C, e.g. the stage-1 conv3 gradient) - every other shape with C >= 256 has N >= 256 as well
@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(8000, 1024, 256), (2000, 864, 256), (2000, 512, 576), (5000, 128, 32), (777, 256, 128), (64, 1728, 512), (130, 8, 8),
                                   (64, 8, 8), (390, 8, 8), (130, 8, 256)])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_conv1x1_wgrad_direct_vs_torch(shape, dtype):
    """fsvit_conv1x1_wgrad vs dz^T @ x in fp32 on the same 16-bit-rounded operands (ragged M, N, C tails included).  The operator sums its split
    slabs with a one-job launch of the training step's finalize kernel."""
    from fewshot_vit_amd.engine import ops
    M, N, C = shape
    splits = _wgrad1x1_splits(M, N, C)
    print(f'conv1x1_wgrad {shape}: {splits} splits')
    if shape == (64, 8, 8):
        assert splits == 1
    if shape == (390, 8, 8):
        assert splits == 7          # > 4 and not a multiple of 4: main loop and tail loop
    g = torch.Generator().manual_seed(M + N + C)
    x = torch.randn(M, C, generator=g).to(dtype)
    dz = (torch.randn(M, N, generator=g) * 0.1).to(dtype)
    ref = dz.double().t() @ x.double()
    got = ops.conv1x1_wgrad(x.cuda(), dz.cuda()).cpu().double()
    err = (got - ref).abs().max().item()
    print(f'conv1x1_wgrad {shape} {dtype}: max err {err:.3e} (max |dW| {ref.abs().max():.2f})')
    assert err <= 2e-4 * max(1.0, ref.abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(8000, 1024, 256), (2000, 864, 256), (2000, 512, 576), (5000, 128, 32), (777, 256, 128), (64, 1728, 512), (130, 8, 8),
                                   (130, 8, 256)])
@pytest.mark.parametrize('limbs', ['bf16', 'f16'])
def test_conv1x1_wgrad_two_limb_vs_fp64(shape, limbs):
    """fsvit_conv1x1_wgrad on fp32 rows (FSVIT_BF16X2 / FSVIT_F16X2: the limb split at LDS staging, two MFMAs per 16 values) vs dz^T @ x in fp64 on
    the UNROUNDED fp32 operands: the two-limb product carries 16 (bf16 limbs) / 22 (f16 limbs) significand bits."""
    from fewshot_vit_amd.engine import ops
    M, N, C = shape
    g = torch.Generator().manual_seed(M + N + C + 1)
    x = torch.randn(M, C, generator=g)
    dz = torch.randn(M, N, generator=g) * 0.1
    ref = dz.double().t() @ x.double()
    got = ops.conv1x1_wgrad(x.cuda(), dz.cuda(), limbs).cpu().double()
    err = (got - ref).abs().max().item()
    scale = (dz.double().abs().t() @ x.double().abs()).max().item()            # sum of |products|: what a relative operand error multiplies
    print(f'conv1x1_wgrad two-limb {shape} {limbs}: max err {err:.3e} (sum |products| {scale:.1f})')
    assert err <= (3e-5 if limbs == 'bf16' else 2e-6) * scale
    assert torch.equal(got, ops.conv1x1_wgrad(x.cuda(), dz.cuda(), limbs).cpu().double())


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(3, 20, 20), (1, 12, 16), (7, 20, 20), (2, 5, 7)])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_gconv3x3_vs_torch(shape, dtype):
    """fsvit_gconv3x3 (wave = group, register-resident weights, taps as addresses into the staged pixel window) vs torch's grouped conv2d on
    the same 16-bit-rounded operands: forward, and the data gradient as the trainer computes it - the same kernel on the transposed, tap-flipped
    weights - vs torch's conv_transpose (image borders, ragged last chunk, several images per 64-pixel chunk)."""
    from fewshot_vit_amd.engine import ops
    B, H, W = shape
    g = torch.Generator().manual_seed(B * 100 + H)
    x = torch.randn(B, 256, H, W, generator=g).to(dtype).float()
    w = (torch.randn(256, 32, 3, 3, generator=g) / 17.0).to(dtype).float()

    def pack(wt):                         # [256][32][3][3] -> [256][320], columns (ky, kx, c)
        p = torch.zeros(256, 320)
        p[:, :288] = wt.permute(0, 2, 3, 1).reshape(256, 288)
        return p.to(dtype).cuda()
    xd = x.permute(0, 2, 3, 1).contiguous().to('cuda', dtype)
    ref = F.conv2d(x, w, padding=1, groups=8)
    got = ops.gconv3x3(xd, pack(w)).float().cpu().permute(0, 3, 1, 2)
    err = (got - ref).abs().max().item()
    # data gradient: dx = conv(dz, W^T flipped) per group
    wt = w.reshape(8, 32, 32, 3, 3).transpose(1, 2).flip(-1, -2).reshape(256, 32, 3, 3)
    ref_t = F.conv_transpose2d(x, w, padding=1, groups=8)
    got_t = ops.gconv3x3(xd, pack(wt)).float().cpu().permute(0, 3, 1, 2)
    err_t = (got_t - ref_t).abs().max().item()
    print(f'gconv3x3 {shape} {dtype}: forward {err:.3e}, data gradient {err_t:.3e} (max |y| {ref.abs().max():.2f})')
    tol = 1.2e-2 * max(1.0, ref.abs().max().item())       # the 16-bit rounding of the output
    assert err <= tol and err_t <= tol


# ------------------------------------------------------------------------------------------------ BASELINE configs[2] at its own size
def _full_size_batch(E=8, way=10, shot=5, query=5, seed=31):
    from fewshot_vit_amd import synthetic
    from fewshot_vit_amd.utils import few_shot as fs
    x = synthetic.synthetic_episodes(seed, E, way, shot, query)
    xs, xq = fs.split_shot_query(x, way, shot, query, E)
    return xs.cuda(), xq.cuda(), fs.make_nk_label(way, query, E).cuda()


@pytest.mark.parametrize('numerics', ['parity', 'bf16', 'bf16x2'])
def test_full_size_800_image_step_equals_mean_of_single_episode_steps(numerics):
    """The SUN-M step at the size train_meta_mini_visformer_5shot.yaml runs it (8 episodes x 10-way x (5 + 5) = 800 images, drop_path 0.5):
    with frozen BatchNorm (train_meta.py:156-157) and fixed DropPath masks every image is independent, so the gradient of the 8-episode
    step must equal the mean of the eight single-episode gradients - the full-size launch (split-slab weight gradients over 800 x 1600 rows,
    the 800-image arenas, wgrad3x3 at full batch) against eight 100-image launches of the same kernels.  fp32 summation order is the only
    difference in `parity`; in `bf16` the loss scale differs by 8 = 2^3, which is exact in bf16, so the same bound holds (`bf16x2`: the limb
    split of an operand commutes with a power-of-two scale as well)."""
    from fewshot_vit_amd import models, synthetic, utils
    E, way, shot, query = 8, 10, 5, 5
    m = models.make('meta-baseline', encoder='visformer_micro_80', encoder_args={'numerics': numerics, 'drop_path_rate': 0.5})
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict(synthetic.synthetic_checkpoint_sd(shapes), strict=True)
    m = m.cuda().train()
    utils.freeze_bn(m)
    xs, xq, label = _full_size_batch(E, way, shot, query)
    n_shot = E * way * shot
    g = torch.Generator().manual_seed(7)
    n_calls = m.encoder.trainer().n_droppath_calls(0.5)
    rates = [r for b, r in enumerate(torch.linspace(0, 0.5, 9).tolist()) for _ in range(1 if b < 4 else 2) if r > 0]
    assert len(rates) == n_calls
    masks = torch.stack([(1.0 - r + torch.rand(2 * n_shot, generator=g)).floor() for r in rates]).cuda()

    def run(xs_, xq_, label_, mk):
        m.encoder.draw_droppath_masks = lambda n, dev: mk
        m.zero_grad(set_to_none=True)
        logits = m(xs_, xq_).view(-1, way)
        loss = F.cross_entropy(logits, label_)
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
    print(f'[{numerics}] 800-image step vs mean of 8 single-episode steps: worst gradient rel err {worst:.2e} ({worst_k}), loss {loss_full:.5f}')
    assert worst <= 2e-5, (worst, worst_k)


def test_full_size_800_image_step_live_batchnorm():
    """The same 800-image step with live BatchNorm (batch statistics over all 800 x 1600 stem rows): everything finite, and the first
    BatchNorm's running statistics after the step equal momentum-0.1 updates from torch's own statistics of conv1(x) over the batch."""
    from fewshot_vit_amd import models, synthetic
    E, way = 8, 10
    m = models.make('meta-baseline', encoder='visformer_micro_80', encoder_args={'numerics': 'bf16', 'drop_path_rate': 0.5})
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = synthetic.synthetic_checkpoint_sd(shapes)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    xs, xq, label = _full_size_batch()
    logits = m(xs, xq).view(-1, way)
    loss = F.cross_entropy(logits, label)
    loss.backward()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and torch.isfinite(logits).all()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    x = torch.cat([xs.reshape(-1, 3, 80, 80), xq.reshape(-1, 3, 80, 80)])
    z = F.conv2d(x.double(), sd['encoder.stem.conv1.weight'].cuda().double(), stride=2, padding=1)
    mean, var = z.mean(dim=(0, 2, 3)), z.var(dim=(0, 2, 3), unbiased=True)
    rm = 0.9 * sd['encoder.stem.bn1.running_mean'].cuda().double() + 0.1 * mean
    rv = 0.9 * sd['encoder.stem.bn1.running_var'].cuda().double() + 0.1 * var
    torch.testing.assert_close(m.encoder.stem.bn1.running_mean.double(), rm, rtol=2e-2, atol=2e-3)      # bf16 operands of conv1
    torch.testing.assert_close(m.encoder.stem.bn1.running_var.double(), rv, rtol=2e-2, atol=2e-3)
    for k, v in m.state_dict().items():
        if k.endswith(('running_mean', 'running_var')):
            assert torch.isfinite(v).all() and not torch.equal(v.cpu(), sd[k]), k


def test_frozen_teacher_keeps_its_engine_while_a_student_trains():
    """raw-pointer writes invalidate the packed engines of the tensors they touch only - a student's train-mode forward and
    optimizer step must not make a frozen teacher re-pack (offline.py runs both every iteration)."""
    from fewshot_vit_amd import models, synthetic, utils
    from fewshot_vit_amd.utils import few_shot as fs
    teacher = models.make('visformer_micro_80', numerics='bf16').cuda().eval()
    student = models.make('meta-baseline', encoder='visformer_micro_80', encoder_args={'numerics': 'bf16'}).cuda().train()
    opt, _ = utils.make_optimizer(student.parameters(), 'sgd', lr=0.01, weight_decay=5e-4)
    x = synthetic.synthetic_episodes(5, 1, 5, 1, 3).cuda()
    xs, xq = fs.split_shot_query(x, 5, 1, 3, 1)
    label = fs.make_nk_label(5, 3, 1).cuda()
    with torch.no_grad():
        teacher(x)
    eng = teacher.engine()
    for _ in range(2):
        loss = F.cross_entropy(student(xs, xq).view(-1, 5), label)
        opt.zero_grad()
        loss.backward()
        opt.step()
        with torch.no_grad():
            teacher(x)
        assert teacher.engine() is eng
    s_eng = student.encoder.engine()
    loss = F.cross_entropy(student(xs, xq).view(-1, 5), label)           # running statistics written through raw pointers
    assert student.encoder.engine() is not s_eng


def _tune_and_eval(numerics, steps, lr, eval_numerics='parity'):
    """Meta-tune `steps` SUN-M steps (8 episodes x 10-way x (5 + 5), drop_path 0.5, train_meta.py:161-177) on a seeded synthetic stream, then
    evaluate on 500 held-out 5-way 5-shot episodes.  Seeds fix the episode stream, the DropPath draws and the data, so two numerics modes see
    the same training run up to their own rounding."""
    from fewshot_vit_amd import datasets, models, synthetic, utils
    from fewshot_vit_amd.datasets.samplers import CategoriesSampler
    from fewshot_vit_amd.utils import few_shot as fs
    m = models.make('meta-baseline', encoder='visformer_micro_80', encoder_args={'numerics': numerics, 'drop_path_rate': 0.5})
    m.load_state_dict(synthetic.synthetic_checkpoint_sd({k: tuple(v.shape) for k, v in m.state_dict().items()}), strict=True)
    m = m.cuda()
    train = datasets.make('synthetic-episodes', split='train', n_classes=40, n_per_class=20, noise=1.0, seed=1)
    test = datasets.make('synthetic-episodes', split='test', n_classes=20, n_per_class=40, noise=1.0, seed=0)
    opt, _ = utils.make_optimizer(m.parameters(), 'sgd', lr=lr, weight_decay=5e-4)
    E, way, shot, query = 8, 10, 5, 5
    label = fs.make_nk_label(way, query, E).cuda()
    torch.manual_seed(4321)
    torch.cuda.manual_seed_all(4321)
    np.random.seed(4321)
    m.train()
    losses = []
    for idx in CategoriesSampler(train.label, steps, way, shot + query, ep_per_batch=E):
        xs, xq = fs.split_shot_query(train.gather(idx), way, shot, query, ep_per_batch=E)
        loss = F.cross_entropy(m(xs, xq).view(-1, way), label)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu()
    assert torch.isfinite(losses).all()
    m.eval()
    m.encoder.numerics = eval_numerics               # both tuned models are scored by the same (exact-fp32) evaluator
    m.encoder._engine = None
    np.random.seed(99)
    accs = []
    lab = fs.make_nk_label(5, 15, 1).cuda()
    with torch.no_grad():
        batch = []
        for idx in CategoriesSampler(test.label, 500, 5, 5 + 15, ep_per_batch=1):
            batch.append(idx)
            if len(batch) == 50:
                xs, xq = fs.split_shot_query(test.gather(torch.cat(batch)), 5, 5, 15, ep_per_batch=50)
                lg = m(xs, xq)
                accs.append((lg.argmax(-1) == lab.view(1, -1)).float().mean(dim=1))
                batch = []
    accs = torch.cat(accs).double().cpu()
    ci = 1.96 * float(accs.std(unbiased=True)) / len(accs) ** 0.5
    return float(accs.mean()), ci, float(losses[:10].mean()), float(losses[-10:].mean())


def test_two_limb_meta_tuning_follows_the_parity_trajectory():
    """VERDICT r02 'missing' #2: a 1e-3-grade training mode at MFMA-class speed.  `bf16x2` (fp32 storage; every forward, data-gradient and
    weight-gradient GEMM as two-limb bf16 MFMAs on limb words packed on the device each step) against `parity` (exact-fp32 MFMA) on the same
    seeded 12-step SUN-M run at the configs[2] geometry: the loss trajectories must agree to 2e-3 (bf16 drifts by 1e-2 ... 1e-1 over the same
    steps), and the tuned models score the same held-out accuracy to 0.5 %."""
    steps, lr = 12, 0.01
    acc_x, ci_x, l0_x, l1_x = _tune_and_eval('bf16x2', steps, lr)
    acc_p, ci_p, l0_p, l1_p = _tune_and_eval('parity', steps, lr)
    print(f'meta-tuned {steps} steps (lr {lr}): bf16x2 acc {100 * acc_x:.2f} %, loss {l0_x:.5f} -> {l1_x:.5f}; parity acc {100 * acc_p:.2f} %, '
          f'loss {l0_p:.5f} -> {l1_p:.5f}')
    assert abs(l0_x - l0_p) <= 2e-3 and abs(l1_x - l1_p) <= 2e-3
    assert abs(acc_x - acc_p) <= 0.005


def test_bf16_meta_tuning_reaches_the_parity_tuned_accuracy():
    """the bf16 trainer must earn its place - 100 SUN-M steps at the configs[2] geometry (800 images per step) on the same seeded
    stream in `bf16` and in `parity` (exact fp32), both scored on the same 500 held-out episodes by the exact-fp32 evaluator: the accuracies
    must agree within the evaluation's own 95 % CI, and tuning must have moved the model (the loss falls) so the comparison is not vacuous."""
    steps, lr = 100, 0.01
    acc_b, ci_b, l0_b, l1_b = _tune_and_eval('bf16', steps, lr)
    acc_p, ci_p, l0_p, l1_p = _tune_and_eval('parity', steps, lr)
    print(f'meta-tuned {steps} steps (lr {lr}): bf16 acc {100 * acc_b:.2f} +- {100 * ci_b:.2f} %, loss {l0_b:.4f} -> {l1_b:.4f}; '
          f'parity acc {100 * acc_p:.2f} +- {100 * ci_p:.2f} %, loss {l0_p:.4f} -> {l1_p:.4f}; |delta acc| = {100 * abs(acc_b - acc_p):.2f} %')
    assert l1_b < l0_b and l1_p < l0_p
    assert abs(l1_b - l1_p) <= 0.05 * max(l1_p, 1e-3) + 0.02
    assert abs(acc_b - acc_p) <= max(ci_b, ci_p)


@pytest.mark.parametrize('numerics', ['bf16', 'parity', 'bf16x2'])
def test_training_step_is_bit_reproducible(numerics):
    """No atomics on the training path: split-K slabs are summed in fixed order, the attention backward kernels give every output element ONE owner, the
    BatchNorm partials are reduced in block order - the same step twice gives the same bits (logits and every gradient)."""
    from fewshot_vit_amd import models, synthetic
    m = models.make('meta-baseline', encoder='visformer_micro_80', encoder_args={'numerics': numerics, 'drop_path_rate': 0.5})
    m.load_state_dict(synthetic.synthetic_checkpoint_sd({k: tuple(v.shape) for k, v in m.state_dict().items()}), strict=True)
    m = m.cuda().train()
    E, way, shot, query = 2, 5, 2, 3
    xs, xq, label = _full_size_batch(E, way, shot, query)
    masks = (torch.rand(m.encoder.trainer().n_droppath_calls(0.5), E * way * (shot + query), generator=torch.Generator().manual_seed(3)) > 0.3).float().cuda()
    m.encoder.draw_droppath_masks = lambda n, dev: masks
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        sd0 = {k: v.clone() for k, v in m.state_dict().items()}
        logits = m(xs, xq).view(-1, way)
        F.cross_entropy(logits, label).backward()
        torch.cuda.synchronize()
        runs.append((logits.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}))
        m.load_state_dict(sd0)                      # (running statistics back to where they were)
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
