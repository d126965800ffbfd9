"""LV-ViT (`lvvit_micro_80`) on the MI355X: features, taps and meta-baseline logits against the reference goldens (tests/golden/lvvit.npz,
make_lvvit_golden.py), the non-power-of-two-channel conv route and the block kernels at the LV-ViT shape against fp32 torch, launch-size
invariance, and test_few_shot.evaluate() with the synthetic checkpoint."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
# 16-bit storage modes: gate ~1.5x the measured max |dfeat| against the reference (printed by the test; measured on one MI355X:
# parity 2.7e-6, bf16x2 3.2e-5, f16x2 5.9e-6, bf16 2.8e-2 .. 4.4e-2, f16 3.2e-3 .. 3.7e-3 - the ranges: conv_gemm_v2 / dedicated stem kernel)
FEAT_TOL = {'parity': 1e-3, 'bf16x2': 1e-3, 'f16x2': 1e-3, 'bf16': 0.07, 'f16': 5e-3}


def _golden(golden_dir):
    with np.load(os.path.join(golden_dir, 'lvvit.npz')) as z:
        return {k: z[k] for k in z.files}


def _encoder_sd(g):
    from fewshot_vit_amd import synthetic
    shapes = {k: tuple(int(d) for d in s.split(',') if d) for k, s in zip(g['keys'].tolist(), g['shapes'].tolist())}
    return synthetic.procedural_state_dict(shapes)


def _encoder(g, numerics):
    from fewshot_vit_amd import models
    m = models.make('lvvit_micro_80', numerics=numerics)
    m.load_state_dict(_encoder_sd(g), strict=True)
    return m.cuda().eval()


@pytest.mark.parametrize('numerics', ['parity', 'bf16x2', 'f16x2', 'bf16', 'f16'])
def test_lvvit_features_and_taps_vs_reference_golden(golden_dir, numerics):
    g = _golden(golden_dir)
    m = _encoder(g, numerics)
    x = torch.randn(4, 3, 80, 80, generator=torch.Generator().manual_seed(5))
    eng = m.engine()
    bufs = {'stem': eng.set_tap('stem', (1, 20, 20, 96))}
    bufs.update({k: eng.set_tap(k, (2, 26, 384)) for k in ('embed', 'blocks.3', 'blocks.7')})
    with torch.no_grad():
        feat = m(x.cuda()).cpu()
    err = np.abs(feat.numpy() - g['feat']).max()
    ref_taps = {'stem': torch.from_numpy(g['tap.stem']).permute(0, 2, 3, 1)}
    ref_taps.update({k: torch.from_numpy(g['tap.' + k]) for k in ('embed', 'blocks.3', 'blocks.7')})
    worst = {k: ((b.float().cpu() - ref_taps[k]).abs().max() / max(1.0, float(ref_taps[k].abs().max()))).item() for k, b in bufs.items()}
    print(f'[{numerics}] lvvit_micro_80: max|dfeat| vs reference golden = {err:.3e}; tap rel errors {worst}')
    assert feat.shape == (4, 384) and m.out_dim == 384
    assert err <= FEAT_TOL[numerics], (numerics, err)
    for k, v in worst.items():       # the DeiT test's per-mode bounds
        assert v <= (2e-4 if numerics == 'parity' else 1e-3 if numerics.endswith('x2') else 0.1), (k, v)


def test_lvvit_meta_baseline_logits_vs_reference_golden(golden_dir):
    from fewshot_vit_amd import models, synthetic
    g = _golden(golden_dir)
    sd = {'encoder.' + k: v for k, v in _encoder_sd(g).items()}
    sd['temp'] = torch.tensor(10.0)
    m = models.make('meta-baseline', encoder='lvvit_micro_80', encoder_args={'numerics': 'parity'})
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    for shot in (1, 5):
        xe = synthetic.synthetic_episodes(7, 1, 5, shot, 3).view(1, 5, shot + 3, 3, 80, 80)
        xs, xq = xe[:, :, :shot].contiguous(), xe[:, :, shot:].reshape(1, 15, 3, 80, 80).contiguous()
        with torch.no_grad():
            logits = m(xs.cuda(), xq.cuda()).cpu()
        err = (logits - torch.from_numpy(g[f'logits.{shot}shot'])).abs().max().item()
        print(f'lvvit meta-baseline 5-way {shot}-shot: max|dlogit| vs reference = {err:.3e}')
        assert err <= 1e-3, (shot, err)


def _pack(w, dtype):
    O, I, KH, KW = w.shape
    K = KH * KW * I
    bke = 32 if dtype == torch.float32 else 64
    p = torch.zeros(O, (K + bke - 1) // bke * bke)
    p[:, :K] = w.permute(0, 2, 3, 1).reshape(O, K)
    return p


@pytest.mark.parametrize('numerics', ['f32', 'bf16', 'f16', 'bf16x2', 'f16x2'])
@pytest.mark.parametrize('Cin,KH,s,p,H,B', [(96, 3, 1, 1, 40, 3), (160, 3, 1, 1, 12, 5), (96, 4, 4, 0, 20, 7)])
def test_conv_gemm_non_pow2_cin(numerics, Cin, KH, s, p, H, B):
    """conv_gemm_v2 with the tap found per K chunk by division: the stem 3x3 at 96 channels, a 160-channel 3x3, and the LV-ViT patch projection
    (4x4 / stride 4 over the pooled 20x20x96 map, K = 1536).  Odd batches; bias + LeakyReLU epilogue."""
    from fewshot_vit_amd.engine import ops
    x2 = numerics.endswith('x2')
    dtype = torch.float32 if x2 else DT[numerics]
    g = torch.Generator().manual_seed(Cin * 10 + KH)
    N = 96 if KH == 3 else 384
    x = torch.randn(B, Cin, H, H, generator=g)
    w = torch.randn(N, Cin, KH, KH, generator=g) / math.sqrt(Cin * KH * KH)
    bias = torch.randn(N, generator=g) * 0.3
    if not x2:
        x, w = x.to(dtype).float(), w.to(dtype).float()
    ref = F.leaky_relu(F.conv2d(x.double(), w.double(), bias.double(), stride=s, padding=p), 0.1)
    wp = _pack(w, dtype)
    wd = ops.x2_limbs(wp, numerics).cuda() if x2 else wp.to('cuda', dtype)
    y = ops.conv_gemm(x.permute(0, 2, 3, 1).contiguous().to('cuda', dtype), wd, bias.cuda(), None, None, B, H, H, Cin, KH, KH, s, p, N, 1, 2, 0,
                      numerics=numerics if x2 else None)
    torch.cuda.synchronize()
    err = (y.float().cpu().permute(0, 3, 1, 2).double() - ref).abs().max().item()
    scale = max(1.0, float(ref.abs().max()))
    tol = {'f32': 2e-4, 'bf16x2': 1e-4, 'f16x2': 2e-5, 'bf16': 1.2e-2, 'f16': 2e-3}[numerics]
    print(f'conv_gemm[{numerics}] Cin={Cin} k{KH}s{s}: max err {err:.3e}')
    assert err <= tol * scale, (numerics, Cin, KH, err)


def _stem_operands(B, dt_store, seed):
    """conv3 / tail operands at LV-ViT's stem width (96 channels, 40 x 40) pre-rounded to the storage type, the fp32 reference and the im2col rows."""
    g = torch.Generator().manual_seed(seed)
    H = W = 40
    C = 96

    def r(t):
        return t if dt_store is None else t.to(dt_store).float()
    x = r(torch.randn(B, C, H, W, generator=g))
    img = r(torch.randn(B, 3, 2 * H, 2 * W, generator=g))
    w3 = r(torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C))
    wd = r(torch.randn(C, 3, 3, 3, generator=g) / math.sqrt(27))
    bias = torch.randn(C, generator=g) * 0.3
    conv = F.conv2d(x.double(), w3.double(), None, padding=1) + bias.double().view(1, -1, 1, 1)
    ref2 = F.leaky_relu(conv, 0.1)
    ref3 = F.max_pool2d(F.leaky_relu(conv + F.conv2d(img.double(), wd.double(), None, stride=2, padding=1), 0.1), 2)
    cols = F.unfold(img, 3, padding=1, stride=2).view(B, 3, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 27)
    x2 = torch.zeros(B * H * W, 32)
    x2[:, :27] = cols
    return x, w3, wd, bias, x2, ref2, ref3


@pytest.mark.parametrize('numerics,B', [('bf16', 5), ('f16', 5), ('f32', 3), ('bf16x2', 3), ('f16x2', 3)])
def test_stem_tail_96_channels(numerics, B):
    """conv3 (96 -> 96) + the downsample as the tail K slice + LeakyReLU + MaxPool2d(2) at LV-ViT's stem width on conv_gemm_v2, every storage mode."""
    from fewshot_vit_amd.engine import ops
    x2m = numerics.endswith('x2')
    dtype = torch.float32 if x2m else DT[numerics]
    x, w3, wd, bias, x2, _, ref = _stem_operands(B, None if x2m or numerics == 'f32' else dtype, 96 + B)
    bke = 32 if dtype == torch.float32 else 64
    Kmain = (9 * 96 + bke - 1) // bke * bke
    wp = torch.zeros(96, Kmain + bke)
    wp[:, :9 * 96] = w3.permute(0, 2, 3, 1).reshape(96, 9 * 96)
    wp[:, Kmain:Kmain + 27] = wd.permute(0, 2, 3, 1).reshape(96, 27)
    wdev = ops.x2_limbs(wp, numerics).cuda() if x2m else wp.to('cuda', dtype)
    pos = torch.zeros(20 * 20, 96)
    y = ops.conv_stem_tail(x.permute(0, 2, 3, 1).contiguous().to('cuda', dtype), wdev, bias.cuda(), pos.cuda(), x2.to('cuda', dtype), 32,
                           numerics=numerics if x2m else None)
    torch.cuda.synchronize()
    err = (y.float().cpu().permute(0, 3, 1, 2).double() - ref).abs()
    print(f'stem tail 96 [{numerics}]: max err {err.max().item():.3e}')
    if numerics in ('bf16', 'f16'):       # output rounding of the 16-bit type + accumulation order
        bound = (2.0 ** -8 if numerics == 'bf16' else 2.0 ** -10) * ref.abs() + 2e-3
        assert bool((err <= bound).all()), (float(err.max()), float((err - bound).max()))
    else:
        tol = {'f32': 2e-4, 'bf16x2': 1e-4, 'f16x2': 2e-5}[numerics]
        assert err.max().item() <= tol * max(1.0, float(ref.abs().max()))


def _image128(w, tail=None):
    """the dedicated kernel's 128-channel weight image: [128][9*128 (+64)], k = tap*128 + c, zero past 96 channels / rows, tail slice last"""
    Kw = 9 * 128 + (64 if tail is not None else 0)
    img = torch.zeros(128, Kw)
    img[:96, :9 * 128].view(96, 9, 128)[:, :, :96] = w.permute(0, 2, 3, 1).reshape(96, 9, 96)
    if tail is not None:
        img[:96, 9 * 128:9 * 128 + 27] = tail.permute(0, 2, 3, 1).reshape(96, 27)
    return img


@pytest.mark.parametrize('dt', ['bf16', 'f16'])
@pytest.mark.parametrize('B', [5, 13])
def test_dedicated_stem96_kernel(dt, B):
    """The dedicated 96-channel stem kernel (conv3x3_halo at CREAL = 96): conv2 (+ bias + LeakyReLU) and conv3 + downsample tail + LeakyReLU +
    MaxPool2d(2) against fp64 torch on the same rounded operands, and against the conv_gemm_v2 route on the same inputs."""
    from fewshot_vit_amd.engine import ops
    dtype = DT[dt]
    x, w3, wd, bias, x2, ref2, ref3 = _stem_operands(B, dtype, 960 + B)
    xd = x.permute(0, 2, 3, 1).contiguous().to('cuda', dtype)
    y2 = ops.stem96_conv(xd, _image128(w3).to('cuda', dtype), bias.cuda())
    y3 = ops.stem96_conv(xd, _image128(w3, wd).to('cuda', dtype), bias.cuda(), x2.to('cuda', dtype), 32)
    torch.cuda.synchronize()
    assert y2.shape == (B, 40, 40, 96) and y3.shape == (B, 20, 20, 96)
    step = 2.0 ** -8 if dt == 'bf16' else 2.0 ** -10
    for name, y, ref in (('conv2', y2, ref2), ('conv3+tail', y3, ref3)):
        err = (y.float().cpu().permute(0, 3, 1, 2).double() - ref).abs()
        print(f'stem96 dedicated [{dt}] {name} B={B}: max err {err.max().item():.3e}')
        assert bool((err <= step * ref.abs() + 2e-3).all()), (name, float(err.max()))
    # the same layer on conv_gemm_v2 (route (a)): both round once at the output, so they agree to about one output ulp
    w2p = torch.zeros(96, 896)
    w2p[:, :864] = w3.permute(0, 2, 3, 1).reshape(96, 864)
    ya = ops.conv_gemm(xd, w2p.to('cuda', dtype), bias.cuda(), None, None, B, 40, 40, 96, 3, 3, 1, 1, 96, 1, 2, 0)
    d = (ya.float() - y2.float()).abs().cpu()
    assert bool((d <= 2 * step * ya.float().abs().cpu() + 2e-3).all()), float(d.max())


@pytest.mark.parametrize('M', [26 * 3, 26 * 200 + 13])
def test_block_tail_hidden_1152(M):
    """mlp_rows_ln at LV-ViT's hidden width 1152 (36 chunks of 32) against fp32 torch with the kernel's bf16 rounding points."""
    from fewshot_vit_amd.engine import ops
    bf = torch.bfloat16
    C, KC, HID, eps = 384, 384, 1152, 1e-5
    g = torch.Generator().manual_seed(M)

    def r(t):
        return t.to(bf).float()
    x = r(torch.randn(M, C, generator=g) * 2.0 + 0.5)
    ctx = r(torch.randn(M, KC, generator=g))
    wp = r(torch.randn(C, KC, generator=g) / math.sqrt(KC))
    bp = torch.randn(C, generator=g) * 0.3
    w1 = r(torch.randn(HID, C, generator=g) / math.sqrt(C))
    b1 = torch.randn(HID, generator=g) * 0.3
    w2 = r(torch.randn(C, HID, generator=g) / math.sqrt(HID))
    b2 = torch.randn(C, generator=g) * 0.3
    x1 = r(x + ctx @ wp.t() + bp)
    xn = r(F.layer_norm(x1, (C,), eps=eps))
    ref = x1 + r(F.gelu(r(xn @ w1.t() + b1))) @ w2.t() + b2
    args = [x.to('cuda', bf), ctx.to('cuda', bf), wp.to('cuda', bf), bp.cuda(), w1.to('cuda', bf), b1.cuda(), w2.to('cuda', bf), b2.cuda()]
    y0 = ops.vit_block_tail(*args, eps=eps)
    torch.cuda.synchronize()
    err = (y0.float().cpu() - ref).abs()
    print(f'mlp_rows_ln hidden 1152 M={M}: max err {err.max().item():.3e} mean {err.mean().item():.3e}')
    assert err.max().item() <= 4e-2 * max(1.0, float(ref.abs().max())), (M, err.max().item())
    assert err.mean().item() <= 4e-3, (M, err.mean().item())
    assert torch.equal(ops.vit_block_tail(*args, eps=eps), y0)


@pytest.mark.parametrize('B', [1, 13])
def test_vit_attn_rows_26_tokens(B):
    """vit_attn_rows at LV-ViT's 26 tokens, no qkv bias of its own (the packed bias is the folded norm1 shift), LayerNorm eps 1e-5."""
    from fewshot_vit_amd.engine import ops
    bf = torch.bfloat16
    C, heads, hd, S, eps = 384, 6, 64, 26, 1e-5
    g = torch.Generator().manual_seed(B * 26)
    x = (torch.randn(B * S, C, generator=g) * 1.5 + 0.3).to(bf).float()
    w = (torch.randn(3 * heads * hd, C, generator=g) / math.sqrt(C)).to(bf).float()
    beta = torch.randn(C, generator=g) * 0.1
    bias = w @ beta
    scale = hd ** -0.5
    xn = F.layer_norm(x, (C,), eps=eps).to(bf).float()
    qkv = (xn @ w.t() + bias).to(bf).float().reshape(B, S, 3, heads, hd)
    qq, kk, vv = [qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3)]
    ref = (((qq @ kk.transpose(-1, -2)) * scale).softmax(-1) @ vv).permute(0, 2, 1, 3).reshape(B * S, heads * hd)
    got = ops.vit_ln_qkv_attention(x.to('cuda', bf), w.to('cuda', bf), bias.cuda(), B, S, heads, hd, scale, eps=eps).float().cpu()
    err = (got - ref).abs()
    print(f'vit_attn_rows S=26 B={B}: max err {err.max().item():.3e} mean {err.mean().item():.3e}')
    assert torch.isfinite(got).all()
    assert err.max().item() <= 3e-2 * max(1.0, float(ref.abs().max())) and err.mean().item() <= 3e-3


@pytest.mark.parametrize('numerics', ['bf16', 'parity'])
def test_launch_size_invariance_across_stem_slices(golden_dir, numerics):
    """3213 images = one full stem slice (3200) + 13: the last 13 images give the same features as the same 13 run alone (the second slice's input
    and token-row offsets and the reuse of the per-slice scratch)."""
    g = _golden(golden_dir)
    m = _encoder(g, numerics)
    x = torch.randn(3213, 3, 80, 80, generator=torch.Generator().manual_seed(3213)).cuda()
    with torch.no_grad():
        whole = m(x)
        tail = m(x[3200:].contiguous())
        head = m(x[:13].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(whole[3200:], tail)
    assert torch.equal(whole[:13], head)


@pytest.mark.parametrize('numerics', ['bf16', 'parity'])
def test_launch_size_invariance(golden_dir, numerics):
    """13 images give the same features alone, inside a larger launch, and across a chunk boundary (chunk of 8 images, so the stem
    slices and the block launches both split)."""
    from fewshot_vit_amd.engine import LvvitEngine
    g = _golden(golden_dir)
    m = _encoder(g, numerics)
    x = torch.randn(40, 3, 80, 80, generator=torch.Generator().manual_seed(13)).cuda()
    with torch.no_grad():
        alone = m(x[:13].contiguous())
        inside = m(x)[:13]
    eng = LvvitEngine(m.cfg, m.state_dict(), numerics=numerics, device='cuda', chunk_images=8)
    chunked = eng.forward(x[3:16].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(alone, inside)
    assert torch.equal(alone[3:], chunked[:10])


def test_evaluate_synthetic_checkpoint_bf16_vs_parity():
    """test_few_shot.evaluate() with `synthetic_checkpoint: lvvit_micro_80` (procedural weights, no calibration file) over 300 seeded 5-way
    5-shot episodes: finite statistics, and the per-query arg-max of bf16 against parity on the same episodes."""
    import yaml
    from fewshot_vit_amd import test_few_shot
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(repo, 'few-shot-vit_amd', 'configs', 'test_synthetic.yaml')))
    cfg.pop('load', None)
    cfg['synthetic_checkpoint'] = 'lvvit_micro_80'
    n = 300
    logs = []
    a = test_few_shot.evaluate(cfg, shot=5, n_batch=n, launch_batches=64, numerics='bf16', log=logs.append, collect_pred=True)
    p = test_few_shot.evaluate(cfg, shot=5, n_batch=n, launch_batches=64, numerics='parity', log=logs.append, collect_pred=True)
    agree = float((a['pred'] == p['pred']).float().mean())
    print(f"[lvvit agreement] bf16 acc {a['acc']:.4f} +- {a['ci']:.4f}, parity acc {p['acc']:.4f} +- {p['ci']:.4f}, "
          f"per-query arg-max agreement {agree:.5f} over {a['pred'].numel()} queries")
    for r in (a, p):
        assert r['n'] == n and all(math.isfinite(v) for v in (r['acc'], r['ci'], r['loss']))
    assert agree >= 0.98
