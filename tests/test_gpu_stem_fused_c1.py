"""Stem conv1 built inside the conv2 kernel (conv3x3_halo.hip, C1F; FSVIT_STEM_FUSE_C1, default on) against the parent route that keeps
stem_conv1_kernel and the c1 map in HBM (FSVIT_STEM_FUSE_C1=0): the fused kernel runs the statements of stem_conv1_kernel in the same order, so the
`stem` tap and the final features must be EQUAL bit for bit, whatever the batch does to the tile schedule."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _engine(sd, fuse, numerics='bf16'):
    """A Visformer engine created with FSVIT_STEM_FUSE_C1 = fuse (the switch is read once, when the engine is created)."""
    from fewshot_vit_amd import models
    old = os.environ.get('FSVIT_STEM_FUSE_C1')
    os.environ['FSVIT_STEM_FUSE_C1'] = fuse
    try:
        m = models.make('meta-baseline', encoder='visformer_micro_80', encoder_args={'numerics': numerics})
        m.load_state_dict(sd, strict=True)
        m = m.cuda().eval()
        eng = m.encoder.engine()
    finally:
        if old is None:
            del os.environ['FSVIT_STEM_FUSE_C1']
        else:
            os.environ['FSVIT_STEM_FUSE_C1'] = old
    return m, eng


@pytest.fixture(scope='module')
def sd():
    from fewshot_vit_amd import synthetic
    from oracle import visformer_oracle as vo
    shapes = vo.state_dict_shapes(vo.VisformerCfg(), prefix='encoder.')
    shapes['temp'] = ()
    return synthetic.synthetic_checkpoint_sd(shapes)


@pytest.fixture(scope='module')
def engines(sd):
    return _engine(sd, '1'), _engine(sd, '0')


def _run(eng, x):
    tap = eng.set_tap('stem', (x.shape[0], 20, 20, 128))
    feat = eng.forward(x)
    torch.cuda.synchronize()
    return tap, feat


def _images(B, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return torch.randn(B, 3, 80, 80, generator=g, device='cuda')


def _assert_same(got, ref, what):
    same = torch.equal(got, ref)
    n_diff = 0 if same else int((got != ref).sum().item())
    print(f'{what}: {"equal" if same else f"{n_diff} of {got.numel()} values differ"}')
    assert same, what


# 1: five tiles, both image borders; 53: 265 tiles on 256 workgroups - nine workgroups hand a window over to a second tile;
# 3201: the second stem slice holds one image
@pytest.mark.parametrize('B', [1, 53, 3201])
def test_fused_route_equals_parent_route(engines, B):
    (_, fused), (_, parent) = engines
    x = _images(B, 100 + B)
    tap_f, feat_f = _run(fused, x)
    tap_p, feat_p = _run(parent, x)
    assert bool(tap_p.float().abs().max() > 0)
    _assert_same(tap_f, tap_p, f'B={B} stem tap')
    _assert_same(feat_f, feat_p, f'B={B} features')


def test_shot_and_query_pointers(engines):
    """1 shot image + 2 query images in one pass: image 0 comes from the shot tensor, images 1 and 2 from the query tensor."""
    (_, fused), (_, parent) = engines
    xs = _images(1, 7).view(1, 1, 1, 3, 80, 80)
    xq = _images(2, 8).view(1, 2, 3, 80, 80)
    out = []
    for eng in (fused, parent):
        tap = eng.set_tap('stem', (3, 20, 20, 128))
        logits = eng.meta_baseline_forward(xs, xq, 10.0)
        torch.cuda.synchronize()
        out.append((tap, logits))
    # the same three images as one tensor through the plain forward of the parent route: the split itself moves nothing
    tap_cat, _ = _run(parent, torch.cat([xs.view(1, 3, 80, 80), xq.view(2, 3, 80, 80)]))
    _assert_same(out[0][0], out[1][0], 'shot + query stem tap')
    _assert_same(out[0][1], out[1][1], 'shot + query logits')
    _assert_same(out[0][0], tap_cat, 'shot + query stem tap vs one tensor')


def test_constant_images_padding(engines):
    """An all-zero and an all-ones image: c1 next to the border is LeakyReLU(bias + ...) while conv2's padding ring must be zero - a padding row
    written as LeakyReLU(bias), or a left tap that reads the previous row, shows as a mismatch against the parent route."""
    (_, fused), (_, parent) = engines
    x = torch.zeros(2, 3, 80, 80, device='cuda')
    x[1] = 1.0
    tap_f, feat_f = _run(fused, x)
    tap_p, feat_p = _run(parent, x)
    assert bool(tap_p.float().abs().max() > 0)
    _assert_same(tap_f, tap_p, 'constant images stem tap')
    _assert_same(feat_f, feat_p, 'constant images features')


def test_f16_build_of_the_fused_kernel(sd):
    """The -DFSVIT_HALF_F16 build of the same source (numerics 'f16'): 7 images = 35 tiles, every border case."""
    (_, fused), (_, parent) = _engine(sd, '1', 'f16'), _engine(sd, '0', 'f16')
    x = _images(7, 77)
    tap_f, feat_f = _run(fused, x)
    tap_p, feat_p = _run(parent, x)
    assert bool(tap_p.float().abs().max() > 0)
    _assert_same(tap_f, tap_p, 'f16 stem tap')
    _assert_same(feat_f, feat_p, 'f16 features')
