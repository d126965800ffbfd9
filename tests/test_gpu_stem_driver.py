"""The eval stem driver (engine.hip: EvalStem / stem_forward) and the workspace layouts behind `fsvit_*_workspace_bytes`.

The stem runs in slices of 3200 images whose scratch (im2col rows, c1, c2, LV-ViT's pooled map) is sized for ONE slice and overwritten by the next, and a
MetaBaseline call reads the images of a slice from two tensors (shot, query).  Neither may move a bit: eval mode is per-image independent, so every
comparison here is for equality."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SLICE = 3200                  # stem_slice_images() of engine.hip


def _with_env(name, value, make):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return make()
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


@pytest.fixture(scope='module')
def visformer():
    """The encoder module of a meta-baseline model with the synthetic visformer_micro_80 checkpoint (its `cfg` and `state_dict()` build the engines)."""
    from fewshot_vit_amd import models, synthetic
    from oracle import visformer_oracle as vo
    shapes = vo.state_dict_shapes(vo.VisformerCfg(), prefix='encoder.')
    shapes['temp'] = ()
    m = models.make('meta-baseline', encoder='visformer_micro_80', encoder_args={'numerics': 'bf16'})
    m.load_state_dict(synthetic.synthetic_checkpoint_sd(shapes), strict=True)
    return m.cuda().eval().encoder


@pytest.fixture(scope='module')
def lvvit():
    from fewshot_vit_amd import models, synthetic
    m = models.make('lvvit_micro_80', numerics='bf16')
    m.load_state_dict(synthetic.procedural_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}), strict=True)
    return m.cuda().eval()


def _visformer_engine(enc, fuse, chunk=None):
    """A bf16 VisformerEngine built with FSVIT_STEM_FUSE_C1 = fuse (read once, at create): '1' the C1F route, '0' the planar three-launch route."""
    from fewshot_vit_amd import engine as E
    return _with_env('FSVIT_STEM_FUSE_C1', fuse, lambda: E.VisformerEngine(enc.cfg, enc.state_dict(), numerics='bf16', device='cuda', chunk_images=chunk))


@pytest.fixture(scope='module')
def engines(visformer):
    """fuse -> a VisformerEngine at the default chunk (12 800 images)."""
    return {fuse: _visformer_engine(visformer, fuse) for fuse in ('1', '0')}


@pytest.fixture(scope='module')
def images():
    """3201 seeded images: one chunk of two slices (3200 + 1) for an engine whose chunk holds them."""
    return torch.randn(SLICE + 1, 3, 80, 80, generator=torch.Generator(device='cuda').manual_seed(3201), device='cuda')


def _assert_same(got, ref, what):
    same = torch.equal(got, ref)
    print(f'{what}: {"equal" if same else f"{int((got != ref).sum().item())} of {got.numel()} values differ"}')
    assert same, what


# ---------------------------------------------------------------------------------------------------------------- 1. slice reuse
@pytest.mark.parametrize('fuse', ['1', '0'])
def test_visformer_second_slice_overwrites_the_first(visformer, images, fuse):
    """chunk 3300: ONE chunk of two slices, the second (one image) runs in the scratch of the first.  chunk 1000: four chunks of one slice each.  The `stem`
    tap is taken from a call's first chunk: images [0, 1000) of the sliced engine's tap against the small-chunk engine's, and image 3200 - the second
    slice - against the small-chunk engine run on that image alone."""
    two_slices, one_slice = _visformer_engine(visformer, fuse, 3300), _visformer_engine(visformer, fuse, 1000)
    tap2 = two_slices.set_tap('stem', (SLICE + 1, 20, 20, 128))
    feat2 = two_slices.forward(images)
    tap1 = one_slice.set_tap('stem', (1000, 20, 20, 128))
    feat1 = one_slice.forward(images)
    torch.cuda.synchronize()
    assert bool(tap1.float().abs().max() > 0)
    _assert_same(feat2, feat1, f'fuse={fuse} features')
    _assert_same(tap2[:1000], tap1, f'fuse={fuse} stem tap, first slice')
    tap_last = one_slice.set_tap('stem', (1, 20, 20, 128))
    one_slice.forward(images[SLICE:])
    torch.cuda.synchronize()
    _assert_same(tap2[SLICE:], tap_last, f'fuse={fuse} stem tap, second slice')


def test_lvvit_second_slice_overwrites_the_first(lvvit, images):
    """LvvitEngine across the slice boundary (its `stem` tap covers the first slice only: features)."""
    from fewshot_vit_amd import engine as E
    two_slices = E.LvvitEngine(lvvit.cfg, lvvit.state_dict(), numerics='bf16', device='cuda', chunk_images=3300)
    one_slice = E.LvvitEngine(lvvit.cfg, lvvit.state_dict(), numerics='bf16', device='cuda', chunk_images=1000)
    feat2, feat1 = two_slices.forward(images), one_slice.forward(images)
    torch.cuda.synchronize()
    assert bool(feat1.abs().max() > 0)
    _assert_same(feat2, feat1, 'lvvit features')


# ---------------------------------------------------------------------------------------------------------------- 2. two-source split
# (E, way, shot, Q) -> (shots, queries): the split inside slice 0 (5, 10), exactly on the slice boundary (3200, 128), inside slice 1 (3205, 641)
@pytest.mark.parametrize('fuse', ['1', '0'])
@pytest.mark.parametrize('E_,way,shot,Q', [(1, 5, 1, 10), (128, 5, 5, 1), (641, 5, 1, 1)])
def test_shot_query_split_against_one_tensor(engines, fuse, E_, way, shot, Q):
    from fewshot_vit_amd import engine as E
    eng = engines[fuse]
    g = torch.Generator(device='cuda').manual_seed(E_ * 100 + Q)
    xs = torch.randn(E_, way, shot, 3, 80, 80, generator=g, device='cuda')
    xq = torch.randn(E_, Q, 3, 80, 80, generator=g, device='cuda')
    ns = E_ * way * shot
    logits = eng.meta_baseline_forward(xs, xq, 10.0)
    feat = eng.forward(torch.cat([xs.view(ns, 3, 80, 80), xq.view(E_ * Q, 3, 80, 80)]))
    ref, _, _ = E.ops.proto_head(feat[:ns].view(E_, way, shot, -1), feat[ns:].view(E_, Q, -1), 10.0)
    torch.cuda.synchronize()
    assert bool(ref.abs().max() > 0)
    _assert_same(logits, ref, f'fuse={fuse} ({ns} shots, {E_ * Q} queries) logits')


# ---------------------------------------------------------------------------------------------------------------- 3. plan properties
SIZES = list(range(1, 41)) + [SLICE - 1, SLICE, SLICE + 1, 2 * SLICE]


def _ws(eng, n):
    return int(getattr(eng.lib, eng._fn['workspace_bytes'])(eng.h, n))


def _assert_monotone(eng, what):
    got = [_ws(eng, n) for n in SIZES]
    print(what, 'workspace_bytes at', SIZES[-4:], '=', got[-4:])
    assert got[0] > 0
    assert all(a <= b for a, b in zip(got, got[1:])), [(n, a, b) for n, a, b in zip(SIZES, got, got[1:]) if a > b]


def test_workspace_bytes_monotone_visformer(engines):
    _assert_monotone(engines['1'], 'visformer')


def test_workspace_bytes_monotone_lvvit(lvvit):
    _assert_monotone(lvvit.engine(), 'lvvit')


def test_workspace_bytes_monotone_vit():
    from fewshot_vit_amd import models, synthetic
    m = models.make('deit_micro_patch6_84', numerics='bf16')
    m.load_state_dict(synthetic.procedural_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}), strict=True)
    _assert_monotone(m.cuda().eval().engine(), 'deit')


def _a256(v):
    return (v + 255) // 256 * 256


def _padded_head_dim(hd):
    """16-bit storage, maps of at most 224 tokens (attention.hip): multiples of 16 where a tile schedule is built for them, multiples of 32 otherwise."""
    h16 = (hd + 15) // 16 * 16
    return h16 if h16 // 16 in (2, 3, 4, 6, 8) else (hd + 31) // 32 * 32


def test_visformer_c1f_workspace_is_residual_streams_plus_largest_scratch_region(visformer, engines):
    """The layout of a chunk of n bf16 images, restated from the configuration alone (nothing here is read back from the library):

        workspace(n) = R(n) + max(stem(min(n, 3200)), stage1(n), stage23(n)),    every buffer rounded up to 256 bytes

      R(n)       the four residual streams x1, x1b [n][20*20][128], x2 [n][10*10][256], x3 [n][5*5][512]: 281 600 bytes per image
      stem(m)    the scratch of ONE stem slice on the C1F route: im2col rows [m][40*40][32] + c2 [m][40*40][128] (no c1): 512 000 bytes per image
      stage1(n)  the two hidden maps [n][20*20][256]: 409 600 bytes per image
      stage23(n) qkv + ctx + hidden map, each sized for the larger of stage 2 (100 tokens) and stage 3 (25 tokens): 435 200 bytes per image

    While the stem region is the largest - 3200 * 512 000 > n * 435 200, n <= 3764 - the workspace grows by the residual streams alone: that is asserted
    between 3200 and 3300 images (the stem scratch has stopped growing with the chunk).  At 6400 images stage23 (6400 * 435 200) has passed the 3200-image
    stem slice, so workspace(6400) - workspace(3200) = R(6400) - R(3200) + stage23(6400) - stem(3200) = 3200 * (281 600 + 2 * 435 200 - 512 000)
    = 2 048 000 000 bytes, not 3200 * 281 600; with a stem scratch sized for the chunk it would be 3200 * (281 600 + 512 000)."""
    cfg, es = visformer.cfg, 2
    D, heads = cfg['embed_dim'], cfg['num_heads']
    C1, C2, C3 = D // 2, D, 2 * D
    P0, P1, P2, P3 = ((cfg['img_size'] // k) ** 2 for k in (2, 4, 8, 16))
    hdp2, hdp3 = _padded_head_dim(round(C2 // heads)), _padded_head_dim(round(C3 // heads))
    hid1, hid2, hid3 = 2 * C1, int(C2 * cfg.get('mlp_ratio', 4.0)), int(C3 * cfg.get('mlp_ratio', 4.0))

    def resid(n):
        return 2 * _a256(n * P1 * C1 * es) + _a256(n * P2 * C2 * es) + _a256(n * P3 * C3 * es)

    def stem(m):
        return _a256(m * P0 * 32 * es) + _a256(m * P0 * C1 * es)

    def stage1(n):
        return 2 * _a256(n * P1 * hid1 * es)

    def stage23(n):
        return (_a256(n * max(P2 * 3 * heads * hdp2, P3 * 3 * heads * hdp3) * es) + _a256(n * max(P2 * heads * hdp2, P3 * heads * hdp3) * es)
                + _a256(n * max(P2 * hid2, P3 * hid3) * es))

    def expected(n):
        return resid(n) + max(stem(min(n, SLICE)), stage1(n), stage23(n))

    eng = engines['1']
    got = {n: _ws(eng, n) for n in (1, 53, SLICE, SLICE + 100, 2 * SLICE)}
    print('workspace_bytes:', got)
    assert stem(SLICE) > max(stage1(SLICE + 100), stage23(SLICE + 100)) and stage23(2 * SLICE) > max(stem(SLICE), stage1(2 * SLICE))
    assert got[SLICE + 100] - got[SLICE] == resid(SLICE + 100) - resid(SLICE) == 100 * 281600
    assert got[2 * SLICE] - got[SLICE] == resid(2 * SLICE) - resid(SLICE) + stage23(2 * SLICE) - stem(SLICE) == 2048000000
    for n, v in got.items():
        assert v == expected(n), (n, v, expected(n))


# ---------------------------------------------------------------------------------------------------------------- 4. small workspace
def test_forward_in_a_workspace_for_one_image(engines):
    """fsvit_visformer_forward with a workspace of exactly workspace_bytes(1) for 3 images: three chunks of one image, the features of the full-workspace call."""
    from fewshot_vit_amd import _lib
    from fewshot_vit_amd import engine as E
    eng = engines['1']
    x = torch.randn(3, 3, 80, 80, generator=torch.Generator(device='cuda').manual_seed(4), device='cuda')
    ref = eng.forward(x)
    ws = torch.empty(_ws(eng, 1), dtype=torch.uint8, device='cuda')
    assert ws.data_ptr() % 256 == 0 and ws.numel() < _ws(eng, 2)
    feat = torch.zeros_like(ref)
    _lib.check(eng.lib.fsvit_visformer_forward(eng.h, E._ptr(x), 3, 80, 80, E._ptr(feat), E._ptr(ws), ws.numel(), E._stream_ptr(x.device)))
    torch.cuda.synchronize()
    assert bool(ref.abs().max() > 0)
    _assert_same(feat, ref, 'one-image workspace features')
