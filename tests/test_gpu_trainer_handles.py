"""Characterisation of the step driver both trainer handles share (train_engine.hip `trainer_forward` / `trainer_backward`, engine.py `_Trainer`):
every refusal a caller can see - code, exception type and text - on a tiny Visformer (the `tiny_visformer` geometry of test_boundary_cpu.py) and on
deit_nano_patch6_84.  Every expectation is what the library of commit afb0c5c answers, where the Visformer and the ViT driver were two copies
(codes, texts and their order of precedence read off that commit's train_engine.hip / engine.py); the exact workspace sizes of that commit are
in test_trainer_workspace_cpu.py (the sizing pass needs no device).

All refusals are argument errors that return before any launch; the only launches here are ordinary training steps of two or fewer images."""
import pytest
import torch

from fewshot_vit_amd import _lib

pytestmark = pytest.mark.gpu

KINDS = ('visformer', 'deit')
FN = {'visformer': dict(ws='fsvit_visformer_trainer_workspace_bytes', fwd='fsvit_visformer_train_forward', bwd='fsvit_visformer_train_backward'),
      'deit': dict(ws='fsvit_vit_trainer_workspace_bytes', fwd='fsvit_vit_train_forward', bwd='fsvit_vit_train_backward')}
IMG = {'visformer': 80, 'deit': 84}
SIZE_TEXT = {'visformer': 'Input image size (64*64) does not match model (80*80).', 'deit': "Input image size (64*64) doesn't match model (84*84)."}
MISSING = {'visformer': 'stage3.0.norm1.bn.weight', 'deit': 'blocks.7.mlp.fc2.bias'}
NO_FORWARD = 'train_backward called without a preceding train_forward'
BN_TEXT = 'Expected more than 1 value per channel when training (BatchNorm)'


def _model(kind, **kw):
    if kind == 'visformer':
        from fewshot_vit_amd.models.visformer import Visformer
        return Visformer(**{**dict(img_size=80, init_channels=8, embed_dim=64, depth=[1, 1, 1], num_heads=6, mlp_ratio=4., group=8), **kw}).cuda()
    from fewshot_vit_amd.models import deit
    return deit.deit_nano_patch6_84(**kw).cuda()


def _setup(kind, numerics='bf16', **kw):
    """-> (trainer, tensors): a fresh trainer handle and the fp32 cuda tensors of a freshly initialised model."""
    from fewshot_vit_amd import engine
    m = _model(kind, **kw)
    tr = (engine.VisformerTrainer if kind == 'visformer' else engine.VitTrainer)(m.cfg, numerics=numerics, device='cuda:0')
    return tr, {k: v.detach() for k, v in m.state_dict().items() if not k.endswith('num_batches_tracked')}


def _x(kind, n_img, img=None, seed=5):
    img = img or IMG[kind]
    return torch.randn(n_img, 3, img, img, generator=torch.Generator().manual_seed(seed)).cuda()


def _table(tensors, grads):
    from fewshot_vit_amd import engine
    return engine.VisformerTrainer._table(tensors, grads)       # the one table builder both trainers use


def _c_forward(tr, kind, tensors, x, rate=0.0, masks=None, ws=None, ws_bytes=None):
    """The C entry itself (no Python-side sizing in front of it) -> (return code, fsvit_last_error())."""
    arr, keep = _table(tensors, None)
    ws = ws if ws is not None else torch.empty(1 << 20, dtype=torch.uint8, device='cuda:0')
    feat = torch.empty(x.shape[0], tr.out_dim, device='cuda:0')
    rc = getattr(tr.lib, FN[kind]['fwd'])(tr.h, arr, len(tensors), x.data_ptr(), x.shape[0], x.shape[2], x.shape[3], float(rate),
                                          None if masks is None else masks.data_ptr(), feat.data_ptr(), ws.data_ptr(),
                                          ws.numel() if ws_bytes is None else ws_bytes, torch.cuda.current_stream().cuda_stream)
    return rc, tr.lib.fsvit_last_error().decode()


def _c_backward(tr, kind, tensors):
    grads = {k: torch.empty_like(v) for k, v in tensors.items()}
    arr, keep = _table(tensors, grads)
    dfeat = torch.zeros(2, tr.out_dim, device='cuda:0')
    rc = getattr(tr.lib, FN[kind]['bwd'])(tr.h, arr, len(tensors), dfeat.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return rc, tr.lib.fsvit_last_error().decode()


@pytest.mark.parametrize('kind', KINDS)
def test_missing_parameter_is_a_keyerror_naming_it(kind):
    tr, tensors = _setup(kind)
    short = {k: v for k, v in tensors.items() if k != MISSING[kind]}
    with pytest.raises(KeyError, match='missing parameter: ' + MISSING[kind].replace('.', r'\.')):      # the workspace_bytes route (engine.py sizes first)
        tr.forward(short, _x(kind, 2))
    rc, msg = _c_forward(tr, kind, short, _x(kind, 2))                                                 # the forward route (its own sizing pass)
    assert rc == _lib.ERR_KEY and msg == 'missing parameter: ' + MISSING[kind]
    with pytest.raises(KeyError, match='missing parameter'):
        _lib.check(rc)


@pytest.mark.parametrize('kind', KINDS)
def test_wrong_image_size_has_the_models_own_sentence(kind):
    tr, tensors = _setup(kind)
    with pytest.raises(AssertionError) as e:
        tr.forward(tensors, _x(kind, 2, img=64))
    assert str(e.value) == SIZE_TEXT[kind]
    rc, msg = _c_forward(tr, kind, tensors, _x(kind, 2, img=64), rate=0.5)      # the size is checked before the DropPath masks
    assert rc == _lib.ERR_IMG_SIZE and msg == SIZE_TEXT[kind]


@pytest.mark.parametrize('kind', KINDS)
def test_droppath_rate_without_masks_is_an_argument_error(kind):
    tr, tensors = _setup(kind, drop_path_rate=0.5)
    with pytest.raises(ValueError, match='DropPath masks required when drop_path_rate > 0'):
        tr.forward(tensors, _x(kind, 2), drop_path_rate=0.5, masks=None)
    rc, msg = _c_forward(tr, kind, tensors, _x(kind, 2), rate=0.5)
    assert rc == _lib.ERR_ARG and msg == 'DropPath masks required when drop_path_rate > 0'


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('rate', [0.0, 0.5])
def test_workspace_one_byte_short(kind, rate):
    tr, tensors = _setup(kind, drop_path_rate=rate)
    arr, keep = _table(tensors, None)
    need = getattr(tr.lib, FN[kind]['ws'])(tr.h, arr, len(tensors), 2, float(rate))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda:0')
    masks = torch.ones(tr.n_droppath_calls(rate), 2, device='cuda:0') if rate else None
    rc, msg = _c_forward(tr, kind, tensors, _x(kind, 2), rate=rate, masks=masks, ws=ws, ws_bytes=need - 1)
    assert rc == _lib.ERR_WORKSPACE and msg == 'training workspace of %d bytes is too small (need %d)' % (need - 1, need)
    with pytest.raises(_lib.FsvitError, match='need %d' % need):
        _lib.check(rc)
    rc, msg = _c_backward(tr, kind, tensors)             # the refused forward left nothing behind to run a backward on
    assert rc == _lib.ERR_ARG and msg == NO_FORWARD


@pytest.mark.parametrize('kind', KINDS)
def test_backward_before_forward_and_twice(kind):
    tr, tensors = _setup(kind)
    rc, msg = _c_backward(tr, kind, tensors)             # fresh handle
    assert rc == _lib.ERR_ARG and msg == NO_FORWARD
    arr, keep = _table(tensors, None)
    assert getattr(tr.lib, FN[kind]['ws'])(tr.h, arr, len(tensors), 2, 0.0) > 0
    rc, msg = _c_backward(tr, kind, tensors)             # a sizing pass is not a forward
    assert rc == _lib.ERR_ARG and msg == NO_FORWARD
    grads = {k: torch.empty_like(v) for k, v in tensors.items()}
    with pytest.raises(RuntimeError, match='backward without a pending train-mode forward'):
        tr.backward(tensors, grads, torch.zeros(2, tr.out_dim, device='cuda:0'))
    gen = tr.generation
    feat = tr.forward(tensors, _x(kind, 2))
    assert tr.generation == gen + 1 and feat.shape == (2, tr.out_dim) and bool(torch.isfinite(feat).all())
    tr.backward(tensors, grads, torch.ones_like(feat))
    torch.cuda.synchronize()
    params = [k for k in tensors if not k.endswith(('running_mean', 'running_var'))]
    assert all(bool(torch.isfinite(grads[k]).all()) for k in params)
    with pytest.raises(RuntimeError, match='backward without a pending train-mode forward'):
        tr.backward(tensors, grads, torch.ones_like(feat))
    if kind == 'deit':
        tr.forward(tensors, _x(kind, 2))
        with pytest.raises(NotImplementedError, match='the ViT trainer returns the cls feature only'):
            tr.backward(tensors, grads, torch.ones_like(feat), dtokens=torch.zeros(2, 1, tr.out_dim, device='cuda:0'))


def test_visformer_trainer_takes_a_single_80x80_image():
    """n_img * H3^2 = 25 values per channel at the smallest map: the BatchNorm pre-check does not fire."""
    tr, tensors = _setup('visformer')
    before = {k: v.clone() for k, v in tensors.items() if k.endswith('running_mean')}
    feat = tr.forward(tensors, _x('visformer', 1))
    torch.cuda.synchronize()
    assert feat.shape == (1, 128) and bool(torch.isfinite(feat).all())
    assert any(not torch.equal(before[k], tensors[k]) for k in before)        # live BatchNorm: the running statistics moved


def test_visformer_batchnorm_precheck_comes_before_sizing():
    """img_size 16 and one image: n_img * H3^2 = 1 value per channel.  Refused with nn.BatchNorm2d's sentence before anything is sized - a table
    with a parameter missing (a sizing-pass error) still gets the BatchNorm sentence - and after the image-size check."""
    tr, tensors = _setup('visformer', img_size=16)
    short = {k: v for k, v in tensors.items() if k != MISSING['visformer']}
    rc, msg = _c_forward(tr, 'visformer', short, _x('visformer', 1, img=16), rate=0.5)
    assert rc == _lib.ERR_ARG and msg == BN_TEXT
    with pytest.raises(ValueError, match='Expected more than 1 value per channel'):
        _lib.check(rc)
    rc, msg = _c_forward(tr, 'visformer', short, _x('visformer', 1, img=80))
    assert rc == _lib.ERR_IMG_SIZE and msg == 'Input image size (80*80) does not match model (16*16).'
    rc, msg = _c_forward(tr, 'visformer', short, _x('visformer', 2, img=16))       # two images: the pre-check passes, the sizing pass reports the table
    assert rc == _lib.ERR_KEY and msg == 'missing parameter: ' + MISSING['visformer']


@pytest.mark.parametrize('kind', KINDS)
def test_numerics_refusals(kind):
    from fewshot_vit_amd import engine
    cls = engine.VisformerTrainer if kind == 'visformer' else engine.VitTrainer
    cfg = _model(kind).cfg
    for numerics in ('f16', 'f16x2'):
        with pytest.raises(NotImplementedError, match="the %r numerics mode is an eval mode; train in 'bf16', 'bf16x2' or 'parity'" % numerics):
            cls(cfg, numerics=numerics, device='cuda:0')
    with pytest.raises(ValueError, match=r"unknown numerics mode 'fp8' \(bf16 \| parity\)"):
        cls(cfg, numerics='fp8', device='cuda:0')
    with pytest.raises(ValueError):                     # unknown numerics wins over a non-cuda device, eval-only numerics too
        cls(cfg, numerics='fp8', device='cpu')
    with pytest.raises(NotImplementedError):
        cls(cfg, numerics='f16', device='cpu')
    with pytest.raises(RuntimeError, match=cls.__name__ + r' needs a GPU device \(no CPU fallback\)'):
        cls(cfg, numerics='bf16', device='cpu')
