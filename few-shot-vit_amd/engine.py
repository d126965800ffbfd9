"""Python face of the C-ABI: device-pointer plumbing only (torch owns memory and streams).

`VisformerEngine` wraps one packed `fsvit_visformer` handle; `ops` exposes the operator-level
entry points used by the parity tests.  Every call goes through libfsvit.so — see `_lib.py`.
"""
import ctypes as C
import os
import sys
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib

DTYPES = {'f32': _lib.F32, 'parity': _lib.F32, 'fp32': _lib.F32, 'bf16': _lib.BF16, 'f16': _lib.F16, 'fp16': _lib.F16,
          'bf16x2': _lib.BF16X2, 'f16x2': _lib.F16X2}
TORCH_DTYPE = {_lib.F32: torch.float32, _lib.BF16: torch.bfloat16, _lib.F16: torch.float16, _lib.BF16X2: torch.float32, _lib.F16X2: torch.float32}
EVAL_ONLY = (_lib.F16, _lib.F16X2)        # 'bf16x2' trains too (fp32 storage, every forward / dgrad / wgrad GEMM on two-limb bf16 MFMAs)


# Packed eval engines cache BN-folded copies of the weights.  The HIP optimizers and the HIP trainer write parameters and running
# statistics through raw device pointers, which torch's per-tensor `_version` never sees - so every such write bumps a generation
# PER WRITTEN TENSOR (keyed by its data pointer) and the encoders' engine fingerprints include the generations of their own tensors
# only: a frozen teacher keeps its packed engine while a student trains next to it (offline.py), a stale engine is still impossible.
_tensor_generation = {}


def bump_weight_generation(tensors) -> None:
    """`tensors`: the torch tensors a HIP kernel has just written behind torch's back."""
    for t in tensors:
        if t is not None:
            p = t.data_ptr()
            _tensor_generation[p] = _tensor_generation.get(p, 0) + 1


def weight_generation(t) -> int:
    return _tensor_generation.get(t.data_ptr(), 0)


def weights_fingerprint(module) -> tuple:
    """(data_ptr, torch version, HIP-side generation) of every parameter and buffer of `module`."""
    return tuple((t.data_ptr(), t._version, _tensor_generation.get(t.data_ptr(), 0)) for t in list(module.parameters()) + list(module.buffers()))


def default_numerics() -> str:
    """'bf16' (throughput mode) unless FSVIT_NUMERICS selects another one: 'f16' (fp16 storage + MFMA: same kernels, 0.93 x the rate, 7 x smaller
    logit deviation than bf16, eval only), 'bf16x2' / 'f16x2' (fp32 storage, every GEMM on the 16-bit MFMA with two-limb operands: meets the
    1e-3 logit tolerance at several times the fp32-MFMA rate; 'bf16x2' also trains, 'f16x2' is eval only) or 'parity' / 'f32' (exact-fp32 MFMA)."""
    return os.environ.get('FSVIT_NUMERICS', 'bf16')


# What a drop-in user gets from each mode, measured against the reference's CPU path (tests/test_gpu_visformer.py gates every line
# against the reference goldens, bench.py `modes` / `agreement` re-measure the agreement on 2048 episodes): max |dlogit| on the golden 5-shot
# episode, arg-max agreement with `parity` on the bench episodes, throughput relative to bf16.
NUMERICS_NOTE = {
    'bf16': 'bf16 storage + MFMA: logits within ~5e-2 of the reference (golden 5-shot 4.9e-2, 1-shot 5.0e-2), 98.8 % arg-max agreement; the throughput mode - NOT the '
            '1e-3-grade mode: FSVIT_NUMERICS=f16 (0.93 x the rate, 7 x tighter), bf16x2 (1e-3-grade, 0.23 x) or parity (exact fp32, 0.11 x)',
    'f16': 'fp16 storage + MFMA: logits within ~8e-3 of the reference (golden 5-shot 7.2e-3), 99.85 % arg-max agreement, 0.93 x the bf16 rate (its GELUs stay on the VALU); eval only',
    'bf16x2': 'fp32 storage, two-limb bf16 MFMA: logits within 1.5e-4 of the reference (meets the 1e-3 tolerance), 0.24 x the bf16 rate; also trains',
    'f16x2': 'fp32 storage, two-limb fp16 MFMA: logits within 2.2e-5 of the reference (meets the 1e-3 tolerance), 0.24 x the bf16 rate; eval only',
    'parity': 'exact-fp32 MFMA: logits within 1e-3 of the reference (the parity mode), 0.12 x the bf16 rate',
    'f32': 'exact-fp32 MFMA: logits within 1e-3 of the reference (the parity mode), 0.12 x the bf16 rate',
}
_numerics_logged = set()


def log_numerics_once(numerics: str, what: str) -> None:
    """One line per process and (mode, engine kind): which numerics mode an engine was built with and what that means for the logits - so that the
    5e-2 throughput mode is never handed to a drop-in user silently.  FSVIT_QUIET=1 silences it."""
    key = (numerics, what)
    if key in _numerics_logged or os.environ.get('FSVIT_QUIET') == '1':
        return
    _numerics_logged.add(key)
    src = 'FSVIT_NUMERICS' if os.environ.get('FSVIT_NUMERICS') == numerics else 'default / encoder_args'
    sys.stderr.write('fsvit: %s built in numerics mode %r (%s) - %s\n' % (what, numerics, src, NUMERICS_NOTE.get(numerics, '')))


def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError('fsvit kernels run on an MI355X only: tensor is on %s (no CPU fallback)' % t.device)


class _EncoderEngine:
    """One packed eval-mode encoder on one GPU (shared plumbing of the Visformer and ViT handles)."""

    _fn = {}          # C entry points: create / destroy / out_dim / workspace_bytes / forward

    def _make_cfg(self, cfg: dict):
        raise NotImplementedError

    def __init__(self, cfg: dict, state_dict: Dict[str, torch.Tensor], numerics: str = None, device=None,
                 chunk_images: int = None):
        self.lib = _lib.load()
        numerics = numerics or default_numerics()
        if numerics not in DTYPES:
            raise ValueError(f'unknown numerics mode {numerics!r} (bf16 | f16 | bf16x2 | f16x2 | parity)')
        self.dtype = DTYPES[numerics]
        self.numerics = numerics
        self.device = torch.device(device if device is not None else 'cuda')
        if self.device.type != 'cuda':
            raise RuntimeError(f'{type(self).__name__} needs a GPU device (no CPU fallback)')
        log_numerics_once(numerics, type(self).__name__)
        self.chunk_images = int(chunk_images or os.environ.get('FSVIT_CHUNK', self._default_chunk))
        self._chunk_given = bool(chunk_images or os.environ.get('FSVIT_CHUNK'))
        c = self._make_cfg(cfg)
        self.img_size = cfg['img_size']
        keep, arr = [], (_lib.Tensor * len(state_dict))()
        n = 0
        for k, v in state_dict.items():
            if k.endswith('num_batches_tracked'):
                continue
            a = np.ascontiguousarray(v.detach().to('cpu', torch.float32).numpy())
            if self.dtype in (_lib.F16, _lib.F16X2) and a.size and not np.all(np.abs(a) < 65504.0):
                # fp16 limbs top out at 65504 (hi = inf, lo = NaN beyond) and go subnormal below 6e-5: the 'f16' / 'f16x2' modes assume
                # BatchNorm / LayerNorm-scaled networks (weights O(1)); anything else belongs in 'bf16x2' (8-bit exponent, no range limit)
                raise ValueError(f"fsvit: {k} holds values outside the fp16 range; use numerics='bf16x2' (or 'parity') for this checkpoint")
            keep.append(a)
            arr[n].name = k.encode()
            arr[n].data = a.ctypes.data_as(C.POINTER(C.c_float))
            arr[n].ndim = a.ndim
            for i, sdim in enumerate(a.shape):
                arr[n].shape[i] = sdim
            n += 1
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(getattr(self.lib, self._fn['create'])(C.byref(c), arr, n, self.dtype, C.byref(h)))
        self.h = h
        self.out_dim = getattr(self.lib, self._fn['out_dim'])(h)
        self._ws = None
        self._taps = {}

    def __del__(self):
        h, self.h = getattr(self, 'h', None), None
        if h:
            try:
                getattr(self.lib, self._fn['destroy'])(h)
            except Exception:       # interpreter shutdown
                pass

    def workspace(self, n_img: int) -> torch.Tensor:
        chunk = max(1, min(n_img, self.chunk_images))
        ws_bytes = getattr(self.lib, self._fn['workspace_bytes'])
        need = ws_bytes(self.h, chunk)
        if self._ws is None or self._ws.numel() < need:
            if not self._chunk_given:
                # the default chunk (the benched 12 800 images) shrinks on a device that cannot spare half of its free memory for the workspace
                free = torch.cuda.mem_get_info(self.device)[0] + (self._ws.numel() if self._ws is not None else 0)
                while need > 0.5 * free and chunk > 100:
                    chunk //= 2
                    need = ws_bytes(self.h, chunk)
                    self.chunk_images = chunk                # (the C side takes the largest chunk that fits the workspace it is handed)
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def set_tap(self, name: str, shape) -> torch.Tensor:
        t = torch.zeros(shape, dtype=TORCH_DTYPE[self.dtype], device=self.device)
        _lib.check(self.lib.fsvit_encoder_set_tap(self.h, name.encode(), _ptr(t), t.numel() * t.element_size()))
        self._taps[name] = t
        return t

    def profile_begin(self):
        _lib.check(self.lib.fsvit_encoder_profile_begin(self.h))

    def profile_end(self):
        """-> list of dict(layer, kernel, launches, flops, ms): HIP-event time of every launch since
        profile_begin, summed per (layer, kernel template instantiation)."""
        recs = (_lib.ProfRec * 256)()
        n = C.c_int(0)
        _lib.check(self.lib.fsvit_encoder_profile_end(self.h, recs, 256, C.byref(n)))
        return [dict(layer=recs[i].layer.decode(), kernel=self.lib.fsvit_kernel_name(recs[i].kernel_id, self.dtype).decode(),
                     launches=recs[i].launches, flops=recs[i].flops, ms=recs[i].ms) for i in range(n.value)]

    def forward(self, x: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
        """x [B,3,H,W] fp32 cuda -> features [B,out_dim] fp32."""
        _require_cuda(x)
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError('expected [B,3,H,W] input')
        x = x.contiguous().float()
        B = x.shape[0]
        if out is None:
            out = torch.empty(B, self.out_dim, dtype=torch.float32, device=x.device)
        if B == 0:
            return out
        ws = self.workspace(B)
        with torch.cuda.device(x.device):
            _lib.check(getattr(self.lib, self._fn['forward'])(self.h, _ptr(x), B, x.shape[2], x.shape[3], _ptr(out), _ptr(ws),
                                                             ws.numel(), _stream_ptr(x.device)))
        return out

    def last_tokens(self, n_img: int, tokens_per_image: int) -> torch.Tensor:
        """Post-norm token map [n_img, T, out_dim] fp32 of the images of the immediately preceding `forward` call (Visformer only; the
        call must have fitted one chunk) - the `x` of the distillation encoder's `return x, pooled`."""
        out = torch.empty(n_img, tokens_per_image, self.out_dim, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fsvit_visformer_last_tokens(self.h, _ptr(self._ws), self._ws.numel(), n_img, _ptr(out), _stream_ptr(self.device)))
        return out

    def meta_baseline_forward(self, x_shot, x_query, temp: float, method: str = 'cos', want_stats=False):
        """x_shot [E,way,shot,3,H,W], x_query [E,Q,3,H,W] -> logits [E,Q,way] (+ per-episode acc, loss)."""
        _require_cuda(x_shot, x_query)
        E, way, shot = x_shot.shape[:3]
        Q = x_query.shape[1]
        x_shot = x_shot.contiguous().float()
        x_query = x_query.contiguous().float()
        dev = x_shot.device
        feat = torch.empty(E * way * shot + E * Q, self.out_dim, dtype=torch.float32, device=dev)
        logits = torch.empty(E, Q, way, dtype=torch.float32, device=dev)
        acc = torch.empty(E, dtype=torch.float32, device=dev)
        loss = torch.empty(E, dtype=torch.float32, device=dev)
        ws = self.workspace(E * way * shot + E * Q)      # shots + queries go through the encoder in one pass when they fit one chunk
        m = {'cos': _lib.HEAD_COS, 'sqr': _lib.HEAD_SQR, 'dot': _lib.HEAD_DOT}[method]
        with torch.cuda.device(dev):
            _lib.check(self.lib.fsvit_meta_baseline_forward(
                self.h, _ptr(x_shot), _ptr(x_query), E, way, shot, Q, x_shot.shape[-2], x_shot.shape[-1], float(temp), m,
                _ptr(logits), _ptr(acc), _ptr(loss), _ptr(feat), _ptr(ws), ws.numel(), _stream_ptr(dev)))
        if want_stats:
            return logits, acc, loss
        return logits


class VisformerEngine(_EncoderEngine):
    """cfg: dict(img_size, init_channels, embed_dim, depth, num_heads, mlp_ratio, group[, bn_eps]);
    state_dict: encoder-relative reference keys."""
    _fn = dict(create='fsvit_visformer_create', destroy='fsvit_visformer_destroy', out_dim='fsvit_visformer_out_dim',
               workspace_bytes='fsvit_visformer_workspace_bytes', forward='fsvit_visformer_forward')
    _default_chunk = 12800      # the benched launch size (round 6: was 3200 - a drop-in user ran the persistent kernels at a quarter of their launch size)

    def _make_cfg(self, cfg):
        c = _lib.VisformerCfg()
        c.img_size, c.init_channels, c.embed_dim = cfg['img_size'], cfg['init_channels'], cfg['embed_dim']
        for i in range(3):
            c.depth[i] = cfg['depth'][i]
        c.num_heads, c.mlp_ratio, c.group = cfg['num_heads'], cfg.get('mlp_ratio', 4.0), cfg.get('group', 8)
        c.bn_eps = cfg.get('bn_eps', 1e-5)
        return c


class _Trainer:
    """One train-mode encoder handle on one GPU (shared plumbing of the Visformer and ViT trainers): forward with saved activations, backward to
    all parameter gradients.  Parameters are read from (and running stats are updated in) the caller's own fp32 cuda tensors every call -
    nothing is packed ahead of time."""

    _fn = {}          # C entry points: create / destroy / workspace_bytes / forward / backward [/ token_grad: the handle takes a token-map gradient]
    _dfeat_optional = False     # the backward accepts dfeat=None next to a token-map gradient

    def _make_cfg(self, cfg: dict):
        raise NotImplementedError

    def _out_dim(self, cfg: dict) -> int:
        raise NotImplementedError

    def __init__(self, cfg: dict, numerics: str = None, device=None):
        self.lib = _lib.load()
        numerics = numerics or default_numerics()
        if numerics not in DTYPES:
            raise ValueError(f'unknown numerics mode {numerics!r} (bf16 | parity)')
        if DTYPES[numerics] in EVAL_ONLY:
            raise NotImplementedError(f"fsvit: the {numerics!r} numerics mode is an eval mode; train in 'bf16', 'bf16x2' or 'parity'")
        self.dtype = DTYPES[numerics]
        log_numerics_once(numerics, type(self).__name__)
        self.device = torch.device(device if device is not None else 'cuda')
        if self.device.type != 'cuda':
            raise RuntimeError(f'{type(self).__name__} needs a GPU device (no CPU fallback)')
        self.cfg = dict(cfg)
        self.out_dim = self._out_dim(cfg)
        c = self._make_cfg(cfg)
        h = C.c_void_p()
        _lib.check(getattr(self.lib, self._fn['create'])(C.byref(c), self.dtype, C.byref(h)))
        self.h = h
        self._ws = None
        self._keep = None
        self.generation = 0        # bumped by every forward: the ONE set of saved activations belongs to the latest forward only

    def __del__(self):
        h, self.h = getattr(self, 'h', None), None
        if h:
            try:
                getattr(self.lib, self._fn['destroy'])(h)
            except Exception:
                pass

    @staticmethod
    def _table(tensors: Dict[str, torch.Tensor], grads: Optional[Dict[str, torch.Tensor]]):
        arr = (_lib.Param * len(tensors))()
        keep = []
        for i, (k, v) in enumerate(tensors.items()):
            if v.dtype != torch.float32 or not v.is_contiguous() or not v.is_cuda:
                raise ValueError(f'{k}: training tensors must be contiguous fp32 cuda tensors')
            kb = k.encode()
            keep.append(kb)
            arr[i].name = kb
            arr[i].data = v.data_ptr()
            g = None if grads is None else grads.get(k)
            arr[i].grad = g.data_ptr() if g is not None else None
            arr[i].numel = v.numel()
        return arr, keep

    def forward(self, tensors: Dict[str, torch.Tensor], x: torch.Tensor, drop_path_rate: float = 0.0,
                masks: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tensors: encoder-relative name -> fp32 cuda tensor (parameters AND running stats);
        x [B,3,H,W]; masks [n_droppath_calls, B] of 0/1.  Returns feat [B,out_dim]; activations stay in the workspace."""
        _require_cuda(x)
        x = x.contiguous().float()
        B = x.shape[0]
        arr, keep = self._table(tensors, None)
        need = getattr(self.lib, self._fn['workspace_bytes'])(self.h, arr, len(tensors), B, float(drop_path_rate))
        if need == 0:
            _lib.check(_lib.ERR_KEY if 'missing' in self.lib.fsvit_last_error().decode() else _lib.ERR_ARG)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        feat = torch.empty(B, self.out_dim, dtype=torch.float32, device=x.device)
        if masks is not None:
            masks = masks.contiguous().float()
        with torch.cuda.device(x.device):
            _lib.check(getattr(self.lib, self._fn['forward'])(self.h, arr, len(tensors), _ptr(x), B, x.shape[2], x.shape[3],
                                                             float(drop_path_rate), _ptr(masks), _ptr(feat), _ptr(self._ws),
                                                             self._ws.numel(), _stream_ptr(x.device)))
        self._keep = (x, masks)
        self.generation += 1
        # BatchNorm running statistics were updated in place (none in a ViT's table)
        bump_weight_generation(v for k, v in tensors.items() if k.endswith(('running_mean', 'running_var')))
        return feat

    def backward(self, tensors: Dict[str, torch.Tensor], grads: Dict[str, torch.Tensor], dfeat: torch.Tensor, dtokens: torch.Tensor = None):
        """Overwrites grads[name] (same shapes as tensors[name]) from dfeat [B,out_dim] (+ dtokens [B,T,out_dim], the gradient of the
        token map handed out by `tokens`: Visformer and LV-ViT; the LV-ViT trainer takes dfeat=None next to it)."""
        _require_cuda(dfeat, dtokens)
        if self._keep is None:
            raise RuntimeError('fsvit: backward without a pending train-mode forward (the saved activations were already consumed)')
        if dtokens is not None and 'token_grad' not in self._fn:
            raise NotImplementedError('fsvit: the ViT trainer returns the cls feature only')
        if dfeat is None and (dtokens is None or not self._dfeat_optional):
            raise ValueError('fsvit: backward needs dfeat')
        dfeat = dfeat.contiguous().float() if dfeat is not None else None
        arr, keep = self._table(tensors, grads)
        if dtokens is not None:
            dtokens = dtokens.contiguous().float()
            _lib.check(getattr(self.lib, self._fn['token_grad'])(self.h, _ptr(dtokens)))
        dev = dfeat.device if dfeat is not None else dtokens.device
        with torch.cuda.device(dev):
            _lib.check(getattr(self.lib, self._fn['backward'])(self.h, arr, len(tensors), _ptr(dfeat), _stream_ptr(dev)))
        self._keep = None


class VisformerTrainer(_Trainer):
    """Train-mode Visformer (meta-tuning step, train_meta.py:161-177): batch-statistics BN + DropPath."""
    _fn = dict(create='fsvit_visformer_trainer_create', destroy='fsvit_visformer_trainer_destroy', workspace_bytes='fsvit_visformer_trainer_workspace_bytes',
               forward='fsvit_visformer_train_forward', backward='fsvit_visformer_train_backward', token_grad='fsvit_visformer_train_set_token_grad')

    def _make_cfg(self, cfg):
        return VisformerEngine._make_cfg(None, cfg)

    def _out_dim(self, cfg):
        return cfg['embed_dim'] * 2

    def set_freeze_bn(self, on: bool):
        """BatchNorm layers in eval mode inside the step (utils.freeze_bn): the running statistics normalise and are not updated; gamma / beta
        still receive gradients, dz = gamma * invstd * dy."""
        _lib.check(self.lib.fsvit_visformer_trainer_set_freeze_bn(self.h, int(bool(on))))

    def droppath_keep(self, rate: float) -> list:
        """Keep-probability of every DropPath call with a non-zero rate, in call order (a stage-1 block calls once, an attention block twice;
        per-block rates linspace(0, rate, depth), visformer.py:312)."""
        d = self.cfg['depth']
        return [1.0 - r for b, r in enumerate(torch.linspace(0, rate, sum(d)).tolist()) if r > 0 for _ in range(1 if b < d[0] else 2)]

    def n_droppath_calls(self, rate: float) -> int:
        return len(self.droppath_keep(rate))

    def tokens(self, B: int, tokens_per_image: int) -> torch.Tensor:
        """Post-norm token map [B, T, out_dim] fp32 of the last forward (sun_meta_training/models/visformer.py:464)."""
        out = torch.empty(B, tokens_per_image, self.out_dim, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fsvit_visformer_train_tokens(self.h, _ptr(out), _stream_ptr(self.device)))
        return out


class VitTrainer(_Trainer):
    """Train-mode ViT / DeiT (deit.py:61-78, 139-218): LayerNorm row statistics + DropPath - the ViT counterpart of VisformerTrainer."""
    _fn = dict(create='fsvit_vit_trainer_create', destroy='fsvit_vit_trainer_destroy', workspace_bytes='fsvit_vit_trainer_workspace_bytes',
               forward='fsvit_vit_train_forward', backward='fsvit_vit_train_backward')

    def _make_cfg(self, cfg):
        return VitEngine._make_cfg(None, cfg)

    def _out_dim(self, cfg):
        return cfg['embed_dim']

    def n_droppath_calls(self, rate: float) -> int:
        return int(self.lib.fsvit_vit_trainer_droppath_calls(self.h, float(rate)))


class LvvitTrainer(_Trainer):
    """Train-mode LV-ViT (lvvit.py:277-317 stem with batch-statistics BatchNorm, :134-155 blocks with the 1 / skip_lam branch scale, DropPath)."""
    _fn = dict(create='fsvit_lvvit_trainer_create', destroy='fsvit_lvvit_trainer_destroy', workspace_bytes='fsvit_lvvit_trainer_workspace_bytes',
               forward='fsvit_lvvit_train_forward', backward='fsvit_lvvit_train_backward', token_grad='fsvit_lvvit_train_set_token_grad')
    _dfeat_optional = True      # with a token-map gradient the backward takes "no gradient on the cls feature" as a null pointer

    def _make_cfg(self, cfg):
        return LvvitEngine._make_cfg(None, cfg)

    def _out_dim(self, cfg):
        return cfg['embed_dim']

    def tokens(self, B: int, tokens_per_image: int = 25) -> torch.Tensor:
        """The final norm's patch rows [B, 25, out_dim] fp32 of the pending forward (sun_meta_training/models/lvvit.py:552), token-major."""
        out = torch.empty(B, tokens_per_image, self.out_dim, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fsvit_lvvit_train_tokens(self.h, _ptr(out), _stream_ptr(self.device)))
        return out

    def set_freeze_bn(self, on: bool):
        """The stem's BatchNorm layers in eval mode inside the step (utils.freeze_bn), as VisformerTrainer.set_freeze_bn."""
        _lib.check(self.lib.fsvit_lvvit_trainer_set_freeze_bn(self.h, int(bool(on))))

    def droppath_keep(self, rate: float) -> list:
        """Keep-probability of every DropPath call with a non-zero rate, in call order: two calls per block, rates get_dpr(rate, depth, 'linear')
        (lvvit.py:401-404)."""
        return [1.0 - r for r in torch.linspace(0, rate, self.cfg['depth']).tolist() if r > 0 for _ in range(2)]

    def n_droppath_calls(self, rate: float) -> int:
        return int(self.lib.fsvit_lvvit_trainer_droppath_calls(self.h, float(rate)))


class VitEngine(_EncoderEngine):
    """cfg: dict(img_size, patch_size, embed_dim, depth, num_heads[, mlp_ratio, ln_eps]) (deit.py:142-144)."""
    _fn = dict(create='fsvit_vit_create', destroy='fsvit_vit_destroy', out_dim='fsvit_vit_out_dim',
               workspace_bytes='fsvit_vit_workspace_bytes', forward='fsvit_vit_forward')
    _default_chunk = 12800      # the benched launch size (round 6: was 400); shrinks to half of the free device memory in workspace()

    def _make_cfg(self, cfg):
        c = _lib.VitCfg()
        c.img_size, c.patch_size, c.embed_dim, c.depth = cfg['img_size'], cfg['patch_size'], cfg['embed_dim'], cfg['depth']
        c.num_heads, c.mlp_ratio, c.ln_eps = cfg['num_heads'], cfg.get('mlp_ratio', 4.0), cfg.get('ln_eps', 1e-6)
        return c


class LvvitEngine(_EncoderEngine):
    """cfg: dict(img_size, stem_channels, embed_dim, depth, num_heads[, mlp_ratio, skip_lam, ln_eps, bn_eps]) (lvvit.py:583-587);
    the eval engine (LvvitTrainer trains)."""
    _fn = dict(create='fsvit_lvvit_create', destroy='fsvit_lvvit_destroy', out_dim='fsvit_lvvit_out_dim',
               workspace_bytes='fsvit_lvvit_workspace_bytes', forward='fsvit_lvvit_forward')
    _default_chunk = 12800      # as the other encoders; shrinks to half of the free device memory in workspace()

    def forward_map(self, x: torch.Tensor):
        """x [B,3,80,80] fp32 cuda -> (tokens [B,25,out_dim], feat [B,out_dim]) fp32: the final norm's patch rows, token-major, next to the cls feature
        (sun_meta_training/models/lvvit.py:552); feat holds the bits `forward` gives.  Chunked like `forward`: any B."""
        _require_cuda(x)
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError('expected [B,3,H,W] input')
        x = x.contiguous().float()
        B = x.shape[0]
        feat = torch.empty(B, self.out_dim, dtype=torch.float32, device=x.device)
        tokens = torch.empty(B, 25, self.out_dim, dtype=torch.float32, device=x.device)
        if B == 0:
            return tokens, feat
        ws = self.workspace(B)
        with torch.cuda.device(x.device):
            _lib.check(self.lib.fsvit_lvvit_forward_map(self.h, _ptr(x), B, x.shape[2], x.shape[3], _ptr(feat), _ptr(tokens), _ptr(ws), ws.numel(),
                                                        _stream_ptr(x.device)))
        return tokens, feat

    def _make_cfg(self, cfg):
        c = _lib.LvvitCfg()
        c.img_size, c.stem_channels, c.embed_dim, c.depth = cfg['img_size'], cfg['stem_channels'], cfg['embed_dim'], cfg['depth']
        c.num_heads, c.mlp_ratio, c.skip_lam = cfg['num_heads'], cfg.get('mlp_ratio', 3.0), cfg.get('skip_lam', 2.0)
        c.ln_eps, c.bn_eps = cfg.get('ln_eps', 1e-5), cfg.get('bn_eps', 1e-5)
        return c


class ops:
    """Operator-level entry points (storage dtype follows the input tensors: fp32, bf16 or fp16; the fused row operators take the two 16-bit types
    only, activations and weights of the same one)."""

    @staticmethod
    def _dt(t):
        if t.dtype == torch.float32:
            return _lib.F32
        if t.dtype == torch.bfloat16:
            return _lib.BF16
        if t.dtype == torch.float16:
            return _lib.F16
        raise TypeError(t.dtype)

    @staticmethod
    def _dt16(x, *weights):
        """Storage dtype of a fused row operator: x bf16 or fp16 (TypeError otherwise), every 16-bit tensor in `weights` of the same type."""
        if x.dtype not in (torch.bfloat16, torch.float16):
            raise TypeError(f'16-bit activations only (torch.bfloat16 / torch.float16), got {x.dtype}')
        for w in weights:
            if w is not None and w.dtype != x.dtype:
                raise TypeError(f'activations are {x.dtype} but a weight / activation operand is {w.dtype}')
        return ops._dt(x)

    @staticmethod
    def _out(out, x, N):
        """The [M][N] result of a row operator on x [M][.]: a fresh tensor, or the caller's `out` (contiguous, x's dtype and device; `out is x` runs the
        Mlp operators in place, as the engines do)."""
        if out is None:
            return torch.empty(x.shape[0], N, device=x.device, dtype=x.dtype)
        if out.dtype != x.dtype or out.device != x.device or tuple(out.shape) != (x.shape[0], N) or not out.is_contiguous():
            raise ValueError(f'out must be a contiguous [{x.shape[0]}, {N}] {x.dtype} tensor on {x.device}')
        return out

    @staticmethod
    def x2_limbs(w: torch.Tensor, numerics: str) -> torch.Tensor:
        """fp32 weights -> the two-limb words of the 'bf16x2' / 'f16x2' GEMM (upper half hi = w rounded to the 16-bit type, lower half
        lo = (w - hi) rounded to it), as a float32-typed tensor of the same shape (fsvit.h: FSVIT_BF16X2 / FSVIT_F16X2)."""
        t16 = torch.bfloat16 if numerics == 'bf16x2' else torch.float16
        w = w.float()
        hi = w.to(t16)
        lo = (w - hi.float()).to(t16)
        if not (torch.isfinite(hi.float()).all() and torch.isfinite(lo.float()).all()):
            raise ValueError("x2_limbs: values outside the 16-bit type's range (fp16 limbs: |w| < 65504); use 'bf16x2'")
        words = (hi.view(torch.int16).to(torch.int32) << 16) | (lo.view(torch.int16).to(torch.int32) & 0xffff)
        return words.view(torch.float32)

    @staticmethod
    def conv_gemm(x, w, bias, res, pos, B, H, W, Cin, KH, KW, stride, pad, N, groups, act, res_first, x_cstride=None, numerics=None):
        """x NHWC [B,H,W,x_cstride]; w [groups][N][Kw] packed; returns y NHWC [B,OH,OW,groups*N].  numerics 'bf16x2' / 'f16x2': x fp32,
        w = ops.x2_limbs(packed fp32 weights)."""
        _require_cuda(x, w)
        lib = _lib.load()
        OH = (H + 2 * pad - KH) // stride + 1
        OW = (W + 2 * pad - KW) // stride + 1
        x_cstride = x_cstride or x.shape[-1]
        y = torch.empty(B, OH, OW, groups * N, dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.fsvit_conv_gemm(_ptr(x), _ptr(w), _ptr(bias), _ptr(res), _ptr(pos), _ptr(y), B, H, W, Cin, x_cstride,
                                           KH, KW, stride, pad, N, groups * N, w.shape[-1], groups, act, int(res_first),
                                           DTYPES[numerics] if numerics else ops._dt(x), _stream_ptr(x.device)))
        return y

    @staticmethod
    def gconv3x3(x, w_packed):
        """x NHWC [B,H,W,256] (bf16 / fp16), w_packed [256][Kw] -> the grouped 3x3 convolution (8 groups of 32 -> 32) of the training step."""
        _require_cuda(x, w_packed)
        B, H, W, _ = x.shape
        y = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().fsvit_gconv3x3(_ptr(x), _ptr(w_packed), w_packed.shape[-1], _ptr(y), B, H, W, ops._dt(x), _stream_ptr(x.device)))
        return y

    @staticmethod
    def conv_stem_tail(x, w, bias, pos, x2, K2, numerics=None):
        """Fused stem tail: x NHWC [B,H,W,Cin], w [N][Kw] (conv3 taps | one tail K slice), x2 [B*H*W][x2_cstride] im2col rows,
        pos [(H/2)*(W/2)][N] fp32 -> y NHWC [B,H/2,W/2,N].  numerics 'bf16x2' / 'f16x2': x / x2 fp32, w = ops.x2_limbs(packed fp32 weights)."""
        _require_cuda(x, w, x2, pos)
        lib = _lib.load()
        B, H, W, Cin = x.shape
        N = w.shape[0]
        y = torch.empty(B, H // 2, W // 2, N, dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.fsvit_conv_stem_tail(_ptr(x), _ptr(w), _ptr(bias), _ptr(pos), _ptr(x2), x2.shape[-1], int(K2), _ptr(y), B, H, W, Cin, N,
                                                w.shape[-1], DTYPES[numerics] if numerics else ops._dt(x), _stream_ptr(x.device)))
        return y

    @staticmethod
    def stem96_conv(x, w_img, bias, x2=None, K2=32):
        """LV-ViT stem conv2 (x2 None) or conv3 + downsample tail + LeakyReLU + MaxPool2d(2) on the dedicated kernel (fsvit_stem96_conv): x NHWC
        [B,H,40,96] bf16 / f16, w_img the 128-channel image [128][9*128 (+64)] (k = tap*128 + c), bias [96] fp32 -> y NHWC, 96 channels."""
        _require_cuda(x, w_img)
        B, H, W, _ = x.shape
        pool = x2 is not None
        y = torch.empty(B, H // 2 if pool else H, W // 2 if pool else W, 96, dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().fsvit_stem96_conv(_ptr(x), _ptr(w_img), _ptr(bias), _ptr(x2), x2.shape[-1] if pool else 0, int(K2) if pool else 0,
                                                     _ptr(y), B, H, W, int(pool), ops._dt(x), _stream_ptr(x.device)))
        return y

    @staticmethod
    def stage1_block(x, w1, b1, w2, w3):
        """x NHWC [B,20,20,128] bf16; packed w1 [256][128], w2 [8][32][320], w3 [128][256] bf16; b1 [256] fp32."""
        _require_cuda(x, w1, w2, w3, b1)
        lib = _lib.load()
        y = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(lib.fsvit_stage1_block(_ptr(x), _ptr(y), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(w3), x.shape[0], _stream_ptr(x.device)))
        return y

    @staticmethod
    def stage1_block_hw(x, w1, b1, w2, w3):
        """x NHWC [B,H,W,128] (bf16 / fp16), H = W in 4 .. 20: the ring kernel of the stage-1 block (fsvit_stage1_block_hw)."""
        _require_cuda(x, w1, w2, w3, b1)
        lib = _lib.load()
        y = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(lib.fsvit_stage1_block_hw(_ptr(x), _ptr(y), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(w3), x.shape[0], x.shape[1], x.shape[2], ops._dt(x),
                                                 _stream_ptr(x.device)))
        return y

    @staticmethod
    def stage1_block_eval(x, w1, b1, w2, w3, prescaled):
        """stage1_block_hw as the engines launch it (fsvit_op_stage1_block_eval): prescaled = True runs stage1_w4_kernel<true, true> on the 8 x W3 image
        built by the engines' own prescale launch, False the <true, false> instantiation on W3."""
        _require_cuda(x, w1, w2, w3, b1)
        dt = ops._dt16(x, w1, w2, w3)
        y = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().fsvit_op_stage1_block_eval(_ptr(x), _ptr(y), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(w3), x.shape[0], x.shape[1], x.shape[2], dt,
                                                              int(bool(prescaled)), _stream_ptr(x.device)))
        return y

    @staticmethod
    def conv_eval(y, numerics=None, **fields):
        """fsvit_op_conv_eval: one launch through the evaluation dispatcher.  `fields` are those of fsvit_conv_eval_args (fsvit.h) - tensors (or None) for the
        pointer fields, ints for the rest, everything left out 0 / NULL; y is the caller's output buffer (its dtype is the storage type unless `numerics`
        names a two-limb mode).  -> (route, stats_rows)."""
        _require_cuda(y)
        a = _lib.ConvEvalArgs()
        names = {n for n, _ in _lib.ConvEvalArgs._fields_}
        fields = dict(fields, y=y)
        for k, v in fields.items():
            if k not in names:
                raise TypeError(f'conv_eval: unknown field {k}')
            if torch.is_tensor(v):
                _require_cuda(v)
                v = v.data_ptr()
            setattr(a, k, v)
        route, rows = C.c_int(-1), C.c_int(-1)
        with torch.cuda.device(y.device):
            _lib.check(_lib.load().fsvit_op_conv_eval(C.byref(a), DTYPES[numerics] if numerics else ops._dt(y), C.byref(route), C.byref(rows),
                                                      _stream_ptr(y.device)))
        return route.value, rows.value

    # ---- distillation head (sun_meta_training/offline.py): fp32, token-major rows
    @staticmethod
    def linear(x, w, b=None):
        """x [M, K] fp32, w [N, K], b [N] or None -> x w^T + b (classifier.py:27-34)."""
        _require_cuda(x, w)
        x, w = x.contiguous().float(), w.contiguous().float()
        y = torch.empty(x.shape[0], w.shape[0], dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().fsvit_linear_forward(_ptr(x), _ptr(w), _ptr(None if b is None else b.contiguous().float()), _ptr(y),
                                                        x.shape[0], w.shape[0], x.shape[1], _stream_ptr(x.device)))
        return y

    @staticmethod
    def linear_backward(dy, x, w, need_dx=True, need_dw=True, need_db=True):
        _require_cuda(dy, x, w)
        dy, x, w = dy.contiguous().float(), x.contiguous().float(), w.contiguous().float()
        dx = torch.empty_like(x) if need_dx else None
        dw = torch.empty_like(w) if need_dw else None
        db = torch.empty(w.shape[0], dtype=torch.float32, device=x.device) if (need_db and need_dw) else None
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().fsvit_linear_backward(_ptr(dy), _ptr(x), _ptr(w), _ptr(dx), 0, _ptr(dw), _ptr(db), x.shape[0], w.shape[0], x.shape[1],
                                                         _stream_ptr(x.device)))
        return dx, dw, db

    @staticmethod
    def token_softlabel(teacher_logits, k=3, bp=10, smoothing=0.1):
        """teacher token logits [B, T, C] -> soft labels [B*T, C+1] (offline.py:57-76)."""
        _require_cuda(teacher_logits)
        lt = teacher_logits.contiguous().float()
        B, T, Cc = lt.shape
        soft = torch.empty(B * T, Cc + 1, dtype=torch.float32, device=lt.device)
        with torch.cuda.device(lt.device):
            _lib.check(_lib.load().fsvit_token_softlabel(_ptr(lt), _ptr(soft), B, T, Cc, int(k), int(bp), float(smoothing), _stream_ptr(lt.device)))
        return soft

    @staticmethod
    def soft_target_ce(logits, target, grad_scale=None):
        """-> (row_loss [R], dlogits [R, C] = grad_scale * d(sum of row losses)/dlogits, or None)."""
        _require_cuda(logits, target)
        z, t = logits.contiguous().float(), target.contiguous().float()
        R, Cc = z.shape
        row = torch.empty(R, dtype=torch.float32, device=z.device)
        dz = torch.empty_like(z) if grad_scale is not None else None
        with torch.cuda.device(z.device):
            _lib.check(_lib.load().fsvit_soft_target_ce(_ptr(z), _ptr(t), _ptr(row), _ptr(dz), R, Cc, float(grad_scale or 0.0), _stream_ptr(z.device)))
        return row, dz

    @staticmethod
    def row_normalize(x):
        """F.normalize(x, dim=-1) of a [R, D] fp32 matrix -> (y, inv_norm [R])."""
        _require_cuda(x)
        x = x.contiguous().float()
        y, inv = torch.empty_like(x), torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().fsvit_row_normalize(_ptr(x), _ptr(y), _ptr(inv), x.shape[0], x.shape[1], _stream_ptr(x.device)))
        return y, inv

    @staticmethod
    def row_normalize_backward(y, inv, dy):
        _require_cuda(y, inv, dy)
        dy = dy.contiguous().float()
        dx = torch.empty_like(y)
        with torch.cuda.device(y.device):
            _lib.check(_lib.load().fsvit_row_normalize_backward(_ptr(y), _ptr(inv), _ptr(dy), _ptr(dx), y.shape[0], y.shape[1], _stream_ptr(y.device)))
        return dx

    @staticmethod
    def adamw_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step):
        _require_cuda(p, g, m, v)
        bump_weight_generation((p,))
        with torch.cuda.device(p.device):
            _lib.check(_lib.load().fsvit_adamw_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
                                                    float(weight_decay), int(step), _stream_ptr(p.device)))

    @staticmethod
    def adamw_step_multi(params, grads, ms, vs, lr, beta1, beta2, eps, weight_decay, step):
        """One launch for a list of fp32 tensors at the same update number (fsvit_adamw_step_multi).  -> the device table (ops._ptr_table)."""
        if not params:
            return
        _require_cuda(*params)
        lib = _lib.load()
        bump_weight_generation(params)
        dev = params[0].device
        rows = tuple((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()) for p, g, m, v in zip(params, grads, ms, vs))
        table = ops._ptr_table('adamw', dev, rows)
        with torch.cuda.device(dev):
            _lib.check(lib.fsvit_adamw_step_multi(_ptr(table), len(rows), max(r[4] for r in rows), float(lr), float(beta1), float(beta2), float(eps),
                                                  float(weight_decay), int(step), _stream_ptr(dev)))
        return table

    @staticmethod
    def proj_mlp_rows(x, ctx, wp, w1, b1, w2, b2=None, out=None):
        """x [M][C], ctx [M][KC] bf16, wp [C][KpW]: x1 = x + ctx wp^T; y = x1 + W2 GELU(W1 x1 + b1) + b2  ((C, KC) = (256, 288) | (512, 576))."""
        _require_cuda(x, ctx, wp, w1, w2)
        dt = ops._dt16(x, ctx, wp, w1, w2)
        lib = _lib.load()
        y = ops._out(out, x, x.shape[1])
        with torch.cuda.device(x.device):
            _lib.check(lib.fsvit_proj_mlp_rows_dt(_ptr(x), _ptr(y), _ptr(ctx), _ptr(wp), wp.shape[-1], ctx.shape[1], _ptr(w1), w1.shape[-1], _ptr(b1),
                                                  _ptr(w2), w2.shape[-1], _ptr(b2), x.shape[0], x.shape[1], w1.shape[0], dt, _stream_ptr(x.device)))
        return y

    @staticmethod
    def ln_linear_rows(x, w, b, eps=1e-6, out=None):
        """y = b + LN(x) w^T on bf16 rows (x [M][384], w [N][>=384], N % 32 == 0): the DeiT block's norm1 + qkv (deit.py:40-47,:69), LN without
        affine (gamma / beta folded into w / b by the caller).  x [M][512]: the same row-wise kernel without the LayerNorm (Visformer stage-3
        qkv, visformer.py:175), b may be None."""
        _require_cuda(x, w)
        dt = ops._dt16(x, w)
        y = ops._out(out, x, w.shape[0])
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().fsvit_ln_linear_rows_dt(_ptr(x), _ptr(y), _ptr(w), w.shape[-1], _ptr(b), x.shape[0], x.shape[1], w.shape[0], float(eps),
                                                           dt, _stream_ptr(x.device)))
        return y

    @staticmethod
    def patch_embed2x2(x, w, bias, pos):
        """Visformer PatchEmbed (conv k2 s2 with folded BN, + pos_embed; visformer.py:266-288) on the row-wise kernel: x NHWC bf16 [B, H, H, Ci]
        (4 Ci = 512), w [N, 4 Ci] in (ky, kx, c) order, bias [N] or None, pos fp32 [(H/2)^2, N] -> [B (H/2)^2, N]."""
        _require_cuda(x, w, pos)
        dt = ops._dt16(x, w)
        B, H, _, Ci = x.shape
        y = torch.empty(B * (H // 2) * (H // 2), w.shape[0], device=x.device, dtype=x.dtype)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().fsvit_patch_embed2x2_dt(_ptr(x), _ptr(y), _ptr(w), w.shape[-1], _ptr(bias), _ptr(pos), B, H, Ci, w.shape[0],
                                                           dt, _stream_ptr(x.device)))
        return y

    @staticmethod
    def vit_block_tail(x, ctx, wp, bp, w1, b1, w2, b2, eps=1e-6, out=None):
        """DeiT block tail (deit.py:69-72) on bf16 rows, (C, KC, hidden) = (384, 384, 1536): x1 = x + bp + ctx wp^T;
        y = x1 + b2 + W2 GELU(W1 LN(x1) + b1), LN without affine (norm2's gamma / beta folded into w1 / b1 by the caller)."""
        _require_cuda(x, ctx, wp, bp, w1, b1, w2, b2)
        dt = ops._dt16(x, ctx, wp, w1, w2)
        lib = _lib.load()
        y = ops._out(out, x, x.shape[1])
        with torch.cuda.device(x.device):
            _lib.check(lib.fsvit_vit_block_tail_dt(_ptr(x), _ptr(y), _ptr(ctx), _ptr(wp), wp.shape[-1], ctx.shape[1], _ptr(bp), _ptr(w1), w1.shape[-1],
                                                   _ptr(b1), _ptr(w2), w2.shape[-1], _ptr(b2), x.shape[0], x.shape[1], w1.shape[0], float(eps),
                                                   dt, _stream_ptr(x.device)))
        return y

    @staticmethod
    def mlp_rows(x, w1, b1, w2, b2=None, out=None):
        """x [M][C] bf16 / fp16, C = 256 or 512; w1 [4C][K1w], w2 [C][K2w] packed K-major, same type; b1 [4C], b2 [C] fp32 or None.  y = x + W2 GELU(W1 x + b1) + b2."""
        _require_cuda(x, w1, w2)
        dt = ops._dt16(x, w1, w2)
        lib = _lib.load()
        y = ops._out(out, x, x.shape[1])
        with torch.cuda.device(x.device):
            _lib.check(lib.fsvit_mlp_rows_dt(_ptr(x), _ptr(y), _ptr(w1), w1.shape[-1], _ptr(b1), _ptr(w2), w2.shape[-1], _ptr(b2),
                                             x.shape[0], x.shape[1], w1.shape[0], dt, _stream_ptr(x.device)))
        return y

    @staticmethod
    def attention(qkv, B, S, heads, hdp, scale, numerics=None, out=None):
        """qkv [B S, 3 heads hdp] (rows (q | k | v, head, channel), pad channels zero) -> ctx [B S, heads hdp].  numerics 'bf16x2' / 'f16x2': qkv fp32,
        every product from two 16-bit limbs per operand (fsvit.h: fsvit_attention)."""
        _require_cuda(qkv)
        if numerics is not None:
            if numerics not in ('bf16x2', 'f16x2'):
                raise ValueError(f"numerics: None, 'bf16x2' or 'f16x2', got {numerics!r}")
            if qkv.dtype != torch.float32:
                raise TypeError(f'the two-limb modes read fp32 rows, got {qkv.dtype}')
        if tuple(qkv.shape) != (B * S, 3 * heads * hdp) or not qkv.is_contiguous():
            raise ValueError(f'qkv must be a contiguous [{B * S}, {3 * heads * hdp}] tensor')
        lib = _lib.load()
        ctx = ops._out(out, qkv, heads * hdp)
        with torch.cuda.device(qkv.device):
            _lib.check(lib.fsvit_attention(_ptr(qkv), _ptr(ctx), B, S, heads, hdp, float(scale), DTYPES[numerics] if numerics else ops._dt(qkv),
                                           _stream_ptr(qkv.device)))
        return ctx

    @staticmethod
    def qkv_attention(x, wqkv, bias, B, S, heads, hdp, scale):
        """Fused qkv conv + attention core (qkv_attn.hip): x [B*S, C] bf16, wqkv [3*heads*hdp, kw] bf16 -> ctx [B*S, heads*hdp]."""
        _require_cuda(x, wqkv)
        dt = ops._dt16(x, wqkv)
        lib = _lib.load()
        ctx = torch.empty(B * S, heads * hdp, dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.fsvit_qkv_attention_dt(_ptr(x), _ptr(wqkv), wqkv.shape[-1], _ptr(bias), _ptr(ctx), B, S, x.shape[1], heads, hdp,
                                                  float(scale), dt, _stream_ptr(x.device)))
        return ctx

    @staticmethod
    def vit_ln_qkv_attention(x, wqkv, bias, B, S, heads, hdp, scale, eps=1e-6):
        """norm1 + qkv Linear + attention core of a ViT block in one launch (mlp_rows.hip vit_attn_rows): x [B*S, 384] bf16, wqkv [3*heads*64, kw]
        bf16 (LayerNorm affine folded in by the caller) -> ctx [B*S, heads*64]."""
        _require_cuda(x, wqkv)
        dt = ops._dt16(x, wqkv)
        ctx = torch.empty(B * S, heads * hdp, dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().fsvit_vit_ln_qkv_attention_dt(_ptr(x), _ptr(wqkv), wqkv.shape[-1], _ptr(bias), _ptr(ctx), B, S, x.shape[1], heads, hdp,
                                                                 float(eps), float(scale), dt, _stream_ptr(x.device)))
        return ctx

    @staticmethod
    def im2col27(x, dtype):
        _require_cuda(x)
        lib = _lib.load()
        B, _, H, W = x.shape
        out = torch.empty(B * (H // 2) * (W // 2), 32, dtype=dtype, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.fsvit_im2col27(_ptr(x.contiguous()), _ptr(out), B, H, W, ops._dt(out), _stream_ptr(x.device)))
        return out

    @staticmethod
    def stem_conv1(x, w, bias, c1_planar=False):
        """im2col + stem conv1 + LeakyReLU in one pass (stem.hip): x [B,3,80,80] fp32, w [64, kw] bf16 -> (patches [B*1600,32], c1 [B*1600,64]).
        c1_planar: c1 in the row-chunk-planar layout of the eval stem (fsvit_op_stem_conv1), the same number of elements."""
        _require_cuda(x, w)
        if x.dtype != torch.float32:
            raise TypeError(f'stem_conv1 reads the fp32 image, got {x.dtype}')
        dt = ops._dt16(w)
        lib = _lib.load()
        B, _, H, W = x.shape
        patches = torch.empty(B * (H // 2) * (W // 2), 32, dtype=w.dtype, device=x.device)
        c1 = torch.empty(B * (H // 2) * (W // 2), 64, dtype=w.dtype, device=x.device)
        with torch.cuda.device(x.device):
            if c1_planar:
                _lib.check(lib.fsvit_op_stem_conv1(_ptr(x.contiguous()), _ptr(w), w.shape[-1], _ptr(bias), _ptr(patches), _ptr(c1), B, H, W, dt, 1,
                                                   _stream_ptr(x.device)))
            else:
                _lib.check(lib.fsvit_stem_conv1_dt(_ptr(x.contiguous()), _ptr(w), w.shape[-1], _ptr(bias), _ptr(patches), _ptr(c1), B, H, W, dt,
                                                   _stream_ptr(x.device)))
        return patches, c1

    @staticmethod
    def maxpool2_pos(x, pos):
        _require_cuda(x)
        lib = _lib.load()
        B, H, W, Cc = x.shape
        out = torch.empty(B, H // 2, W // 2, Cc, dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.fsvit_maxpool2_pos(_ptr(x), _ptr(pos), _ptr(out), B, H // 2, W // 2, Cc, ops._dt(x), _stream_ptr(x.device)))
        return out

    @staticmethod
    def pool_affine(x, scale, shift):
        _require_cuda(x)
        lib = _lib.load()
        B, HW, Cc = x.shape
        out = torch.empty(B, Cc, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.fsvit_pool_affine(_ptr(x), _ptr(scale), _ptr(shift), _ptr(out), B, HW, Cc, ops._dt(x), _stream_ptr(x.device)))
        return out

    @staticmethod
    def attention_backward(qkv, dctx, B, S, heads, hd, hdp, scale, out=None):
        """qkv [B S, 3 heads hdp], dctx [B S, heads hdp], both fp32 or both bf16, pad channels zero -> dqkv (dQ | dK | dV) (fsvit.h:
        fsvit_attention_backward).  The training kernels have no fp16 build: fp16 tensors raise TypeError."""
        _require_cuda(qkv, dctx)
        if qkv.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f'attention_backward is built for torch.float32 and torch.bfloat16, got {qkv.dtype}')
        if dctx.dtype != qkv.dtype:
            raise TypeError(f'qkv is {qkv.dtype} but dctx is {dctx.dtype}')
        if tuple(qkv.shape) != (B * S, 3 * heads * hdp) or tuple(dctx.shape) != (B * S, heads * hdp) or not qkv.is_contiguous() or not dctx.is_contiguous():
            raise ValueError(f'qkv / dctx must be contiguous [{B * S}, {3 * heads * hdp}] / [{B * S}, {heads * hdp}] tensors')
        lib = _lib.load()
        dqkv = ops._out(out, qkv, 3 * heads * hdp)
        with torch.cuda.device(qkv.device):
            _lib.check(lib.fsvit_attention_backward(_ptr(qkv), _ptr(dctx), _ptr(dqkv), B, S, heads, hd, hdp, float(scale),
                                                    ops._dt(qkv), _stream_ptr(qkv.device)))
        return dqkv

    @staticmethod
    def _head_in(*ts):
        """The head kernels read dense fp32 rows: every wrapper of the head takes any layout / floating type and hands over a contiguous fp32 copy (no copy
        when the tensor already is one), so a permuted view, a strided slice or a float64 temperature gives the bits of its contiguous fp32 copy."""
        return tuple(t.detach().contiguous().float() for t in ts)

    @staticmethod
    def proto_head_backward(feat_shot, feat_query, dlogits, temp, method='cos'):
        """-> dfeat_shot [E,way,shot,D], dfeat_query [E,Q,D], dtemp (scalar tensor); method 'cos' or 'sqr'."""
        if method not in ('cos', 'sqr'):
            raise ValueError(method)
        _require_cuda(feat_shot, feat_query, dlogits)
        lib = _lib.load()
        feat_shot, feat_query, dlogits = ops._head_in(feat_shot, feat_query, dlogits)
        E, way, shot, D = feat_shot.shape
        Q = feat_query.shape[1]
        dev = feat_shot.device
        ds, dq = torch.empty_like(feat_shot), torch.empty_like(feat_query)
        dt = torch.empty(E, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            if isinstance(temp, torch.Tensor) and temp.is_cuda:
                _lib.check(lib.fsvit_proto_head_backward_devtemp(_ptr(feat_shot), _ptr(feat_query), _ptr(dlogits), E, way, shot, Q, D,
                                                                 _ptr(ops._head_in(temp)[0]), _lib.HEAD_COS if method == 'cos' else _lib.HEAD_SQR,
                                                                 _ptr(ds), _ptr(dq), _ptr(dt), _stream_ptr(dev)))
            else:
                fn = lib.fsvit_proto_head_backward if method == 'cos' else lib.fsvit_proto_head_backward_sqr
                _lib.check(fn(_ptr(feat_shot), _ptr(feat_query), _ptr(dlogits), E, way, shot, Q, D, float(temp), _ptr(ds), _ptr(dq), _ptr(dt),
                              _stream_ptr(dev)))
        return ds, dq, dt.sum()

    @staticmethod
    def conv1x1_wgrad(x, dz, limbs='bf16'):
        """x [M,C], dz [M,N] (bf16 / fp16, or fp32 = two-limb arithmetic with `limbs` 'bf16' / 'f16') -> dW [N,C] fp32 (fsvit_conv1x1_wgrad)."""
        _require_cuda(x, dz)
        lib = _lib.load()
        assert x.dtype == dz.dtype and x.dtype in (torch.bfloat16, torch.float16, torch.float32) and x.shape[0] == dz.shape[0]
        x, dz = x.contiguous(), dz.contiguous()
        dw = torch.empty(dz.shape[1], x.shape[1], dtype=torch.float32, device=x.device)
        dt = {torch.bfloat16: _lib.BF16, torch.float16: _lib.F16, torch.float32: _lib.BF16X2 if limbs == 'bf16' else _lib.F16X2}[x.dtype]
        with torch.cuda.device(x.device):
            _lib.check(lib.fsvit_conv1x1_wgrad(_ptr(x), _ptr(dz), _ptr(dw), x.shape[0], dz.shape[1], x.shape[1], dt, _stream_ptr(x.device)))
        return dw

    @staticmethod
    def conv3x3_wgrad(x_nhwc, dz, O, Ig, groups, limbs='bf16'):
        """x [B,H,W,groups*Ig], dz [B,H,W,O] (bf16 / fp16, or fp32 = two-limb arithmetic with `limbs` 'bf16' / 'f16') -> dW [O,Ig,3,3] fp32 of a
        3x3 / stride 1 / pad 1 convolution (fsvit_conv3x3_wgrad)."""
        _require_cuda(x_nhwc, dz)
        lib = _lib.load()
        assert x_nhwc.dtype == dz.dtype and x_nhwc.dtype in (torch.bfloat16, torch.float16, torch.float32)
        B, H, W, C = x_nhwc.shape
        assert C == groups * Ig and dz.shape == (B, H, W, O)
        x_nhwc, dz = x_nhwc.contiguous(), dz.contiguous()
        dw = torch.empty(O, Ig, 3, 3, dtype=torch.float32, device=x_nhwc.device)
        with torch.cuda.device(x_nhwc.device):
            dt = {torch.bfloat16: _lib.BF16, torch.float16: _lib.F16, torch.float32: _lib.BF16X2 if limbs == 'bf16' else _lib.F16X2}[x_nhwc.dtype]
            _lib.check(lib.fsvit_conv3x3_wgrad(_ptr(x_nhwc), _ptr(dz), _ptr(dw), B, H, W, O, Ig, groups, dt, _stream_ptr(x_nhwc.device)))
        return dw

    _ptr_tables = {}

    @staticmethod
    def _ptr_table(kind, dev, rows):
        """The int64 device table of a multi-tensor launch (rows of pointers and a length, the item layouts of csrc/optim.hip), cached per
        (kind, device, number of rows).  Pinned allocation + upload only when a pointer changed: with parallel.GradBucket or
        zero_grad(set_to_none=False) the gradients keep their addresses and a step uploads nothing (hipHostMalloc per step stalled the host
        behind the whole backward).  The same tensor object is returned while `rows` is unchanged; the pinned host copy lives with the entry."""
        key = (kind, dev, len(rows))
        cached = ops._ptr_tables.get(key)
        if cached is None or cached[0] != rows:
            host = torch.tensor(rows, dtype=torch.int64).pin_memory()
            with torch.cuda.device(dev):
                cached = (rows, host.to(dev, non_blocking=True), host)
            ops._ptr_tables[key] = cached
        return cached[1]

    @staticmethod
    def _sgd_multi(entry, params, grads, bufs, lr, momentum, weight_decay, first_step):
        if not params:
            return
        _require_cuda(*params)
        lib = _lib.load()
        bump_weight_generation(params)
        dev = params[0].device
        rows = tuple((p.data_ptr(), g.data_ptr(), b.data_ptr(), p.numel()) for p, g, b in zip(params, grads, bufs))
        table = ops._ptr_table(entry, dev, rows)
        with torch.cuda.device(dev):
            _lib.check(getattr(lib, entry)(_ptr(table), len(params), max(r[3] for r in rows), float(lr), float(momentum), float(weight_decay),
                                           int(bool(first_step)), _stream_ptr(dev)))
        return table

    @staticmethod
    def _sgd_single(entry, param, grad, buf, lr, momentum, weight_decay, first_step):
        _require_cuda(param, grad, buf)
        lib = _lib.load()
        bump_weight_generation((param,))
        with torch.cuda.device(param.device):
            _lib.check(getattr(lib, entry)(_ptr(param), _ptr(grad), _ptr(buf), param.numel(), float(lr), float(momentum), float(weight_decay),
                                           int(bool(first_step)), _stream_ptr(param.device)))

    @staticmethod
    def sgd_step_multi(params, grads, bufs, lr, momentum, weight_decay, first_step):
        """torch.optim.SGD with momentum for a list of fp32 tensors in one launch (fsvit_sgd_step_multi).  -> the device table (ops._ptr_table)."""
        return ops._sgd_multi('fsvit_sgd_step_multi', params, grads, bufs, lr, momentum, weight_decay, first_step)

    @staticmethod
    def sgd_step(param, grad, buf, lr, momentum, weight_decay, first_step):
        ops._sgd_single('fsvit_sgd_step', param, grad, buf, lr, momentum, weight_decay, first_step)

    @staticmethod
    def sgd_nesterov_step_multi(params, grads, bufs, lr, momentum, weight_decay, first_step):
        """torch.optim.SGD(nesterov=True) for a list of fp32 tensors in one launch (fsvit_sgd_nesterov_step_multi).  -> the device table."""
        return ops._sgd_multi('fsvit_sgd_nesterov_step_multi', params, grads, bufs, lr, momentum, weight_decay, first_step)

    @staticmethod
    def sgd_nesterov_step(param, grad, buf, lr, momentum, weight_decay, first_step):
        ops._sgd_single('fsvit_sgd_nesterov_step', param, grad, buf, lr, momentum, weight_decay, first_step)

    @staticmethod
    def grad_nan_guard(grads, device=None):
        """detect_grad_nan of the reference for a list of contiguous fp32 gradient tensors (fsvit_grad_nan_guard_multi): a tensor holding any NaN is
        zeroed entirely (Inf does not count) -> int32 device tensor [len(grads)] of 0 / 1 flags.  No host synchronisation; the {pointer, numel}
        table is cached (ops._ptr_table)."""
        if not grads:
            return torch.zeros(0, dtype=torch.int32, device=device if device is not None else 'cuda')
        _require_cuda(*grads)
        for g in grads:
            if g.dtype != torch.float32 or not g.is_contiguous():
                raise ValueError('grad_nan_guard: contiguous fp32 tensors')
        lib = _lib.load()
        dev = grads[0].device
        rows = tuple((g.data_ptr(), g.numel()) for g in grads)
        table = ops._ptr_table('guard', dev, rows)
        flags = torch.empty(len(grads), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.fsvit_grad_nan_guard_multi(_ptr(table), len(grads), max(r[1] for r in rows), _ptr(flags), _stream_ptr(dev)))
        return flags

    _tickets = {}

    @staticmethod
    def _ticket(dev):
        """Two zeroed device words per (device, STREAM): forward / backward of the fused CE head count their workgroups on them and leave them at
        zero.  Launches on one stream are ordered; two models stepping on different streams each get their own pair (one pair per device
        let concurrent launches race on the counter)."""
        key = (dev.type, dev.index, torch.cuda.current_stream(dev).cuda_stream)
        if key not in ops._tickets:
            ops._tickets[key] = torch.zeros(2, dtype=torch.int32, device=dev)
        return ops._tickets[key]

    @staticmethod
    def proto_head_ce(feat_shot, feat_query, temp, label=None, method='cos'):
        """Head + F.cross_entropy + compute_acc of the meta-tuning step in one launch (fsvit_proto_head_ce): -> logits [E,Q,way], dlogits [E,Q,way]
        (of the mean CE), stats [2 + 2 E] = {loss, acc, acc per episode .., loss per episode ..}.  label: int64 [E*Q] on the device (None: make_nk_label)."""
        _require_cuda(feat_shot, feat_query)
        lib = _lib.load()
        feat_shot, feat_query = ops._head_in(feat_shot, feat_query)
        E, way, shot, D = feat_shot.shape
        Q = feat_query.shape[1]
        dev = feat_shot.device
        logits = torch.empty(E, Q, way, dtype=torch.float32, device=dev)
        dlogits = torch.empty(E, Q, way, dtype=torch.float32, device=dev)
        stats = torch.full((2 + 2 * E,), float('nan'), dtype=torch.float32, device=dev)      # (a skipped final reduction must not read as a loss)
        m = {'cos': _lib.HEAD_COS, 'sqr': _lib.HEAD_SQR, 'dot': _lib.HEAD_DOT}[method]
        if label is not None:
            if label.dtype != torch.int64 or not label.is_cuda or label.numel() != E * Q:
                raise ValueError('label: int64 [E*Q] on the device')
            label = label.contiguous()
        dev_temp = isinstance(temp, torch.Tensor) and temp.is_cuda
        temp_d = ops._head_in(temp)[0] if dev_temp else None
        tk = ops._ticket(dev)
        with torch.cuda.device(dev):
            _lib.check(lib.fsvit_proto_head_ce(_ptr(feat_shot), _ptr(feat_query), _ptr(label) if label is not None else None, E, way, shot, Q, D,
                                               0.0 if dev_temp else float(temp), _ptr(temp_d), m, _ptr(logits), _ptr(dlogits),
                                               _ptr(stats[2:2 + E]), _ptr(stats[2 + E:]), _ptr(stats), tk.data_ptr(), _stream_ptr(dev)))
        return logits, dlogits, stats

    @staticmethod
    def proto_head_ce_backward(feat_shot, feat_query, dlogits, dloss, temp, method='cos'):
        """-> dfeat_shot, dfeat_query, dtemp (0-d tensor): fsvit_proto_head_ce_backward with the upstream gradient `dloss` read on the device."""
        if method not in ('cos', 'sqr'):
            raise ValueError(method)
        _require_cuda(feat_shot, feat_query, dlogits)
        lib = _lib.load()
        feat_shot, feat_query, dlogits = ops._head_in(feat_shot, feat_query, dlogits)
        E, way, shot, D = feat_shot.shape
        Q = feat_query.shape[1]
        dev = feat_shot.device
        ds, dq = torch.empty_like(feat_shot), torch.empty_like(feat_query)
        dt = torch.empty(E + 1, dtype=torch.float32, device=dev)
        dev_temp = isinstance(temp, torch.Tensor) and temp.is_cuda
        temp_d = ops._head_in(temp)[0] if dev_temp else None
        if dloss is not None and not (dloss.is_cuda and dloss.dtype == torch.float32 and dloss.numel() == 1):
            raise ValueError('dloss: one fp32 value on the device')
        tk = ops._ticket(dev)
        with torch.cuda.device(dev):
            _lib.check(lib.fsvit_proto_head_ce_backward(_ptr(feat_shot), _ptr(feat_query), _ptr(dlogits), _ptr(dloss) if dloss is not None else None, E, way,
                                                        shot, Q, D, 0.0 if dev_temp else float(temp), _ptr(temp_d),
                                                        _lib.HEAD_COS if method == 'cos' else _lib.HEAD_SQR, _ptr(ds), _ptr(dq), _ptr(dt),
                                                        tk.data_ptr() + 4, _stream_ptr(dev)))
        return ds, dq, dt[E]

    @staticmethod
    def proto_head(feat_shot, feat_query, temp, method='cos'):
        """feat_shot [E,way,shot,D], feat_query [E,Q,D] fp32 -> logits [E,Q,way], acc [E], loss [E]."""
        _require_cuda(feat_shot, feat_query)
        lib = _lib.load()
        feat_shot, feat_query = ops._head_in(feat_shot, feat_query)
        E, way, shot, D = feat_shot.shape
        Q = feat_query.shape[1]
        dev = feat_shot.device
        logits = torch.empty(E, Q, way, dtype=torch.float32, device=dev)
        acc = torch.empty(E, dtype=torch.float32, device=dev)
        loss = torch.empty(E, dtype=torch.float32, device=dev)
        m = {'cos': _lib.HEAD_COS, 'sqr': _lib.HEAD_SQR, 'dot': _lib.HEAD_DOT}[method]
        with torch.cuda.device(dev):
            if isinstance(temp, torch.Tensor) and temp.is_cuda:      # the learnable temperature stays on the device: no .item() synchronisation per step
                _lib.check(lib.fsvit_proto_head_devtemp(_ptr(feat_shot), _ptr(feat_query), E, way,
                                                        shot, Q, D, _ptr(ops._head_in(temp)[0]), m, _ptr(logits), _ptr(acc), _ptr(loss),
                                                        _stream_ptr(dev)))
            else:
                _lib.check(lib.fsvit_proto_head(_ptr(feat_shot), _ptr(feat_query), E, way,
                                                shot, Q, D, float(temp), m, _ptr(logits), _ptr(acc), _ptr(loss), _stream_ptr(dev)))
        return logits, acc, loss

    @staticmethod
    def proto_head_gather(table, idx, shot, temp, invalid, method='cos'):
        """The head of `proto_head` over rows of a feature table: table [N,D] fp32, idx [E,way,shot+n_query] (int32 / int64) slot numbers in the sampler's
        class-major order -> logits [E,way*n_query,way], acc [E], loss [E]; for the same rows the bits of `proto_head`.  invalid [1] int32 is raised by
        one per slot outside [0, N); such an episode's outputs are NaN.  Limits: fsvit_proto_head_gather (fsvit.h)."""
        _require_cuda(table, idx, invalid)
        lib = _lib.load()
        table, = ops._head_in(table)
        if table.dim() != 2 or idx.dim() != 3 or idx.dtype not in (torch.int32, torch.int64):
            raise ValueError('expected table [N,D] and idx [E,way,shot+n_query] int32 / int64')
        if invalid.dtype != torch.int32 or invalid.numel() != 1:
            raise ValueError('invalid: one int32')
        idx = idx.contiguous()
        N, D = table.shape
        E, way, per_class = idx.shape
        n_query = per_class - int(shot)
        dev = table.device
        logits = torch.empty(E, way * max(n_query, 0), way, dtype=torch.float32, device=dev)
        acc = torch.empty(E, dtype=torch.float32, device=dev)
        loss = torch.empty(E, dtype=torch.float32, device=dev)
        dev_temp = isinstance(temp, torch.Tensor) and temp.is_cuda
        temp_d = ops._head_in(temp)[0] if dev_temp else None
        if E == 0:
            return logits, acc, loss
        with torch.cuda.device(dev):
            _lib.check(lib.fsvit_proto_head_gather(_ptr(table), N, D, _ptr(idx), int(idx.dtype == torch.int64), E, way, int(shot), n_query,
                                                   0.0 if dev_temp else float(temp), _ptr(temp_d), ops._HEAD_METHOD[method], _ptr(logits), _ptr(acc),
                                                   _ptr(loss), _ptr(invalid), _stream_ptr(dev)))
        return logits, acc, loss

    # ---- prototype bank over a labelled support set (proto_bank.hip; limits in fsvit.h) and the single-prototype ROC-AUC of --sauc
    _HEAD_METHOD = {'cos': _lib.HEAD_COS, 'sqr': _lib.HEAD_SQR, 'dot': _lib.HEAD_DOT}

    @staticmethod
    def _bank_state(sum_, count, invalid, way, D):
        for t, shape, dt in ((sum_, (way, D), torch.float32), (count, (way,), torch.int32), (invalid, (1,), torch.int32)):
            if t is None:
                continue
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f'bank state: expected a contiguous {dt} tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}')

    @staticmethod
    def proto_bank_accumulate(feat, labels, sum_, count, invalid):
        """feat [S,D], labels [S] (int32 / int64) added into the bank state in place: sum_ [way,D] fp32, count [way] int32, invalid [1] int32 (the number of
        labels outside [0, way); they add nothing else).  Rows of a class are added in ascending index on top of the stored sum."""
        _require_cuda(feat, labels, sum_, count, invalid)
        lib = _lib.load()
        feat, = ops._head_in(feat)
        if feat.dim() != 2 or sum_.dim() != 2:
            raise ValueError('expected feat [S,D] and sum [way,D]')
        way, D = sum_.shape
        ops._bank_state(sum_, count, invalid, way, D)
        if labels.dtype not in (torch.int32, torch.int64) or labels.dim() != 1 or labels.shape[0] != feat.shape[0] or feat.shape[1] != D:
            raise ValueError('expected labels [S] int32 / int64 for feat [S,D] and sum [way,D]')
        labels = labels.contiguous()
        with torch.cuda.device(feat.device):
            _lib.check(lib.fsvit_proto_bank_accumulate(_ptr(feat), _ptr(labels), int(labels.dtype == torch.int64), feat.shape[0], way, D, _ptr(sum_),
                                                       _ptr(count), _ptr(invalid), _stream_ptr(feat.device)))

    @staticmethod
    def proto_bank_finalize(sum_, count, method='cos'):
        """-> proto [way,D] fp32 (the class means; 'cos': F.normalize of them), empty [way] int32 (1 where count == 0: zero prototype)."""
        _require_cuda(sum_, count)
        lib = _lib.load()
        if sum_.dim() != 2:
            raise ValueError('expected sum [way,D]')
        way, D = sum_.shape
        ops._bank_state(sum_, count, None, way, D)
        proto = torch.empty(way, D, dtype=torch.float32, device=sum_.device)
        empty = torch.empty(way, dtype=torch.int32, device=sum_.device)
        with torch.cuda.device(sum_.device):
            _lib.check(lib.fsvit_proto_bank_finalize(_ptr(sum_), _ptr(count), way, D, ops._HEAD_METHOD[method], _ptr(proto), _ptr(empty),
                                                     _stream_ptr(sum_.device)))
        return proto, empty

    @staticmethod
    def proto_bank_logits(query, proto, empty, temp, method='cos', want_pred=True):
        """query [Q,D], proto [way,D] / empty [way] of proto_bank_finalize (empty None: no class is) -> logits [Q,way] fp32, pred [Q] int32 (the first
        maximum; None without want_pred).  temp: a Python number or a device scalar read where it lives."""
        _require_cuda(query, proto, empty)
        lib = _lib.load()
        query, proto = ops._head_in(query, proto)
        if query.dim() != 2 or proto.dim() != 2 or query.shape[1] != proto.shape[1]:
            raise ValueError('expected query [Q,D] and proto [way,D]')
        Q, D = query.shape
        way = proto.shape[0]
        if empty is not None:
            if empty.dtype != torch.int32 or tuple(empty.shape) != (way,):
                raise ValueError('empty: int32 [way]')
            empty = empty.contiguous()
        dev = query.device
        logits = torch.empty(Q, way, dtype=torch.float32, device=dev)
        pred = torch.empty(Q, dtype=torch.int32, device=dev) if want_pred else None
        dev_temp = isinstance(temp, torch.Tensor) and temp.is_cuda
        temp_d = ops._head_in(temp)[0] if dev_temp else None
        with torch.cuda.device(dev):
            _lib.check(lib.fsvit_proto_bank_logits(_ptr(query), _ptr(proto), _ptr(empty), Q, way, D, 0.0 if dev_temp else float(temp), _ptr(temp_d),
                                                   ops._HEAD_METHOD[method], _ptr(logits), _ptr(pred), _stream_ptr(dev)))
        return logits, pred

    @staticmethod
    def check_topk_k(k, what):
        """the list length of proto_bank_topk: an int in [1, 32]; the argument alone decides, so callers check it before they look at a device"""
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 32:
            raise ValueError(f'{what}: k = {k!r} is outside [1, 32]')

    @staticmethod
    def proto_bank_topk(query, proto, empty, temp, method='cos', k=5, n_split=0, want_lse=True):
        """The k best classes of every row of proto_bank_logits(query, proto, empty, temp, method) without the [Q,way] matrix -> (values [Q,k] fp32,
        indices [Q,k] int32, lse [Q] fp32 or None): the head of a stable descending sort of the row (ties: the lower class; ranks beyond `way`: -inf, -1)
        and the row's log-sum-exp over the non-empty classes.  1 <= k <= 32; n_split: how many workgroups share the class axis of a query tile
        (0: chosen from Q, way and the CU count, fsvit.h) - the results do not depend on it."""
        ops.check_topk_k(k, 'proto_bank_topk')
        if isinstance(n_split, bool) or not isinstance(n_split, int) or n_split < 0:
            raise ValueError(f'proto_bank_topk: n_split = {n_split!r} (0: the library chooses)')
        _require_cuda(query, proto, empty)
        lib = _lib.load()
        query, proto = ops._head_in(query, proto)
        if query.dim() != 2 or proto.dim() != 2 or query.shape[1] != proto.shape[1]:
            raise ValueError('expected query [Q,D] and proto [way,D]')
        Q, D = query.shape
        way = proto.shape[0]
        if empty is not None:
            if empty.dtype != torch.int32 or tuple(empty.shape) != (way,):
                raise ValueError('empty: int32 [way]')
            empty = empty.contiguous()
        dev = query.device
        values = torch.empty(Q, k, dtype=torch.float32, device=dev)
        indices = torch.empty(Q, k, dtype=torch.int32, device=dev)
        lse = torch.empty(Q, dtype=torch.float32, device=dev) if want_lse else None
        dev_temp = isinstance(temp, torch.Tensor) and temp.is_cuda
        temp_d = ops._head_in(temp)[0] if dev_temp else None
        if Q == 0:                                               # nothing to score (an empty tensor has no address to hand over)
            return values, indices, lse
        with torch.cuda.device(dev):
            ws_bytes = int(lib.fsvit_proto_bank_topk_workspace_bytes(Q, way, k, n_split))      # 0 for arguments the call below refuses with its message
            ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=dev)
            _lib.check(lib.fsvit_proto_bank_topk(_ptr(query), _ptr(proto), _ptr(empty), Q, way, D, 0.0 if dev_temp else float(temp), _ptr(temp_d),
                                                 ops._HEAD_METHOD[method], k, n_split, _ptr(values), _ptr(indices), _ptr(lse), _ptr(ws), ws_bytes,
                                                 _stream_ptr(dev)))
        return values, indices, lse

    @staticmethod
    def proto_auc(feat_shot, feat_query, want_score=False):
        """feat_shot [E,shot,D] (the shots of class 0), feat_query [E,Q,D] with the first Q / 2 queries positive -> auc [E] fp32: roc_auc_score of the cosine
        scores against the normalised mean shot (test_few_shot.py --sauc); with want_score also score [E,Q]."""
        _require_cuda(feat_shot, feat_query)
        lib = _lib.load()
        feat_shot, feat_query = ops._head_in(feat_shot, feat_query)
        if feat_shot.dim() != 3 or feat_query.dim() != 3 or feat_shot.shape[0] != feat_query.shape[0] or feat_shot.shape[2] != feat_query.shape[2]:
            raise ValueError('expected feat_shot [E,shot,D] and feat_query [E,Q,D]')
        E, shot, D = feat_shot.shape
        Q = feat_query.shape[1]
        dev = feat_shot.device
        auc = torch.empty(E, dtype=torch.float32, device=dev)
        score = torch.empty(E, Q, dtype=torch.float32, device=dev) if want_score else None
        with torch.cuda.device(dev):
            _lib.check(lib.fsvit_proto_auc(_ptr(feat_shot), _ptr(feat_query), E, shot, Q, D, _ptr(auc), _ptr(score), _stream_ptr(dev)))
        return (auc, score) if want_score else auc

    @staticmethod
    def proto_auc_gather(table, shot_slots, query_slots, invalid, want_score=False):
        """The reduction of `proto_auc` over rows of a feature table: table [N,D] fp32, shot_slots [E,shot] (the shots of class 0), query_slots [E,Q]
        (positives first, then as many negatives), both int32 or both int64 -> auc [E] fp32, with want_score also score [E,Q]; for the same rows the bits
        of `proto_auc`.  invalid [1] int32 is raised by one per slot outside [0, N); such an episode's outputs are NaN.  Limits: fsvit_proto_auc_gather
        (fsvit.h)."""
        _require_cuda(table, shot_slots, query_slots, invalid)
        lib = _lib.load()
        table, = ops._head_in(table)
        if (table.dim() != 2 or shot_slots.dim() != 2 or query_slots.dim() != 2 or shot_slots.shape[0] != query_slots.shape[0]
                or shot_slots.dtype not in (torch.int32, torch.int64) or query_slots.dtype != shot_slots.dtype):
            raise ValueError('expected table [N,D], shot_slots [E,shot] and query_slots [E,Q] of one dtype, int32 / int64')
        if invalid.dtype != torch.int32 or invalid.numel() != 1:
            raise ValueError('invalid: one int32')
        shot_slots, query_slots = shot_slots.contiguous(), query_slots.contiguous()
        N, D = table.shape
        E, shot = shot_slots.shape
        Q = query_slots.shape[1]
        dev = table.device
        auc = torch.empty(E, dtype=torch.float32, device=dev)
        score = torch.empty(E, Q, dtype=torch.float32, device=dev) if want_score else None
        if E == 0:                                               # (an empty tensor has no address to hand over)
            return (auc, score) if want_score else auc
        with torch.cuda.device(dev):
            _lib.check(lib.fsvit_proto_auc_gather(_ptr(table), N, D, _ptr(shot_slots), _ptr(query_slots), int(shot_slots.dtype == torch.int64), E, shot, Q,
                                                  _ptr(auc), _ptr(score), _ptr(invalid), _stream_ptr(dev)))
        return (auc, score) if want_score else auc

    # ---- operator entry points of the memory-bound training kernels (fsvit_op_*: tests, tools).  Maps are [M, C] / NHWC tensors in the storage
    # dtype (fp32 or bf16), statistics / parameters fp32; outputs and the kernels' `partial` scratch are allocated here.
    @staticmethod
    def _op(x, name, *args):
        lib = _lib.load()
        with torch.cuda.device(x.device):
            _lib.check(getattr(lib, 'fsvit_op_' + name)(*args, _stream_ptr(x.device)))

    @staticmethod
    def _scratch(n, dev):
        return torch.empty(max(int(n), 1), dtype=torch.float32, device=dev)

    @staticmethod
    def bn_train_forward(z, gamma, beta, running_mean=None, running_var=None, eps=1e-5, momentum=0.1, frozen=False, add_a=None, add_b=None,
                         add_scale=None, rows_per_img=0, res=None, act=_lib.ACT_NONE, apply=True):
        """z [M,C] (overwritten with add_a + scale * add_b when add_b is given) -> (y or None, mean, invstd, sa, sb); running stats updated in place."""
        _require_cuda(z, gamma, beta, running_mean, running_var, add_a, add_b, add_scale, res)
        M, Cc = z.shape
        stats = torch.empty(4, Cc, dtype=torch.float32, device=z.device)
        partial = ops._scratch(_lib.load().fsvit_op_bn_reduce_blocks(M) * 2 * Cc, z.device)
        y = torch.empty_like(z) if apply else None
        ops._op(z, 'bn_train_forward', _ptr(z), M, Cc, ops._dt(z), _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), float(eps), float(momentum),
                int(frozen), _ptr(add_a), _ptr(add_b), _ptr(add_scale), int(rows_per_img), _ptr(res), int(act), _ptr(y), _ptr(stats), _ptr(partial))
        return y, stats[0], stats[1], stats[2], stats[3]

    @staticmethod
    def bn_train_backward(dy, z, mean, invstd, gamma, frozen=False, act_sa=None, act_sb=None, acc=None, scale2=None, out2=None, rows_per_img=0, dz=None):
        """-> (dz, dgamma, dbeta, coef [3,C]); dz may be `acc`, out2 may be `dy` (both written in place when passed)."""
        _require_cuda(dy, z, mean, invstd, gamma, act_sa, act_sb, acc, scale2, out2, dz)
        M, Cc = z.shape
        dz = torch.empty_like(z) if dz is None else dz
        dgamma, dbeta = ops._scratch(Cc, z.device), ops._scratch(Cc, z.device)
        coef = torch.empty(3, Cc, dtype=torch.float32, device=z.device)
        partial = ops._scratch(_lib.load().fsvit_op_bn_reduce_blocks(M) * 2 * Cc, z.device)
        ops._op(z, 'bn_train_backward', _ptr(dy), _ptr(z), _ptr(mean), _ptr(invstd), _ptr(gamma), M, Cc, ops._dt(z), int(frozen), _ptr(act_sa), _ptr(act_sb),
                _ptr(acc), _ptr(scale2), _ptr(out2), int(rows_per_img), _ptr(dz), _ptr(dgamma), _ptr(dbeta), _ptr(coef), _ptr(partial))
        return dz, dgamma, dbeta, coef

    @staticmethod
    def bn_act_bwd(dout, z, sa, sb, res=None):
        _require_cuda(dout, z, sa, sb, res)
        g = torch.empty_like(z)
        ops._op(z, 'bn_act_bwd', _ptr(dout), _ptr(z), _ptr(sa), _ptr(sb), _ptr(res), _ptr(g), z.shape[0], z.shape[1], ops._dt(z))
        return g

    @staticmethod
    def stem_tail_train_forward(z, sa, sb, res=None, rsa=None, rsb=None, pos=None):
        """z / res [B,2OH,2OW,C] -> (out [B,OH,OW,C], arg uint8 [B,OH,OW,C]); pos [OH*OW, C] fp32."""
        _require_cuda(z, sa, sb, res, rsa, rsb, pos)
        B, H, W, Cc = z.shape
        out = torch.empty(B, H // 2, W // 2, Cc, dtype=z.dtype, device=z.device)
        arg = torch.empty(B, H // 2, W // 2, Cc, dtype=torch.uint8, device=z.device)
        ops._op(z, 'stem_tail_train_forward', _ptr(z), _ptr(sa), _ptr(sb), _ptr(res), _ptr(rsa), _ptr(rsb), _ptr(pos), _ptr(out), _ptr(arg), B, H // 2, W // 2, Cc,
                ops._dt(z))
        return out, arg

    @staticmethod
    def stem_tail_train_backward(dout, arg, z3, zd, mean3, invstd3, meand, invstdd, gamma3, gammad, frozen=False):
        """-> (dz3, dzd, dgamma3, dbeta3, dgammad, dbetad)"""
        _require_cuda(dout, arg, z3, zd, mean3, invstd3, meand, invstdd, gamma3, gammad)
        B, OH, OW, Cc = dout.shape
        dev = z3.device
        nb = _lib.load().fsvit_op_pool_bn_bwd_blocks(B, OH, OW, Cc, ops._dt(z3))
        stats3, statsd = torch.stack([mean3, invstd3]).contiguous(), torch.stack([meand, invstdd]).contiguous()
        dz3, dzd = torch.empty_like(z3), torch.empty_like(zd)
        pg = [ops._scratch(Cc, dev) for _ in range(4)]
        coef, partial = ops._scratch(6 * Cc, dev), ops._scratch(nb * 4 * Cc, dev)
        ops._op(z3, 'stem_tail_train_backward', _ptr(dout), _ptr(arg), _ptr(z3), _ptr(zd), _ptr(stats3), _ptr(statsd), _ptr(gamma3), _ptr(gammad), _ptr(dz3), _ptr(dzd),
                _ptr(pg[0]), _ptr(pg[1]), _ptr(pg[2]), _ptr(pg[3]), _ptr(coef), _ptr(partial), B, OH, OW, Cc, ops._dt(z3), int(frozen))
        return (dz3, dzd) + tuple(pg)

    @staticmethod
    def pool_act_bwd(dout, arg):
        _require_cuda(dout, arg)
        B, OH, OW, Cc = dout.shape
        g = torch.empty(B, 2 * OH, 2 * OW, Cc, dtype=dout.dtype, device=dout.device)
        ops._op(dout, 'pool_act_bwd', _ptr(dout), _ptr(arg), _ptr(g), B, OH, OW, Cc, ops._dt(dout))
        return g

    @staticmethod
    def maxpool2_idx(x, pos=None):
        _require_cuda(x, pos)
        B, H, W, Cc = x.shape
        out = torch.empty(B, H // 2, W // 2, Cc, dtype=x.dtype, device=x.device)
        arg = torch.empty(B, H // 2, W // 2, Cc, dtype=torch.uint8, device=x.device)
        ops._op(x, 'maxpool2_idx', _ptr(x), _ptr(pos), _ptr(out), _ptr(arg), B, H // 2, W // 2, Cc, ops._dt(x))
        return out, arg

    @staticmethod
    def maxpool2_bwd(dout, arg):
        _require_cuda(dout, arg)
        B, OH, OW, Cc = dout.shape
        din = torch.empty(B, 2 * OH, 2 * OW, Cc, dtype=dout.dtype, device=dout.device)
        ops._op(dout, 'maxpool2_bwd', _ptr(dout), _ptr(arg), _ptr(din), B, OH, OW, Cc, ops._dt(dout))
        return din

    @staticmethod
    def ln_train_forward(x, gamma, beta, eps=1e-6):
        """x [M,D] -> (y, mean [M], rstd [M])"""
        _require_cuda(x, gamma, beta)
        M, D = x.shape
        y = torch.empty_like(x)
        mean, rstd = ops._scratch(M, x.device), ops._scratch(M, x.device)
        ops._op(x, 'ln_train_forward', _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean), _ptr(rstd), M, D, float(eps), ops._dt(x))
        return y, mean, rstd

    @staticmethod
    def ln_train_backward(dy, x, mean, rstd, gamma, add=None, dx=None, param_grads=True):
        """-> (dx, dgamma, dbeta) (the last two None without param_grads); dx may be `add`."""
        _require_cuda(dy, x, mean, rstd, gamma, add, dx)
        M, D = x.shape
        dx = torch.empty_like(x) if dx is None else dx
        dgamma = ops._scratch(D, x.device) if param_grads else None
        dbeta = ops._scratch(D, x.device) if param_grads else None
        partial = ops._scratch(_lib.load().fsvit_op_ln_bwd_blocks(M) * 2 * D, x.device)
        ops._op(x, 'ln_train_backward', _ptr(dy), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(add), _ptr(dx), _ptr(partial), _ptr(dgamma), _ptr(dbeta), M, D,
                ops._dt(x))
        return dx, dgamma, dbeta

    @staticmethod
    def vit_assemble(zpe, cls, pos, B, S):
        """zpe [B*(S-1), D], cls [D], pos [S, D] -> tokens [B, S, D]"""
        _require_cuda(zpe, cls, pos)
        D = pos.shape[-1]
        tokens = torch.empty(B, S, D, dtype=zpe.dtype, device=zpe.device)
        ops._op(zpe, 'vit_assemble', _ptr(zpe), _ptr(cls), _ptr(pos), _ptr(tokens), B, S, D, ops._dt(zpe))
        return tokens

    @staticmethod
    def vit_patch_rows(dtok):
        _require_cuda(dtok)
        B, S, D = dtok.shape
        dzpe = torch.empty(B * (S - 1), D, dtype=dtok.dtype, device=dtok.device)
        ops._op(dtok, 'vit_patch_rows', _ptr(dtok), _ptr(dzpe), B, S, D, ops._dt(dtok))
        return dzpe

    @staticmethod
    def vit_cls_ln_forward(tokens, gamma, beta, eps=1e-6):
        _require_cuda(tokens, gamma, beta)
        B, S, D = tokens.shape
        feat = torch.empty(B, D, dtype=torch.float32, device=tokens.device)
        mean, rstd = ops._scratch(B, tokens.device), ops._scratch(B, tokens.device)
        ops._op(tokens, 'vit_cls_ln_forward', _ptr(tokens), _ptr(gamma), _ptr(beta), _ptr(feat), _ptr(mean), _ptr(rstd), B, S, D, float(eps), ops._dt(tokens))
        return feat, mean, rstd

    @staticmethod
    def vit_cls_ln_backward(dfeat, tokens, mean, rstd, gamma):
        _require_cuda(dfeat, tokens, mean, rstd, gamma)
        B, S, D = tokens.shape
        dtok = torch.empty_like(tokens)
        dgamma, dbeta, partial = ops._scratch(D, tokens.device), ops._scratch(D, tokens.device), ops._scratch(B * 2 * D, tokens.device)
        ops._op(tokens, 'vit_cls_ln_backward', _ptr(dfeat), _ptr(tokens), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(dtok), _ptr(partial), _ptr(dgamma), _ptr(dbeta),
                B, S, D, ops._dt(tokens))
        return dtok, dgamma, dbeta

    @staticmethod
    def vit_map_ln_forward(tokens, gamma, beta, eps=1e-6):
        """The final norm on the patch rows: tokens [B,S,D] -> (map [B,S-1,D] fp32, mean [B*(S-1)], rstd [B*(S-1)])"""
        _require_cuda(tokens, gamma, beta)
        B, S, D = tokens.shape
        rows = B * max(S - 1, 0)
        fmap = torch.empty(B, max(S - 1, 0), D, dtype=torch.float32, device=tokens.device)
        mean, rstd = ops._scratch(max(rows, 1), tokens.device), ops._scratch(max(rows, 1), tokens.device)
        ops._op(tokens, 'vit_map_ln_forward', _ptr(tokens), _ptr(gamma), _ptr(beta), _ptr(fmap), _ptr(mean), _ptr(rstd), B, S, D, float(eps), ops._dt(tokens))
        return fmap, mean[:rows], rstd[:rows]

    @staticmethod
    def vit_map_ln_backward(dfeat, dmap, tokens, mean0, rstd0, meanp, rstdp, gamma):
        """The fused backward of (feat, map): dfeat [B,D] and dmap [B,S-1,D] fp32, either may be None -> (dtok [B,S,D], dgamma, dbeta)"""
        _require_cuda(dfeat, dmap, tokens, mean0, rstd0, meanp, rstdp, gamma)
        B, S, D = tokens.shape
        dtok = torch.empty_like(tokens)
        nblk = max(_lib.load().fsvit_op_vit_map_ln_bwd_blocks(B, S), 1)
        dgamma, dbeta, partial = ops._scratch(D, tokens.device), ops._scratch(D, tokens.device), ops._scratch(nblk * 2 * D, tokens.device)
        ops._op(tokens, 'vit_map_ln_backward', _ptr(dfeat), _ptr(dmap), _ptr(tokens), _ptr(mean0), _ptr(rstd0), _ptr(meanp), _ptr(rstdp), _ptr(gamma), _ptr(dtok),
                _ptr(partial), _ptr(dgamma), _ptr(dbeta), B, S, D, ops._dt(tokens))
        return dtok, dgamma, dbeta

    @staticmethod
    def gelu_train(z, dh=None):
        """gelu(z), or with dh its backward dh * gelu'(z)"""
        _require_cuda(z, dh)
        out = torch.empty_like(z)
        ops._op(z, 'gelu', _ptr(dh), _ptr(z), _ptr(out), z.numel(), ops._dt(z))
        return out

    @staticmethod
    def add_scaled(a, br, scale=None, per_img=0):
        _require_cuda(a, br, scale)
        out = torch.empty_like(br)
        ops._op(br, 'add_scaled', _ptr(a), _ptr(br), _ptr(scale), _ptr(out), br.numel(), int(per_img), ops._dt(br))
        return out

    @staticmethod
    def avgpool_bwd(dfeat, HW, dtype):
        _require_cuda(dfeat)
        B, Cc = dfeat.shape
        dx = torch.empty(B, HW, Cc, dtype=dtype, device=dfeat.device)
        ops._op(dfeat, 'avgpool_bwd', _ptr(dfeat), _ptr(dx), B, HW, Cc, ops._dt(dx))
        return dx

    @staticmethod
    def batch_sum(g):
        """g [B, n] -> [n] fp32"""
        _require_cuda(g)
        out = torch.empty(g.shape[1], dtype=torch.float32, device=g.device)
        ops._op(g, 'batch_sum', _ptr(g), _ptr(out), g.shape[0], g.shape[1], ops._dt(g))
        return out

    @staticmethod
    def bcast_add(x, p):
        _require_cuda(x, p)
        y = torch.empty_like(x)
        ops._op(x, 'bcast_add', _ptr(x), _ptr(p), _ptr(y), x.shape[0], x[0].numel(), ops._dt(x))
        return y

    @staticmethod
    def colsum(a):
        _require_cuda(a)
        M, Cc = a.shape
        out = torch.empty(Cc, dtype=torch.float32, device=a.device)
        partial = ops._scratch(_lib.load().fsvit_op_bn_reduce_blocks(M) * 2 * Cc, a.device)
        ops._op(a, 'colsum', _ptr(a), _ptr(partial), _ptr(out), M, Cc, ops._dt(a))
        return out

    @staticmethod
    def unpatch2(g, B, OH, OW):
        """g [B*OH*OW, 4*C] -> dx [B, 2*OH, 2*OW, C]"""
        _require_cuda(g)
        Cc = g.shape[1] // 4
        dx = torch.empty(B, 2 * OH, 2 * OW, Cc, dtype=g.dtype, device=g.device)
        ops._op(g, 'unpatch2', _ptr(g), _ptr(dx), B, OH, OW, Cc, ops._dt(g))
        return dx

    @staticmethod
    def droppath_scales(masks, keep):
        """masks [ncalls, n_img] fp32, keep: ncalls probabilities -> scales [ncalls, n_img]"""
        _require_cuda(masks)
        scales = torch.empty_like(masks)
        k = (C.c_float * len(keep))(*[float(v) for v in keep])
        ops._op(masks, 'droppath_scales', _ptr(masks), _ptr(scales), masks.shape[0], masks.shape[1], k)
        return scales

    @staticmethod
    def fold_prenorm(W, sa, sb, Kw, dtype):
        """W [N,C] fp32 -> (wf [N,Kw] in `dtype`, bf [N] fp32)"""
        _require_cuda(W, sa, sb)
        N, Cc = W.shape
        wf = torch.empty(N, Kw, dtype=dtype, device=W.device)
        bf = torch.empty(N, dtype=torch.float32, device=W.device)
        ops._op(W, 'fold_prenorm', _ptr(W), _ptr(sa), _ptr(sb), _ptr(wf), _ptr(bf), N, Cc, Kw, ops._dt(wf))
        return wf, bf

    @staticmethod
    def fill_f32(n, v, device):
        out = torch.empty(n, dtype=torch.float32, device=device)
        ops._op(out, 'fill_f32', _ptr(out), float(v), n)
        return out

    @staticmethod
    def scale_copy(x, scale):
        _require_cuda(x)
        out = torch.empty_like(x)
        ops._op(x, 'scale_copy', _ptr(x), _ptr(out), x.numel(), float(scale))
        return out

    # ---- the MFMA side of the training step: weight packs, the conv launchers' training epilogues, the stage-1 ring kernels (fsvit.h)
    ACT_NONE, ACT_GELU, ACT_MUL = 0, 1, 3

    @staticmethod
    def _pack_dt(dtype):
        """-> (fsvit dtype code, torch dtype of the packed buffer, elements per 128-byte K slice); 'bf16x2': two-limb words in a float32-typed tensor"""
        if dtype == 'bf16x2':
            return _lib.BF16X2, torch.float32, 32
        if dtype == torch.float32:
            return _lib.F32, torch.float32, 32
        if dtype == torch.bfloat16:
            return _lib.BF16, torch.bfloat16, 64
        if dtype == torch.float16:
            return _lib.F16, torch.float16, 64          # (refused by the entry: no f16 build of the pack kernel)
        raise TypeError(dtype)

    @staticmethod
    def pack_geometry(shape, groups, mode, bke, hd_rows=1, hdp_rows=1, hd_cols=1, hdp_cols=1):
        """(rows_pad, Kw) as the trainer sizes a pack of a conv weight [O, Ig, KH, KW]: padded rows, padded columns rounded up to the K slice of bke elements"""
        O, Ig, KH, KW = shape
        Ng = O // groups
        if mode == 2:
            rows, K = KH * KW * Ig, Ng
        else:
            rows = (Ng if mode == 0 else Ig) // hd_rows * hdp_rows
            K = KH * KW * (Ig if mode == 0 else Ng) // hd_cols * hdp_cols
        return rows, -(-K // bke) * bke

    @staticmethod
    def pack_weight_multi(jobs, dtype):
        """jobs: dicts(w [O,Ig,KH,KW] fp32, groups, mode[, rows_pad, Kw, hd_rows, hdp_rows, hd_cols, hdp_cols]) -> the packed [groups, rows_pad, Kw] of each, in
        ONE call of launch_pack_weight_multi (any number of jobs: the launcher walks its 40-job table)."""
        code, tdt, bke = ops._pack_dt(dtype)
        ws, outs, fields = [], [], []
        for j in jobs:
            w = j['w']
            _require_cuda(w)
            assert w.dtype == torch.float32 and w.is_contiguous() and w.dim() == 4
            groups, mode = int(j.get('groups', 1)), int(j['mode'])
            hd = [int(j.get(k, 1)) for k in ('hd_rows', 'hdp_rows', 'hd_cols', 'hdp_cols')]
            rows, Kw = ops.pack_geometry(w.shape, groups, mode, bke, *hd)
            rows, Kw = int(j.get('rows_pad') or rows), int(j.get('Kw') or Kw)
            out = torch.full((groups, max(rows, 1), max(Kw, 1)), float('nan'), dtype=tdt, device=w.device)
            ws.append(w)
            outs.append(out)
            fields += [w.shape[0], w.shape[1], w.shape[2], w.shape[3], groups, mode, rows, Kw] + hd
        n = len(jobs)
        wp = (C.c_void_p * n)(*[w.data_ptr() for w in ws])
        op = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
        fl = (C.c_int * (12 * n))(*fields)
        ops._op(ws[0], 'pack_weight_multi', wp, op, fl, n, code)
        return outs

    @staticmethod
    def pack_weight(w, groups=1, mode=0, rows_pad=None, Kw=None, hd_rows=1, hdp_rows=1, hd_cols=1, hdp_cols=1, dtype=torch.bfloat16):
        """One job through fsvit_op_pack_weight: conv weight w [O,Ig,KH,KW] fp32 -> packed [groups, rows_pad, Kw] (mode 0 forward, 1 transposed + flipped
        taps, 2 patch-conv data gradient); dtype torch.float32 | torch.bfloat16 | 'bf16x2'."""
        _require_cuda(w)
        assert w.dtype == torch.float32 and w.is_contiguous() and w.dim() == 4
        code, tdt, bke = ops._pack_dt(dtype)
        rows, kw = ops.pack_geometry(w.shape, groups, mode, bke, hd_rows, hdp_rows, hd_cols, hdp_cols) if mode in (0, 1, 2) else (1, 1)
        rows, kw = int(rows_pad or rows), int(Kw or kw)
        out = torch.full((groups, max(rows, 1), max(kw, 1)), float('nan'), dtype=tdt, device=w.device)
        ops._op(w, 'pack_weight', _ptr(w), _ptr(out), w.shape[0], w.shape[1], w.shape[2], w.shape[3], groups, mode, rows, kw, hd_rows, hdp_rows, hd_cols,
                hdp_cols, code)
        return out

    @staticmethod
    def conv_train(x, w, bias, KH, KW, stride, pad, N, groups, act, with_y2=False, mul=None):
        """launch_conv_gemm with the training epilogues: x NHWC [B,H,W,groups*Cin], w packed [groups][N][Kw] -> (y, y2 | None, route).  act ops.ACT_GELU with
        with_y2: y = GELU(conv + bias) and y2 = the GELU derivative; act ops.ACT_MUL: y = (conv + bias) * mul.  route: 0 conv3x3_halo, 1 gemm256, 2 conv_gemm_v2."""
        _require_cuda(x, w, bias, mul)
        B, H, W, xc = x.shape
        OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
        y = torch.full((B, OH, OW, groups * N), float('nan'), dtype=x.dtype, device=x.device)
        y2 = torch.full_like(y, float('nan')) if with_y2 else None
        route = C.c_int(-1)
        ops._op(x, 'conv_train', _ptr(x), _ptr(w), _ptr(bias), _ptr(mul), _ptr(y), _ptr(y2), B, H, W, xc // groups, xc, KH, KW, stride, pad, N, groups * N,
                w.shape[-1], groups, int(act), ops._dt(x), C.byref(route))
        return y, y2, route.value

    @staticmethod
    def gconv3x3_train(x, w_packed, with_y2=False, mul=None):
        """launch_gconv3x3 with its training epilogues: x NHWC [B,H,W,256] bf16, w_packed [256][Kw] -> (y, y2 | None); with_y2: y = GELU(conv), y2 the
        derivative; mul: y = conv * mul."""
        _require_cuda(x, w_packed, mul)
        B, H, W, _ = x.shape
        y = torch.full_like(x, float('nan'))
        y2 = torch.full_like(x, float('nan')) if with_y2 else None
        ops._op(x, 'gconv3x3_train', _ptr(x), _ptr(w_packed), w_packed.shape[-1], _ptr(y), _ptr(y2), _ptr(mul), B, H, W, ops._dt(x))
        return y, y2

    @staticmethod
    def stage1_block_train(x, w1f, b1f, w2, w3, sa, sb, scale=None, out=None):
        """launch_stage1_ring_block_train: x NHWC [B,H,W,128] bf16, w1f [256,128] / b1f [256] (ops.fold_prenorm), w2 [256,320], w3 [128,256], sa / sb [128] fp32,
        scale [B] fp32 or None -> dict(out, h1, g1, h2, g2, xn) (maps [B,H,W,128 | 256])."""
        _require_cuda(x, w1f, b1f, w2, w3, sa, sb, scale, out)
        B, H, W, _ = x.shape
        nan = lambda c: torch.full((B, H, W, c), float('nan'), dtype=x.dtype, device=x.device)
        r = dict(out=nan(128) if out is None else out, h1=nan(256), g1=nan(256), h2=nan(256), g2=nan(256), xn=nan(128))
        ops._op(x, 'stage1_block_train', _ptr(x), _ptr(r['out']), _ptr(w1f), _ptr(b1f), _ptr(w2), w2.shape[-1], _ptr(w3), _ptr(r['h1']), _ptr(r['g1']),
                _ptr(r['h2']), _ptr(r['g2']), _ptr(r['xn']), _ptr(sa), _ptr(sb), _ptr(scale), B, H, W, ops._dt(x))
        return r

    @staticmethod
    def stage1_block_dgrad(dz3, w3t, w2t, w1t, g2, g1, dxn=None):
        """launch_stage1_ring_dgrad: dz3 NHWC [B,H,W,128] bf16, the transposed packs w3t [256,128], w2t [256,320] (tap-flipped), w1t [128,256], the saved
        derivatives g2 / g1 [B,H,W,256] -> (dxn [B,H,W,128], dz2, dz1 [B,H,W,256])."""
        _require_cuda(dz3, w3t, w2t, w1t, g2, g1, dxn)
        B, H, W, _ = dz3.shape
        nan = lambda c: torch.full((B, H, W, c), float('nan'), dtype=dz3.dtype, device=dz3.device)
        dxn = nan(128) if dxn is None else dxn
        dz2, dz1 = nan(256), nan(256)
        ops._op(dz3, 'stage1_block_dgrad', _ptr(dz3), _ptr(dxn), _ptr(w3t), _ptr(w2t), w2t.shape[-1], _ptr(w1t), _ptr(g2), _ptr(g1), _ptr(dz2), _ptr(dz1),
                B, H, W, ops._dt(dz3))
        return dxn, dz2, dz1

    # ---- DeepEMD head (emd_head.hip): fp32 in every numerics mode
    _emd_ws = {}

    @staticmethod
    def _emd_workspace(E, P, Q, N, Cc, dev):
        need = _lib.load().fsvit_emd_head_workspace_bytes(E, P, Q, N, Cc)
        ws = ops._emd_ws.get(dev)
        if ws is None or ws.numel() < max(need, 16):
            ws = ops._emd_ws[dev] = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        return ws

    @staticmethod
    def emd_head_forward(shot_tok, query_tok, temperature, want_flow=True):
        """shot_tok [E,P,N,C] (the class prototypes' token maps), query_tok [E,Q,N,C] -> (logits [E,Q,P], flow [E,Q,P,N,N] or None, status [E,Q,P] int32)."""
        _require_cuda(shot_tok, query_tok)
        if shot_tok.dim() != 4 or query_tok.dim() != 4 or shot_tok.shape[0] != query_tok.shape[0] or shot_tok.shape[2:] != query_tok.shape[2:]:
            raise ValueError('expected shot_tok [E,P,N,C] and query_tok [E,Q,N,C]')
        s, q = shot_tok.detach().contiguous().float(), query_tok.detach().contiguous().float()
        E, P, N, Cc = s.shape
        Q = q.shape[1]
        dev = s.device
        logits = torch.empty(E, Q, P, dtype=torch.float32, device=dev)
        flow = torch.empty(E, Q, P, N, N, dtype=torch.float32, device=dev) if want_flow else None
        status = torch.empty(E, Q, P, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            ws = ops._emd_workspace(E, P, Q, N, Cc, dev)
            _lib.check(_lib.load().fsvit_emd_head_forward(_ptr(s), _ptr(q), E, P, Q, N, Cc, float(temperature), _ptr(logits), _ptr(flow), _ptr(status),
                                                          _ptr(ws), ws.numel(), _stream_ptr(dev)))
        return logits, flow, status

    @staticmethod
    def emd_head_backward(shot_tok, query_tok, dlogits, flow, temperature):
        """-> (d_shot_tok [E,P,N,C], d_query_tok [E,Q,N,C]); the flows are constants."""
        _require_cuda(shot_tok, query_tok, dlogits, flow)
        s, q = shot_tok.detach().contiguous().float(), query_tok.detach().contiguous().float()
        E, P, N, Cc = s.shape
        Q = q.shape[1]
        dev = s.device
        dl, fl = dlogits.contiguous().float(), flow.contiguous().float()
        if dl.shape != (E, Q, P) or fl.shape != (E, Q, P, N, N):
            raise ValueError('expected dlogits [E,Q,P] and flow [E,Q,P,N,N]')
        ds, dq = torch.empty_like(s), torch.empty_like(q)
        with torch.cuda.device(dev):
            ws = ops._emd_workspace(E, P, Q, N, Cc, dev)
            _lib.check(_lib.load().fsvit_emd_head_backward(_ptr(s), _ptr(q), _ptr(dl), _ptr(fl), E, P, Q, N, Cc, float(temperature), _ptr(ds), _ptr(dq),
                                                           _ptr(ws), ws.numel(), _stream_ptr(dev)))
        return ds, dq

    @staticmethod
    def emd_table_prep(tok, xhat, pooled):
        """Rows of a token-map table: tok [n,N,C] fp32 -> xhat [n,N,C], pooled [n,C] written IN PLACE (contiguous fp32; views of the table's arrays): the
        nodes and token means `emd_head_forward` prepares for the same maps (fsvit_emd_table_prep)."""
        _require_cuda(tok, xhat, pooled)
        if tok.dim() != 3 or xhat.shape != tok.shape or pooled.shape != (tok.shape[0], tok.shape[2]):
            raise ValueError('expected tok [n,N,C], xhat [n,N,C] and pooled [n,C]')
        for t in (tok, xhat, pooled):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError('tok, xhat and pooled must be contiguous float32 tensors (xhat and pooled are written in place)')
        n, N, Cc = tok.shape
        if n:
            with torch.cuda.device(tok.device):
                _lib.check(_lib.load().fsvit_emd_table_prep(_ptr(tok), n, N, Cc, _ptr(xhat), _ptr(pooled), _stream_ptr(tok.device)))
        return xhat, pooled

    @staticmethod
    def emd_head_gather(tok, xhat, pooled, query_slots, temperature, invalid, proto_slots=None, proto_tok=None):
        """The head of `emd_head_forward` over rows of a token-map table: tok / xhat [n_slots,N,C], pooled [n_slots,C] fp32 (emd_table_prep),
        query_slots [E,Q] and either proto_slots [E,P] (int32 / int64 slot numbers, one dtype for both) or a dense proto_tok [E,P,N,C] ->
        (logits [E,Q,P], status [E,Q,P] int32); for the same maps the bits of `emd_head_forward`.  invalid [1] int32 is raised by one per slot outside
        [0, n_slots); the problems of such a slot are NaN with status 0.  Limits: fsvit_emd_head_gather (fsvit.h)."""
        _require_cuda(tok, xhat, pooled, query_slots, invalid, proto_slots, proto_tok)
        if (proto_slots is None) == (proto_tok is None):
            raise ValueError('emd_head_gather: exactly one of proto_slots and proto_tok')
        if tok.dim() != 3 or xhat.shape != tok.shape or pooled.shape != (tok.shape[0], tok.shape[2]):
            raise ValueError('expected tok [n_slots,N,C], xhat [n_slots,N,C] and pooled [n_slots,C]')
        for t in (tok, xhat, pooled):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError('tok, xhat and pooled must be contiguous float32 tensors')
        if query_slots.dim() != 2 or query_slots.dtype not in (torch.int32, torch.int64):
            raise ValueError('expected query_slots [E,Q] int32 / int64')
        if invalid.dtype != torch.int32 or invalid.numel() != 1:
            raise ValueError('invalid: one int32')
        n_slots, N, Cc = tok.shape
        E, Q = query_slots.shape
        qs = query_slots.contiguous()
        ps = pt = None
        if proto_slots is not None:
            if proto_slots.dim() != 2 or proto_slots.shape[0] != E or proto_slots.dtype != qs.dtype:
                raise ValueError('expected proto_slots [E,P] of the dtype of query_slots')
            ps = proto_slots.contiguous()
            P = ps.shape[1]
        else:
            if proto_tok.dim() != 4 or proto_tok.shape[0] != E or tuple(proto_tok.shape[2:]) != (N, Cc):
                raise ValueError('expected proto_tok [E,P,N,C] with the N and C of the table')
            pt = proto_tok.detach().contiguous().float()
            P = pt.shape[1]
        dev = tok.device
        logits = torch.empty(E, Q, P, dtype=torch.float32, device=dev)
        status = torch.empty(E, Q, P, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            lib = _lib.load()
            ws = None
            if pt is not None:
                need = lib.fsvit_emd_head_gather_workspace_bytes(E, P, N, Cc)
                ws = ops._emd_ws.get(dev)
                if ws is None or ws.numel() < max(need, 16):
                    ws = ops._emd_ws[dev] = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            _lib.check(lib.fsvit_emd_head_gather(_ptr(tok), _ptr(xhat), _ptr(pooled), n_slots, _ptr(qs), _ptr(ps), int(qs.dtype == torch.int64), _ptr(pt),
                                                 E, P, Q, N, Cc, float(temperature), _ptr(logits), _ptr(status), _ptr(invalid), _ptr(ws),
                                                 0 if ws is None else ws.numel(), _stream_ptr(dev)))
        return logits, status

    # ---- a bank of class token maps over a labelled support set, and the exact re-rank of a shortlist (emd_head.hip; limits in fsvit.h)
    @staticmethod
    def _f32_dense(what, *ts):
        for t in ts:
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f'{what}: expected contiguous float32 tensors, got {t.dtype} {tuple(t.shape)}')

    @staticmethod
    def emd_bank_accumulate(tok, labels, sum_, count, invalid):
        """tok [S,N,C] (any float type), labels [S] (int32 / int64) added into the bank state in place: sum_ [n_classes,N,C] fp32, count [n_classes]
        int32, invalid [1] int32 (the number of labels outside [0, n_classes); they add nothing else).  Rows of a class are added in ascending index on
        top of the stored sum: two calls over a split give the bits of one."""
        _require_cuda(tok, labels, sum_, count, invalid)
        if tok.dim() != 3 or sum_.dim() != 3 or tuple(tok.shape[1:]) != tuple(sum_.shape[1:]):
            raise ValueError('expected tok [S,N,C] and sum [n_classes,N,C]')
        n_classes, N, Cc = sum_.shape
        ops._f32_dense('emd_bank_accumulate: sum', sum_)
        ops._bank_state(None, count, invalid, n_classes, 0)
        if labels.dtype not in (torch.int32, torch.int64) or labels.dim() != 1 or labels.shape[0] != tok.shape[0]:
            raise ValueError('expected labels [S] int32 / int64 for tok [S,N,C]')
        tok, labels = tok.detach().contiguous().float(), labels.contiguous()
        with torch.cuda.device(tok.device):
            _lib.check(_lib.load().fsvit_emd_bank_accumulate(_ptr(tok), _ptr(labels), int(labels.dtype == torch.int64), tok.shape[0], n_classes, N, Cc,
                                                             _ptr(sum_), _ptr(count), _ptr(invalid), _stream_ptr(tok.device)))

    @staticmethod
    def emd_bank_finalize(sum_, count):
        """-> (tok [n_classes,N,C] = sum / count, xhat [n_classes,N,C] and pooled [n_classes,C]: the bits of emd_table_prep(tok), proto [n_classes,C] =
        F.normalize(pooled), empty [n_classes] int32: 1 where count == 0, all outputs of such a class zero rows)."""
        _require_cuda(sum_, count)
        if sum_.dim() != 3:
            raise ValueError('expected sum [n_classes,N,C]')
        n_classes, N, Cc = sum_.shape
        ops._f32_dense('emd_bank_finalize: sum', sum_)
        ops._bank_state(None, count, None, n_classes, 0)
        dev = sum_.device
        tok, xhat = torch.empty_like(sum_), torch.empty_like(sum_)
        pooled, proto = (torch.empty(n_classes, Cc, dtype=torch.float32, device=dev) for _ in range(2))
        empty = torch.empty(n_classes, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().fsvit_emd_bank_finalize(_ptr(sum_), _ptr(count), n_classes, N, Cc, _ptr(tok), _ptr(xhat), _ptr(pooled), _ptr(proto),
                                                           _ptr(empty), _stream_ptr(dev)))
        return tok, xhat, pooled, proto, empty

    @staticmethod
    def check_shortlist(k, shortlist, what):
        """the list lengths of a shortlist re-rank: ints with 1 <= k <= shortlist <= 32 (shortlist None: the caller's default, only k is checked); the
        arguments alone decide, so callers check them before they look at a device"""
        ops.check_topk_k(k, what)
        if shortlist is None:
            return
        if isinstance(shortlist, bool) or not isinstance(shortlist, int) or not 1 <= shortlist <= 32:
            raise ValueError(f'{what}: shortlist = {shortlist!r} is outside [1, 32]')
        if k > shortlist:
            raise ValueError(f'{what}: k = {k} exceeds the shortlist of {shortlist}')

    @staticmethod
    def emd_rerank(query, bank, cand, temperature, k, status_count=None, invalid=None, want_logits=False):
        """query = (tok [Q,N,C], xhat [Q,N,C], pooled [Q,C]) as emd_table_prep writes them, bank = (tok, xhat, pooled, empty) of emd_bank_finalize
        (proto is not read), cand [Q,M] int32 class numbers (-1: an empty slot) -> (classes [Q,k] int32, values [Q,k], prob [Q,k], logits [Q,M] in
        candidate order or None, status_count [1] int32, invalid [1] int32).  Only the Q * M listed problems are solved (the bits of emd_head_gather
        for the same rows); the row is ranked by larger logit, lower class, lower position, empty slots (class -1, -inf) last; prob is the softmax
        over the row's M logits.  status_count / invalid are ADDED to when given (problems at a loop bound of the solver; candidates outside
        [-1, n_classes), which are treated as -1).  1 <= k <= M <= 32."""
        ops.check_topk_k(k, 'emd_rerank')
        _require_cuda(*query, *bank, cand, status_count, invalid)
        qtok, qxhat, qpooled = query
        btok, bxhat, bpooled, empty = bank
        if qtok.dim() != 3 or btok.dim() != 3 or tuple(qtok.shape[1:]) != tuple(btok.shape[1:]):
            raise ValueError('expected query tok [Q,N,C] and bank tok [n_classes,N,C]')
        Q, N, Cc = qtok.shape
        n_classes = btok.shape[0]
        if qxhat.shape != qtok.shape or tuple(qpooled.shape) != (Q, Cc) or bxhat.shape != btok.shape or tuple(bpooled.shape) != (n_classes, Cc):
            raise ValueError('expected xhat of the shape of tok and pooled [.,C] on either side')
        ops._f32_dense('emd_rerank', qtok, qxhat, qpooled, btok, bxhat, bpooled)
        if empty.dtype != torch.int32 or tuple(empty.shape) != (n_classes,) or not empty.is_contiguous():
            raise ValueError('empty: contiguous int32 [n_classes]')
        if cand.dtype != torch.int32 or cand.dim() != 2 or cand.shape[0] != Q:
            raise ValueError('expected cand [Q,M] int32')
        M = cand.shape[1]
        if not k <= M <= 32:
            raise ValueError(f'emd_rerank: k = {k}, M = {M}: 1 <= k <= M <= 32')
        cand = cand.contiguous()
        dev = qtok.device
        status_count = torch.zeros(1, dtype=torch.int32, device=dev) if status_count is None else status_count
        invalid = torch.zeros(1, dtype=torch.int32, device=dev) if invalid is None else invalid
        ops._bank_state(None, None, status_count, 0, 0)
        ops._bank_state(None, None, invalid, 0, 0)
        classes = torch.empty(Q, k, dtype=torch.int32, device=dev)
        values, prob = torch.empty(Q, k, dtype=torch.float32, device=dev), torch.empty(Q, k, dtype=torch.float32, device=dev)
        logits = torch.empty(Q, M, dtype=torch.float32, device=dev) if want_logits else None
        with torch.cuda.device(dev):
            _lib.check(_lib.load().fsvit_emd_rerank(_ptr(qtok), _ptr(qxhat), _ptr(qpooled), Q, _ptr(btok), _ptr(bxhat), _ptr(bpooled), _ptr(empty), n_classes,
                                                    _ptr(cand), M, N, Cc, float(temperature), k, _ptr(logits), _ptr(classes), _ptr(values), _ptr(prob),
                                                    _ptr(status_count), _ptr(invalid), _stream_ptr(dev)))
        return classes, values, prob, logits, status_count, invalid

    _emd_sfc_ws = {}

    @staticmethod
    def emd_sfc_steps(support, label, ids, sfc, buf=None, status_count=None, *, temperature, lr, momentum=0.9, dampening=0.9, first=True):
        """Mini-batch updates of the 5-shot SFC fine-tune in one launch, one workgroup per episode (fsvit_emd_sfc_steps): support [E,n,N,C] (the support
        maps, shot-major), label [n], ids a CPU int tensor [steps,E,bs] of support indices (-1: an empty slot of a partial batch; models.deepemd.
        sfc_step_table), sfc [E,way,N,C] float32 contiguous on the device, updated IN PLACE, as are buf (the momentum buffer; None: a fresh one, which
        needs first=True) and status_count [E] int32 (None: zeros).  first: step 0 of this call is the first update of the fine-tune (buf = grad).
        -> (sfc, buf, status_count)."""
        _require_cuda(support, label, sfc, buf, status_count)
        if not isinstance(ids, torch.Tensor) or ids.device.type != 'cpu' or ids.dtype not in (torch.int32, torch.int64) or ids.dim() != 3:
            raise ValueError('expected ids as a CPU int32 / int64 tensor [steps,E,bs]')
        if support.dim() != 4 or sfc.dim() != 4 or sfc.shape[0] != support.shape[0] or sfc.shape[2:] != support.shape[2:]:
            raise ValueError('expected support [E,n,N,C] and sfc [E,way,N,C]')
        E, n, N, Cc = support.shape
        way = sfc.shape[1]
        steps, bs = ids.shape[0], ids.shape[2]
        if ids.shape[1] != E or label.shape != (n,):
            raise ValueError('expected ids [steps,E,bs] and label [n]')
        if ids.numel() and (int(ids.min()) < -1 or int(ids.max()) >= n):
            raise ValueError(f'ids must lie in [-1, {n}): found {int(ids.min())} .. {int(ids.max())}')
        if sfc.dtype != torch.float32 or not sfc.is_contiguous():
            raise ValueError('sfc must be a contiguous float32 tensor (it is updated in place)')
        if buf is None:
            if not first:
                raise ValueError('first=False needs the buf of the earlier steps')
            buf = torch.zeros_like(sfc)
        if buf.shape != sfc.shape or buf.dtype != torch.float32 or not buf.is_contiguous():
            raise ValueError('buf must be a contiguous float32 tensor of the shape of sfc')
        dev = sfc.device
        if status_count is None:
            status_count = torch.zeros(E, dtype=torch.int32, device=dev)
        if status_count.shape != (E,) or status_count.dtype != torch.int32:
            raise ValueError('status_count must be int32 [E]')
        if E == 0 or steps == 0:
            return sfc, buf, status_count
        s = support.detach().contiguous().float()
        lab = label.to(device=dev, dtype=torch.int32).contiguous()
        table = ids.to(torch.int32).contiguous().to(dev)
        with torch.cuda.device(dev):
            lib = _lib.load()
            need = lib.fsvit_emd_sfc_workspace_bytes(E, way, n, bs, N, Cc)
            ws = ops._emd_sfc_ws.get(dev)
            if ws is None or ws.numel() < max(need, 16):
                ws = ops._emd_sfc_ws[dev] = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            _lib.check(lib.fsvit_emd_sfc_steps(_ptr(s), _ptr(lab), _ptr(table), steps, int(bool(first)), E, way, n, bs, N, Cc, float(temperature), float(lr),
                                               float(momentum), float(dampening), _ptr(sfc), _ptr(buf), _ptr(status_count), _ptr(ws), ws.numel(),
                                               _stream_ptr(dev)))
        return sfc, buf, status_count

    @staticmethod
    def emd_solve(cost, w1, w2, counts=False):
        """The transport solver alone: cost [B,N,N], w1 / w2 [B,N] with equal sums -> (flow [B,N,N], status [B] int32[, augmentations [B] int32])."""
        _require_cuda(cost, w1, w2)
        c, a, b = cost.contiguous().float(), w1.contiguous().float(), w2.contiguous().float()
        if c.dim() != 3 or c.shape[1] != c.shape[2] or a.shape != c.shape[:2] or b.shape != c.shape[:2]:
            raise ValueError('expected cost [B,N,N] and w1, w2 [B,N]')
        B, N = a.shape
        flow = torch.empty_like(c)
        status = torch.empty(B, dtype=torch.int32, device=c.device)
        with torch.cuda.device(c.device):
            if counts:
                n_aug = torch.empty(B, dtype=torch.int32, device=c.device)
                _lib.check(_lib.load().fsvit_op_emd_solve_counts(_ptr(c), _ptr(a), _ptr(b), B, N, _ptr(flow), _ptr(status), _ptr(n_aug), _stream_ptr(c.device)))
                return flow, status, n_aug
            _lib.check(_lib.load().fsvit_op_emd_solve(_ptr(c), _ptr(a), _ptr(b), B, N, _ptr(flow), _ptr(status), _stream_ptr(c.device)))
        return flow, status
