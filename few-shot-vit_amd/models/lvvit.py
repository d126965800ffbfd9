"""LV-ViT encoder `lvvit_micro_80` with the reference's constructor / state-dict surface (meta_tuning_sun_m/models/lvvit.py:277-318,
:413-546, factory :583) and an MI355X-native eval forward (engine.LvvitEngine, libfsvit.so).

The nn.Module tree only owns parameters and buffers under the reference's key names (`cls_token`, `pos_embed`,
`patch_embed.{conv1,bn1,conv2,bn2,conv3,bn3,downsample.0,downsample.1,proj}.*`, `blocks.N.{norm1,attn.qkv,attn.proj,norm2,mlp.fc1,mlp.fc2}.*`,
`norm.*`; 118 entries, no qkv bias), so checkpoints saved by the reference load unchanged.  Eval runs on engine.LvvitEngine, model.train() on
engine.LvvitTrainer (fsvit_lvvit_train_forward / _backward: batch-statistics or frozen BatchNorm in the stem, DropPath, the 1 / skip_lam branch scale,
every parameter gradient).  Neither has a CPU form: a train-mode call on host tensors raises NotImplementedError.

`return_map=True` is the encoder of the classifier / distillation phases (sun_meta_training/models/lvvit.py:529-552, which differs from the file above in
its return line only): forward returns `(x_local [B,embed_dim,5,5], x1 [B,embed_dim])`, the final norm's patch rows next to the cls feature - eval through
LvvitEngine.forward_map, train through autograd.LvvitTrainMapFn (fsvit_lvvit_train_tokens / fsvit_lvvit_train_set_token_grad)."""
import torch
import torch.nn as nn

from ._host import EngineHost
from .models import register

_NO_CPU_TRAIN = ('fsvit: LV-ViT (lvvit_micro_80) trains on the HIP trainer only - the training path has no CPU form, and this call has tensors on %s '
                 '(move the model and its input to an MI355X)')


class _Attention(nn.Module):
    def __init__(self, dim, heads, head_dim):
        super().__init__()
        self.qkv = nn.Linear(dim, 3 * heads * head_dim, bias=False)          # lvvit.py:116, qkv_bias=False
        self.proj = nn.Linear(heads * head_dim, dim)


class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class _Block(nn.Module):
    def __init__(self, dim, heads, mlp_ratio, eps):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.attn = _Attention(dim, heads, dim // heads)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio))


class _ConvBlock(nn.Module):
    """lvvit.py:277-318: conv1 s2 -> bn1 -> LeakyReLU(0.1) -> conv2 -> bn2 -> LeakyReLU -> conv3 -> bn3, + downsample(x), LeakyReLU, MaxPool2d(2),
    proj (4x4 / stride 4)."""

    def __init__(self, hidden, planes):
        super().__init__()
        self.conv1 = nn.Conv2d(3, hidden, 3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(hidden)
        self.conv2 = nn.Conv2d(hidden, hidden, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(hidden)
        self.conv3 = nn.Conv2d(hidden, hidden, 3, padding=1, bias=False)
        self.bn3 = nn.BatchNorm2d(hidden)
        self.downsample = nn.Sequential(nn.Conv2d(3, hidden, 3, stride=2, padding=1, bias=False), nn.BatchNorm2d(hidden))
        self.proj = nn.Conv2d(hidden, planes, kernel_size=4, stride=4)
        self.num_patches = 25


class LvVit(EngineHost, nn.Module):
    _engine_cls, _trainer_cls = 'LvvitEngine', 'LvvitTrainer'

    def __init__(self, img_size=80, embed_dim=384, depth=8, num_heads=6, mlp_ratio=3., stem_channels=96, skip_lam=2., ln_eps=1e-5,
                 drop_path_rate=0., numerics=None, return_map=False):
        super().__init__()
        if img_size != 80:
            raise NotImplementedError('fsvit: LV-ViT has a fixed 5 x 5 patch grid (lvvit.py:290, num_patches = 25): img_size must be 80')
        self.cfg = dict(img_size=img_size, stem_channels=stem_channels, embed_dim=embed_dim, depth=depth, num_heads=num_heads,
                        mlp_ratio=mlp_ratio, skip_lam=skip_lam, ln_eps=ln_eps, bn_eps=1e-5)
        self.numerics = numerics
        self.img_size = img_size
        self.return_map = bool(return_map)
        self.drop_path_rate = float(drop_path_rate)                          # per-block rates get_dpr(rate, depth, 'linear') (lvvit.py:401-404, :453)
        self.out_dim = self.num_features = self.embed_dim = embed_dim        # lvvit.py:432
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, 26, embed_dim))
        self.patch_embed = _ConvBlock(stem_channels, embed_dim)
        self.blocks = nn.ModuleList([_Block(embed_dim, num_heads, mlp_ratio, ln_eps) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=ln_eps)
        nn.init.trunc_normal_(self.pos_embed, std=.02)                       # lvvit.py:475-488
        nn.init.trunc_normal_(self.cls_token, std=.02)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=.02)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.LayerNorm):
                nn.init.constant_(m.bias, 0)
                nn.init.constant_(m.weight, 1.0)

    def trainer(self):
        if self.pos_embed.device.type != 'cuda':
            raise NotImplementedError(_NO_CPU_TRAIN % self.pos_embed.device)
        return super().trainer()

    def draw_droppath_masks(self, n_img, device):
        """The reference's DropPath (lvvit.py drop_path): floor(keep_prob + U[0,1)) per sample, drawn per block in forward order (attention branch, then Mlp)."""
        keep = self.trainer().droppath_keep(self.drop_path_rate)
        if not keep:
            return None
        return torch.rand(len(keep), n_img, device=device).add_(torch.tensor(keep, device=device).unsqueeze(1)).floor_()

    def forward(self, x, droppath_masks=None):
        """[B,3,80,80] fp32 -> [B,embed_dim] = norm(tokens)[:, 0] (lvvit.py:529-546); with return_map (x_local [B,embed_dim,5,5], x1 [B,embed_dim]), x_local
        a view of the token-major patch rows.  eval: packed engine; train: the HIP trainer through the autograd bridge of the other encoders
        (`droppath_masks` overrides the random draws)."""
        if not self.training:
            if not self.return_map:
                return self.engine().forward(x)
            tokens, feat = self.engine().forward_map(x)
            return self._as_map(tokens), feat
        if self.pos_embed.device.type != 'cuda' or not x.is_cuda:
            raise NotImplementedError(_NO_CPU_TRAIN % (self.pos_embed.device if self.pos_embed.device.type != 'cuda' else x.device))
        assert x.shape[-2] == self.img_size and x.shape[-1] == self.img_size, \
            f"Input image size ({x.shape[-2]}*{x.shape[-1]}) doesn't match model ({self.img_size}*{self.img_size})."
        bn_modes = {m.training for m in self.modules() if isinstance(m, nn.BatchNorm2d)}
        if len(bn_modes) > 1:
            raise NotImplementedError('fsvit: BatchNorm layers must be all in train mode or all frozen (utils.freeze_bn) inside a training step')
        frozen = bn_modes == {False}                    # utils.freeze_bn (train_meta.py:156-157): running statistics normalise, nothing is updated
        trainer = self.trainer()
        trainer.set_freeze_bn(frozen)
        from ..autograd import LvvitTrainMapFn, VisformerTrainFn
        named = [(k, p) for k, p in self.named_parameters()]
        names = tuple(k for k, _ in named)
        buffers = {k: b for k, b in self.named_buffers() if not k.endswith('num_batches_tracked')}
        masks = droppath_masks if droppath_masks is not None else self.draw_droppath_masks(x.shape[0], x.device)
        trainer.grad_sink = getattr(self, '_grad_sink', None)       # parallel.GradBucket: gradients land in the flat all-reduce buffer
        if self.return_map:
            tokens, feat = LvvitTrainMapFn.apply(x, trainer, names, buffers, self.drop_path_rate, masks, *[p for _, p in named])
        else:
            feat = VisformerTrainFn.apply(x, trainer, names, buffers, self.drop_path_rate, masks, *[p for _, p in named])
        if not frozen:      # nn.BatchNorm2d counts its train-mode forwards
            torch._foreach_add_([b for k, b in self.named_buffers() if k.endswith('num_batches_tracked')], 1)
        return (self._as_map(tokens), feat) if self.return_map else feat

    @staticmethod
    def _as_map(tokens):
        """tokens [B,25,D] token-major -> the reference's x_local [B,D,5,5] (lvvit.py:550-551), as a view"""
        B, T, D = tokens.shape
        return tokens.permute(0, 2, 1).reshape(B, D, 5, 5)


@register('lvvit_micro_80')
def lvvit_micro_80(pretrained=False, **kwargs):
    """lvvit.py:583-587: embed_dim 384, depth 8, 6 heads, mlp_ratio 3, skip_lam 2, drop_path_rate 0.5 (acts in training only).  mix_token /
    return_dense are dead code in the reference (commented out): accepted and ignored."""
    if pretrained:
        raise NotImplementedError('pretrained LV-ViT weights are loaded through load_state_dict (no network here)')
    for k in ('mix_token', 'return_dense'):
        kwargs.pop(k, None)
    kwargs.setdefault('drop_path_rate', 0.5)
    return LvVit(**kwargs)
