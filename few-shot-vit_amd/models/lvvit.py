"""LV-ViT encoder `lvvit_micro_80` with the reference's constructor / state-dict surface (meta_tuning_sun_m/models/lvvit.py:277-318,
:413-546, factory :583) and an MI355X-native eval forward (engine.LvvitEngine, libfsvit.so).

The nn.Module tree only owns parameters and buffers under the reference's key names (`cls_token`, `pos_embed`,
`patch_embed.{conv1,bn1,conv2,bn2,conv3,bn3,downsample.0,downsample.1,proj}.*`, `blocks.N.{norm1,attn.qkv,attn.proj,norm2,mlp.fc1,mlp.fc2}.*`,
`norm.*`; 118 entries, no qkv bias), so checkpoints saved by the reference load unchanged.  Eval runs on the HIP engine; training is not
built (the 96-channel stem has no weight-gradient kernel yet) and raises NotImplementedError."""
import torch
import torch.nn as nn

from ._host import EngineHost
from .models import register

_NO_TRAIN = ('fsvit: LV-ViT (lvvit_micro_80) is built for evaluation only - training, meta-tuning and distillation of this encoder '
             'are not implemented')


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
    _engine_cls = 'LvvitEngine'

    def __init__(self, img_size=80, embed_dim=384, depth=8, num_heads=6, mlp_ratio=3., stem_channels=96, skip_lam=2., ln_eps=1e-5,
                 numerics=None, return_map=False):
        super().__init__()
        if img_size != 80:
            raise NotImplementedError('fsvit: LV-ViT has a fixed 5 x 5 patch grid (lvvit.py:290, num_patches = 25): img_size must be 80')
        self.cfg = dict(img_size=img_size, stem_channels=stem_channels, embed_dim=embed_dim, depth=depth, num_heads=num_heads,
                        mlp_ratio=mlp_ratio, skip_lam=skip_lam, ln_eps=ln_eps, bn_eps=1e-5)
        self.numerics = numerics
        self.img_size = img_size
        self.return_map = bool(return_map)
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
        raise NotImplementedError(_NO_TRAIN)

    def forward(self, x):
        """[B,3,80,80] fp32 -> [B,embed_dim] = norm(tokens)[:, 0] (lvvit.py:529-546), eval mode on the packed engine."""
        if self.training:
            raise NotImplementedError(_NO_TRAIN)
        if self.return_map:
            raise NotImplementedError('fsvit: LV-ViT returns the cls feature only; the (map, pooled) output of the classifier / distillation '
                                      'phase is not built (evaluate a teacher through load_encoder + meta-baseline)')
        return self.engine().forward(x)


@register('lvvit_micro_80')
def lvvit_micro_80(pretrained=False, **kwargs):
    """lvvit.py:583-587: embed_dim 384, depth 8, 6 heads, mlp_ratio 3, skip_lam 2 (drop_path_rate / mix_token / return_dense only act in
    training)."""
    if pretrained:
        raise NotImplementedError('pretrained LV-ViT weights are loaded through load_state_dict (no network here)')
    for k in ('drop_path_rate', 'mix_token', 'return_dense'):
        kwargs.pop(k, None)
    return LvVit(**kwargs)
