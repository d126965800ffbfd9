"""'meta-baseline': cosine-prototype few-shot classifier over an encoder
(surface of test_phase/models/meta_baseline.py:10-47)."""
import torch
import torch.nn as nn

from ..episodic import head_temp
from .models import make as _make
from .models import register


@register('meta-baseline')
class MetaBaseline(nn.Module):

    def __init__(self, encoder, encoder_args={}, method='cos', temp=10., temp_learnable=True):
        super().__init__()
        self.encoder = _make(encoder, **encoder_args)
        self.method = method
        if temp_learnable:
            self.temp = nn.Parameter(torch.tensor(temp))
        else:
            self.temp = temp

    def forward(self, x_shot, x_query):
        """x_shot [E,way,shot,C,H,W], x_query [E,way*query,C,H,W] -> logits [E,way*query,way].
        Dim 0 stays the episode axis.  Eval mode runs encoder + head through the HIP engine in one
        C-ABI call (fsvit_meta_baseline_forward)."""
        if self.method not in ('cos', 'sqr'):
            raise ValueError(self.method)
        if x_shot.dim() != 6 or x_query.dim() != 5:
            raise ValueError('expected x_shot [E,way,shot,C,H,W] and x_query [E,Q,C,H,W]')
        if self.training:
            return self._forward_train(x_shot, x_query)
        return self._forward_eval(x_shot, x_query)

    def _forward_train(self, x_shot, x_query, label=None):
        """The meta-tuning step's forward (train_meta.py:167): one encoder pass over shot + query images of all
        episodes (so BatchNorm sees the whole batch, meta_baseline.py:31), then the differentiable head ('cos' or 'sqr')."""
        if not hasattr(self.encoder, 'trainer'):
            raise NotImplementedError('fsvit: the training path is built for the Visformer, ViT / DeiT and LV-ViT encoders')
        from ..autograd import ProtoHeadFn
        E, way, shot = x_shot.shape[:3]
        Q = x_query.shape[1]
        img = x_shot.shape[-3:]
        x_tot = self.encoder(torch.cat([x_shot.reshape(-1, *img), x_query.reshape(-1, *img)], dim=0))
        if isinstance(x_tot, tuple):                       # distillation-phase encoder: `_, x_tot = self.encoder(...)` (sun_meta_training/models/meta_baseline.py:31)
            x_tot = x_tot[1]
        n_shot = E * way * shot
        f_shot = x_tot[:n_shot].view(E, way, shot, -1)
        f_query = x_tot[n_shot:].view(E, Q, -1)
        temp = self.temp if isinstance(self.temp, torch.Tensor) else torch.tensor(float(self.temp))      # (a host scalar: passed by value)
        if label is not None:
            from ..autograd import ProtoHeadCEFn
            return ProtoHeadCEFn.apply(f_shot, f_query, temp, label, self.method)
        return ProtoHeadFn.apply(f_shot, f_query, temp, self.method)

    def forward_loss(self, x_shot, x_query, label):
        """Training only: (loss, acc, logits) of train_meta.py:167-169 - `logits = model(x_shot, x_query).view(-1, n_way)`, `F.cross_entropy(logits, label)`,
        `utils.compute_acc(logits, label)` - with head, loss and accuracy in one launch (fsvit_proto_head_ce).  loss / acc are 0-d device tensors."""
        if not self.training:
            raise RuntimeError('forward_loss is the training-step entry; eval mode returns logits from forward()')
        if x_shot.dim() != 6 or x_query.dim() != 5:
            raise ValueError('expected x_shot [E,way,shot,C,H,W] and x_query [E,Q,C,H,W]')
        if self.method not in ('cos', 'sqr'):
            raise ValueError(self.method)
        return self._forward_train(x_shot, x_query, label)

    # ---- a labelled support set of any shape: encode once into a PrototypeBank, query many times (eval mode only)
    def _encode_eval(self, x, what):
        if self.training:
            raise RuntimeError(f'MetaBaseline.{what} is an eval-mode entry: call model.eval() first')
        if self.method not in ('cos', 'sqr'):
            raise ValueError(self.method)
        if x.dim() != 4:
            raise ValueError(f'{what}: expected images [N,3,H,W]')
        if not x.is_cuda:
            raise RuntimeError('fsvit: MetaBaseline.%s got images on %s; the HIP engine needs an MI355X (no CPU fallback)' % (what, x.device))
        # the engine's own chunks; its output is the pooled feature also for encoders whose module forward returns (map, feat)
        return self.encoder.engine().forward(x)

    def fit(self, x_support, y_support, n_classes=None, bank=None):
        """x_support [S,3,H,W], y_support [S] integer labels -> PrototypeBank holding them.  `bank`: extend this one instead of making one; otherwise
        `n_classes` (None: int(y_support.max()) + 1, one device read) sizes a new bank with the model's method."""
        from .proto_bank import PrototypeBank
        feat = self._encode_eval(x_support, 'fit')
        y = y_support.to(feat.device)
        if y.dim() != 1 or y.shape[0] != feat.shape[0]:
            raise ValueError('fit: expected one label per support image')
        if bank is None:
            if n_classes is None:
                n_classes = int(y.max()) + 1
            bank = PrototypeBank(n_classes, feat.shape[1], self.method, feat.device)
        elif bank.method != self.method or bank.dim != feat.shape[1]:
            raise ValueError(f'fit: the bank is {bank.method!r} x {bank.dim}, the model {self.method!r} x {feat.shape[1]}')
        return bank.add(feat, y)

    def predict(self, bank, x_query):
        """x_query [Q,3,H,W] -> logits [Q, bank.n_classes] with the model's temperature (read on the device when it is a parameter) and method"""
        feat = self._encode_eval(x_query, 'predict')
        if bank.method != self.method:
            raise ValueError(f'predict: the bank was built for {bank.method!r}, the model scores with {self.method!r}')
        temp = head_temp(self, on_device=True)
        return bank.logits(feat, temp)

    def predict_topk(self, bank, x_query, k):
        """x_query [Q,3,H,W] -> (classes [Q,k] int64, logits [Q,k], prob [Q,k]) of PrototypeBank.topk: the head of a stable descending sort of
        predict(bank, x_query)'s rows and the softmax probabilities of those classes, without the [Q, bank.n_classes] matrix.  1 <= k <= 32."""
        from ..engine import ops
        ops.check_topk_k(k, 'predict_topk')
        feat = self._encode_eval(x_query, 'predict_topk')
        if bank.method != self.method:
            raise ValueError(f'predict_topk: the bank was built for {bank.method!r}, the model scores with {self.method!r}')
        temp = head_temp(self, on_device=True)
        return bank.topk(feat, k, temp)

    def _forward_eval(self, x_shot, x_query):
        engine = self.encoder.engine()
        return engine.meta_baseline_forward(x_shot, x_query, head_temp(self), self.method)
