"""'deepemd': the SUN-D few-shot head - a query is scored against a class by the earth mover's distance between the token maps of the
two images (surface of meta_tuning_sun_d/Models/models/Network.py:9-204 with `solver: opencv`).

The encoder is one of this package's encoders built with return_map=True; the head runs on the HIP kernels of csrc/emd_head.hip (node
preparation, cost / weights / exact transport solver per (query, proto) pair, the backward with the flows as constants, and - with
`sfc_fused=True` - the 5-shot SFC fine-tune as one on-device loop per episode).  State-dict keys
are the reference's (`encoder.*`), so the `params` of a SUN-D checkpoint load.
"""
import torch
import torch.nn as nn

from .models import make as _make
from .models import register

MAX_NODES = 32          # one lane per node on either side of the transportation problem


def check_status_count(count) -> None:
    """Raise when any transportation problem reached one of the solver's loop bounds (its logit is then not an optimum).  `count` is the
    accumulated status sum: a Python int or a tensor (reading a device tensor is the one synchronisation of an evaluation)."""
    n = int(count.sum().item()) if isinstance(count, torch.Tensor) else int(count)
    if n != 0:
        raise RuntimeError(f'fsvit: {n} DeepEMD transportation problem(s) stopped at a loop bound of the solver (status 1); their logits are not optimal')


def encoder_state_dict(checkpoint, model_keys=None):
    """load_model (meta_tuning_sun_d/Models/utils.py:76-99) up to the load itself: the checkpoint's `model_sd` or else `params` (or the mapping
    itself), without `temp`, the DataParallel prefix `module.` stripped, keys of a bare pre-trained encoder prefixed with `encoder.`, and then the
    `encoder.*` keys only (with `model_keys`: those the model has, as the reference's `k in model_dict`).  Following load_model, a checkpoint of bare
    keys is accepted and `encoder.*` keys the model lacks are dropped silently: such a checkpoint no longer fails the strict load that
    eval_deepemd.load_params did before this helper; a MISSING encoder key still fails it."""
    sd = checkpoint.get('model_sd', checkpoint.get('params', checkpoint)) if isinstance(checkpoint, dict) else checkpoint
    sd = {k: v for k, v in sd.items() if k != 'temp'}
    sd = {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in sd.items()}
    if sd and not any(k.startswith('encoder.') for k in sd):
        sd = {'encoder.' + k: v for k, v in sd.items()}
    return {k: v for k, v in sd.items() if k.startswith('encoder.') and (model_keys is None or k in model_keys)}


def load_encoder_params(model, path):
    """Load the encoder of a SUN-D / pre-training checkpoint file into a DeepEMD model (strict: every encoder key must be there)."""
    model.load_state_dict(encoder_state_dict(torch.load(path, map_location='cpu'), set(model.state_dict().keys())), strict=True)
    return model


SFC_CHUNK = 100        # mini-batch updates per launch of the fused SFC fine-tune (DESIGN.md 4f has the launch time)


def sfc_step_table(perms, bs):
    """The mini-batches of get_sfc in its loop order, for ops.emd_sfc_steps: perms [steps, E, n] (one permutation of the n support images per update
    step and episode) -> a CPU int32 table [steps * ceil(n / bs), E, bs]; row k * ceil(n / bs) + j holds perms[k, :, j * bs:(j + 1) * bs], and the
    slots a partial last batch leaves empty hold -1.  Pure torch, runs on the CPU."""
    perms = torch.as_tensor(perms).to('cpu', torch.int32)
    steps, E, n = perms.shape
    per = -(-n // bs)
    table = torch.full((steps, E, per * bs), -1, dtype=torch.int32)
    table[:, :, :n] = perms
    return table.reshape(steps, E, per, bs).permute(0, 2, 1, 3).reshape(steps * per, E, bs).contiguous()


@register('deepemd')
class DeepEMD(nn.Module):

    def __init__(self, encoder, encoder_args={}, temperature=12.5, metric='cosine', norm='center', deepemd='fcn', feature_pyramid=None,
                 solver='opencv', form=None, sfc_lr=100., sfc_update_step=100, sfc_bs=4, sfc_fused=False):
        super().__init__()
        if feature_pyramid is not None:
            raise NotImplementedError('fsvit: DeepEMD feature_pyramid is not built (DESIGN.md 7)')
        if metric != 'cosine':
            raise NotImplementedError(f"fsvit: DeepEMD metric {metric!r}: the head is built for 'cosine'")
        if solver != 'opencv' or form is not None:
            raise NotImplementedError("fsvit: the DeepEMD head solves the transport LP exactly with constant flows (`solver: opencv`); qpth / form are not built")
        if norm != 'center':
            raise NotImplementedError(f"fsvit: DeepEMD norm {norm!r}: the node preparation kernel centres over channels ('center')")
        if deepemd not in ('fcn', 'grid', 'sampling'):
            raise ValueError(deepemd)
        self.encoder = _make(encoder, **{**encoder_args, 'return_map': True})
        self.temperature = float(temperature)
        self.deepemd = deepemd
        self.sfc_lr, self.sfc_update_step, self.sfc_bs = float(sfc_lr), int(sfc_update_step), int(sfc_bs)
        self.sfc_fused = bool(sfc_fused)   # get_sfc as one on-device loop (emd_sfc_kernel) instead of one head forward / backward pair per mini-batch
        self.sfc_generator = None          # torch.Generator of get_sfc's permutations inside forward (None: the global one)
        self._status_count = None          # device int64 scalar: status sum of every head call since the last check_status()

    # ---- status: accumulated on the device, read once per evaluation
    def add_status(self, status):
        s = status.sum(dtype=torch.int64)
        self._status_count = s if self._status_count is None else self._status_count.to(s.device) + s

    def check_status(self):
        count, self._status_count = self._status_count, None
        if count is not None:
            check_status_count(count)

    # ---- nodes
    def encode(self, x, patches):
        """[B,3,H,W] -> token map [B,N,C] (fcn); [B,n_patch,3,H,W] -> the pooled feature of every patch [B,n_patch,C] (grid / sampling, :179-187)."""
        if patches:
            B, n_patch = x.shape[:2]
            _, feat = self.encoder(x.reshape(-1, *x.shape[2:]))
            return feat.reshape(B, n_patch, -1)
        fmap, _ = self.encoder(x)
        return fmap.flatten(2).transpose(1, 2).contiguous()

    def forward(self, x_shot, x_query):
        """x_shot [E,way,shot,3,H,W], x_query [E,Q,3,H,W] -> logits [E,Q,way]; 'grid' / 'sampling' take one more patch axis before the image axes."""
        patches = self.deepemd != 'fcn'
        nd = 1 if patches else 0
        if x_shot.dim() != 6 + nd or x_query.dim() != 5 + nd:
            raise ValueError('expected x_shot [E,way,shot,(n_patch,)3,H,W] and x_query [E,Q,(n_patch,)3,H,W]')
        E, way, shot = x_shot.shape[:3]
        Q = x_query.shape[1]
        img = x_shot.shape[3:]
        if patches and img[0] > MAX_NODES:
            raise NotImplementedError(f'fsvit: {img[0]} patches per image; the DeepEMD head holds at most {MAX_NODES} nodes')
        # one encoder pass over shot + query images of all episodes (train mode: BatchNorm sees the whole batch, one forward per backward)
        tok = self.encode(torch.cat([x_shot.reshape(-1, *img), x_query.reshape(-1, *img)], dim=0), patches)
        if tok.shape[1] > MAX_NODES:
            raise NotImplementedError(f'fsvit: a {tok.shape[1]}-token map; the DeepEMD head holds at most {MAX_NODES} nodes')
        n_shot = E * way * shot
        shot_tok = tok[:n_shot].reshape(E, way, shot, *tok.shape[1:])
        query_tok = tok[n_shot:].reshape(E, Q, *tok.shape[1:])
        proto = shot_tok[:, :, 0] if shot == 1 else self.get_sfc(shot_tok, generator=self.sfc_generator)
        return self.emd_forward(proto, query_tok)

    # ---- a labelled support set of any shape: encode once into a TokenBank, query many times (eval mode, whole images only)
    def _encode_eval(self, x, what):
        if self.deepemd != 'fcn':
            raise NotImplementedError(f"fsvit: DeepEMD.{what} is built for deepemd='fcn' (one token map per image), not {self.deepemd!r}")
        if self.training:
            raise RuntimeError(f'DeepEMD.{what} is an eval-mode entry: call model.eval() first')
        if x.dim() != 4:
            raise ValueError(f'{what}: expected images [N,3,H,W]')
        if not x.is_cuda:
            raise RuntimeError('fsvit: DeepEMD.%s got images on %s; the HIP engine needs an MI355X (no CPU fallback)' % (what, x.device))
        chunk = self.encoder.engine().chunk_images              # encode() reads the token map of the engine's last launch: one launch per chunk
        with torch.no_grad():
            tok = torch.cat([self.encode(x[i:i + chunk], False) for i in range(0, x.shape[0], chunk)]) if x.shape[0] else self.encode(x, False)
        if tok.shape[1] > MAX_NODES:
            raise NotImplementedError(f'fsvit: a {tok.shape[1]}-token map; the DeepEMD head holds at most {MAX_NODES} nodes')
        return tok

    def _scored(self, bank, fn):
        before = bank.status_count.clone()
        out = fn()
        self.add_status(bank.status_count - before)
        return out

    def fit(self, x_support, y_support, n_classes=None, bank=None):
        """x_support [S,3,H,W], y_support [S] integer labels -> TokenBank holding their token maps (the class map of a class is the mean of its support
        maps; no SFC fine-tune).  `bank`: extend this one instead of making one; otherwise `n_classes` (None: int(y_support.max()) + 1, one device
        read) sizes a new bank."""
        from .emd_bank import TokenBank
        tok = self._encode_eval(x_support, 'fit')
        y = y_support.to(tok.device)
        if y.dim() != 1 or y.shape[0] != tok.shape[0]:
            raise ValueError('fit: expected one label per support image')
        if bank is None:
            if n_classes is None:
                n_classes = int(y.max()) + 1
            bank = TokenBank(n_classes, tok.shape[1], tok.shape[2], tok.device)
        elif (bank.N, bank.C) != tuple(tok.shape[1:]):
            raise ValueError(f'fit: the bank holds maps of {bank.N} x {bank.C}, the encoder gives {tok.shape[1]} x {tok.shape[2]}')
        return bank.add(tok, y)

    def predict(self, bank, x_query):
        """x_query [Q,3,H,W] -> logits [Q, bank.n_classes]: every query against every class map with the model's temperature (TokenBank.logits)"""
        tok = self._encode_eval(x_query, 'predict')
        return self._scored(bank, lambda: bank.logits(tok, self.temperature))

    def predict_topk(self, bank, x_query, k, shortlist=None):
        """x_query [Q,3,H,W] -> (classes [Q,k] int64, logits [Q,k], prob [Q,k]) of TokenBank.topk: a shortlist of `shortlist` classes (None: min(32,
        bank.n_classes)) by the cosine of token means, re-ranked by their exact logits.  With shortlist >= bank.n_classes the head of a stable
        descending sort of predict(bank, x_query)'s rows.  1 <= k <= shortlist <= 32."""
        from ..engine import ops
        ops.check_shortlist(k, shortlist, 'predict_topk')
        tok = self._encode_eval(x_query, 'predict_topk')
        return self._scored(bank, lambda: bank.topk(tok, k, self.temperature, shortlist))

    def emd_forward(self, proto, query_tok):
        """emd_forward_1shot (:67-81): proto [E,P,N,C], query_tok [E,Q,N,C] -> logits [E,Q,P]."""
        from ..engine import ops
        if torch.is_grad_enabled() and (proto.requires_grad or query_tok.requires_grad):
            from ..autograd import EmdHeadFn
            logits, status = EmdHeadFn.apply(proto, query_tok, self.temperature)
        else:
            logits, _, status = ops.emd_head_forward(proto, query_tok, self.temperature, want_flow=False)
        self.add_status(status)
        return logits

    def get_sfc(self, shot_maps, perms=None, generator=None, fused=None, chunk=None):
        """Structured fully connected layer (:83-107), batched over episodes: shot_maps [E,way,shot,N,C] -> SFC [E,way,N,C].  Initialised with the
        mean over shots, then sfc_update_step epochs of SGD(lr=sfc_lr, momentum=0.9, dampening=0.9) over mini-batches of sfc_bs support images
        (labels arange(way).repeat(shot): the support set in shot-major order), cross entropy of the EMD logits per episode.  `perms`
        [steps, way*shot] or [steps, E, way*shot] fixes the permutation of every step (tests); otherwise a fresh torch.randperm per step and episode
        from `generator`.  Head forward / backward are the HIP kernels; the update of the one small tensor is torch arithmetic.
        `fused` (None: self.sfc_fused) keeps the whole loop on the device instead, one workgroup per episode (emd_sfc_kernel), in launches of at most
        `chunk` (None: SFC_CHUNK) mini-batch updates; the permutations are drawn by the same calls in the same order, so both routes see the same
        mini-batches for one generator state."""
        from ..engine import ops
        maps = shot_maps.detach().float()
        E, way, shot, N, Cc = maps.shape
        dev = maps.device
        n = way * shot
        support = maps.permute(0, 2, 1, 3, 4).reshape(E, n, N, Cc)             # index s * way + c
        label = torch.arange(way, device=dev).repeat(shot)
        sfc = maps.mean(dim=2).contiguous()
        if (self.sfc_fused if fused is None else fused):
            if perms is not None:
                drawn = [torch.as_tensor(perms[k]).cpu() for k in range(self.sfc_update_step)]
                drawn = [p.expand(E, n) if p.dim() == 1 else p for p in drawn]
            else:
                drawn = [torch.stack([torch.randperm(n, generator=generator) for _ in range(E)]).cpu() for _ in range(self.sfc_update_step)]
            if not drawn:
                return sfc
            table = sfc_step_table(torch.stack(drawn), self.sfc_bs)
            chunk = SFC_CHUNK if chunk is None else int(chunk)
            if chunk < 1:
                raise ValueError('chunk must be at least 1')
            support = support.contiguous()
            buf = count = None
            for i in range(0, table.shape[0], chunk):
                sfc, buf, count = ops.emd_sfc_steps(support, label, table[i:i + chunk], sfc, buf, count, temperature=self.temperature, lr=self.sfc_lr,
                                                    momentum=0.9, dampening=0.9, first=i == 0)
            self.add_status(count)
            return sfc
        buf = None
        rows = torch.arange(E, device=dev)[:, None]
        eye = torch.eye(way, device=dev)
        for k in range(self.sfc_update_step):
            if perms is not None:
                perm = torch.as_tensor(perms[k]).to(dev).long()
                perm = perm.expand(E, n) if perm.dim() == 1 else perm
            else:
                perm = torch.stack([torch.randperm(n, generator=generator) for _ in range(E)]).to(dev)
            for j in range(0, n, self.sfc_bs):
                ids = perm[:, j:j + self.sfc_bs]                               # [E, b]
                batch = support[rows, ids].contiguous()                         # [E, b, N, C]
                logits, flow, status = ops.emd_head_forward(sfc, batch, self.temperature)
                self.add_status(status)
                dlogits = (torch.softmax(logits, dim=-1) - eye[label[ids]]) / ids.shape[1]      # mean cross entropy per episode
                grad, _ = ops.emd_head_backward(sfc, batch, dlogits, flow, self.temperature)
                buf = grad.clone() if buf is None else buf.mul_(0.9).add_(grad, alpha=1.0 - 0.9)   # torch.optim.SGD: no dampening on the first step
                sfc = sfc - self.sfc_lr * buf
        return sfc
