"""PrototypeBank: the prototypes of a labelled support set, encoded once and queried many times (proto_bank.hip).

Classes may hold any number of examples, support features may arrive in any number of `add` calls, and the label space may be the 5 classes of
an episode or the 351 base classes.  The bank keeps per-class feature sums and counts on the device; prototypes are formed from them when they
are first needed after an `add`.  There is no CPU path."""
import torch

from ..engine import _require_cuda, ops

METHODS = ('cos', 'sqr', 'dot')


class PrototypeBank:

    def __init__(self, n_classes, dim, method='cos', device=None):
        if method not in METHODS:
            raise ValueError(method)
        if int(n_classes) < 1 or int(dim) < 1:
            raise ValueError('PrototypeBank needs n_classes >= 1 and dim >= 1')
        self.device = torch.device(device if device is not None else 'cuda')
        if self.device.type != 'cuda':
            raise RuntimeError('fsvit: PrototypeBank lives on an MI355X, not on %s (no CPU fallback)' % self.device)
        self.n_classes, self.dim, self.method = int(n_classes), int(dim), method
        self.sum = torch.zeros(self.n_classes, self.dim, dtype=torch.float32, device=self.device)
        self.count = torch.zeros(self.n_classes, dtype=torch.int32, device=self.device)
        self.invalid = torch.zeros(1, dtype=torch.int32, device=self.device)       # labels outside [0, n_classes) seen so far: read by check()
        self._proto = None                                                         # (proto, empty) of the current sums

    def add(self, feat, labels):
        """feat [S,dim] (any float type), labels [S] (int32 / int64), both on the device: extends the classes they name.  A label outside
        [0, n_classes) adds nothing and is counted; check() reports it (no synchronisation here)."""
        _require_cuda(feat, labels)
        ops.proto_bank_accumulate(feat, labels, self.sum, self.count, self.invalid)
        self._proto = None
        return self

    def _finalized(self):
        if self._proto is None:
            self._proto = ops.proto_bank_finalize(self.sum, self.count, self.method)
        return self._proto

    def prototypes(self):
        """[n_classes, dim]: the class means, normalised for 'cos'; zero rows for classes without examples"""
        return self._finalized()[0]

    @property
    def counts(self):
        return self.count

    def logits(self, feat, temp=1.0):
        """feat [Q,dim] -> [Q,n_classes]; a class without examples scores -inf"""
        return self.predict(feat, temp)[1]

    def predict(self, feat, temp=1.0):
        """-> (pred [Q] int64: the first maximum of every row, logits [Q,n_classes])"""
        _require_cuda(feat)
        proto, empty = self._finalized()
        logits, pred = ops.proto_bank_logits(feat, proto, empty, temp, self.method)
        return pred.long(), logits

    def topk(self, feat, k, temp=1.0):
        """feat [Q,dim] -> (classes [Q,k] int64, logits [Q,k], prob [Q,k]): the k best classes of every row of logits(feat, temp) in the order of a
        stable descending sort (ties: the lower class) and their softmax probabilities over all classes with examples, prob = exp(logit - lse); the
        [Q,n_classes] matrix is never formed.  1 <= k <= 32.  An empty class scores -inf with prob 0; where k exceeds n_classes the tail holds class
        -1, logit -inf, prob 0."""
        ops.check_topk_k(k, 'PrototypeBank.topk')
        _require_cuda(feat)
        proto, empty = self._finalized()
        values, indices, lse = ops.proto_bank_topk(feat, proto, empty, temp, self.method, k)
        prob = torch.where(torch.isneginf(values), torch.zeros_like(values), torch.exp(values - lse[:, None]))
        return indices.long(), values, prob

    def check(self):
        """One synchronisation, when the caller asks: raises if any label handed to add() was outside [0, n_classes)."""
        n = int(self.invalid.item())
        if n:
            raise ValueError(f'fsvit: {n} support label(s) were outside [0, {self.n_classes}) and were left out of the bank')

    def state_dict(self):
        return {'sum': self.sum.clone(), 'count': self.count.clone(), 'method': self.method}

    def load_state_dict(self, sd):
        s, c = sd['sum'], sd['count']
        if tuple(s.shape) != (self.n_classes, self.dim) or tuple(c.shape) != (self.n_classes,):
            raise ValueError(f'bank state of shape {tuple(s.shape)} / {tuple(c.shape)} does not fit a bank of {self.n_classes} classes x {self.dim}')
        if sd['method'] not in METHODS:
            raise ValueError(sd['method'])
        self.sum.copy_(s.to(self.device, torch.float32))
        self.count.copy_(c.to(self.device, torch.int32))
        self.method = sd['method']
        self._proto = None
        return self

    @classmethod
    def from_state_dict(cls, sd, device=None):
        return cls(sd['sum'].shape[0], sd['sum'].shape[1], sd['method'], device).load_state_dict(sd)
