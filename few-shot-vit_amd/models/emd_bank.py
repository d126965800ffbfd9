"""TokenBank: the class token maps of a labelled support set for the DeepEMD head, encoded once and queried many times (emd_head.hip).

The DeepEMD counterpart of PrototypeBank: classes may hold any number of examples and support maps may arrive in any number of `add` calls.  The
bank keeps per-class sums of token maps and counts on the device; the class map of a k-shot class is the mean of its support maps (the value
`DeepEMD.get_sfc` starts from; the SFC fine-tune of a bank is not built).  `logits` scores a query against every class - n_classes exact
transportation problems per query.  `topk` shortlists classes by the cosine of token means (ops.proto_bank_topk, which never forms the
[Q, n_classes] matrix) and solves only the shortlisted problems (ops.emd_rerank).  There is no CPU path."""
import torch

from ..engine import _require_cuda, ops

MAX_SHORTLIST = 32      # one lane per candidate in the re-rank kernel; also the list limit of ops.proto_bank_topk


class TokenBank:

    def __init__(self, n_classes, N, C, device=None):
        if int(n_classes) < 1 or int(N) < 1 or int(C) < 1:
            raise ValueError('TokenBank needs n_classes >= 1, N >= 1 and C >= 1')
        self.device = torch.device(device if device is not None else 'cuda')
        if self.device.type != 'cuda':
            raise RuntimeError('fsvit: TokenBank lives on an MI355X, not on %s (no CPU fallback)' % self.device)
        self.n_classes, self.N, self.C = int(n_classes), int(N), int(C)
        self.sum = torch.zeros(self.n_classes, self.N, self.C, dtype=torch.float32, device=self.device)
        self.count = torch.zeros(self.n_classes, dtype=torch.int32, device=self.device)
        self.invalid = torch.zeros(1, dtype=torch.int32, device=self.device)       # labels / candidates outside their range seen so far: read by check()
        self.status_count = torch.zeros(1, dtype=torch.int32, device=self.device)  # problems of topk() that stopped at a loop bound of the solver
        self._maps = None                                                          # (tok, xhat, pooled, proto, empty) of the current sums

    def add(self, tok, labels):
        """tok [S,N,C] (any float type), labels [S] (int32 / int64), both on the device: extends the classes they name.  A label outside
        [0, n_classes) adds nothing and is counted; check() reports it (no synchronisation here)."""
        _require_cuda(tok, labels)
        ops.emd_bank_accumulate(tok, labels, self.sum, self.count, self.invalid)
        self._maps = None
        return self

    @property
    def counts(self):
        return self.count

    def class_maps(self):
        """-> (tok [n_classes,N,C]: the class means, xhat, pooled: their prepared nodes and token means, proto [n_classes,C]: the unit-length token
        means the shortlist is drawn with, empty [n_classes] int32); zero rows for a class without examples.  Formed on first use after an add()."""
        if self._maps is None:
            self._maps = ops.emd_bank_finalize(self.sum, self.count)
        return self._maps

    def _prepare(self, query_tok):
        _require_cuda(query_tok)
        if query_tok.dim() != 3 or tuple(query_tok.shape[1:]) != (self.N, self.C):
            raise ValueError(f'expected query token maps [Q,{self.N},{self.C}], got {tuple(query_tok.shape)}')
        tok = query_tok.detach().contiguous().float()
        xhat, pooled = torch.empty_like(tok), torch.empty(tok.shape[0], self.C, dtype=torch.float32, device=tok.device)
        ops.emd_table_prep(tok, xhat, pooled)
        return tok, xhat, pooled

    def logits(self, query_tok, temperature):
        """query_tok [Q,N,C] -> logits [Q,n_classes]: every query against every class map, the dense route (ops.emd_head_gather with the class maps
        as the dense prototypes); a class without examples scores -inf.  Problems at a loop bound of the solver are counted in self.status_count."""
        tok, xhat, pooled = self._prepare(query_tok)
        maps = self.class_maps()
        Q = tok.shape[0]
        if Q == 0:
            return tok.new_empty(0, self.n_classes)
        slots = torch.arange(Q, dtype=torch.int32, device=tok.device)[None]
        invalid = torch.zeros(1, dtype=torch.int32, device=tok.device)             # (the slots are arange(Q): nothing can raise it)
        logits, status = ops.emd_head_gather(tok, xhat, pooled, slots, temperature, invalid, proto_tok=maps[0][None])
        self.status_count += status.sum(dtype=torch.int32)
        return logits[0].masked_fill(maps[4].bool()[None], float('-inf'))

    def topk(self, query_tok, k, temperature, shortlist=None, cand=None):
        """query_tok [Q,N,C] -> (classes [Q,k] int64, logits [Q,k], prob [Q,k]): the k best of a shortlist of classes, each scored exactly, in the order
        larger logit, lower class, lower shortlist position; prob is the softmax over the shortlist.  The shortlist holds `shortlist` classes (None:
        min(32, n_classes)): the best by the cosine between the token means of the query and the class maps, or the rows of `cand` [Q,M] int32 when
        given (-1: an empty slot; it ranks last with class -1, logit -inf, prob 0, as does the tail where the shortlist exceeds n_classes).  With
        shortlist >= n_classes the result is the head of a stable descending sort of logits()'s rows.  Problems at a loop bound of the solver are
        counted in self.status_count, candidates outside [-1, n_classes) in self.invalid.  1 <= k <= shortlist <= 32."""
        ops.check_shortlist(k, shortlist, 'TokenBank.topk')
        if cand is not None and (cand.dim() != 2 or not k <= cand.shape[1] <= MAX_SHORTLIST):
            raise ValueError(f'TokenBank.topk: expected cand [Q,M] with k <= M <= {MAX_SHORTLIST}')
        query = self._prepare(query_tok)
        tok_c, xhat_c, pooled_c, proto, empty = self.class_maps()
        if cand is None:
            m = min(MAX_SHORTLIST, self.n_classes) if shortlist is None else shortlist
            if k > m:
                raise ValueError(f'TokenBank.topk: k = {k} exceeds the shortlist of {m} (a bank of {self.n_classes} classes)')
            cand = ops.proto_bank_topk(query[2], proto, empty, 1.0, 'cos', k=m, want_lse=False)[1]
        else:
            _require_cuda(cand)
            cand = cand.clamp(-2, 2 ** 31 - 1).to(torch.int32)      # (an int64 entry beyond int32 stays out of range instead of wrapping into it)
        classes, values, prob, _, _, _ = ops.emd_rerank(query, (tok_c, xhat_c, pooled_c, empty), cand, temperature, k, self.status_count, self.invalid)
        return classes.long(), values, prob

    def check(self):
        """One synchronisation, when the caller asks: raises if any label handed to add() or candidate handed to topk() was out of range."""
        n = int(self.invalid.item())
        if n:
            raise ValueError(f'fsvit: {n} support label(s) or candidate(s) were outside [0, {self.n_classes}) and were left out')

    def state_dict(self):
        return {'sum': self.sum.clone(), 'count': self.count.clone(), 'dims': (self.n_classes, self.N, self.C)}

    def load_state_dict(self, sd):
        s, c = sd['sum'], sd['count']
        if tuple(sd['dims']) != (self.n_classes, self.N, self.C) or tuple(s.shape) != (self.n_classes, self.N, self.C) or tuple(c.shape) != (self.n_classes,):
            raise ValueError(f'bank state of dims {tuple(sd["dims"])} / shape {tuple(s.shape)} does not fit a bank of {self.n_classes} classes x {self.N} x {self.C}')
        self.sum.copy_(s.to(self.device, torch.float32))
        self.count.copy_(c.to(self.device, torch.int32))
        self._maps = None
        return self

    @classmethod
    def from_state_dict(cls, sd, device=None):
        return cls(*sd['dims'], device).load_state_dict(sd)
