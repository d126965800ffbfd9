"""Case builder and oracle of the token-map bank tests (a helper, not a test module).

A case is a labelled support set and a query set of token maps with class structure: every class has a centre map, and a support or query map is
0.6 * centre[label] + unit noise + a per-channel offset of 0.5 sigma (the offset of emd_cases.token_case: pooled dot products take both signs and
some node weights sit at the floor).  The oracle is float64 throughout: the class map is the float64 mean of the class's support maps, and a logit
is emd_cases.emd_logits of a query map against it (the reference's head with an exact LP solver); a class without examples scores -inf.

Found on the CPU for (12 classes, up to 3 shots, N = 25, C = 64, Q = 6) and (40, 3, 7, 64, 5), seeds 0 .. 2: the 66 or 195 linprog problems of a case
take 0.25 - 1.0 s; the arg-max of the oracle's EMD logits names the query's class at least as often as the cosine of token means in all six cases
(0.83 / 0.83 / 1.0 / 1.0 / 0.6 / 1.0 against 0.33 / 0.5 / 0.17 / 0.6 / 0.4 / 0.6); and consecutive oracle logits of a row come as close as 4.9e-5 -
closer than the 1e-4 the fp32 head is held to, so no test compares an ORDER with this oracle.
"""
import torch

import emd_cases as ec

T = 12.5


def ragged_shots(n_classes, shots, seed):
    """`shots` as a tuple: taken as it is; as an int: between 1 and `shots` per class, and none at all for class 1 (class 0 of a single class)"""
    if not isinstance(shots, int):
        assert len(shots) == n_classes
        return tuple(int(s) for s in shots)
    g = torch.Generator().manual_seed(9000 + seed)
    out = torch.randint(1, shots + 1, (n_classes,), generator=g).tolist()
    if n_classes > 1:
        out[1] = 0
    return tuple(out)


def bank_case(n_classes, shots, Q, N, C, seed):
    """-> dict(sup [S,N,C], sup_lab [S], qry [Q,N,C], qry_lab [Q], shots): float64 tensors holding float32 values, int64 labels.  The support rows
    are shuffled (the rows of a class are neither adjacent nor in class order); query labels are drawn from the classes that have examples."""
    shots = ragged_shots(n_classes, shots, seed)
    g = torch.Generator().manual_seed(seed)
    centre = torch.randn(n_classes, N, C, generator=g, dtype=torch.float64)
    offset = 0.5 * torch.randn(1, 1, C, generator=g, dtype=torch.float64)
    sup_lab = torch.cat([torch.full((s,), c, dtype=torch.int64) for c, s in enumerate(shots)])
    sup_lab = sup_lab[torch.randperm(sup_lab.shape[0], generator=g)]
    filled = torch.tensor([c for c, s in enumerate(shots) if s > 0])
    qry_lab = filled[torch.randint(0, filled.shape[0], (Q,), generator=g)]
    draw = lambda lab: 0.6 * centre[lab] + torch.randn(lab.shape[0], N, C, generator=g, dtype=torch.float64) + offset
    sup, qry = draw(sup_lab), draw(qry_lab)
    return dict(sup=sup.float().double(), sup_lab=sup_lab, qry=qry.float().double(), qry_lab=qry_lab, shots=shots)


def class_means(case):
    """float64 mean map of every class [n_classes,N,C] (zeros for a class without examples) and empty [n_classes] bool"""
    n_classes = len(case['shots'])
    mean = torch.zeros(n_classes, *case['sup'].shape[1:], dtype=torch.float64)
    for c, s in enumerate(case['shots']):
        if s:
            mean[c] = case['sup'][case['sup_lab'] == c].mean(dim=0)
    return mean, torch.tensor([s == 0 for s in case['shots']])


_oracle = {}


def bank_oracle(key):
    """key = the arguments of bank_case -> (case, logits [Q,n_classes] float64, -inf for a class without examples); computed once per key"""
    if key not in _oracle:
        case = bank_case(*key)
        mean, empty = class_means(case)
        logits = torch.full((case['qry'].shape[0], len(case['shots'])), float('-inf'), dtype=torch.float64)
        logits[:, ~empty] = ec.emd_logits(mean[~empty], case['qry'], T)[0]
        _oracle[key] = (case, logits)
    return _oracle[key]


def ranked(values, classes):
    """The order of the re-rank for one row: positions sorted by larger value, then lower class, then lower position, an empty slot (class -1) after
    every class.  values / classes: sequences of equal length -> list of positions."""
    key = lambda i: (-float(values[i]), classes[i] if classes[i] >= 0 else 1 << 40, i)
    return sorted(range(len(values)), key=key)
