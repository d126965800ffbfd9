"""Oracle and case builders of the DeepEMD head tests (a helper, not a test module).

The oracle is a float64 restatement of the reference's head, meta_tuning_sun_d/Models/models/Network.py:48-81 (weights, emd_forward_1shot),
:109-124 (get_emd_distance, `solver: opencv`), :143-175 (normalize_feature, get_similiarity_map), :83-107 (get_sfc) and
Models/models/emd_utils.py:65-76 (emd_inference_opencv).  `cv2.EMD` is replaced by `scipy.optimize.linprog(method='highs')`: after the
normalisation of emd_utils.py:72-73 both weight vectors sum to N, the optimal cost of the linear program is unique whichever exact solver
finds it, and logit = temperature / N * sum S F = temperature / N * (N - optimal cost).

Token maps are token-major here: [.., N, C] (the reference's [.., C, H, W] with H * W flattened and moved in front of C).
"""
import numpy as np
import torch
from scipy.optimize import linprog

_HIGHS = dict(primal_feasibility_tolerance=1e-10, dual_feasibility_tolerance=1e-10)


def solve_transport(cost, w1, w2):
    """min sum c F, F >= 0, row sums w1, column sums w2 in float64 -> (optimum, F).  One equality row is redundant (sum w1 == sum w2) and dropped,
    which also keeps the program feasible when the two sums differ in the last bits."""
    cost = np.asarray(cost, dtype=np.float64)
    n1, n2 = cost.shape
    A = np.zeros((n1 + n2, n1 * n2))
    for i in range(n1):
        A[i, i * n2:(i + 1) * n2] = 1.0
    for j in range(n2):
        A[n1 + j, j::n2] = 1.0
    b = np.concatenate([np.asarray(w1, dtype=np.float64), np.asarray(w2, dtype=np.float64)])
    res = linprog(cost.ravel(), A_eq=A[:-1], b_eq=b[:-1], bounds=(0, None), method='highs', options=_HIGHS)
    assert res.status == 0, res.message
    return float(res.fun), res.x.reshape(n1, n2)


# ---- the head (one episode): proto [P, N, C], query [Q, N, C]
def weight_vector(A, B):
    """get_weight_vector (:48-65): [M, K, N] = relu(<token n of A[m], token mean of B[k]>) + 1e-3; the pooling sees the UN-centred map (:70-71)."""
    pooled = B.mean(dim=1)                                          # adaptive_avg_pool2d(B, [1, 1]) (:53)
    return torch.relu(torch.einsum('mnc,kc->mkn', A, pooled)) + 1e-3   # (:62-64)


def centre(x):
    """normalize_feature, norm 'center' (:143-146): the mean is over channels (dim 1 of [B, C, H, W])."""
    return x - x.mean(dim=-1, keepdim=True)


def similarity_map(proto, query):
    """get_similiarity_map, metric 'cosine' (:151-167): [Q, P, query node, proto node]; F.cosine_similarity clamps each norm at 1e-8."""
    qn = query / query.norm(dim=-1, keepdim=True).clamp_min(1e-8)
    pn = proto / proto.norm(dim=-1, keepdim=True).clamp_min(1e-8)
    return torch.einsum('qac,pbc->qpab', qn, pn)


def normalise_weight(w):
    """emd_inference_opencv (emd_utils.py:69-73): relu(w) + 1e-5, scaled to sum N."""
    w = torch.relu(w) + 1e-5
    return w * (w.shape[0] / w.sum())


def emd_logits(proto, query, temperature, flows=None):
    """emd_forward_1shot (:67-81) + get_emd_distance (:109-124): -> (logits [Q, P], flows [Q, P, N, N]).  With `flows` given they replace the
    solver's (constants either way: the logits are differentiable in proto / query through the similarity map only, :118-120)."""
    P, N = proto.shape[:2]
    Q = query.shape[0]
    w1 = weight_vector(query, proto)                                # [Q, P, N] (:70)
    w2 = weight_vector(proto, query)                                # [P, Q, N] (:71)
    S = similarity_map(centre(proto), centre(query))                # (:73-76)
    if flows is None:
        flows = torch.zeros(Q, P, N, N, dtype=torch.float64)
        for i in range(Q):
            for j in range(P):
                _, f = solve_transport((1.0 - S[i, j]).detach().numpy(), normalise_weight(w1[i, j].detach()).numpy(),
                                       normalise_weight(w2[j, i].detach()).numpy())      # (:118)
                flows[i, j] = torch.from_numpy(f)
    flows = torch.as_tensor(flows, dtype=torch.float64)
    return (S * flows).sum(-1).sum(-1) * (temperature / N), flows  # (:120-123)


def head_oracle(shot_tok, query_tok, temperature, flows=None):
    """Episodes one by one: shot_tok [E, P, N, C], query_tok [E, Q, N, C] float64 -> logits [E, Q, P] (and the flows [E, Q, P, N, N])."""
    out = [emd_logits(shot_tok[e], query_tok[e], temperature, None if flows is None else flows[e]) for e in range(shot_tok.shape[0])]
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


def sfc_oracle(shot_maps, perms, temperature, sfc_lr, steps, bs):
    """get_sfc (:83-107) for one episode: shot_maps [way, shot, N, C] float64, perms [steps][way * shot] -> SFC [way, N, C].  The reference's support
    set is shot-major (`view(shot, -1, ...)`, labels arange(way).repeat(shot))."""
    way, shot = shot_maps.shape[:2]
    support = shot_maps.permute(1, 0, 2, 3).reshape(way * shot, *shot_maps.shape[2:])
    sfc = torch.nn.Parameter(shot_maps.mean(dim=1).clone().detach())                       # (:86-87)
    opt = torch.optim.SGD([sfc], lr=sfc_lr, momentum=0.9, dampening=0.9, weight_decay=0)   # (:89)
    label = torch.arange(way).repeat(shot)                                                 # (:92)
    for k in range(steps):
        rand_id = torch.as_tensor(perms[k]).long()                                         # (:97)
        for j in range(0, way * shot, bs):
            sel = rand_id[j:min(j + bs, way * shot)]
            opt.zero_grad()
            logits, _ = emd_logits(sfc, support[sel].detach(), temperature)                # (:103)
            torch.nn.functional.cross_entropy(logits, label[sel]).backward()
            opt.step()
    return sfc.detach()


# ---- case builders
SOLVER_KINDS = ('random', 'duplicates', 'constant', 'zero_diagonal', 'equal_weights', 'floor_weights')


def _weights(rng, n, kind):
    if kind == 'floor_weights':                 # most nodes at the 1e-3 floor of get_weight_vector, a few carry the mass
        w = np.full(n, 1e-3 + 1e-5)
        heavy = rng.choice(n, size=max(1, n // 8), replace=False)
        w[heavy] += rng.uniform(0.5, 3.0, size=heavy.size)
    else:
        w = rng.uniform(0.05, 1.0, size=n)
    return (w * (n / w.sum())).astype(np.float32)


def solver_cases(N, count=32, seed=0):
    """`count` problems of N nodes, the kinds of SOLVER_KINDS in turn: (kinds, cost [count, N, N], w1, w2 [count, N]) float32."""
    rng = np.random.default_rng(1000 * N + seed)
    kinds, cost, w1, w2 = [], [], [], []
    for i in range(count):
        kind = SOLVER_KINDS[i % len(SOLVER_KINDS)]
        c = rng.uniform(0.0, 2.0, size=(N, N))
        if kind == 'duplicates' and N > 1:      # tied costs: duplicated rows and columns
            c[rng.integers(N)] = c[rng.integers(N)]
            c[:, N - 1] = c[:, 0]
            c[N - 1] = c[0]
        elif kind == 'constant':
            c[:] = rng.uniform(0.1, 1.9)
        elif kind == 'zero_diagonal':
            np.fill_diagonal(c, 0.0)
        a = _weights(rng, N, kind)
        b = a.copy() if kind == 'equal_weights' else _weights(rng, N, kind)
        kinds.append(kind)
        cost.append(c.astype(np.float32))
        w1.append(a)
        w2.append(b)
    return kinds, np.stack(cost), np.stack(w1), np.stack(w2)


def token_case(E, P, Q, N, C, seed, constant_token=False, shared_image=False):
    """Token maps like an encoder's post-norm output: unit noise on a per-channel offset (so pooled dot products take both signs and some weights sit
    at the floor).  float64; the GPU gets the float32 rounding, and so does the oracle."""
    g = torch.Generator().manual_seed(seed)
    bias = 0.5 * torch.randn(1, 1, 1, C, generator=g, dtype=torch.float64)
    shot = torch.randn(E, P, N, C, generator=g, dtype=torch.float64) + bias
    query = torch.randn(E, Q, N, C, generator=g, dtype=torch.float64) + bias
    if constant_token:
        query[0, 0, 0] = 0.75                   # centred vector zero: similarity 0, not NaN
        shot[0, 0, N - 1] = -1.25
    if shared_image:
        query[0, Q - 1] = shot[0, 0]            # one image as query and as proto: its logit is the temperature
    return shot.float().double(), query.float().double()


# SFC: E = 2, way = 3, shot = 2, N = 13, C = 64, sfc_bs = 4, 3 update steps, sfc_lr = 0.1
SFC_CFG = dict(E=2, way=3, shot=2, N=13, C=64, bs=4, steps=3, lr=0.1, temperature=12.5)
# seeds of sfc_case() whose float64 result is stable under float32 rounding of the inputs (sfc_case(seed, screen=True) passes); found by
# running the screen over seeds 0 .. 7 (all eight pass)
SFC_SEEDS = (0, 1, 2)


def sfc_case(seed, screen=False):
    """-> (shot_maps [E, way, shot, N, C] float64 holding float32 values, perms [steps, E, way * shot], oracle SFC [E, way, N, C]).  With `screen` the
    float64 run on the unrounded inputs must agree with the run on the rounded ones to 1e-5 of the largest entry (a flow that flips between two
    near-tied vertices under a 1e-7 perturbation of the costs would not): returns None otherwise."""
    c = SFC_CFG
    g = torch.Generator().manual_seed(7000 + seed)
    raw = torch.randn(c['E'], c['way'], c['shot'], c['N'], c['C'], generator=g, dtype=torch.float64) + \
        0.5 * torch.randn(1, 1, 1, 1, c['C'], generator=g, dtype=torch.float64)
    perms = torch.stack([torch.stack([torch.randperm(c['way'] * c['shot'], generator=g) for _ in range(c['E'])]) for _ in range(c['steps'])])
    rounded = raw.float().double()
    run = lambda x: torch.stack([sfc_oracle(x[e], perms[:, e], c['temperature'], c['lr'], c['steps'], c['bs']) for e in range(c['E'])])
    ref = run(rounded)
    if screen:
        if ((run(raw) - ref).abs().max() / ref.abs().max()).item() > 1e-5:
            return None
    return rounded, perms, ref
