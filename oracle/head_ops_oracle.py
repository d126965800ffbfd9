"""float64 references of pool_affine (feat_out.hip), the episode head (head.hip), the distillation losses / linear head / row normalisation
(token_label.hip) and the SGD / AdamW updates (optim.hip), written from the formulas in the kernels' header comments, and the first-order fp32
allowances the tests gate the kernels with (tests/head_cases.py; the derivations are written out in the header of tests/test_gpu_head_ops.py).

Every function takes float64 tensors holding fp32-representable values and returns float64.  The allowance functions return, per output element, a bound
`a` on |fp32 kernel - float64 result| that is built from float64 quantities only:
    U = 2^-24 (half an fp32 ulp), E = 2^-20 (one expf / logf / sqrtf / reciprocal or division of the device library),
    sum_tol(t, n) = 4 sqrt(n) U t (a chain of n additions whose terms have absolute sum t), dot(t, n) = sum_tol(t, n) + U t (the products' roundings).
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
E = 2.0 ** -20
EPS = 1e-12          # F.normalize's clamp


def sum_tol(t, n):
    return 4.0 * math.sqrt(n) * U * t


def dot(t, n):
    return sum_tol(t, n) + U * t


def wave_depth(n):
    """chain length of a lane-strided wave reduction over n terms: ceil(n / 64) terms per lane, then 6 butterfly levels"""
    return (n + 63) // 64 + 6


def _rel(num, den):
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.zeros_like(num))


# ------------------------------------------------------------------------------------------------------------------------------- F.normalize
def normalize(x):
    """-> (x / max(|x|, 1e-12), 1 / max(|x|, 1e-12) [..., 1])"""
    inv = 1.0 / x.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(EPS)
    return x * inv, inv


def normalize_backward(x, g):
    """gradient of normalize(x) under an upstream g, the clamp as torch differentiates it: (g - y <y, g>) / |x| where |x| >= 1e-12, g / 1e-12 below"""
    n = x.pow(2).sum(-1, keepdim=True).sqrt()
    y = x / n.clamp_min(EPS)
    return torch.where(n >= EPS, (g - y * (y * g).sum(-1, keepdim=True)) / n.clamp_min(EPS), g / EPS)


def _inv_rel(x, a_x=None):
    """relative allowance of 1 / max(sqrt(sum x^2), 1e-12): half the relative error of the sum of squares (its own chain, the inputs' allowance a_x),
    one sqrtf, one reciprocal.  A zero row is exact up to the two library calls."""
    D = x.shape[-1]
    ss = x.pow(2).sum(-1, keepdim=True)
    r = 4.0 * math.sqrt(wave_depth(D)) * U + U
    if a_x is not None:
        r = r + _rel(2.0 * (x.abs() * a_x).sum(-1, keepdim=True), ss)
    return torch.where(ss > 0, 0.5 * r, torch.zeros_like(ss)) + 2.0 * E


# ------------------------------------------------------------------------------------------------------------------------------- episode head
def _proto(fs):
    shot = fs.shape[2]
    p = fs.sum(2) / shot
    a_p = dot(fs.abs().sum(2), shot) / shot + U * p.abs()
    return p, a_p


def make_nk_label(E_, way, Q):
    per = Q // way
    q = torch.arange(Q)
    lab = q // per if per > 0 else torch.zeros_like(q)
    return lab.repeat(E_)


def head_forward(fs, fq, temp, method, labels=None):
    """fs [E, way, shot, D], fq [E, Q, D], labels int64 [E Q] or None (make_nk_label) ->
    dict(logits [E,Q,way], nll [E,Q], loss [E], count [E] (queries whose FIRST maximum is the label), dlogits [E,Q,way] of the mean CE over all E Q rows,
         a_logits, a_nll, a_loss, a_dlogits: the allowances, margin [E,Q]: top-1 minus top-2 logit)"""
    E_, way, shot, D = fs.shape
    Q = fq.shape[1]
    n = wave_depth(D)
    p, a_p = _proto(fs)
    if method == 'cos':
        ph, pinv = normalize(p)
        a_ph = a_p * pinv + ph.abs() * (_inv_rel(p, a_p) + U)
        qh, _ = normalize(fq)
        r_q = _inv_rel(fq)                                                         # [E, Q, 1]
        L = temp * qh @ ph.transpose(1, 2)
        T = qh.abs() @ ph.abs().transpose(1, 2)
        a_l = abs(temp) * (qh.abs() @ a_ph.transpose(1, 2) + T * (r_q + U) + dot(T, n)) + U * L.abs()
    elif method == 'dot':
        L = temp * fq @ p.transpose(1, 2)
        T = fq.abs() @ p.abs().transpose(1, 2)
        a_l = abs(temp) * (fq.abs() @ a_p.transpose(1, 2) + dot(T, n)) + U * L.abs()
    else:
        df = fq[:, :, None, :] - p[:, None, :, :]                                  # [E, Q, way, D]
        T = df.pow(2).sum(-1)
        L = -temp * T
        a_l = abs(temp) * ((2.0 * df.abs() * (a_p[:, None] + U * df.abs())).sum(-1) + dot(T, n)) + U * L.abs()
    lab = (make_nk_label(E_, way, Q) if labels is None else labels).reshape(E_, Q)
    mx = L.max(-1, keepdim=True).values
    ex = (L - mx).exp()
    se = ex.sum(-1, keepdim=True)
    P = ex / se
    lse = mx + se.log()
    l_lab = L.gather(-1, lab[..., None])
    nll = (lse - l_lab).squeeze(-1)
    r_ex = U * (L - mx).abs() + E
    r_se = (P * r_ex).sum(-1, keepdim=True) + 4.0 * math.sqrt(way) * U
    a_nll = ((P * a_l).sum(-1, keepdim=True) + a_l.gather(-1, lab[..., None]) + r_se + E * se.log().abs() + U * lse.abs()).squeeze(-1) + U * nll.abs()
    loss = nll.sum(1) / Q
    a_loss = a_nll.sum(1) / Q + dot(nll.abs().sum(1), Q) / Q + U * loss.abs()
    onehot = torch.zeros_like(L).scatter_(-1, lab[..., None], 1.0)
    rows = float(E_ * Q)
    dl = (P - onehot) / rows
    a_dl = (P * (a_l + (P * a_l).sum(-1, keepdim=True)) + P * (r_ex + r_se + E + U) + U * (P - onehot).abs()) / rows + (E + U) * dl.abs()
    top2 = L.topk(min(2, way), -1).values
    margin = (top2[..., 0] - top2[..., 1]) if way > 1 else torch.full_like(nll, math.inf)
    first = torch.where(L == mx, torch.arange(way).expand_as(L), torch.full_like(L, way, dtype=torch.int64)).min(-1).values      # the FIRST maximum
    count = (first == lab).sum(1).double()
    return dict(logits=L, nll=nll, loss=loss, count=count, dlogits=dl, a_logits=a_l, a_nll=a_nll, a_loss=a_loss, a_dlogits=a_dl, margin=margin,
                a_row=a_l.max(-1).values)


def head_backward(fs, fq, dl, temp, method, up=1.0):
    """dl [E, Q, way] upstream gradient of the logits, up: the scalar the loss gradient is scaled with ->
    dict(dshot [E,way,shot,D], dq [E,Q,D], dtemp [E] and a_dshot, a_dq, a_dtemp)"""
    E_, way, shot, D = fs.shape
    Q = fq.shape[1]
    n = wave_depth(D)
    p, a_p = _proto(fs)
    t = temp * up
    g = dl * up
    if method == 'cos':
        ph, pinv = normalize(p)
        r_p = _inv_rel(p, a_p)
        a_ph = a_p * pinv + ph.abs() * (r_p + U)
        qh, qinv = normalize(fq)
        r_q = _inv_rel(fq)
        s = qh @ ph.transpose(1, 2)                                                # [E, Q, way]
        S_abs = qh.abs() @ ph.abs().transpose(1, 2)
        a_s = qh.abs() @ a_ph.transpose(1, 2) + S_abs * (r_q + U) + dot(S_abs, n)
        # query side
        gq = t * dl @ ph                                                           # dq^ [E, Q, D]
        G = (t * dl).abs() @ ph.abs()
        a_gq = (t * dl).abs() @ a_ph + dot(G, way) + 3.0 * U * G
        dotqg = (t * dl * s).sum(-1, keepdim=True)
        DA = (t * dl * s).abs().sum(-1, keepdim=True)
        a_dot = ((t * dl).abs() * a_s).sum(-1, keepdim=True) + dot(DA, way) + 3.0 * U * DA
        dq = normalize_backward(fq, gq)
        inner = gq - qh * dotqg
        a_dq = qinv * (a_gq + qh.abs() * a_dot + (qh * dotqg).abs() * (r_q + 2.0 * U) + U * inner.abs()) + dq.abs() * (r_q + U)
        # temperature
        dtemp = (g * s).sum((1, 2))
        a_dt = abs(up) * ((dl.abs() * a_s).sum((1, 2)) + dot((dl * s).abs().sum((1, 2)), ((Q + 15) // 16) * way + 16)) + 2.0 * U * dtemp.abs()
        # shot side: dp^ = t sum_q dl q^ ; dp = (dp^ - p^ <p^, dp^>) / |p| ; every shot of a class gets dp / shot
        dph = t * dl.transpose(1, 2) @ qh                                          # [E, way, D]
        PA = dl.abs().transpose(1, 2) @ qh.abs()
        a_dph = abs(t) * (dl.abs().transpose(1, 2) @ (qh.abs() * (r_q + 2.0 * U)) + sum_tol(PA, Q)) + 2.0 * U * dph.abs()
        dotp = (ph * dph).sum(-1, keepdim=True)
        a_dotp = (a_ph * dph.abs() + ph.abs() * a_dph).sum(-1, keepdim=True) + dot((ph * dph).abs().sum(-1, keepdim=True), n)
        dp = normalize_backward(p, dph)
        innerp = dph - ph * dotp
        a_dp = pinv * (a_dph + a_ph * dotp.abs() + ph.abs() * a_dotp + U * (ph * dotp).abs() + U * innerp.abs()) + dp.abs() * (r_p + 2.0 * U)
        dshot, a_dshot = dp / shot, a_dp / shot + U * dp.abs() / shot
    else:
        df = fq[:, :, None, :] - p[:, None, :, :]                                  # [E, Q, way, D]
        a_df = a_p[:, None] + U * df.abs()
        dq = -2.0 * t * (dl[..., None] * df).sum(2)
        a_dq = 2.0 * abs(t) * ((dl.abs()[..., None] * a_df).sum(2) + dot((dl[..., None] * df).abs().sum(2), way)) + 3.0 * U * dq.abs()
        dsq = df.pow(2).sum(-1)
        a_dsq = (2.0 * df.abs() * a_df).sum(-1) + dot(dsq, n)
        dtemp = -(g * dsq).sum((1, 2))
        a_dt = abs(up) * ((dl.abs() * a_dsq).sum((1, 2)) + dot((dl * dsq).abs().sum((1, 2)), ((Q + 3) // 4) * way + 4)) + 2.0 * U * dtemp.abs()
        dp = 2.0 * t / shot * (dl[..., None] * df).sum(1)
        a_dp = 2.0 * abs(t) / shot * ((dl.abs()[..., None] * a_df).sum(1) + dot((dl[..., None] * df).abs().sum(1), Q)) + 4.0 * U * dp.abs()
        dshot, a_dshot = dp, a_dp
    ex = lambda x: x[:, :, None, :].expand(E_, way, shot, D).contiguous()
    return dict(dshot=ex(dshot), dq=dq, dtemp=dtemp, a_dshot=ex(a_dshot), a_dq=a_dq, a_dtemp=a_dt)


def fixed_order_mean(v):
    """(A, a) of sum_i v_i / n summed in index order from the fp32 values the kernel itself wrote"""
    n = v.numel()
    A = float(v.double().sum()) / n
    return A, sum_tol(float(v.double().abs().sum()), n) / n + 2.0 * U * abs(A)


def fixed_order_sum(v):
    A = float(v.double().sum())
    return A, sum_tol(float(v.double().abs().sum()), v.numel()) + U * abs(A)


# ------------------------------------------------------------------------------------------------------------------------------- pool_affine
def pool_affine(x, scale, shift):
    """x [B, HW, C] -> (scale * mean_hw x + shift [B, C], allowance)"""
    HW = x.shape[1]
    mean = x.sum(1) / HW
    y = mean * scale + shift
    a = scale.abs() * (sum_tol(x.abs().sum(1), HW) / HW + (E + U) * mean.abs()) + U * (mean * scale).abs() + U * y.abs()
    return y, a


# ------------------------------------------------------------------------------------------------------------------------------- linear
def linear(x, w, b=None):
    K = x.shape[1]
    y = x @ w.t() + (0.0 if b is None else b)
    return y, dot(x.abs() @ w.abs().t(), 4 * ((K + 255) // 256) + 6) + U * y.abs()


def linear_backward(dy, x, w):
    """-> dict(dx, dw, db, a_dx, a_dw, a_db); the weight gradient sums rows serially below 256 rows, in at most 64 slabs summed in order from there"""
    M, N = dy.shape
    if M >= 256:
        S = min(M // 32, 64)
        rps = (M + S - 1) // S
        S = (M + rps - 1) // rps
        n_w = rps + S
    else:
        n_w = M
    return dict(dx=dy @ w, a_dx=dot(dy.abs() @ w.abs(), N),
                dw=dy.t() @ x, a_dw=dot(dy.abs().t() @ x.abs(), n_w),
                db=dy.sum(0), a_db=sum_tol(dy.abs().sum(0), n_w))


def _fma32(a, b, s):
    """fmaf(a, b, s) of float32 arrays bit for bit: the product is exact in double (48 bits), TwoSum with s, round to odd, one rounding to float32"""
    t = a.astype(np.float64) * b.astype(np.float64)
    s = s.astype(np.float64)
    r = t + s
    bb = r - t
    err = (t - (r - bb)) + (s - bb)
    fix = (err != 0) & ((r.view(np.int64) & 1) == 0)
    return np.where(fix, np.nextafter(r, np.where(err > 0, np.inf, -np.inf)), r).astype(np.float32)


def linear_dw_bits(dy, x):
    """numpy float32 dy [M, N], x [M, K] -> (dw [N, K], db [N]) with the bits the weight-gradient kernels produce: below 256 rows one fmaf chain over the
    rows (db: plain additions); from 256 rows min(M / 32, 64) slabs of ceil(M / slabs) rows, each an fmaf chain from zero (the bias column multiplies
    by 1), the slabs added in index order.  Which of the two a row count takes is part of what this pins down."""
    M, N = dy.shape
    K = x.shape[1]
    if M >= 256:
        S = min(M // 32, 64)
        rps = (M + S - 1) // S
        S = (M + rps - 1) // rps
        x1 = np.concatenate([x, np.ones((M, 1), np.float32)], 1)
        tot = np.zeros((N, K + 1), np.float32)
        for sl in range(S):
            acc = np.zeros((N, K + 1), np.float32)
            for m in range(sl * rps, min((sl + 1) * rps, M)):
                acc = _fma32(dy[m][:, None], x1[m][None, :], acc)
            tot = tot + acc
        return tot[:, :K], tot[:, K]
    acc, db = np.zeros((N, K), np.float32), np.zeros(N, np.float32)
    for m in range(M):
        acc = _fma32(dy[m][:, None], x[m][None, :], acc)
        db = db + dy[m]
    return acc, db


# ------------------------------------------------------------------------------------------------------------------------------- token soft labels
def token_softlabel(lt, k, bp, smoothing):
    """numpy: lt [B, T, C] fp32 -> soft [B T, C + 1] fp32.  Positive tokens: the T - bp tokens with the largest per-token maximum, ties to the lower token
    index; a positive row has `on` at its k largest classes, ties to the lower class index; a background row has `on` at column 1; `off` elsewhere.
    Both tie rules are np.argsort(-x, kind='stable')."""
    lt = np.asarray(lt, dtype=np.float32)
    B, T, C = lt.shape
    off = np.float32(smoothing / C)
    on = np.float32(1.0 - smoothing + smoothing / C)
    soft = np.full((B, T, C + 1), off, dtype=np.float32)
    for b in range(B):
        order = np.argsort(-lt[b].max(1), kind='stable')
        pos = np.zeros(T, dtype=bool)
        pos[order[:T - bp]] = True
        for t in range(T):
            if pos[t]:
                soft[b, t, np.argsort(-lt[b, t], kind='stable')[:k]] = on
            else:
                soft[b, t, 1] = on
    return soft.reshape(B * T, C + 1)


# ------------------------------------------------------------------------------------------------------------------------------- soft-target CE
def soft_target_ce(z, t, gscale=None):
    """rowloss[r] = -sum_c t log_softmax(z) = lse(z) sum_c t - sum_c t z;  dz = gscale (softmax(z) sum_c t - t) -> dict(row, dz, a_row, a_dz)"""
    C = z.shape[1]
    n = wave_depth(C)
    mx = z.max(1, keepdim=True).values
    ex = (z - mx).exp()
    se = ex.sum(1, keepdim=True)
    P = ex / se
    lse = mx + se.log()
    st = t.sum(1, keepdim=True)
    tz = (t * z).sum(1, keepdim=True)
    row = lse * st - tz
    r_ex = U * (z - mx).abs() + E
    r_se = (P * r_ex).sum(1, keepdim=True) + 4.0 * math.sqrt(n) * U
    a_lse = r_se + E * se.log().abs() + U * lse.abs()
    a_st = sum_tol(t.abs().sum(1, keepdim=True), n)
    a_tz = dot((t * z).abs().sum(1, keepdim=True), n)
    a_row = st.abs() * a_lse + lse.abs() * a_st + U * (lse * st).abs() + a_tz + U * row.abs()
    out = dict(row=row.squeeze(1), a_row=a_row.squeeze(1), dz=None, a_dz=None)
    if gscale is not None:
        out['dz'] = gscale * (P * st - t)
        out['a_dz'] = abs(gscale) * (P * st.abs() * (r_ex + r_se + 2.0 * E + U) + P * a_st + U * (P * st - t).abs()) + U * out['dz'].abs()
    return out


# ------------------------------------------------------------------------------------------------------------------------------- row_normalize
def row_normalize(x):
    """-> dict(y, inv [R], a_y, a_inv)"""
    y, inv = normalize(x)
    r = _inv_rel(x)
    return dict(y=y, inv=inv.squeeze(1), a_y=y.abs() * (r + U), a_inv=(inv * r).squeeze(1))


def row_normalize_backward(y, inv, dy):
    """from the forward's stored y and inv: dx = (dy - y <y, dy>) inv -> (dx, allowance)"""
    n = wave_depth(y.shape[1])
    d = (y * dy).sum(1, keepdim=True)
    a_d = dot((y * dy).abs().sum(1, keepdim=True), n)
    inner = dy - y * d
    dx = inner * inv[:, None]
    return dx, inv[:, None] * (y.abs() * a_d + U * (y * d).abs() + U * inner.abs()) + U * dx.abs()


# ------------------------------------------------------------------------------------------------------------------------------- optimizers
def f32(v):
    """a Python float as the C entry receives it"""
    return float(np.float32(v))


def sgd(p, g, buf, lr, momentum, wd, first):
    """torch.optim.SGD (dampening 0, no nesterov): d = g + wd p; buf = d (first step) or momentum buf + d; p -= lr buf -> dict(p, buf, a_p, a_buf)"""
    lr, momentum, wd = f32(lr), f32(momentum), f32(wd)
    d = g + wd * p
    a_d = U * (wd * p).abs() + U * d.abs()
    if first:
        b, a_b = d, a_d
    else:
        b = momentum * buf + d
        a_b = a_d + U * (momentum * buf).abs() + U * b.abs()
    pn = p - lr * b
    return dict(p=pn, buf=b, a_buf=a_b, a_p=abs(lr) * a_b + U * (lr * b).abs() + U * pn.abs())


def adamw(p, g, m, v, lr, beta1, beta2, eps, wd, step, round_bc=True):
    """decoupled weight decay, update number `step` (1-based): p (1 - lr wd) - lr / bc1 * m' / (sqrt(v') / sqrt(bc2) + eps) with bc1 and 1 / sqrt(bc2)
    formed in double from the fp32 betas and rounded once (round_bc = False: kept in double, torch.optim.AdamW's own arithmetic) -> dict(p, m, v, a_p, a_m, a_v)"""
    lr, beta1, beta2, eps, wd = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(wd)
    bc1, rs = 1.0 - beta1 ** step, 1.0 / math.sqrt(1.0 - beta2 ** step)
    if round_bc:
        bc1, rs = f32(bc1), f32(rs)
    c1 = 1.0 - lr * wd
    pi = p * c1
    a_pi = p.abs() * (U * abs(lr * wd) + U * abs(c1)) + U * pi.abs()
    mi = beta1 * m + (1.0 - beta1) * g
    a_m = 2.0 * U * ((beta1 * m).abs() + ((1.0 - beta1) * g).abs()) + U * mi.abs()
    vi = beta2 * v + (1.0 - beta2) * g * g
    a_v = U * (beta2 * v).abs() + 3.0 * U * (1.0 - beta2) * g * g + U * vi.abs()
    sq = vi.sqrt()
    a_sq = torch.where(vi > 0, a_v / (2.0 * sq).clamp_min(1e-300), a_v.sqrt()) + E * sq
    den = sq * rs + eps
    a_den = rs * a_sq + U * sq * rs + U * den
    q = mi / den
    a_q = a_m / den + q.abs() * a_den / den + E * q.abs()
    k = lr / bc1
    upd = k * q
    pn = pi - upd
    return dict(p=pn, m=mi, v=vi, a_m=a_m, a_v=a_v, a_p=a_pi + abs(k) * a_q + upd.abs() * (E + U) + U * pn.abs())
