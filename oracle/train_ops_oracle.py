"""Float64 references of the memory-bound training kernels (train_kernels.hip), one per operator entry point (fsvit_op_*).

Each is the plain formula in torch on the CPU - F.batch_norm(training=True), F.leaky_relu(., 0.1), F.max_pool2d, F.layer_norm, F.gelu - with
gradients from autograd, on operands the caller has already rounded to the storage type.  The kernels' documented rounding points are restated
through `rnd` (a function that rounds a float64 tensor to the storage type and returns float64; identity-like for fp32 storage):

* the residual add fused into bn_reduce stores T(add_a + s * add_b) and takes the statistics of the STORED values;
* out2 of bn_bwd_apply scales the value rounded to T;
* bn_pool_fwd rounds the normalised identity value T(rsa * res + rsb) before the add;
* pool_act_bwd / pool_bn_bwd_* route T(slope * dout).

tests/test_train_ops_ref_cpu.py holds these references to finite differences; tests/test_gpu_train_ops.py holds the kernels to them.

The MFMA side (tests/test_gpu_train_conv_ops.py): gelu_sig / gelu_sig_d (the sigmoid-form GELU of fsvit_common.h and its derivative), pack_weight (the
packed weight layouts of pack_weight_multi_kernel, modes 0 .. 2), stage1_block_forward / stage1_block_dgrad (the stage-1 ring kernels, every stored
map, with the kernel's own stored maps optionally standing in for the stage in front).
"""
import torch
import torch.nn.functional as F

SLOPE = 0.1


def rounder(dtype):
    """rnd(t): float64 -> rounded to `dtype` -> float64"""
    return lambda t: t.to(dtype).double()


def bn_stats(z, eps):
    """z [M,C] float64 -> mean, biased var, invstd"""
    mean = z.mean(0)
    var = z.var(0, unbiased=False)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def bn_train_forward(z, gamma, beta, eps, res=None, act=False, running_mean=None, running_var=None, momentum=0.1):
    """z [M,C]: the map the statistics are taken of (with a fused add: the stored sum).  -> dict(y, mean, invstd, sa, sb, running_mean, running_var)"""
    M = z.shape[0]
    rm = running_mean.clone() if running_mean is not None else None
    rv = running_var.clone() if running_var is not None else None
    y = F.batch_norm(z, rm, rv, gamma, beta, True, momentum, eps)          # updates rm / rv with the unbiased variance
    if res is not None:
        y = y + res
    if act:
        y = F.leaky_relu(y, SLOPE)
    mean, var, invstd = bn_stats(z, eps)
    if rm is not None:       # the update F.batch_norm made, restated
        assert torch.allclose(rm, (1 - momentum) * running_mean + momentum * mean, rtol=1e-12, atol=1e-12)
        assert torch.allclose(rv, (1 - momentum) * running_var + momentum * var * M / (M - 1), rtol=1e-12, atol=1e-12)
    return dict(y=y, mean=mean, invstd=invstd, sa=gamma * invstd, sb=beta - mean * gamma * invstd, running_mean=rm, running_var=rv)


def bn_frozen_forward(z, gamma, beta, eps, running_mean, running_var, res=None, act=False):
    y = F.batch_norm(z, running_mean, running_var, gamma, beta, False, 0.0, eps)
    if res is not None:
        y = y + res
    if act:
        y = F.leaky_relu(y, SLOPE)
    invstd = 1.0 / torch.sqrt(running_var + eps)
    return dict(y=y, mean=running_mean, invstd=invstd, sa=gamma * invstd, sb=beta - running_mean * gamma * invstd)


def bn_train_backward(dy, z, gamma, beta, eps, act=False, acc=None):
    """Gradient of sum(dy * f(BN(z))) by autograd, f = LeakyReLU(0.1) with `act` (dy is then the gradient behind it).  -> dz, dgamma, dbeta"""
    z = z.clone().requires_grad_(True)
    g = gamma.clone().requires_grad_(True)
    b = beta.clone().requires_grad_(True)
    y = F.batch_norm(z, None, None, g, b, True, 0.0, eps)
    if act:
        y = F.leaky_relu(y, SLOPE)
    dz, dg, db = torch.autograd.grad(y, (z, g, b), dy)
    return (dz if acc is None else dz + acc), dg, db


def pool_nhwc(y):
    """y [B,H,W,C] -> MaxPool2d(2) values [B,H/2,W/2,C] and the window position 0..3 of the first maximum (F.max_pool2d's choice)"""
    B, H, W, C = y.shape
    v, idx = F.max_pool2d(y.permute(0, 3, 1, 2), 2, return_indices=True)
    iy, ix = idx // W, idx % W
    k = (iy % 2) * 2 + (ix % 2)
    return v.permute(0, 2, 3, 1).contiguous(), k.permute(0, 2, 3, 1).contiguous()


def window_gap(y):
    """top-two gap of every 2 x 2 window of y [B,H,W,C] -> [B,H/2,W/2,C] (0 for an exact tie)"""
    B, H, W, C = y.shape
    w = y.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)
    top = w.topk(2, dim=-1).values
    return top[..., 0] - top[..., 1]


def stem_tail_forward(z, sa, sb, res=None, rsa=None, rsb=None, pos=None, rnd=None):
    """-> dict(y (pre-pool activated map), out, k (0..3), positive (bool))"""
    v = z * sa + sb
    if res is not None:
        r = res
        if rsa is not None:
            r = rnd(res * rsa + rsb)
        v = v + r
    y = F.leaky_relu(v, SLOPE)
    best, k = pool_nhwc(y)
    out = best if pos is None else best + pos.reshape(1, *best.shape[1:])
    return dict(y=y, out=out, k=k, positive=best > 0, best=best)


def route(dout, k, positive, rnd):
    """pooled gradient -> [B,2OH,2OW,C]: T(slope * dout) at the arg-max position, zero elsewhere"""
    B, OH, OW, C = dout.shape
    g = rnd(torch.where(positive, dout, SLOPE * dout))
    onehot = F.one_hot(k.long(), 4).to(dout.dtype)                      # [B,OH,OW,C,4]
    return (onehot * g[..., None]).reshape(B, OH, OW, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * OH, 2 * OW, C)


def stem_tail_autograd(z, zd, g3, b3, gd, bd, eps, pos, dout):
    """The whole tail by autograd in one piece: out = MaxPool(LeakyReLU(BN3(z) + BNd(zd))) + pos.  -> out, dz, dzd, dg3, db3, dgd, dbd"""
    B, H, W, C = z.shape
    ins = [t.clone().requires_grad_(True) for t in (z, zd, g3, b3, gd, bd)]
    y3 = F.batch_norm(ins[0].reshape(-1, C), None, None, ins[2], ins[3], True, 0.0, eps)
    yd = F.batch_norm(ins[1].reshape(-1, C), None, None, ins[4], ins[5], True, 0.0, eps)
    y = F.leaky_relu(y3 + yd, SLOPE).reshape(B, H, W, C)
    out = F.max_pool2d(y.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    if pos is not None:
        out = out + pos.reshape(1, H // 2, W // 2, C)
    grads = torch.autograd.grad(out, ins, dout)
    return (out.detach(),) + tuple(grads)


def ln_forward(x, gamma, beta, eps):
    y = F.layer_norm(x, (x.shape[-1],), gamma, beta, eps)
    mean = x.mean(-1)
    rstd = 1.0 / torch.sqrt(x.var(-1, unbiased=False) + eps)
    return y, mean, rstd


def ln_backward(dy, x, gamma, eps, add=None):
    x = x.clone().requires_grad_(True)
    g = gamma.clone().requires_grad_(True)
    b = torch.zeros_like(gamma).requires_grad_(True)
    y = F.layer_norm(x, (x.shape[-1],), g, b, eps)
    dx, dg, db = torch.autograd.grad(y, (x, g, b), dy)
    if add is not None:
        dx = dx + add
    return dx, dg, db


def gelu_backward(dh, z):
    z = z.clone().requires_grad_(True)
    return torch.autograd.grad(F.gelu(z), z, dh)[0]


def unpatch2(g, B, OH, OW):
    C = g.shape[1] // 4
    return g.reshape(B, OH, OW, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * OH, 2 * OW, C)


# ------------------------------------------------------------------------------------------------ the MFMA side
# gelu_sig of fsvit_common.h: x * sigmoid(x * poly(x^2)) with x^2 clamped at 64; the three fp32 coefficients carry the -log2(e) of the exp2
_GS_C2, _GS_C1, _GS_C0 = (float(torch.tensor(v, dtype=torch.float32)) for v in (1.0153755e-3, -1.0678257e-1, -2.3011138))
_LN2 = 0.69314718055994530942


def _gelu_sig_s(z):
    u = (z * z).clamp(max=64.0)
    p = (_GS_C2 * u + _GS_C1) * u + _GS_C0
    return u, 1.0 / (1.0 + torch.exp2(z * p))


def gelu_sig(z):
    return z * _gelu_sig_s(z)[1]


def gelu_sig_d(z):
    """d/dz gelu_sig as the kernels evaluate it: s (1 + z (1 - s) q(u)), q = d/dz [z poly(z^2)] = c0 + 3 c1 u + 5 c2 u^2 (kept beyond the clamp of u,
    where s (1 - s) < 2e-12 has long vanished)"""
    u, s = _gelu_sig_s(z)
    q = ((5.0 * _GS_C2 * u + 3.0 * _GS_C1) * u + _GS_C0) * -_LN2
    return s * (1.0 + z * (1.0 - s) * q)


def _pad_heads(t, dim, hd, hdp):
    """index j of `dim` -> (j / hd) * hdp + j % hd, the slots hd .. hdp - 1 of every head zero"""
    if hd == hdp:
        return t
    shape = list(t.shape)
    n = shape[dim]
    assert n % hd == 0
    t = t.unflatten(dim, (n // hd, hd))
    pad = [0, 0] * (t.dim() - dim - 2) + [0, hdp - hd]
    return F.pad(t, pad).flatten(dim, dim + 1)


def pack_weight(w, groups=1, mode=0, rows_pad=None, Kw=None, hd_rows=1, hdp_rows=1, hd_cols=1, hdp_cols=1):
    """PyTorch conv weight w [O, Ig, KH, KW] -> packed [groups, rows_pad, Kw] (the layout comment above pack_weight_multi_kernel):
      mode 0: row = output channel of the group, column = (ky, kx, input channel)
      mode 1: row = input channel of the group, column = (ky, kx, output channel) of the taps rotated by 180 degrees
      mode 2: row = (ky, kx, input channel), column = output channel
    rows / columns head-padded hd -> hdp (modes 0 / 1), then zero-filled up to rows_pad x Kw."""
    O, Ig, KH, KW = w.shape
    v = w.reshape(groups, O // groups, Ig, KH, KW)
    if mode == 0:
        m = v.permute(0, 1, 3, 4, 2)
    elif mode == 1:
        m = v.flip(3, 4).permute(0, 2, 3, 4, 1)
    elif mode == 2:
        m = v.permute(0, 3, 4, 2, 1).flatten(1, 3)
    else:
        raise ValueError(mode)
    if mode != 2:
        m = m.flatten(2)
        m = _pad_heads(_pad_heads(m, 1, hd_rows, hdp_rows), 2, hd_cols, hdp_cols)
    rows_pad, Kw = rows_pad or m.shape[1], Kw or m.shape[2]
    out = torch.zeros(groups, rows_pad, Kw, dtype=w.dtype)
    out[:, :m.shape[1], :m.shape[2]] = m
    return out


def gconv(h, w, groups, transposed=False):
    """h NHWC [B,H,W,C], w [O, Ig, 3, 3]: the 3 x 3 / pad 1 convolution, or its transpose (the gradient with respect to its input) -> NHWC"""
    f = F.conv_transpose2d if transposed else F.conv2d
    return f(h.permute(0, 3, 1, 2), w, None, 1, 1, groups=groups).permute(0, 2, 3, 1)


def stage1_block_forward(x, w1f, b1f, w2, w3, sa, sb, scale, rnd, h1_stored=None, h2_stored=None):
    """The training forward of a stage-1 block as stage1_ring.hip MODE 3 stores it.  x [B,H,W,128]; w1f [256,128] / b1f [256]: conv1 with the BatchNorm folded;
    w2 [256,32,3,3] (8 groups); w3 [128,256]; sa / sb [128]; scale [B] or None; every operand already rounded to its storage type.  h1 / h2 are rounded (rnd)
    where they are stored and consumed rounded.  h1_stored / h2_stored: maps (the kernel's own, read back) that stand in for this function's h1 / h2 in
    the stages behind them.  Returns the stored maps, the pre-activations z1 / z2 / the conv3 result acc3, and for the error bounds the sums of the
    magnitudes of each dot product's terms (abs1 / abs2 / abs3)."""
    B = x.shape[0]
    z1 = x @ w1f.T + b1f
    h1, g1 = rnd(gelu_sig(z1)), rnd(gelu_sig_d(z1))
    h1u = h1 if h1_stored is None else h1_stored
    z2 = gconv(h1u, w2, 8)
    h2, g2 = rnd(gelu_sig(z2)), rnd(gelu_sig_d(z2))
    h2u = h2 if h2_stored is None else h2_stored
    acc3 = h2u @ w3.T
    sc = torch.ones(B, dtype=x.dtype) if scale is None else scale
    out = rnd(x + sc[:, None, None, None] * acc3)
    return dict(xn=rnd(x * sa + sb), z1=z1, h1=h1, g1=g1, z2=z2, h2=h2, g2=g2, acc3=acc3, out=out, abs1=x.abs() @ w1f.abs().T,
                abs2=gconv(h1u.abs(), w2.abs(), 8), abs3=h2u.abs() @ w3.abs().T)


def stage1_block_dgrad(dz3, w3, w2, w1, g2, g1, rnd, dz2_stored=None, dz1_stored=None):
    """The block's data-gradient chain as stage1_ring.hip MODE 2 stores it: dz2 = T((dz3 W3) * g2), dz1 = T(conv2^T(dz2) * g1), dxn = T(dz1 W1), with w3
    [128,256], w2 [256,32,3,3], w1 [256,128] in the FORWARD layout (the kernel reads their transposed packs).  dz2_stored / dz1_stored as above."""
    acc2 = dz3 @ w3
    dz2 = rnd(acc2 * g2)
    d2 = dz2 if dz2_stored is None else dz2_stored
    acc1 = gconv(d2, w2, 8, transposed=True)
    dz1 = rnd(acc1 * g1)
    d1 = dz1 if dz1_stored is None else dz1_stored
    acc0 = d1 @ w1
    return dict(acc2=acc2, dz2=dz2, acc1=acc1, dz1=dz1, acc0=acc0, dxn=rnd(acc0), abs2=dz3.abs() @ w3.abs(), abs1=gconv(d2.abs(), w2.abs(), 8, transposed=True),
                abs0=d1.abs() @ w1.abs())
