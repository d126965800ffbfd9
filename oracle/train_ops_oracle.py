"""Float64 references of the memory-bound training kernels (train_kernels.hip), one per operator entry point (fsvit_op_*).

Each is the plain formula in torch on the CPU - F.batch_norm(training=True), F.leaky_relu(., 0.1), F.max_pool2d, F.layer_norm, F.gelu - with
gradients from autograd, on operands the caller has already rounded to the storage type.  The kernels' documented rounding points are restated
through `rnd` (a function that rounds a float64 tensor to the storage type and returns float64; identity-like for fp32 storage):

* the residual add fused into bn_reduce stores T(add_a + s * add_b) and takes the statistics of the STORED values;
* out2 of bn_bwd_apply scales the value rounded to T;
* bn_pool_fwd rounds the normalised identity value T(rsa * res + rsb) before the add;
* pool_act_bwd / pool_bn_bwd_* route T(slope * dout).

tests/test_train_ops_ref_cpu.py holds these references to finite differences; tests/test_gpu_train_ops.py holds the kernels to them.
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
