"""The float64 references of tests/test_gpu_train_ops.py (oracle/train_ops_oracle.py) held to finite differences on tiny shapes: a wrong reference
is the other way those operator tests can be wrong.  No GPU."""
import torch
import torch.nn.functional as F

from oracle import train_ops_oracle as ref


def fd(f, x, eps=1e-6):
    """central finite differences of the scalar f at x"""
    g = torch.zeros_like(x)
    flat, gf = x.reshape(-1), g.reshape(-1)
    for i in range(flat.numel()):
        old = flat[i].item()
        flat[i] = old + eps
        hi = f()
        flat[i] = old - eps
        lo = f()
        flat[i] = old
        gf[i] = (hi - lo) / (2 * eps)
    return g


def test_bn_backward_reference_is_the_gradient():
    g = torch.Generator().manual_seed(0)
    M, C, eps = 7, 4, 1e-5
    z = torch.randn(M, C, generator=g, dtype=torch.float64) + 1.0
    gamma = torch.tensor([1.2, -0.7, 0.9, -1.4], dtype=torch.float64)
    beta = torch.tensor([0.3, -0.2, 0.1, 0.0], dtype=torch.float64)
    dy = torch.randn(M, C, generator=g, dtype=torch.float64) + 0.4
    for act in (False, True):
        def loss():
            r = ref.bn_train_forward(z, gamma, beta, eps, None, act)
            return float((r['y'] * dy).sum())
        dz, dg, db = ref.bn_train_backward(dy, z, gamma, beta, eps, act)
        assert torch.allclose(dz, fd(loss, z), atol=1e-7)
        assert torch.allclose(dg, fd(loss, gamma), atol=1e-7)
        assert torch.allclose(db, fd(loss, beta), atol=1e-7)
        # the closed form the kernels evaluate: dz = ca d + cb + cc xhat with d the gradient at the BatchNorm output
        mean, var, inv = ref.bn_stats(z, eps)
        xh = (z - mean) * inv
        d = torch.where(xh * gamma + beta > 0, dy, ref.SLOPE * dy) if act else dy
        gi = gamma * inv
        assert torch.allclose(dz, gi * d - gi * d.sum(0) / M - gi * (d * xh).sum(0) / M * xh, atol=1e-12)
        assert torch.allclose(dg, (d * xh).sum(0), atol=1e-12) and torch.allclose(db, d.sum(0), atol=1e-12)


def test_bn_forward_reference_statistics():
    g = torch.Generator().manual_seed(1)
    z = torch.randn(9, 4, generator=g, dtype=torch.float64) * 2 + 3
    gamma, beta = torch.randn(4, generator=g, dtype=torch.float64), torch.randn(4, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(4, generator=g, dtype=torch.float64), torch.rand(4, generator=g, dtype=torch.float64) + 0.5
    r = ref.bn_train_forward(z, gamma, beta, 1e-5, None, False, rm, rv, 0.1)
    assert torch.allclose(r['y'], z * r['sa'] + r['sb'], atol=1e-12)
    assert torch.allclose(r['running_var'], 0.9 * rv + 0.1 * z.var(0, unbiased=True), atol=1e-12)
    assert torch.allclose(r['running_mean'], 0.9 * rm + 0.1 * z.mean(0), atol=1e-12)


def test_stem_tail_decomposition_is_the_gradient_of_the_tail():
    """pooled gradient -> route (arg-max position, LeakyReLU slope) -> two BatchNorm backwards  ==  autograd of the whole tail"""
    g = torch.Generator().manual_seed(2)
    B, OH, OW, C, eps = 2, 3, 2, 4, 1e-5
    z = torch.randn(B, 2 * OH, 2 * OW, C, generator=g, dtype=torch.float64)
    zd = torch.randn(B, 2 * OH, 2 * OW, C, generator=g, dtype=torch.float64)
    g3, b3 = torch.tensor([1.1, -0.8, 0.6, 1.3], dtype=torch.float64), torch.tensor([0.2, -0.1, -3.0, 0.4], dtype=torch.float64)
    gd, bd = torch.tensor([-0.9, 0.7, 1.2, 0.5], dtype=torch.float64), torch.tensor([0.0, 0.3, -3.0, -0.2], dtype=torch.float64)
    pos = torch.randn(OH * OW, C, generator=g, dtype=torch.float64)
    dout = torch.randn(B, OH, OW, C, generator=g, dtype=torch.float64) + 0.3
    out, dz, dzd, dg3, db3, dgd, dbd = ref.stem_tail_autograd(z, zd, g3, b3, gd, bd, eps, pos, dout)
    M0 = B * 4 * OH * OW
    s3 = ref.bn_train_forward(z.reshape(M0, C), g3, b3, eps)
    sd = ref.bn_train_forward(zd.reshape(M0, C), gd, bd, eps)
    ident = lambda t: t
    f = ref.stem_tail_forward(z, s3['sa'], s3['sb'], res=zd, rsa=sd['sa'], rsb=sd['sb'], pos=pos, rnd=ident)
    assert torch.allclose(f['out'], out, atol=1e-12)
    assert bool((f['best'] < 0).any()) and bool((f['best'] > 0).any())
    groute = ref.route(dout, f['k'], f['positive'], ident).reshape(M0, C)
    a3 = ref.bn_train_backward(groute, z.reshape(M0, C), g3, b3, eps)
    ad = ref.bn_train_backward(groute, zd.reshape(M0, C), gd, bd, eps)
    for got, want in ((a3[0], dz.reshape(M0, C)), (ad[0], dzd.reshape(M0, C)), (a3[1], dg3), (a3[2], db3), (ad[1], dgd), (ad[2], dbd)):
        assert torch.allclose(got, want, atol=1e-12)


def test_pool_reference_routes_to_the_first_of_equals():
    y = torch.tensor([[1.0, 1.0], [1.0, 0.5]], dtype=torch.float64).reshape(1, 2, 2, 1).repeat(1, 1, 1, 3).clone()
    y[0, :, :, 1] = torch.tensor([[0.0, 2.0], [2.0, 2.0]])
    y[0, :, :, 2] = torch.tensor([[-3.0, -2.0], [-1.0, -1.0]])
    best, k = ref.pool_nhwc(y)
    assert k.flatten().tolist() == [0, 1, 2] and best.flatten().tolist() == [1.0, 2.0, -1.0]
    assert ref.window_gap(y).flatten().tolist() == [0.0, 0.0, 0.0]
    dout = torch.tensor([1.0, 2.0, 4.0], dtype=torch.float64).reshape(1, 1, 1, 3)
    r = ref.route(dout, k, best > 0, lambda t: t)
    assert r[0, :, :, 0].flatten().tolist() == [1.0, 0.0, 0.0, 0.0]
    assert r[0, :, :, 1].flatten().tolist() == [0.0, 2.0, 0.0, 0.0]
    assert torch.allclose(r[0, :, :, 2].flatten(), torch.tensor([0.0, 0.0, 0.4, 0.0], dtype=torch.float64))


def test_layernorm_and_gelu_references():
    g = torch.Generator().manual_seed(3)
    M, D, eps = 3, 8, 1e-6
    x = torch.randn(M, D, generator=g, dtype=torch.float64) + 0.5
    gamma, beta = torch.randn(D, generator=g, dtype=torch.float64), torch.randn(D, generator=g, dtype=torch.float64)
    dy = torch.randn(M, D, generator=g, dtype=torch.float64)
    loss = lambda: float((ref.ln_forward(x, gamma, beta, eps)[0] * dy).sum())
    dx, dg, db = ref.ln_backward(dy, x, gamma, eps)
    assert torch.allclose(dx, fd(loss, x), atol=1e-7) and torch.allclose(dg, fd(loss, gamma), atol=1e-7) and torch.allclose(db, fd(loss, beta), atol=1e-7)
    y, mean, rstd = ref.ln_forward(x, gamma, beta, eps)
    assert torch.allclose(y, (x - mean[:, None]) * rstd[:, None] * gamma + beta, atol=1e-12)
    z = torch.randn(11, generator=g, dtype=torch.float64) * 2
    dh = torch.randn(11, generator=g, dtype=torch.float64)
    assert torch.allclose(ref.gelu_backward(dh, z), fd(lambda: float((F.gelu(z) * dh).sum()), z), atol=1e-7)


def test_unpatch2_reference():
    B, OH, OW, C = 2, 2, 3, 2
    g = torch.arange(B * OH * OW * 4 * C, dtype=torch.float64).reshape(B * OH * OW, 4 * C)
    dx = ref.unpatch2(g, B, OH, OW)
    for b in range(B):
        for oy in range(OH):
            for ox in range(OW):
                for tap in range(4):
                    assert torch.equal(dx[b, 2 * oy + tap // 2, 2 * ox + tap % 2], g[(b * OH + oy) * OW + ox, tap * C:(tap + 1) * C])
