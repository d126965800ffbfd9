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


# ------------------------------------------------------------------------------------------------ references of tests/test_gpu_train_conv_ops.py
def test_gelu_sig_reference():
    """gelu_sig is within the 2.6e-5 of F.gelu that fsvit_common.h claims; gelu_sig_d is its derivative."""
    z = torch.arange(-12.0, 12.0 + 5e-4, 1e-3, dtype=torch.float64)
    assert float((ref.gelu_sig(z) - F.gelu(z)).abs().max()) <= 2.6e-5
    zr = z.clone().requires_grad_(True)
    auto = torch.autograd.grad(ref.gelu_sig(zr).sum(), zr)[0]
    d = ref.gelu_sig_d(z)
    inside = z.abs() <= 8.0                                  # z^2 <= 64: not clamped, the kernel's closed form IS the derivative
    assert float((d - auto)[inside].abs().max()) <= 1e-12
    # beyond the clamp the function's polynomial is constant and its true derivative has p(64) where the closed form keeps q(z^2 = 64); the sigmoid has
    # saturated there, s (1 - s) <= 2^-39: the two differ by less than 1e-10 (and the kernels' fp32 cannot see it)
    assert float((d - auto)[~inside].abs().max()) <= 1e-10
    # and against the erf form's derivative: the two GELUs differ by 2.6e-5 in value, their slopes by well under 1e-3
    assert float((d - ref.gelu_backward(torch.ones_like(z), z)).abs().max()) <= 1e-3


def _patches(x, KH, KW, pad, groups, stride=1):
    """x NCHW -> [B * OH * OW, groups, (ky, kx, c)]: the rows an implicit GEMM multiplies the packed weights with"""
    B, Cc = x.shape[:2]
    cols = F.unfold(x, (KH, KW), padding=pad, stride=stride)                       # [B, (c, ky, kx), L]
    L = cols.shape[-1]
    return cols.reshape(B, groups, Cc // groups, KH * KW, L).permute(0, 4, 1, 3, 2).reshape(B * L, groups, KH * KW * (Cc // groups))


def _pad_channels(t, hd, hdp):
    """channels (last dim) of whole heads hd -> hdp, zero slots"""
    return F.pad(t.unflatten(-1, (t.shape[-1] // hd, hd)), (0, hdp - hd)).flatten(-2)


def test_pack_weight_reference_is_the_convolution():
    """A matmul of the im2col rows with the packed rows equals F.conv2d (mode 0), the gradient of the conv with respect to its input (mode 1: autograd
    and F.conv_transpose2d; mode 2: the 2 x 2 / stride 2 patch conv) - with and without groups, and with head padding 42 -> 48 of the rows and of the
    columns."""
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    for (O, Ig, groups, k) in ((8, 6, 1, 1), (12, 4, 1, 3), (12, 2, 3, 3), (8, 4, 2, 1)):
        B, H, W, pad = 2, 4, 5, k // 2
        w, x = rn(O, Ig, k, k), rn(B, groups * Ig, H, W)
        Ng = O // groups
        want = F.conv2d(x, w, None, 1, pad, groups=groups).permute(0, 2, 3, 1).reshape(B * H * W, O)
        pk = ref.pack_weight(w, groups, 0, rows_pad=Ng + 3, Kw=k * k * Ig + 5)
        assert pk.shape == (groups, Ng + 3, k * k * Ig + 5)
        assert float(pk[:, Ng:].abs().max()) == 0.0 and float(pk[:, :, k * k * Ig:].abs().max()) == 0.0
        got = torch.einsum('mgk,gnk->mgn', _patches(x, k, k, pad, groups), pk[:, :Ng, :k * k * Ig]).reshape(B * H * W, O)
        assert torch.allclose(got, want, atol=1e-12)
        # mode 1: a stride-1 conv of dY with the transposed, tap-flipped pack is the transposed convolution
        dy = rn(B, O, H, W)
        xr = x.clone().requires_grad_(True)
        dx = torch.autograd.grad(F.conv2d(xr, w, None, 1, pad, groups=groups), xr, dy)[0]
        assert torch.allclose(dx, F.conv_transpose2d(dy, w, None, 1, pad, groups=groups), atol=1e-12)
        pk1 = ref.pack_weight(w, groups, 1)
        assert pk1.shape == (groups, Ig, k * k * Ng)
        got = torch.einsum('mgk,gck->mgc', _patches(dy, k, k, pad, groups), pk1).reshape(B * H * W, groups * Ig)
        assert torch.allclose(got, dx.permute(0, 2, 3, 1).reshape(B * H * W, groups * Ig), atol=1e-12)
    # mode 2 (and mode 0) of the non-overlapping 2 x 2 / stride 2 patch conv
    B, OH, OW, O, Ig = 2, 3, 2, 6, 4
    w, x, dy = rn(O, Ig, 2, 2), rn(B, Ig, 2 * OH, 2 * OW), rn(B, O, OH, OW)
    got = torch.einsum('mgk,gnk->mgn', _patches(x, 2, 2, 0, 1, stride=2), ref.pack_weight(w, 1, 0)).reshape(B * OH * OW, O)
    assert torch.allclose(got, F.conv2d(x, w, None, 2).permute(0, 2, 3, 1).reshape(B * OH * OW, O), atol=1e-12)
    xr = x.clone().requires_grad_(True)
    dx = torch.autograd.grad(F.conv2d(xr, w, None, 2), xr, dy)[0].permute(0, 2, 3, 1)
    pk2 = ref.pack_weight(w, 1, 2, rows_pad=4 * Ig, Kw=O + 2)
    assert float(pk2[:, :, O:].abs().max()) == 0.0
    rows = dy.permute(0, 2, 3, 1).reshape(B * OH * OW, O) @ pk2[0, :, :O].T                # [M][(ky, kx, i)]
    assert torch.allclose(ref.unpatch2(rows, B, OH, OW), dx, atol=1e-12)
    # head padding 42 -> 48: qkv rows (3 * 2 heads), proj columns (2 heads), forward and transposed
    hd, hdp, heads, Cc, M = 42, 48, 2, 8, 5
    wq, xq = rn(3 * heads * hd, Cc, 1, 1), rn(M, Cc)
    pq = ref.pack_weight(wq, 1, 0, rows_pad=3 * heads * hdp + 4, Kw=16, hd_rows=hd, hdp_rows=hdp)
    want = _pad_channels(xq @ wq[:, :, 0, 0].T, hd, hdp)
    assert torch.allclose((xq @ pq[0, :, :Cc].T)[:, :3 * heads * hdp], want, atol=1e-12) and float(pq[0, 3 * heads * hdp:].abs().max()) == 0.0
    assert float(pq[0].reshape(-1, 16)[:3 * heads * hdp].reshape(3 * heads, hdp, 16)[:, hd:].abs().max()) == 0.0 and float(pq[0, :, Cc:].abs().max()) == 0.0
    wp, ctx = rn(Cc, heads * hd, 1, 1), rn(M, heads * hd)
    pp = ref.pack_weight(wp, 1, 0, Kw=128, hd_cols=hd, hdp_cols=hdp)
    assert torch.allclose(_pad_channels(ctx, hd, hdp) @ pp[0, :, :heads * hdp].T, ctx @ wp[:, :, 0, 0].T, atol=1e-12)
    assert float(pp[0, :, heads * hdp:].abs().max()) == 0.0 and float(pp[0, :, :heads * hdp].reshape(Cc, heads, hdp)[:, :, hd:].abs().max()) == 0.0
    # transposed: d(x) from the padded dqkv (rows = input channels, padded columns), d(ctx) padded from dy (padded rows)
    dq = rn(M, 3 * heads * hd)
    pq1 = ref.pack_weight(wq, 1, 1, hd_cols=hd, hdp_cols=hdp)
    assert torch.allclose(_pad_channels(dq, hd, hdp) @ pq1[0].T, dq @ wq[:, :, 0, 0], atol=1e-12)
    dyp = rn(M, Cc)
    pp1 = ref.pack_weight(wp, 1, 1, hd_rows=hd, hdp_rows=hdp)
    assert torch.allclose(dyp @ pp1[0].T, _pad_channels(dyp @ wp[:, :, 0, 0], hd, hdp), atol=1e-12)


def test_stage1_block_references():
    """stage1_block_forward is the block of torch ops it restates (conv1 + BatchNorm folded, GELU, grouped 3 x 3, GELU, conv3, scaled residual) and
    stage1_block_dgrad is autograd of it (with the stored GELU derivatives as multipliers), on a non-square map."""
    g = torch.Generator().manual_seed(12)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    B, H, W = 2, 3, 5
    x, w1, w2, w3 = rn(B, H, W, 128), rn(256, 128) * 0.1, rn(256, 32, 3, 3) * 0.06, rn(128, 256) * 0.06
    sa, sb, scale = rn(128), rn(128), torch.tensor([0.0, 1.25], dtype=torch.float64)
    ident = lambda t: t
    w1f, b1f = w1 * sa, w1 @ sb
    r = ref.stage1_block_forward(x, w1f, b1f, w2, w3, sa, sb, scale, ident)
    xr = x.clone().requires_grad_(True)
    xn = xr * sa + sb
    gs = lambda t: t * torch.sigmoid(-ref._LN2 * t * ((ref._GS_C2 * (t * t).clamp(max=64) + ref._GS_C1) * (t * t).clamp(max=64) + ref._GS_C0))
    z1 = F.conv2d(xn.permute(0, 3, 1, 2), w1[:, :, None, None])
    z2 = F.conv2d(gs(z1), w2, None, 1, 1, groups=8)
    br = F.conv2d(gs(z2), w3[:, :, None, None]).permute(0, 2, 3, 1)
    out = x + scale[:, None, None, None] * br
    assert torch.allclose(r['xn'], xn.detach(), atol=1e-12) and torch.allclose(r['z1'], z1.detach().permute(0, 2, 3, 1), atol=1e-11)
    assert torch.allclose(r['z2'], z2.detach().permute(0, 2, 3, 1), atol=1e-11) and torch.allclose(r['out'], out.detach(), atol=1e-11)
    assert torch.equal(r['out'][0], x[0]), 'scale 0: the image passes through'
    assert torch.allclose(r['abs1'], x.abs() @ w1f.abs().T) and bool((r['abs3'] >= r['acc3'].abs() - 1e-12).all()) and bool((r['abs2'] >= (r['z2']).abs() - 1e-12).all())
    # stored maps standing in: the stage behind uses them
    r2 = ref.stage1_block_forward(x, w1f, b1f, w2, w3, sa, sb, scale, ident, h1_stored=torch.zeros_like(r['h1']))
    assert float(r2['z2'].abs().max()) == 0.0 and torch.equal(r2['h1'], r['h1'])
    dz3 = rn(B, H, W, 128)
    d = ref.stage1_block_dgrad(dz3, w3, w2, w1, r['g2'], r['g1'], ident)
    dxn = torch.autograd.grad(br, xn, dz3)[0]
    assert torch.allclose(d['dxn'], dxn, atol=1e-10)
    d2 = ref.stage1_block_dgrad(dz3, w3, w2, w1, r['g2'], r['g1'], ident, dz1_stored=torch.zeros_like(d['dz1']))
    assert float(d2['dxn'].abs().max()) == 0.0 and torch.equal(d2['dz2'], d['dz2'])
