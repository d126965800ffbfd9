"""Operator tests of the memory-bound training kernels (train_kernels.hip) through the fsvit_op_* entry points, against float64 torch on the CPU
(oracle/train_ops_oracle.py: autograd of the plain formula on operands pre-rounded to the storage type, the kernels' rounding points restated).

Launchers of train_kernels.h and where they are held:
  bn_reduce / bn_fwd_finalize / bn_frozen_coeffs / bn_apply                 test_bn_train_forward, test_bn_frozen, test_bn_variance_ratio
  bn_reduce (bwd) / bn_bwd_finalize / bn_bwd_apply, bn_act_bwd              test_bn_train_backward
  bn_pool_fwd, maxpool2_idx, pool_act_bwd, maxpool2_bwd,
  pool_bn_bwd_reduce / _apply, bn_*_finalize_nblk                           test_stem_tail
  ln_train_fwd, ln_bwd (+ ln_param_grad)                                    test_layernorm
  vit_assemble, vit_patch_rows, vit_cls_ln_fwd / _bwd                       test_vit_cls_ln_and_tokens
  gelu_fwd / gelu_bwd, add_scaled, avgpool_bwd, batch_sum, bcast_add,
  colsum, unpatch2, droppath_scales, fold_prenorm                           test_elementwise, test_batch_sum, test_small_ops
 covered elsewhere: launch_sgd* (test_gpu_train: SGD), launch_attention_bwd (test_gpu_attention_ops.py), launch_proto_head*_bwd (test_gpu_train.py);
 launch_pack_weight_multi (modes 0 / 1 / 2, head padding, two-limb words, the 40-job table), the training epilogues of launch_conv_gemm / launch_gconv3x3
 (y2, ACT_MUL, mul) and launch_stage1_ring_block_train / launch_stage1_ring_dgrad: test_gpu_train_conv_ops.py, same conventions; fill_f32 / scale_copy:
 test_small_ops.  Reached only through whole train steps (the golden / oracle step tests of test_gpu_train.py, no operator entry): launch_patchk,
 launch_im2col_t, launch_transpose_cols, launch_wgrad_finalize_multi.
Storage types: fp32 and bf16.  train_kernels.hip is a single-build source (Makefile SINGLE): there is no f16 build of these kernels, the trainers take
fp32 / bf16 / bf16x2 only, and the entries reject f16 (test_rejections) instead of reading f16 bits as bf16.

Tolerances (u = 2^-24; every bound is computed from the reference and the inputs, never from the kernel's output):
 * a value stored in the storage type T: |err| <= half_ulp_T(ref) + a, where a bounds the fp32 evaluation of the expression: c * u * (sum of the
   magnitudes of its terms) with c = the number of roundings, plus the propagated bounds of fp32 inputs that are themselves kernel results
   (coefficients).  half_ulp_T is the exact half ulp of the reference's binade, 2^(e-24) for fp32 and 2^(e-8) for bf16 (between 2^-9 and 2^-8
   relative; the binade is taken of |ref| + a so that a reference just below a power of two is not held to the smaller ulp).
 * an fp32 sum: the kernels add `depth` terms in one fp32 chain (per-thread row walk, then an in-order LDS pass) and finish across blocks in
   fp64.  The bound is of the worst-case kind: a chain of d additions errs by at most d * u * sum|term|; we allow 4 * sqrt(depth) * u * sum|term|,
   i.e. that worst case scaled by 4 / sqrt(depth) (rounding errors of a chain do not all point one way; sqrt(depth) is their random-walk growth,
   4 the headroom), with depth from the documented block layout (rows per thread + row lanes).  This is NOT the form k * u * sqrt(M) * max|term|
   with k read off torch's own fp32 sum: torch's CPU sum is a vectorised cascade whose error grows like log M and sits two to three orders below
   any depth-d chain at M = 40000, so a k from it would refuse a correct chain-summing kernel, and max|term| * sqrt(M) mis-sizes one-signed sums
   (z^2).  The bound is still fp32-grade (about 1e-6 relative on a mean) and 20 x or more inside the mutations the suite must catch (a dropped
   row, M - 1).  Beside every sum the test prints torch's fp32 sum error on the same terms for comparison.
 * discrete outputs (arg, routed gradients): exact.  Windows whose float64 top-two gap is non-zero and below 2^-20 * max(1, |y|) (or whose maximum
   is non-zero and that close to 0) are skipped, at most 0.1 % per case (asserted); exact ties are never skipped.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TD = {'f32': torch.float32, 'bf16': torch.bfloat16}
PBITS = {'f32': 24, 'bf16': 8}
DTS = ['f32', 'bf16']
LRELU = 2


def _mods():
    from fewshot_vit_amd.engine import ops
    from oracle import train_ops_oracle as ref
    return ops, ref


def gen(seed):
    return torch.Generator().manual_seed(seed)


def q(t, dt):
    """round to the storage type; float64 result"""
    return t.to(TD[dt]).double()


def dev(t, dt=None):
    if t is None:
        return None
    return (t.to(TD[dt]) if dt else t.float()).contiguous().cuda()


def half_ulp(ref, dt, a):
    mag = (ref.abs() + a).clamp_min(2.0 ** -120)
    return torch.ldexp(torch.ones_like(mag), (torch.floor(torch.log2(mag)) - PBITS[dt]).to(torch.int32))


def stored_tol(ref, dt, a):
    return half_ulp(ref, dt, a) + a


def check(name, got, ref, tol, mask=None):
    err = (got.detach().double().cpu() - ref).abs()
    tol = tol if torch.is_tensor(tol) else torch.full_like(err, float(tol))
    tol = tol.expand_as(err)
    if mask is not None:
        err, tol = err[mask], tol[mask]
    if err.numel() == 0:
        return
    ratio = err / tol.clamp_min(1e-300)
    i = int(ratio.argmax())
    print(f'    {name}: max err {float(err.max()):.3e}, worst err/bound {float(ratio.flatten()[i]):.3f} (bound there {float(tol.flatten()[i]):.3e})')
    assert bool((err <= tol).all()), (name, float(err.max()), float(ratio.max()))


def ref32_sum_err(terms):
    """error of torch's own fp32 sum over dim 0 against float64 (printed beside the kernel's)"""
    return float((terms.float().sum(0).double() - terms.sum(0)).abs().max())


def channel_params(C, g, signed=True):
    cm = (torch.rand(C, generator=g, dtype=torch.float64) * 3 - 1.5)
    cs = 0.5 + 1.5 * torch.rand(C, generator=g, dtype=torch.float64)
    gamma = (0.5 + torch.rand(C, generator=g, dtype=torch.float64)) * (torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0) if signed else 1.0)
    beta = torch.rand(C, generator=g, dtype=torch.float64) - 0.5
    return cm, cs, gamma.float().double(), beta.float().double()


# ------------------------------------------------------------------------------------------------ BatchNorm
def bn_layout(M, C, dt):
    """block layout of bn_reduce_kernel: (blocks, row lanes R, rows per thread n)"""
    V = 8 if (dt == 'bf16' and C % 8 == 0) else 4
    LC = min(C // V, 256)
    R = 256 // LC
    nblk = min((M + 63) // 64, 512)
    return nblk, R, -(-M // (nblk * R))


def sum_tol(abs_terms_sum, depth):
    return 4.0 * math.sqrt(depth) * U * abs_terms_sum


def clamp_M(C, dt, delta):
    nblk, R, _ = bn_layout(40000, C, dt)
    return 4 * nblk * R + delta


# (M, C); M < 0: 4 * step + M + 2 rows of the clamped 512-block grid (so -3 -> 4 step - 1, -1 -> 4 step + 1)
# (12800, 256): a stage-1-sized map of 32 images (20 x 20 x 256); the 800-image map takes minutes in float64.
# (40000, 96) / (40000, 132): the element-indexed apply kernels at a large M (C = 96: 12 / 24 channel lanes, idle threads in the reduce) and the
#   4-channel bf16 lanes of bn_reduce (C % 8 != 0) in their 4-unrolled walk + scalar tail on the clamped 512-block grid.
# (17000, 1024) fp32 / (17000, 2048) bf16: 256 channel lanes, one row lane (R = 1) -> rows_grid() CLAMPS at 4096 blocks (M > 4096 * R * U = 16384 in the
#   forward, U = 4; 8192 in the backward, U = 2): the row loops of bn_apply_rows / bn_bwd_apply_rows repeat, with the `mm < M` guard live in the last
#   iteration and scale2[mm / rows_per_img] on later iterations.  (The other storage type takes the element-indexed kernels there - fp32 C = 2048 has
#   512 lanes - or stays below the clamp, so each case runs in the one type that takes it.)
BN_CASES = [(2, 8), (63, 64), (64, 96), (65, 128), (70, 132), (1000, 256), (130, 2048), (66, 4096), (40000, 8), (40000, 64), (-3, 64), (-1, 64),
            (12800, 256), (40000, 96), (40000, 132), (17000, 1024, 'f32'), (17000, 2048, 'bf16')]
BN_PARAMS = [(c[:2], dt) for c in BN_CASES for dt in DTS if len(c) == 2 or c[2] == dt]
BN_IDS = [(f'M{m}_C{c}' if m > 0 else f'M4step{m + 2:+d}_C{c}') + '-' + dt for (m, c), dt in BN_PARAMS]


def rows_form_sweeps(M, C, dt, U):
    """iterations of the row loop of bn_apply_rows (U = 4) / bn_bwd_apply_rows (U = 2), or 0 where the element-indexed kernel runs"""
    V = 4 if dt == 'f32' else 8
    if C % V or C // V > 256 or 256 % (C // V):
        return 0
    R = 256 // (C // V)
    nb = min(max(-(-M // (R * U)), 1), 4096)
    return -(-M // (nb * R * U))


def rows_per_img_of(M):
    for d in (400, 100, 64, 31, 16, 13, 11, 10, 9, 7, 5, 3, 2):
        if M % d == 0 and M // d >= 2:
            return d
    return 1


def bn_fwd_bounds(z, gamma, beta, eps, M, C, dt):
    """bounds on mean / invstd / sa / sb / var from the layout of the reduce pass (module docstring)"""
    nblk, R, n = bn_layout(M, C, dt)
    depth = n + R
    mean, var = z.mean(0), z.var(0, unbiased=False)
    inv = 1.0 / torch.sqrt(var + eps)
    e0, e1 = sum_tol(z.abs().sum(0), depth), sum_tol((z * z).sum(0), depth)
    t_mean_x = e0 / M                                            # before the fp32 rounding of the output
    t_var = e1 / M + 2 * mean.abs() * t_mean_x + t_mean_x ** 2
    t_inv = 0.5 * inv ** 3 * t_var + 2 * U * inv
    t_mean = t_mean_x + U * mean.abs()
    t_sa = gamma.abs() * t_inv + 2 * U * (gamma * inv).abs()
    t_sb = gamma.abs() * (mean.abs() * t_inv + inv * t_mean) + 4 * U * (beta.abs() + (mean * gamma * inv).abs())
    return dict(mean=t_mean, var=t_var, invstd=t_inv, sa=t_sa, sb=t_sb, depth=depth)


@pytest.mark.parametrize('variant', ['plain', 'add', 'add_res_act'])
@pytest.mark.parametrize('case,dt', BN_PARAMS, ids=BN_IDS)
def test_bn_train_forward(case, dt, variant):
    """bn_reduce (+ fused residual add) -> bn_fwd_finalize (+ running statistics) -> bn_apply (+ res, LeakyReLU), every output against float64."""
    ops, ref = _mods()
    M, C = case
    if M < 0:
        M = clamp_M(C, dt, M + 2)
        assert bn_layout(M, C, dt)[0] == 512
    if M == 17000:
        assert rows_form_sweeps(M, C, dt, 4) == 2, 'this case is here for the clamped rows_grid'
    g = gen(1000 + 7 * C + M % 1000)
    cm, cs, gamma, beta = channel_params(C, g)
    eps, mom = 1e-5, 0.1
    rm0, rv0 = torch.randn(C, generator=g).double(), (0.5 + torch.rand(C, generator=g)).double()
    rm, rv = dev(rm0), dev(rv0)
    mk = lambda: q(torch.randn(M, C, generator=g, dtype=torch.float64) * cs + cm, dt)
    if variant == 'plain':
        z = mk()
        zk = dev(z, dt)
        y, mean, invstd, sa, sb = ops.bn_train_forward(zk, dev(gamma), dev(beta), rm, rv, eps, mom)
        res, act = None, False
    else:
        rpi = rows_per_img_of(M)
        a, b = mk(), mk()
        zk = torch.full((M, C), float('nan'), dtype=TD[dt]).cuda()
        if variant == 'add':                   # the fused add without per-image scales, nothing behind the BatchNorm
            y, mean, invstd, sa, sb = ops.bn_train_forward(zk, dev(gamma), dev(beta), rm, rv, eps, mom, add_a=dev(a, dt), add_b=dev(b, dt))
            res, sb_ = None, b
        else:
            scale = (0.5 + torch.rand(M // rpi, generator=g)).double()
            res = q(torch.randn(M, C, generator=g, dtype=torch.float64), dt)
            y, mean, invstd, sa, sb = ops.bn_train_forward(zk, dev(gamma), dev(beta), rm, rv, eps, mom, add_a=dev(a, dt), add_b=dev(b, dt), add_scale=dev(scale),
                                                           rows_per_img=rpi, res=dev(res, dt), act=LRELU)
            sb_ = scale.repeat_interleave(rpi)[:, None] * b
        want = a + sb_
        # the stored sum: fp32 a + s * b (two roundings, or one when fused), then the rounding to T
        check('stored add', zk, want, stored_tol(want, dt, 2 * U * (a.abs() + sb_.abs())))
        z = zk.double().cpu()                      # the statistics are those of the STORED values
        act = variant == 'add_res_act'
    r = ref.bn_train_forward(z, gamma, beta, eps, res, act, rm0, rv0, mom)
    t = bn_fwd_bounds(z, gamma, beta, eps, M, C, dt)
    print(f'\n  bn_fwd M={M} C={C} {dt} {variant}: depth {t["depth"]}, torch fp32 sum error: z {ref32_sum_err(z):.2e}, z^2 {ref32_sum_err(z * z):.2e} '
          f'(kernel bound on the sums {float(sum_tol(z.abs().sum(0), t["depth"]).max()):.2e} / {float(sum_tol((z * z).sum(0), t["depth"]).max()):.2e})')
    check('mean', mean, r['mean'], t['mean'])
    check('invstd', invstd, r['invstd'], t['invstd'])
    check('sa', sa, r['sa'], t['sa'])
    check('sb', sb, r['sb'], t['sb'])
    check('running_mean', rm, r['running_mean'], mom * t['mean'] + 4 * U * (rm0.abs() + r['mean'].abs()))
    check('running_var', rv, r['running_var'], mom * t['var'] * M / (M - 1) + 4 * U * (rv0.abs() + z.var(0)))
    pre = (z * r['sa']).abs() + r['sb'].abs() + (res.abs() if res is not None else 0)
    a_y = z.abs() * t['sa'] + t['sb'] + 4 * U * pre
    check('y', y, r['y'], stored_tol(r['y'], dt, a_y))
    # determinism: block-ordered partial sums
    zk2 = dev(z, dt)
    _, mean2, invstd2, _, _ = ops.bn_train_forward(zk2, dev(gamma), dev(beta), None, None, eps, mom, apply=False)
    _, mean3, invstd3, _, _ = ops.bn_train_forward(zk2, dev(gamma), dev(beta), None, None, eps, mom, apply=False)
    assert torch.equal(mean2, mean3) and torch.equal(invstd2, invstd3)
    if variant == 'plain':
        assert torch.equal(mean2, mean) and torch.equal(invstd2, invstd)


@pytest.mark.parametrize('dt', DTS)
def test_bn_frozen(dt):
    """bn_frozen_coeffs + the un-fused add + bn_apply (running statistics normalise, nothing is updated); C = 96 takes the element-indexed apply."""
    ops, ref = _mods()
    M, C, eps = 130, 96, 1e-5
    g = gen(5)
    cm, cs, gamma, beta = channel_params(C, g)
    rm0, rv0 = torch.randn(C, generator=g).double(), (0.5 + torch.rand(C, generator=g)).double()
    a, b = q(torch.randn(M, C, generator=g, dtype=torch.float64) * cs + cm, dt), q(torch.randn(M, C, generator=g, dtype=torch.float64), dt)
    scale = (0.5 + torch.rand(M // 13, generator=g)).double()
    rm, rv = dev(rm0), dev(rv0)
    zk = torch.zeros(M, C, dtype=TD[dt]).cuda()
    y, mean, invstd, sa, sb = ops.bn_train_forward(zk, dev(gamma), dev(beta), rm, rv, eps, 0.1, frozen=True, add_a=dev(a, dt), add_b=dev(b, dt), add_scale=dev(scale),
                                                   rows_per_img=13, act=LRELU)
    assert torch.equal(rm.cpu(), rm0.float()) and torch.equal(rv.cpu(), rv0.float())
    sb_ = scale.repeat_interleave(13)[:, None] * b
    check('stored add', zk, a + sb_, stored_tol(a + sb_, dt, 2 * U * (a.abs() + sb_.abs())))
    z = zk.double().cpu()
    r = ref.bn_frozen_forward(z, gamma, beta, eps, rm0, rv0, None, True)
    check('invstd', invstd, r['invstd'], 2 * U * r['invstd'])
    check('sa', sa, r['sa'], 4 * U * r['sa'].abs())
    check('sb', sb, r['sb'], 6 * U * (beta.abs() + (rm0 * r['sa']).abs()))
    a_y = z.abs() * 4 * U * r['sa'].abs() + 6 * U * (beta.abs() + (rm0 * r['sa']).abs()) + 4 * U * ((z * r['sa']).abs() + r['sb'].abs())
    check('y', y, r['y'], stored_tol(r['y'], dt, a_y))


@pytest.mark.parametrize('variant', ['plain', 'act', 'acc_out2', 'act_acc_out2'])
@pytest.mark.parametrize('case,dt', BN_PARAMS, ids=BN_IDS)
def test_bn_train_backward(case, dt, variant):
    """bn_reduce (backward form, + LeakyReLU gradient) -> bn_bwd_finalize -> bn_bwd_apply (+ acc, scale2, out2, in place) against autograd of
    F.batch_norm in float64.  dy has a per-channel mean (cb) and is correlated with xhat (cc).  acc_out2: acc + per-image scale2 + out2;
    act_acc_out2: the LeakyReLU gradient, acc and out2 WITHOUT scale2 in one call."""
    ops, ref = _mods()
    M, C = case
    if M < 0:
        M = clamp_M(C, dt, M + 2)
    if M == 17000:
        assert rows_form_sweeps(M, C, dt, 2) == 3, 'this case is here for the clamped rows_grid'
    g = gen(2000 + 7 * C + M % 1000)
    cm, cs, gamma, beta = channel_params(C, g)
    eps = 1e-5
    z = q(torch.randn(M, C, generator=g, dtype=torch.float64) * cs + cm, dt)
    mean, var, inv = ref.bn_stats(z, eps)
    mean, inv = mean.float().double(), inv.float().double()                 # the kernel's fp32 inputs
    xh = (z - mean) * inv
    dmean = torch.rand(C, generator=g, dtype=torch.float64) - 0.3
    dy = q(torch.randn(M, C, generator=g, dtype=torch.float64) + dmean + 0.5 * xh * torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0), dt)
    kw, rkw = {}, {}
    sa = (gamma * inv).float().double()
    sb = (beta - mean * gamma * inv).float().double()
    d_eff = dy
    near = torch.zeros(M, C, dtype=torch.bool)
    if 'act' in variant.split('_'):
        kw = dict(act_sa=dev(sa), act_sb=dev(sb))
        yv = z * sa + sb
        near = yv.abs() < 2.0 ** -20 * (1 + (z * sa).abs() + sb.abs())        # the sign of an activation input this close to 0 is fp32 noise
        d_eff = torch.where(yv > 0, dy, 0.1 * dy)
    rpi = rows_per_img_of(M)
    acc = scale2 = None
    with_out2 = variant.endswith('acc_out2')
    if with_out2:
        acc = q(torch.randn(M, C, generator=g, dtype=torch.float64), dt)
        if variant == 'acc_out2':
            scale2 = (0.5 + torch.rand(M // rpi, generator=g)).double()
    dyk, zk = dev(dy, dt), dev(z, dt)
    out2k = torch.empty_like(zk) if with_out2 else None
    dz, dgamma, dbeta, coef = ops.bn_train_backward(dyk, zk, dev(mean), dev(inv), dev(gamma), acc=dev(acc, dt), scale2=dev(scale2), out2=out2k, rows_per_img=rpi, **kw)
    # reference: autograd of F.batch_norm (+ LeakyReLU with the kernel's fp32 sa / sb deciding the sign: y = sa z + sb)
    zr = z.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.batch_norm(zr, None, None, gr, br, True, 0.0, eps)
    gz, gg, gb = torch.autograd.grad(y, (zr, gr, br), d_eff)
    if acc is not None:
        gz = gz + acc
    nblk, R, n = bn_layout(M, C, dt)
    depth = n + R
    flip = 0.9 * (near * dy.abs()).sum(0)
    xerr = 4 * U * (dy.abs() * (z.abs() + mean.abs()) * inv).sum(0)          # xhat evaluated in fp32
    # the reference normalises with the float64 statistics of z, the kernel with their fp32 roundings: xhat moves by u (|mean| + |xhat|)
    stat = 2 * U * (d_eff.abs() * (mean.abs() * inv + xh.abs())).sum(0)
    e0 = sum_tol(d_eff.abs().sum(0), depth) + flip
    e1 = sum_tol((d_eff * xh).abs().sum(0), depth) + flip * xh.abs().max(0).values + xerr + stat
    print(f'\n  bn_bwd M={M} C={C} {dt} {variant}: depth {depth}, torch fp32 sum error: dy {ref32_sum_err(d_eff):.2e}, dy*xhat {ref32_sum_err(d_eff * xh):.2e} '
          f'(kernel bound {float(e0.max()):.2e} / {float(e1.max()):.2e}), near-zero activation inputs {int(near.sum())}')
    assert near.float().mean() <= 1e-3
    check('dbeta', dbeta, gb, e0 + U * gb.abs())
    check('dgamma', dgamma, gg, e1 + U * gg.abs())
    gi = gamma * inv
    ca, cb, cc = gi, -gi * gb / M, -gi * gg / M
    t_cb, t_cc = gi.abs() * e0 / M + 4 * U * cb.abs(), gi.abs() * e1 / M + 4 * U * cc.abs()
    check('ca', coef[0], ca, 2 * U * ca.abs())
    check('cb', coef[1], cb, t_cb)
    check('cc', coef[2], cc, t_cc)
    mag = (ca * d_eff).abs() + cb.abs() + (cc * xh).abs() + (acc.abs() if acc is not None else 0)
    a_dz = 8 * U * mag + t_cb + t_cc * xh.abs() + cc.abs() * 2 * U * ((z.abs() + mean.abs()) * inv + mean.abs() * inv + xh.abs())
    check('dz', dz, gz, stored_tol(gz, dt, a_dz), mask=~near)
    if with_out2:
        # out2 scales the STORED dz (rounded to T): one fp32 product, one rounding to T (no scale2: the stored dz itself)
        want = dz.double().cpu() * (scale2.float().double().repeat_interleave(rpi)[:, None] if scale2 is not None else 1.0)
        check('out2', out2k, want, stored_tol(want, dt, U * want.abs()))
        # in place, as the engine aliases: dz == acc, out2 == dy -> bit-identical to the separate buffers
        acck, dyk2 = dev(acc, dt), dev(dy, dt)
        dz_i, dg_i, db_i, _ = ops.bn_train_backward(dyk2, zk, dev(mean), dev(inv), dev(gamma), acc=acck, scale2=dev(scale2), out2=dyk2, rows_per_img=rpi, dz=acck, **kw)
        assert torch.equal(dz_i, dz) and torch.equal(dyk2, out2k) and torch.equal(dg_i, dgamma) and torch.equal(db_i, dbeta)
    else:
        dz2, dg2, db2, _ = ops.bn_train_backward(dyk, zk, dev(mean), dev(inv), dev(gamma), **kw)
        assert torch.equal(dz2, dz) and torch.equal(dg2, dgamma) and torch.equal(db2, dbeta)
    if variant == 'act' and M <= 1000:
        # bn_act_bwd (the separate LeakyReLU-gradient pass) + the plain backward = the fused form, to the rounding of the stored gradient
        gk = ops.bn_act_bwd(dyk, zk, dev(sa), dev(sb))
        check('bn_act_bwd', gk, d_eff, stored_tol(d_eff, dt, 2 * U * d_eff.abs()), mask=~near)
        frozen = ops.bn_train_backward(dyk, zk, dev(mean), dev(inv), dev(gamma), frozen=True, **kw)
        check('frozen dz', frozen[0], ca * d_eff, stored_tol(ca * d_eff, dt, 4 * U * (ca * d_eff).abs()), mask=~near)
        assert float(frozen[3][1:].abs().max()) == 0.0


# largest |mean| / std over the 21 pre-BatchNorm maps of visformer_micro_80 (synthetic checkpoint, 30 synthetic images, oracle stats_out): 3.5
# (patch_embed2.norm), 2.2 in stage 1, 1.7 in the stem.  Ratios the network reaches are gated; the others are measured and printed.
REACHABLE_RATIO = 4


@pytest.mark.parametrize('ratio', [0, 4, 10, 100, 1000])
def test_bn_variance_ratio(ratio):
    """The variance is s1 / M - mean^2 from fp32 per-block partial sums (fp64 in the finalize only): it cancels when a channel's mean is large
    against its std.  fp32 storage, M = 40000, C = 64, channel mean = +-ratio * std.  Gate: 4 x the error of an fp32 TWO-PASS torch computation
    (x.float().var) of the same input against float64 - for ratio <= 4, which bounds what the network produces (3.5, see above).

    Measured on an MI355X, kernel (two-pass gate):      relative invstd error        max |y| error
      ratio 0                                           4.7e-08 (3.5e-07)            4.0e-07 (2.6e-06)
      ratio 4                                           1.5e-07 (4.8e-07)            8.4e-07 (4.3e-06)
      ratio 10                                          9.4e-07 (4.0e-07)  over      4.1e-06 (7.6e-06)
      ratio 100                                         7.3e-05 (4.3e-07)  over      3.0e-04 (8.3e-05)  over
      ratio 1000                                        7.7e-03 (3.8e-07)  over      3.7e-02 (6.0e-04)  over
    The single-pass form loses ~ratio^2 * 2^-24 * sqrt(chain depth) of the variance; beyond ratio ~5 it is worse than a two-pass fp32 computation.
    No pre-BatchNorm map of this network comes near that, so the kernel keeps its single pass (training section) and ratios above
    REACHABLE_RATIO are printed, not gated."""
    ops, ref = _mods()
    M, C, eps = 40000, 64, 1e-5
    g = gen(77 + ratio)
    std = (0.5 + 1.5 * torch.rand(C, generator=g)).double()
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).double()
    x = (torch.randn(M, C, generator=g, dtype=torch.float64) * std + sign * ratio * std).float().double()
    ones, zeros = torch.ones(C), torch.zeros(C)
    y, mean, invstd, sa, sb = ops.bn_train_forward(dev(x, 'f32'), dev(ones), dev(zeros), None, None, eps, 0.1)
    m64, v64, i64 = ref.bn_stats(x, eps)
    y64 = (x - m64) * i64
    x32 = x.float()
    i32 = 1.0 / torch.sqrt(x32.var(0, unbiased=False) + eps)
    y32 = (x32 - x32.mean(0)) * i32
    gate_i = 4 * float(((i32.double() - i64) / i64).abs().max())
    gate_y = 4 * float((y32.double() - y64).abs().max())
    err_i = float(((invstd.double().cpu() - i64) / i64).abs().max())
    err_y = float((y.double().cpu() - y64).abs().max())
    gated = ratio <= REACHABLE_RATIO
    print(f'\n  bn variance ratio {ratio} ({"gated" if gated else "measured only"}): rel invstd err {err_i:.3e} (gate {gate_i:.3e}), '
          f'max |y| err {err_y:.3e} (gate {gate_y:.3e})')
    assert bool(torch.isfinite(invstd).all()) and bool(torch.isfinite(y).all())
    if gated:
        assert err_i <= gate_i and err_y <= gate_y, (ratio, err_i, gate_i, err_y, gate_y)


# ------------------------------------------------------------------------------------------------ stem tail
def pool_layout(npix, C, dt):
    V = 4 if dt == 'f32' else 8
    R = 256 // (C // V)
    nb = min(-(-npix // R), 512)
    return nb, R, -(-npix // (nb * R))


STEM_CASES = [(1, 1, 1, 8), (3, 20, 20, 128), (2, 7, 9, 96), (70, 20, 20, 128)]


# the 70-image case is there for the block walk of the reductions: it runs the full form (identity BatchNorm + pos + backward) only
STEM_PARAMS = [(c, o) for c in STEM_CASES for o in ('plain', 'pos', 'res', 'res_pos', 'res_bn_pos') if c[0] < 70 or o == 'res_bn_pos']


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('case,opts', STEM_PARAMS, ids=['x'.join(map(str, c)) + '-' + o for c, o in STEM_PARAMS])
def test_stem_tail(case, opts, dt):
    """bn_pool_fwd (BN + identity BN + LeakyReLU + MaxPool2d(2) + pos, arg code) and the backwards behind it - pool_bn_bwd_reduce / _apply fused,
    pool_act_bwd + two bn_train_backward unfused - against float64, and the fused forms against the unfused chain of the same library.
    C = 96: the channel lanes (24 fp32 / 12 bf16) do not divide 256 - the forward runs, the fused backward is REJECTED (asserted), the unfused
    chain is the path there.  (70, 20, 20, 128): 28000 pooled pixels > 512 blocks x 8 (16) pixel lanes: blocks walk several pixel groups."""
    ops, ref = _mods()
    B, OH, OW, C = case
    g = gen(3000 + B + C)
    rnd = ref.rounder(TD[dt])
    eps = 1e-5
    H, W = 2 * OH, 2 * OW
    M0 = B * H * W
    cm, cs, g3, b3 = channel_params(C, g)
    _, _, gd, bd = channel_params(C, g)
    b3 = b3.clone()
    b3[1] = -6.0                                   # channel 1: all-negative windows (arg & 4 clear, slope 0.1)
    b3[0] = 0.0
    bd = bd.clone()
    bd[0] = 0.0
    z = q(torch.randn(B, H, W, C, generator=g, dtype=torch.float64) * cs + cm, dt)
    zd = q(torch.randn(B, H, W, C, generator=g, dtype=torch.float64) * cs.flip(0) - cm, dt)
    # planted exact ties (the same z and zd at two or four window positions) in ~2 % of the windows; rounding to bf16 makes more
    wz = z.reshape(B, OH, 2, OW, 2, C)
    wd = zd.reshape(B, OH, 2, OW, 2, C)
    plant = torch.rand(B, OH, OW, C, generator=g)
    for (lo, hi, src, dst) in ((0.0, 0.005, (0, 0), (1, 1)), (0.005, 0.01, (0, 1), (1, 0)), (0.01, 0.015, (1, 0), (1, 1)), (0.015, 0.02, (0, 0), (0, 1))):
        m = (plant >= lo) & (plant < hi)
        for w in (wz, wd):
            w[:, :, dst[0], :, dst[1], :] = torch.where(m, w[:, :, src[0], :, src[1], :], w[:, :, dst[0], :, dst[1], :])
    # y == 0 exactly: channel 0 (positive gamma, shifts zeroed below), z = zd = 0 in whole windows (a tie at zero) and at single positions next to
    # negative values
    zero_w = plant[..., 0] > 0.9
    for w in (wz, wd):
        for dy_ in (0, 1):
            for dx_ in (0, 1):
                w[:, :, dy_, :, dx_, 0] = torch.where(zero_w, torch.zeros(()).double(), w[:, :, dy_, :, dx_, 0])
    one_zero = (plant[..., 0] > 0.8) & ~zero_w
    assert g3[0] > 0 and gd[0] > 0
    sgn = sgnd = 1.0
    for dy_ in (0, 1):
        for dx_ in (0, 1):
            first = dy_ == 1 and dx_ == 0                 # the zero sits at window position 2
            wz[:, :, dy_, :, dx_, 0] = torch.where(one_zero, torch.zeros(()).double() if first else -sgn * (1.0 + wz[:, :, dy_, :, dx_, 0].abs()), wz[:, :, dy_, :, dx_, 0])
            wd[:, :, dy_, :, dx_, 0] = torch.where(one_zero, torch.zeros(()).double() if first else -sgnd * wd[:, :, dy_, :, dx_, 0].abs(), wd[:, :, dy_, :, dx_, 0])
    z, zd = q(wz.reshape(B, H, W, C), dt), q(wd.reshape(B, H, W, C), dt)
    zk, zdk = dev(z, dt), dev(zd, dt)
    # statistics of the library itself (held to float64 by test_bn_train_forward) are the fp32 coefficients of both the kernel and the reference
    _, mean3, is3, sa3, sb3 = ops.bn_train_forward(zk.reshape(M0, C), dev(g3), dev(b3), apply=False)
    _, meand, isd, sad, sbd = ops.bn_train_forward(zdk.reshape(M0, C), dev(gd), dev(bd), apply=False)
    sa3c, sb3c, sadc, sbdc = sa3.clone(), sb3.clone(), sad.clone(), sbd.clone()
    sb3c[0] = 0.0
    sbdc[0] = 0.0
    pos = (torch.randn(OH * OW, C, generator=g) * 0.5).double() if opts.endswith('pos') else None
    f64 = lambda t: t.double().cpu()
    if opts in ('plain', 'pos'):
        out, arg = ops.stem_tail_train_forward(zk, sa3c, sb3c, pos=dev(pos))
        r = ref.stem_tail_forward(z, f64(sa3c), f64(sb3c), pos=pos)
        mag = (z * f64(sa3c)).abs() + f64(sb3c).abs()
    elif opts in ('res', 'res_pos'):
        out, arg = ops.stem_tail_train_forward(zk, sa3c, sb3c, res=zdk, pos=dev(pos))
        r = ref.stem_tail_forward(z, f64(sa3c), f64(sb3c), res=zd, pos=pos)
        mag = (z * f64(sa3c)).abs() + f64(sb3c).abs() + zd.abs()
    else:
        out, arg = ops.stem_tail_train_forward(zk, sa3c, sb3c, res=zdk, rsa=sadc, rsb=sbdc, pos=dev(pos))
        r = ref.stem_tail_forward(z, f64(sa3c), f64(sb3c), res=zd, rsa=f64(sadc), rsb=f64(sbdc), pos=pos, rnd=rnd)
        mag = (z * f64(sa3c)).abs() + f64(sb3c).abs() + (zd * f64(sadc)).abs() + f64(sbdc).abs()
    y, best = r['y'], r['best']
    gap = ref.window_gap(y)
    skip = ((gap > 0) & (gap < 2.0 ** -20 * best.abs().clamp_min(1.0))) | ((best != 0) & (best.abs() < 2.0 ** -20))
    if opts == 'res_bn_pos' and dt != 'f32':
        # T(rsa * res + rsb) is rounded from an fp32 value that the compiler may form with one rounding (fma) or two (mul, add); where those two
        # or the float64 value round to different T the window's values differ by an ulp of T between legitimate evaluations: such windows are
        # found on the reference side alone and count as skipped
        v = zd * f64(sadc) + f64(sbdc)
        two = (zd.float() * sadc.cpu()) + sbdc.cpu()
        amb = (rnd(two.double()) != rnd(v)) | (rnd(v.float().double()) != rnd(v))
        skip = skip | amb.reshape(B, OH, 2, OW, 2, C).any(dim=4).any(dim=2)
    share = float(skip.float().mean())
    ties = float((gap == 0).float().mean())
    print(f'\n  stem tail {case} {dt} {opts}: skipped windows {share:.5f}, exact ties {ties:.4f}, all-negative windows {float((best < 0).float().mean()):.3f}, '
          f'zero maxima {int((best == 0).sum())}')
    assert share <= 1e-3
    assert ties > 0 or B * OH * OW * C < 1000
    argc = arg.cpu()
    keep = ~skip
    assert torch.equal((argc & 3)[keep].long(), r['k'][keep].long()), 'arg-max position (first of equals, as F.max_pool2d)'
    assert torch.equal(((argc & 4) != 0)[keep], r['positive'][keep]), 'arg & 4 = the maximum is positive'
    assert int((argc >> 3).max()) == 0
    wmag = F.max_pool2d(mag.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    a_out = 4 * U * wmag + (U * pos.abs().reshape(1, OH, OW, C) if pos is not None else 0)
    check('out', out, r['out'], stored_tol(r['out'], dt, a_out), mask=keep)

    # ---- unfused forward chain of the same library: bn_apply (identity) -> bn_apply + res + LeakyReLU -> maxpool2_idx + pos
    if opts == 'res_bn_pos':
        yd_k, *_ = ops.bn_train_forward(zdk.reshape(M0, C), dev(gd), dev(bd))
        y_k, *_ = ops.bn_train_forward(zk.reshape(M0, C), dev(g3), dev(b3), res=yd_k, act=LRELU)
        # (the chain runs on the library's own coefficients, without the zeroed channel-0 shifts of the float64 comparison above)
        out_f, arg_f = ops.stem_tail_train_forward(zk, sa3, sb3, res=zdk, rsa=sad, rsb=sbd, pos=dev(pos))
        out_u, arg_u = ops.maxpool2_idx(y_k.reshape(B, H, W, C), dev(pos))
        yk64 = y_k.reshape(B, H, W, C).double().cpu()
        bk, kk = ref.pool_nhwc(yk64)
        assert torch.equal(arg_u.cpu().long(), kk.long()), 'maxpool2_idx: first of equals on the stored map'
        wantu = bk + pos.reshape(1, OH, OW, C)
        check('maxpool2_idx out', out_u, wantu, stored_tol(wantu, dt, U * (bk.abs() + pos.abs().reshape(1, OH, OW, C))))
        # fused vs unfused: the unfused chain rounds the activated map to T before the pool, the fused one does not -> one more half ulp of T
        of = out_f.double().cpu()
        check('fused vs unfused out', out_u, of, 2 * half_ulp(of, dt, 0 * of) + 2 * half_ulp(bk, dt, 0 * bk) + 8 * U * wmag)
        clear = ref.window_gap(yk64) > 0
        agree = ((arg_f.cpu() & 3) == arg_u.cpu())[clear & keep]
        print(f'    fused vs unfused arg: {float(agree.float().mean()):.5f} equal over the windows whose stored map has a unique maximum')
        # both chains form the same fp32 values up to the contraction of one multiply-add; the unfused chain then rounds them to T before pooling.
        # Rounding is monotone: it can merge two values into a tie (removed by `clear`) but never invert their order, so in both storage types
        # the positions agree wherever the stored map has a unique maximum, except for fp32 contraction noise at near-ties (<= 0.1 %)
        assert float(agree.float().mean()) >= 0.999
        din = ops.maxpool2_bwd(out_u, arg_u).double().cpu()
        wantd = (F.one_hot(kk.long(), 4).double() * out_u.double().cpu()[..., None]).reshape(B, OH, OW, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, H, W, C)
        assert torch.equal(din, wantd), 'maxpool2_bwd: exact scatter'

    # ---- backward: routed gradient and the two BatchNorm backwards
    if opts != 'res_bn_pos':
        return
    dout = q(torch.randn(B, OH, OW, C, generator=g, dtype=torch.float64) + 0.3 + 0.2 * r['best'].clamp(-2, 2), dt)
    doutk = dev(dout, dt)
    k_k, pos_k = (argc & 3), (argc & 4) != 0
    groute = ref.route(dout, k_k, pos_k, rnd)
    g_k = ops.pool_act_bwd(doutk, arg)
    check('pool_act_bwd', g_k, groute, stored_tol(groute, dt, 2 * U * groute.abs()))
    m3, i3, md, idd = f64(mean3), f64(is3), f64(meand), f64(isd)
    zf, zdf = z.reshape(M0, C), zd.reshape(M0, C)
    gfl = groute.reshape(M0, C)
    npix = B * OH * OW

    def bn_bwd_ref(zz, mu, inv, gam):
        xh = (zz - mu) * inv
        s0, s1 = gfl.sum(0), (gfl * xh).sum(0)
        gi = gam * inv
        return xh, s0, s1, gi, -gi * s0 / M0, -gi * s1 / M0

    def bounds(zz, mu, inv, gam, depth):
        xh, s0, s1, gi, cb, cc = bn_bwd_ref(zz, mu, inv, gam)
        e0 = sum_tol(gfl.abs().sum(0), depth)
        e1 = sum_tol((gfl * xh).abs().sum(0), depth) + 4 * U * (gfl.abs() * (zz.abs() + mu.abs()) * inv).sum(0)
        t_cb, t_cc = gi.abs() * e0 / M0 + 4 * U * cb.abs(), gi.abs() * e1 / M0 + 4 * U * cc.abs()
        ref_dz = gi * gfl + cb + cc * xh
        a_dz = 8 * U * ((gi * gfl).abs() + cb.abs() + (cc * xh).abs()) + t_cb + t_cc * xh.abs() + cc.abs() * 2 * U * (zz.abs() + mu.abs()) * inv
        return s0, s1, e0, e1, ref_dz, a_dz

    # (xhat with the library's fp32 statistics as given inputs: this is the formula of the BatchNorm backward at those statistics)
    fused_ok = (256 % (C // (4 if dt == 'f32' else 8)) == 0)
    nb, R, n = pool_layout(npix, C, dt) if fused_ok else (0, 0, 0)
    outs = {}
    if fused_ok:
        outs['fused'] = ops.stem_tail_train_backward(doutk, arg, zk, zdk, mean3, is3, meand, isd, dev(g3), dev(gd))
        again = ops.stem_tail_train_backward(doutk, arg, zk, zdk, mean3, is3, meand, isd, dev(g3), dev(gd))
        assert all(torch.equal(a_, b_) for a_, b_ in zip(outs['fused'], again)), 'pool_bn_bwd_*: bit-reproducible'
    else:
        with pytest.raises(ValueError, match='row-walking'):
            ops.stem_tail_train_backward(doutk, arg, zk, zdk, mean3, is3, meand, isd, dev(g3), dev(gd))
    u3 = ops.bn_train_backward(g_k.reshape(M0, C), zk.reshape(M0, C), mean3, is3, dev(g3))
    ud = ops.bn_train_backward(g_k.reshape(M0, C), zdk.reshape(M0, C), meand, isd, dev(gd))
    outs['unfused'] = (u3[0].reshape(B, H, W, C), ud[0].reshape(B, H, W, C), u3[1], u3[2], ud[1], ud[2])
    for name, o in outs.items():
        if name == 'fused':
            depth = n + R
        else:
            bl = bn_layout(M0, C, dt)
            depth = bl[2] + bl[1]
        for tag, zz, mu, inv, gam, dzk, dgk, dbk in (('bn3', zf, m3, i3, g3, o[0], o[2], o[3]), ('bn_d', zdf, md, idd, gd, o[1], o[4], o[5])):
            s0, s1, e0, e1, ref_dz, a_dz = bounds(zz, mu, inv, gam, depth)
            check(f'{name} {tag} dbeta', dbk, s0, e0 + U * s0.abs())
            check(f'{name} {tag} dgamma', dgk, s1, e1 + U * s1.abs())
            check(f'{name} {tag} dz', dzk.reshape(M0, C), ref_dz, stored_tol(ref_dz, dt, a_dz))
    if fused_ok:
        # the pair agrees to accumulation order: same terms, a different walk -> the two sum bounds, and two roundings of the stored maps
        f, u_ = outs['fused'], outs['unfused']
        for i, tag in ((2, 'dgamma3'), (3, 'dbeta3'), (4, 'dgammad'), (5, 'dbetad')):
            zz, mu, inv, gam = (zf, m3, i3, g3) if i < 4 else (zdf, md, idd, gd)
            bl = bn_layout(M0, C, dt)
            _, _, e0a, e1a, _, _ = bounds(zz, mu, inv, gam, n + R)
            _, _, e0b, e1b, _, _ = bounds(zz, mu, inv, gam, bl[2] + bl[1])
            check(f'fused vs unfused {tag}', f[i], u_[i].double().cpu(), (e1a + e1b) if i % 2 == 0 else (e0a + e0b))


@pytest.mark.parametrize('dt', DTS)
def test_stem_backward_apply_grid_clamp(dt):
    """pool_bn_bwd_apply clamps its grid at 8192 blocks: with 256 channel lanes (one pixel lane per block: C = 1024 fp32, 2048 bf16) and 8400 pooled
    pixels (21 x 20 x 20) blocks 0 .. 207 walk a second pixel.  Maps of 34 / 69 M elements are too large for a float64 reference in a test, so this
    case holds the fused backward to the UNFUSED chain of the same library (pool_act_bwd + two bn_train_backward, each held to float64 at smaller
    shapes above): same terms, same coefficients formula, a different walk.  Bounds as in test_stem_tail's pair check, evaluated on the GPU in
    float64: the two sum bounds for the parameter gradients; for the maps two roundings to T plus the propagated coefficient difference."""
    ops, ref = _mods()
    B, OH, OW = 21, 20, 20
    C = 1024 if dt == 'f32' else 2048
    npix, M0 = B * OH * OW, B * OH * OW * 4
    assert npix > 8192 and 256 // (C // (4 if dt == 'f32' else 8)) == 1
    gg = torch.Generator(device='cuda').manual_seed(9)
    rn = lambda *sh: torch.randn(*sh, generator=gg, device='cuda')
    cs, cm = 0.5 + 1.5 * torch.rand(C, generator=gg, device='cuda'), torch.rand(C, generator=gg, device='cuda') * 3 - 1.5
    z3 = (rn(B, 2 * OH, 2 * OW, C) * cs + cm).to(TD[dt])
    zd = (rn(B, 2 * OH, 2 * OW, C) * cs.flip(0) - cm).to(TD[dt])
    sign = torch.where(torch.arange(C, device='cuda') % 3 == 1, -1.0, 1.0)
    g3, gd = (0.5 + torch.rand(C, generator=gg, device='cuda')) * sign, (0.5 + torch.rand(C, generator=gg, device='cuda')) * sign.flip(0)
    b3, bd = torch.rand(C, generator=gg, device='cuda') - 0.5, torch.rand(C, generator=gg, device='cuda') - 0.5
    _, mean3, is3, sa3, sb3 = ops.bn_train_forward(z3.reshape(M0, C), g3, b3, apply=False)
    _, meand, isd, sad, sbd = ops.bn_train_forward(zd.reshape(M0, C), gd, bd, apply=False)
    out, arg = ops.stem_tail_train_forward(z3, sa3, sb3, res=zd, rsa=sad, rsb=sbd)
    dout = (rn(B, OH, OW, C) + 0.3).to(TD[dt])
    fused = ops.stem_tail_train_backward(dout, arg, z3, zd, mean3, is3, meand, isd, g3, gd)
    gk = ops.pool_act_bwd(dout, arg).reshape(M0, C)
    u3 = ops.bn_train_backward(gk, z3.reshape(M0, C), mean3, is3, g3)
    ud = ops.bn_train_backward(gk, zd.reshape(M0, C), meand, isd, gd)
    nb, R, n = pool_layout(npix, C, dt)
    bl = bn_layout(M0, C, dt)
    d_f, d_u = n + R, bl[2] + bl[1]
    g64 = gk.double()
    print(f'\n  stem backward grid clamp {dt}: {npix} pooled pixels, C = {C}')
    for tag, zz, mu, inv, gam, (dz_f, dg_f, db_f), (dz_u, dg_u, db_u) in (
            ('bn3', z3, mean3, is3, g3, (fused[0], fused[2], fused[3]), (u3[0], u3[1], u3[2])),
            ('bn_d', zd, meand, isd, gd, (fused[1], fused[4], fused[5]), (ud[0], ud[1], ud[2]))):
        zz64, mu, inv, gam = zz.reshape(M0, C).double(), mu.double(), inv.double(), gam.double()
        xh = (zz64 - mu) * inv
        e0 = sum_tol(g64.abs().sum(0), d_f) + sum_tol(g64.abs().sum(0), d_u)
        e1 = sum_tol((g64 * xh).abs().sum(0), d_f) + sum_tol((g64 * xh).abs().sum(0), d_u) + 8 * U * (g64.abs() * (zz64.abs() + mu.abs()) * inv).sum(0)
        s0, s1 = g64.sum(0), (g64 * xh).sum(0)
        for name, a_, b_, e in (('dbeta', db_f, db_u, e0 + 2 * U * s0.abs()), ('dgamma', dg_f, dg_u, e1 + 2 * U * s1.abs())):
            err = (a_.double() - b_.double()).abs()
            print(f'    {tag} {name}: max |fused - unfused| {float(err.max()):.3e}, worst err/bound {float((err / e).max()):.3f}')
            assert bool((err <= e).all())
        gi = (gam * inv).abs()
        val = gam * inv * g64 - gam * inv * s0 / M0 - gam * inv * s1 / M0 * xh
        a_dz = 16 * U * ((gam * inv * g64).abs() + (gi * s0.abs() / M0) + (gi * s1.abs() / M0 * xh.abs())) + gi * e0 / M0 + gi * e1 / M0 * xh.abs()
        bound = 2 * (torch.ldexp(torch.ones_like(val), (torch.floor(torch.log2((val.abs() + a_dz).clamp_min(2.0 ** -120))) - PBITS[dt]).to(torch.int32)) + a_dz)
        err = (dz_f.reshape(M0, C).double() - dz_u.double()).abs()
        print(f'    {tag} dz: max |fused - unfused| {float(err.max()):.3e}, worst err/bound {float((err / bound).max()):.3f}')
        assert bool((err <= bound).all())
        del zz64, xh, val, a_dz, bound, err
    again = ops.stem_tail_train_backward(dout, arg, z3, zd, mean3, is3, meand, isd, g3, gd)
    assert all(torch.equal(a_, b_) for a_, b_ in zip(fused, again))


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_CASES = [(1, 4), (3, 64), (64, 192), (65, 256), (591, 260), (591, 384), (65, 768), (64, 1024), (3, 1028), (65, 2048), (70000, 64), (70000, 192)]


def ln_inputs(M, D, dt, g):
    rs = 0.5 + 1.5 * torch.rand(M, 1, generator=g, dtype=torch.float64)
    rmu = torch.rand(M, 1, generator=g, dtype=torch.float64) * 2 - 1
    col = torch.randn(D, generator=g, dtype=torch.float64) * 0.5
    x = q(torch.randn(M, D, generator=g, dtype=torch.float64) * rs + rmu + col, dt)
    gamma = ((0.5 + torch.rand(D, generator=g)) * torch.where(torch.arange(D) % 3 == 1, -1.0, 1.0)).double()
    beta = (torch.rand(D, generator=g) - 0.5).double()
    return x, gamma, beta


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('case', LN_CASES, ids=[f'M{m}_D{d}' for m, d in LN_CASES])
def test_layernorm(case, dt):
    """ln_train_fwd and ln_bwd (the NG = 1 .. 4 register forms for D <= 1024, the generic LDS form above; 1024 blocks clamp at M = 70000), with and
    without `add` (also in place), with null dgamma / dbeta, against F.layer_norm autograd in float64."""
    ops, ref = _mods()
    M, D = case
    eps = 1e-6
    g = gen(4000 + M + D)
    x, gamma, beta = ln_inputs(M, D, dt, g)
    xk = dev(x, dt)
    y, mean, rstd = ops.ln_train_forward(xk, dev(gamma), dev(beta), eps)
    yr, mr, rr = ref.ln_forward(x, gamma, beta, eps)
    # one wave per row: a lane adds ceil(D / 256) * 4 values in a chain, then 6 shuffle levels; mean and variance are formed in fp32
    depth = 4 * -(-D // 256) + 6
    e0 = sum_tol(x.abs().sum(1), depth) / D
    e1 = sum_tol((x * x).sum(1), depth) / D
    t_mean = e0 + 2 * U * mr.abs()
    t_var = e1 + 2 * mr.abs() * t_mean + 4 * U * ((x * x).mean(1) + mr * mr)
    t_rstd = 0.5 * rr ** 3 * t_var + 4 * U * rr
    print(f'\n  layernorm M={M} D={D} {dt}: torch fp32 row-sum error x {float((x.float().sum(1).double() - x.sum(1)).abs().max()):.2e} '
          f'(kernel bound on the sum {float((e0 * D).max()):.2e})')
    check('mean', mean, mr, t_mean)
    check('rstd', rstd, rr, t_rstd)
    xh = (x - mr[:, None]) * rr[:, None]
    a_y = (rr[:, None] * t_mean[:, None] + (x - mr[:, None]).abs() * t_rstd[:, None]) * gamma.abs() + 6 * U * ((xh * gamma).abs() + beta.abs()) \
        + 2 * U * (x.abs() + mr.abs()[:, None]) * rr[:, None] * gamma.abs()
    check('y', y, yr, stored_tol(yr, dt, a_y))

    # backward at the reference statistics rounded to fp32 (the kernel's inputs)
    mu, rs = mr.float().double(), rr.float().double()
    xh = (x - mu[:, None]) * rs[:, None]
    dy = q(torch.randn(M, D, generator=g, dtype=torch.float64) + (torch.rand(D, generator=g, dtype=torch.float64) - 0.3) + 0.5 * xh, dt)
    add = q(torch.randn(M, D, generator=g, dtype=torch.float64), dt)
    dyk, muk, rsk, gk = dev(dy, dt), dev(mu), dev(rs), dev(gamma)
    dx, dgam, dbet = ops.ln_train_backward(dyk, xk, muk, rsk, gk)
    dxr, dgr, dbr = ref.ln_backward(dy, x, gamma, eps)
    gg = dy * gamma
    c1, c2 = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
    xh_err = 2 * U * (x.abs() + mu.abs()[:, None]) * rs[:, None] + U * (mu.abs() * rs)[:, None] + U * xh.abs()      # fp32 xhat + the fp32 rounding of mean / rstd
    e_c1 = (sum_tol(gg.abs().sum(1), depth) / D)[:, None]
    e_c2 = ((sum_tol((gg * xh).abs().sum(1), depth) + (gg.abs() * xh_err).sum(1)) / D)[:, None]
    a_dx = rs[:, None] * (e_c1 + xh.abs() * e_c2 + c2.abs() * xh_err + 8 * U * (gg.abs() + c1.abs() + (xh * c2).abs()))
    check('dx', dx, dxr, stored_tol(dxr, dt, a_dx))
    nb = min(max((M + 63) // 64, 1), 1024)
    rpb = -(-M // nb)
    pdepth = -(-rpb // 4) + 4                      # rows of a block per wave in one register chain, then the four waves
    t_db = sum_tol(dy.abs().sum(0), pdepth) + U * dbr.abs()
    t_dg = sum_tol((dy * xh).abs().sum(0), pdepth) + (dy.abs() * xh_err).sum(0) + U * dgr.abs()
    print(f'    torch fp32 column-sum error dy {ref32_sum_err(dy):.2e}, dy*xhat {ref32_sum_err(dy * xh):.2e} (kernel bound {float(t_db.max()):.2e} / {float(t_dg.max()):.2e})')
    check('dbeta', dbet, dbr, t_db)
    check('dgamma', dgam, dgr, t_dg)
    # with add, out of place and in place (add == dx); null parameter gradients; determinism
    addk = dev(add, dt)
    dxa, dg2, db2 = ops.ln_train_backward(dyk, xk, muk, rsk, gk, add=addk)
    check('dx + add', dxa, dxr + add, stored_tol(dxr + add, dt, a_dx + U * add.abs()))
    assert torch.equal(dg2, dgam) and torch.equal(db2, dbet)
    dxi, none_g, none_b = ops.ln_train_backward(dyk, xk, muk, rsk, gk, add=addk, dx=addk, param_grads=False)
    assert none_g is None and none_b is None and torch.equal(dxi, dxa)


def test_vit_cls_ln_and_tokens():
    """vit_cls_ln_fwd / _bwd at S in {1, 2, 197} and vit_assemble / vit_patch_rows as exact copies (bit-equal to the rounding of the fp32 sum)."""
    ops, ref = _mods()
    eps = 1e-6
    for dt in DTS:
        for (B, S, D) in ((3, 1, 64), (5, 2, 260), (4, 197, 384), (2, 5, 2052), (800, 3, 4)):
            g = gen(5000 + S + D)
            x, gamma, beta = ln_inputs(B * S, D, dt, g)
            tok = x.reshape(B, S, D)
            tk = dev(tok, dt)
            feat, mean, rstd = ops.vit_cls_ln_forward(tk, dev(gamma), dev(beta), eps)
            x0 = tok[:, 0]
            yr, mr, rr = ref.ln_forward(x0, gamma, beta, eps)
            depth = -(-D // 64) + 6
            t_mean = sum_tol(x0.abs().sum(1), depth) / D + 2 * U * mr.abs()
            t_var = sum_tol((x0 * x0).sum(1), depth) / D + 2 * mr.abs() * t_mean + 4 * U * ((x0 * x0).mean(1) + mr * mr)
            t_rstd = 0.5 * rr ** 3 * t_var + 4 * U * rr
            print(f'\n  vit_cls_ln B={B} S={S} D={D} {dt}')
            check('mean', mean, mr, t_mean)
            check('rstd', rstd, rr, t_rstd)
            xh = (x0 - mr[:, None]) * rr[:, None]
            a_y = (rr[:, None] * t_mean[:, None] + (x0 - mr[:, None]).abs() * t_rstd[:, None]) * gamma.abs() + 8 * U * ((xh * gamma).abs() + beta.abs() + (x0.abs() + mr.abs()[:, None]) * rr[:, None] * gamma.abs())
            check('feat', feat, yr, stored_tol(yr, 'f32', a_y))
            mu, rs = mr.float().double(), rr.float().double()
            xh = (x0 - mu[:, None]) * rs[:, None]
            dfeat = (torch.randn(B, D, generator=g) + 0.3).double() + 0.5 * xh.float().double()
            dfeat = dfeat.float().double()
            dtok, dgam, dbet = ops.vit_cls_ln_backward(dev(dfeat), tk, dev(mu), dev(rs), dev(gamma))
            again = ops.vit_cls_ln_backward(dev(dfeat), tk, dev(mu), dev(rs), dev(gamma))
            assert torch.equal(again[0], dtok) and torch.equal(again[1], dgam) and torch.equal(again[2], dbet)
            dxr, dgr, dbr = ref.ln_backward(dfeat, x0, gamma, eps)
            gg = dfeat * gamma
            c1, c2 = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
            xh_err = 2 * U * (x0.abs() + mu.abs()[:, None]) * rs[:, None] + U * (mu.abs() * rs)[:, None] + U * xh.abs()
            e_c1 = (sum_tol(gg.abs().sum(1), depth) / D)[:, None]
            e_c2 = ((sum_tol((gg * xh).abs().sum(1), depth) + (gg.abs() * xh_err).sum(1)) / D)[:, None]
            a_dx = rs[:, None] * (e_c1 + xh.abs() * e_c2 + c2.abs() * xh_err + 8 * U * (gg.abs() + c1.abs() + (xh * c2).abs()))
            check('dtok[:, 0]', dtok[:, 0], dxr, stored_tol(dxr, dt, a_dx))
            assert S == 1 or float(dtok[:, 1:].float().abs().max()) == 0.0, 'every other row of dtok is zero'
            check('dbeta', dbet, dbr, U * dfeat.abs().sum(0) + U * dbr.abs())            # fp64 sum of fp32 terms, one rounding
            check('dgamma', dgam, dgr, (dfeat.abs() * (xh_err + 2 * U * xh.abs())).sum(0) + U * dgr.abs())
            if D % 4:
                continue
            # token assembly / patch rows: exact
            zpe = q(torch.randn(B * (S - 1), D, generator=g, dtype=torch.float64), dt)
            cls = torch.randn(D, generator=g).double()
            pos = torch.randn(S, D, generator=g).double()
            tokens = ops.vit_assemble(dev(zpe, dt) if S > 1 else torch.empty(0, D, dtype=TD[dt]).cuda(), dev(cls), dev(pos), B, S)
            want = torch.empty(B, S, D, dtype=torch.float32)
            want[:, 0] = (pos[0].float() + cls.float())
            if S > 1:
                want[:, 1:] = pos[1:].float() + zpe.float().reshape(B, S - 1, D)
            assert torch.equal(tokens.cpu(), want.to(TD[dt])), 'vit_assemble: the fp32 sum rounded to T, bit for bit'
            if S > 1:
                rows = ops.vit_patch_rows(tokens)
                assert torch.equal(rows.cpu(), tokens.cpu()[:, 1:].reshape(B * (S - 1), D)), 'vit_patch_rows: exact copy'


# ------------------------------------------------------------------------------------------------ elementwise and small reductions
@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('n', [4, 1020, 256 * 4 * 7, 1028 * 32643], ids=['n4', 'n1020', 'n7168', 'n_past_grid'])
def test_elementwise(n, dt):
    """gelu_fwd / gelu_bwd, add_scaled, bcast_add at n that is and is not a multiple of a block's 1024 elements and past the 32768-block grid clamp."""
    ops, ref = _mods()
    g = gen(6000 + n % 977)
    z = q(torch.randn(n, generator=g, dtype=torch.float64) * 2, dt)
    dh = q(torch.randn(n, generator=g, dtype=torch.float64), dt)
    zk, dhk = dev(z, dt), dev(dh, dt)
    print(f'\n  elementwise n={n} {dt}')
    # gelu backward: dh * (Phi(z) + z phi(z)) - erff / expf of the device library: 4 ulp each (documented bounds), O(1) factors
    want = ref.gelu_backward(dh, z)
    check('gelu_bwd', ops.gelu_train(zk, dhk), want, stored_tol(want, dt, 16 * U * dh.abs() * (1 + z.abs())))
    if dt == 'f32':
        wf = F.gelu(z)
        check('gelu_fwd', ops.gelu_train(zk), wf, stored_tol(wf, dt, 8 * U * z.abs()))
    else:
        # 16-bit storage runs the sigmoid-form GELU, max |gelu_sig - gelu_erf| = 2.6e-5 (fsvit_common.h), exp2 / rcp approximations 2^-22 relative
        wf = F.gelu(z)
        check('gelu_fwd', ops.gelu_train(zk), wf, stored_tol(wf, dt, 2.6e-5 + 2.0 ** -20 * z.abs()))
    per = {4: 4, 1020: 204, 7168: 1024}.get(n, 1028)       # 1028 * 32643 elements: past one sweep of the 32768-block grid, not a multiple of it
    nimg = n // per
    scale = (0.5 + torch.rand(nimg, generator=g)).double()
    want = z + scale.repeat_interleave(per) * dh
    check('add_scaled', ops.add_scaled(zk, dhk, dev(scale), per), want, stored_tol(want, dt, 2 * U * (z.abs() + (want - z).abs())))
    check('add_scaled (no a, no scale)', ops.add_scaled(None, dhk), dh, 0.0)
    p = torch.randn(per, generator=g).double()
    want = z + p.repeat(nimg)
    check('bcast_add', ops.bcast_add(zk.reshape(nimg, per), dev(p)).reshape(-1), want, stored_tol(want, dt, U * (z.abs() + p.repeat(nimg).abs())))


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('B', [1, 2, 800])
def test_batch_sum(B, dt):
    """batch_sum (16 waves over the batch, two images in flight, LDS reduce in wave order) at B in {1, 2, 800}, per_img not a multiple of 256."""
    ops, ref = _mods()
    per = 1300
    g = gen(7000 + B)
    x = q(torch.randn(B, per, generator=g, dtype=torch.float64) + 0.5, dt)
    xk = dev(x, dt)
    out = ops.batch_sum(xk)
    depth = -(-B // 16) + 16
    print(f'\n  batch_sum B={B} {dt}: torch fp32 sum error {ref32_sum_err(x):.2e}')
    check('batch_sum', out, x.sum(0), sum_tol(x.abs().sum(0), depth) + U * x.sum(0).abs())
    assert torch.equal(out, ops.batch_sum(xk))


@pytest.mark.parametrize('dt', DTS)
def test_small_ops(dt):
    """colsum, avgpool_bwd, unpatch2, droppath_scales, fold_prenorm."""
    ops, ref = _mods()
    g = gen(8000)
    print(f'\n  small ops {dt}')
    for (M, C) in ((1, 8), (65, 132), (40000, 64), (70, 4096)):
        a = q(torch.randn(M, C, generator=g, dtype=torch.float64) + torch.rand(C, generator=g, dtype=torch.float64), dt)
        ak = dev(a, dt)
        nblk, R, n = bn_layout(M, C, dt)
        out = ops.colsum(ak)
        check(f'colsum {M}x{C}', out, a.sum(0), sum_tol(a.abs().sum(0), n + R) + U * a.sum(0).abs())
        assert torch.equal(out, ops.colsum(ak))
    for (B, HW, C) in ((1, 1, 3), (7, 25, 130), (800, 25, 512)):
        df = torch.randn(B, C, generator=g).double()
        want = (df / HW)[:, None, :].expand(B, HW, C)
        check(f'avgpool_bwd {B}x{HW}x{C}', ops.avgpool_bwd(dev(df), HW, TD[dt]), want, stored_tol(want, dt, U * want.abs()))
    for (B, OH, OW, C) in ((1, 1, 1, 1), (3, 5, 7, 6), (9, 10, 10, 128)):
        gq = q(torch.randn(B * OH * OW, 4 * C, generator=g, dtype=torch.float64), dt)
        assert torch.equal(ops.unpatch2(dev(gq, dt), B, OH, OW).double().cpu(), ref.unpatch2(gq, B, OH, OW)), 'unpatch2: exact scatter'
    if dt == 'f32':
        for ncalls, nimg in ((1, 1), (70, 800)):               # 70 calls: two launches of the 64-entry keep table
            masks = (torch.rand(ncalls, nimg, generator=g) > 0.3).float()
            keep = [1.0 - 0.5 * i / max(ncalls - 1, 1) for i in range(ncalls)]
            want = masks.double() / torch.tensor(keep).float().double()[:, None]
            check(f'droppath_scales {ncalls}x{nimg}', ops.droppath_scales(masks.cuda(), keep), want, 3 * U * want.abs())
    if dt == 'f32':
        for n in (1, 1000, 32768 * 256 + 77):                     # past one sweep of the grid
            assert torch.equal(ops.fill_f32(n, -2.5, 'cuda'), torch.full((n,), -2.5, device='cuda')), 'fill_f32'
            x = torch.randn(n, generator=g)
            assert torch.equal(ops.scale_copy(x.cuda(), 0.3).cpu(), x * torch.tensor(0.3)), 'scale_copy: one fp32 product'
    for (N, C, Kw) in ((1, 4, 4), (5, 130, 192), (384, 192, 192)):
        W = torch.randn(N, C, generator=g).double()
        sa, sb = (0.5 + torch.rand(C, generator=g)).double() * torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0), torch.randn(C, generator=g).double()
        wf, bf = ops.fold_prenorm(dev(W), dev(sa), dev(sb), Kw, TD[dt])
        want = torch.zeros(N, Kw, dtype=torch.float64)
        want[:, :C] = W * sa
        check(f'fold_prenorm wf {N}x{C}', wf, want, stored_tol(want, dt, U * want.abs()))
        check(f'fold_prenorm bf {N}x{C}', bf, (W * sb).sum(1), sum_tol((W * sb).abs().sum(1), -(-C // 64) + 6) + U * (W * sb).sum(1).abs())


# ------------------------------------------------------------------------------------------------ what the entries refuse (nothing is launched)
def test_rejections():
    ops, ref = _mods()
    f = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt).cuda()
    ones = lambda n: torch.ones(n).cuda()
    # train-mode BatchNorm over one value per channel (torch refuses it too; the finalize divides by M - 1)
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        ops.bn_train_forward(f(1, 8), ones(8), ones(8))
    # channels: not a multiple of 4; a partial pass of channel lanes (fp32: 2052 / 4 = 513 lanes)
    with pytest.raises(ValueError, match='multiple of 4'):
        ops.bn_train_forward(f(4, 6), ones(6), ones(6))
    with pytest.raises(ValueError, match='whole passes'):
        ops.bn_train_forward(f(4, 2052), ones(2052), ones(2052))
    with pytest.raises(ValueError, match='whole passes'):
        ops.colsum(f(4, 2056, dt=torch.bfloat16))
    # M is images * rows_per_img: a ragged last image is refused, forward and backward
    with pytest.raises(ValueError, match='images \\* rows_per_img'):
        ops.bn_train_forward(f(10, 8), ones(8), ones(8), add_a=f(10, 8), add_b=f(10, 8), add_scale=ones(3), rows_per_img=4)
    with pytest.raises(ValueError, match='images \\* rows_per_img'):
        ops.bn_train_backward(f(10, 8), f(10, 8), ones(8), ones(8), ones(8), scale2=ones(3), out2=f(10, 8), rows_per_img=4)
    # no f16 build of the training kernels
    h = torch.float16
    with pytest.raises(ValueError, match='FSVIT_F32 and FSVIT_BF16'):
        ops.bn_train_forward(f(4, 8, dt=h), ones(8), ones(8))
    with pytest.raises(ValueError, match='FSVIT_F32 and FSVIT_BF16'):
        ops.ln_train_forward(f(4, 8, dt=h), ones(8), ones(8))
    with pytest.raises(ValueError, match='FSVIT_F32 and FSVIT_BF16'):
        ops.gelu_train(f(8, dt=h))
    with pytest.raises(ValueError, match='FSVIT_F32 and FSVIT_BF16'):
        ops.stem_tail_train_forward(f(1, 2, 2, 8, dt=h), ones(8), ones(8))
    # LayerNorm: D beyond the LDS form, D not a multiple of 4
    for D in (2052, 6, 4098):
        with pytest.raises(ValueError, match='multiple of 4, at most 2048'):
            ops.ln_train_forward(f(2, D), ones(D), ones(D))
        with pytest.raises(ValueError, match='multiple of 4, at most 2048'):
            ops.ln_train_backward(f(2, D), f(2, D), ones(2), ones(2), ones(D))
    # stem tail: C % 8; the fused backward where the channel lanes do not divide 256
    with pytest.raises(ValueError, match='multiple of 8'):
        ops.stem_tail_train_forward(f(1, 2, 2, 12), ones(12), ones(12))
    with pytest.raises(ValueError, match='row-walking'):
        ops.stem_tail_train_backward(f(2, 7, 9, 96), torch.zeros(2, 7, 9, 96, dtype=torch.uint8).cuda(), f(2, 14, 18, 96), f(2, 14, 18, 96), ones(96), ones(96), ones(96),
                                     ones(96), ones(96), ones(96))
    # 4-element accesses
    with pytest.raises(ValueError, match='multiple of 4'):
        ops.gelu_train(f(6))
    with pytest.raises(ValueError, match='multiple of 4'):
        ops.batch_sum(f(3, 6))
    with pytest.raises(ValueError, match='multiple of 4'):
        ops.vit_assemble(f(2, 6), ones(6), f(2, 6), 2, 2)
    torch.cuda.synchronize()
