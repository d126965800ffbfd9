"""Operator tests of the MFMA side of the training step through the fsvit_op_* entries, against float64 torch on the CPU (oracle/train_ops_oracle.py):

  launch_stage1_ring_block_train (stage1_ring.hip MODE 3), launch_stage1_ring_dgrad (MODE 2)       test_ring_forward, test_ring_dgrad
  launch_conv_gemm with y2 (gelu_sig_d / gelu_erf_d) and ACT_MUL: gemm256, conv_gemm_v2             test_conv_epilogues
  launch_gconv3x3 with y2 / mul                                                                     test_gconv3x3_train
  launch_pack_weight_multi modes 0 / 1 / 2, head padding, the two-limb words, the job table          test_pack_weight, test_pack_weight_table
  what the entries refuse                                                                           test_rejections_conv

Conventions and helpers are those of test_gpu_train_ops.py (check / stored_tol / half_ulp / sum_tol / q / dev; u = 2^-24; no bound is computed from the
kernel's output).

CHECKING BY STAGES.  A hidden map the kernel rounds to bf16 can land one ulp beside the reference's rounding, and that flip pollutes everything
downstream.  Every stored map is therefore held to float64 of ITS operation applied to the maps the kernel stored one stage earlier, read back: xn, h1 /
g1 from x; h2 / g2 from the stored h1; out from the stored h2 and x; dz2 from dz3 and g2; dz1 from the stored dz2 and g1; dxn from the stored dz1.
Nothing is lost: if the LDS copy a later stage consumed differs from the HBM copy (a halo pixel recomputed by the neighbouring workgroup included), the
later stage fails.

BOUNDS.
 * a dot product of K products: a_z = sum_tol(sum_k |x_k w_k|, depth = K) - the order inside and across the MFMAs is not documented, so the chain is
   taken as long as it can be.  Products of two bf16 values are exact in fp32; fp32 storage (the fp32 MFMA) adds u * sum |x_k w_k|; a bias u * |b|.
 * GELU value a_h = L0 a_z + 2^-20 |z|, derivative a_g = L1 a_z + 2^-20 (1 + |z|): L0 / L1 = 1.01 x the largest slope of the reference GELU / of its
   derivative on a float64 grid over [-9, 9] (step 1e-3; properties of the reference, printed); 2^-20 = 16 u is the allowance test_elementwise gives
   the hardware exp2 / rcp behind gelu_sig and the erff / expf behind the fp32-storage form (reference there: F.gelu and its autograd).
 * ACT_MUL and the ring dgrad stages: a = |mul| a_z + u |acc mul|;  xn: 2 u (|sa x| + |sb|) (an fma, or a mul and an add);
   out: |scale| a_z + 2 u (|scale acc| + |x|).
 * every stored value: |err| <= stored_tol(ref, dt, a) = half ulp of the storage type at the reference + a.
Exact: packs are bit-equal to the oracle's pack rounded to the type (two-limb words: ops.x2_limbs), pad rows / columns / head slots exactly zero;
images with scale[b] == 0 leave `out` bit-equal to x; every ring op called twice is bit-identical.

No number in this file was read off a kernel run: the GELU coefficients come from fsvit_common.h (restated in the oracle), 2^-20 and the sum bound from
test_gpu_train_ops.py (test_elementwise, sum_tol), L0 / L1 from the oracle grid, the grid restatement from s1r_grid (stage1_ring.hip).
"""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_train_ops import TD, U, check, dev, gen, half_ulp, q, stored_tol, sum_tol

pytestmark = pytest.mark.gpu

E20 = 2.0 ** -20
BKE = {'f32': 32, 'bf16': 64}


def _mods():
    from fewshot_vit_amd.engine import ops
    from oracle import train_ops_oracle as ref
    return ops, ref


_L = {}


def lipschitz(kind):
    """(L0, L1) = 1.01 x (max |f'|, max |f''|) of the reference GELU on a float64 grid over [-9, 9], step 1e-3; kind 'sig': gelu_sig / gelu_sig_d of the
    oracle, 'erf': F.gelu and its autograd"""
    if kind not in _L:
        _, ref = _mods()
        z = torch.arange(-9.0, 9.0 + 5e-4, 1e-3, dtype=torch.float64).requires_grad_(True)
        d = ref.gelu_sig_d(z) if kind == 'sig' else torch.autograd.grad(F.gelu(z).sum(), z, create_graph=True)[0]
        dd = torch.autograd.grad(d.sum(), z)[0]
        _L[kind] = (1.01 * float(d.detach().abs().max()), 1.01 * float(dd.abs().max()))
        print(f'\n  GELU ({kind}) on the grid: L0 = {_L[kind][0]:.4f}, L1 = {_L[kind][1]:.4f}')
    return _L[kind]


def gelu_ref(z, kind):
    """(value, derivative) of the reference GELU in float64"""
    _, ref = _mods()
    if kind == 'sig':
        return ref.gelu_sig(z), ref.gelu_sig_d(z)
    return F.gelu(z), ref.gelu_backward(torch.ones_like(z), z)


def gelu_bounds(z, a_z, kind):
    L0, L1 = lipschitz(kind)
    return L0 * a_z + E20 * z.abs(), L1 * a_z + E20 * (1 + z.abs())


def held(name, got, ref, dt, a):
    """check(got, ref, stored_tol(ref, dt, a)) - and, printed only: in 16-bit storage the rounding of the stored value itself takes the half ulp, so
    err / bound approaches 1 on any correct kernel; what tells how the ARITHMETIC sits in its allowance a is the worst (err - half ulp) / a."""
    check(name, got, ref, stored_tol(ref, dt, a))
    if dt != 'f32':
        a_t = a if torch.is_tensor(a) else torch.full_like(ref, float(a))
        over = ((got.detach().double().cpu() - ref).abs() - half_ulp(ref, dt, a_t)) / a_t.expand_as(ref).clamp_min(1e-300)
        print(f'      beyond the half ulp of {dt}: worst (err - half ulp) / a = {max(float(over.max()), 0.0):.3f}')


def rnd_of(dt):
    return lambda t: q(t, dt)


# ------------------------------------------------------------------------------------------------ weight packs
def rounded_pack(ops, packed64, dt):
    """the oracle's float64 pack -> what the kernel must have stored, in the tensor type ops.pack_weight returns"""
    if dt == 'x2':
        return ops.x2_limbs(packed64.float(), 'bf16x2')
    return packed64.to(TD[dt])


def same_bits(a, b):
    a, b = a.cpu(), b.cpu()
    if a.dtype == torch.float32:
        return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    return a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


# name: (weight shape, groups, [(mode, head fields, extra rows, Kw or None)]); hd: (hd_rows, hdp_rows, hd_cols, hdp_cols) of the PACKED rows / columns -
# the transposed pack of a layer swaps them, as the trainer does
NOHD = (1, 1, 1, 1)
PACK_CASES = {
    'conv1x1_256x128': ((256, 128, 1, 1), 1, [(0, NOHD, 0, None), (1, NOHD, 0, None)]),
    'gconv3x3_256x32_g8': ((256, 32, 3, 3), 8, [(0, NOHD, 0, 320), (1, NOHD, 0, 320)]),
    'conv3x3_128x64': ((128, 64, 3, 3), 1, [(0, NOHD, 0, None), (1, NOHD, 0, None)]),
    'patch2x2_256x128': ((256, 128, 2, 2), 1, [(0, NOHD, 0, None), (2, NOHD, 0, None)]),
    'qkv_rows_42to48': ((3 * 6 * 42, 128, 1, 1), 1, [(0, (42, 48, 1, 1), 0, None), (1, (1, 1, 42, 48), 0, None)]),
    'proj_cols_252to288': ((256, 252, 1, 1), 1, [(0, (1, 1, 42, 48), 0, None), (1, (42, 48, 1, 1), 0, None)]),
    'stem_27_columns': ((64, 3, 3, 3), 1, [(0, NOHD, 5, None)]),
}
PACK_X2 = ('conv1x1_256x128', 'qkv_rows_42to48', 'proj_cols_252to288')
PACK_PARAMS = [(n, dt) for n in PACK_CASES for dt in ('f32', 'bf16', 'x2') if dt != 'x2' or n in PACK_X2]


def pack_dtype(dt):
    return 'bf16x2' if dt == 'x2' else TD[dt]


def check_pad_is_zero(got, shape, groups, mode, hd):
    """rows past the padded rows, columns past the padded columns and the head slots hd .. hdp - 1: exactly zero"""
    O, Ig, KH, KW = shape
    Ng = O // groups
    g = got.cpu()
    g = g.view(torch.int32) if g.dtype == torch.float32 else g.view(torch.int16)
    if mode == 2:
        rows, cols = KH * KW * Ig, Ng
    else:
        rows, cols = (Ng if mode == 0 else Ig) // hd[0] * hd[1], KH * KW * (Ig if mode == 0 else Ng) // hd[2] * hd[3]
    assert int(g[:, rows:].abs().max() if g.shape[1] > rows else 0) == 0 and int(g[:, :, cols:].abs().max() if g.shape[2] > cols else 0) == 0
    if hd[0] != hd[1]:
        assert int(g[:, :rows].reshape(groups, rows // hd[1], hd[1], -1)[:, :, hd[0]:].abs().max()) == 0
    if hd[2] != hd[3]:
        assert int(g[:, :, :cols].reshape(groups, g.shape[1], cols // hd[3], hd[3])[..., hd[2]:].abs().max()) == 0


@pytest.mark.parametrize('name,dt', PACK_PARAMS, ids=[f'{n}-{dt}' for n, dt in PACK_PARAMS])
def test_pack_weight(name, dt):
    """fsvit_op_pack_weight, one job: bit-equal to the oracle's pack (its own index arithmetic) rounded to the type."""
    ops, ref = _mods()
    shape, groups, variants = PACK_CASES[name]
    w = torch.randn(*shape, generator=gen(9000 + sum(shape)))
    bke = 32 if dt != 'bf16' else 64
    for mode, hd, extra_rows, Kw in variants:
        rows, kw = ops.pack_geometry(shape, groups, mode, bke, *hd)
        kw = Kw or kw
        got = ops.pack_weight(w.cuda(), groups, mode, rows + extra_rows, kw, *hd, dtype=pack_dtype(dt))
        want = ref.pack_weight(w.double(), groups, mode, rows + extra_rows, kw, *hd)
        assert got.shape == want.shape
        assert same_bits(got, rounded_pack(ops, want, dt)), (name, dt, mode)
        check_pad_is_zero(got, shape, groups, mode, hd)
        if name == 'stem_27_columns':
            assert kw == bke and got.shape == (1, 69, bke), 'the 27 columns are padded to ONE K slice'


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_pack_weight_table(dt):
    """fsvit_op_pack_weight_multi with 41 jobs: one more than the launcher's table holds, so the last job rides in a second launch.  Jobs of every mode,
    of unequal sizes (the grid is sized by the biggest of a launch; the small ones leave blocks idle)."""
    ops, ref = _mods()
    g = gen(9100)
    shapes = [((16, 8, 1, 1), 1), ((24, 4, 3, 3), 2), ((8, 12, 2, 2), 1), ((96, 64, 3, 3), 1), ((3 * 2 * 42, 16, 1, 1), 1)]
    jobs, specs = [], []
    for i in range(41):
        shape, groups = shapes[i % len(shapes)] if i != 40 else ((40, 24, 1, 1), 1)
        mode = (0, 1, 2)[i % 3] if shape[2] == 2 else (0, 1)[i % 2]
        hd = NOHD
        if shape[0] == 3 * 2 * 42:
            hd = (42, 48, 1, 1) if mode == 0 else (1, 1, 42, 48)
        w = torch.randn(*shape, generator=g)
        jobs.append(dict(w=w.cuda(), groups=groups, mode=mode, hd_rows=hd[0], hdp_rows=hd[1], hd_cols=hd[2], hdp_cols=hd[3]))
        specs.append((w, shape, groups, mode, hd))
    outs = ops.pack_weight_multi(jobs, TD[dt])
    assert len(outs) == 41
    for i, (got, (w, shape, groups, mode, hd)) in enumerate(zip(outs, specs)):
        rows, kw = ops.pack_geometry(shape, groups, mode, BKE[dt], *hd)
        want = ref.pack_weight(w.double(), groups, mode, rows, kw, *hd)
        assert same_bits(got, rounded_pack(ops, want, dt)), ('job', i, shape, mode)
        check_pad_is_zero(got, shape, groups, mode, hd)


# ------------------------------------------------------------------------------------------------ stage-1 ring kernels
def s1r_grid(M):
    """stage1_ring.hip s1r_grid restated: (64-pixel chunks, workgroups, chunks per workgroup)"""
    n = -(-M // 64)
    w = min(n, 256)
    cpw = -(-n // w)
    return n, -(-n // cpw), cpw


# (B, H, W): see the issue of each in the test docstrings; expected chunks per workgroup where the case is there for the ring walk
RING_CASES = [(1, 4, 4), (2, 5, 7), (7, 10, 10), (3, 20, 20), (42, 20, 20), (83, 20, 20), (1025, 4, 4)]
RING_CPW = {(42, 20, 20): 2, (83, 20, 20): 3, (1025, 4, 4): 2}
RING_IDS = ['x'.join(map(str, c)) for c in RING_CASES]
DEVICE_BUILT = (2, 5, 7)                   # the case whose weight operands are all made on the device (fold_prenorm, pack_weight), as the trainer does


def ring_weights(g):
    w1 = torch.randn(256, 128, generator=g) * 0.09                       # pre-activations of O(1): both GELU branches and the clamp-free range
    w2 = torch.randn(256, 32, 3, 3, generator=g) * 0.08
    w3 = torch.randn(128, 256, generator=g) * 0.07
    return w1, w2, w3


def scale_vectors(B):
    """per-image DropPath scales holding 0, 1 and 1 / keep values; for B < 3 several vectors so that every kind is met"""
    pat = [0.0, 1.0, 1 / 0.9, 1 / 0.75, 0.0, 1 / 0.6]
    return [torch.tensor([pat[(b + r) % len(pat)] for b in range(B)], dtype=torch.float32) for r in range(-(-3 // min(B, 3)))]


@pytest.mark.parametrize('case', RING_CASES, ids=RING_IDS)
def test_ring_forward(case):
    """launch_stage1_ring_block_train, bf16, every stored map by stages (module docstring).
    (1,4,4): M = 16, a quarter of a chunk - the first window reads pixels below 0 and past M.  (2,5,7): non-square, W does not divide the 16-pixel
    tile, a chunk straddles the two images and is ragged.  (3,20,20): W = 20, the halo limit; 18 chunks + a 48-pixel tail.  (42,20,20): 263 chunks on 132
    workgroups, two per workgroup - seams, own-pixel stores, a last workgroup with one chunk.  (83,20,20): three per workgroup, the third pass reuses
    ring slots.  (1025,4,4): two per workgroup, four images per chunk, every pixel on a border.
    Runs with scale NULL and with per-image scales (0, 1, 1 / keep); sa has mixed signs."""
    ops, ref = _mods()
    B, H, W = case
    M = B * H * W
    n_chunks, wgs, cpw = s1r_grid(M)
    if case in RING_CPW:
        assert cpw == RING_CPW[case], (case, n_chunks, wgs, cpw)
    if case == (42, 20, 20):
        assert (n_chunks, wgs) == (263, 132) and n_chunks - (wgs - 1) * cpw == 1
    dt = 'bf16'
    rnd = rnd_of(dt)
    g = gen(10000 + M)
    x = q(torch.randn(B, H, W, 128, generator=g, dtype=torch.float64) * 1.5 + 0.3, dt)
    w1, w2, w3 = ring_weights(g)
    sa = ((0.5 + torch.rand(128, generator=g)) * torch.where(torch.arange(128) % 3 == 1, -1.0, 1.0)).float()
    sb = (torch.rand(128, generator=g) - 0.5).float()
    if case == DEVICE_BUILT:
        w1f_k, b1f_k = ops.fold_prenorm(w1.cuda(), sa.cuda(), sb.cuda(), 128, TD[dt])          # (held to float64 by test_small_ops)
        w2_k = ops.pack_weight(w2.cuda(), 8, 0, Kw=320, dtype=TD[dt]).reshape(256, 320)
        w3_k = ops.pack_weight(w3.reshape(128, 256, 1, 1).cuda(), 1, 0, dtype=TD[dt]).reshape(128, 256)
        w1f, b1f = w1f_k.double().cpu(), b1f_k.double().cpu()
    else:
        w1f, b1f = q(w1.double() * sa.double(), dt), (w1.double() @ sb.double()).float().double()
        w1f_k, b1f_k = dev(w1f, dt), dev(b1f)
        w2_k = dev(ref.pack_weight(w2.double(), 8, 0, Kw=320).reshape(256, 320), dt)
        w3_k = dev(w3.double(), dt)
    w2q, w3q = q(w2.double(), dt), q(w3.double(), dt)
    xk, sak, sbk = dev(x, dt), sa.cuda(), sb.cuda()
    run = lambda scale: ops.stage1_block_train(xk, w1f_k, b1f_k, w2_k, w3_k, sak, sbk, None if scale is None else scale.cuda())
    k = run(None)
    f64 = lambda t: t.double().cpu()
    r = ref.stage1_block_forward(x, w1f, b1f, w2q, w3q, sa.double(), sb.double(), None, rnd, h1_stored=f64(k['h1']), h2_stored=f64(k['h2']))
    print(f'\n  ring forward {case}: M = {M}, {n_chunks} chunks on {wgs} workgroups, {cpw} per workgroup')
    xs = x * sa.double()
    # (the oracle's maps are ROUNDED where the kernel rounds - they feed the next stage; every comparison here is with the unrounded float64 value)
    want = xs + sb.double()
    held('xn', k['xn'], want, dt, 2 * U * (xs.abs() + sb.double().abs()))
    a1 = sum_tol(r['abs1'], 128) + U * b1f.abs()
    ah, ag = gelu_bounds(r['z1'], a1, 'sig')
    hv, dv = gelu_ref(r['z1'], 'sig')
    held('h1', k['h1'], hv, dt, ah)
    held('g1', k['g1'], dv, dt, ag)
    a2 = sum_tol(r['abs2'], 288)
    ah, ag = gelu_bounds(r['z2'], a2, 'sig')
    hv, dv = gelu_ref(r['z2'], 'sig')
    held('h2 (from the stored h1)', k['h2'], hv, dt, ah)
    held('g2 (from the stored h1)', k['g2'], dv, dt, ag)
    a3 = sum_tol(r['abs3'], 256)
    want = x + r['acc3']
    held('out (from the stored h2), scale NULL', k['out'], want, dt, a3 + 2 * U * (r['acc3'].abs() + x.abs()))
    again = run(None)
    assert all(torch.equal(k[n], again[n]) for n in k), 'bit-reproducible'
    for scale in scale_vectors(B):
        ks = run(scale)
        assert all(torch.equal(ks[n], k[n]) for n in k if n != 'out'), 'the hidden maps do not depend on the DropPath scales'
        s = scale.double()[:, None, None, None]
        want = x + s * r['acc3']
        held(f'out, scales {[round(float(v), 3) for v in scale[:6]]}', ks['out'], want, dt, s.abs() * a3 + 2 * U * ((s * r['acc3']).abs() + x.abs()))
        dropped = scale == 0
        assert bool(dropped.any()) or B < 3
        assert torch.equal(ks['out'].cpu()[dropped], xk.cpu()[dropped]), 'scale[b] == 0: the image passes through bit for bit'


@pytest.mark.parametrize('case', RING_CASES, ids=RING_IDS)
def test_ring_dgrad(case):
    """launch_stage1_ring_dgrad, bf16, by stages: dz2 from dz3 and g2, dz1 from the stored dz2 and g1, dxn from the stored dz1 (cases: test_ring_forward).
    The multipliers are independent maps over the range of a GELU derivative, negative values and exact zeros included."""
    ops, ref = _mods()
    B, H, W = case
    M = B * H * W
    n_chunks, wgs, cpw = s1r_grid(M)
    if case in RING_CPW:
        assert cpw == RING_CPW[case], (case, n_chunks, wgs, cpw)
    dt = 'bf16'
    rnd = rnd_of(dt)
    g = gen(11000 + M)
    dz3 = q(torch.randn(B, H, W, 128, generator=g, dtype=torch.float64), dt)
    w1, w2, w3 = ring_weights(g)
    mk = lambda: q((torch.rand(B, H, W, 256, generator=g, dtype=torch.float64) * 1.4 - 0.2) * (torch.rand(B, H, W, 256, generator=g) > 0.05), dt)
    g2, g1 = mk(), mk()
    if case == DEVICE_BUILT:
        w3t = ops.pack_weight(w3.reshape(128, 256, 1, 1).cuda(), 1, 1, dtype=TD[dt]).reshape(256, 128)
        w2t = ops.pack_weight(w2.cuda(), 8, 1, Kw=320, dtype=TD[dt]).reshape(256, 320)
        w1t = ops.pack_weight(w1.reshape(256, 128, 1, 1).cuda(), 1, 1, dtype=TD[dt]).reshape(128, 256)
    else:
        w3t = dev(ref.pack_weight(w3.double().reshape(128, 256, 1, 1), 1, 1).reshape(256, 128), dt)
        w2t = dev(ref.pack_weight(w2.double(), 8, 1, Kw=320).reshape(256, 320), dt)
        w1t = dev(ref.pack_weight(w1.double().reshape(256, 128, 1, 1), 1, 1).reshape(128, 256), dt)
    w1q, w2q, w3q = q(w1.double(), dt), q(w2.double(), dt), q(w3.double(), dt)
    args = (dev(dz3, dt), w3t, w2t, w1t, dev(g2, dt), dev(g1, dt))
    dxn, dz2, dz1 = ops.stage1_block_dgrad(*args)
    f64 = lambda t: t.double().cpu()
    r = ref.stage1_block_dgrad(dz3, w3q, w2q, w1q, g2, g1, rnd, dz2_stored=f64(dz2), dz1_stored=f64(dz1))
    print(f'\n  ring dgrad {case}: M = {M}, {n_chunks} chunks on {wgs} workgroups, {cpw} per workgroup')
    a = g2.abs() * sum_tol(r['abs2'], 128) + U * (r['acc2'] * g2).abs()
    want = r['acc2'] * g2
    held('dz2', dz2, want, dt, a)
    a = g1.abs() * sum_tol(r['abs1'], 288) + U * (r['acc1'] * g1).abs()
    want = r['acc1'] * g1
    held('dz1 (from the stored dz2)', dz1, want, dt, a)
    held('dxn (from the stored dz1)', dxn, r['acc0'], dt, sum_tol(r['abs0'], 256))
    again = ops.stage1_block_dgrad(*args)
    assert torch.equal(again[0], dxn) and torch.equal(again[1], dz2) and torch.equal(again[2], dz1), 'bit-reproducible'


# ------------------------------------------------------------------------------------------------ training epilogues of the conv launchers
GEMM256, V2 = 1, 2
BOTH = ('f32', 'bf16')
# (B, H, W, Cin per group, N per group, k, groups), storage types, the route launch_conv_gemm must take for the forward (y2) and the data-gradient (ACT_MUL) form
CONV_CASES = [
    ((13, 10, 10, 256, 1024, 1, 1), ('bf16',), GEMM256, GEMM256),       # M = 1300: five 256-row tiles + 20 rows
    ((13, 10, 10, 256, 1152, 1, 1), ('bf16',), GEMM256, GEMM256),       # N = 1152: four 256-column tiles + 128
    ((11, 10, 10, 256, 1024, 1, 1), ('bf16',), GEMM256, GEMM256),       # M = 1100, just past the M >= 1024 threshold: 76 rows in the last tile
    ((2, 20, 20, 128, 256, 1, 1), BOTH, V2, V2),     # N = 256 but M = 800 < 1024: conv_gemm_v2's 128 x 128 tile
    ((1, 5, 5, 288, 96, 1, 1), BOTH, V2, V2),                           # M = 25, Cin no power of two, K = 288 / 96 not whole K slices in bf16
    ((5, 7, 9, 32, 32, 3, 8), BOTH, V2, V2),                            # grouped 3 x 3, ragged map: the 128 x 32 tile, taps across image borders
    ((2, 6, 10, 96, 96, 3, 1), BOTH, V2, V2),                           # LV-ViT's 96 -> 96 3 x 3 (Cin a multiple of 32, no power of two)
]
CONV_PARAMS = [(c, dt, form) for c, dts, _, _ in CONV_CASES for dt in dts for form in ('y2', 'mul')]
CONV_ROUTE = {(c, form): (rf if form == 'y2' else rm) for c, _, rf, rm in CONV_CASES for form in ('y2', 'mul')}


def conv_operands(case, dt, seed):
    B, H, W, Ci, N, k, groups = case
    g = gen(seed)
    w = torch.randn(groups * N, Ci, k, k, generator=g) / (k * k * Ci) ** 0.5 * 1.5
    wq = w.double() if dt == 'f32' else q(w.double(), dt)
    return g, w, wq


@pytest.mark.parametrize('case,dt,form', CONV_PARAMS, ids=['x'.join(map(str, c)) + f'-{dt}-{form}' for c, dt, form in CONV_PARAMS])
def test_conv_epilogues(case, dt, form):
    """launch_conv_gemm: y2 - y = GELU(conv + bias) and the GELU's derivative (gelu_sig_d in bf16, gelu_erf_d in fp32 storage) against float64 F.conv2d;
    mul - (conv^T dz) * mul on the device-built transposed pack (ops.pack_weight mode 1) against autograd of F.conv2d times the multiplier.  The
    route the dispatcher took is asserted."""
    ops, ref = _mods()
    B, H, W, Ci, N, k, groups = case
    pad = k // 2
    g, w, wq = conv_operands(case, dt, 12000 + B * H * W + N)
    kind = 'sig' if dt == 'bf16' else 'erf'
    extra = U if dt == 'f32' else 0.0                       # the fp32 MFMA rounds its products
    nchw = lambda t: t.permute(0, 3, 1, 2)
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    print(f'\n  conv epilogue {case} {dt} {form}')
    if form == 'y2':
        x = q(torch.randn(B, H, W, groups * Ci, generator=g, dtype=torch.float64) * 1.5, dt)
        bias = (torch.randn(groups * N, generator=g) * 0.5).float()
        rows, kw = ops.pack_geometry(w.shape, groups, 0, BKE[dt])
        wk = dev(ref.pack_weight(w.double(), groups, 0, rows, kw), dt)
        y, y2, route = ops.conv_train(dev(x, dt), wk, bias.cuda(), k, k, 1, pad, N, groups, ops.ACT_GELU, with_y2=True)
        assert route == CONV_ROUTE[(case, form)], route
        z = nhwc(F.conv2d(nchw(x), wq, bias.double(), 1, pad, groups=groups))
        s_abs = nhwc(F.conv2d(nchw(x.abs()), wq.abs(), None, 1, pad, groups=groups))
        a_z = sum_tol(s_abs, k * k * Ci) + extra * s_abs + U * bias.double().abs()
        hv, dv = gelu_ref(z, kind)
        ah, ag = gelu_bounds(z, a_z, kind)
        held('y = GELU(z)', y, hv, dt, ah)
        held('y2 = GELU\'(z)', y2, dv, dt, ag)
    else:
        dz = q(torch.randn(B, H, W, groups * N, generator=g, dtype=torch.float64), dt)
        mul = q((torch.rand(B, H, W, groups * Ci, generator=g, dtype=torch.float64) * 1.4 - 0.2) * (torch.rand(B, H, W, groups * Ci, generator=g) > 0.05), dt)
        wk = ops.pack_weight(w.cuda(), groups, 1, dtype=TD[dt])
        assert wk.shape == (groups,) + ops.pack_geometry(w.shape, groups, 1, BKE[dt])
        y, _, route = ops.conv_train(dev(dz, dt), wk, None, k, k, 1, pad, Ci, groups, ops.ACT_MUL, mul=dev(mul, dt))
        assert route == CONV_ROUTE[(case, form)], route
        xr = torch.zeros(B, groups * Ci, H, W, dtype=torch.float64, requires_grad=True)
        acc = nhwc(torch.autograd.grad(F.conv2d(xr, wq, None, 1, pad, groups=groups), xr, nchw(dz))[0])
        s_abs = nhwc(F.conv_transpose2d(nchw(dz.abs()), wq.abs(), None, 1, pad, groups=groups))
        a_z = sum_tol(s_abs, k * k * N) + extra * s_abs
        want = acc * mul
        held('y = conv^T(dz) * mul', y, want, dt, mul.abs() * a_z + U * want.abs())


@pytest.mark.parametrize('form', ['y2', 'mul', 'both'])
@pytest.mark.parametrize('case', [(3, 20, 20), (2, 5, 7), (7, 20, 20)], ids=['3x20x20', '2x5x7', '7x20x20'])
def test_gconv3x3_train(case, form):
    """launch_gconv3x3 (wave = group, weights in registers) with its training epilogues, bf16: y2 - GELU + derivative (gelu_sig_d); mul - the data
    gradient on the tap-flipped pack times the multiplier.  (7,20,20): 44 chunks; (2,5,7): ragged, one chunk over two images.  The kernel's epilogue has
    no form with BOTH (it would store the GELU form and drop the multiplier without a word): entry and launcher refuse that, nothing is launched."""
    ops, ref = _mods()
    B, H, W = case
    dt = 'bf16'
    g = gen(13000 + B * H * W)
    w = torch.randn(256, 32, 3, 3, generator=g) * 0.09
    wq = q(w.double(), dt)
    x = q(torch.randn(B, H, W, 256, generator=g, dtype=torch.float64), dt)
    mul = q((torch.rand(B, H, W, 256, generator=g, dtype=torch.float64) * 1.4 - 0.2) * (torch.rand(B, H, W, 256, generator=g) > 0.05), dt)
    print(f'\n  gconv3x3_train {case} {form}')
    if form == 'both':
        wk = dev(ref.pack_weight(w.double(), 8, 0, Kw=320).reshape(256, 320), dt)
        with pytest.raises(ValueError, match='y2 and mul together'):
            ops.gconv3x3_train(dev(x, dt), wk, with_y2=True, mul=dev(mul, dt))
        torch.cuda.synchronize()
        return
    if form == 'y2':
        wk = dev(ref.pack_weight(w.double(), 8, 0, Kw=320).reshape(256, 320), dt)
        y, y2 = ops.gconv3x3_train(dev(x, dt), wk, with_y2=True)
        z = ref.gconv(x, wq, 8)
        a_z = sum_tol(ref.gconv(x.abs(), wq.abs(), 8), 288)
        hv, dv = gelu_ref(z, 'sig')
        ah, ag = gelu_bounds(z, a_z, 'sig')
        held('y = GELU(z)', y, hv, dt, ah)
        held('y2 = GELU\'(z)', y2, dv, dt, ag)
    else:
        wk = ops.pack_weight(w.cuda(), 8, 1, Kw=320, dtype=TD[dt]).reshape(256, 320)
        y, _ = ops.gconv3x3_train(dev(x, dt), wk, mul=dev(mul, dt))
        xr = torch.zeros(B, 256, H, W, dtype=torch.float64, requires_grad=True)
        acc = torch.autograd.grad(F.conv2d(xr, wq, None, 1, 1, groups=8), xr, x.permute(0, 3, 1, 2))[0].permute(0, 2, 3, 1)
        a_z = sum_tol(ref.gconv(x.abs(), wq.abs(), 8, transposed=True), 288)
        want = acc * mul
        held('y = conv^T(x) * mul', y, want, dt, mul.abs() * a_z + U * want.abs())


# ------------------------------------------------------------------------------------------------ what the entries refuse (nothing is launched)
def test_rejections_conv():
    ops, ref = _mods()
    z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt).cuda()
    ones = lambda n: torch.ones(n).cuda()
    w1, w2, w3 = z(256, 128), z(256, 320), z(128, 256)
    fwd = lambda x, w2_=w2, **kw: ops.stage1_block_train(x, w1, ones(256), w2_, w3, ones(128), ones(128), **kw)
    bwd = lambda d, w2_=w2, **kw: ops.stage1_block_dgrad(d, w1, w2_, w3, z(*d.shape[:3], 256, dt=d.dtype), z(*d.shape[:3], 256, dt=d.dtype), **kw)
    for bad in (torch.float16, torch.float32):              # f16 bits must not be read as bf16; there is no fp32 ring kernel
        with pytest.raises(ValueError, match='FSVIT_BF16 only'):
            fwd(z(1, 4, 4, 128, dt=bad))
        with pytest.raises(ValueError, match='FSVIT_BF16 only'):
            bwd(z(1, 4, 4, 128, dt=bad))
    for shape in ((1, 4, 21), (1, 3, 3)):                   # W = 21: past the ring's halo; H * W = 9: less than one 16-pixel tile
        with pytest.raises(ValueError, match='W <= 20, H \\* W >= 16'):
            fwd(z(*shape, 128))
        with pytest.raises(ValueError, match='W <= 20, H \\* W >= 16'):
            bwd(z(*shape, 128))
    x = z(2, 4, 4, 128)
    with pytest.raises(ValueError, match='overlaps'):
        fwd(x, out=x)
    with pytest.raises(ValueError, match='overlaps'):
        bwd(x, dxn=x)
    for f in (fwd, bwd):
        with pytest.raises(ValueError, match='row length 288'):
            f(x, w2_=z(256, 288))
    wf = torch.zeros(8, 8, 1, 1).cuda()
    with pytest.raises(ValueError, match='mode 3'):
        ops.pack_weight(wf, mode=3, rows_pad=32, Kw=32)
    with pytest.raises(ValueError, match='mode 4'):
        ops.pack_weight(wf, mode=4, rows_pad=32, Kw=32)
    with pytest.raises(ValueError, match='FSVIT_BF16X2'):
        ops.pack_weight(wf, dtype=torch.float16)
    with pytest.raises(ValueError, match='needs rows_pad'):
        ops.pack_weight(wf, rows_pad=4, Kw=64)                 # rows that would be dropped silently
    xc, wc = z(1, 4, 4, 64), z(1, 64, 64)
    with pytest.raises(ValueError, match='y2 .* without act = GELU'):
        ops.conv_train(xc, wc, None, 1, 1, 1, 0, 64, 1, ops.ACT_NONE, with_y2=True)
    with pytest.raises(ValueError, match='act = MUL without mul'):
        ops.conv_train(xc, wc, None, 1, 1, 1, 0, 64, 1, ops.ACT_MUL)
    with pytest.raises(ValueError, match='mul without act = MUL'):
        ops.conv_train(xc, wc, None, 1, 1, 1, 0, 64, 1, ops.ACT_GELU, mul=z(1, 4, 4, 64))
    with pytest.raises(ValueError, match='FSVIT_F32 and FSVIT_BF16'):
        ops.conv_train(z(1, 4, 4, 64, dt=torch.float16), z(1, 64, 64, dt=torch.float16), None, 1, 1, 1, 0, 64, 1, ops.ACT_NONE)
    with pytest.raises(ValueError, match='FSVIT_BF16 only'):
        ops.gconv3x3_train(z(1, 4, 4, 256, dt=torch.float16), z(256, 320, dt=torch.float16), with_y2=True)
    with pytest.raises(ValueError, match='W <= 20'):
        ops.gconv3x3_train(z(1, 2, 21, 256), z(256, 320), with_y2=True)
    torch.cuda.synchronize()
