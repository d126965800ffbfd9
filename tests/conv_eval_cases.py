"""Cases, inputs, checked subsets, references and bounds of the kernels every evaluation runs first - conv3x3_halo.hip, conv_gemm_v2.hip, gemm256.hip with
their eval epilogues and the stage-1 block (stage1_w4.hip, stage1_ring.hip) - shared by test_conv_eval_ref_cpu.py (the references alone, no GPU) and
test_gpu_conv_eval_ops.py (the kernels against them).  The references are those of oracle/conv_eval_oracle.py.

SINGLE-GEMM KERNELS.  One output is one dot product plus an epilogue; no stored intermediate can flip, so EVERY element is held to float64:
    |got - ref| <= stored_tol(ref, dt, a),     a = slope (sum_tol(sum_k |x_k w_k|, K_total) + u (|bias| + |res| + |pos|)) [+ 2^-20 |z| behind a GELU]
with u = 2^-24, K_total the chain's length (the tail slice included), slope 1 (none, LeakyReLU) or L0 (GELU: 1.01 x the largest slope of the reference
GELU, test_gpu_train_conv_ops.lipschitz).  fp32 storage adds u sum |x_k w_k| (the fp32 MFMA rounds its products); the two-limb modes add the
operand-precision term of test_conv_gemm_two_limb, 1e-4 (bf16 limbs) / 2e-5 (fp16 limbs), times the ELEMENT's sum |x_k w_k|.  A pooled element takes the
largest bound of its window.  check / sum_tol / U are those of test_gpu_train_ops.py; half_ulp / stored_tol / q are restated here with fp16 added
(11 bits) - the formulas are the same.  None of these constants comes from a kernel run.

LARGE CASES.  Where a case exists for the second walk of a persistent grid, the float64 reference is formed for a subset - images: the first two, the last
four and every image of a tile that a workgroup reaches on its second walk; rows: rows_cases.rows_subset - and every other image (row) is a COPY of a
subset image (row): its output must be bit-equal to its twin's, which also asserts that a value does not depend on its position in the launch.

STAGE-1 BLOCK.  The hidden maps never leave the chip: the two gates of rows_cases.gate against stage1_exact with stage1_points as the model of the
rounding points (the CPU test proves the model itself passes gate 1 for every case and type).

The row-chunk-planar converters are written from the formula of conv_gemm.h (ConvGemmParams::x_planar): element (b, row, col, c) at
((b H + row) (C / 8) + c / 8) W 8 + col 8 + c % 8.
"""
import math

import torch

import rows_cases as rc
from oracle import conv_eval_oracle as co
from rows_cases import _gen, rows_subset, weight
from test_gpu_train_ops import U, check, sum_tol      # noqa: F401  (check is re-exported for the GPU test)

DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
PBITS = {'f32': 24, 'bf16': 8, 'f16': 11}
E20 = 2.0 ** -20
X2_GATE = {'bf16x2': 1e-4, 'f16x2': 2e-5}       # test_gpu_ops.test_conv_gemm_two_limb: operand precision 2^-16 / 2^-21
HALO_GRID = 256                                 # conv3x3_halo: persistent grid, tile t of workgroup t % 256
TW, TR = 40, 8                                  # its tile: 8 rows of the 40-pixel-wide map


def q(t, dt):
    """round to the storage type; float64 result"""
    return t.to(DTYPES[dt]).double()


def half_ulp(ref, dt, a):
    mag = (ref.abs() + a).clamp_min(2.0 ** -120)
    return torch.ldexp(torch.ones_like(mag), (torch.floor(torch.log2(mag)) - PBITS[dt]).to(torch.int32))


def stored_tol(ref, dt, a):
    return half_ulp(ref, dt, a) + a


# --------------------------------------------------------------------------------------------------------------------------- planar <-> NHWC
def _planar_index(B, H, W, C, device=None):
    b, r, c, ch = torch.meshgrid(*(torch.arange(n, device=device) for n in (B, H, W, C)), indexing='ij')
    return (((b * H + r) * (C // 8) + ch // 8) * W * 8 + c * 8 + ch % 8).reshape(-1)


def to_planar(x):
    """x NHWC [B, H, W, C] -> the same elements in the row-chunk-planar order, flat [B H W C]"""
    B, H, W, C = x.shape
    out = torch.empty(x.numel(), dtype=x.dtype, device=x.device)
    out[_planar_index(B, H, W, C, x.device)] = x.reshape(-1)
    return out


def from_planar(p, B, H, W, C):
    """flat row-chunk-planar -> NHWC [B, H, W, C]"""
    return p.reshape(-1)[_planar_index(B, H, W, C, p.device)].reshape(B, H, W, C)


# --------------------------------------------------------------------------------------------------------------------------- the halo kernel's cases
# kind -> (Cin, act, tail); N = 128, 'c96*': N = 96, the 96-channel layer on the 128-channel weight image (w_cpad = 128)
HALO_KINDS = {'conv2': (64, 2, False), 'plain128': (128, 0, False), 'gelu128': (128, 1, False), 'tail128': (128, 2, True), 'c96': (96, 2, False),
              'c96tail': (96, 2, True)}


def _halo_cases():
    out = []

    def add(kind, B, H, xl, yl):
        out.append((f'{kind}-B{B}-H{H}-x{xl}-y{yl}', dict(kind=kind, B=B, H=H, xl=xl, yl=yl)))
    for B, H in ((1, 8), (2, 16), (1, 40), (259, 8)):
        for xl, yl in ((('n', 'n'), ('n', 'p'), ('p', 'n'), ('p', 'p')) if (B, H) in ((1, 8), (1, 40)) else (('p', 'p'),)):
            add('conv2', B, H, xl, yl)
    for kind in ('plain128', 'gelu128'):
        for B, H in ((1, 8), (1, 40)):
            for xl in 'np':
                add(kind, B, H, xl, 'n')
    for B, H in ((1, 8), (1, 40), (259, 8)):
        for xl in 'np':
            add('tail128', B, H, xl, 'n')
    for B, H in ((1, 8), (1, 40)):
        add('c96', B, H, 'n', 'n')
    for B, H in ((1, 8), (1, 40), (259, 8)):
        add('c96tail', B, H, 'n', 'n')
    return out


HALO_CASES = _halo_cases()
HALO_STATS_CASES = [(f'{kind}-B{B}-H8', dict(kind=kind, B=B, H=8, xl='n', yl='n')) for kind in ('stats64', 'stats128') for B in (1, 259)]
HALO_KINDS.update(stats64=(64, 0, False), stats128=(128, 0, False))
C1F_CASES = [('B1', dict(B=1, split=1)), ('B3-split1', dict(B=3, split=1)), ('B53', dict(B=53, split=53))]


def image_subset(B, tiles_per_img):
    """images the float64 reference is formed for: all of a small case; else the first two, the last four, the images of the second-walk tiles"""
    if B <= 8:
        return torch.arange(B)
    second = torch.arange(HALO_GRID, B * tiles_per_img) // tiles_per_img
    return torch.unique(torch.cat([torch.arange(2), torch.arange(B - 4, B), second]))


def twins(B, sub):
    """-> src [B]: the subset image each image is a copy of (itself for a subset image)"""
    src = sub[torch.arange(B) % len(sub)].clone()
    src[sub] = sub
    return src


def halo_inputs(p, dt):
    """CPU tensors of a halo case in the storage type: x NHWC (the copies included), sub / src, the conv weights w [N, C, 3, 3] and their packed image wp,
    bias, and for a tail case x2 [B H 40, 32], w2 [N, 32], pos"""
    C, act, tail = HALO_KINDS[p['kind']]
    dtype, B, H = DTYPES[dt], p['B'], p['H']
    g = _gen('halo', p['kind'], B, H)
    sub = image_subset(B, H // TR)
    src = twins(B, sub)
    N = 96 if C == 96 else 128
    t = dict(sub=sub, src=src, C=C, N=N, act=act, tail=tail)
    x = torch.zeros(B, H, TW, C)
    x[sub] = torch.randn(len(sub), H, TW, C, generator=g)
    t['x'] = x[src].to(dtype)
    w = weight(g, N, 9 * C, dtype).float().reshape(N, 3, 3, C)                  # [n][ky][kx][c]: the packed K order
    t['w'] = w.permute(0, 3, 1, 2).contiguous()
    t['bias'] = torch.randn(N, generator=g) * 0.3
    cp = 128 if C == 96 else C                                                  # channels per tap of the packed rows (128 rows in every kind)
    kw = 9 * cp + (64 if tail else 0)
    wp = torch.zeros(128, kw)
    wimg = torch.zeros(128, 3, 3, cp)
    wimg[:N, :, :, :C] = w
    wp[:, :9 * cp] = wimg.reshape(128, 9 * cp)
    if tail:
        x2 = torch.zeros(B, H * TW, 32)
        x2[sub] = torch.randn(len(sub), H * TW, 32, generator=g)
        t['x2'] = x2[src].reshape(B * H * TW, 32).to(dtype)
        t['w2'] = weight(g, N, 32, dtype).float()
        wp[:N, 9 * cp:9 * cp + 32] = t['w2']
        if p['kind'] == 'tail128':
            t['pos'] = torch.randn((H // 2) * (TW // 2), N, generator=g) * 0.2
    t['wp'] = wp.to(dtype)
    return t


def gelu_slope(z, a_z, kind):
    from test_gpu_train_conv_ops import lipschitz
    return lipschitz(kind)[0] * a_z + E20 * z.abs()


def conv_reference(x, w, bias, dt, act=0, stride=1, pad=0, groups=1, x2=None, w2=None, res=None, res_first=False, pool2=False, pos=None, numerics=None):
    """float64 reference and per-element bound of one conv launch.  x NCHW / w [O, Ig, KH, KW] float64 values of the storage type (two-limb modes: the
    unrounded fp32 values) -> (ref, a, pre): NCHW output, its arithmetic allowance, and the UNPOOLED map behind the activation with its allowance"""
    z, s = co.conv_pre(x, w, bias, stride, pad, groups, x2, w2)
    K = w.shape[1] * w.shape[2] * w.shape[3] + (0 if x2 is None else x2.shape[1])
    a = sum_tol(s, K) + U * (0.0 if bias is None else bias.abs().view(1, -1, 1, 1))
    if dt == 'f32':
        a = a + U * s
    if numerics:
        a = a + X2_GATE[numerics] * s
    kind = 'sig' if dt != 'f32' else 'erf'
    if res is not None and res_first:
        a = a + U * res.abs()
    zz = z + res if (res is not None and res_first) else z
    y = co.act_fn(act, kind)(zz)
    if act == 1:
        a = gelu_slope(zz, a, kind)
    if res is not None and not res_first:
        y, a = y + res, a + U * res.abs()
    pre = (y, a)
    if pool2:
        y = torch.nn.functional.max_pool2d(y, 2)
        a = torch.nn.functional.max_pool2d(a, 2)
    if pos is not None:
        pm = pos.t().reshape(1, y.shape[1], y.shape[2], y.shape[3])
        y, a = y + pm, a + U * pm.abs()
    return y, a, pre


def halo_reference(p, t, dt):
    """-> (ref, a, pre) of the subset images, NHWC"""
    sub, C = t['sub'], t['C']
    x = t['x'][sub].double().permute(0, 3, 1, 2)
    n = len(sub)
    H = p['H']
    x2 = None
    if t['tail']:
        x2 = t['x2'].reshape(p['B'], H * TW, 32)[sub].reshape(n * H * TW, 32).double()
    y, a, pre = conv_reference(x, t['w'].double(), t['bias'].double(), dt, act=t['act'], pad=1, x2=x2, w2=t['w2'].double() if t['tail'] else None,
                               pool2=t['tail'], pos=t['pos'].double() if 'pos' in t else None)
    nhwc = lambda v: v.permute(0, 2, 3, 1).contiguous()
    return nhwc(y), nhwc(a), (nhwc(pre[0]), nhwc(pre[1]))


def c1f_inputs(p, dt):
    """raw images [B, 3, 80, 80] fp32 (values of the storage type; copies of the subset images), conv1's packed weights [64, 64] / bias, conv2's weights"""
    dtype, B = DTYPES[dt], p['B']
    g = _gen('c1f', B)
    sub = image_subset(B, 5)
    src = twins(B, sub)
    img = torch.zeros(B, 3, 80, 80)
    img[sub] = torch.randn(len(sub), 3, 80, 80, generator=g)
    w1 = torch.zeros(64, 64)
    w1[:, :27] = weight(g, 64, 27, dtype).float()
    w = weight(g, 128, 9 * 64, dtype)
    return dict(sub=sub, src=src, img=img[src].to(dtype).float(), w1=w1.to(dtype), b1=torch.randn(64, generator=g) * 0.2, wp=w,
                bias=torch.randn(128, generator=g) * 0.3)


# --------------------------------------------------------------------------------------------------------------------------- conv_gemm_v2 / gemm256
def conv_case_inputs(case, dt, numerics=None):
    """a row of CASES of test_gpu_ops.py -> x NCHW, w [O, Ig, KH, KH], bias, res NCHW, pos in the storage type (two-limb modes: unrounded fp32)"""
    name, B, H, W, Cin, O, KH, s, p, groups, act, use_res, res_first, use_bias, use_pos = case
    dtype = DTYPES[dt]
    g = _gen('conv', name)
    Ig = Cin // groups
    OH, OW = (H + 2 * p - KH) // s + 1, (W + 2 * p - KH) // s + 1
    x = torch.randn(B, Cin, H, W, generator=g).to(dtype)
    w = weight(g, O, KH * KH * Ig, dtype).float().reshape(O, KH, KH, Ig).permute(0, 3, 1, 2).contiguous()
    return dict(x=x, w=w, bias=torch.randn(O, generator=g) * 0.3 if use_bias else None,
                res=torch.randn(B, O, OH, OW, generator=g).to(dtype) if use_res else None, pos=torch.randn(OH * OW, O, generator=g) * 0.2 if use_pos else None)


def gemm_rows_inputs(M, N, K, dt, BM, wrap, key, numerics=None, bias=True):
    """a plain [M][K] x [N][K] layer: the rows of rows_subset(M, BM, wrap) random, every other row a copy of one of them -> dict(x, w, bias, sub, src)"""
    dtype = DTYPES[dt]
    g = _gen('gemm', key, M, N, K)
    sub = rows_subset(M, BM, wrap)
    src = twins(M, sub)
    x = torch.zeros(M, K)
    x[sub] = torch.randn(len(sub), K, generator=g)
    w = weight(g, N, K, dtype if not numerics else torch.float32).float()
    return dict(sub=sub, src=src, x=x[src].to(dtype), w=w, bias=torch.randn(N, generator=g) * 0.3 if bias else None)


# rows of the CASES form of test_gpu_ops.py: the y_rpi / y_row0 case (3 images of 16 patch rows behind a cls row each, S = 17) and the grouped 3 x 3 second walk
Y_RPI_CASE = ('y_rpi', 3, 4, 4, 64, 96, 1, 1, 0, 1, 0, False, 0, True, True)
Y_RPI_S = 17
GROUPED_WALK_CASE = ('3x3_grouped_walk', 31, 20, 20, 256, 256, 3, 1, 1, 8, 1, False, 0, False, False)


def case_reference(case, t, dt, numerics=None, images=None):
    """conv_reference of a CASES-form row on the inputs t (of the images `images`, default all) -> (ref, a) NCHW"""
    B, H, W, Cin, O, KH, s, p, groups, act, use_res, res_first = case[1:13]
    d = lambda v: None if v is None else v.double()
    pick = (lambda v: v) if images is None else (lambda v: None if v is None else v[images])
    ref, a, _ = conv_reference(d(pick(t['x'])), d(t['w']), d(t['bias']), dt, act=act, stride=s, pad=p, groups=groups, res=d(pick(t['res'])),
                               res_first=bool(res_first), pos=d(t['pos']), numerics=numerics)
    return ref, a


def rows_reference(t, dt, act=0, numerics=None):
    """conv_reference of the reference rows of a plain [M][K] x [N][K] layer (gemm_rows_inputs) -> (ref, a) [len(sub), N]"""
    sub, (N, K) = t['sub'], t['w'].shape
    ref, a, _ = conv_reference(t['x'][sub].double().reshape(len(sub), K, 1, 1), t['w'].double().reshape(N, K, 1, 1),
                               None if t['bias'] is None else t['bias'].double(), dt, act=act, numerics=numerics)
    return ref.reshape(len(sub), N), a.reshape(len(sub), N)


# name: (M, N, K, BM, wrap = first row of the tile a workgroup reaches on its second walk, expected route per dtype family)
WALK_CASES = {
    'v2_128x128': dict(M=128 * 513, N=128, K=64, BM=128),
    'v2_128x64': dict(M=128 * 769, N=64, K=32, BM=128),
    'v2_128x32': dict(M=128 * 769, N=32, K=32, BM=128),
    'g256_k128': dict(M=8448, N=2048, K=128, BM=256),          # 33 x 8 tiles of 256 x 256; bf16: below gemm256's arithmetic-intensity gate -> conv_gemm_v2
    'g256_k256': dict(M=8448, N=2048, K=256, BM=256),          # ... the same tiles on gemm256 in bf16 as well (264 tiles on 256 workgroups)
}
V2_STATS_CASES = {'N64-M200': dict(M=200, N=64, K=64, rows=8, idle=6), 'N128-M600': dict(M=600, N=128, K=64, rows=16, idle=6),
                  'N128-M33280': dict(M=128 * 260, N=128, K=64, rows=512, idle=0)}


# --------------------------------------------------------------------------------------------------------------------------- stage-1 block
def _stage1_cases():
    out = [(f'B{B}-H{H}', dict(B=B, H=H, b1='randn')) for B, H in ((4, 4), (3, 7), (5, 10), (1, 20), (5, 20), (42, 20))]
    out.append(('B5-H20-b1wide', dict(B=5, H=20, b1='wide')))
    return out


STAGE1_CASES = _stage1_cases()


def stage1_inputs(p, dt):
    """x rows [B H H, 128], w1 [256, 128], b1 [256] fp32, w2 [256, 32, 3, 3], w3 [128, 256] - storage-typed"""
    dtype, B, H = DTYPES[dt], p['B'], p['H']
    g = _gen('stage1', B, H, p['b1'])
    t = dict(x=torch.randn(B * H * H, 128, generator=g).to(dtype), w1=weight(g, 256, 128, dtype), w2=weight(g, 256, 288, dtype), w3=weight(g, 128, 256, dtype))
    b1 = torch.randn(256, generator=g) * 0.2
    if p['b1'] == 'wide':      # a quarter of the channels at +- 30 (the table's upper end), a quarter at magnitudes in [2^-14, 2^-11)
        sign = torch.where(torch.rand(256, generator=g) < 0.5, -1.0, 1.0)
        tiny = torch.exp2(-14.0 + 3.0 * torch.rand(256, generator=g)).clamp(max=2.0 ** -11 * (1 - 2.0 ** -10))
        sel = torch.arange(256) % 4
        b1 = torch.where(sel == 0, 30.0 * sign, torch.where(sel == 1, tiny * sign, b1))
    t['b1'] = b1
    return t


def stage1_w2_conv(w2):
    """[256, 288] rows in the packed K order (tap, c) -> [256, 32, 3, 3]"""
    return w2.reshape(256, 3, 3, 32).permute(0, 3, 1, 2).contiguous()


def stage1_pack_w2(w2, dtype):
    """-> [256][320]: the packed rows, zero-padded to the K slice"""
    out = torch.zeros(256, 320)
    out[:, :288] = w2.float()
    return out.to(dtype)


def stage1_reference(p, t, dt, table=None):
    """-> (A, P) of the whole map; table = False: the points of the 16-wave ring kernel (no GELU table in bf16)"""
    d = lambda v: v.double()
    a = (d(t['x']), d(t['w1']), d(t['b1']), stage1_w2_conv(d(t['w2'])), d(t['w3']), p['B'], p['H'], p['H'])
    return co.stage1_exact(*a), co.stage1_points(*a, DTYPES[dt], table)


gate = rc.gate


# --------------------------------------------------------------------------------------------------------------------------- the GELU table sweep
SWEEP_BINADES = list(range(-11, 6))       # 2^-11 (below the table), the table's fifteen, 2^5 (above): 17 x 128 codes per sign and call site


def sweep_inputs(dt):
    """One 16 x 16 image: pixel (sign, mantissa m) has x[0] = +-(1 + m / 128), every other channel 0.  Every dot product of the block is then ONE exact
    product and the output is a GELU value itself (stage1_w4.hip in exact arithmetic but for the two GELUs):
      hidden channel j < 17 (group 0):  W1[j, 0] = 2^e_j             -> z1 = +-(1 + m / 128) 2^e_j: every code of binade e_j at the FIRST GELU;
      hidden channel 32 + j (group 1):  W1 = 8                        -> z1 = +-8 (1 + m / 128); the bf16 GELU of z in [8, 32) is z: h1 = z1 for the positive pixels;
      conv2, centre tap only:  j <- j with 2^k (k = 4 - e_j held to the table: the positive results of the first GELU land in [8, 32) and pass the
        second GELU untouched); 64 + j <- j with -2^k (the negative results likewise); 32 + j <- 32 + j with 2^(e_j - 3) and 96 + j <- 32 + j with
        -2^(e_j - 3): z2 = +-(1 + m / 128) 2^e_j, every code of binade e_j of both signs at the SECOND GELU;
      conv3: hidden j, 32 + j, 64 + j, 96 + j -> output channels 1 + j, 33 + j, 65 + j, 97 + j (x is zero there) with weight 1."""
    dtype = DTYPES[dt]
    m = torch.arange(128, dtype=torch.float32)
    x = torch.zeros(256, 128)
    x[:128, 0] = 1.0 + m / 128.0
    x[128:, 0] = -(1.0 + m / 128.0)
    w1, w2, w3 = torch.zeros(256, 128), torch.zeros(256, 3, 3, 32), torch.zeros(128, 256)
    for j, e in enumerate(SWEEP_BINADES):
        k = 4 - min(max(e, -10), 4)
        w1[j, 0] = 2.0 ** e
        w1[32 + j, 0] = 8.0
        w2[j, 1, 1, j] = 2.0 ** k
        w2[64 + j, 1, 1, j] = -2.0 ** k             # group 2 reads hidden channels 64 .. 95: see below
        w2[32 + j, 1, 1, j] = 2.0 ** (e - 3)
        w2[96 + j, 1, 1, j] = -2.0 ** (e - 3)
        for blk in range(4):
            w3[1 + 32 * blk + j, 32 * blk + j] = 1.0
    # conv2 is grouped (hidden channels 32 g .. 32 g + 31 read only their own group): groups 2 and 3 get their own copies of the first GELU's channels
    w1[64:64 + 17] = w1[0:17]
    w1[96:96 + 17] = w1[32:32 + 17]
    return dict(x=x.to(dtype), w1=w1.to(dtype), b1=torch.zeros(256), w2=w2.reshape(256, 288).to(dtype), w3=w3.to(dtype))


def sweep_codes(t):
    """the pre-activations the two GELU call sites see on the sweep's input, by the oracle's model of the bf16 build: (z1, z2) [256 pixels, 256 channels]"""
    d = lambda v: v.double()
    z1 = d(t['x']) @ d(t['w1']).t()
    h1 = co.gelu_table(z1)
    z2 = co._conv2_g8(h1, stage1_w2_conv(d(t['w2'])), 1, 16, 16)
    return z1, z2
