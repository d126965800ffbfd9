"""Cases, inputs, references and gates of the stand-alone attention kernels (attention.hip, attention_bwd.hip), shared by test_attention_ref_cpu.py (the
references and the route table, no GPU) and test_gpu_attention_ops.py (the kernels).

A case: (id, dict(dt, S, hd, hdp, B, heads, regime, route)).  `route` is the id the launcher's own route function must return for the shape
(fsvit.h: fsvit_op_attention_route / fsvit_op_attention_bwd_route; -1 = refused) - the CPU test asserts it for every case and asserts that the table
reaches every instantiation listed in FWD_INSTANCES / BWD_INSTANCES.  B = 2, heads = 3 (b > 0 and h > 0 offsets) except one case per operator with
B = heads = 1.  The float64 reference covers every (image, head) and element.

dt: 'f32' | 'bf16' | 'f16' (storage types) | 'bf16x2' | 'f16x2' (forward only: fp32 rows, two-limb products).

Input regimes (all rounded to the storage type; pad channels hd .. hdp-1 of q, k, v, dO zero):
  flat      randn
  peaked    q x 4: the scaled scores have deviation 4 - at 100 keys the median row maximum of P is above 0.5 and a tenth of the rows is nearly
            one-hot (max P > 0.9), where dS cancels
  offset    k + 25 sqrt(hd) w, w a unit vector: every score of query i moves by 25 (q_i . w), past +-60 over the rows, the same for all keys of a row -
            only the max-subtraction keeps exp in range; P is unchanged in exact arithmetic
  zero_row  query row 1 of every head all zero (uniform P) and key row S - 2 all zero (score 0 for every query)
fp16 / f16x2 inputs stay below 2^10 (asserted on the CPU), nothing nears 65504.

Gates.  None of their constants comes from a kernel run.
  16-bit storage and two-limb: gate 1 and gate 2 of tests/rows_cases.py (rc.gate) with A = *_exact, P = *_points of oracle/attention_oracle.py - per
    element |got - A| <= u |A| + 6 max(sigma, P.sig) + P.acc, mean |got - A| <= 1.25 mean |P.out - A|; backward: dQ, dK, dV each on its own.
  fp32 storage: |got - A| <= P.acc + u32 |A|, P.acc = the deterministic first-order fp32 allowance (oracle/attention_oracle.py fp32_allowance_*; written
    out in the header of test_gpu_attention_ops.py).
"""
import math
import zlib

import torch

import rows_cases as rc
from oracle import attention_oracle as ao

TD = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16, 'bf16x2': torch.float32, 'f16x2': torch.float32}
LIMB = {'bf16x2': torch.bfloat16, 'f16x2': torch.float16}
# fsvit.h dtype codes (few-shot-vit_amd/_lib.py F32 .. F16X2)
CODE = {'f32': 0, 'bf16': 1, 'f16': 2, 'bf16x2': 3, 'f16x2': 4}
ELEM = {'f32': 0, 'bf16': 1, 'f16': 1, 'bf16x2': 2, 'f16x2': 2}
HD_OF = {16: 10, 32: 21, 48: 42, 64: 64, 80: 70, 96: 85, 112: 100, 128: 120}      # the real head dim the forward cases put into a padded one
REGIMES = ('peaked', 'offset', 'zero_row')


def fwd_id(family, elem, nkt=0, ndt=0):
    return family * 100000 + elem * 10000 + nkt * 100 + ndt


bwd_id = fwd_id

# every kernel instantiation behind launch_attention, as (dt, route id): attention_v2_kernel<T, NKT, NDT> of dispatch_ndt + the generic attention_kernel<T>.
# (the exact-fp32 kernels exist in both 16-bit builds of attention.hip: 'f32' runs the bf16 build's, a two-limb shape without a two-limb kernel its own
# build's - only the generic kernel is reachable that way, the v2 sets of float and f32x2l being equal)
_NDT = {0: (1, 2, 3, 4, 5, 6, 8), 1: (2, 3, 4, 6, 8), 2: (1, 2, 3, 4, 5, 6, 8)}
_NKT = {0: (2, 7, 13), 1: (2, 8, 14), 2: (2, 7, 13)}
_NO_LDS = ((13, 6), (13, 8))      # fp32 rows at 13 key tiles: head dims 96 and 128 need 164 / 217 KB of LDS - not built, refused by the route
FWD_INSTANCES = [(dt, fwd_id(1, ELEM[dt], nkt, ndt)) for dt in TD for nkt in _NKT[ELEM[dt]] for ndt in _NDT[ELEM[dt]]
                 if ELEM[dt] == 1 or (nkt, ndt) not in _NO_LDS] + \
                [('f32', fwd_id(2, 0)), ('bf16', fwd_id(2, 1)), ('f16', fwd_id(2, 1)), ('bf16x2', fwd_id(2, 0)), ('f16x2', fwd_id(2, 0))]
BWD_INSTANCES = [('bf16', bwd_id(1, 1, nkt, ndt)) for nkt, ndts in ((2, (2, 4, 6, 8)), (8, (2, 4, 6)), (14, (2, 4))) for ndt in ndts] + \
                [('f32', bwd_id(2, 0, 2, 3)), ('f32', bwd_id(2, 0, 2, 6)), ('f32', bwd_id(2, 0, 3, 4)), ('f32', bwd_id(2, 0, 7, 3)), ('f32', bwd_id(3, 0, 13, 4)),
                 ('f32', bwd_id(4, 0)), ('bf16', bwd_id(4, 1)), ('f32', bwd_id(5, 0))]


def _case(dt, S, hd, hdp, route, regime='flat', B=2, heads=3):
    cid = f'{dt}-S{S}-hd{hd}' + (f'to{hdp}' if hdp != hd else '') + ('' if regime == 'flat' else f'-{regime}') + ('-B1h1' if B == 1 else '')
    return cid, dict(dt=dt, S=S, hd=hd, hdp=hdp, B=B, heads=heads, regime=regime, route=route)


def _forward_cases():
    out = []
    # token counts of each key-tile count: both sides of every dispatch threshold, exact multiples of 16, S = 1
    s_of = {1: {2: (1, 16, 17, 32), 8: (33, 112, 113, 128), 14: (129, 197, 208, 209, 224)},
            0: {2: (1, 16, 17, 32), 7: (33, 100, 112), 13: (113, 128, 129, 197, 208)}}
    s_of[2] = s_of[0]
    for dt in TD:
        el = ELEM[dt]
        for nkt in _NKT[el]:
            ss = s_of[el][nkt]
            for i, ndt in enumerate(_NDT[el]):          # every instantiated hdp / 16 (16-bit: 3 = the half chunk; fp32: 1 and 5), the token counts in turn
                hdp = 16 * ndt
                fits = el == 1 or (nkt, ndt) not in _NO_LDS
                out.append(_case(dt, ss[i % len(ss)] if fits else 197, HD_OF[hdp], hdp, fwd_id(1, el, nkt, ndt) if fits else -1))
            for regime in REGIMES:                       # the regimes at one shape per route: 42 -> 64 at the largest token count but one
                out.append(_case(dt, ss[-2], 42, 64, fwd_id(1, el, nkt, 4), regime))
    out.append(_case('bf16', 100, 42, 64, fwd_id(1, 1, 8, 4), B=1, heads=1))
    # the generic v1 kernel: hdp / 16 = 5 (16-bit) and 7 (fp32: also where a two-limb mode lands), at its own edges S = 1 and S = 128
    for dt in ('bf16', 'f16'):
        for S in (25, 1, 128):
            out.append(_case(dt, S, 70, 80, fwd_id(2, 1)))
        out.append(_case(dt, 100, 100, 112, fwd_id(2, 1)))
    for dt in ('f32', 'bf16x2', 'f16x2'):
        out.append(_case(dt, 25, 100, 112, fwd_id(2, 0)))
    out.append(_case('f32', 80, 100, 112, fwd_id(2, 0)))        # (its LDS image passes 160 KB from S = 96)
    for regime in REGIMES:
        out.append(_case('bf16', 25, 70, 80, fwd_id(2, 1), regime))
        out.append(_case('f32', 25, 100, 112, fwd_id(2, 0), regime))
    # refused
    for dt in TD:
        out.append(_case(dt, 25, 40, 40, -1))                                      # hdp % 16 != 0
        out.append(_case(dt, 225 if ELEM[dt] == 1 else 209, 64, 64, -1))          # past the last key-tile count
    out.append(_case('f32', 129, 100, 112, -1))                                    # no v2 instantiation and past the v1 limit
    out.append(_case('bf16', 129, 70, 80, -1))
    return out


def _backward_cases():
    out = []
    for nkt, tokens, dims in ((2, (1, 15, 16, 17, 32), ((21, 32), (64, 64), (85, 96), (120, 128))),
                              (8, (33, 100, 112, 113, 128), ((21, 32), (42, 64), (85, 96))),
                              (14, (129, 197, 209, 224), ((32, 32), (64, 64)))):
        for S in tokens:
            for hd, hdp in dims:
                out.append(_case('bf16', S, hd, hdp, bwd_id(1, 1, nkt, hdp // 16)))
    out += [_case('bf16', 100, 42, 48, bwd_id(4, 1)), _case('bf16', 40, 120, 128, bwd_id(4, 1)),
            _case('bf16', 197, 85, 96, -1), _case('bf16', 225, 32, 32, -1)]
    for S in (1, 25, 32):
        for hd, hdp in ((21, 32), (42, 48)):
            out.append(_case('f32', S, hd, hdp, bwd_id(2, 0, 2, 3)))
    out.append(_case('f32', 25, 85, 96, bwd_id(2, 0, 2, 6)))
    out += [_case('f32', S, 64, 64, bwd_id(2, 0, 3, 4)) for S in (33, 48)]
    out += [_case('f32', S, 42, 48, bwd_id(2, 0, 7, 3)) for S in (49, 100, 112)]
    out += [_case('f32', S, hd, hdp, bwd_id(3, 0, 13, 4)) for S, hd, hdp in ((100, 64, 64), (113, 56, 64), (197, 64, 64), (208, 32, 32))]
    out += [_case('f32', 40, 80, 80, bwd_id(4, 0)), _case('f32', 120, 80, 80, bwd_id(5, 0)), _case('f32', 209, 64, 64, bwd_id(5, 0))]
    # the regimes at one shape per route; B = heads = 1
    for regime in REGIMES:
        out += [_case('bf16', 17, 21, 32, bwd_id(1, 1, 2, 2), regime), _case('bf16', 100, 42, 64, bwd_id(1, 1, 8, 4), regime),
                _case('bf16', 197, 64, 64, bwd_id(1, 1, 14, 4), regime), _case('bf16', 40, 120, 128, bwd_id(4, 1), regime),
                _case('f32', 25, 42, 48, bwd_id(2, 0, 2, 3), regime), _case('f32', 25, 85, 96, bwd_id(2, 0, 2, 6), regime),
                _case('f32', 48, 64, 64, bwd_id(2, 0, 3, 4), regime), _case('f32', 100, 42, 48, bwd_id(2, 0, 7, 3), regime),
                _case('f32', 113, 56, 64, bwd_id(3, 0, 13, 4), regime), _case('f32', 40, 80, 80, bwd_id(4, 0), regime),
                _case('f32', 120, 80, 80, bwd_id(5, 0), regime)]
    out.append(_case('bf16', 100, 42, 64, bwd_id(1, 1, 8, 4), B=1, heads=1))
    return out


CASES = {'forward': _forward_cases(), 'backward': _backward_cases()}
for _op in CASES:
    assert len(dict(CASES[_op])) == len(CASES[_op]), 'duplicate case id'


def params_of(op, cid):
    return dict(CASES[op])[cid]


def ids(op, refused=False):
    return [cid for cid, p in CASES[op] if (p['route'] < 0) == refused]


def kind_of(op, p):
    """the rounding-points form of the case's kernel family (oracle/attention_oracle.py)"""
    family, dt = p['route'] // 100000, p['dt']
    if dt == 'f32' or (dt in LIMB and p['route'] // 10000 % 10 == 0):
        return 'f32'
    if op == 'forward':
        return 'x2' if dt in LIMB else ('v2' if family == 1 else 'v1')
    return 'mfma' if family == 1 else 'fma'


def points_dtype(p):
    """the type the points form rounds to: the storage type, or the limb type of a two-limb case"""
    return LIMB.get(p['dt'], TD[p['dt']])


def gate_dtype(op, p):
    """the type whose half ulp is gate 1's u: the storage type"""
    return TD[p['dt']]


# ------------------------------------------------------------------------------------------------------------------------------- inputs
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) % (2 ** 31))


def inputs(op, p):
    """-> dict(qkv [B S, 3 heads hdp], dctx [B S, heads hdp] (backward only)) in the storage type, pad channels zero"""
    B, S, heads, hd, hdp = p['B'], p['S'], p['heads'], p['hd'], p['hdp']
    g = _gen(op, sorted((k, v) for k, v in p.items() if k != 'route'))
    x = torch.randn(B, S, 3, heads, hd, generator=g)
    if p['regime'] == 'peaked':
        x[:, :, 0] *= 4.0
    elif p['regime'] == 'offset':
        w = torch.randn(hd, generator=g)
        x[:, :, 1] += 25.0 * math.sqrt(hd) * w / w.norm()
    elif p['regime'] == 'zero_row':
        x[:, 1 % S, 0] = 0.0
        x[:, max(S - 2, 0), 1] = 0.0
    qkv = torch.zeros(B, S, 3, heads, hdp)
    qkv[..., :hd] = x
    t = {'qkv': qkv.reshape(B * S, 3 * heads * hdp).to(TD[p['dt']])}
    if op == 'backward':
        do = torch.zeros(B, S, heads, hdp)
        do[..., :hd] = torch.randn(B, S, heads, hd, generator=g)
        t['dctx'] = do.reshape(B * S, heads * hdp).to(TD[p['dt']])
    return t


def scale_of(p):
    return p['hd'] ** -0.5


_REF = {}


def reference(op, cid):
    """-> (A, P): *_exact and *_points of the case in float64, computed once per process"""
    if (op, cid) not in _REF:
        p = params_of(op, cid)
        t = {k: v.double() for k, v in inputs(op, p).items()}
        a = (p['B'], p['S'], p['heads'], p['hdp'], scale_of(p))
        kind, dtype = kind_of(op, p), points_dtype(p)
        if op == 'forward':
            _REF[(op, cid)] = ao.forward_exact(t['qkv'], *a), ao.forward_points(t['qkv'], *a, kind, dtype)
        else:
            _REF[(op, cid)] = ao.backward_exact(t['qkv'], t['dctx'], *a), ao.backward_points(t['qkv'], t['dctx'], *a, kind, dtype)
    return _REF[(op, cid)]


# ------------------------------------------------------------------------------------------------------------------------------- gates
def parts(op, p, t):
    """the tensors the gates are applied to separately: ctx, or dQ / dK / dV of a [B S, 3 heads hdp] map (Points too)"""
    if op == 'forward':
        return {'ctx': t}
    n = p['heads'] * p['hdp']
    cut = lambda x, i: None if x is None else x.reshape(-1, 3, n)[:, i]
    if isinstance(t, ao.Points):
        return {name: ao.Points(*(cut(f, i) for f in t)) for i, name in enumerate(('dQ', 'dK', 'dV'))}
    return {name: cut(t, i) for i, name in enumerate(('dQ', 'dK', 'dV'))}


def gate(op, p, got, A, P):
    """got (float64, the kernel's output or P.out / another evaluation for the reference-alone test) against the case's gates ->
    dict(worst = max err / bound over the parts, ratio = the largest mean ratio (None for fp32 storage), per = the parts' figures)"""
    gp, ap, pp = parts(op, p, got), parts(op, p, A), parts(op, p, P)
    per = {}
    for name in gp:
        if kind_of(op, p) == 'f32':      # fp32 arithmetic on fp32 rows (a two-limb shape on the exact-fp32 kernel included)
            bound = pp[name].acc + ao.U * ap[name].abs()
            err = (gp[name] - ap[name]).abs()
            worst = float(torch.where(bound > 0, err / bound, torch.where(err > 0, math.inf, 0.0).double()).max())
            per[name] = dict(worst=worst, ratio=None)
        else:
            per[name] = rc.gate(gp[name], ap[name], pp[name], gate_dtype(op, p))
    ratios = [g['ratio'] for g in per.values() if g['ratio'] is not None]
    return dict(worst=max(g['worst'] for g in per.values()), ratio=max(ratios) if ratios else None, per=per)
