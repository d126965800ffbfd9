"""TEST HELPER (a plain module, imported by tests/test_randaug_cpu.py and tests/test_gpu_randaug.py): numpy restatement of the Pillow operations
behind timm's RandAugment set 'rand-m9-mstd0.5-inc1' as the kernel behind fsvit_image_rand_augment computes them from a parameter row
(datasets/transforms.py RA_*) - `Image.transform(AFFINE, BICUBIC, fillcolor)`, the point tables (invert, posterize, solarize, solarize-add),
`ImageOps.autocontrast / equalize`, `ImageEnhance.Color / Contrast / Brightness / Sharpness` - and of the two pipelines built on it (the
distillation phase's pair with the weak view's RandAugment, the classifier phase's crop).  The parts that tests/augment_ref.py already restates
are imported from it.  Pinned bit for bit against Pillow itself and against tests/golden/randaug_pil.npz by tests/test_randaug_cpu.py."""
import numpy as np

import augment_ref as A
from fewshot_vit_amd.datasets import transforms as T


def affine(img, coef, fill):
    """Image.transform(size, AFFINE, coef, BICUBIC, fillcolor=fill) (Geometry.c affine_transform + bicubic_filter32RGB): float64, truncation."""
    H, W = img.shape[:2]
    a = [float(c) for c in coef]
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    xin = a[0] * (x + 0.5) + a[1] * (y + 0.5) + a[2]
    yin = a[3] * (x + 0.5) + a[4] * (y + 0.5) + a[5]
    with np.errstate(invalid='ignore'):
        inside = ~((xin < 0.0) | (xin >= W) | (yin < 0.0) | (yin >= H)) & np.isfinite(xin) & np.isfinite(yin)
    xin, yin = np.where(inside, xin, 0.5) - 0.5, np.where(inside, yin, 0.5) - 0.5
    fx, fy = np.floor(xin), np.floor(yin)
    dx, dy = (xin - fx)[..., None], (yin - fy)[..., None]
    fx, fy = fx.astype(np.int64), fy.astype(np.int64)
    src = img.astype(np.float64)

    def cubic(v1, v2, v3, v4, d):
        p1 = v2
        p2 = -v1 + v3
        p3 = 2 * (v1 - v2) + v3 - v4
        p4 = -v1 + v2 - v3 + v4
        return p1 + d * (p2 + d * (p3 + d * p4))
    cols = [np.clip(fx - 1 + k, 0, W - 1) for k in range(4)]
    rows = []
    for j in range(4):
        r = fy - 1 + j
        v = cubic(*(src[np.clip(r, 0, H - 1), c] for c in cols), dx)
        if j:                                             # a later row outside the image repeats the previous value
            v = np.where(((r >= 0) & (r < H))[..., None], v, rows[-1])
        rows.append(v)
    v = cubic(*rows, dy)
    out = np.where(v <= 0.0, 0.0, np.where(v >= 255.0, 255.0, v)).astype(np.uint8)
    return np.where(inside[..., None], out, np.asarray(fill, np.uint8)).astype(np.uint8)


def point_table(code, arg):
    i = np.arange(256, dtype=np.int64)
    arg = int(arg)
    if code == T.RA_INVERT:
        lut = 255 - i
    elif code == T.RA_POSTERIZE:
        lut = i & (~(2 ** (8 - arg) - 1) & 255)
    elif code == T.RA_SOLARIZE:
        lut = np.where(i < arg, i, 255 - i)
    elif code == T.RA_SOLARIZE_ADD:
        lut = np.where(i < 128, np.minimum(255, i + arg), i)
    else:
        raise ValueError(code)
    return lut.astype(np.uint8)


def autocontrast_table(h):
    """One channel's histogram -> the table of ImageOps.autocontrast(cutoff = 0)."""
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.clip((np.arange(256, dtype=np.float64) * scale + offset).astype(np.int64), 0, 255).astype(np.uint8)


def equalize_table_unclamped(h):
    """One channel's histogram -> the table of ImageOps.equalize before Pillow clamps it to 255 (None: the channel is left as it is)."""
    h = [int(v) for v in h]
    histo = [v for v in h if v]
    if len(histo) <= 1:
        return None
    step = (sum(histo) - histo[-1]) // 255
    if not step:
        return None
    lut, n = [], step // 2
    for i in range(256):
        lut.append(n // step)
        n += h[i]
    return np.asarray(lut, np.int64)


def _per_channel(img, table_of):
    out = np.empty_like(img)
    for c in range(3):
        out[..., c] = table_of(np.bincount(img[..., c].ravel(), minlength=256))[img[..., c]]
    return out


def autocontrast(img):
    return _per_channel(img, autocontrast_table)


def equalize(img):
    def table(h):
        lut = equalize_table_unclamped(h)
        return np.arange(256, dtype=np.uint8) if lut is None else np.minimum(lut, 255).astype(np.uint8)
    return _per_channel(img, table)


def smooth(img):
    """filter(ImageFilter.SMOOTH) (Filter.c ImagingFilter3x3): the border copied, inside the float32 sum 0.5 + row(y+1) + row(y) + row(y-1) with each
    row's three products added first, truncated."""
    f32 = np.float32
    k = (np.asarray([1, 1, 1, 1, 5, 1, 1, 1, 1], np.float64) / 13.0).astype(f32)
    v = img.astype(f32)
    H, W = img.shape[:2]
    acc = np.full((H - 2, W - 2, 3), f32(0.5), f32)
    for j, dy in enumerate((1, 0, -1)):
        r = v[1 + dy:H - 1 + dy]
        acc = acc + ((r[:, 0:W - 2] * k[3 * j] + r[:, 1:W - 1] * k[3 * j + 1]) + r[:, 2:W] * k[3 * j + 2])
    out = img.copy()
    out[1:-1, 1:-1] = np.where(acc <= 0, f32(0), np.where(acc >= 255, f32(255), acc)).astype(np.uint8)
    return out


def sharpness(img, f):
    return A.blend(smooth(img), img, f)


def color(img, f):
    return A.saturation(img, f)


ENHANCE = {T.RA_COLOR: color, T.RA_CONTRAST: A.contrast, T.RA_BRIGHTNESS: A.brightness, T.RA_SHARPNESS: sharpness}


def apply_op(img, op, fill=T.RA_FILL):
    """One operation slot (int32 [T.RA_OP_COLS]: code, argument, six float64 coefficients) on img uint8 [80, 80, 3]."""
    op = np.ascontiguousarray(np.asarray(op, np.int32))
    code, arg = int(op[T.RA_CODE]), op[T.RA_ARG]
    if code == T.RA_NONE:
        return img
    if code == T.RA_AFFINE:
        return affine(img, op[T.RA_COEF:T.RA_COEF + 12].view(np.float64), fill)
    if code in (T.RA_INVERT, T.RA_POSTERIZE, T.RA_SOLARIZE, T.RA_SOLARIZE_ADD):
        return point_table(code, arg)[img]
    if code == T.RA_AUTOCONTRAST:
        return autocontrast(img)
    if code == T.RA_EQUALIZE:
        return equalize(img)
    return ENHANCE[code](img, float(np.asarray([arg], np.int32).view(np.float32)[0]))


def apply_row(img, row, fill=T.RA_FILL):
    """The kernel's work on one listed image: the row's two operation slots in order."""
    row = np.asarray(row, np.int32)
    for s in range(T.RA_SLOTS):
        img = apply_op(img, row[s * T.RA_OP_COLS:(s + 1) * T.RA_OP_COLS], fill)
    return img


def rand_augment(views, slots, table, fill=T.RA_FILL):
    """views uint8 [B, 80, 80, 3] -> a copy with the listed images augmented (fsvit_image_rand_augment)."""
    out = np.array(views, copy=True)
    for k, b in enumerate(np.asarray(slots).tolist()):
        out[b] = apply_row(views[b], np.asarray(table)[k], fill)
    return out


def weak_views(data, idx, params, fill=T.RA_FILL):
    """The uint8 weak views of a batch from the params of DeviceStrongWeakPair / DeviceRandAugCrop (bicubic crop + flip, then RandAugment)."""
    views = np.stack([A.weak_view(data[i], params['boxes'][k].tolist(), bool(params['flips'][k])) for k, i in enumerate(idx)])
    if 'randaug' in params:
        views = rand_augment(views, np.asarray(params['randaug'][0]), np.asarray(params['randaug'][1]), fill)
    return views


def sources(size=80):
    """The test images, uint8 [size, size, 3]: noise; the noise of tests/test_gpu_strong_weak.py's source with its band of saturating 2-pixel stripes
    (bicubic overshoot past both clamps); a constant; a narrow histogram (the unclamped Equalize table passes 255); and all 255 but 100 dark pixels
    (Equalize's step is 0)."""
    rng = np.random.default_rng(7)
    s84 = rng.integers(0, 256, size=(84, 84, 3), dtype=np.uint8)
    s84[:, 30:60] = np.where((np.arange(30) // 2 % 2)[None, :, None] == 0, 255, 0)
    o = (84 - size) // 2
    noise = np.random.default_rng(17).integers(0, 256, size=(size, size, 3), dtype=np.uint8)
    bright = np.full((size * size, 3), 255, np.uint8)
    bright[::size * size // 100][:100] = np.random.default_rng(18).integers(0, 40, size=(100, 3), dtype=np.uint8)
    return {'noise': noise, 'stripes': np.ascontiguousarray(s84[:size, o:o + size]),
            'constant': np.broadcast_to(np.array([77, 130, 201], np.uint8), (size, size, 3)).copy(), 'narrow': noise // 3 + 40,
            'bright': bright.reshape(size, size, 3)}


def timm_op_pil(img, name, magnitude, negate, fill=T.RA_FILL, translate_pct=0.45):
    """timm's operation `name` (auto_augment.py: the NAME_TO_OP function on the LEVEL_TO_ARG value) at `magnitude` through the installed Pillow,
    with the reference's hparams (BICUBIC, img_mean fill)."""
    from PIL import Image, ImageEnhance, ImageOps
    im = Image.fromarray(img)
    sign, level = (-1.0 if negate else 1.0), magnitude / 10.0
    kw = dict(resample=Image.BICUBIC, fillcolor=tuple(fill))
    if name == 'AutoContrast':
        out = ImageOps.autocontrast(im)
    elif name == 'Equalize':
        out = ImageOps.equalize(im)
    elif name == 'Invert':
        out = ImageOps.invert(im)
    elif name == 'Rotate':
        out = im.rotate(sign * (level * 30.0), **kw)
    elif name == 'PosterizeIncreasing':
        bits = 4 - int(level * 4)
        out = im if bits >= 8 else ImageOps.posterize(im, bits)
    elif name == 'SolarizeIncreasing':
        thresh = 256 - int(level * 256)
        out = im.point([i if i < thresh else 255 - i for i in range(256)] * 3)
    elif name == 'SolarizeAdd':
        add = min(128, int(level * 110))
        out = im.point([min(255, i + add) if i < 128 else i for i in range(256)] * 3)
    elif name in ('ColorIncreasing', 'ContrastIncreasing', 'BrightnessIncreasing', 'SharpnessIncreasing'):
        out = getattr(ImageEnhance, name[:-len('Increasing')])(im).enhance(max(0.1, 1.0 + sign * (level * 0.9)))
    elif name == 'ShearX':
        out = im.transform(im.size, Image.AFFINE, (1, sign * (level * 0.3), 0, 0, 1, 0), **kw)
    elif name == 'ShearY':
        out = im.transform(im.size, Image.AFFINE, (1, 0, 0, sign * (level * 0.3), 1, 0), **kw)
    elif name == 'TranslateXRel':
        out = im.transform(im.size, Image.AFFINE, (1, 0, sign * (level * translate_pct) * im.size[0], 0, 1, 0), **kw)
    elif name == 'TranslateYRel':
        out = im.transform(im.size, Image.AFFINE, (1, 0, 0, 0, 1, sign * (level * translate_pct) * im.size[1]), **kw)
    else:
        raise ValueError(name)
    return np.asarray(out)
