"""TEST HELPER (a plain module, imported by tests/test_strong_weak_cpu.py and tests/test_gpu_strong_weak.py): numpy restatement of the Pillow
operations behind the distillation phase's strong / weak view pair (sun_meta_training/datasets/mini_imagenet.py:91-124, :194-204) -
`Image.resize(BICUBIC)` on the tables of datasets/transforms.py:pil_resample_tables, `convert('L')`, `ImageEnhance.Brightness / Contrast / Color`,
`ImageFilter.GaussianBlur`, `ImageOps.solarize` - and of the whole pair as the kernels compute it from a parameter row.  Pinned bit for bit against
Pillow itself and against tests/golden/strong_weak_pil.npz by tests/test_strong_weak_cpu.py."""
import numpy as np

from fewshot_vit_amd.datasets import transforms as T

PB = T.PRECISION_BITS


def _pass(img, xmin, cnt, coef, axis):
    """One 8-bit resampling pass along `axis` of img [H, W, C] uint8 (ImagingResampleHorizontal / Vertical_8bpc)."""
    img = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(xmin),) + img.shape[1:], np.uint8)
    for o in range(len(xmin)):
        acc = np.full(img.shape[1:], 1 << (PB - 1), np.int64)
        for k in range(cnt[o]):
            acc += img[xmin[o] + k] * int(coef[o, k])
        out[o] = np.clip(acc >> PB, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def pil_resize(img, out_h, out_w, filter='bicubic'):
    """img [H, W, 3] uint8 -> [out_h, out_w, 3] uint8 == np.asarray(Image.fromarray(img).resize((out_w, out_h), BICUBIC / BILINEAR))."""
    h, w = img.shape[:2]
    if w != out_w:                                    # horizontal pass first (Resample.c ImagingResample)
        img = _pass(img, *T.pil_resample_tables(w, out_w, filter), axis=1)
    if h != out_h:
        img = _pass(img, *T.pil_resample_tables(h, out_h, filter), axis=0)
    return img


def weak_view(img, box, flip, size=80, filter='bicubic'):
    i, j, h, w = (int(v) for v in box)
    r = pil_resize(img[i:i + h, j:j + w], size, size, filter)
    return np.ascontiguousarray(r[:, ::-1] if flip else r)


def luma(img):
    """convert('L'): Convert.c L24."""
    v = img.astype(np.int64)
    return ((v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(deg, img, alpha):
    """Image.blend(degenerate, image, alpha) (Blend.c): fp32 multiply, fp32 add, truncation; clamped first when alpha is outside [0, 1]."""
    a = np.float32(alpha)
    d = np.broadcast_to(np.asarray(deg), img.shape).astype(np.int32)
    t = d.astype(np.float32) + a * (img.astype(np.int32) - d).astype(np.float32)
    if not (np.float32(0) <= a <= np.float32(1)):
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.int32).astype(np.uint8)


def brightness(img, f):
    return blend(0, img, f)


def contrast(img, f):
    L = luma(img)
    return blend(int(int(L.astype(np.int64).sum()) / float(L.size) + 0.5), img, f)


def saturation(img, f):
    return blend(luma(img)[..., None], img, f)


COLOUR_OPS = (brightness, contrast, saturation)          # indexed by T.OP_*


def _box_pass(img, r, ww, fw, axis):
    v = np.moveaxis(img, axis, 0).astype(np.uint64)
    n = v.shape[0]
    idx = np.arange(n)
    acc = np.zeros_like(v)
    for k in range(-r, r + 1):
        acc += v[np.clip(idx + k, 0, n - 1)]
    far = v[np.clip(idx - r - 1, 0, n - 1)] + v[np.clip(idx + r + 1, 0, n - 1)]
    out = (acc * np.uint64(ww) + far * np.uint64(fw) + np.uint64(1 << 23)) >> np.uint64(24)
    assert int(out.max()) <= 255
    return np.moveaxis(out.astype(np.uint8), 0, axis)


def box_blur(img, r, ww, fw):
    """BoxBlur.c ImagingBoxBlur(n = 3): three passes along x, then three along y."""
    for axis in (1, 1, 1, 0, 0, 0):
        img = _box_pass(img, int(r), int(ww), int(fw), axis)
    return img


def gaussian_blur(img, radius):
    r, ww, fw = T.gaussian_blur_box(radius)
    return box_blur(img, r, ww, fw)


def solarize(img):
    return np.where(img < 128, img, 255 - img).astype(np.uint8)


def grayscale(img):
    return np.repeat(luma(img)[..., None], 3, axis=2)


def normalise(u8, mean=T.IMAGENET_MEAN, std=T.IMAGENET_STD):
    """uint8 [H, W, 3] -> float32 [3, H, W]: ToTensor + Normalize, two correctly rounded fp32 operations after the division by 255."""
    t = u8.astype(np.float32) / np.float32(255)
    return np.ascontiguousarray(((t - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)).transpose(2, 0, 1))


def strong_u8(view, row):
    """The strong view's bytes from the weak view's and one parameter row (int32 [T.SW_COLS])."""
    row = np.asarray(row, np.int32)
    if not row[T.SW_STRONG]:
        return view
    out = view
    factors = row[T.SW_FACTOR:T.SW_FACTOR + 3].view(np.float32)
    for op in row[T.SW_ORDER:T.SW_ORDER + 3]:
        out = COLOUR_OPS[int(op)](out, factors[int(op)])
    if row[T.SW_BLUR]:
        out = box_blur(out, row[T.SW_R], row[T.SW_WW], row[T.SW_FW])
    if row[T.SW_SOLARIZE]:
        out = solarize(out)
    if row[T.SW_GRAY]:
        out = grayscale(out)
    return out


def erase_mask(row, size=80):
    top, left, h, w = (int(v) for v in np.asarray(row)[T.SW_ERASE:T.SW_ERASE + 4])
    m = np.zeros((size, size), bool)
    m[top:top + h, left:left + w] = h > 0
    return m


def pair(view, row, mean=T.IMAGENET_MEAN, std=T.IMAGENET_STD):
    """-> (strong, weak) float32 [3, 80, 80] as the kernel stores them, and the erase mask [80, 80] inside which strong is noise."""
    return normalise(strong_u8(view, row), mean, std), normalise(view, mean, std), erase_mask(row, view.shape[0])


def make_row(strong=1, order=(0, 1, 2), factors=(1.0, 1.0, 1.0), radius=None, solarize=0, gray=0, erase=(0, 0, 0, 0)):
    """A parameter row from readable values (radius None = no blur)."""
    row = np.zeros(T.SW_COLS, np.int32)
    row[T.SW_STRONG] = strong
    row[T.SW_ORDER:T.SW_ORDER + 3] = order
    row[T.SW_FACTOR:T.SW_FACTOR + 3] = np.asarray(factors, np.float32).view(np.int32)
    r, ww, fw = T.gaussian_blur_box(0.1 if radius is None else radius)
    row[T.SW_BLUR], row[T.SW_R], row[T.SW_WW], row[T.SW_FW] = radius is not None, r, ww, fw
    row[T.SW_SOLARIZE], row[T.SW_GRAY] = solarize, gray
    row[T.SW_ERASE:T.SW_ERASE + 4] = erase
    return row
