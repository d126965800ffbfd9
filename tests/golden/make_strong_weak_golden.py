#!/usr/bin/env python3
"""Golden vectors of the distillation phase's strong / weak view pair (sun_meta_training/datasets/mini_imagenet.py:91-124), produced by Pillow itself:
weak = `img.crop(box).resize((80, 80), BICUBIC)` (+ `transpose(FLIP_LEFT_RIGHT)`), strong = ImageEnhance.Brightness / Contrast / Color in the case's
order -> ImageFilter.GaussianBlur -> ImageOps.solarize -> convert('L') on three channels, each step only where the case asks for it (what
torchvision's ColorJitter / RandomGrayscale and the reference's GaussianBlur / Solarization do to a PIL image).  Fixed cases, nothing drawn.
    python tests/golden/make_strong_weak_golden.py   ->  tests/golden/strong_weak_pil.npz
Sources: the four 84 x 84 `images` of transform_pil.npz (not stored again); 1 and 2 are structured (a ramp, saturating stripes), 0 and 3 noise."""
import os

import numpy as np
from PIL import Image, ImageEnhance, ImageFilter, ImageOps

OUT = os.path.dirname(os.path.abspath(__file__))
SIZE = 80
ENHANCE = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)          # operation codes 0, 1, 2

# (source, (top, left, height, width), flip, order, (brightness, contrast, saturation), blur radius or 0, solarize, gray)
CASES = [
    (1, (0, 0, 84, 84), 0, (0, 1, 2), (1.0, 1.0, 1.0), 0.0, 0, 0),            # every factor 1: strong == weak
    (1, (3, 5, 70, 60), 1, (0, 1, 2), (0.6, 1.4, 0.6), 0.0, 0, 0),
    (2, (10, 20, 36, 48), 0, (2, 1, 0), (1.4, 0.6, 1.4), 0.0, 0, 0),          # saturating stripes: bicubic overshoot clipped, clamped blends
    (2, (0, 0, 84, 84), 1, (1, 0, 2), (0.8125, 1.1875, 0.9375), 0.1, 0, 0),   # smallest radius: box radius 0
    (1, (20, 0, 30, 84), 0, (1, 2, 0), (1.25, 0.75, 1.0), 1.4142134, 1, 0),   # just below the box-radius step
    (2, (40, 40, 44, 44), 1, (2, 0, 1), (1.0, 1.0, 0.6), 1.4142135, 0, 1),    # just above it
    (1, (0, 42, 84, 21), 1, (0, 2, 1), (1.4, 1.4, 1.4), 2.0, 1, 1),           # everything on, largest radius
    (2, (83, 83, 1, 1), 0, (0, 1, 2), (0.6, 0.6, 0.6), 0.58, 1, 0),           # 1 x 1 box: a uniform view
    (0, (0, 0, 84, 84), 0, (1, 0, 2), (0.7, 1.3, 1.1), 1.0, 0, 0),            # noise sources
    (3, (30, 50, 21, 27), 1, (2, 1, 0), (1.3, 0.7, 0.9), 0.0, 1, 1),
    (0, (5, 6, 60, 72), 1, (0, 2, 1), (0.9, 1.1, 1.3), 1.7, 1, 0),
    (1, (0, 0, 84, 84), 0, (0, 1, 2), (1.0, 1.0, 1.0), 0.0, 0, 1),            # grayscale alone
]


def views(img, box, flip, order, factors, radius, solarize, gray):
    i, j, h, w = box
    im = Image.fromarray(img).crop((j, i, j + w, i + h)).resize((SIZE, SIZE), Image.BICUBIC)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    weak = np.asarray(im)
    for op in order:
        im = ENHANCE[op](im).enhance(factors[op])
    if radius:
        im = im.filter(ImageFilter.GaussianBlur(radius))
    if solarize:
        im = ImageOps.solarize(im)
    if gray:
        L = np.asarray(im.convert('L'))
        im = Image.fromarray(np.dstack([L, L, L]))
    return weak, np.asarray(im)


def main():
    import PIL
    base = np.load(os.path.join(OUT, 'transform_pil.npz'))['images']
    pairs = [views(base[c[0]], *c[1:]) for c in CASES]
    out = {'case_source': np.array([c[0] for c in CASES], np.int32), 'case_box': np.array([c[1] for c in CASES], np.int32),
           'case_flip': np.array([c[2] for c in CASES], np.uint8), 'case_order': np.array([c[3] for c in CASES], np.int32),
           'case_factors': np.array([c[4] for c in CASES], np.float32), 'case_radius': np.array([c[5] for c in CASES], np.float32),
           'case_solarize': np.array([c[6] for c in CASES], np.uint8), 'case_gray': np.array([c[7] for c in CASES], np.uint8),
           'weak': np.stack([p[0] for p in pairs]), 'strong': np.stack([p[1] for p in pairs]), 'pillow_version': np.array(PIL.__version__)}
    path = os.path.join(OUT, 'strong_weak_pil.npz')
    np.savez_compressed(path, **out)
    print('wrote strong_weak_pil.npz', os.path.getsize(path), 'bytes', {k: getattr(v, 'shape', None) for k, v in out.items()})


if __name__ == '__main__':
    main()
