#!/usr/bin/env python3
"""Golden vectors of the train-time augmentation `augment: resize`, produced by Pillow itself: torchvision's RandomResizedCrop(80) on a PIL image is
`img.crop((j, i, j + w, i + h)).resize((80, 80), BILINEAR)` and RandomHorizontalFlip is `transpose(FLIP_LEFT_RIGHT)` (torchvision is not installed
here, Pillow is).  The boxes are fixed edge cases, not drawn.
    python tests/golden/make_transform_rrc_golden.py   ->  tests/golden/transform_rrc_pil.npz
Sources: the four 84 x 84 `images` of transform_pil.npz (source 0..3, not stored again), one 32 x 32 image (source 4) and one 60 x 100 image (source 5)."""
import os

import numpy as np
from PIL import Image

OUT = os.path.dirname(os.path.abspath(__file__))
SIZE = 80

# (source, (top i, left j, height h, width w), flip)
CASES = [
    (0, (0, 0, 84, 84), 0),          # the whole image
    (1, (0, 0, 84, 84), 1),          # ... flipped (smooth ramp: the mirror is visible in every row)
    (0, (2, 3, 50, 80), 0),          # w == 80: identity horizontal pass
    (1, (30, 4, 33, 80), 1),
    (3, (4, 10, 80, 40), 1),         # h == 80: identity vertical pass
    (0, (83, 83, 1, 1), 0),          # 1 x 1 box at the last row and column
    (2, (0, 41, 84, 1), 1),          # one-column strip
    (3, (30, 50, 21, 27), 0),        # minimum-area box (0.08 * 84 * 84 = 564.5 <= 21 * 27)
    (2, (10, 20, 36, 48), 1),        # w = 48 (saturating stripes)
    (0, (5, 6, 60, 72), 0),          # w = 72
    (5, (0, 2, 60, 96), 1),          # w = 96: 5-tap downscale, scale 1.2
    (5, (3, 0, 50, 100), 0),         # w = 100: scale 1.25
    (5, (0, 0, 60, 100), 1),         # the whole 60 x 100 image
    (5, (59, 99, 1, 1), 1),
    (4, (20, 5, 8, 10), 1),          # 8 x 10 box on the 32 x 32 source
    (4, (0, 0, 32, 32), 0),
]


def main():
    import PIL
    base = np.load(os.path.join(OUT, 'transform_pil.npz'))['images']
    rng = np.random.default_rng(2025)
    src32 = rng.integers(0, 256, size=(32, 32, 3), dtype=np.uint8)
    src60x100 = rng.integers(0, 256, size=(60, 100, 3), dtype=np.uint8)
    sources = list(base) + [src32, src60x100]
    outs = []
    for s, (i, j, h, w), flip in CASES:
        im = Image.fromarray(sources[s]).crop((j, i, j + w, i + h)).resize((SIZE, SIZE), Image.BILINEAR)
        if flip:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        outs.append(np.asarray(im))
    out = {'src32': src32, 'src60x100': src60x100,
           'case_source': np.array([c[0] for c in CASES], np.int32), 'case_box': np.array([c[1] for c in CASES], np.int32),
           'case_flip': np.array([c[2] for c in CASES], np.uint8), 'out': np.stack(outs), 'pillow_version': np.array(PIL.__version__)}
    path = os.path.join(OUT, 'transform_rrc_pil.npz')
    np.savez_compressed(path, **out)
    print('wrote transform_rrc_pil.npz', os.path.getsize(path), 'bytes', {k: getattr(v, 'shape', None) for k, v in out.items()})


if __name__ == '__main__':
    main()
