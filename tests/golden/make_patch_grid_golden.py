#!/usr/bin/env python3
"""Generate tests/golden/patch_grid_pil.npz: the SUN-D grid patch loader's boxes as the REFERENCE computes them and its patches as Pillow makes them
(build container only: needs /root/reference, read-only, and Pillow; never runs on the GPU box).

Run from the repo root:  python tests/golden/make_patch_grid_golden.py

  loc_case  int32 [n, 2]  (size, num_grid)       loc_ratio float64 [n]      loc_out int32 [n, 3, 2]  (lo, hi) of every cell, rows past num_grid = -1
      recorded by calling the reference's own MiniImageNet.get_grid_location (meta_tuning_sun_d/Models/dataloader/miniimagenet/grid/
      mini_imagenet.py:78-97) unbound; torchvision, which that file imports and this call does not use, is stubbed in sys.modules
  eval_source / eval_box [13, 4] (top, left, height, width) / eval_out uint8 [13, 80, 80, 3]
      the 13 val / test patches (patch_list 2,3, patch_ratio 2) of one 84 x 84 source of transform_pil.npz: crop -> resize((80, 80), BILINEAR)
  train_source (0: image 1 of transform_pil.npz, 1: src60x100 of transform_rrc_pil.npz) / train_level / train_ratio / train_cell (row, col) /
  train_box / train_flip / train_out uint8 [8, 80, 80, 3]
      8 train patches: crop -> resize -> FLIP_LEFT_RIGHT where train_flip is set
"""
import importlib.util
import os
import sys
import types

import numpy as np
import PIL
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF_FILE = '/root/reference/meta_tuning_sun_d/Models/dataloader/miniimagenet/grid/mini_imagenet.py'
OUT = os.path.join(REPO, 'tests', 'golden')

SIZES, GRIDS, RATIOS = (84, 60, 100), (2, 3), (2, 1.0, 1.37, 2.5, 2.999, 2.9999999)
EVAL_SOURCE = 0
# (source, level, ratio, (row, col), flip)
TRAIN = [(0, 2, 2, (0, 1), 1), (0, 3, 1.0, (1, 1), 0), (0, 2, 1.37, (1, 0), 1), (0, 3, 2.5, (2, 0), 1),
         (1, 2, 2.999, (1, 1), 0), (1, 3, 2.9999999, (0, 2), 1), (1, 2, 1.37, (0, 0), 0), (1, 3, 2.5, (1, 2), 1)]


def reference_get_grid_location():
    tv = types.ModuleType('torchvision')
    tv.transforms = types.ModuleType('torchvision.transforms')
    sys.modules.setdefault('torchvision', tv)
    sys.modules.setdefault('torchvision.transforms', tv.transforms)
    spec = importlib.util.spec_from_file_location('sund_grid_mini_imagenet', REF_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return lambda size, ratio, num_grid: mod.MiniImageNet.get_grid_location(None, size, ratio, num_grid)


def patch(img, box, flip):
    top, left, h, w = box
    p = Image.fromarray(img).crop((left, top, left + w, top + h)).resize((80, 80), Image.BILINEAR)
    if flip:
        p = p.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(p)


def main():
    loc = reference_get_grid_location()
    loc_case, loc_ratio, loc_out = [], [], []
    for size in SIZES:
        for n in GRIDS:
            for r in RATIOS:
                cells = loc(size, r, n)
                loc_case.append((size, n))
                loc_ratio.append(float(r))
                loc_out.append(list(cells) + [(-1, -1)] * (3 - n))

    def boxes(H, W, ratio, n):
        cols, rows = loc(W, ratio, n), loc(H, ratio, n)
        return [[(t, l, b - t, r - l) for l, r in cols] for t, b in rows]

    images = np.load(os.path.join(OUT, 'transform_pil.npz'))['images']
    sources = [images[1], np.load(os.path.join(OUT, 'transform_rrc_pil.npz'))['src60x100']]
    src = images[EVAL_SOURCE]
    eval_box = [b for n in (2, 3) for row in boxes(84, 84, 2, n) for b in row]
    eval_out = [patch(src, b, 0) for b in eval_box]
    train_box = [boxes(*sources[s].shape[:2], ratio, level)[cell[0]][cell[1]] for s, level, ratio, cell, _ in TRAIN]
    train_out = [patch(sources[s], b, flip) for (s, _, _, _, flip), b in zip(TRAIN, train_box)]
    path = os.path.join(OUT, 'patch_grid_pil.npz')
    np.savez_compressed(
        path, loc_case=np.array(loc_case, np.int32), loc_ratio=np.array(loc_ratio, np.float64), loc_out=np.array(loc_out, np.int32),
        eval_source=np.int32(EVAL_SOURCE), eval_box=np.array(eval_box, np.int32), eval_out=np.stack(eval_out),
        train_source=np.array([t[0] for t in TRAIN], np.int32), train_level=np.array([t[1] for t in TRAIN], np.int32),
        train_ratio=np.array([t[2] for t in TRAIN], np.float64), train_cell=np.array([t[3] for t in TRAIN], np.int32),
        train_box=np.array(train_box, np.int32), train_flip=np.array([t[4] for t in TRAIN], np.uint8), train_out=np.stack(train_out),
        pillow_version=np.array(PIL.__version__))
    print(path, os.path.getsize(path), 'bytes;', len(loc_case), 'location cases, 13 eval patches,', len(TRAIN), 'train patches')


if __name__ == '__main__':
    main()
