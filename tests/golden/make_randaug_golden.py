"""Writes tests/golden/randaug_pil.npz: RandAugment operations computed by the installed Pillow (run once, by hand; tests/test_randaug_cpu.py
compares tests/randaug_ref.py with it, so the restatement stays pinned where Pillow is not installed).  One output per operation of timm's
'increasing' set at magnitude 9, both signs for the signed ones, and four two-operation chains, on two 56 x 56 sources (noise, and the
saturating stripes): 56 pixels keep the file under 512 KB, and the restatement is the same code at every size.

  python tests/golden/make_randaug_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import randaug_ref as R                                                 # noqa: E402
from fewshot_vit_amd.datasets import transforms as T                    # noqa: E402

SIZE = 56
CHAINS = [(('Rotate', 4.3, True), ('Equalize', 9.0, False)), (('SharpnessIncreasing', 10.0, False), ('ShearX', 9.0, False)),
          (('AutoContrast', 9.0, False), ('TranslateYRel', 4.3, True)), (('SolarizeAdd', 9.0, False), ('ContrastIncreasing', 9.37, True))]


def cases():
    out = []
    for name in T.RAND_INCREASING_OPS:
        out += [((name, 9.0, neg),) for neg in ((False, True) if name in T.RA_SIGNED else (False,))]
    return out + CHAINS


def main():
    import PIL
    src = R.sources(SIZE)
    names = ('noise', 'stripes')
    all_cases = cases()
    outputs = np.empty((len(names), len(all_cases), SIZE, SIZE, 3), np.uint8)
    for s, key in enumerate(names):
        for k, chain in enumerate(all_cases):
            img = src[key]
            for name, m, neg in chain:
                img = R.timm_op_pil(img, name, m, neg)
            outputs[s, k] = img
    pad = lambda chain: list(chain) + [('', 0.0, False)] * (2 - len(chain))
    np.savez_compressed(os.path.join(HERE, 'randaug_pil.npz'), sources=np.stack([src[k] for k in names]), outputs=outputs,
                        case_op=np.array([[T.RAND_INCREASING_OPS.index(n) if n else -1 for n, _, _ in pad(c)] for c in all_cases], np.int32),
                        case_magnitude=np.array([[m for _, m, _ in pad(c)] for c in all_cases], np.float64),
                        case_negate=np.array([[g for _, _, g in pad(c)] for c in all_cases], np.uint8), pillow=np.array(PIL.__version__))
    print(len(all_cases), 'cases,', os.path.getsize(os.path.join(HERE, 'randaug_pil.npz')), 'bytes')


if __name__ == '__main__':
    main()
