"""Write tests/golden/coco_pair_pillow.npz: what Pillow gives on the cases of tests/test_coco_pair.py -- the COCO pre-training
mapper's chain flip -> resize -> crop -> resize, by literal calls: `np.flip`, `Image.resize(BILINEAR)`,
slicing, `Image.resize(BILINEAR)`.

Run on the CPU, where Pillow is installed (`python tools/make_golden_coco_pair.py`); the tests read the file and import Pillow
only where it is there.  Everything is regenerated from fixed seeds, so a rerun with the same Pillow rewrites the same bytes.
  sources: `src<k>` uint8 [h, w, 3];
  cases:   `c<i>_src` the index k of the case's source, `c<i>_plan` int32 {h1, w1, x0, y0, cw, ch, nh, nw} (the window inside
           the FLIPPED and resized h1 x w1 image), and for flip f in {0, 1}: `c<i>_mid<f>` uint8 [ch, cw, 3], the window after
           the first resample, `c<i>_out<f>` uint8 [nh, nw, 3], the chain's result.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "coco_pair_pillow.npz")

SOURCES = [(37, 53), (40, 50), (33, 47), (90, 120)]
# source index, (h1, w1), window (x0, y0, cw, ch), target (nh, nw): tests/test_coco_pair.py says what each is for
CASES = [
    (0, (45, 64), (5, 3, 41, 35), (33, 39)),
    (0, (45, 64), (23, 10, 41, 35), (20, 30)),
    (0, (45, 64), (17, 9, 1, 1), (2, 3)),
    (1, (52, 50), (4, 6, 40, 33), (33, 29)),
    (2, (70, 100), (10, 8, 77, 55), (21, 30)),
    (3, (41, 55), (3, 2, 40, 30), (52, 70)),
    (0, (37, 53), (0, 0, 53, 37), (30, 43)),
    (3, (90, 120), (30, 20, 64, 48), (40, 53)),
]


def main():
    import PIL
    from PIL import Image

    arrays = {"pillow_version": np.array(PIL.__version__)}
    srcs = [np.random.default_rng(500 + k).integers(0, 256, (h, w, 3), dtype=np.uint8) for k, (h, w) in enumerate(SOURCES)]
    for k, a in enumerate(srcs):
        arrays["src%d" % k] = a
    for i, (k, (h1, w1), (x0, y0, cw, ch), (nh, nw)) in enumerate(CASES):
        arrays["c%d_src" % i] = np.array(k, dtype=np.int32)
        arrays["c%d_plan" % i] = np.array([h1, w1, x0, y0, cw, ch, nh, nw], dtype=np.int32)
        for flip in (0, 1):
            a = np.ascontiguousarray(np.flip(srcs[k], axis=1)) if flip else srcs[k]
            big = np.asarray(Image.fromarray(a).resize((w1, h1), Image.BILINEAR))
            mid = np.ascontiguousarray(big[y0:y0 + ch, x0:x0 + cw])
            arrays["c%d_mid%d" % (i, flip)] = mid
            arrays["c%d_out%d" % (i, flip)] = np.asarray(Image.fromarray(mid).resize((nw, nh), Image.BILINEAR))
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    print("%s: %d sources, %d cases, Pillow %s, %d bytes" % (OUT, len(SOURCES), len(CASES), PIL.__version__, size))
    assert size < 300 * 1024
    return 0


if __name__ == "__main__":
    sys.exit(main())
