"""Write tests/golden/resize_pillow.npz: what Pillow's bilinear resize gives on the cases of tests/test_resize.py.

Run on the CPU, where Pillow is installed (`python tools/make_golden_resize.py`); the GPU tests read the file and never
import Pillow.  Per case `<name>_src` (uint8 [h, w, 3], the source) and `<name>_out` (uint8 [nh, nw, 3],
`Image.fromarray(src).resize((nw, nh), Image.BILINEAR)`), plus `pillow_version`.  The sources are regenerated from fixed
seeds, so a rerun with the same Pillow rewrites the same bytes.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "resize_pillow.npz")

# (source h, w) -> (target h, w): each the smallest shape that reaches its branch (tests/test_resize.py says which)
CASES = [((37, 53), (19, 27)), ((48, 64), (24, 32)), ((45, 63), (15, 21)), ((19, 27), (37, 53)), ((40, 56), (40, 28)),
         ((40, 56), (20, 56)), ((33, 47), (33, 47)), ((130, 70), (17, 9)), ((150, 260), (75, 130))]
EXTREMES = [((37, 53), (19, 27)), ((48, 64), (24, 32))]      # also as a 0/255 checkerboard and as an all-255 frame


def case_name(src, dst, content="random"):
    return "%dx%d_%dx%d_%s" % (src + dst + (content,))


def source(src, content, seed):
    h, w = src
    if content == "random":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if content == "checker":
        yy, xx = np.mgrid[:h, :w]
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    return np.full((h, w, 3), 255, dtype=np.uint8)


def all_cases():
    out = [(s, d, "random") for s, d in CASES]
    out += [(s, d, c) for s, d in EXTREMES for c in ("checker", "white")]
    return out


def main():
    import PIL
    from PIL import Image
    arrays = {"pillow_version": np.array(PIL.__version__)}
    for i, (src, dst, content) in enumerate(all_cases()):
        a = source(src, content, 100 + i)
        arrays[case_name(src, dst, content) + "_src"] = a
        arrays[case_name(src, dst, content) + "_out"] = np.asarray(Image.fromarray(a).resize((dst[1], dst[0]), Image.BILINEAR))
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    print("%s: %d cases, Pillow %s, %d bytes" % (OUT, len(arrays) // 2, PIL.__version__, size))
    assert size < 256 * 1024
    return 0


if __name__ == "__main__":
    sys.exit(main())
