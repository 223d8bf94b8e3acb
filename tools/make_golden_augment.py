"""Write tests/golden/augment_pillow.npz: what Pillow gives on the cases of tests/test_augment.py -- the reference mapper's
crop + `resize(BILINEAR)` of frames, crop + `resize(NEAREST)` of mode-L masks (as detectron2 passes them), and the NEAREST
source-index ramps of every (720 | 1280 -> config size) pair and a few dozen odd pairs.

Run on the CPU, where Pillow is installed (`python tools/make_golden_augment.py`); the tests read the file and never import
Pillow.  Everything is regenerated from fixed seeds, so a rerun with the same Pillow rewrites the same bytes.
  frames: `f<i>_src` uint8 [h, w, 3], `f<i>_plan` int32 {x0, y0, cw, ch, nh, nw}, `f<i>_out` uint8 [nh, nw, 3] (not flipped: the
          flip is `np.flip(axis=1)` of it, as the reference flips);
  masks:  `m<i>_size` {h, w}, `m<i>_plan`, `m<i>_counts` int32 (COCO counts of the source mask, column-major, zeros first),
          `m<i>_out` uint8 [nh, nw];
  ramps:  `ramp_pairs` int32 [k, 2] = (n_in, n_out), `ramp_starts` int32 [k + 1], `ramp_data` int32: the source index Pillow's
          NEAREST resize reads for every output index (a ramp image resized: low and high byte in two mode-L images).
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "augment_pillow.npz")

# (source h, w), window (x0, y0, cw, ch), target (nh, nw): tests/test_train_augment_gpu.py says what each is for
FRAME_CASES = [
    ((45, 70), (3, 5, 37, 29), (50, 64)),
    ((45, 70), (3, 5, 63, 29), (50, 33)),
    ((140, 100), (3, 2, 88, 136), (17, 11)),      # 8x: the limit (the GPU tests' 300 x 280 source would fill the file)
    ((40, 70), (2, 1, 64, 36), (18, 32)),
    ((40, 50), (5, 3, 40, 30), (15, 40)),
    ((37, 53), (12, 14, 41, 23), (20, 30)),
    ((33, 47), (0, 0, 47, 33), (20, 29)),
]
TRAIN_SHORT = (320, 352, 392, 416, 448, 480, 512, 544, 576, 608, 640, 672, 704, 736, 768, 800)
TRAIN_MAX = (768, 1333)


def config_pairs():
    from vnext_amd.ops.resize import shortest_edge_size
    pairs = set()
    for short in TRAIN_SHORT:
        for max_size in TRAIN_MAX:
            for h, w in ((720, 1280), (1280, 720)):
                nh, nw = shortest_edge_size(h, w, short, max_size)
                pairs |= {(h, nh), (w, nw)}
    return sorted(pairs)


def odd_pairs():
    rng = np.random.default_rng(77)
    pairs = {(37, 64), (29, 50), (272, 34), (264, 33), (33, 27), (35, 21), (1, 1), (1, 9), (9, 1), (600, 384), (384, 600),
             (437, 333), (599, 640), (1280, 7)}
    while len(pairs) < 48:
        pairs.add((int(rng.integers(1, 700)), int(rng.integers(1, 700))))
    return sorted(pairs)


def blob(h, w, seed):
    """a few random rectangles and a diagonal band"""
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), dtype=np.uint8)
    for _ in range(3):
        y, x = int(rng.integers(0, h - 2)), int(rng.integers(0, w - 2))
        m[y:y + int(rng.integers(2, h // 2 + 2)), x:x + int(rng.integers(2, w // 2 + 2))] ^= 1
    yy, xx = np.mgrid[:h, :w]
    m[(yy + 2 * xx) % 17 == 0] ^= 1
    return m


def mask_cases():
    """(h, w), window, target, dense source mask"""
    out = []
    size, win, dst = (45, 70), (3, 5, 37, 29), (50, 64)
    h, w = size
    x0, y0, cw, ch = win
    empty = np.zeros(size, dtype=np.uint8)
    corner = empty.copy()
    corner[y0 + ch - 1, x0 + cw - 1] = 1
    outside = empty.copy()
    outside[36:44, 45:69] = 1
    outside[0:4, 0:2] = 1
    flat = np.zeros(h * w, dtype=np.uint8)
    flat[10 * h + 7:16 * h + 20] = 1               # one run over columns 10 .. 16
    run = flat.reshape((h, w), order="F").copy()
    for m in (empty, np.ones(size, dtype=np.uint8), corner, outside, run, blob(h, w, 5), blob(h, w, 6)):
        out.append((size, win, dst, m))
    yy, xx = np.mgrid[:40, :40]
    out.append(((40, 40), (4, 2, 33, 35), (21, 27), ((yy + xx) & 1).astype(np.uint8)))
    out.append(((40, 40), (0, 0, 40, 40), (40, 40), ((yy + xx) & 1).astype(np.uint8)))
    out.append(((300, 280), (7, 11, 264, 272), (34, 33), blob(300, 280, 7)))
    out.append(((45, 70), (3, 5, 63, 29), (50, 33), blob(45, 70, 8)))
    return out


def main():
    import PIL
    from PIL import Image

    from vnext_amd.utils.ytvis_json import rle_counts
    arrays = {"pillow_version": np.array(PIL.__version__)}
    for i, ((h, w), (x0, y0, cw, ch), (nh, nw)) in enumerate(FRAME_CASES):
        a = np.random.default_rng(300 + i).integers(0, 256, (h, w, 3), dtype=np.uint8)
        arrays["f%d_src" % i] = a
        arrays["f%d_plan" % i] = np.array([x0, y0, cw, ch, nh, nw], dtype=np.int32)
        arrays["f%d_out" % i] = np.asarray(Image.fromarray(a[y0:y0 + ch, x0:x0 + cw]).resize((nw, nh), Image.BILINEAR))
    for i, ((h, w), (x0, y0, cw, ch), (nh, nw), m) in enumerate(mask_cases()):
        arrays["m%d_size" % i] = np.array([h, w], dtype=np.int32)
        arrays["m%d_plan" % i] = np.array([x0, y0, cw, ch, nh, nw], dtype=np.int32)
        arrays["m%d_counts" % i] = np.asarray(rle_counts(m), dtype=np.int32)
        crop = np.ascontiguousarray(m[y0:y0 + ch, x0:x0 + cw])
        arrays["m%d_out" % i] = np.asarray(Image.fromarray(crop, mode="L").resize((nw, nh), Image.NEAREST))
    pairs = sorted(set(config_pairs()) | set(odd_pairs()))
    data, starts = [], [0]
    for n_in, n_out in pairs:
        ramp = np.arange(n_in, dtype=np.int32)[None, :]
        lo = np.asarray(Image.fromarray((ramp & 255).astype(np.uint8), mode="L").resize((n_out, 1), Image.NEAREST))
        hi = np.asarray(Image.fromarray((ramp >> 8).astype(np.uint8), mode="L").resize((n_out, 1), Image.NEAREST))
        col = np.arange(n_in, dtype=np.int32)[:, None]      # the vertical axis takes the same path: check it agrees
        lo_v = np.asarray(Image.fromarray((col & 255).astype(np.uint8), mode="L").resize((1, n_out), Image.NEAREST))
        hi_v = np.asarray(Image.fromarray((col >> 8).astype(np.uint8), mode="L").resize((1, n_out), Image.NEAREST))
        tab = lo[0].astype(np.int32) + 256 * hi[0].astype(np.int32)
        assert np.array_equal(tab, lo_v[:, 0].astype(np.int32) + 256 * hi_v[:, 0].astype(np.int32)), (n_in, n_out)
        data.append(tab)
        starts.append(starts[-1] + n_out)
    arrays["ramp_pairs"] = np.array(pairs, dtype=np.int32)
    arrays["ramp_starts"] = np.array(starts, dtype=np.int32)
    arrays["ramp_data"] = np.concatenate(data).astype(np.int32)
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    print("%s: %d frames, %d masks, %d ramps, Pillow %s, %d bytes" % (OUT, len(FRAME_CASES), len(mask_cases()), len(pairs),
                                                                      PIL.__version__, size))
    assert size < 300 * 1024
    return 0


if __name__ == "__main__":
    sys.exit(main())
