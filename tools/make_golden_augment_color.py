"""Write tests/golden/augment_color.npz: detectron2's RandomBrightness, RandomContrast and RandomSaturation (DESIGN section
31) applied, literally and in numpy, to frames Pillow cropped, resized and flipped -- the cases of tests/test_augment_color.py
and tests/test_train_augment_color_gpu.py.

Run on the CPU, where Pillow is installed (`python tools/make_golden_augment_color.py`); numpy and Pillow only, nothing of
the package: the three steps below are written out here, independently of `vnext_amd.ops.augment.color_frame`, which the
tests hold to this file.  Everything is regenerated from fixed seeds.
  per case i:  `c<i>_src` uint8 [h, w, 3]; `c<i>_plan` int32 {x0, y0, cw, ch, nh, nw, flip}; `c<i>_weights` float64
               {brightness, contrast, saturation}; `c<i>_s0` uint8 [nh, nw, 3]: the frame cropped, resized (BILINEAR) and
               flipped; `c<i>_s<k>`, k = 1 .. 7: the frame after the steps of subset k (1 brightness | 2 contrast | 4
               saturation), so s1, s3 and s7 are the frame after each of the three stages of the full list;
  batches:     `batch<j>` int32: the cases of one step; `batch<j>_x` float32 [n, 3, H, W] and `batch<j>_mask` bool [n, H, W]:
               the normalised, padded network input with all three steps on; `pixel_mean`, `pixel_std` float32 [3];
  the gray sum: `dot_disagreements`: on how many of the 2^24 (c0, c1, c2) byte triples `image.dot([0.299, 0.587, 0.114])` --
               numpy's BLAS -- differs from the left-to-right sum of three rounded products that the package defines.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "augment_color.npz")

# (source h, w), what fills it, window (x0, y0, cw, ch), target (nh, nw), flip, weights (None: drawn from [0.9, 1.1])
CASES = [
    ((100, 64), "random", (2, 3, 58, 90), (70, 45), False, None),           # 3 x 2 tiles feed one mean
    ((40, 50), "random", (5, 3, 40, 30), (24, 34), True, None),             # crop and flip
    ((1, 1), "random", (0, 0, 1, 1), (1, 1), False, None),                  # one pixel
    ((6, 9), 255, (0, 0, 9, 6), (5, 7), False, (1.1, 1.1, 1.1)),            # every step clips at 255
    ((6, 9), 0, (0, 0, 9, 6), (5, 7), True, (0.9, 1.1, 0.9)),               # all zero
    ((20, 30), "random", (1, 2, 27, 17), (13, 17), False, (0.9, 0.9, 0.9)),     # the ends of the range, exactly
    ((20, 30), "random", (0, 0, 30, 20), (13, 17), True, (1.1, 1.1, 1.1)),
]
BATCHES = [(0, 1, 2), (3, 4, 5, 6)]      # the first: three frames of different targets (the mean ignores padding and the others)
PIXEL_MEAN, PIXEL_STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def to_bytes(x):
    return np.clip(x, 0, 255).astype(np.uint8)


def brightness(u, w):
    """BlendTransform(src_image=0, src_weight=1 - w, dst_weight=w) on a uint8 image: float32"""
    img = u.astype(np.float32)
    return to_bytes((1 - w) * 0 + w * img)


def contrast(u, w):
    """BlendTransform(src_image=u.mean(), src_weight=1 - w, dst_weight=w): float64"""
    return to_bytes((1 - w) * u.mean() + w * u.astype(np.float64))


def gray_sum(u):
    """the package's definition of `u.dot([0.299, 0.587, 0.114])`: three rounded products, summed left to right"""
    f = u.astype(np.float64)
    return f[..., 0] * 0.299 + f[..., 1] * 0.587 + f[..., 2] * 0.114


def saturation(u, w):
    """BlendTransform(src_image=gray[:, :, None], src_weight=1 - w, dst_weight=w): float64"""
    return to_bytes((1 - w) * gray_sum(u)[:, :, np.newaxis] + w * u.astype(np.float64))


def dot_disagreements():
    """over all 2^24 byte triples, as 256 images of 256 x 256"""
    c1, c2 = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    n = 0
    for c0 in range(256):
        image = np.stack((np.full_like(c1, c0), c1, c2), axis=-1)
        n += int(np.count_nonzero(image.dot([0.299, 0.587, 0.114]) != gray_sum(image)))
    return n


def main():
    import PIL
    from PIL import Image

    rng = np.random.default_rng(31)
    arrays = {"pillow_version": np.array(PIL.__version__), "numpy_version": np.array(np.__version__),
              "pixel_mean": np.array(PIXEL_MEAN, dtype=np.float32), "pixel_std": np.array(PIXEL_STD, dtype=np.float32)}
    full = []
    for i, ((h, w), fill, (x0, y0, cw, ch), (nh, nw), flip, weights) in enumerate(CASES):
        src = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if fill == "random" else np.full((h, w, 3), fill, dtype=np.uint8)
        weights = tuple(float(v) for v in (rng.uniform(0.9, 1.1, 3) if weights is None else weights))
        u = np.asarray(Image.fromarray(np.ascontiguousarray(src[y0:y0 + ch, x0:x0 + cw])).resize((nw, nh), Image.BILINEAR))
        u = np.ascontiguousarray(np.flip(u, axis=1) if flip else u)
        arrays["c%d_src" % i] = src
        arrays["c%d_plan" % i] = np.array([x0, y0, cw, ch, nh, nw, int(flip)], dtype=np.int32)
        arrays["c%d_weights" % i] = np.array(weights, dtype=np.float64)
        arrays["c%d_s0" % i] = u
        for k in range(1, 8):
            v = u
            for bit, step, wgt in zip((1, 2, 4), (brightness, contrast, saturation), weights):
                if k & bit:
                    v = step(v, wgt)
            assert v.dtype == np.uint8 and v.shape == u.shape
            arrays["c%d_s%d" % (i, k)] = v
        full.append(arrays["c%d_s7" % i])
    mean, std = arrays["pixel_mean"].reshape(3, 1, 1), arrays["pixel_std"].reshape(3, 1, 1)
    for j, cases in enumerate(BATCHES):
        H = (max(full[i].shape[0] for i in cases) + 31) // 32 * 32
        W = (max(full[i].shape[1] for i in cases) + 31) // 32 * 32
        x, mask = np.zeros((len(cases), 3, H, W), dtype=np.float32), np.ones((len(cases), H, W), dtype=bool)
        for b, i in enumerate(cases):
            nh, nw = full[i].shape[:2]
            x[b, :, :nh, :nw] = (full[i].transpose(2, 0, 1).astype(np.float32) - mean) / std
            mask[b, :nh, :nw] = False
        arrays["batch%d" % j], arrays["batch%d_x" % j], arrays["batch%d_mask" % j] = np.array(cases, dtype=np.int32), x, mask
    arrays["dot_disagreements"] = np.array(dot_disagreements(), dtype=np.int64)
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    print("%s: %d cases, %d batches, Pillow %s, numpy %s, %d of 2^24 triples where dot differs from the definition, %d bytes"
          % (OUT, len(CASES), len(BATCHES), PIL.__version__, np.__version__, int(arrays["dot_disagreements"]), size))
    assert size < 400 * 1024
    return 0


if __name__ == "__main__":
    sys.exit(main())
