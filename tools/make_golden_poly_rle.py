"""Write tests/golden/poly_rle.npz: frozen results of the host restatement of pycocotools' `rleFrPoly`
(vnext_amd/ops/poly_rle.py poly_counts_host) and the contraction sweep of tests/test_poly_rle_gpu.py.

pycocotools is imported when it is there and then supplies the expected counts (`source` says which); where it is not -- it
was not when the committed fixture was written -- the counts are the restatement's own, and the fixture freezes them so that
a later change of the host code shows.  Run on the CPU: `python tools/make_golden_poly_rle.py`.

  triangle_xy, triangle_size, triangle_counts: the triangle [1,1, 5,1, 5,5] on 8 x 8;
  sweep_seed, sweep_size, sweep_num int16 [20000, 6]: triangles on a 24 x 24 canvas with vertices on the 0.2 grid, the
      coordinates being sweep_num / 5 (numerators from `default_rng(seed).integers(-10, 130)`);
  sweep_counts uint16, sweep_starts int32 [20001]: every triangle's counts, back to back;
  sweep_fused int32: the triangles whose counts CHANGE when the two line expressions are evaluated with a fused
      multiply-add (exact rational arithmetic rounded once) -- the form a contracted build of the kernel would compute.  At
      least 10 must: without them the sweep cannot tell a contracted build from a correct one.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "poly_rle.npz")
SWEEP_SEED, SWEEP_N, SWEEP_SIZE = 3, 20000, (24, 24)


def sweep_numerators(seed=SWEEP_SEED, n=SWEEP_N):
    return np.random.default_rng(seed).integers(-10, 130, size=(n, 6)).astype(np.int16)


def main():
    from vnext_amd.ops.poly_rle import poly_counts_host
    try:
        from pycocotools import mask as coco_mask
        from vnext_amd.utils.ytvis_json import string_to_counts

        def expected(xy, h, w):
            return [int(c) for c in string_to_counts(coco_mask.frPyObjects([list(xy)], h, w)[0]["counts"].decode("ascii"))]
        source = "pycocotools"
    except ImportError:
        expected, source = poly_counts_host, "restatement"
    tri = np.array([1, 1, 5, 1, 5, 5], dtype=np.float64)
    h, w = SWEEP_SIZE
    num = sweep_numerators()
    counts, starts, fused = [], [0], []
    for i, row in enumerate(num):
        xy = row.astype(np.float64) / 5
        c = expected(xy, h, w)
        assert c == poly_counts_host(xy, h, w), f"triangle {i}: the restatement differs from {source}"
        if poly_counts_host(xy, h, w, fused=True) != c:
            fused.append(i)
        counts += c
        starts.append(len(counts))
    assert len(fused) >= 10, f"only {len(fused)} triangles change under contraction: the sweep cannot see a contracted build"
    np.savez_compressed(OUT, source=np.array(source), triangle_xy=tri, triangle_size=np.array([8, 8], dtype=np.int32),
                        triangle_counts=np.array(expected(tri, 8, 8), dtype=np.int32),
                        sweep_seed=np.array(SWEEP_SEED), sweep_size=np.array(SWEEP_SIZE, dtype=np.int32), sweep_num=num,
                        sweep_counts=np.array(counts, dtype=np.uint16), sweep_starts=np.array(starts, dtype=np.int32),
                        sweep_fused=np.array(fused, dtype=np.int32))
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; source {source}; {len(fused)} of {len(num)} triangles change under contraction")


if __name__ == "__main__":
    main()
