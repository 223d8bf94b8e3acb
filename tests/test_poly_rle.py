"""CPU: the host restatement of pycocotools' rleFrPoly / merge / frPyObjects (vnext_amd/ops/poly_rle.py), checked on its own
merits -- pycocotools is not available, so nothing here compares with the package itself: exact integer rectangles, frozen
counts (tests/golden/poly_rle.npz, tools/make_golden_poly_rle.py), the canonical form, an independent even-odd
point-in-polygon test away from the edges, and the union against numpy."""
import functools
import importlib.util
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT
from vnext_amd.ops import poly_rle as P
from vnext_amd.ops import video_iou as V


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(GOLDEN_DIR, "poly_rle.npz")))


def sweep_triangles():
    """-> (xy float64 [20000, 6], expected count lists) of the contraction sweep"""
    fx = golden()
    xy = fx["sweep_num"].astype(np.float64) / 5
    starts, counts = fx["sweep_starts"], fx["sweep_counts"].astype(np.int64)
    return xy, [counts[a:b].tolist() for a, b in zip(starts[:-1], starts[1:])]


def rect_polygons(mask):
    """bool [h, w] -> integer-rectangle polygons whose union is the mask: the set runs of every column, a run repeated in the
    next column widening its rectangle"""
    h, w = mask.shape
    open_, out = {}, []
    for x in range(w + 1):
        col = mask[:, x] if x < w else np.zeros(h, dtype=bool)
        edge = np.flatnonzero(np.diff(np.concatenate(([0], col.astype(np.int8), [0]))))
        runs = set(zip(edge[0::2].tolist(), edge[1::2].tolist()))
        for r in list(open_):
            if r not in runs:
                x0 = open_.pop(r)
                out.append([x0, r[0], x0, r[1], x, r[1], x, r[0]])
        for r in runs:
            open_.setdefault(r, x)
    return [[float(v) for v in p] for p in out]


def point_in_polygon(poly, h, w):
    """even-odd rule at the pixel centres (x + 0.5, y + 0.5), and every centre's distance to the nearest edge"""
    x, y = poly[0::2], poly[1::2]
    px, py = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    inside, dist, n = np.zeros((h, w), bool), np.full((h, w), np.inf), len(x)
    for j in range(n):
        x1, y1, x2, y2 = x[j], y[j], x[(j + 1) % n], y[(j + 1) % n]
        with np.errstate(divide="ignore", invalid="ignore"):
            xi = (x2 - x1) * (py - y1) / (y2 - y1) + x1
        inside ^= ((y1 > py) != (y2 > py)) & (px < xi)
        ex, ey = x2 - x1, y2 - y1
        l2 = ex * ex + ey * ey
        t = np.clip(((px - x1) * ex + (py - y1) * ey) / l2, 0, 1) if l2 > 0 else np.zeros_like(px)
        dist = np.minimum(dist, np.hypot(px - (x1 + t * ex), py - (y1 + t * ey)))
    return inside, dist


def random_polygon(rng, h, w, k=None, margin=10.0):
    k = int(rng.integers(3, 9)) if k is None else k
    xy = np.empty(2 * k)
    xy[0::2], xy[1::2] = rng.uniform(-margin, w + margin, k), rng.uniform(-margin, h + margin, k)
    return xy


def test_integer_rectangles_are_exact_as_boxes_and_as_polygons():
    rng = np.random.default_rng(0)
    for _ in range(300):
        h, w = (int(v) for v in rng.integers(1, 41, 2))
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        bw, bh = int(rng.integers(1, w - x0 + 1)), int(rng.integers(1, h - y0 + 1))
        want = np.zeros((h, w), bool)
        want[y0:y0 + bh, x0:x0 + bw] = True
        box = P.object_counts_host([x0, y0, bw, bh], h, w)
        assert box == P.object_counts_host([[x0, y0, bw, bh]], h, w)
        assert box == P.object_counts_host([[x0, y0, x0, y0 + bh, x0 + bw, y0 + bh, x0 + bw, y0]], h, w)
        assert box == P.object_counts_host([x0, y0, x0, y0 + bh, x0 + bw, y0 + bh, x0 + bw, y0], h, w)
        assert box == P.mask_to_counts(want) and (P.counts_to_mask(box, h, w) == want).all()


def test_frozen_counts():
    fx = golden()
    assert P.poly_counts_host([1, 1, 5, 1, 5, 5], 8, 8) == [17, 1, 7, 2, 6, 3, 28] == fx["triangle_counts"].tolist()
    assert P.poly_counts_host(fx["triangle_xy"], *fx["triangle_size"]) == fx["triangle_counts"].tolist()
    for h, w in ((1, 1), (7, 9), (480, 640)):
        assert P.object_counts_host([[0.0] * 6], h, w) == [h * w]              # the reference's dummy annotation
        assert P.object_counts_host([np.array([0.0] * 6)], h, w) == [h * w]
        assert P.object_counts_host([], h, w) == [h * w]                        # polygons_to_bitmask of no polygon
    xy, want = sweep_triangles()
    h, w = golden()["sweep_size"]
    picked = sorted(set(range(0, len(xy), 40)) | set(fx["sweep_fused"].tolist()))
    for i in picked:
        assert P.poly_counts_host(xy[i], h, w) == want[i], i


def test_the_sweep_can_see_a_contracted_evaluation():
    """the triangles the fixture lists change their counts when ys + s * t is rounded once (a fused multiply-add)"""
    fx = golden()
    xy, want = sweep_triangles()
    h, w = fx["sweep_size"]
    assert len(fx["sweep_fused"]) >= 10
    for i in fx["sweep_fused"].tolist():
        assert P.poly_counts_host(xy[i], h, w, fused=True) != want[i], i


def test_canonical_form_outside_the_canvas_and_with_negative_coordinates():
    rng = np.random.default_rng(1)
    for _ in range(400):
        h, w = (int(v) for v in rng.integers(1, 41, 2))
        c = P.poly_counts_host(random_polygon(rng, h, w), h, w)
        assert sum(c) == h * w and c[0] >= 0 and all(v > 0 for v in c[1:])
    assert P.poly_counts_host([-9.5, -3, -2.5, -3, -2.5, -1], 5, 6) == [30]       # wholly outside
    assert P.poly_counts_host([7, 1, 9, 1, 9, 3], 5, 6) == [30]


def test_truncation_toward_zero():
    X, Y = P.upsampled_vertices([-0.25, -0.11, -0.3, 0.1, 0.29, -1.0])
    assert X.tolist() == [0, -1, 1] and Y.tolist() == [0, 1, -4]                # (int)(-0.75), (int)(-0.05), (int)(-1.0) ...


def test_integer_form_of_the_crossing_tests():
    """the kernel's integer restatement of step 3 equals the floating form for every residue, sign and clamp"""
    for d in list(range(-200, 200)) + [2 ** 27 - 3 + k for k in range(6)] + [-(2 ** 27) + k for k in range(6)]:
        f = (d + 0.5) / 5.0 - 0.5
        col = P.column_of(d)
        assert (col is not None) == (np.floor(f) == f)
        assert col is None or col == f
        for h in (1, 3, 50, 2 ** 27):
            assert P.row_of(d, h) == int(np.ceil(min(max(f, 0.0), float(h))))


def test_even_odd_rule_away_from_the_edges():
    rng = np.random.default_rng(2)
    pixels = wrong = 0
    for _ in range(400):
        h, w = (int(v) for v in rng.integers(8, 41, 2))
        xy = random_polygon(rng, h, w)
        got = P.counts_to_mask(P.poly_counts_host(xy, h, w), h, w)
        inside, dist = point_in_polygon(xy, h, w)
        far = dist > 1.0
        pixels += int(far.sum())
        wrong += int((got != inside)[far].sum())
    assert pixels > 100000 and wrong == 0


def test_merge_is_the_union():
    rng = np.random.default_rng(3)
    for _ in range(100):
        h, w = (int(v) for v in rng.integers(1, 30, 2))
        masks = [rng.random((h, w)) < rng.random() for _ in range(int(rng.integers(2, 5)))]
        got = P.merge_counts_host([P.mask_to_counts(m) for m in masks], h, w)
        assert got == P.mask_to_counts(np.logical_or.reduce(masks))
    assert P.merge_counts_host([[3, 2, 4]], 3, 3) == [3, 2, 4] and P.merge_counts_host([], 3, 3) == [9]
    assert P.merge_counts_host([[0, 9], [9]], 3, 3) == [0, 9]
    same = P.poly_counts_host([1, 1, 5, 1, 5, 5], 8, 8)
    assert P.merge_counts_host([same, same], 8, 8) == same                      # the union, not XOR


def test_objects_and_their_errors():
    assert P.object_counts_host([[1, 1, 2, 2], [4, 1, 1, 3]], 5, 6) == \
        P.mask_to_counts(np.logical_or(P.counts_to_mask(P.object_counts_host([1, 1, 2, 2], 5, 6), 5, 6),
                                       P.counts_to_mask(P.object_counts_host([4, 1, 1, 3], 5, 6), 5, 6)))
    for bad in ([[1, 2, 3, 4, 5]], [[1, 2, 3, 4, 5, 6, 7]], [1, 2], [[1.0, 2.0]], [[0, 0, 1, float("nan"), 1, 1]],
                [[0, 0, 1, 1, 2.0 ** 25, 1]], {"counts": [9], "size": [3, 3]}):
        with pytest.raises(ValueError):
            P.object_counts_host(bad, 9, 9)
    with pytest.raises(ValueError):
        P.object_counts_host([0, 0, 1, 1], 0, 5)
    with pytest.raises(ValueError, match="object 1"):
        P.polygons_to_runs([[0, 0, 2, 2], [[1, 2, 3]]], [(4, 4), (4, 4)])


def test_polygons_to_runs_on_the_host():
    objects = [[[1, 1, 5, 1, 5, 5]], [], [1, 1, 2, 2], [[0.5, 0.5, 3, 0.5, 3, 3], [2, 2, 6, 2, 6, 6, 2, 6]]]
    sizes = [(8, 8), (3, 3), (4, 5), (7, 9)]
    for device in (None, "cpu"):
        t = P.polygons_to_runs(objects, sizes, device=device)
        want = V.runs_from_counts([P.object_counts_host(o, *s) for o, s in zip(objects, sizes)], sizes)
        for a, b in zip((t.ends, t.ones, t.rows), (want.ends, want.ones, want.rows)):
            assert a.dtype == b.dtype and (a == b).all()
        assert not t.status.any() and (t.slot_rows == t.rows[:, :2]).all()
    both = V.concat_tables(t, t)
    assert len(both) == 8 and (both.rows[4:, 0] == t.rows[:, 0] + len(t.ends)).all()
    assert len(P.polygons_to_runs([], [])) == 0


def test_the_crossing_bound_holds_and_is_tight():
    rng = np.random.default_rng(4)
    worst = 0.0
    for _ in range(1000):
        h, w = (int(v) for v in rng.integers(1, 60, 2))
        xy = random_polygon(rng, h, w, k=int(rng.integers(3, 12)))
        X, Y = P.upsampled_vertices(xy)
        u, v = P.dense_points(X, Y)
        n = len(P.crossings(u, v, h, w))
        assert n <= P.crossing_bound(X, w)
        worst = max(worst, n / P.crossing_bound(X, w))
    assert worst > 0.8


def test_pack_tables_layout():
    polys, slots, fits = P.plan_objects([[[1, 1, 5, 1, 5, 5], [0, 0, 2, 0, 2, 2]], [], [0, 0, 3, 3]], [(8, 8), (3, 3), (4, 5)])
    assert fits.all() and slots[1] == 1
    coords, prow, orow, total = P.pack_tables(polys, [(8, 8), (3, 3), (4, 5)], slots)
    assert prow.tolist() == [[0, 3, 0, 0], [6, 3, 0, 0], [12, 4, 2, 0]] and len(coords) == 20
    assert orow[:, :2].tolist() == [[0, 2], [2, 0], [2, 1]] and orow[:, 4:].tolist() == [[8, 8], [3, 3], [4, 5]]
    assert (orow[:, 2] == np.cumsum(slots) - slots).all() and (orow[:, 3] == slots).all() and total == slots.sum()
    big = [[float(v) for k in range(1100) for v in (k % 7, k % 5)]]            # more vertices than the kernel takes
    assert not P.plan_objects([big], [(9, 9)])[2].any() and not P.fits_caps([big], [(9, 9)])


def test_the_standin_takes_polygons_and_boxes():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    spec = importlib.util.spec_from_file_location("pycocotools_standin", os.path.join(tools, "pycocotools_standin.py"))
    S = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(S)
    from vnext_amd.utils.ytvis_json import string_to_counts
    polys = [[1, 1, 5, 1, 5, 5], [2, 2, 6, 2, 6, 6, 2, 6]]
    rles = S.frPyObjects(polys, 8, 8)
    assert [list(string_to_counts(r["counts"])) for r in rles] == [P.poly_counts_host(p, 8, 8) for p in polys]
    assert list(string_to_counts(S.merge(rles)["counts"])) == P.object_counts_host(polys, 8, 8)
    assert list(string_to_counts(S.frPyObjects([1, 1, 2, 2], 4, 5)["counts"])) == P.object_counts_host([1, 1, 2, 2], 4, 5)
    assert S.frPyObjects({"size": [3, 3], "counts": [4, 2, 3]}, 3, 3)["size"] == [3, 3]      # RLE input as before
    assert int(S.area(S.merge(rles))) == sum(P.object_counts_host(polys, 8, 8)[1::2])
