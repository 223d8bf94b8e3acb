"""Polygon ground truth in the evaluators (`COCOEval(polygons=True)`, `YTVISEval(polygons=True)` and the evaluator classes):
the documents of tests/golden/coco_eval.npz and ytvis_eval.npz with their RLE ground truth replaced by integer-rectangle
polygons of the same masks must give the numbers of the RLE documents, exactly."""
import copy
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from test_poly_rle import rect_polygons
from vnext_amd.evaluation import COCOEval, COCOEvaluator, YTVISEval, YTVISEvaluator
from vnext_amd.utils.ytvis_json import rle_decode

DEV = "cuda:0"


def decode(seg):
    counts = seg["counts"]
    if isinstance(counts, (str, bytes)):
        return rle_decode(seg).astype(bool)
    h, w = seg["size"]
    return np.repeat(np.arange(len(counts)) & 1, counts).astype(bool).reshape(w, h).T


@functools.lru_cache(maxsize=None)
def coco_documents():
    fx = dict(np.load(os.path.join(GOLDEN_DIR, "coco_eval.npz")))
    gt, dt = json.loads(str(fx["gt_json"])), json.loads(str(fx["dt_json"]))
    poly = copy.deepcopy(gt)
    n = 0
    for i, a in enumerate(poly["annotations"]):
        if i % 4 != 3:                                         # every fourth annotation keeps its RLE: one table of both
            a["segmentation"] = rect_polygons(decode(a["segmentation"]))
            n += bool(a["segmentation"])
    assert n > 8
    return gt, poly, dt, fx["area_rng"].tolist()


@functools.lru_cache(maxsize=None)
def ytvis_documents():
    fx = dict(np.load(os.path.join(GOLDEN_DIR, "ytvis_eval.npz")))
    gt, dt = json.loads(str(fx["gt_json"])), json.loads(str(fx["dt_json"]))
    sizes = {v["id"]: (v["height"], v["width"]) for v in gt["videos"]}
    poly = copy.deepcopy(gt)
    n = 0
    for i, a in enumerate(poly["annotations"]):
        for f, seg in enumerate(a["segmentations"]):
            if seg and (i + f) % 3:
                seg = dict(seg, size=seg.get("size") or list(sizes[a["video_id"]]))
                a["segmentations"][f] = rect_polygons(decode(seg)) or seg      # (an empty mask has no rectangle)
                n += isinstance(a["segmentations"][f], list)
    assert n > 8
    return gt, poly, dt, fx["area_rng"].tolist()


def same(a, b):
    for key in ("precision", "recall", "scores", "stats"):
        assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), key
    assert sorted(a["ious"]) == sorted(b["ious"])
    for k, v in a["ious"].items():
        assert np.array_equal(np.asarray(v), np.asarray(b["ious"][k])), k


@functools.lru_cache(maxsize=None)
def coco_host():
    gt, poly, dt, area_rng = coco_documents()
    return COCOEval(gt, "segm", device="cpu", area_rng=area_rng).add(dt).evaluate()


def test_coco_polygon_ground_truth_gives_the_numbers_of_the_rle_document():
    gt, poly, dt, area_rng = coco_documents()
    got = COCOEval(poly, "segm", device="cpu", area_rng=area_rng, polygons=True).add(dt).evaluate()
    assert got["AP"] > 0
    same(got, coco_host())


def test_coco_bbox_ignores_polygon_segmentations():
    gt, poly, dt, area_rng = coco_documents()
    same(COCOEval(poly, "bbox", device="cpu", area_rng=area_rng, polygons=True).add(dt).evaluate(),
         COCOEval(gt, "bbox", device="cpu", area_rng=area_rng).add(dt).evaluate())


def test_the_default_still_raises():
    gt, poly, dt, _ = coco_documents()
    for iou_type in ("bbox", "segm"):
        with pytest.raises(ValueError, match="is a polygon; only RLE ground truth is supported"):
            COCOEval(poly, iou_type, device="cpu")
        with pytest.raises(ValueError, match="is a polygon"):
            COCOEval(poly, iou_type, device="cpu", polygons=False)
    with pytest.raises(ValueError, match="is a polygon; only RLE ground"):
        YTVISEval(ytvis_documents()[1], device="cpu")


def test_coco_errors_name_the_annotation():
    gt, poly, dt, area_rng = coco_documents()
    bad = copy.deepcopy(poly)
    victim = next(a for a in bad["annotations"] if isinstance(a["segmentation"], list))
    victim["segmentation"] = [[1.0, 2.0, 3.0]]
    with pytest.raises(ValueError, match="malformed polygon ground truth"):
        COCOEval(bad, "segm", device="cpu", area_rng=area_rng, polygons=True).add(dt).evaluate()
    lost = copy.deepcopy(poly)
    for im in lost["images"]:
        del im["height"]
    with pytest.raises(ValueError, match="states no height / width"):
        COCOEval(lost, "segm", device="cpu", area_rng=area_rng, polygons=True).add(dt).evaluate()


def test_the_stated_area_is_kept():
    """COCO's polygon areas differ from pixel counts and COCOeval ranks by the stated one"""
    gt, poly, dt, area_rng = coco_documents()
    moved = copy.deepcopy(poly)
    for a in moved["annotations"]:
        a["area"] = 5.0                                          # everything "small", whatever the masks hold
    got = COCOEval(moved, "segm", device="cpu", area_rng=area_rng, polygons=True).add(dt).evaluate()
    rle = copy.deepcopy(gt)
    for a in rle["annotations"]:
        a["area"] = 5.0
    same(got, COCOEval(rle, "segm", device="cpu", area_rng=area_rng).add(dt).evaluate())


def test_coco_evaluator_class_passes_the_switch():
    gt, poly, dt, area_rng = coco_documents()
    ev = COCOEvaluator(poly, device="cpu", area_rng=area_rng, polygons=True)
    ev.process(None, dt)
    out = ev.evaluate()
    want = COCOEvaluator(gt, device="cpu", area_rng=area_rng)
    want.process(None, dt)
    assert set(out) == {"bbox", "segm"}
    np.testing.assert_equal(out, want.evaluate())              # (NaN where the reference has -1)
    with pytest.raises(ValueError, match="is a polygon"):
        e = COCOEvaluator(poly, device="cpu", area_rng=area_rng)
        e.process(None, dt)
        e.evaluate()


def test_ytvis_polygon_ground_truth_gives_the_numbers_of_the_rle_document():
    gt, poly, dt, area_rng = ytvis_documents()
    want = YTVISEval(gt, device="cpu", area_rng=area_rng).add(dt).evaluate()
    got = YTVISEval(poly, device="cpu", area_rng=area_rng, polygons=True).add(dt).evaluate()
    assert got["AP"] > 0
    same(got, want)
    ev = YTVISEvaluator(poly, device="cpu", area_rng=area_rng, polygons=True)
    ev.process(None, dt)
    assert ev.evaluate()["segm"]["AP"] == got["AP"] * 100


@pytest.mark.gpu
def test_coco_polygons_on_the_device_equal_the_cpu_route():
    gt, poly, dt, area_rng = coco_documents()
    ev = COCOEval(poly, "segm", device=DEV, area_rng=area_rng, polygons=True).add(dt)
    same(ev.evaluate(), coco_host())
    from vnext_amd.ops import poly_rle as P
    polys = [a["segmentation"] for a in poly["annotations"] if isinstance(a["segmentation"], list)]
    assert P.plan_objects(polys, [(64, 64)] * len(polys))[2].any()           # the kernel had objects of its own


@pytest.mark.gpu
def test_ytvis_polygons_on_the_device_equal_the_cpu_route():
    gt, poly, dt, area_rng = ytvis_documents()
    want = YTVISEval(gt, device="cpu", area_rng=area_rng).add(dt).evaluate()
    same(YTVISEval(poly, device=DEV, area_rng=area_rng, polygons=True).add(dt).evaluate(), want)
