"""The local COCO evaluator (vnext_amd/evaluation/coco_eval.py) against the reference's own numbers
(tests/golden/coco_eval.npz, written by tools/make_golden_coco_eval.py: the reference's matching, accumulation and
summary on IoUs computed on dense masks and on the box formula).  Every comparison is exact."""
import functools
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT
from vnext_amd.evaluation import STAT_NAMES, COCOEval, COCOEvaluator, YTVISEval
from vnext_amd.utils.ytvis_json import rle_decode

REFERENCE = "/root/reference"
TYPES = ("bbox", "segm")


def _tool(name):
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    spec = importlib.util.spec_from_file_location(name, os.path.join(tools, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(GOLDEN_DIR, "coco_eval.npz")))


def documents():
    fx = golden()
    return json.loads(str(fx["gt_json"])), json.loads(str(fx["dt_json"]))


def evaluate(iou_type, records=None, **kw):
    gt, recs = documents()
    ev = COCOEval(gt, iou_type, area_rng=golden()["area_rng"].tolist(), **kw).add(recs if records is None else records)
    return ev.evaluate(eval_imgs=True), ev


def assert_equals_golden(res, fx, t):
    """every recorded array with ==, the summary included"""
    imgs, cats = fx["img_ids"].tolist(), fx["cat_ids"].tolist()
    assert sorted(res["ious"]) == sorted((v, c) for v in imgs for c in cats)
    pairs = 0
    for (v, c), iou in res["ious"].items():
        want = fx[f"{t}_ious_{v}_{c}"]
        if want.ndim == 1:
            assert isinstance(iou, list) and iou == []
        else:
            assert iou.shape == want.shape and iou.dtype == np.float64 and (iou == want).all(), (v, c)
            pairs += want.size
    assert pairs > 100
    assert len(res["eval_imgs"]) == len(fx[f"{t}_eval_none"]) == len(cats) * 4 * len(imgs)
    for n, e in enumerate(res["eval_imgs"]):
        assert (e is None) == bool(fx[f"{t}_eval_none"][n]), n
        if e is None:
            continue
        for key, name in (("dtMatches", "dtm"), ("gtMatches", "gtm"), ("dtIgnore", "dtig"), ("gtIgnore", "gtig")):
            want = fx[f"{t}_ev{n}_{name}"]
            got = np.asarray(e[key])
            assert got.shape == want.shape and (got == want).all(), (n, key)
    for key in ("precision", "recall", "scores"):
        assert res[key].shape == fx[f"{t}_{key}"].shape and (res[key] == fx[f"{t}_{key}"]).all(), key
    assert (res["stats"] == fx[f"{t}_stats"]).all()
    assert [res[n] for n in STAT_NAMES] == res["stats"].tolist()
    assert set(STAT_NAMES) | {"stats", "per_category", "precision", "recall", "scores", "ious"} <= set(res)


@functools.lru_cache(maxsize=None)
def host_result(iou_type):
    return evaluate(iou_type, device="cpu")


@pytest.mark.parametrize("iou_type", TYPES)
def test_host_route_reproduces_the_reference(iou_type):
    res, ev = host_result(iou_type)
    assert ev.matching == "host" and ev.timings["matching"] == "host"
    assert_equals_golden(res, golden(), iou_type)


@pytest.mark.parametrize("iou_type", TYPES)
def test_vectorised_host_route_equals_match_host(iou_type):
    res, ev = evaluate(iou_type, device="cpu", matching="vectorised")
    assert ev.matching == "vectorised"
    assert_equals_golden(res, golden(), iou_type)
    want, _ = host_result(iou_type)
    for a, b in zip(res["eval_imgs"], want["eval_imgs"]):
        assert (a is None) == (b is None)
        if a is not None:
            assert a["dtIds"] == b["dtIds"] and a["gtIds"] == b["gtIds"] and a["dtScores"] == b["dtScores"]
            for k in ("dtMatches", "gtMatches", "dtIgnore", "gtIgnore"):
                assert a[k].tobytes() == b[k].tobytes() and a[k].dtype == b[k].dtype


def test_match_vectorised_equals_match_host_on_random_problems():
    from test_ap_match import random_problems
    from vnext_amd.ops import ap_match as M
    args = random_problems(seed=5, problems=60)
    a, b = M.match_vectorised(*args), M.match_host(*args)
    for name in ("dt_match", "dt_ignore", "gt_match", "gt_ignore"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), name


def test_eval_imgs_only_on_request():
    gt, recs = documents()
    res = COCOEval(gt, "bbox", device="cpu").add(recs).evaluate()
    assert "eval_imgs" not in res and res["AP"] > 0


def test_segm_ignores_the_bbox_key():
    """detectron2 drops `bbox` before a segm evaluation (`_evaluate_predictions_on_coco`): the area is the mask's"""
    gt, recs = documents()
    assert any(r["bbox"][2] * r["bbox"][3] != rle_decode(r["segmentation"]).sum() for r in recs)
    without = [{k: v for k, v in r.items() if k != "bbox"} for r in recs]
    wrong = [dict(r, bbox=[0.0, 0.0, 1.0, 1.0]) for r in recs]
    want, _ = host_result("segm")
    for records in (without, wrong):
        res, _ = evaluate("segm", records=records, device="cpu")
        for k in ("precision", "recall", "scores", "stats"):
            assert res[k].tobytes() == want[k].tobytes(), k
    with pytest.raises(ValueError, match="record 0 has no 'bbox'"):
        evaluate("bbox", records=without, device="cpu")


def test_fixture_conditions():
    cond = _tool("make_golden_coco_eval").fixture_conditions(golden())
    assert len(cond) >= 20 and all(cond.values()), [k for k, ok in cond.items() if not ok]
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "coco_eval.npz")) < 400 * 1024


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not on this machine")
def test_generator_reproduces_the_fixture():
    fx, again = golden(), _tool("make_golden_coco_eval").generate(REFERENCE)
    assert sorted(fx) == sorted(again)
    for k in fx:
        a, b = np.asarray(fx[k]), np.asarray(again[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_per_category_ap_and_gt_as_a_path(tmp_path):
    fx = golden()
    for t in TYPES:
        res, _ = host_result(t)
        assert list(res["per_category"]) == ["person", "dog", "car"]
        for k, name in enumerate(res["per_category"]):
            p = fx[f"{t}_precision"][:, :, k, 0, -1]
            assert res["per_category"][name] == float(np.mean(p[p > -1]) * 100)
    gt, recs = documents()
    path = tmp_path / "gt.json"
    path.write_text(json.dumps(gt))
    ev = COCOEval(str(path), "bbox", device="cpu", area_rng=fx["area_rng"].tolist())
    for v in (6, 1, 2, 3, 4, 5):                  # batches in any order of images: ids follow the order of arrival
        ev.add([r for r in recs if r["image_id"] == v])
    assert (ev.evaluate()["precision"] == fx["bbox_precision"]).all()
    assert COCOEval(gt, "bbox", device="cpu").area_rng[1:3] == [[0, 32 ** 2], [32 ** 2, 96 ** 2]]


def test_error_cases():
    gt, recs = documents()
    poly = json.loads(json.dumps(gt))
    poly["annotations"][2]["segmentation"] = [[1.0, 1.0, 5.0, 1.0, 5.0, 5.0]]
    for t in TYPES:
        with pytest.raises(ValueError, match="annotation 3 is a polygon"):
            COCOEval(poly, t, device="cpu")
    with pytest.raises(ValueError, match="record 0 names image 99"):
        COCOEval(gt, "bbox", device="cpu").add([dict(recs[0], image_id=99)])
    with pytest.raises(ValueError, match="iou_type 'keypoints'"):
        COCOEval(gt, "keypoints", device="cpu")
    wrong = dict(recs[0], segmentation={"size": [40, 24], "counts": recs[0]["segmentation"]["counts"]})
    with pytest.raises(ValueError, match="mask-size mismatch: record 0 .* is 40 x 24"):
        COCOEval(gt, "segm", device="cpu").add([wrong]).evaluate()
    with pytest.raises(ValueError, match="matching 'device'"):
        COCOEval(gt, "bbox", device="cpu", matching="device")


def test_evaluator_protocol_on_records_and_on_instances():
    gt, recs = documents()
    fx = golden()
    ev = COCOEvaluator(gt, device="cpu", area_rng=fx["area_rng"].tolist())
    for _ in range(2):                                  # reset() starts over
        ev.reset()
        for v in gt["images"]:
            mine = [r for r in recs if r["image_id"] == v["id"]]
            inputs = [{"image_id": v["id"], "height": v["height"], "width": v["width"]}]
            if v["id"] % 2:                             # `IDOL.coco_records`-shaped: a list of records
                ev.process(inputs, mine)
            else:                                       # `model(inputs)`: xyxy boxes, class indices, dense masks
                b = np.array([r["bbox"] for r in mine], dtype=np.float64)
                ev.process(inputs, [{"instances": {
                    "image_size": (v["height"], v["width"]), "scores": np.array([r["score"] for r in mine]),
                    "pred_boxes": np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1),
                    "pred_classes": np.array([r["category_id"] for r in mine]),
                    "pred_masks": np.stack([rle_decode(r["segmentation"]) for r in mine]).astype(np.uint8)}}])
        out = ev.evaluate()
    assert list(out) == ["bbox", "segm"]
    # xyxy -> xywh is (x + w) - x in float64: not the recorded w for every box, so the bbox numbers are compared with
    # an evaluation of the records as the evaluator formed them; segm has no such step and equals the fixture
    for n, want in zip(STAT_NAMES[:6], fx["segm_stats"]):
        assert out["segm"][n] == want * 100, n
    again = COCOEval(gt, "bbox", device="cpu", area_rng=fx["area_rng"].tolist()).add(ev.records).evaluate()
    for n in STAT_NAMES[:6]:
        assert out["bbox"][n] == again[n] * 100, n
    assert set(out["bbox"]) == set(out["segm"]) == set(STAT_NAMES[:6]) | {"AP-person", "AP-dog", "AP-car"}
    # MASK_ON false: no record carries a mask, no "segm"
    ev.reset()
    ev.process(None, [{k: v for k, v in r.items() if k != "segmentation"} for r in recs])
    out = ev.evaluate()
    assert list(out) == ["bbox"]
    assert [out["bbox"][n] for n in STAT_NAMES[:6]] == (fx["bbox_stats"][:6] * 100).tolist()
    ev.reset()
    assert list(ev.evaluate()) == ["bbox"] and all(np.isnan(x) for x in ev.evaluate()["bbox"].values())


def test_class_indices_map_to_category_ids():
    gt, recs = documents()
    ev = COCOEvaluator(gt, device="cpu", category_ids=[1, 2, 3])
    ev.process([{"image_id": 1}], [{"instances": {"pred_boxes": np.array([[1.0, 2.0, 4.0, 8.0]]), "scores": np.array([0.5]),
                                                  "pred_classes": np.array([2])}}])
    assert ev.records == [{"image_id": 1, "score": 0.5, "bbox": [1.0, 2.0, 3.0, 6.0], "category_id": 3}]


def test_abi_declares_the_op():
    from vnext_amd import _lib
    assert _lib.ABI_VERSION == 17
    assert "vnx_ap_match" in _lib.SIGNATURES and hasattr(_lib.product_lib(), "vnx_ap_match")


# ---- the device route ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("iou_type", TYPES)
def test_device_route_reproduces_the_reference_twice(iou_type):
    res, ev = evaluate(iou_type, device="cuda")
    assert ev.matching == "device" and not ev.timings["host_fallback"]
    assert_equals_golden(res, golden(), iou_type)
    again, _ = evaluate(iou_type, device="cuda")
    for k in ("precision", "recall", "scores", "stats"):
        assert res[k].tobytes() == again[k].tobytes(), k
    for a, b in zip(res["eval_imgs"], again["eval_imgs"]):
        assert (a is None) == (b is None)
        if a is not None:
            for k in ("dtMatches", "gtMatches", "dtIgnore", "gtIgnore"):
                assert a[k].tobytes() == b[k].tobytes(), k
    for key in res["ious"]:
        assert np.asarray(res["ious"][key]).tobytes() == np.asarray(again["ious"][key]).tobytes()


@pytest.mark.gpu
def test_ytvis_eval_with_device_matching_reproduces_its_fixture():
    from test_ytvis_eval import assert_equals_golden as assert_ytvis, golden as ytvis_golden, golden_documents
    gt, recs = golden_documents()
    fx = ytvis_golden()
    ev = YTVISEval(gt, device="cuda", area_rng=fx["area_rng"].tolist(), device_matching=True).add(recs)
    res = ev.evaluate()
    assert ev.matching == "device" and ev.timings["matching"] == "device" and not ev.timings["host_fallback"]
    assert_ytvis(res, fx)
    plain = YTVISEval(gt, device="cuda", area_rng=fx["area_rng"].tolist()).add(recs).evaluate()
    for a, b in zip(res["eval_vids"], plain["eval_vids"]):
        assert (a is None) == (b is None)
        if a is not None:
            assert a["dtIds"] == b["dtIds"] and a["gtIds"] == b["gtIds"]
            for k in ("dtMatches", "gtMatches", "dtIgnore", "gtIgnore"):
                assert (np.asarray(a[k]) == np.asarray(b[k])).all(), k
