"""The local YTVIS evaluator (vnext_amd/evaluation/ytvis_eval.py) on its numpy path against the reference's own
numbers (tests/golden/ytvis_eval.npz, written by tools/make_golden_ytvis_eval.py from YTVOS.loadRes + YTVOSeval), the
host run-table builder (vnext_amd/ops/video_iou.py) and the pycocotools stand-in the generator runs the reference with."""
import functools
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT
from vnext_amd import _lib
from vnext_amd.evaluation import STAT_NAMES, YTVISEval, YTVISEvaluator
from vnext_amd.ops import video_iou as V
from vnext_amd.utils.ytvis_json import counts_to_string, rle_counts, rle_decode, rle_encode

REFERENCE = "/root/reference"


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
    return dict(np.load(os.path.join(GOLDEN_DIR, "ytvis_eval.npz")))


def golden_documents():
    fx = golden()
    return json.loads(str(fx["gt_json"])), json.loads(str(fx["dt_json"]))


def assert_equals_golden(res, fx):
    """every recorded array with ==; stats within 1e-12 (numpy's `mean` owns its summation order)"""
    vids, cats = fx["vid_ids"].tolist(), fx["cat_ids"].tolist()
    assert sorted(res["ious"]) == sorted((v, c) for v in vids for c in cats)
    pairs = 0
    for (v, c), iou in res["ious"].items():
        want = fx[f"ious_{v}_{c}"]
        if want.ndim == 1:
            assert isinstance(iou, list) and iou == []
        else:
            assert iou.shape == want.shape and iou.dtype == np.float64 and (iou == want).all(), (v, c)
            pairs += want.size
    assert pairs > 100
    assert len(res["eval_vids"]) == len(fx["eval_none"]) == len(cats) * 4 * len(vids)
    for n, e in enumerate(res["eval_vids"]):
        assert (e is None) == bool(fx["eval_none"][n]), n
        if e is None:
            continue
        for key, name in (("dtMatches", "dtm"), ("gtMatches", "gtm"), ("dtIgnore", "dtig"), ("gtIgnore", "gtig")):
            want = fx[f"ev{n}_{name}"]
            got = np.asarray(e[key])
            assert got.shape == want.shape and (got == want).all(), (n, key)
    for key in ("precision", "recall", "scores"):
        assert res[key].shape == fx[key].shape and (res[key] == fx[key]).all(), key
    np.testing.assert_allclose(res["stats"], fx["stats"], rtol=0, atol=1e-12)
    assert [res[n] for n in STAT_NAMES] == res["stats"].tolist()


@functools.lru_cache(maxsize=None)
def host_result():
    gt, recs = golden_documents()
    return YTVISEval(gt, device="cpu", area_rng=golden()["area_rng"].tolist()).add(recs).evaluate()


def test_numpy_path_reproduces_the_reference():
    assert_equals_golden(host_result(), golden())


def test_records_may_arrive_per_video_and_gt_as_a_path(tmp_path):
    gt, recs = golden_documents()
    path = tmp_path / "gt.json"
    path.write_text(json.dumps(gt))
    ev = YTVISEval(str(path), device="cpu", area_rng=golden()["area_rng"].tolist())
    for v in (1, 2, 3, 4):                        # the records are ordered by nothing: ids follow the order of arrival
        ev.add([r for r in recs if r["video_id"] == v])
    res = ev.evaluate()
    np.testing.assert_allclose(res["stats"], golden()["stats"], rtol=0, atol=1e-12)
    assert (res["precision"] == golden()["precision"]).all()


def test_fixture_conditions():
    cond = _tool("make_golden_ytvis_eval").fixture_conditions(golden())
    assert len(cond) >= 10 and all(cond.values()), [k for k, ok in cond.items() if not ok]
    fx = golden()
    assert 0.2 < fx["stats"][0] < 0.9
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "ytvis_eval.npz")) < 200 * 1024
    gt, recs = golden_documents()
    assert {(v["height"], v["width"]) for v in gt["videos"]} == {(24, 40), (37, 53)}
    assert all(6 <= v["length"] <= 9 for v in gt["videos"])


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not on this machine")
def test_generator_reproduces_the_fixture():
    fx, again = golden(), _tool("make_golden_ytvis_eval").generate(REFERENCE)
    assert sorted(fx) == sorted(again)
    for k in fx:
        a, b = np.asarray(fx[k]), np.asarray(again[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_per_category_ap_and_untouched_entries():
    res, fx = host_result(), golden()
    assert list(res["per_category"]) == ["person", "dog", "car"]
    for k, name in enumerate(res["per_category"]):
        p = fx["precision"][:, :, k, 0, -1]
        assert res["per_category"][name] == float(np.mean(p[p > -1]) * 100)
    # what the reference leaves at -1 stays -1: with one max_dets entry fewer there is no "maxDets=100" column
    gt, recs = golden_documents()
    few = YTVISEval(gt, device="cpu", area_rng=fx["area_rng"].tolist(), max_dets=(1, 10)).add(recs).evaluate()
    assert few["AP"] == -1 and few["AR1"] > 0
    none = YTVISEval(gt, device="cpu", area_rng=[[0, 1e10], [0, 1], [1, 2], [2, 3]]).add(recs).evaluate()
    assert none["APs"] == none["APm"] == none["APl"] == -1 and none["AP"] > 0
    assert (none["precision"][:, :, :, 1:, :] == -1).all()


# ---- the matching routes, and the arithmetic shared with COCOEval ----------------------------------------------------
def assert_same_eval_vids(a, b):
    """two results' `eval_vids`: the same ids and scores, the four match arrays byte for byte with equal dtypes"""
    assert len(a["eval_vids"]) == len(b["eval_vids"]) > 0
    for x, y in zip(a["eval_vids"], b["eval_vids"]):
        assert (x is None) == (y is None)
        if x is not None:
            assert x["dtIds"] == y["dtIds"] and x["gtIds"] == y["gtIds"] and x["dtScores"] == y["dtScores"]
            for k in ("dtMatches", "gtMatches", "dtIgnore", "gtIgnore"):
                assert x[k].tobytes() == y[k].tobytes() and x[k].dtype == y[k].dtype, k


def test_vectorised_host_route_equals_match_host():
    gt, recs = golden_documents()
    res = {}
    for matching in ("host", "vectorised"):
        ev = YTVISEval(gt, device="cpu", area_rng=golden()["area_rng"].tolist(), matching=matching).add(recs)
        res[matching] = ev.evaluate()
        assert ev.matching == ev.timings["matching"] == matching
        assert_equals_golden(res[matching], golden())
    assert_same_eval_vids(res["vectorised"], res["host"])


def test_matching_defaults_and_the_device_route_without_a_device():
    gt, _ = golden_documents()
    assert YTVISEval(gt, device="cpu").matching == "host"
    assert YTVISEval(gt, device="cpu", device_matching=True).matching == "host"       # silently off without a device
    with pytest.raises(ValueError, match="matching 'device'"):
        YTVISEval(gt, device="cpu", matching="device")


def test_coco_eval_and_ytvis_eval_share_their_arithmetic():
    """COCO's segm documents restated as one-frame videos score the same under both classes once the crowds are gone:
    the crowd's union (the detection's area alone) is COCOEval's, and with the crowds in, the two differ."""
    from vnext_amd.evaluation import COCOEval
    fx = dict(np.load(os.path.join(GOLDEN_DIR, "coco_eval.npz")))
    gt, recs = json.loads(str(fx["gt_json"])), json.loads(str(fx["dt_json"]))
    area_rng = fx["area_rng"].tolist()
    assert len(gt["annotations"]) == 18 and sum(bool(a["iscrowd"]) for a in gt["annotations"]) == 2

    def both(anns):
        coco = dict(gt, annotations=anns)
        videos = {"videos": [dict(v, length=1) for v in gt["images"]], "categories": gt["categories"],
                  "annotations": [{"id": a["id"], "video_id": a["image_id"], "category_id": a["category_id"],
                                   "iscrowd": a["iscrowd"], "segmentations": [a["segmentation"]], "areas": [a["area"]]}
                                  for a in anns]}
        tracks = [{"video_id": r["image_id"], "category_id": r["category_id"], "score": r["score"],
                   "segmentations": [r["segmentation"]]} for r in recs]
        return (COCOEval(coco, "segm", device="cpu", area_rng=area_rng).add(recs).evaluate(),
                YTVISEval(videos, device="cpu", area_rng=area_rng).add(tracks).evaluate())
    a, b = both([a for a in gt["annotations"] if not a["iscrowd"]])
    assert a["AP"] > 0.5
    for key in ("precision", "recall", "scores", "stats"):
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key
    a, b = both(gt["annotations"])
    assert a["precision"].tobytes() != b["precision"].tobytes()


# ---- run tables ------------------------------------------------------------------------------------------------------
def alternating(h, w):
    """the checkerboard of the column-major order: every pixel differs from the one before it, h * w runs"""
    return (np.arange(h * w) % 2 == 1).reshape((h, w), order="F")


def _table_masks():
    rng = np.random.default_rng(3)
    one = np.zeros((7, 9), bool)
    one[4, 5] = True
    yield "empty", np.zeros((7, 9), bool)
    yield "full", np.ones((7, 9), bool)
    yield "single pixel", one
    yield "checkerboard", alternating(24, 40)
    yield "random", rng.random((37, 53)) > 0.6


def bit_from_table(t, m, x):
    off, n = t.rows[m, 0], t.rows[m, 1]
    return np.searchsorted(t.ends[off:off + n], x, side="right") & 1


def test_runs_from_counts_against_decoded_masks():
    names, masks = zip(*_table_masks())
    counts = [rle_counts(m).tolist() for m in masks]
    assert counts[1][0] == 0 and len(counts[3]) == 24 * 40          # the full mask starts with a zero count
    zero_runs = [3, 0, 0, 2, 0, 4, 5, 0, 49]                        # zero-length runs inside a list: 7 x 9 = 63 pixels
    counts.append(zero_runs)
    sizes = [m.shape for m in masks] + [(7, 9)]
    t = V.runs_from_counts(counts, sizes)
    assert t.ends.dtype == t.ones.dtype == t.rows.dtype == np.int32
    assert t.rows[:, 1].tolist() == [len(c) for c in counts] and t.rows[:, 0].tolist() == \
        (np.cumsum([len(c) for c in counts]) - [len(c) for c in counts]).tolist()
    dense = list(masks) + [rle_decode({"size": [7, 9], "counts": counts_to_string(zero_runs)})]
    for m, d in enumerate(dense):
        flat = d.reshape(-1, order="F")
        assert t.rows[m, 2] == flat.size and t.rows[m, 3] == flat.sum()
        assert (bit_from_table(t, m, np.arange(flat.size)) == flat).all(), m
        off, n = t.rows[m, 0], t.rows[m, 1]
        ends = t.ends[off:off + n]
        assert ends[-1] == flat.size
        assert (t.ones[off:off + n] == np.concatenate(([0], np.cumsum(flat)))[ends]).all()
    with pytest.raises(ValueError, match="sum to"):
        V.runs_from_counts([[5, 5]], [(3, 3)])
    with pytest.raises(ValueError, match="negative"):
        V.runs_from_counts([[12, -3]], [(3, 3)])
    with pytest.raises(ValueError, match="2\\^31"):
        V.runs_from_counts([[1]], [(65536, 32768)])


def test_host_sums_against_dense_masks():
    rng = np.random.default_rng(8)
    h, w = 37, 53
    masks = [rng.random((h, w)) > p for p in (0.5, 0.9, 0.2, 0.7)] + [np.zeros((h, w), bool), np.ones((h, w), bool)]
    masks += [np.kron(rng.random((5, 7)) > 0.5, np.ones((8, 8), bool))[:h, :w]]
    t = V.decode_strings([rle_encode(m)["counts"] for m in masks], [(h, w)] * len(masks))
    frame_mask = [0, 1, -1, 6, 2, -1, 3, 4, 5, 6, -1, 1]        # three tracks of four frames
    tracks = [(0, 4), (4, 4), (8, 4)]
    pairs = [(0, 1), (1, 0), (0, 2), (2, 2), (1, 2)]
    sums = V.pair_sums(t, frame_mask, tracks, pairs)

    def dense(tr, f):
        m = frame_mask[tracks[tr][0] + f]
        return np.zeros((h, w), bool) if m < 0 else masks[m]
    for (d, g), s in zip(pairs, sums):
        assert s.tolist() == [sum(int((dense(d, f) & dense(g, f)).sum()) for f in range(4)),
                              sum(int(dense(d, f).sum()) for f in range(4)),
                              sum(int(dense(g, f).sum()) for f in range(4)), 0]
    iou = V.ious_from_sums(sums)
    assert iou[3] == 1.0 and 0 < iou[0] == iou[1] < 1
    assert V.ious_from_sums(np.array([[0, 0, 0, 0]], dtype=np.int64)).tolist() == [0.0]
    # statuses: tracks of different length, masks of different pixel counts
    t2 = V.concat_tables(t, V.runs_from_counts([[6, 3]], [(3, 3)]))
    bad = V.pair_sums(t2, [0, 1, 7, 2, 3], [(0, 2), (2, 1), (3, 2)], [(0, 1), (0, 2), (1, 1), (2, 1)])
    assert bad[:, 3].tolist() == [_lib.VIDEO_IOU_FRAMES, 0, 0, _lib.VIDEO_IOU_FRAMES] and (bad[0, :3] == 0).all()
    bad = V.pair_sums(t2, [0, 7], [(0, 1), (1, 1)], [(0, 1), (1, 1)])
    assert bad[:, 3].tolist() == [_lib.VIDEO_IOU_PIXELS, 0] and bad[1].tolist() == [3, 3, 3, 0]


# ---- the stand-in ----------------------------------------------------------------------------------------------------
def test_stand_in_area_and_merge_against_numpy():
    S = _tool("pycocotools_standin")
    rng = np.random.default_rng(1)
    for h, w in ((24, 40), (37, 53), (1, 7)):
        a, b = rng.random((h, w)) > 0.5, rng.random((h, w)) > 0.8
        ra, rb = rle_encode(a), rle_encode(b)
        rb["counts"] = rb["counts"].encode("ascii")            # pycocotools hands bytes around
        assert S.area(ra) == a.sum() and S.area([ra, rb]).tolist() == [a.sum(), b.sum()]
        assert S.area(ra).dtype == np.uint32
        assert (rle_decode(S.merge([ra, rb], True)) == (a & b)).all()
        assert (rle_decode(S.merge([ra, rb], False)) == (a | b)).all()
        assert (rle_decode(S.merge([ra, rb])) == (a | b)).all()
        un = S.frPyObjects({"size": [h, w], "counts": rle_counts(a).tolist()}, h, w)
        assert un == ra
        ys, xs = np.nonzero(a)
        assert S.toBbox(ra).tolist() == [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1]
    empty = rle_encode(np.zeros((5, 6), bool))
    assert S.area(empty) == 0 and S.toBbox(empty).tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        S.merge([empty, rle_encode(np.zeros((6, 5), bool))], True)


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_error_cases():
    gt, recs = golden_documents()
    poly = json.loads(json.dumps(gt))
    poly["annotations"][2]["segmentations"][1] = [[1.0, 1.0, 5.0, 1.0, 5.0, 5.0]]
    with pytest.raises(ValueError, match="annotation 3 frame 1 is a polygon"):
        YTVISEval(poly, device="cpu")
    with pytest.raises(ValueError, match="record 0 names video 99"):
        YTVISEval(gt, device="cpu").add([dict(recs[0], video_id=99)])
    wrong = dict(recs[5], segmentations=[rle_encode(np.zeros((40, 24), bool))] * len(recs[5]["segmentations"]))
    with pytest.raises(ValueError, match="mask-size mismatch: record 1 .* frame 0 is 40 x 24"):
        YTVISEval(gt, device="cpu").add([recs[0], wrong]).evaluate()
    n = len(recs[0]["segmentations"])
    h, w = recs[0]["segmentations"][0]["size"]
    for counts, why in (("\x7f" + recs[0]["segmentations"][2]["counts"][1:], "byte outside"),
                        (counts_to_string([h * w])[:-1] + "o", "ends inside a count"),
                        (counts_to_string([h * w + 5, -5]), "negative count"),
                        (counts_to_string([h * w - 1]), "do not sum")):
        segs = [dict(s) for s in recs[0]["segmentations"]]
        segs[2] = {"size": [h, w], "counts": counts}
        with pytest.raises(ValueError, match=f"malformed RLE string of record 1 .*frame 2: .*{why}"):
            YTVISEval(gt, device="cpu").add([recs[1], dict(recs[0], segmentations=segs)]).evaluate()
    short = dict(recs[0], segmentations=recs[0]["segmentations"][:n - 1])
    with pytest.raises(ValueError, match="differ in frame count"):
        YTVISEval(gt, device="cpu").add([short]).evaluate()


def test_checked_string_decode_is_string_to_counts():
    from vnext_amd.utils.ytvis_json import string_to_counts
    for _, m in _table_masks():
        s = rle_encode(m)["counts"]
        assert V.string_counts_checked(s, m.size) == (string_to_counts(s), 0)
    assert V.string_counts_checked("", 4) == ([], _lib.RLE_RUNS_BAD_SUM)
    assert V.string_counts_checked("4", 4) == ([4], 0)


# ---- the evaluator protocol ----------------------------------------------------------------------------------------------
def test_evaluator_protocol():
    gt, recs = golden_documents()
    fx = golden()
    ev = YTVISEvaluator(gt, device="cpu", area_rng=fx["area_rng"].tolist())
    for _ in range(2):                                  # reset() starts over
        ev.reset()
        for v in gt["videos"]:
            mine = [r for r in recs if r["video_id"] == v["id"]]
            inputs = [{"video_id": v["id"], "height": v["height"], "width": v["width"], "length": v["length"]}]
            if v["id"] % 2:                             # a list of records, or a model's ytvis_results-style output
                ev.process(inputs, mine)
            elif v["id"] == 4:                          # or model(inputs): bool masks, None where the track is absent
                ev.process(inputs, {"pred_scores": [r["score"] for r in mine],
                                    "pred_labels": [r["category_id"] for r in mine],
                                    "pred_masks": [[None if s is None else rle_decode(s) for s in r["segmentations"]]
                                                   for r in mine]})
            else:
                ev.process(inputs, {"pred_scores": [r["score"] for r in mine],
                                    "pred_labels": [r["category_id"] for r in mine],
                                    "pred_masks": [r["segmentations"] for r in mine]})
        out = ev.evaluate()
    assert list(out) == ["segm"]
    for n, want in zip(STAT_NAMES, fx["stats"]):
        assert out["segm"][n] == pytest.approx(want * 100, abs=1e-10), n
    assert {"AP-person", "AP-dog", "AP-car"} <= set(out["segm"])
    ev.reset()
    assert all(np.isnan(x) for x in ev.evaluate()["segm"].values())


def test_abi_declares_the_two_ops():
    assert _lib.ABI_VERSION == 17
    for name in ("vnx_rle_runs_measure", "vnx_rle_runs_write", "vnx_video_iou_sums"):
        assert name in _lib.SIGNATURES and hasattr(_lib.product_lib(), name)
