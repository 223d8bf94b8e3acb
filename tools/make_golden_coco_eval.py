"""Write tests/golden/coco_eval.npz: a small synthetic COCO annotation set and result records, scored for "bbox" and
"segm" by the reference's own matching, accumulation and summary.

The reference scores its COCO-pretrain stage with pycocotools' COCOeval, which is not on this machine.  Its YouTube-VIS
fork of that evaluator (projects/InstMove/MinVIS_motion/minvis/data_video/datasets/ytvis_api: `YTVOS.loadRes` +
`YTVOSeval`) is, and is the same code for everything but the IoU, so the set is presented to it as one-frame videos
(tools/make_golden_ytvis_eval.py's stand-ins for `pycocotools.mask`, `np.float` and matplotlib).  A subclass made here
replaces only `computeIoU`, with the two COCO IoUs in float64 numpy -- on dense decoded masks and on the box formula,
independent of the run-length code under test:

    box   w = min(dx + dw, gx + gw) - max(dx, gx), h likewise; 0 if w <= 0 or h <= 0; i = w * h
    mask  i = |d & g|
    u = crowd ? area(d) : area(d) + area(g) - i;  iou = i / u, 0 where u is 0

The fork's `loadRes` has no box branch, so for "bbox" the detections' area is set to w * h here.  The fixture holds data
only: the two JSON documents as strings, every `ious[(image, category)]`, per `evalImgs` entry `dtMatches` / `gtMatches`
/ `dtIgnore` / `gtIgnore`, `precision`, `recall`, `scores`, `stats` for both IoU types, and the area ranges used.

    python tools/make_golden_coco_eval.py [--vnext /root/reference] [--out tests/golden/coco_eval.npz]
"""
from __future__ import annotations

import argparse
import contextlib
import copy
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_golden_ytvis_eval import ellipse, reference_modules  # noqa: E402
from vnext_amd.utils.ytvis_json import rle_counts, rle_decode, rle_encode  # noqa: E402

# COCO's area ranges (32^2, 96^2 for images of about 480 x 640) scaled to images of 24 x 40 and 37 x 53
AREA_RNG = [[0, 1e5 ** 2], [0, 60], [60, 250], [250, 1e5 ** 2]]
IMAGES = [(1, 24, 40), (2, 37, 53), (3, 24, 40), (4, 37, 53), (5, 24, 40), (6, 37, 53)]              # id, height, width
CATEGORIES = [(1, "person"), (2, "dog"), (3, "car")]
# ground truth: image, category, shape ("e", cy, cx, ry, rx) or ("r", y0, x0, y1, x1), crowd, uncompressed, area (None =
# the pixel count; a number = what the annotation states, as COCO's polygon areas differ from the mask's)
OBJECTS = [
    (1, 1, ("e", 8, 8, 4, 5), 0, False, None),
    (1, 1, ("e", 14, 28, 7, 9), 0, True, None),
    (1, 2, ("e", 12, 20, 10, 16), 0, False, None),
    (2, 1, ("e", 18, 24, 14, 18), 0, False, None),
    (2, 1, ("r", 2, 30, 30, 52), 1, True, None),            # the crowd: two detections lie inside it
    (2, 2, ("e", 30, 8, 4, 4), 0, False, 58.5),             # stated area below the small / medium boundary's 60
    (2, 3, ("e", 12, 12, 9, 9), 0, True, None),
    (3, 1, ("r", 4, 4, 12, 14), 0, False, None),            # two overlapping boxes and a detection midway: equal IoU
    (3, 1, ("r", 4, 6, 12, 16), 0, False, None),
    (3, 3, ("r", 14, 20, 22, 28), 0, False, None),          # 8 x 8: a detection on its half (0.5) and on all of it (1.0)
    (4, 1, ("e", 20, 26, 15, 17), 0, True, None),
    (4, 2, ("r", 5, 5, 11, 15), 0, False, None),            # 6 x 10 = 60: on the boundary, inside both ranges
    (4, 3, ("e", 28, 40, 4, 5), 0, False, None),
    (5, 1, ("r", 2, 2, 12, 27), 0, False, 250.0),           # stated area exactly on the medium / large boundary
    (5, 2, ("e", 12, 30, 6, 7), 0, False, None),
    (6, 1, ("e", 18, 20, 12, 14), 0, False, None),
    (6, 3, ("e", 10, 40, 7, 8), 1, False, None),
    (6, 3, ("e", 26, 12, 6, 9), 0, True, None),
]
NO_DETECTIONS = {(4, 3)}                 # an (image, category) with ground truth and no detection
ONLY_DETECTIONS = (5, 3)                 # and one the other way round
CROWDED = (1, 1)                         # the (image, category) that gets 103 detections
SIZES = {v: (h, w) for v, h, w in IMAGES}


def shape_mask(v, shape, dy=0.0, dx=0.0, scale=1.0):
    h, w = SIZES[v]
    if shape[0] == "e":
        return ellipse(h, w, shape[1] + dy, shape[2] + dx, shape[3] * scale, shape[4] * scale)
    m = np.zeros((h, w), bool)
    m[shape[1]:shape[3], shape[2]:shape[4]] = True
    return m


def tight_box(mask):
    ys, xs = np.nonzero(mask)
    if not len(ys):
        return [0.0, 0.0, 0.0, 0.0]
    return [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]


def build_dataset():
    """-> (annotation dict, result records): plain JSON-able Python, COCO's format"""
    rng = np.random.default_rng(21)
    gt = {"images": [{"id": v, "height": h, "width": w} for v, h, w in IMAGES],
          "categories": [{"id": c, "name": n} for c, n in CATEGORIES], "annotations": []}
    records = []

    def record(v, c, score, mask, box=None):
        records.append({"image_id": v, "category_id": c, "bbox": tight_box(mask) if box is None else box,
                        "score": score, "segmentation": rle_encode(mask)})

    for i, (v, c, shape, crowd, uncompressed, area) in enumerate(OBJECTS):
        h, w = SIZES[v]
        m = shape_mask(v, shape)
        seg = {"size": [h, w], "counts": [int(x) for x in rle_counts(m)]} if uncompressed else rle_encode(m)
        gt["annotations"].append({"id": i + 1, "image_id": v, "category_id": c, "iscrowd": crowd, "segmentation": seg,
                                  "bbox": tight_box(m), "area": float(m.sum()) if area is None else area})
        if (v, c) in NO_DETECTIONS or crowd or shape[0] == "r":
            continue
        radii = np.array(shape[3:5], dtype=np.float64)
        for j in range(5):                               # detections around the object, from tight to loose
            spread = 0.12 * (j + 1)
            dy, dx = (rng.uniform(-1, 1, 2) * spread * radii).tolist()
            scale = float(1 + rng.uniform(-1, 1) * spread * 0.5)
            score = float(np.round(0.95 - 0.1 * j + rng.uniform(-0.15, 0.15), 2))
            record(v, c, score, shape_mask(v, shape, dy, dx, scale))
    # the crowd of image 2: two detections inside it (crowd IoU 1.0 each), far from the image's regular person
    record(2, 1, 0.81, shape_mask(2, ("r", 4, 32, 12, 40)))
    record(2, 1, 0.64, shape_mask(2, ("r", 16, 40, 28, 50)))
    # image 3, persons: a detection midway between two ground truths, and one on the first
    record(3, 1, 0.9, shape_mask(3, ("r", 4, 5, 12, 15)))
    record(3, 1, 0.8, shape_mask(3, ("r", 4, 4, 12, 14)))
    # image 3, cars: IoU exactly 1.0, exactly 0.5 (half of the 8 x 8 square), and an empty mask with an empty box
    record(3, 3, 0.7, shape_mask(3, ("r", 14, 20, 22, 28)))
    record(3, 3, 0.9, shape_mask(3, ("r", 14, 20, 22, 24)))
    record(3, 3, 0.5, np.zeros(SIZES[3], bool))
    # image 4, dogs: the ground truth of area 60; detections of area 60 (6 x 10, shifted) and 250 (10 x 25)
    record(4, 2, 0.85, shape_mask(4, ("r", 5, 6, 11, 16)))
    record(4, 2, 0.3, shape_mask(4, ("r", 20, 5, 30, 30)))
    # image 5, persons: the ground truth whose stated area is 250; a detection whose box is not its mask's (the segm
    # area is the mask's pixel count, whatever the box says)
    record(5, 1, 0.88, shape_mask(5, ("r", 2, 2, 12, 27)))
    record(5, 1, 0.42, shape_mask(5, ("r", 3, 4, 12, 26)), box=[1.0, 1.0, 30.0, 14.0])
    # false positives in every image; one (image, category) without ground truth
    for v, h, w in IMAGES:
        for j in range(4):
            c = int(rng.integers(1, 4)) if (v, j) != (ONLY_DETECTIONS[0], 0) else ONLY_DETECTIONS[1]
            if (v, c) in NO_DETECTIONS:
                c = 1
            shape = ("e", float(rng.uniform(4, h - 4)), float(rng.uniform(4, w - 4)), float(rng.uniform(2, h / 3)),
                     float(rng.uniform(2, w / 3)))
            record(v, c, float(np.round(rng.uniform(0.05, 0.7), 2)), shape_mask(v, shape))
    # one (image, category) with 103 detections in all, most of them low-score noise around its two objects
    v, c = CROWDED
    have = sum(1 for r in records if (r["image_id"], r["category_id"]) == CROWDED)
    for j in range(103 - have):
        o = OBJECTS[j % 2]
        dy, dx = (rng.uniform(-1.2, 1.2, 2) * np.array(o[2][3:5])).tolist()
        record(v, c, float(np.round(rng.uniform(0.01, 0.45), 2)), shape_mask(v, o[2], dy, dx, float(rng.uniform(0.6, 1.4))))
    records[1]["score"] = records[0]["score"]            # two detections of one group with equal scores
    return gt, records


def as_videos(gt, records):
    """The COCO documents as the fork's one-frame videos: what `YTVOS` / `loadRes` read"""
    vgt = {"videos": [{"id": v["id"], "height": v["height"], "width": v["width"], "length": 1} for v in gt["images"]],
           "categories": copy.deepcopy(gt["categories"]),
           "annotations": [{"id": a["id"], "video_id": a["image_id"], "category_id": a["category_id"],
                            "iscrowd": a["iscrowd"], "segmentations": [copy.deepcopy(a["segmentation"])],
                            "bboxes": [list(a["bbox"])], "areas": [a["area"]], "avg_area": a["area"]}
                           for a in gt["annotations"]]}
    vdt = [{"video_id": r["image_id"], "category_id": r["category_id"], "score": r["score"],
            "segmentations": [copy.deepcopy(r["segmentation"])], "bboxes": [list(r["bbox"])]} for r in records]
    return vgt, vdt


def coco_ious(dt, gt, iou_type):
    """float64 [D, G]: the two COCO IoUs on dense masks / on boxes (the module docstring's formulas)"""
    out = np.zeros((len(dt), len(gt)), dtype=np.float64)
    for i, d in enumerate(dt):
        for j, g in enumerate(gt):
            crowd = bool(g["iscrowd"])
            if iou_type == "segm":
                a, b = rle_decode_any(d["segmentations"][0]), rle_decode_any(g["segmentations"][0])
                inter, da, ga = float((a & b).sum()), float(a.sum()), float(b.sum())
            else:
                (dx, dy, dw, dh), (gx, gy, gw, gh) = (np.float64(x) for x in d["bboxes"][0]), \
                    (np.float64(x) for x in g["bboxes"][0])
                w = min(dx + dw, gx + gw) - max(dx, gx)
                h = min(dy + dh, gy + gh) - max(dy, gy)
                inter, da, ga = (0.0 if w <= 0 or h <= 0 else float(w * h)), float(dw * dh), float(gw * gh)
            u = da if crowd else da + ga - inter
            out[i, j] = inter / u if u > 0 and inter > 0 else 0.0
    return out


def rle_decode_any(seg):
    import pycocotools_standin as S
    h, w = seg["size"]
    return S._flat(seg).reshape((h, w), order="F").astype(bool)


def run_reference(vnext, gt, records, iou_type):
    """-> the fork's evaluator object after evaluate / accumulate / summarize"""
    vgt, vdt = as_videos(gt, records)
    with reference_modules(vnext) as (ytvos, ytvoseval), contextlib.redirect_stdout(io.StringIO()):
        class CocoIoU(ytvoseval.YTVOSeval):
            def computeIoU(self, vidId, catId):
                p = self.params
                g, d = self._gts[vidId, catId], self._dts[vidId, catId]
                if len(g) == 0 and len(d) == 0:
                    return []
                inds = np.argsort([-x["score"] for x in d], kind="mergesort")
                d = [d[i] for i in inds][:p.maxDets[-1]]
                return coco_ious(d, g, p.iouType)

        api = ytvos.YTVOS()
        api.dataset = vgt
        api.createIndex()
        res = api.loadRes(vdt)
        if iou_type == "bbox":                           # the fork's loadRes has no box branch: area = w * h
            for ann in res.dataset["annotations"]:
                ann["avg_area"] = float(np.float64(ann["bboxes"][0][2]) * np.float64(ann["bboxes"][0][3]))
        E = CocoIoU(api, res, iouType=iou_type)
        E.params.areaRng = copy.deepcopy(AREA_RNG)
        E.params.maxDets = [1, 10, 100]
        E.evaluate()
        E.accumulate()
        E.summarize()
    return E


def generate(vnext):
    """-> the fixture as a dict of arrays"""
    gt, records = build_dataset()
    gt_json, dt_json = json.dumps(gt), json.dumps(records)
    fx = {"gt_json": np.array(gt_json), "dt_json": np.array(dt_json), "area_rng": np.array(AREA_RNG, dtype=np.float64)}
    for iou_type in ("bbox", "segm"):
        E = run_reference(vnext, json.loads(gt_json), json.loads(dt_json), iou_type)
        fx["img_ids"] = np.array(E.params.vidIds, dtype=np.int64)
        fx["cat_ids"] = np.array(E.params.catIds, dtype=np.int64)
        for (v, c), iou in E.ious.items():
            fx[f"{iou_type}_ious_{v}_{c}"] = np.zeros(0) if isinstance(iou, list) else np.asarray(iou, dtype=np.float64)
        fx[f"{iou_type}_eval_none"] = np.array([e is None for e in E.evalImgs])
        for n, e in enumerate(E.evalImgs):
            if e is not None:
                fx[f"{iou_type}_ev{n}_dtm"] = np.asarray(e["dtMatches"], dtype=np.float64)
                fx[f"{iou_type}_ev{n}_gtm"] = np.asarray(e["gtMatches"], dtype=np.float64)
                fx[f"{iou_type}_ev{n}_dtig"] = np.asarray(e["dtIgnore"], dtype=bool)
                fx[f"{iou_type}_ev{n}_gtig"] = np.asarray(e["gtIgnore"], dtype=np.int64)
        for k in ("precision", "recall", "scores"):
            fx[f"{iou_type}_{k}"] = np.asarray(E.eval[k], dtype=np.float64)
        fx[f"{iou_type}_stats"] = np.asarray(E.stats, dtype=np.float64)
    return fx


def fixture_conditions(fx):
    """What the fixture must exercise -> {condition: bool}; checked here and asserted again by the test."""
    gt, recs = json.loads(str(fx["gt_json"])), json.loads(str(fx["dt_json"]))
    rng = fx["area_rng"]
    groups_gt, groups_dt = {}, {}
    for a in gt["annotations"]:
        groups_gt.setdefault((a["image_id"], a["category_id"]), []).append(a)
    for r in recs:
        groups_dt.setdefault((r["image_id"], r["category_id"]), []).append(r)
    imgs, cats = fx["img_ids"].tolist(), fx["cat_ids"].tolist()
    crowd_ids = [a["id"] for a in gt["annotations"] if a["iscrowd"]]
    cond = {}
    for t in ("bbox", "segm"):
        ious = [fx[f"{t}_ious_{v}_{c}"] for v in imgs for c in cats]
        flat = np.concatenate([i.reshape(-1) for i in ious])
        dtm = [fx[k] for k in fx if k.startswith(f"{t}_ev") and k.endswith("_dtm")]
        cond[f"{t}: 0.2 < AP < 0.9"] = bool(0.2 < fx[f"{t}_stats"][0] < 0.9)
        cond[f"{t}: every AP and AR of the summary is defined"] = bool((fx[f"{t}_stats"] > -1).all())
        cond[f"{t}: a crowd ground truth that two detections match"] = any(
            ((m[0] == c).sum() >= 2) for m in dtm for c in crowd_ids)
        cond[f"{t}: IoUs exactly 0.5 and exactly 1.0"] = bool((flat == 0.5).any() and (flat == 1.0).any())
        cond[f"{t}: a detection with two ground truths at equal IoU >= 0.5"] = any(
            i.ndim == 2 and i.shape[1] >= 2 and ((i[:, 0] == i[:, 1]) & (i[:, 0] >= 0.5)).any() for i in ious)
    areas_d = [float(rle_decode(r["segmentation"]).sum()) for r in recs]
    boxes_d = [r["bbox"][2] * r["bbox"][3] for r in recs]
    areas_g = [a["area"] for a in gt["annotations"]]
    edges = (rng[1][1], rng[2][1])
    for name, areas in (("ground truths", areas_g), ("detections (mask)", areas_d), ("detections (box)", boxes_d)):
        cond[f"{name} on both sides of the area boundaries"] = all(
            any(x < e for x in areas) and any(x > e for x in areas) for e in edges)
    cond["areas exactly on a boundary"] = all(e in areas_g for e in edges) and all(e in areas_d for e in edges)
    cond["a stated area that differs from the mask's"] = any(
        a["area"] != float(rle_decode_any(a["segmentation"]).sum()) for a in gt["annotations"])
    cond["ground truth without detections"] = any(k not in groups_dt for k in groups_gt)
    cond["detections without ground truth"] = any(k not in groups_gt for k in groups_dt)
    cond["103 detections in a group"] = any(len(v) == 103 for v in groups_dt.values())
    cond["equal scores in a group"] = any(len({r["score"] for r in v}) < len(v) for v in groups_dt.values())
    cond["an empty predicted mask"] = any(a == 0 for a in areas_d)
    cond["every record carries bbox and segmentation"] = all("bbox" in r and "segmentation" in r for r in recs)
    cond["a record whose box is not its mask's"] = any(
        r["bbox"] != tight_box(rle_decode(r["segmentation"])) for r in recs)
    cond["uncompressed and compressed ground truth"] = len({isinstance(a["segmentation"]["counts"], list)
                                                            for a in gt["annotations"]}) == 2
    cond["6 images of two sizes, 3 categories"] = len(gt["images"]) == 6 and len(gt["categories"]) == 3 and \
        {(v["height"], v["width"]) for v in gt["images"]} == {(24, 40), (37, 53)}
    return cond


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vnext", default="/root/reference", help="root of a VNext checkout (the reference)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "coco_eval.npz"))
    a = ap.parse_args()
    fx = generate(a.vnext)
    cond = fixture_conditions(fx)
    for k, ok in cond.items():
        print(("ok   " if ok else "FAIL ") + k)
    for t in ("bbox", "segm"):
        print(t, "stats", np.round(fx[f"{t}_stats"], 4).tolist())
    if not all(cond.values()):
        raise SystemExit("the fixture does not meet its conditions; nothing written")
    np.savez_compressed(a.out, **fx)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
