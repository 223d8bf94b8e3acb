"""COCO AP (bbox, segm), locally: `COCO.loadRes` + `COCOeval.evaluate / accumulate / summarize` for the records
`IDOL.coco_results(images)` returns, and the `COCOEvaluator` protocol of the reference's COCO-pretrain stage
(detectron2/evaluation/coco_evaluation.py) around it, without pycocotools or detectron2.

The evaluation is ap_eval.py's, shared with `YTVISEval`; here is what COCO adds.  The unit is the image and a mask a
track of one frame.  `area` is the annotation's for ground truth; w * h of a result box for "bbox", the mask's pixel
count for "segm", whatever `bbox` a record carries.  Area ranges at 32^2 and 96^2.  IoU, in float64: box  w = min(dx +
dw, gx + gw) - max(dx, gx), h likewise, 0 if w <= 0 or h <= 0, else i = w * h and u = crowd ? d_area : d_area + g_area
- i;  mask  i = the intersection's pixel count, u = crowd ? area(dt) : area(dt) + area(gt) - i.  The quotient is one
IEEE double division on the host, 0 where u is 0.
"""
from __future__ import annotations

import time

import numpy as np

from .ap_eval import STAT_NAMES, APEval, in_percent, load_json


class COCOEval(APEval):
    """`COCOEval(gt, iou_type).add(records)`, then `.evaluate()` -> the numbers of COCOeval.evaluate / accumulate /
    summarize.

    gt: `images`, `categories`, `annotations` with `bbox` (xywh), `area`, `iscrowd` and, for "segm", `segmentation` as
    an RLE dict (compressed or not) or, with polygons=True, a list (COCO's polygon areas differ from pixel counts, and
    COCOeval uses the stated one); "bbox" ignores the segmentation.  iou_type: "bbox" or "segm".  records: what
    `IDOL.coco_results(images)` returns ({"image_id", "category_id", "score", "bbox" xywh and / or "segmentation" RLE}).
    The other parameters are `APEval`'s: without `matching`, a CUDA device takes the kernel, device="cpu" `match_host`,
    and device=None without a device `match_vectorised`.  `evaluate(eval_imgs=True)` adds "eval_imgs".
    """
    UNIT, EVAL_KEY = "image", "eval_imgs"
    AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]

    def __init__(self, gt, iou_type, device=None, iou_thrs=None, rec_thrs=None, max_dets=(1, 10, 100), area_rng=None,
                 matching=None, polygons=False):
        if iou_type not in ("bbox", "segm"):
            raise ValueError(f"COCOEval: iou_type {iou_type!r} (bbox or segm; keypoints are out of scope)")
        self.iou_type, self.need = iou_type, "bbox" if iou_type == "bbox" else "segmentation"
        super().__init__(gt, device, iou_thrs, rec_thrs, max_dets, area_rng, matching, polygons)
        if iou_type == "segm":
            for ann in self.gt.get("annotations") or []:
                seg = ann.get("segmentation")
                if not isinstance(seg, dict) and not (isinstance(seg, list) and seg):
                    raise ValueError(f"COCOEval: annotation {ann.get('id')} has no RLE segmentation")

    def _masks_of(self, items):
        return [x.get("segmentation") for x in items], [1] * len(items)

    def _gt_area(self, ann):
        return ann["area"]

    def _dt_areas(self, area, frame_mask, rows):
        return area[frame_mask[rows[:, 0]]].astype(np.float64)

    def _ious_from_sums(self, sums, crowd):
        i = sums[:, 0].astype(np.float64)
        u = np.where(crowd != 0, sums[:, 1], sums[:, 1] + sums[:, 2] - sums[:, 0]).astype(np.float64)
        return np.divide(i, u, out=np.zeros(len(i), dtype=np.float64), where=u > 0)

    def _ious(self, g, d, di, gi):
        if self.iou_type == "segm":
            return super()._ious(g, d, di, gi)
        gb = np.array([a["bbox"] for a in g["ann"]], dtype=np.float64).reshape(-1, 4)
        db = np.array([r["bbox"] for r in d["rec"]], dtype=np.float64).reshape(-1, 4)
        d_area = db[:, 2] * db[:, 3]
        a, b = db[di], gb[gi]
        w = np.minimum(a[:, 0] + a[:, 2], b[:, 0] + b[:, 2]) - np.maximum(a[:, 0], b[:, 0])
        h = np.minimum(a[:, 1] + a[:, 3], b[:, 1] + b[:, 3]) - np.maximum(a[:, 1], b[:, 1])
        hit = (w > 0) & (h > 0)
        i = np.where(hit, w * h, 0.0)
        u = np.where(g["crowd"][gi] != 0, d_area[di], d_area[di] + gb[gi, 2] * gb[gi, 3] - i)
        return np.divide(i, u, out=np.zeros(len(i), dtype=np.float64), where=hit & (u > 0)), d_area, 0, time.perf_counter()


class COCOEvaluator:
    """detectron2's `COCOEvaluator` protocol (`reset()` / `process(inputs, outputs)` / `evaluate()`) around `COCOEval`.

    `outputs` is `model(inputs)`'s [{"instances": {"pred_boxes" xyxy, "scores", "pred_classes", "pred_masks"}}] of the
    COCO branch (boxes go to xywh, masks through `utils.ytvis_json.rle_encode`; `category_ids[class]` is the dataset's
    category id, the class index itself when None), or a list of `coco_results` records.  `evaluate()` returns {"bbox":
    {...}, "segm": {...}} in percent under detectron2's names (AP, AP50, AP75, APs, APm, APl, NaN where the reference has
    -1, and "AP-<name>" per category when there is more than one); "segm" is absent when no record carries a mask
    (MASK_ON false).  Gathering records across ranks stays the caller's `gather_object`.
    """
    NAMES = STAT_NAMES[:6]

    def __init__(self, gt, device=None, category_ids=None, **params):
        self._args = (load_json(gt), device, params)
        self.category_ids = category_ids
        self.reset()

    def reset(self):
        self.records = []

    def process(self, inputs, outputs):
        from ..utils.ytvis_json import rle_encode
        if not (len(outputs) and isinstance(outputs[0], dict) and "instances" in outputs[0]):
            self.records.extend(outputs)
            return
        host = lambda x: np.asarray(x.cpu() if hasattr(x, "cpu") else x)                 # noqa: E731
        for b, (x, o) in enumerate(zip(inputs, outputs)):
            inst = o["instances"]
            boxes = host(inst["pred_boxes"]).reshape(-1, 4).astype(np.float64)
            masks = host(inst["pred_masks"]) if inst.get("pred_masks") is not None else None
            for i, (score, label) in enumerate(zip(host(inst["scores"]).tolist(), host(inst["pred_classes"]).tolist())):
                x0, y0, x1, y1 = boxes[i].tolist()
                rec = {"image_id": x.get("image_id", b), "score": float(score), "bbox": [x0, y0, x1 - x0, y1 - y0],
                       "category_id": int(label) if self.category_ids is None else self.category_ids[int(label)]}
                if masks is not None:
                    rec["segmentation"] = rle_encode(masks[i])
                self.records.append(rec)

    def evaluate(self):
        gt, device, params = self._args
        types = ["bbox"] + (["segm"] if any("segmentation" in r for r in self.records) else [])
        if not self.records:
            return {"bbox": in_percent(None, self.NAMES)}
        out, self.results = {}, {}
        for iou_type in types:
            res = COCOEval(gt, iou_type, device=device, **params).add(self.records).evaluate()
            out[iou_type], self.results[iou_type] = in_percent(res, self.NAMES), res
        return out
