"""YTVIS AP, locally: the YouTube-VIS cocoapi fork's `YTVOS.loadRes` + `YTVOSeval` (reference:
projects/InstMove/MinVIS_motion/minvis/data_video/datasets/ytvis_api/ytvos.py:218-266, ytvoseval.py:88-130, 176-190,
267-345, 347-452, 459-503, 534-545) and the evaluator protocol around it (minvis/data_video/ytvis_eval.py), for the
records `model.ytvis_results(inputs)` returns.

The evaluation is ap_eval.py's, shared with `COCOEval`; here is what YTVIS adds.  The unit is the video and a mask a
track of per-frame `segmentations`.  The video mask IoU -- the reference's Python double loop of RLE merges -- is the
quotient of integer sums over the frames (ops/video_iou.py), bit-identical to the reference's, with no crowd rule.  An
area is `avg_area`, the mean of the non-zero frame areas.  Area ranges at 128^2 and 256^2.
"""
from __future__ import annotations

import numpy as np

from .. import _lib
from ..ops import video_iou as V
from .ap_eval import STAT_NAMES, APEval, in_percent, summarize  # noqa: F401  (the tools import both names from here)


def _avg_area(areas):
    """the reference's `avg_area`: the mean of the non-zero frame areas, 0 if none"""
    l = [a for a in areas if a]
    return np.array(l).mean() if l else 0


class YTVISEval(APEval):
    """`YTVISEval(gt).add(records)`, then `.evaluate()` -> the numbers of YTVOSeval.evaluate / accumulate / summarize,
    "eval_vids" (the reference's `evalImgs`) always among them.

    gt: `videos`, `categories`, `annotations` with per-frame `segmentations` (uncompressed RLE, compressed RLE, None or,
    with polygons=True, a list), `areas` and `iscrowd`.  records: what `model.ytvis_results(inputs)` returns ({"video_id",
    "score", "category_id", "segmentations"}).  The other parameters are `APEval`'s, but for the matching's default:
    `match_host`, also on a CUDA device; device_matching=True on a CUDA device means matching="device" (without a device
    it is silently off).  The results of the three routes are identical.
    """
    UNIT, EVAL_KEY, FRAMES = "video", "eval_vids", True
    AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 128 ** 2], [128 ** 2, 256 ** 2], [256 ** 2, 1e5 ** 2]]
    STATUS_TEXT = {_lib.VIDEO_IOU_FRAMES: "differ in frame count",
                   _lib.VIDEO_IOU_PIXELS: "have masks of different sizes in one frame (mask-size mismatch)"}

    def __init__(self, gt, device=None, iou_thrs=None, rec_thrs=None, max_dets=(1, 10, 100), area_rng=None,
                 device_matching=False, polygons=False, matching=None):
        self._device_matching = bool(device_matching)
        super().__init__(gt, device, iou_thrs, rec_thrs, max_dets, area_rng, matching, polygons)

    def _default_matching(self, device):
        return "device" if self._device_matching and self.device is not None else "host"

    def evaluate(self):
        return super().evaluate(eval_imgs=True)

    def _masks_of(self, items):
        tracks = [x["segmentations"] for x in items]
        return [seg for track in tracks for seg in track], [len(track) for track in tracks]

    def _size_of(self, seg, video, *where):
        if seg.get("size") is None:
            seg = dict(seg, size=[video["height"], video["width"]])
        return super()._size_of(seg, video, *where)

    def _gt_area(self, ann):
        return _avg_area(ann["areas"])                      # per annotation: numpy's `mean` owns its summation order

    def _dt_areas(self, area, frame_mask, rows):
        # loadRes: the areas of the present masks as pycocotools gives them (uint32), None for absent frames
        masks = [frame_mask[first:first + frames] for first, frames in rows.tolist()]
        return np.array([_avg_area(list(area[m[m >= 0]].astype(np.uint32))) for m in masks], dtype=np.float64)

    def _ious_from_sums(self, sums, crowd):
        return V.ious_from_sums(sums)


class YTVISEvaluator:
    """The reference evaluators' protocol (`reset()` / `process(inputs, outputs)` / `evaluate()`) around `YTVISEval`,
    without detectron2.

    `outputs` is a model's output dict -- `model.ytvis_results`-style, "pred_masks" holding RLE dicts (through
    `utils.ytvis_json.ytvis_records`), or `model(inputs)` with mask arrays (through `instances_to_coco_json_video`) -- or
    a list of result records.  `evaluate()` returns {"segm": {...}}: the numbers of `summarize` in percent under the
    reference's names (NaN where the reference has -1: `_derive_coco_results`; AR100 / ARs / ARm / ARl beside the
    eight it lists) and "AP-<category>" per category when there is more than one.

    The evaluator scores the records this process has seen.  Gathering records across ranks stays the caller's
    `gather_object` (call `process(None, gathered_records)` on the main rank, or merge the lists before `evaluate`).
    """

    def __init__(self, gt, device=None, **params):
        self._args = (gt, device, params)
        self.reset()

    def reset(self):
        gt, device, params = self._args
        self._eval = YTVISEval(gt, device=device, **params)
        self._args = (self._eval.gt, device, params)            # a path is read once

    def process(self, inputs, outputs):
        from ..utils.ytvis_json import instances_to_coco_json_video, ytvis_records
        if isinstance(outputs, dict):
            first = next((m for track in outputs["pred_masks"] for m in track if m is not None), None)
            outputs = ytvis_records(inputs, outputs) if isinstance(first, dict) \
                else instances_to_coco_json_video(inputs, outputs)
        self._eval.add(outputs)

    def evaluate(self):
        if not self._eval.records:
            return {"segm": in_percent(None, STAT_NAMES)}
        self.results = self._eval.evaluate()
        return {"segm": in_percent(self.results, STAT_NAMES)}
