"""What is left of a training mapper when the augmentation runs on the device (vnext_amd/ops/augment.py):
read the frames, draw the random numbers, put the annotations in slot order.

`sample_plan(cfg, sizes, num_frames, rng) -> [FramePlan]`: the draws of the reference's `build_augmentation(cfg, True)` for one
clip whose source frames have `sizes` [(h, w)]:
  * INPUT.CROP.ENABLED: ONE coin per clip picks the list with the crop or the list without it (the mapper's
    `np.random.rand() > 0.5` -> no crop);
  * detectron2's RandomCrop("absolute_range", (lo, hi)), PER FRAME: ch in [min(h, lo), min(h, hi)], cw likewise, then the
    origin y0 in [0, h - ch], x0 in [0, w - cw] -- four integers, in that order; "relative" and "absolute" fix the size
    (`crop_size`) and draw the origin only;
  * ResizeShortestEdge(MIN_SIZE_TRAIN, MAX_SIZE_TRAIN, MIN_SIZE_TRAIN_SAMPLING) on the CROPPED size: "choice" / "range" draw
    a short edge per frame, "choice_by_clip" / "range_by_clip" once per clip; the target through `resize.shortest_edge_size`;
  * INPUT.RANDOM_FLIP: "horizontal" a coin (p = 0.5) per frame, "flip_by_clip" once per clip, "none" never;
  * INPUT.AUGMENTATIONS: for each of "brightness", "contrast", "saturation" that is listed, in that order, ONE
    `uniform(0.9, 1.1)` PER FRAME after the frame's other draws -- the stock detectron2 classes know nothing of clips, so the
    weights differ between the frames of a clip even under `flip_by_clip`.
It reproduces the SAME DISTRIBUTIONS, not the same random stream: the reference draws from numpy's global generator inside
detectron2's transform classes, which cannot be replayed (or checked) without detectron2; `rng` is a `numpy.random.Generator`.
Keys absent from `cfg.INPUT` take detectron2's defaults.  A cfg that asks for what the device route does not build ("rotation"
or an unknown name in INPUT.AUGMENTATIONS, a vertical flip, RandomCrop("relative_range")) raises: such a config keeps the
host mapper.

`stage_clip(frames, annotations, plan, num_classes) -> dict`: the mapper's bookkeeping that has nothing to do with pixels --
one slot per instance id of the clip (ids in order of first appearance; the reference iterates a `set`), in every frame the
dummy annotation (class `num_classes`, id -1, an empty mask) where an instance is absent, `iscrowd` annotations dropped (their
slot stays, filled with the dummy, as in the reference).  The entry of `batched_inputs` it returns holds "image" (the SOURCE
frames), "augment" (the plan) and "instances": per frame a dict with gt_classes int64 [n], gt_ids int64 [n], gt_rle (the
masks' COCO counts at SOURCE resolution, a list per slot) and image_size = (nh, nw).  A model with `device_augment` fills
gt_masks, gt_boxes and the filtered gt_ids from one `augment_masks` call for the whole step.

`stage_clip(..., polygons=True)` keeps an annotation whose `segmentation` is a list (polygons or boxes, as `frPyObjects`
takes them) as it is: the frame dict then also holds gt_poly, a list per slot -- the polygon list, or None where the slot is
RLE, whose gt_rle entry is None where the slot is a polygon -- and the dummy slot is the reference's polygon [0.0] * 6
(`_get_dummy_anno`).  The model transforms the coordinates on the host and rasterises them at the target size on the device
(vnext_amd/ops/poly_rle.py).

COCO pre-training (IDOL's `COCO_CLIP_DatasetMapper`, INPUT.COCO_PRETRAIN): `sample_coco_plan` draws the
mapper's chain flip -> [resize -> crop] -> resize per frame of the pair as `augment.ChainPlan`s, and `stage_coco_pair` makes
the pair's entry of `batched_inputs` from ONE source image and its COCO annotations.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

from ..ops import resize
from ..ops.augment import ChainPlan, FramePlan
from ..utils.ytvis_json import string_to_counts


def _get(node, key, default):
    if node is None:
        return default
    return node.get(key, default) if isinstance(node, dict) else getattr(node, key, default)


COLOR_NAMES = ("brightness", "contrast", "saturation")      # in `build_augmentation`'s order


def color_names(cfg, who: str = "sample_plan"):
    """INPUT.AUGMENTATIONS -> the colour steps it lists, in `build_augmentation`'s order; any other entry ("rotation": OpenCV's
    warpAffine, which nothing here restates) raises, naming it"""
    listed = _get(cfg.INPUT, "AUGMENTATIONS", None) or ()
    listed = (listed,) if isinstance(listed, str) else tuple(listed)
    for name in listed:
        if name not in COLOR_NAMES:
            raise ValueError("%s: INPUT.AUGMENTATIONS entry %r is not built on the device" % (who, name))
    return tuple(name for name in COLOR_NAMES if name in listed)


def crop_size(crop_type: str, size, h: int, w: int, rng):
    """detectron2's `RandomCrop.get_crop_size` for an image of h x w -> (ch, cw), with its expressions:
      "relative"        int(h * c0 + 0.5), int(w * c1 + 0.5);
      "relative_range"  the same with fractions c + rand * (1 - c), c = `size` in float32, drawn for (h, w) together;
      "absolute"        min(size, dim);
      "absolute_range"  ch in [min(h, lo), min(h, hi)], then cw likewise."""
    if crop_type == "relative":
        return int(h * size[0] + 0.5), int(w * size[1] + 0.5)
    if crop_type == "relative_range":
        lo = np.asarray(size, dtype=np.float32)
        fh, fw = lo + rng.random(2) * (1 - lo)
        return int(h * fh + 0.5), int(w * fw + 0.5)
    if crop_type == "absolute":
        return min(int(size[0]), h), min(int(size[1]), w)
    if crop_type == "absolute_range":
        ch = int(rng.integers(min(h, size[0]), min(h, size[1]) + 1))
        return ch, int(rng.integers(min(w, size[0]), min(w, size[1]) + 1))
    raise ValueError("crop_size: RandomCrop(%r)" % (crop_type,))


def _read_input(cfg, who: str, styles, crop_types=("absolute_range",), color: bool = False):
    """What both samplers read of `cfg.INPUT`, and their refusals (`who`: the sampler's name in the messages; `styles`: the
    MIN_SIZE_TRAIN_SAMPLING values it takes; `crop_types`: the RandomCrop types; `color`: INPUT.AUGMENTATIONS is the
    caller's to read) -> (crop on, crop SIZE's two values, short edges, max size, sampling, flip mode)"""
    inp = cfg.INPUT
    if not color and _get(inp, "AUGMENTATIONS", None):
        raise ValueError("%s: INPUT.AUGMENTATIONS %r are not built on the device" % (who, inp.AUGMENTATIONS))
    crop = _get(inp, "CROP", None)
    crop_on = bool(_get(crop, "ENABLED", False))
    crop_type = _get(crop, "TYPE", "relative_range")
    if crop_on and crop_type not in crop_types:
        raise ValueError("%s: RandomCrop(%r) is not built on the device (it takes %s)" % (who, crop_type, ", ".join(crop_types)))
    lo, hi = _get(crop, "SIZE", (384, 600)) if crop_on else (0, 0)
    if not crop_type.startswith("relative"):
        lo, hi = int(lo), int(hi)
    short = _get(inp, "MIN_SIZE_TRAIN", (800,))
    short = (int(short),) if isinstance(short, int) else tuple(int(s) for s in short)
    max_size = int(_get(inp, "MAX_SIZE_TRAIN", 1333))
    style = _get(inp, "MIN_SIZE_TRAIN_SAMPLING", "choice")
    flip_mode = _get(inp, "RANDOM_FLIP", "horizontal")
    if style not in styles:
        raise ValueError("%s: MIN_SIZE_TRAIN_SAMPLING %r" % (who, style))
    if flip_mode not in ("none", "horizontal", "flip_by_clip"):
        raise ValueError("%s: RANDOM_FLIP %r is not built on the device" % (who, flip_mode))
    if "range" in style:
        assert len(short) == 2, "MIN_SIZE_TRAIN must be two values with a 'range' sampling"
    return crop_on, lo, hi, short, max_size, style, flip_mode


def sample_plan(cfg, sizes, num_frames, rng):
    """-> a FramePlan per frame of one clip; see the module docstring"""
    assert len(sizes) == num_frames
    crop_on, lo, hi, short, max_size, style, flip_mode = _read_input(
        cfg, "sample_plan", ("choice", "range", "choice_by_clip", "range_by_clip"),
        crop_types=("absolute_range", "absolute", "relative"), color=True)
    crop_type = _get(_get(cfg.INPUT, "CROP", None), "TYPE", "relative_range")
    steps = color_names(cfg)

    use_crop = crop_on and not rng.random() > 0.5      # the coin per clip
    plan, size, flip = [], None, False
    for i, (h, w) in enumerate(sizes):
        x0, y0, cw, ch = 0, 0, int(w), int(h)
        if use_crop:
            ch, cw = crop_size(crop_type, (lo, hi), int(h), int(w), rng)
            y0 = int(rng.integers(h - ch + 1))
            x0 = int(rng.integers(w - cw + 1))
        if size is None or "by_clip" not in style:
            size = int(rng.integers(short[0], short[1] + 1)) if "range" in style else int(rng.choice(short))
        if flip_mode != "none" and (i == 0 or flip_mode == "horizontal"):
            flip = bool(rng.random() < 0.5)
        nh, nw = resize.shortest_edge_size(ch, cw, size, max_size)
        drawn = {name: float(rng.uniform(0.9, 1.1)) for name in steps}      # per frame, in the steps' order
        plan.append(FramePlan(x0, y0, cw, ch, nh, nw, flip, *(drawn.get(name) for name in COLOR_NAMES)))
    return plan


COCO_CROP_SHORT_EDGES = (400, 500, 600)      # the mapper's own ResizeShortestEdge in front of the crop; no maximum
_NO_MAXIMUM = sys.maxsize


def sample_coco_plan(cfg, size, rng, frames: int = 2):
    """-> a ChainPlan per frame of one COCO pre-training pair whose source image has `size` = (h, w): the draws of IDOL's
    `COCO_CLIP_DatasetMapper`.  Per frame (INPUT.PRETRAIN_SAME_CROP true: ONE draw, shared by all frames):
      * the mapper's coin: no crop when `rng.random() > 0.5`, and never with INPUT.CROP.ENABLED false;
      * RandomFlip(): a horizontal flip with p = 0.5;
      * on the crop side ResizeShortestEdge((400, 500, 600), no maximum, "choice") and RandomCrop("absolute_range",
        INPUT.CROP.SIZE) on the RESIZED size: `sample_plan`'s four integers, in its order;
      * ResizeShortestEdge(MIN_SIZE_TRAIN, MAX_SIZE_TRAIN, MIN_SIZE_TRAIN_SAMPLING) on the cropped size.
    As `sample_plan`, it reproduces the same DISTRIBUTIONS, not the same random stream: the reference draws from numpy's
    global generator inside detectron2's transform classes, which cannot be replayed (or checked) without detectron2; `rng`
    is a `numpy.random.Generator`.  Refused here: INPUT.AUGMENTATIONS (the mapper builds its own list and never reads the
    key: a config that sets it means the other mapper), a crop type other than "absolute_range", a RANDOM_FLIP it does not
    know (a vertical flip).  The mapper itself never reads RANDOM_FLIP -- it always builds
    RandomFlip() -- so every accepted value flips per frame; and its ResizeShortestEdge takes "choice" or "range" only."""
    crop_on, lo, hi, short, max_size, style, _ = _read_input(cfg, "sample_coco_plan", ("choice", "range"))
    h, w = int(size[0]), int(size[1])

    def draw():
        use_crop = crop_on and not rng.random() > 0.5
        flip = bool(rng.random() < 0.5)
        h1, w1, x0, y0, cw, ch = h, w, 0, 0, w, h
        if use_crop:
            h1, w1 = resize.shortest_edge_size(h, w, int(rng.choice(COCO_CROP_SHORT_EDGES)), _NO_MAXIMUM)
            ch = int(rng.integers(min(h1, lo), min(h1, hi) + 1))
            cw = int(rng.integers(min(w1, lo), min(w1, hi) + 1))
            y0 = int(rng.integers(h1 - ch + 1))
            x0 = int(rng.integers(w1 - cw + 1))
        edge = int(rng.integers(short[0], short[1] + 1)) if style == "range" else int(rng.choice(short))
        nh, nw = resize.shortest_edge_size(ch, cw, edge, max_size)
        return ChainPlan(h, w, flip, h1, w1, x0, y0, cw, ch, nh, nw)

    if bool(_get(cfg.INPUT, "PRETRAIN_SAME_CROP", False)):
        return [draw()] * frames
    return [draw() for _ in range(frames)]


def stage_coco_pair(image, annotations, plans, num_classes, layout: str = "chw"):
    """image: ONE uint8 source image; annotations: its COCO annotations (dicts with "category_id", "bbox" = [x, y, w, h],
    "segmentation" and optionally "iscrowd"); plans: a ChainPlan per frame of the pair -> the pair's entry of
    `batched_inputs`, as `COCO_CLIP_DatasetMapper` arranges it: "image" lists the SAME tensor once per frame (staging uploads
    it once), "augment" the plans; every frame's instance dict holds the non-crowd annotations in their order -- an
    `iscrowd` annotation is dropped and gets NO slot -- with gt_ids 1..n (the same in every frame; a model with
    `device_augment` sets -1 where the transformed box or the mask is empty), gt_classes, gt_poly (the polygon list; None
    for an RLE slot, whose counts are in gt_rle: such a step takes the host route), gt_bbox (the annotations' boxes as XYXY,
    float64 [n, 4]) and image_size = (nh, nw).  `num_classes` is unused (no dummy slot exists here); it keeps the signature
    of `stage_clip`."""
    assert len(plans) >= 1 and all(isinstance(p, ChainPlan) for p in plans)
    kept = [a for a in annotations if a.get("iscrowd", 0) == 0]
    classes = torch.tensor([int(a["category_id"]) for a in kept], dtype=torch.int64)
    bbox = np.array([[a["bbox"][0], a["bbox"][1], a["bbox"][0] + a["bbox"][2], a["bbox"][1] + a["bbox"][3]] for a in kept],
                    dtype=np.float64).reshape(len(kept), 4)
    polys = [a["segmentation"] if _is_polygons(a["segmentation"]) else None for a in kept]
    rles = [None if q is not None else _counts(a["segmentation"]) for a, q in zip(kept, polys)]
    instances = [{"gt_classes": classes, "gt_ids": torch.arange(1, len(kept) + 1, dtype=torch.int64), "gt_rle": list(rles),
                  "gt_poly": list(polys), "gt_bbox": bbox, "image_size": (p.nh, p.nw)} for p in plans]
    entry = {"image": [image] * len(plans), "augment": list(plans), "instances": instances}
    if layout != "chw":
        entry["image_layout"] = layout
    return entry


def _counts(segmentation):
    """an annotation's mask as COCO counts: a count list, an RLE dict with a count list or a compressed string, or a string"""
    if isinstance(segmentation, dict):
        segmentation = segmentation["counts"]
    if isinstance(segmentation, bytes):
        segmentation = segmentation.decode("ascii")
    if isinstance(segmentation, str):
        return [int(c) for c in string_to_counts(segmentation)]
    segmentation = list(segmentation)
    if not segmentation or any(isinstance(c, (list, tuple, np.ndarray)) for c in segmentation):
        raise ValueError("stage_clip: polygons go through frPyObjects to RLE first")
    return [int(c) for c in segmentation]


def _is_polygons(segmentation):
    """a list of polygons or of boxes (a FLAT list of numbers stays what it was: COCO counts; one box goes in as [[x, y, w, h]])"""
    return isinstance(segmentation, (list, tuple)) and (
        len(segmentation) == 0 or isinstance(segmentation[0], (list, tuple, np.ndarray)))


def stage_clip(frames, annotations, plan, num_classes, layout: str = "chw", polygons: bool = False):
    """frames: the clip's uint8 SOURCE frames; annotations: per frame a list of dicts with "id", "category_id",
    "segmentation" (COCO counts: a list, a compressed string, or an RLE dict of either; with `polygons=True` also a list of
    polygons or boxes) and optionally "iscrowd" -> the clip's entry of `batched_inputs`; see the module docstring."""
    assert len(frames) == len(annotations) == len(plan)
    slots = {}
    for annos in annotations:
        for a in annos:
            slots.setdefault(a["id"], len(slots))
    instances = []
    for f, annos, p in zip(frames, annotations, plan):
        h, w = resize.frame_size(f, layout)
        classes, ids, rles = [num_classes] * len(slots), [-1] * len(slots), [[h * w] for _ in slots]      # the dummy
        polys = [None] * len(slots)
        if polygons:                         # the reference's dummy is a polygon
            rles, polys = [None] * len(slots), [[[0.0] * 6] for _ in slots]
        for a in annos:
            if a.get("iscrowd", 0) != 0:
                continue
            s = slots[a["id"]]
            classes[s], ids[s] = int(a["category_id"]), int(a["id"])
            if polygons and _is_polygons(a["segmentation"]):
                rles[s], polys[s] = None, a["segmentation"]
            else:
                rles[s], polys[s] = _counts(a["segmentation"]), None
        instances.append({"gt_classes": torch.tensor(classes, dtype=torch.int64), "gt_ids": torch.tensor(ids, dtype=torch.int64),
                          "gt_rle": rles, "image_size": (p.nh, p.nw)})
        if polygons:
            instances[-1]["gt_poly"] = polys
    entry = {"image": list(frames), "augment": list(plan), "instances": instances}
    if layout != "chw":
        entry["image_layout"] = layout
    return entry
