"""From a list of frames to what the backbone and the transformer are fed, and the graph caches around the trunks: the part
of SeqFormer and IDOL that does not differ between them, once.  Plain functions; a model hands in its own numbers and its own
tail (`_clip_trunk_tail`, `_chunk_trunk`, `_train_trunk`), and nothing here asks which model is calling.

  pad_normalise            a same-sized float stack -> (x, mask): the expression the training and inference graphs capture
  pad_normalise_list       float frames of unequal sizes -> (x, mask), frame by frame
  ingest_staged / resize_staged      staged uint8 frames / resize sources -> (x, mask, table): one launch of the op
  augment_staged, augment_step, host_augmented       `device_augment`: a training step's source frames and run-length ground
                           truth -> (x, mask, table) and filled instance dicts; the host route of the same plan
  preprocess               a list of frames -> (x, mask) or (x, mask, table): what both `_preprocess` are
  level_inputs             the pyramid levels' padding masks and sine positions
  stage_chunk              the frames of one inference call -> `StagedFrames`, or None for the eager list path
  replay_captured          the inference hipGraph cache: capture on a miss, copy in, replay
  TrainTrunk, graphed_callable       the training trunk as a module, and its forward + backward hipGraphs
  front_end_state, plan_resize       what a model's `__init__` derives from the cfg; the `device_resize` planning of a video
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from ..ops import augment, ingest, poly_rle, resize
from ..ops.fused_norm import step_scope
from ..ops.ingest import sine_position


def front_end_state(cfg, short_edge):
    """-> (pixel statistics as host floats ([3], [3]): what the ingest kernels take; (MIN_SIZE_TEST, MAX_SIZE_TEST) with the
    model's own default short edge; the empty inference-graph cache; the empty training-trunk cache)"""
    stats = ([float(v) for v in cfg.MODEL.PIXEL_MEAN], [float(v) for v in cfg.MODEL.PIXEL_STD])
    test_size = (int(getattr(cfg.INPUT, "MIN_SIZE_TEST", short_edge)), int(getattr(cfg.INPUT, "MAX_SIZE_TEST", 1333)))
    return stats, test_size, {}, {}


def front_end(model):
    """what `preprocess` and `stage_chunk` take after the frames, read off a model NOW (the switch is flipped and the buffers
    move after construction): (device_ingest, device, pixel statistics as host floats, pixel mean and std buffers, backbone)"""
    return (model.device_ingest, model.device, model._pixel_stats, model.pixel_mean, model.pixel_std,
            model.detr.detr.backbone)


def plan_resize(on, video, test_size, device):
    """`device_resize` for one video dict -> (frames, (targets, layout) or None, the first source frame's size or None); see
    `resize.plan_video`.  `on` false (the switch is off, or training mode): the frames untouched."""
    frames = list(video["image"])
    if not on:
        return frames, None, None
    return resize.plan_video(frames, video.get("image_layout", "chw"), *test_size, device)


# ---- frames -> (x, mask[, table]) -------------------------------------------------------------------------------------------
def pad_normalise(stack, mean, std):
    """[B, 3, h, w] raw float frames -> (x [B, 3, H, W] normalised, zero-padded to multiples of 32; mask bool [B, H, W], True
    on the padding).  Shape-static and free of host synchronisation: the form the graphs capture."""
    h, w = stack.shape[-2:]
    H, W = (h + 31) // 32 * 32, (w + 31) // 32 * 32
    x = stack.new_zeros(stack.shape[0], 3, H, W)
    x[:, :, :h, :w] = (stack - mean) / std
    mask = torch.ones(stack.shape[0], H, W, dtype=torch.bool, device=stack.device)
    mask[:, :h, :w] = False
    return x, mask


def pad_normalise_list(frames, mean, std, device):
    """`pad_normalise` for frames of unequal sizes, frame by frame (seqformer.py:413-429, idol.py:473-482,
    util/misc.py:298-302)."""
    frames = [(f.to(device, torch.float32) - mean) / std for f in frames]
    H, W = ingest.padded_size(frames)
    x = frames[0].new_zeros(len(frames), 3, H, W)
    mask = torch.ones(len(frames), H, W, dtype=torch.bool, device=device)
    for i, f in enumerate(frames):
        x[i, :, :f.shape[-2], :f.shape[-1]] = f
        mask[i, :f.shape[-2], :f.shape[-1]] = False
    return x, mask


def ingest_staged(pixels, table, B, H, W, stats, backbone):
    """staged uint8 frames -> (x, mask, table): one launch; channels-last exactly where the backbone would convert (the
    ResNet trunk in a training step with the switch on; the Swin backbone has no such method: never)"""
    asks = getattr(backbone, "wants_channels_last", None)
    nhwc = bool(pixels.is_cuda and asks is not None and asks())
    x, mask = ingest.ingest_frames(pixels, table, B, H, W, *stats, channels_last=nhwc)
    return x, mask, table


def resize_staged(pixels, src_table, dst_table, coeffs, B, H, W, layout, stats):
    """staged uint8 SOURCE frames -> (x, mask, table) of the frames resized to the targets in dst_table: one launch
    (eval mode only: never channels-last); dst_table is the geometry `level_inputs` hands to the level launch"""
    x, mask = resize.resize_ingest_frames(pixels, src_table, dst_table, coeffs, B, H, W, *stats, channels_last=False,
                                          layout=layout)
    return x, mask, dst_table


def augment_staged(staged, stats, backbone):
    """one step's staged SOURCE frames (`augment.stage_step`) -> (x, mask, table) of the frames cropped, resized and flipped
    as their plan says: one launch; channels-last where `ingest_staged` would be (a training step); the table is the
    destination geometry `level_inputs` hands to the level launch.  Plans that carry colour weights have
    them applied by the same call: still one launch for brightness and saturation, one more when a frame asks for contrast"""
    asks = getattr(backbone, "wants_channels_last", None)
    nhwc = bool(staged.pixels.is_cuda and asks is not None and asks())
    x, mask = augment.augment_frames(staged, *stats, channels_last=nhwc)
    return x, mask, staged.dst_table


def host_augmented(batched_inputs):
    """The host route of the same plan: every clip's frames and ground truth through `augment.reference_*` on the CPU
    -> `batched_inputs` as a mapper of the reference would have made them (CHW uint8 frames at their targets; gt_masks,
    gt_boxes, the filtered gt_ids).  What a model with `device_augment` takes when `augment.applies` says no, and what the
    tests compare the device route with.  Frames, RLE masks and polygons go through their own plan's `frame` (which ends
    with the plan's colour steps, `augment.color_frame`), `mask` and `coords`; only the boxes and the keep flags differ by kind (`truth`): a FramePlan takes them from the masks, a ChainPlan
    (a COCO pre-training pair) from the annotations' boxes (`chain_boxes`), gt_ids = -1 where the box OR
    the mask is empty."""
    out = []
    for clip in batched_inputs:
        layout, plan = clip.get("image_layout", "chw"), clip["augment"]
        frames = augment.reference_augment_frames(clip["image"], plan, layout)
        frames = [f if layout == "chw" else f.permute(2, 0, 1).contiguous() for f in frames]
        instances = []
        for fr, p, src in zip(clip["instances"], plan, clip["image"]):
            polys = fr.get("gt_poly") or [None] * len(fr["gt_rle"])
            masks = [augment.reference_polygon_mask(q, p) if q is not None else
                     augment.reference_rle_mask(c, resize.frame_size(src, layout), p) for c, q in zip(fr["gt_rle"], polys)]
            boxes, keep = p.truth(masks, fr.get("gt_bbox"))
            gm = torch.from_numpy(np.stack(masks)) if masks else torch.zeros(0, p.nh, p.nw, dtype=torch.bool)
            instances.append({"gt_classes": fr["gt_classes"], "image_size": fr["image_size"], "gt_masks": gm,
                              "gt_boxes": torch.from_numpy(boxes), "gt_ids": torch.where(torch.from_numpy(keep), fr["gt_ids"], -1)})
        out.append({**{k: v for k, v in clip.items() if k not in ("augment", "image_layout")}, "image": frames,
                    "instances": instances})
    return out


def _step_masks(truths, plan, chain):
    """A step's frame dicts and plans -> (masks [(frame, counts or polygon object index, is a polygon)], ids, the polygon
    slots' transformed objects and target sizes, boxes or None); None where a ChainPlan meets an RLE slot: the host route.
    Under ChainPlans the boxes are the annotations' through the chain and a slot whose box is empty gets id -1 (the
    mapper's box test, here; its mask test on the device)."""
    listed, ids, objects, sizes, boxes = [], [], [], [], []
    for f, (fr, p) in enumerate(zip(truths, plan)):
        polys = fr.get("gt_poly") or [None] * len(fr["gt_rle"])
        if chain and any(q is None for q in polys):
            return None
        for c, q in zip(fr["gt_rle"], polys):
            if q is not None:
                c = len(objects)                               # replaced by the object's run slot after the rasterisation
                objects.append(augment.transform_polygons(q, p))
                sizes.append((p.nh, p.nw))
            listed.append((f, c, q is not None))
        if chain:
            boxes.append(augment.chain_boxes(fr["gt_bbox"], p))
            ids += np.where(augment.boxes_nonempty(boxes[-1]), fr["gt_ids"].numpy(), -1).tolist()
        else:
            ids += fr["gt_ids"].tolist()
    return listed, ids, objects, sizes, np.concatenate(boxes) if boxes else None


def augment_step(model, batched_inputs):
    """`device_augment` for one training step.  -> (batched_inputs, pre):
      the switch is off, the model is not training, or a clip carries no "augment": the inputs untouched, pre None;
      the plan is in the kernels' range: pre = (x, mask, table) from ONE `augment_frames` call, and the clips' instance dicts
        (copies) filled with gt_masks, gt_boxes and gt_ids from ONE `augment_masks` call for the whole step -- views of its
        outputs; gt_ids = nonempty ? id : -1 (`filter_empty_instances`: with boxes taken from masks its box test and its
        mask test are the same test).  The clips' "image" entries stay the source frames: nothing reads their pixels again;
      beyond it (`augment.applies`): `host_augmented` inputs, pre None -- the path without the switch.
    Frames staged with `stage_clip(polygons=True)` carry gt_poly: those slots are transformed on the host
    (`augment.transform_polygons`), rasterised at the target size by ONE `polygons_to_runs` call and read by the same
    `augment_masks` call through pseudo-frame rows; nothing is read back from the device.
    A step whose clips ALL carry `augment.ChainPlan`s (COCO pre-training pairs) takes the same route with one launch in front:
    `resize_window_bytes` for the frames that are resampled twice (none for a step without such a frame), then the same
    `augment_frames`, `polygons_to_runs` and `augment_masks` calls.  Its gt_boxes are the annotations' boxes through the
    chain, computed on the host and uploaded with the tables (the masks' own boxes are ignored), and a slot whose box is
    empty is staged with id -1, so `nonempty ? id : -1` is the mapper's box AND mask test.  A step that mixes the two kinds
    of plan, or holds an RLE slot under a ChainPlan, takes the host route."""
    if not (getattr(model, "device_augment", False) and model.training
            and all("augment" in clip for clip in batched_inputs)):
        return batched_inputs, None
    layout = batched_inputs[0].get("image_layout", "chw")
    frames = [f for clip in batched_inputs for f in clip["image"]]
    plan = [p for clip in batched_inputs for p in clip["augment"]]
    truths = [fr for clip in batched_inputs for fr in clip["instances"]]
    kinds = {isinstance(p, augment.ChainPlan) for p in plan}
    chain = kinds == {True}
    listed = _step_masks(truths, plan, chain) if len(kinds) == 1 else None      # (a step that mixes the kinds: the host route)
    if listed is None:
        return host_augmented(batched_inputs), None
    listed, ids, objects, sizes, boxes = listed
    # polygon slots: the coordinates through the frame's plan on the host, ONE rasterisation at the targets on the device
    planned = poly_rle.plan_objects(objects, sizes) if objects else None
    if any(clip.get("image_layout", "chw") != layout for clip in batched_inputs) or \
            not augment.applies(frames, plan, model.device, layout, polygons=planned) or \
            (chain and objects and torch.device(model.device).type != "cuda"):      # (polygons are rasterised on the device)
        return host_augmented(batched_inputs), None
    poly_ends = None
    if objects:
        tables = poly_rle.polygons_to_runs(objects, sizes, device=model.device, check=False, planned=planned)
        poly_ends = tables.ends
        listed = [(f, augment.PolyRuns(*tables.slot_rows[c]) if is_poly else c, is_poly) for f, c, is_poly in listed]
    staged = augment.stage_step(frames, plan, [(f, c) for f, c, _ in listed], model.device, layout, ids, poly_ends=poly_ends,
                                boxes=boxes)
    augment.resize_window_bytes(staged)                        # (a chain step's first resample; otherwise nothing)
    pre = augment_staged(staged, model._pixel_stats, model.detr.detr.backbone)
    masks, mask_boxes, nonempty = augment.augment_masks(staged)
    boxes = staged.boxes if chain else mask_boxes
    gt_ids = torch.where(nonempty, staged.ids, -1).to(torch.int64)
    views, filled = staged.mask_views(masks), []
    for fr, gm, (first, k, _, _) in zip(truths, views, staged.groups):
        filled.append({"gt_classes": fr["gt_classes"], "image_size": fr["image_size"], "gt_masks": gm,
                       "gt_boxes": boxes[first:first + k], "gt_ids": gt_ids[first:first + k]})
    filled = iter(filled)
    return [{**clip, "instances": [next(filled) for _ in clip["instances"]]} for clip in batched_inputs], pre


def takes_bytes(frames, device_ingest, device) -> bool:
    """`device_ingest` is on and these are uint8 frames: they stay bytes until the kernel"""
    return bool(device_ingest) and ingest.applies(frames, device)


def preprocess(frames, device_ingest, device, stats, mean, std, backbone):
    """normalise + pad a list of frames to a multiple of 32 -> (x, mask); with `device_ingest` and uint8 frames ->
    (x, mask, table) from the ingest kernel (`level_inputs` takes the table)."""
    if takes_bytes(frames, device_ingest, device):
        return ingest_staged(*ingest.stage_frames(frames, device), len(frames), *ingest.padded_size(frames), stats, backbone)
    return pad_normalise_list(frames, mean, std, device)


def level_inputs(srcs, mask, table=None):
    """The projected levels [B, C, h, w], the padding mask [B, H, W] -> (masks, poss) per level: the nearest-resized mask and
    its sine position in the level's dtype.  table: the frames' geometry on the device when x, mask came from
    `ingest_staged` / `resize_staged`: the level masks and positions are then one launch of the ingest op instead of ~20
    small ones per level."""
    if table is not None:
        masks, poss = ingest.level_constants(table, *mask.shape, [s.shape[-2:] for s in srcs], srcs[0].shape[1] // 2)
        return masks, [p.to(s.dtype) for p, s in zip(poss, srcs)]
    masks = [F.interpolate(mask[None].float(), size=s.shape[-2:]).to(torch.bool)[0] for s in srcs]
    return masks, [sine_position(mk, s.shape[1] // 2).to(s.dtype) for s, mk in zip(srcs, masks)]


# ---- one inference call's frames, staged ------------------------------------------------------------------------------------
class StagedFrames(NamedTuple):
    tensors: tuple          # on the device; with graph replay, the graph's static inputs (the upload stays outside the capture)
    size: tuple             # (H, W) the frames are padded to
    key: tuple              # of the captured graph
    to_net: Callable        # (*tensors) -> (x, mask, table or None); its launches are inside the capture


def stage_chunk(frames, plan, device_ingest, device, stats, mean, std, backbone):
    """The frames of one clip / chunk -> `StagedFrames`, or None: frames of unequal sizes (float or uint8), which take the
    eager padded-batch path (`preprocess`).  Three kinds:
      float frames of one size (uint8 ones too when `device_ingest` is off): the stack; key = its shape.
      uint8 frames of one size with `device_ingest`: the staged byte buffer and the table; key = (buffer shape, uint8, frames,
        H, W) -- a replay reads the frames' sizes from the table.
      plan = (targets, layout) (`device_resize`): the frames are uint8 sources of ANY sizes, resized to their targets by the
        ingest; the four tensors of `resize.stage_sources`.  The coefficients' layout follows the sizes, so the key holds the
        source and target sizes as well: ("resize", buffer shape, layout, source sizes, targets, H, W).
    Frame counts inside `to_net` come from the tables' shapes and sizes from the key: nothing synchronises or uploads."""
    if plan is not None:
        targets, layout = plan
        tensors = resize.stage_sources(frames, targets, device, layout)
        H, W = resize.padded_size(targets)
        sizes = [resize.frame_size(f, layout) for f in frames]
        key = ("resize", tuple(tensors[0].shape), layout, tuple(sizes), tuple(targets), H, W)
        return StagedFrames(tuple(tensors), (H, W), key,
                            lambda p, s, d, c: resize_staged(p, s, d, c, s.shape[0], H, W, layout, stats))
    if not all(f.shape == frames[0].shape for f in frames):
        return None
    if takes_bytes(frames, device_ingest, device):
        pixels, table = ingest.stage_frames(frames, device)
        H, W = ingest.padded_size(frames)
        key = (tuple(pixels.shape), pixels.dtype, table.shape[0], H, W)
        return StagedFrames((pixels, table), (H, W), key,
                            lambda p, t: ingest_staged(p, t, t.shape[0], H, W, stats, backbone))
    stack = torch.stack([f.to(device, torch.float32) for f in frames])
    return StagedFrames((stack,), ingest.padded_size(frames), tuple(stack.shape),
                        lambda s: (*pad_normalise(s, mean, std), None))


def replay_captured(cache, key, inputs, fn, keep=4):
    """`fn(*inputs)` replayed from a hipGraph captured per `key`: the ~1 500 launches of backbone + 6+6 transformer layers +
    mask-feature convs become one graph launch.  `cache`: the owner's dict, at most `keep`
    entries (a few resolutions; a video is chunks of BATCH_INFER_LEN frames + one shorter tail: two graphs).  `fn` is
    shape-static and free of host synchronisation.  The outputs live in the graph's static buffers until the next call."""
    entry = cache.get(key)
    if entry is None:
        device = inputs[0].device
        static_in = tuple(t.clone() for t in inputs)
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):           # warm-up outside capture: lazy inits, cached level tensors
            for _ in range(2):
                fn(*static_in)
        torch.cuda.current_stream(device).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = fn(*static_in)
        if len(cache) >= keep:                  # a few resolutions at most; drop the oldest
            cache.pop(next(iter(cache)))
        entry = cache[key] = (graph, static_in, static_out)
    graph, static_in, static_out = entry
    for s, t in zip(static_in, inputs):
        s.copy_(t)
    graph.replay()
    return static_out


# ---- the training trunk -----------------------------------------------------------------------------------------------------
class TrainTrunk(nn.Module):
    """The shape-static, sync-free part of a training step -- normalise + pad, then the owner's `_train_trunk(x, mask)`:
    backbone, input projections, 6 + 6 transformer layers, the heads and the mask-feature convs, returned as a flat tuple of
    tensors -- as one module, so that `torch.cuda.make_graphed_callables` can capture its forward AND its backward into two
    hipGraphs.  Shares the owner's parameters; not registered on the owner.

    Why IDOL wants it more than SeqFormer: a key / reference pair is TWO frames -- the ~3 300 launches of a step carry 38 ms of
    kernels (720p, bf16) and the step took 52-56 ms: the host could not issue them fast enough (round 6)."""

    def __init__(self, owner):
        super().__init__()
        self.detr = owner.detr
        object.__setattr__(self, "_owner", owner)

    def forward(self, stack):
        o = self._owner
        with step_scope(stack.device):     # the fused dropout sites read a device-side step seed bumped HERE per replay
            return o._train_trunk(*pad_normalise(stack, o.pixel_mean, o.pixel_std))


def graphed_callable(cache, make_module, stack, keep=2):
    """`make_module()(stack)` replayed from forward + backward hipGraphs captured per (input shape, autocast dtype); `cache`: the
    owner's dict (at most `keep` entries).  Under torch.autocast the capture -- warm-up iterations included -- runs with
    autocast's weight cache off: a weight cast cached BEFORE the capture is a tensor outside the graph's memory pool, and one
    cached DURING it would be served, stale, to the eager code after it.  Replays run no Python of the module, so they need
    nothing from the ambient autocast state."""
    amp = torch.is_autocast_enabled() and stack.is_cuda
    adt = torch.get_autocast_dtype("cuda") if amp else None
    key = (tuple(stack.shape), adt)
    fn = cache.get(key)
    if fn is None:
        if len(cache) >= keep:
            cache.pop(next(iter(cache)))
        with torch.autocast("cuda", dtype=adt, enabled=amp, cache_enabled=False):
            fn = cache[key] = torch.cuda.make_graphed_callables(make_module(), (stack.clone(),), allow_unused_input=True)
    return fn(stack)
