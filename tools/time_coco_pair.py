"""Time the COCO pre-training front end: one CPU source image and its polygon annotations per pair to network inputs and
targets on the device, on the host route and through the device route of the chain flip -> resize -> crop -> resize
(vnext_amd/ops/augment.py, vnext_amd/models/frames.py).  MI355X only.  Both routes alternate in one process;
every round is kept.

The input is what a mapper has after `read_image`, `sample_coco_plan` and `stage_coco_pair`: a decoded uint8 image on the CPU,
two ChainPlans, the annotations' polygon lists and boxes.
  host route:  `frames.host_augmented` on the chain plans (the integer restatement of Pillow's resize twice per cropped frame,
      the polygons rasterised by numpy at the target size -- what a data-loader worker of the reference does with Pillow and
      pycocotools, neither of which this route imports; its figure is NOT asserted), the upload of masks, boxes and ids, then
      the ingest op (`device_ingest`): stage_frames + ingest_frames + level_constants.
  device route:  `frames.augment_step`: the coordinates and boxes on the host, polygons_to_runs, stage_step (one pinned buffer,
      one copy), resize_window_bytes, augment_frames, augment_masks, the id filter; then level_constants.
(a) the workload, host wall clock from the call to a device synchronise and the HIP-event region of the same stretch.  x, the
    padding mask, every gt mask, box and id of both routes are compared.
(b) kernel launches and copies of both routes, from torch.profiler, in a pass of their own.
(c) the bytes kernel alone: HIP events around 50 back-to-back launches (an upper bound of the kernel's own time: it includes
    the launch gaps).

    python tools/time_coco_pair.py [--out FILE.json] [--rounds N] [--warmup N]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.time_ingest import counts, level_sizes, stats, timed  # noqa: E402
from vnext_amd.data import clip_mapper  # noqa: E402
from vnext_amd.models import frames as frames_mod  # noqa: E402
from vnext_amd.ops import augment, ingest  # noqa: E402

DEV = "cuda:0"
SHORT = (320, 352, 392, 416, 448, 480, 512, 544, 576, 608, 640)      # r50_coco_sequence.yaml


def blob_polygon(h, w, rng, vertices=24):
    """an instance: a wobbly ellipse somewhere in the image, as one polygon, and its XYWH box"""
    cy, cx = rng.uniform(h / 4, 3 * h / 4), rng.uniform(w / 4, 3 * w / 4)
    ry, rx = rng.uniform(h / 10, h / 3), rng.uniform(w / 10, w / 3)
    t = np.linspace(0, 2 * np.pi, vertices, endpoint=False)
    r = rng.uniform(0.8, 1.0, vertices)
    x, y = np.clip(cx + rx * r * np.cos(t), 0, w), np.clip(cy + ry * r * np.sin(t), 0, h)
    poly = np.stack((x, y), 1).reshape(-1).tolist()
    return {"category_id": int(rng.integers(1, 80)), "segmentation": [poly],
            "bbox": [float(x.min()), float(y.min()), float(x.max() - x.min()), float(y.max() - y.min())]}


def workload(seed, pairs=4, objects=7, size=(480, 640)):
    """a per-GPU batch of r50_coco_sequence.yaml: `pairs` images of `size`, `objects` polygon instances each, seeded plans"""
    rng = np.random.default_rng(seed)
    cfg = SimpleNamespace(INPUT=SimpleNamespace(
        MIN_SIZE_TRAIN=SHORT, MAX_SIZE_TRAIN=1333, MIN_SIZE_TRAIN_SAMPLING="choice", PRETRAIN_SAME_CROP=False,
        CROP=SimpleNamespace(ENABLED=True, TYPE="absolute_range", SIZE=(384, 600))))
    g = torch.Generator().manual_seed(seed)
    clips = []
    for _ in range(pairs):
        image = torch.randint(0, 256, (3,) + tuple(size), dtype=torch.uint8, generator=g)
        annos = [blob_polygon(*size, rng) for _ in range(objects)]
        clips.append(clip_mapper.stage_coco_pair(image, annos, clip_mapper.sample_coco_plan(cfg, size, rng), 80))
    return clips


def stub_model(stats_):
    return SimpleNamespace(device_augment=True, training=True, device=torch.device(DEV), _pixel_stats=stats_,
                           detr=SimpleNamespace(detr=SimpleNamespace(backbone=SimpleNamespace())))


def host_route(clips, stats_):
    out = frames_mod.host_augmented(clips)
    frames = [f for clip in out for f in clip["image"]]
    n = len(frames)
    H, W = ingest.padded_size(frames)
    pixels, table = ingest.stage_frames(frames, DEV)
    x, mask = ingest.ingest_frames(pixels, table, n, H, W, *stats_)
    levels = ingest.level_constants(table, n, H, W, level_sizes(H, W), 128)
    inst = [fr for clip in out for fr in clip["instances"]]
    gt = [fr["gt_masks"].to(DEV, non_blocking=True) for fr in inst]
    boxes = torch.cat([fr["gt_boxes"] for fr in inst]).to(DEV, non_blocking=True)
    ids = torch.cat([fr["gt_ids"] for fr in inst]).to(DEV, non_blocking=True)
    return x, mask, levels, gt, boxes, ids


def device_route(clips, stats_):
    out, (x, mask, table) = frames_mod.augment_step(stub_model(stats_), clips)
    H, W = mask.shape[-2:]
    levels = ingest.level_constants(table, x.shape[0], H, W, level_sizes(H, W), 128)
    inst = [fr for clip in out for fr in clip["instances"]]
    return x, mask, levels, [fr["gt_masks"] for fr in inst], torch.cat([fr["gt_boxes"] for fr in inst]), \
        torch.cat([fr["gt_ids"] for fr in inst])


def same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(u, v) for u, v in zip(a[3], b[3]))
                and torch.equal(a[4], b[4]) and torch.equal(a[5], b[5]))


def bytes_kernel_alone(clips, reps=50):
    """`resize_window_bytes` alone, HIP events around `reps` back-to-back launches, against the bytes it moves"""
    frames = [f for clip in clips for f in clip["image"]]
    plan = [p for clip in clips for p in clip["augment"]]
    staged = augment.stage_step(frames, plan, [], DEV)
    twice = [p for p in plan if p.resamples_twice]
    if not twice:
        return {"not_measured": "no frame of this workload is resampled twice"}
    for _ in range(5):
        augment.resize_window_bytes(staged)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        augment.resize_window_bytes(staged)
    end.record()
    torch.cuda.synchronize()
    ms = start.elapsed_time(end) / reps
    moved = sum(3 * p.cw * p.ch for p in twice) + sum(int(3 * p.cw * p.ch * (p.h / p.h1) * (p.w / p.w1)) for p in twice)
    return {"frames": len(twice), "windows": [(p.ch, p.cw) for p in twice], "event_ms_per_launch": ms,
            "bytes_moved_at_least": int(moved), "gigabytes_per_second": moved / ms / 1e6,
            "note": "the windows' source bytes read once + the windows written once; the time includes the launch gaps"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_pair.json"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_coco_pair.py: needs an MI355X (no CPU fallback for timings)")
    from vnext_amd.registry import get_idol_cfg
    cfg = get_idol_cfg()
    stats_ = ([float(v) for v in cfg.MODEL.PIXEL_MEAN], [float(v) for v in cfg.MODEL.PIXEL_STD])
    clips = workload(seed=95)
    plan = [p for clip in clips for p in clip["augment"]]
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup,
           "host_threads": torch.get_num_threads(),
           "host_resize": "vnext_amd.ops.resize.reference_resize (numpy; the reference's workers call Pillow)"}
    times = {"host": [], "device": []}
    for r in range(a.rounds + a.warmup):
        for key, fn in (("host", host_route), ("device", device_route)):
            t = timed(lambda: fn(clips, stats_))
            if r >= a.warmup:
                times[key].append(t)
    case = {"pairs": len(clips), "frames": len(plan), "frames_resampled_twice": sum(p.resamples_twice for p in plan),
            "objects": sum(len(fr["gt_poly"]) for clip in clips for fr in clip["instances"]),
            "targets": sorted({(p.nh, p.nw) for p in plan}),
            "outputs_equal": same(host_route(clips, stats_), device_route(clips, stats_))}
    for key, v in times.items():
        case[key + "_route"] = {"host_wall_clock": stats([t[0] for t in v]), "event_region": stats([t[1] for t in v])}
    hw, dw = case["host_route"]["host_wall_clock"], case["device_route"]["host_wall_clock"]
    spread = max(hw["max_ms"] - hw["min_ms"], dw["max_ms"] - dw["min_ms"])
    case["spread_of_rounds_ms"] = spread
    case["device_route_meets_the_bar"] = bool(dw["median_ms"] <= hw["median_ms"] + spread)
    try:
        case["launches_and_copies"] = {"host_route": counts(lambda: host_route(clips, stats_)),
                                       "device_route": counts(lambda: device_route(clips, stats_))}
    except Exception as e:      # no device tracer in this torch build: the counts are not measured
        case["launches_and_copies"] = {"not_measured": repr(e)}
    case["bytes_kernel_alone"] = bytes_kernel_alone(clips)
    res["cases"] = {"idol_coco_4_pairs_480x640_crop384-600_7_polygons": case}
    res["timing"] = ("one CPU uint8 CHW image + polygon annotations per pair to x, mask, four levels of masks and positions, gt "
                     "masks, boxes and ids on the device; host wall clock from the call to a device synchronise and the "
                     "HIP-event region of the same stretch, host / device route alternating per round; launch counts in a pass "
                     "of their own; the bar: the device route's median is not above the host route's by more than the spread "
                     "of the rounds")
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
