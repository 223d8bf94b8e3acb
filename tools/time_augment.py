"""Time the training front end: source frames and annotations on the CPU to network inputs and targets on the device, on the
host route and through the augment ops (vnext_amd/ops/augment.py).  MI355X only.  Both routes alternate in
one process; every round is kept.

The input is what a mapper has after `read_image`, `sample_plan` and `stage_clip`: decoded uint8 [h, w, 3] frames on the CPU,
a plan, and per (instance, frame) the mask's COCO counts.
  host route (what the parent commit needs):  per frame numpy crop, Pillow's `resize(BILINEAR)`, `np.flip`, transpose to CHW;
      per (instance, frame) mask: decode the run lengths (one vectorised `np.repeat`: pycocotools' C decoder is not installed
      here, this stands in for it), crop, Pillow's `resize(NEAREST)` of the mode-L mask, `np.flip`; the box loop of
      `BitMasks.get_bounding_boxes`; `filter_empty_instances`; the upload of masks, boxes and ids; then the ingest op
      (`device_ingest`): stage_frames + ingest_frames + level_constants.  Where Pillow does not import, the integer
      restatements stand in and the JSON says so.
  device route:  stage_step (one pinned buffer, one copy) + augment_frames + augment_masks + level_constants + the id filter.
(a) both workloads, host wall clock from the call to a device synchronise and the HIP-event region of the same stretch.  x, the
    padding mask, every gt mask, box and id of both routes are compared.
(b) kernel launches and copies of both routes, from torch.profiler, in a pass of their own.
(c) the two ops alone against the bytes they move: HIP events around 50 back-to-back calls (an upper bound of the kernels' own
    time: it includes the launch gaps).

    python tools/time_augment.py [--out FILE.json] [--rounds N] [--warmup N]

`--color` (profiles/augment_color.json): the same two workloads with a brightness, a contrast and a
saturation weight per frame.  Three routes alternate per round, every round kept: the host route with colour (the three
numpy steps of `augment.color_frame` on every resized frame), the device route with colour (two frame launches) and the
device route without (the plan as it was: the figure to hold against profiles/augment.json).  The bar is the same, between
the two routes WITH colour; the colour's cost on the device route is reported next to the bytes its extra pass moves.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.time_ingest import counts, level_sizes, stats, timed  # noqa: E402
from vnext_amd.ops import augment, ingest, resize  # noqa: E402
from vnext_amd.ops.augment import FramePlan  # noqa: E402
from vnext_amd.utils.ytvis_json import rle_counts  # noqa: E402

DEV = "cuda:0"

try:
    from PIL import Image
    HOST_RESIZE = "Pillow " + __import__("PIL").__version__
except ImportError:
    Image = None
    HOST_RESIZE = "vnext_amd.ops.augment.reference_augment_* (Pillow is not installed here)"


def blob_counts(h, w, rng):
    """an instance: an ellipse somewhere in the frame, as COCO counts"""
    yy, xx = np.mgrid[:h, :w]
    cy, cx = rng.integers(h // 4, 3 * h // 4), rng.integers(w // 4, 3 * w // 4)
    ry, rx = rng.integers(h // 10, h // 3), rng.integers(w // 10, w // 3)
    return rle_counts((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0).astype(np.uint8)).tolist()


def workload(name, seed):
    """-> (frames uint8 HWC, plan, masks [(frame, counts)], ids)"""
    rng = np.random.default_rng(seed)
    h, w = 720, 1280
    if name == "seqformer_2x5x720p_short480_4inst":      # the bench's SeqFormer clips: two clips of five frames, no crop
        n_clips, n_frames, inst = 2, 5, 4
        plan = []
        for c in range(n_clips):
            flip = bool(c)
            plan += [FramePlan(0, 0, w, h, *resize.shortest_edge_size(h, w, 480, 1333), flip)] * n_frames
    else:                                                # an IDOL batch: two key / reference pairs, cropped per frame
        n_clips, n_frames, inst = 2, 2, 4
        plan = []
        for c in range(n_clips):
            for _ in range(n_frames):
                ch, cw = int(rng.integers(384, 601)), int(rng.integers(384, 601))
                y0, x0 = int(rng.integers(h - ch + 1)), int(rng.integers(w - cw + 1))
                plan.append(FramePlan(x0, y0, cw, ch, *resize.shortest_edge_size(ch, cw, 480, 768), bool(c)))
    g = torch.Generator().manual_seed(seed)
    n = n_clips * n_frames
    frames = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g) for _ in range(n)]
    masks = [(f, blob_counts(h, w, rng)) for f in range(n) for _ in range(inst)]
    return frames, plan, masks, list(range(1, len(masks) + 1))


def decode(counts_, h, w):
    """COCO counts -> uint8 [h, w] (what mask_util.decode returns)"""
    vals = np.arange(len(counts_), dtype=np.uint8) & 1
    return np.repeat(vals, counts_).reshape((h, w), order="F")


def host_route(frames, plan, masks, ids, stats_):
    out_frames = []
    for f, p in zip(frames, plan):
        a = f.numpy()[p.y0:p.y0 + p.ch, p.x0:p.x0 + p.cw]
        if Image is not None:
            a = np.asarray(Image.fromarray(np.ascontiguousarray(a)).resize((p.nw, p.nh), Image.BILINEAR))
        else:
            a = resize.reference_resize(np.ascontiguousarray(a), p.nh, p.nw, "hwc")
        if p.flip:
            a = np.flip(a, axis=1)
        if p.color != augment.NO_COLOR:
            a = augment.color_frame(a, 2, *p.color)
        out_frames.append(torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))))
    gt, boxes, keep = [], [], []
    for f, c in masks:
        p = plan[f]
        h, w = frames[f].shape[:2]
        m = decode(c, h, w)[p.y0:p.y0 + p.ch, p.x0:p.x0 + p.cw]
        if Image is not None:
            m = np.asarray(Image.fromarray(np.ascontiguousarray(m), mode="L").resize((p.nw, p.nh), Image.NEAREST))
        else:
            m = m[augment.nearest_table(p.ch, p.nh)][:, augment.nearest_table(p.cw, p.nw)]
        if p.flip:
            m = np.flip(m, axis=1)
        m = np.ascontiguousarray(m).astype(bool)
        b, k = augment.mask_box(m)
        gt.append(torch.from_numpy(m))
        boxes.append(b)
        keep.append(k)
    n = len(frames)
    H, W = ingest.padded_size(out_frames)
    pixels, table = ingest.stage_frames(out_frames, DEV)
    x, mask = ingest.ingest_frames(pixels, table, n, H, W, *stats_)
    levels = ingest.level_constants(table, n, H, W, level_sizes(H, W), 128)
    per_frame = [[g for (f, _), g in zip(masks, gt) if f == i] for i in range(n)]
    gt_dev = [torch.stack(m).to(DEV, non_blocking=True) for m in per_frame]
    boxes_dev = torch.from_numpy(np.stack(boxes)).to(DEV, non_blocking=True)
    ids_dev = torch.where(torch.tensor(keep), torch.tensor(ids), -1).to(DEV, non_blocking=True)
    return x, mask, levels, gt_dev, boxes_dev, ids_dev


def device_route(frames, plan, masks, ids, stats_):
    staged = augment.stage_step(frames, plan, masks, DEV, "hwc", ids)
    x, mask = augment.augment_frames(staged, *stats_)
    H, W = staged.size
    levels = ingest.level_constants(staged.dst_table, len(frames), H, W, level_sizes(H, W), 128)
    flat, boxes, nonempty = augment.augment_masks(staged)
    gt_ids = torch.where(nonempty, staged.ids, -1).to(torch.int64)
    return x, mask, levels, staged.mask_views(flat), boxes, gt_ids


def same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(u, v) for u, v in zip(a[3], b[3]))
                and torch.equal(a[4], b[4]) and torch.equal(a[5], b[5]))


def ops_alone(frames, plan, masks, ids, stats_, reps=50):
    """the two ops alone, HIP events around `reps` back-to-back calls, against the bytes they move"""
    staged = augment.stage_step(frames, plan, masks, DEV, "hwc", ids)
    H, W = staged.size
    n, m = len(frames), len(masks)
    out = {}
    for name, call, moved in (
            ("augment_frames", lambda: augment.augment_frames(staged, *stats_),
             sum(3 * p.cw * p.ch for p in plan) + n * H * W * (3 * 4 + 1)),
            ("augment_masks", lambda: augment.augment_masks(staged),
             4 * staged.ends.numel() + staged.mask_bytes + 2 * 16 * m * (H // 32) * (W // 32) + 21 * m)):
        for _ in range(5):
            call()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(reps):
            call()
        end.record()
        torch.cuda.synchronize()
        ms = start.elapsed_time(end) / reps
        out[name] = {"event_ms_per_call": ms, "bytes_moved_at_least": int(moved), "gigabytes_per_second": moved / ms / 1e6,
                     "note": "window bytes read once + every output byte written once (+ the runs and the tiles' boxes for the "
                             "masks); the time includes the launch gaps and, for the masks, the output allocations"}
    return out


def with_color(plan, seed):
    """the plan with a weight per frame and step, as `sample_plan` draws them"""
    rng = np.random.default_rng(seed)
    return [p._replace(**{name: float(rng.uniform(0.9, 1.1)) for name in ("brightness", "contrast", "saturation")}) for p in plan]


def color_main(a, stats_):
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup, "host_resize": HOST_RESIZE,
           "host_threads": torch.get_num_threads(), "cases": {}}
    for i, name in enumerate(("seqformer_2x5x720p_short480_4inst", "idol_2_pairs_720p_crop384-600_short480_4inst")):
        frames, plan, masks, ids = workload(name, seed=90 + i)
        plans = {"host_color": with_color(plan, 190 + i), "device_color": with_color(plan, 190 + i), "device_plain": plan}
        routes = {"host_color": host_route, "device_color": device_route, "device_plain": device_route}
        times = {key: [] for key in routes}
        for r in range(a.rounds + a.warmup):
            for key, fn in routes.items():
                t = timed(lambda: fn(frames, plans[key], masks, ids, stats_))
                if r >= a.warmup:
                    times[key].append(t)
        n, (H, W) = len(frames), augment.padded_size(plan)
        case = {"frames": n, "masks": len(masks), "targets": sorted({(p.nh, p.nw) for p in plan}),
                "outputs_equal": same(host_route(frames, plans["host_color"], masks, ids, stats_),
                                      device_route(frames, plans["device_color"], masks, ids, stats_))}
        for key, v in times.items():
            case[key + "_route"] = {"host_wall_clock": stats([t[0] for t in v]), "event_region": stats([t[1] for t in v])}
        hw, dw, pw = (case[k + "_route"]["host_wall_clock"] for k in routes)
        spread = max(hw["max_ms"] - hw["min_ms"], dw["max_ms"] - dw["min_ms"])
        case["spread_of_rounds_ms"] = spread
        case["device_route_meets_the_bar"] = bool(dw["median_ms"] <= hw["median_ms"] + spread)
        inside = sum(3 * p.nh * p.nw for p in plan)
        case["color_on_cost"] = {
            "host_wall_clock_median_ms": dw["median_ms"] - pw["median_ms"],
            "event_region_median_ms": case["device_color_route"]["event_region"]["median_ms"]
            - case["device_plain_route"]["event_region"]["median_ms"],
            "extra_pass_bytes": {"written_by_the_first_launch": inside + 4 * n * (H // 32) * (W // 32),
                                 "read_by_the_second_launch": inside + 4 * n * (H // 32) * (W // 32) * (H // 32) * (W // 32),
                                 "note": "the post-brightness bytes inside the frames, once each way, and a uint32 per tile; "
                                         "every workgroup of the second launch reads its frame's tile sums (from cache)"}}
        try:
            case["launches_and_copies"] = {k: counts(lambda: fn(frames, plans[k], masks, ids, stats_)) for k, fn in routes.items()}
        except Exception as e:      # no device tracer in this torch build: the counts are not measured
            case["launches_and_copies"] = {"not_measured": repr(e)}
        res["cases"][name] = case
    res["timing"] = ("as profiles/augment.json, three routes alternating per round: the host route with the three colour steps in "
                     "numpy, the device route with them (vnx_augment_frames_color, two launches) and the device route without; "
                     "the bar: the device route's median with colour is not above the host route's with colour by more than "
                     "the spread of the rounds; device_plain is the figure to compare with profiles/augment.json")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--color", action="store_true", help="time the colour steps (profiles/augment_color.json)")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_augment.py: needs an MI355X (no CPU fallback for timings)")
    from vnext_amd.registry import get_seqformer_cfg
    cfg = get_seqformer_cfg()
    stats_ = ([float(v) for v in cfg.MODEL.PIXEL_MEAN], [float(v) for v in cfg.MODEL.PIXEL_STD])
    a.out = a.out or os.path.join(ROOT, "profiles", "augment_color.json" if a.color else "augment.json")
    if a.color:
        return write(color_main(a, stats_), a.out)
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup, "host_resize": HOST_RESIZE,
           "host_threads": torch.get_num_threads(), "cases": {}}
    for i, name in enumerate(("seqformer_2x5x720p_short480_4inst", "idol_2_pairs_720p_crop384-600_short480_4inst")):
        args = workload(name, seed=90 + i) + (stats_,)
        times = {"host": [], "device": []}
        for r in range(a.rounds + a.warmup):
            for key, fn in (("host", host_route), ("device", device_route)):
                t = timed(lambda: fn(*args))
                if r >= a.warmup:
                    times[key].append(t)
        case = {"frames": len(args[0]), "masks": len(args[2]), "runs": sum(len(c) for _, c in args[2]),
                "targets": sorted({(p.nh, p.nw) for p in args[1]}), "outputs_equal": same(host_route(*args), device_route(*args))}
        for key, v in times.items():
            case[key + "_route"] = {"host_wall_clock": stats([t[0] for t in v]), "event_region": stats([t[1] for t in v])}
        hw, dw = case["host_route"]["host_wall_clock"], case["device_route"]["host_wall_clock"]
        spread = max(hw["max_ms"] - hw["min_ms"], dw["max_ms"] - dw["min_ms"])
        case["spread_of_rounds_ms"] = spread
        case["device_route_meets_the_bar"] = bool(dw["median_ms"] <= hw["median_ms"] + spread)
        try:
            case["launches_and_copies"] = {"host_route": counts(lambda: host_route(*args)),
                                           "device_route": counts(lambda: device_route(*args))}
        except Exception as e:      # no device tracer in this torch build: the counts are not measured
            case["launches_and_copies"] = {"not_measured": repr(e)}
        case["ops_alone"] = ops_alone(*args)
        res["cases"][name] = case
    res["timing"] = ("CPU uint8 HWC source frames + COCO counts to x, mask, four levels of masks and positions, gt masks, boxes and "
                     "ids on the device; host wall clock from the call to a device synchronise and the HIP-event region of the "
                     "same stretch, host / device route alternating per round; launch counts in a pass of their own; the bar: "
                     "the device route's median is not above the host route's by more than the spread of the rounds")
    write(res, a.out)


def write(res, out):
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
