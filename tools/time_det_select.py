"""Time detection selection -- best class, score threshold, class-aware NMS, top-k -- on the host and on the device
(DESIGN section 17).  MI355X only.

Video selection: F = 10 frames (the default BATCH_INFER_LEN), Q = 300, K = 40, about 40 candidates per frame;
  host    IDOL.select_candidates with device_selection off  (one [F, Q, 6] copy to the host, a NumPy NMS loop per frame)
  device  IDOL.select_candidates with device_selection on   (ops/det_select.py: one kernel, one copy of the picks)
COCO selection: B = 1, 2, 8 images, Q = 300, K = 80, no threshold, NMS at 0.7, top 100;
  host    select_detections on a host copy of the tensors (class_aware_nms + torch.topk), the copy included
  device  select_detections on the device tensors
End to end, each call with the copies it needs: the inputs are on the device and the picks end on the host.  One round =
one timed call of each path, alternating in one process; device events around the call, which ends in the copy's
synchronise, and a device synchronise before the elapsed time is read; medians over the rounds after warm-up, with min
and max.  The launch and copy counts of one call of each path come from torch.profiler, in a pass of their own.

    python tools/time_det_select.py [--out FILE.json] [--rounds N] [--warmup N]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def timed(call):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    call()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end)


def counts(call):
    """kernel launches and memory copies of one call (torch.profiler, device activities)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    kernels = copies = 0
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            if "memcpy" in ev.name.lower() or "copy" in ev.name.lower() and "kernel" not in ev.name.lower():
                copies += 1
            else:
                kernels += 1
    return {"kernels": kernels, "copies": copies}


def inputs(seed, B, Q, K, objects, dup_spread):
    """logits -4 + 0.5 N(0,1) and random boxes with planted objects (1-5 near-duplicate boxes each, logits 1.5 - 0.6 d +
    0.5 N(0,1) on a random class): the recipe of tests/test_det_select.py"""
    g = torch.Generator().manual_seed(seed)
    logits = -4.0 + 0.5 * torch.randn(B, Q, K, generator=g)
    boxes = torch.cat([0.2 + 0.6 * torch.rand(B, Q, 2, generator=g), 0.05 + 0.2 * torch.rand(B, Q, 2, generator=g)], -1)
    for b in range(B):
        slots = torch.randperm(Q, generator=g).tolist()
        for _ in range(objects):
            cls = int(torch.randint(0, K, (1,), generator=g))
            base = torch.cat([0.2 + 0.6 * torch.rand(2, generator=g), 0.05 + 0.2 * torch.rand(2, generator=g)])
            for d in range(int(torch.randint(1, 6, (1,), generator=g))):
                q = slots.pop()
                boxes[b, q] = base + dup_spread * d * torch.randn(4, generator=g)
                logits[b, q, cls] = 1.5 - 0.6 * d + 0.5 * torch.randn(1, generator=g).item()
    return logits.cuda(), boxes.cuda()


def run(paths, rounds, warmup, same):
    for _ in range(warmup):
        for call in paths.values():
            call()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for k, call in paths.items():
            times[k].append(timed(call))
    out = {k: stats(v) for k, v in times.items()}
    out["device_below_host_in_every_round"] = all(d < h for d, h in zip(times["device"], times["host"]))
    out["same_result"] = bool(same(paths["host"](), paths["device"]()))
    try:
        out["launches_and_copies"] = {k: counts(call) for k, call in paths.items()}
    except Exception as e:      # no device tracer in this torch build: the counts are not measured
        out["launches_and_copies"] = {"not_measured": repr(e)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_det_select.py: needs an MI355X (no CPU fallback for timings)")
    import numpy as np
    from vnext_amd.models.idol import IDOL
    from vnext_amd.ops.det_select import select_detections
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup}

    # video selection: about 40 candidates per frame (14 objects x ~3 duplicates above the 0.1 threshold)
    logits, boxes = inputs(1, 10, 300, 40, 14, 0.004)
    host_self = types.SimpleNamespace(device_selection=False, inference_select_thres=0.1)
    dev_self = types.SimpleNamespace(device_selection=True, inference_select_thres=0.1)
    paths = {"host": lambda: IDOL.select_candidates(host_self, logits, boxes),
             "device": lambda: IDOL.select_candidates(dev_self, logits, boxes)}
    entry = run(paths, a.rounds, a.warmup, lambda h, d: all(np.array_equal(x, y) for x, y in zip(h, d)))
    entry["frames"], entry["queries"], entry["classes"] = 10, 300, 40
    entry["candidates_per_frame"] = float((logits.sigmoid().amax(-1) > 0.1).sum(1).float().mean())
    entry["picks_per_frame"] = float(np.mean([len(p) for p in paths["device"]()]))
    res["video_selection"] = entry

    res["coco_selection"] = {}
    for B in (1, 2, 8):
        logits, boxes = inputs(2 + B, B, 300, 80, 12, 0.012)
        paths = {"host": lambda: select_detections(logits.cpu(), boxes.cpu(), iou_thr=0.7, topk=100),
                 "device": lambda: select_detections(logits, boxes, iou_thr=0.7, topk=100)}

        def same(h, d):
            return all(np.array_equal(x, y) for x, y in zip(h.kept, d.kept)) and \
                all(np.array_equal(x, y) for x, y in zip(h.topk, d.topk))
        entry = run(paths, a.rounds, a.warmup, same)
        entry["images"], entry["queries"], entry["classes"] = B, 300, 80
        entry["kept_per_image"] = float(np.mean(paths["device"]().counts))
        res["coco_selection"][f"B{B}"] = entry
    res["timing"] = ("device events around each call (inputs on the device, picks on the host), a device synchronise "
                     "before and after; host / device alternating per round")
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
