"""Time the test-time resize: decoded uint8 frames to network inputs, on the host route and through the resize op
(vnext_amd/ops/resize.py).  MI355X only.  Both routes alternate in one process; every round is kept.

The frames are what a video decoder hands over: uint8 [h, w, 3] on the CPU.
  host route (the parent commit's):  per frame Pillow's `Image.resize(..., BILINEAR)` on the host and a transpose to CHW,
      then the ingest op (`device_ingest` on): stage_frames + ingest_frames + level_constants.  Where Pillow does not import,
      `resize.reference_resize` stands in for it and the JSON says so ("host_resize").
  device route:  stage_sources + resize_ingest_frames + level_constants on the destination table.
(a) frames -> network inputs (x, mask, four levels of masks and positions), host wall clock from the frames to a device
    synchronise and the HIP-event region of the same stretch: 10 x 720p -> 360p, 36 x 720p -> 360p in chunks of 10,
    10 x 1080p -> 360p.  x and the masks of both routes are compared.
(b) kernel launches and copies of both routes for the first shape, from torch.profiler, in a pass of their own.
(c) SeqFormer-R50 (random weights), a 36-frame 720p video end to end (`inference`, graph replay), host route against
    `enable_device_resize`; wall clock, synchronised on both sides.

    python tools/time_resize.py [--out FILE.json] [--rounds N] [--warmup N] [--model-rounds N] [--no-model]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.time_ingest import counts, level_sizes, stats, timed  # noqa: E402

DEV = "cuda:0"
SHORT, MAX_SIZE = 360, 640      # 720 x 1280 and 1080 x 1920 -> 360 x 640

try:
    from PIL import Image
    HOST_RESIZE = "Pillow " + __import__("PIL").__version__
except ImportError:      # the baseline is then the integer restatement, which is slower than Pillow
    Image = None
    HOST_RESIZE = "vnext_amd.ops.resize.reference_resize (Pillow is not installed here)"


def decoded_frames(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g) for _ in range(n)]


def host_resized(frames):
    """the parent's route up to the model's door: resize on the host, CHW"""
    from vnext_amd.ops import resize
    out = []
    for f in frames:
        nh, nw = resize.shortest_edge_size(f.shape[0], f.shape[1], SHORT, MAX_SIZE)
        if Image is not None:
            r = torch.from_numpy(np.array(Image.fromarray(f.numpy()).resize((nw, nh), Image.BILINEAR)))
        else:
            r = resize.reference_resize(f, nh, nw, "hwc")
        out.append(r.permute(2, 0, 1).contiguous())
    return out


def entry(frames, chunk, stats_, device_route):
    """decoded frames -> x, mask, level masks and positions of every chunk, on the device"""
    from vnext_amd.ops import ingest, resize
    out = []
    for s in range(0, len(frames), chunk):
        part = frames[s:s + chunk]
        if device_route:
            targets = [resize.shortest_edge_size(f.shape[0], f.shape[1], SHORT, MAX_SIZE) for f in part]
            H, W = resize.padded_size(targets)
            pixels, src, table, coeffs = resize.stage_sources(part, targets, DEV, "hwc")
            x, mask = resize.resize_ingest_frames(pixels, src, table, coeffs, len(part), H, W, *stats_, layout="hwc")
        else:
            small = host_resized(part)
            H, W = ingest.padded_size(small)
            pixels, table = ingest.stage_frames(small, DEV)
            x, mask = ingest.ingest_frames(pixels, table, len(part), H, W, *stats_)
        out.append((x, mask) + ingest.level_constants(table, len(part), H, W, level_sizes(H, W), 128))
    return out


def entry_case(n, h, w, chunk, stats_, rounds, warmup):
    frames = decoded_frames(n, h, w, seed=n + h)
    times = {"host": [], "device": []}
    for r in range(rounds + warmup):
        for key, on in (("host", False), ("device", True)):
            t = timed(lambda: entry(frames, chunk, stats_, on))
            if r >= warmup:
                times[key].append(t)
    a, b = entry(frames, chunk, stats_, False), entry(frames, chunk, stats_, True)
    same = all(torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]) and all(torch.equal(u, v) for u, v in zip(p[2], q[2]))
               and all(torch.equal(u, v) for u, v in zip(p[3], q[3])) for p, q in zip(a, b))
    res = {"frames": n, "height": h, "width": w, "chunk": chunk, "target": [SHORT, MAX_SIZE],
           "source_megabytes": n * 3 * h * w / 1e6, "network_inputs_equal": bool(same)}
    for key, v in times.items():
        res[key + "_route"] = {"host_wall_clock": stats([t[0] for t in v]), "event_region": stats([t[1] for t in v])}
    res["device_route_slower"] = res["device_route"]["host_wall_clock"]["median_ms"] > res["host_route"]["host_wall_clock"]["median_ms"]
    return res


def model_case(rounds, warmup):
    import vnext_amd.models  # noqa: F401
    from vnext_amd import train
    from vnext_amd.registry import build_model, get_seqformer_cfg
    torch.manual_seed(0)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": DEV, "INPUT.MIN_SIZE_TEST": SHORT,
                                             "INPUT.MAX_SIZE_TEST": MAX_SIZE})).eval()
    train.enable_device_ingest(model)
    frames = decoded_frames(36, 720, 1280, seed=1)
    times = {"host": [], "device": []}
    for r in range(rounds + warmup):
        for key, on in (("host", False), ("device", True)):
            train.enable_device_resize(model, on)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if on:
                model.inference([{"image": frames, "image_layout": "hwc"}])
            else:
                model.inference([{"image": host_resized(frames), "height": 720, "width": 1280}])
            torch.cuda.synchronize()
            if r >= warmup:
                times[key].append((time.perf_counter() - t0) * 1e3)
    return {"video_36x720p_to_360p": {"graph_inference": bool(model.graph_inference), "input": "CPU uint8 HWC frames",
                                      "host_route": stats(times["host"]), "device_route": stats(times["device"])}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize.json"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model-rounds", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_resize.py: needs an MI355X (no CPU fallback for timings)")
    from vnext_amd.registry import get_seqformer_cfg
    cfg = get_seqformer_cfg()
    stats_ = ([float(v) for v in cfg.MODEL.PIXEL_MEAN], [float(v) for v in cfg.MODEL.PIXEL_STD])
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup, "host_resize": HOST_RESIZE,
           "host_threads": torch.get_num_threads(), "frames_to_inputs": {}}
    for name, (n, h, w, chunk) in (("10x720x1280", (10, 720, 1280, 10)), ("36x720x1280_chunks_of_10", (36, 720, 1280, 10)),
                                   ("10x1080x1920", (10, 1080, 1920, 10))):
        res["frames_to_inputs"][name] = entry_case(n, h, w, chunk, stats_, a.rounds, a.warmup)
    frames = decoded_frames(10, 720, 1280, seed=730)
    try:
        res["launches_and_copies_10x720x1280"] = {"host_route": counts(lambda: entry(frames, 10, stats_, False)),
                                                  "device_route": counts(lambda: entry(frames, 10, stats_, True))}
    except Exception as e:      # no device tracer in this torch build: the counts are not measured
        res["launches_and_copies_10x720x1280"] = {"not_measured": repr(e)}
    if not a.no_model:
        res["seqformer_r50"] = model_case(a.model_rounds, 2)
    res["timing"] = ("frames_to_inputs: CPU uint8 HWC frames to x, mask and four levels of masks and positions; host wall "
                     "clock from the call to a device synchronise and the HIP-event region of the same stretch, host / device "
                     "route alternating per round.  seqformer_r50: wall clock around the host resize (host route) and "
                     "inference, synchronised on both sides, routes alternating; the launch counts in a pass of their own")
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
