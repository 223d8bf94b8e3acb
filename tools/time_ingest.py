"""Time the entry of the models -- CPU uint8 frames to network inputs -- on the eager path and through the ingest op
(vnext_amd/ops/ingest.py).  MI355X only.  Both variants alternate in one process; every round is kept.

(a) frames -> network inputs: CPU uint8 CHW frames (what detectron2's mappers hand over) to the synchronised x, padding
    mask, and the four levels' masks and positions, switch off (`_preprocess` as it stands: cast on the host, pageable
    upload of floats, subtract, divide, slice copy and mask fill per frame; then F.interpolate + sine_position per level)
    and on (stage_frames + ingest_frames + level_constants).  Per round two figures: the host wall clock from the frames to
    a device synchronise, and the HIP-event region of the same stretch.  Shapes: 10 frames of 360 x 640, 5 of 720 x 1280,
    and 36 of 720 x 1280 in chunks of 10.
(b) kernel launches and copies of both variants for the first shape, from torch.profiler, in a pass of their own.
(c) SeqFormer-R50 (random weights) fed with CPU uint8 frames both ways: the 36-frame 360p video (`inference`, graph
    replay) and the eager fp32 training step of two 360p clips; wall clock, synchronised on both sides; and the launch
    count of one training step of each variant.

    python tools/time_ingest.py [--out FILE.json] [--rounds N] [--warmup N] [--model-rounds N] [--no-model]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DEV = "cuda:0"


def stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "rounds_ms": list(ts)}


def timed(call):
    """-> (host wall clock from the call to a device synchronise, HIP-event region of the same stretch), ms"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    call()
    end.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, start.elapsed_time(end)


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
            name = ev.name.lower()
            if "memcpy" in name or "copy" in name and "kernel" not in name:
                copies += 1
            else:
                kernels += 1
    return {"kernels": kernels, "copies": copies}


def uint8_frames(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g) for _ in range(n)]


def level_sizes(H, W):
    """the four pyramid levels of a padded H x W input: strides 8, 16, 32 and the 3 x 3 stride-2 convolution on the last"""
    return [(H // 8, W // 8), (H // 16, W // 16), (H // 32, W // 32), ((H // 32 + 1) // 2, (W // 32 + 1) // 2)]


def entry(model, frames, chunk, on):
    """CPU uint8 frames -> x, mask, level masks and positions of every chunk, on the device"""
    from vnext_amd.ops.ingest import sine_position
    from vnext_amd.ops import ingest
    model.device_ingest = on
    out = []
    for s in range(0, len(frames), chunk):
        pre = model._preprocess([{"image": frames[s:s + chunk]}])
        x, mask = pre[:2]
        sizes = level_sizes(*x.shape[-2:])
        if on:
            out.append((x, mask) + ingest.level_constants(pre[2], x.shape[0], x.shape[-2], x.shape[-1], sizes, 128))
        else:
            masks = [F.interpolate(mask[None].float(), size=s_).to(torch.bool)[0] for s_ in sizes]
            out.append((x, mask, masks, [sine_position(mk, 128) for mk in masks]))
    return out


def entry_case(model, n, h, w, chunk, rounds, warmup):
    frames = uint8_frames(n, h, w, seed=n + h)
    times = {"off": [], "on": []}
    with torch.no_grad():
        for r in range(rounds + warmup):
            for key, on in (("off", False), ("on", True)):
                t = timed(lambda: entry(model, frames, chunk, on))
                if r >= warmup:
                    times[key].append(t)
        a, b = entry(model, frames, chunk, False), entry(model, frames, chunk, True)
        same = all(torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]) and all(torch.equal(u, v) for u, v in zip(p[2], q[2]))
                   for p, q in zip(a, b))
        pos_diff = max(float((u - v).abs().max()) for p, q in zip(a, b) for u, v in zip(p[3], q[3]))
    res = {"frames": n, "height": h, "width": w, "chunk": chunk, "uint8_megabytes": n * 3 * h * w / 1e6,
           "x_and_masks_equal": bool(same), "largest_position_difference": pos_diff}
    for key, v in times.items():
        res["switch_" + key] = {"host_wall_clock": stats([t[0] for t in v]), "event_region": stats([t[1] for t in v])}
    return res


def model_cases(rounds, warmup):
    import vnext_amd.models  # noqa: F401
    from vnext_amd import train
    from vnext_amd.registry import build_model, get_seqformer_cfg
    torch.manual_seed(0)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": DEV})).eval()
    video = [{"image": uint8_frames(36, 360, 640, seed=1), "height": 360, "width": 640}]
    res = {}
    times = {"off": [], "on": []}
    for r in range(rounds + warmup):
        for key, on in (("off", False), ("on", True)):
            train.enable_device_ingest(model, on)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.inference(video)
            torch.cuda.synchronize()
            if r >= warmup:
                times[key].append((time.perf_counter() - t0) * 1e3)
    res["video_36x360p"] = {"graph_inference": True, "input": "CPU uint8 frames", "switch_off": stats(times["off"]),
                            "switch_on": stats(times["on"])}
    model._graphs.clear()
    model.train()
    optimizer = train.build_optimizer(model)
    clips = train.synthetic_clips(2, model.num_frames, 360, 640, DEV, seed=2)
    for c in clips:
        c["image"] = [f.to(torch.uint8).cpu() for f in c["image"]]
    times = {"off": [], "on": []}
    for r in range(rounds + warmup):
        for key, on in (("off", False), ("on", True)):
            train.enable_device_ingest(model, on)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            train.train_step(model, optimizer, clips)
            torch.cuda.synchronize()
            if r >= warmup:
                times[key].append((time.perf_counter() - t0) * 1e3)
    step = {"clips": 2, "frames_per_clip": model.num_frames, "height": 360, "width": 640, "precision": "fp32, eager",
            "input": "CPU uint8 frames", "switch_off": stats(times["off"]), "switch_on": stats(times["on"])}
    try:
        launches = {}
        for key, on in (("off", False), ("on", True)):
            train.enable_device_ingest(model, on)
            launches["switch_" + key] = counts(lambda: train.train_step(model, optimizer, clips))
        step["launches_and_copies"] = launches
    except Exception as e:      # no device tracer in this torch build: the counts are not measured
        step["launches_and_copies"] = {"not_measured": repr(e)}
    train.enable_device_ingest(model, False)
    res["eager_step_2x360p"] = step
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest.json"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model-rounds", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ingest.py: needs an MI355X (no CPU fallback for timings)")
    import vnext_amd.models  # noqa: F401
    from vnext_amd.registry import build_model, get_seqformer_cfg
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup, "frames_to_inputs": {}}
    torch.manual_seed(0)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": DEV})).eval()
    for name, (n, h, w, chunk) in (("10x360x640", (10, 360, 640, 10)), ("5x720x1280", (5, 720, 1280, 5)),
                                   ("36x720x1280_chunks_of_10", (36, 720, 1280, 10))):
        res["frames_to_inputs"][name] = entry_case(model, n, h, w, chunk, a.rounds, a.warmup)
    frames = uint8_frames(10, 360, 640, seed=370)
    try:
        with torch.no_grad():
            res["launches_and_copies_10x360x640"] = {"switch_off": counts(lambda: entry(model, frames, 10, False)),
                                                     "switch_on": counts(lambda: entry(model, frames, 10, True))}
    except Exception as e:
        res["launches_and_copies_10x360x640"] = {"not_measured": repr(e)}
    del model
    if not a.no_model:
        res["seqformer_r50"] = model_cases(a.model_rounds, 2)
    res["timing"] = ("frames_to_inputs: CPU uint8 frames to x, mask and four levels of masks and positions; host wall clock "
                     "from the call to a device synchronise and the HIP-event region of the same stretch, switch off / on "
                     "alternating per round.  seqformer_r50: wall clock around inference / train_step, synchronised on "
                     "both sides, switch off / on alternating; the launch counts in a pass of their own")
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
