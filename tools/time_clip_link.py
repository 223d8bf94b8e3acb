"""Time SeqFormer's clip linkage on the host and on the device.  MI355X only.

Per-clip update: n = 10 instances, T = 5 frames, clips every frame (CLIP_LENGTH 5, CLIP_STRIDE 1, so four stored clips
share frames with the incoming one), masks of 90 x 160 and 184 x 320, K = 40;
  host    Videos.update on a Clips object      (a loop of small launches per stored clip, two copies to the host, scipy)
  device  DeviceVideos.update_logits           (ops/clip_link.py: three launches, nothing copied)
Both paths take the same clip of a planted video in a steady state (the ring full), alternating in one process.  Per
round and path two figures: the HIP-event region around the call, and the host wall clock from the call to its return
WITHOUT a device synchronise -- how long the host is held, which is what the linkage costs a caller that wants to run
ahead of the device.  Medians over the rounds after warm-up, with min and max; every round is kept in the file.  The
launch and copy counts of one update of each path come from torch.profiler, in a pass of their own.

Whole video: a 36-frame 360p video through SeqFormer-R50 (random weights) with CLIP_MATCHING and graph_inference, the
switch off and on alternating, wall clock around `model.inference` with a device synchronise on both sides.

    python tools/time_clip_link.py [--out FILE.json] [--rounds N] [--warmup N] [--video-rounds N] [--no-video]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

DEV = "cuda:0"


def stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "rounds_ms": list(ts)}


def timed(call):
    """-> (HIP-event region, host wall clock until the call returns), ms"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    t0 = time.perf_counter()
    call()
    host = (time.perf_counter() - t0) * 1e3
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end), host


def counts(call):
    """kernel launches, memory copies and device-to-host copies of one call (torch.profiler, device activities)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    kernels = copies = to_host = 0
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            name = ev.name.lower()
            if "memcpy" in name or "copy" in name and "kernel" not in name:
                copies += 1
                to_host += "dtoh" in name or "device -> host" in name
            else:
                kernels += 1
    return {"kernels": kernels, "copies": copies, "device_to_host": to_host}


def planted_clips(n, T, h, w, K, clips, seed):
    """`clips` consecutive clips (stride 1) of n instances: n drifting rectangles of +4 on a background of -8 with
    N(0, 0.5^2) noise, permuted per clip -- every instance of a clip finds its track in the stored ones"""
    g = torch.Generator().manual_seed(seed)
    boxes = [(int(torch.randint(4, h // 2, (1,), generator=g)), int(torch.randint(4, w // 2, (1,), generator=g)),
              int(torch.randint(0, h // 2, (1,), generator=g)), int(torch.randint(0, w // 2, (1,), generator=g)))
             for _ in range(n)]
    out = []
    for c in range(clips):
        logits = torch.full((n, T, h, w), -8.0)
        for i, (bh, bw, y, x) in enumerate(boxes):
            for k in range(T):
                d = (c + k) % 8
                logits[i, k, y + d:y + d + bh, x + d:x + d + bw] = 4.0
        logits = (logits + 0.5 * torch.randn(n, T, h, w, generator=g))[torch.randperm(n, generator=g)]
        out.append((list(range(c, c + T)), torch.rand(n, K, generator=g).to(DEV), logits.to(DEV)))
    return out


def as_clip(frames, cls, logits):
    from vnext_amd.models.clip_matching import Clips
    score, label = cls.max(-1)
    return Clips(frames, types.SimpleNamespace(pred_classes=label, scores=score, cls_probs=cls, pred_masks=logits))


def per_clip(h, w, rounds, warmup, n=10, T=5, K=40):
    from vnext_amd.models.clip_matching import DeviceVideos, Videos
    steady = T + 1                                   # clips before the timed ones: the ring is full
    total = steady + 2 * (rounds + warmup) + 2
    clips = planted_clips(n, T, h, w, K, total, seed=h)
    L = total + T
    host, dev = Videos(T, L, K, (h, w), DEV), DeviceVideos(T, L, K, (h, w), DEV, capacity=4 * n, max_instances=n)
    ids = []
    for c in clips[:steady]:
        host.update(as_clip(*c))
        ids.append(dev.update_logits(*c))
    same = [i.cpu().tolist() for i in ids] == [c[1].cpu().tolist() for c in host.clips]
    times = {"host": [], "device": []}
    for r, c in enumerate(clips[steady:steady + rounds + warmup]):
        # the host path makes its sigmoid copy inside Clips: part of what an update costs there
        th = timed(lambda: host.update(as_clip(*c)))
        td = timed(lambda: ids.append(dev.update_logits(*c)))
        if r >= warmup:
            times["host"].append(th)
            times["device"].append(td)
    same = same and ids[-1].cpu().tolist() == host.clips[-1][1].cpu().tolist()
    out = {k: {"event_region": stats([e for e, _ in v]), "host_wall_clock": stats([s for _, s in v])}
           for k, v in times.items()}
    out.update(instances=n, frames=T, height=h, width=w, classes=K, same_ids=bool(same), tracks=dev.counters()[0])
    nxt = clips[steady + rounds + warmup]
    try:
        out["launches_and_copies"] = {"host": counts(lambda: host.update(as_clip(*nxt))),
                                      "device": counts(lambda: dev.update_logits(*nxt))}
    except Exception as e:      # no device tracer in this torch build: the counts are not measured
        out["launches_and_copies"] = {"not_measured": repr(e)}
    return out


def whole_video(rounds, warmup):
    import vnext_amd.models  # noqa: F401
    from vnext_amd import train
    from vnext_amd.registry import build_model, get_seqformer_cfg
    torch.manual_seed(0)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": DEV, "MODEL.SeqFormer.CLIP_MATCHING": True})).eval()
    model.graph_inference = True
    g = torch.Generator().manual_seed(1)
    video = [{"image": [(torch.rand(3, 360, 640, generator=g) * 255).to(DEV) for _ in range(36)], "height": 360,
              "width": 640}]
    times = {"off": [], "on": []}
    for r in range(rounds + warmup):
        for key, on in (("off", False), ("on", True)):
            train.enable_device_clip_matching(model, on)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.inference(video, rle=True)
            torch.cuda.synchronize()
            if r >= warmup:
                times[key].append((time.perf_counter() - t0) * 1e3)
    train.enable_device_clip_matching(model, False)
    return {"frames": 36, "height": 360, "width": 640, "backbone": "R-50", "clip_length": model.clip_length,
            "clip_stride": model.clip_stride, "graph_inference": True, "switch_off": stats(times["off"]),
            "switch_on": stats(times["on"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_link_timing.json"))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--video-rounds", type=int, default=5)
    ap.add_argument("--no-video", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_clip_link.py: needs an MI355X (no CPU fallback for timings)")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup, "per_clip": {}}
    for h, w in ((90, 160), (184, 320)):
        res["per_clip"][f"{h}x{w}"] = per_clip(h, w, a.rounds, a.warmup)
    if not a.no_video:
        res["whole_video"] = whole_video(a.video_rounds, 1)
    res["timing"] = ("per clip: device events around each update and the host wall clock until the call returns (no "
                     "synchronise inside the region), a device synchronise before and after; host / device alternating "
                     "per round.  whole video: wall clock around inference, synchronised on both sides, switch off / on "
                     "alternating")
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
