"""Time the dense mask stage: mask logits -> thresholded masks at the output size.  MI355X only.

  (a) op level: `ops.mask_dense.masks_from_logits` against the eager chain it replaces (bilinear x stride, sigmoid, crop,
      nearest, > 0.5: `ops.mask_dense.host_masks`, the expression the models keep for the switch off) on the same logits,
      alternating, device events around each call, median of `--rounds` after `--warmup`; the peak of device memory over
      one call of each; the kernel's output bytes per second.  Workloads:
        video  360 maps of 180 x 320 -> (720, 1280) -> (720, 1280)      10 queries x 36 frames at 720p
        coco   100 maps of 200 x 304 -> (800, 1216) -> (480, 640)       one COCO image's top 100
      The `bits` form is timed beside them (no eager counterpart: `np.packbits` is host work).
  (b) the video branches' other half: `.cpu()` of the bool masks the op returns (what `_report` and `_track_masks` then do).
  (c) model level: a 36-frame 720p video through SeqFormer-R50's `model(inputs)`, switch off and on alternating, host clock
      around the whole call.  Random-init weights, so the model reports each of its 10 queries under its best class
      (`multi_cls` off): 360 masks, the op-level video workload.

    python tools/time_mask_dense.py [--out FILE.json] [--skip-models] [--rounds N] [--warmup N]
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

from tools.time_mask_rle import logit_field  # noqa: E402

WORKLOADS = {"video": (360, 180, 320, (720, 1280), (720, 1280)), "coco": (100, 200, 304, (800, 1216), (480, 640))}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def summary(times):
    return {"median": statistics.median(times), "min": min(times), "max": max(times), "all": times}


def alternating(legs, rounds, warmup, timer):
    """legs {name: fn} -> {name: [time per round]}: every round runs each leg once, in turn"""
    times = {k: [] for k in legs}
    for r in range(warmup + rounds):
        for k, fn in legs.items():
            t = timer(fn)
            if r >= warmup:
                times[k].append(t)
    return times


def op_leg(name, rounds, warmup, dev):
    from vnext_amd.ops.mask_dense import host_masks, masks_from_logits
    M, h, w, image, out = WORKLOADS[name]
    logits = logit_field(M, h, w, dev, seed=len(name))
    legs = {"eager_chain": lambda: host_masks(logits, 4, image, out),
            "device_u8": lambda: masks_from_logits(logits, 4, image, out),
            "device_bits": lambda: masks_from_logits(logits, 4, image, out, bits=True)}
    differing = int((legs["eager_chain"]() != legs["device_u8"]()).sum())
    times = alternating(legs, rounds, warmup, event_ms)
    res = {"masks": M, "logits": [h, w], "image": list(image), "out": list(out), "output_pixels": M * out[0] * out[1],
           "pixels_differing_from_the_eager_chain": differing,
           "ms": {k: summary(v) for k, v in times.items()},
           "peak_bytes": {k: peak_bytes(fn) for k, fn in legs.items()},
           "timing": "device events around one call, the legs alternating; peak_bytes = max_memory_allocated over one call, "
                     "the result included"}
    u8, eager = res["ms"]["device_u8"], res["ms"]["eager_chain"]
    res["u8_output_bytes_per_s"] = res["output_pixels"] / (u8["median"] * 1e-3)
    res["speedup_median"] = eager["median"] / u8["median"]
    res["bar_device_not_above_eager_by_more_than_the_spread"] = bool(
        u8["median"] <= eager["median"] + max(eager["max"] - eager["min"], u8["max"] - u8["min"]))
    masks = legs["device_u8"]()
    torch.cuda.synchronize()

    def copy():
        t0 = time.perf_counter()
        masks.cpu()
        return 1e3 * (time.perf_counter() - t0)
    cp = [copy() for _ in range(warmup + rounds)][warmup:]
    res["device_to_host_copy_ms"] = summary(cp)
    res["device_to_host_copy_bytes_per_s"] = res["output_pixels"] / (statistics.median(cp) * 1e-3)
    return res


def model_leg(rounds, warmup, dev):
    import vnext_amd.models  # noqa: F401  (registers the meta-architectures)
    from vnext_amd import train as T
    from vnext_amd.registry import build_model, get_seqformer_cfg
    g = torch.Generator(device=dev).manual_seed(1)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": str(dev)})).eval()
    model.multi_cls = False      # one label per query: 10 pairs x 36 frames whatever the untrained class scores are
    video = [{"video_id": 1, "image": [torch.rand(3, 720, 1280, device=dev, generator=g) * 255 for _ in range(36)],
              "height": 720, "width": 1280}]

    def run(on):
        def fn():
            T.enable_device_masks(model, on)
            return model(video)
        return fn

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)
    res = run(True)()
    times = alternating({"switch_off": run(False), "switch_on": run(True)}, rounds, warmup, wall)
    return {"model": "SeqFormer-R50, 36 frames at 720p, random-init weights", "reported_pairs": len(res["pred_scores"]),
            "ms": {k: summary(v) for k, v in times.items()},
            "peak_bytes": {"switch_off": peak_bytes(run(False)), "switch_on": peak_bytes(run(True))},
            "timing": "host clock around model(inputs), ending in a synchronise; the legs alternating"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-models", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mask_dense.py: needs an MI355X (no CPU fallback for timings)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup}
    for name in WORKLOADS:
        res["op_" + name] = op_leg(name, a.rounds, a.warmup, dev)
    if not a.skip_models:
        res["model_seqformer"] = model_leg(a.rounds, a.warmup, dev)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
