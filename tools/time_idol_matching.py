"""Time IDOL's matching phase -- simOTA matching of every (decoder layer, key image) and the contrastive sets of every
reference image -- on the host and on the device, and the training step both ways.  MI355X only.

Matching phase: the trunk runs once; on its outputs, one round = one timed call of each path, alternating in one process,
host clock with a device synchronisation before and after, medians over the rounds after warm-up, with min / max.
  host    OTAMatcher.match_all_layers + pos_neg_masks          (copies logits, boxes, targets to the host, ATen CPU ops)
  device  OTAMatcher.match_all_layers_device                   (one kernel, one copy of the compact result)
Step: `train.train_step` un-instrumented, fp32 and bf16 autocast, host / device alternating three times, each figure the
median of 25 steps after 5 warm-up steps (the protocol of DESIGN section 11).
Kernel time: `rocprofv3 --kernel-trace --stats -- python tools/time_idol_matching.py --device-only`, a run of its own.

    python tools/time_idol_matching.py [--out FILE.json] [--rounds N] [--no-steps] [--device-only]
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

CASES = {  # name: (pairs, height, width, objects per pair)
    "bench_idol_leg_1x720p_8obj": (1, 720, 1280, 8),
    "two_pairs_720p_6obj": (2, 720, 1280, 6),
}


def stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def wall(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def matching_inputs(model, pairs, autocast):
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        det_t, ref_t = model.prepare_targets(pairs)
        frames = [f for video in pairs for f in video["image"]]
        hs, logits, boxes, ref_xy, ref_last, feats, ref_logits, embeds = model._train_trunk(*model._preprocess(frames))
    return logits, boxes, det_t, ref_last, ref_logits, ref_t


def time_matching(model, pairs, autocast, rounds, warmup, device_only=False):
    from vnext_amd.models.idol_criterion import pos_neg_masks
    logits, boxes, det_t, ref_last, ref_logits, ref_t = matching_inputs(model, pairs, autocast)
    m = model.criterion.matcher

    def host():
        return m.match_all_layers(logits, boxes, det_t), pos_neg_masks(ref_last, ref_logits.sigmoid(), ref_t)

    def device():
        return m.match_all_layers_device(logits, boxes, det_t, ref=(ref_last, ref_logits.sigmoid(), ref_t))
    paths = {"device": device} if device_only else {"host": host, "device": device}
    for _ in range(warmup):
        for call in paths.values():
            call()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for k, call in paths.items():
            times[k].append(wall(call))
    out = {k: stats(v) for k, v in times.items()}
    out["logits_dtype"] = str(logits.dtype)
    out["targets"] = [len(t["labels"]) for t in det_t]
    if not device_only:
        out["device_below_host_in_every_round"] = all(d < h for d, h in zip(times["device"], times["host"]))
        out["device_max_below_host_min"] = max(times["device"]) < min(times["host"])
        (ind_h, matched_h), sel_h = host()
        ind_d, matched_d, sel_d = device()
        out["same_indices"] = all(torch.equal(a, b) for lh, ld in zip(ind_h, ind_d) for x, y in zip(lh, ld) for a, b in zip(x, y)) and \
            all(torch.equal(a, b) for a, b in zip(matched_h, matched_d)) and \
            all(torch.equal(a, b) for x, y in zip(sel_h, sel_d) for a, b in zip(x, y))
    return out


def time_steps(model, opt, pairs, autocast, repeats=3, steps=25, warmup=5):
    from vnext_amd import train as T

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            return T.train_step(model, opt, pairs)
    out = {"host": [], "device": []}
    for _ in range(repeats):
        for name, on in (("host", False), ("device", True)):
            T.enable_device_matching(model, on)
            for _ in range(warmup):
                step()
            ts = [wall(step) for _ in range(steps)]
            out[name].append(statistics.median(ts))
    T.enable_device_matching(model, False)
    return {"median_ms_of_25_steps_per_repeat": out,
            "host_median_ms": statistics.median(out["host"]), "device_median_ms": statistics.median(out["device"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-steps", action="store_true", help="the matching phase only")
    ap.add_argument("--device-only", action="store_true", help="the device path's matching phase alone (for a rocprofv3 run)")
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_idol_matching.py: needs an MI355X (no CPU fallback for timings)")
    import vnext_amd.models  # noqa: F401
    from vnext_amd import train as T
    from vnext_amd import tuning
    from vnext_amd.registry import build_model, get_idol_cfg
    tuning.enable()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": str(dev)})).train()
    opt = None if a.no_steps or a.device_only else T.build_optimizer(model, base_lr=1e-4)
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": {}}
    for name in a.cases.split(","):
        pairs_n, h, w, objects = CASES[name]
        pairs = T.synthetic_clips(pairs_n, 2, h, w, dev, seed=8, num_instances=objects)
        entry = {"pairs": pairs_n, "height": h, "width": w, "objects_per_pair": objects}
        for label, autocast in (("fp32", False), ("bf16", True)):
            entry["matching_" + label] = time_matching(model, pairs, autocast, a.rounds, a.warmup, a.device_only)
        if opt is not None:
            for label, autocast in (("fp32", False), ("bf16", True)):
                entry["train_step_" + label] = time_steps(model, opt, pairs, autocast)
        res["cases"][name] = entry
    res["timing"] = ("matching: host clock, device synchronised before and after each call, paths alternating per round; "
                     "train_step: the same clock around un-instrumented steps, host / device alternating three times")
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
