"""Time the mask losses (focal + dice) of the criteria: the ATen composition against the fused kernel.
MI355X only.

Both paths run forward + backward on the same logits [R, F, h, w], ground truth and row -> target indices, alternating
in one process: one round = one timed call of each, device events around the call, medians over the rounds after
warm-up, with min / max.  The ATen path is the expression of `SetCriterion.forward_all_layers` (slice, cast, pad, cat,
gather, the element-wise chain, the row sums) from `t["masks"]` on; the fused path is `ops.mask_loss.mask_focal_dice`.
Launch counts come from torch.profiler in a separate pass after the timing (the profiler is off while timing).
Algorithmic bytes: forward 4 B of logits + the sampled ground-truth byte per element, backward the same + 4 B written;
`fused_*_GBps` is those bytes over the EVENT time of the whole call (launch gaps included), not a kernel's rate --
kernel times come from `rocprofv3 --kernel-trace --stats -- python tools/time_mask_loss.py --fused-only`.

    python tools/time_mask_loss.py [--out FILE.json] [--rounds N] [--fused-only]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = [  # (R, F, h, w, clips, stride): Ld = 6 layers x 4 instances of one 360p clip; 6 x 20 instances over two 720p clips
    (24, 5, 90, 160, 1, 4),
    (120, 5, 180, 320, 2, 4),
]


def make_case(R, frames, h, w, clips, stride, dev, layers=6, seed=0):
    """logits, per-clip bool ground truth at image resolution (blobs), row_gt (every target once per layer)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    n = R // layers
    per = [n // clips + (1 if i < n % clips else 0) for i in range(clips)]
    H, W = h * stride, w * stride
    yy = torch.arange(H, device=dev, dtype=torch.float32)[:, None]
    xx = torch.arange(W, device=dev, dtype=torch.float32)[None, :]
    gts = []
    for k in per:
        cy = torch.rand(k, frames, 1, 1, device=dev, generator=g) * H
        cx = torch.rand(k, frames, 1, 1, device=dev, generator=g) * W
        rad = H / 12 + torch.rand(k, frames, 1, 1, device=dev, generator=g) * H / 4
        gts.append(((yy - cy) ** 2 + (xx - cx) ** 2) < rad * rad)
    row_gt = torch.arange(n, device=dev).repeat(layers)
    logits = torch.randn(R, frames, h, w, device=dev, generator=g) * 3 - 1
    return logits, gts, row_gt


def aten_rows(logits, gts, row_gt, stride, alpha=0.25, gamma=2.0):
    """the criteria's expression (their own term functions), from t["masks"] to the per-row focal mean and dice"""
    from vnext_amd.models.criterion import dice_term, focal_term, gt_canvas
    h, w = logits.shape[-2:]
    gt = gt_canvas(gts, stride, h, w, logits.dtype)[row_gt].flatten(1)
    src = logits.flatten(1)
    pm = src.sigmoid()
    return focal_term(src, gt, alpha, gamma, p=pm).mean(1), dice_term(pm, gt)


def fused_rows(logits, gts, row_gt, stride):
    from vnext_amd.ops.mask_loss import mask_focal_dice
    return mask_focal_dice(logits, gts, row_gt, stride)


def step(fn, logits, gts, row_gt, stride, wf, wd):
    x = logits.detach().requires_grad_(True)
    focal, dice = fn(x, gts, row_gt, stride)
    ((focal * wf).sum() + (dice * wd).sum()).backward()
    return x.grad


def timed(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def launches(call):
    from torch.profiler import ProfilerActivity, profile
    call()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        call()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len(names)


def stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true", help="the fused op alone (for a rocprofv3 --kernel-trace run)")
    ap.add_argument("--no-launch-count", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mask_loss.py: needs an MI355X (no CPU fallback for timings)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "shapes": []}
    for R, frames, h, w, clips, stride in SHAPES:
        logits, gts, row_gt = make_case(R, frames, h, w, clips, stride, dev)
        g = torch.Generator(device=dev).manual_seed(1)
        wf, wd = torch.rand(R, device=dev, generator=g), torch.rand(R, device=dev, generator=g)
        paths = {"fused": lambda: step(fused_rows, logits, gts, row_gt, stride, wf, wd)}
        if not a.fused_only:
            paths["aten"] = lambda: step(aten_rows, logits, gts, row_gt, stride, wf, wd)
        for _ in range(a.warmup):
            for call in paths.values():
                call()
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        for _ in range(a.rounds):                       # alternating: one call of each per round
            for k, call in paths.items():
                times[k].append(timed(call))
        elems = R * frames * h * w
        entry = {"R": R, "F": frames, "h": h, "w": w, "clips": clips, "stride": stride, "elements": elems,
                 "algorithmic_bytes": {"forward": 5 * elems, "backward": 9 * elems}}
        for k in paths:
            entry[k + "_fwd_bwd"] = stats(times[k])
        entry["fused_fwd_bwd_GBps_over_event_time"] = 14 * elems / (statistics.median(times["fused"]) * 1e-3) / 1e9
        if not a.fused_only:
            ga, gf = paths["aten"](), paths["fused"]()
            entry["max_abs_grad_difference"] = float((ga - gf).abs().max())
            entry["speedup_median"] = statistics.median(times["aten"]) / statistics.median(times["fused"])
        if not a.no_launch_count and not a.fused_only:
            try:
                entry["launches_fwd_bwd"] = {k: launches(call) for k, call in paths.items()}
            except Exception as e:                      # a profiler that does not start costs the count, not the timings
                entry["launches_fwd_bwd"] = "not measured: %s" % e
        res["shapes"].append(entry)
    res["timing"] = ("device events around one forward + backward call (loss weights applied, .backward() included), "
                     "profiler off, paths alternating per round")
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
