"""Time IDOL's reid stage: the per-image loop of `reid_terms` + `heads.loss_reid` against the fused op.
MI355X only.

Both paths run forward + backward of the same stage -- from the two embedding views `embeds[0::2]` / `embeds[1::2]` to
the two loss scalars and back to `embeds.grad` -- on the same embeddings [2 B, Q, C], matched ids and selections,
alternating in one process: one round = one timed call of each, the unfused path first, device events around the call,
medians over the rounds after warm-up, with min / max.  The selections are synthetic with the set sizes simOTA gives on the
bench's IDOL leg (a handful of positives per instance, nearly every other query negative, aux = the positives + ten times
as many negatives).  Launch counts come from torch.profiler in a separate pass after the timing (the profiler is off while
timing).
--steps: also `train.train_step` un-instrumented on the bench's IDOL leg (one 720 x 1280 pair, 8 objects), fp32 and bf16
autocast, switch off / on alternating three times, each figure the median of 25 steps after 5 warm-up steps (the protocol
of DESIGN section 11), and the launches of one step each way.

    python tools/time_reid_loss.py [--out FILE.json] [--rounds N] [--fused-only] [--steps]
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

SHAPES = [  # (name, B, Q = R, C, instances per image): the bench's IDOL leg, then two pairs of six objects
    ("idol_leg", 1, 300, 256, (8,)),
    ("two_pairs", 2, 300, 256, (6, 6)),
]


def make_case(B, Q, C, counts, dev, seed=0):
    """embeds [2 B, Q, C], matched ids and per-image (inst, pos, neg, aux) as the matcher and sample_aux_masks give them"""
    g = torch.Generator().manual_seed(seed)
    embeds = torch.randn(2 * B, Q, C, generator=g).to(dev)
    matched, sel = [], []
    for n in counts:
        pos = torch.zeros(Q, n, dtype=torch.bool)
        for c in range(n):
            pos[torch.randperm(Q, generator=g)[:int(torch.randint(2, 8, (1,), generator=g))], c] = True
        neg = ~pos & (torch.rand(Q, n, generator=g) < 0.95)
        aux = pos.clone()
        for c in range(n):
            rows = torch.nonzero(neg[:, c]).flatten()
            aux[rows[torch.randperm(len(rows), generator=g)[:10 * int(pos[:, c].sum())]], c] = True
        sel.append((torch.arange(n), pos, neg, aux))
        matched.append(torch.randperm(Q, generator=g)[:n])
    return embeds, matched, sel


def stage(fused, embeds, matched, sel):
    from vnext_amd.heads import loss_reid
    from vnext_amd.models.idol_criterion import reid_terms, reid_terms_fused
    e = embeds.detach().requires_grad_(True)
    if fused:
        qd = reid_terms_fused(e[0::2], e[1::2], matched, sel)
    else:
        qd = reid_terms(e[0::2], e[1::2], matched, sel, loss_reid)
    a, b = qd["contrast"] / qd["count"], qd["aux"] / qd["count"]
    (2.0 * a + 3.0 * b).backward()
    return a.detach(), b.detach(), e.grad


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
    copies = sum(1 for n in names if n.lower().startswith(("memcpy", "memset")))
    return {"kernels": len(names) - copies, "copies": copies}


def stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def wall(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def time_steps(model, opt, clips, autocast, repeats=3, steps=25, warmup=5):
    from vnext_amd import train as T

    def one():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            return T.train_step(model, opt, clips)
    out = {"off": [], "on": []}
    for _ in range(repeats):
        for name, on in (("off", False), ("on", True)):
            T.enable_fused_reid_loss(model, on)
            for _ in range(warmup):
                one()
            out[name].append(statistics.median([wall(one) for _ in range(steps)]))
    counts = {}
    for name, on in (("off", False), ("on", True)):
        T.enable_fused_reid_loss(model, on)
        try:
            counts[name] = launches(one)
        except Exception as e:
            counts[name] = "not measured: %s" % e
    T.enable_fused_reid_loss(model, False)
    return {"median_ms_of_25_steps_per_repeat": out, "off_median_ms": statistics.median(out["off"]),
            "on_median_ms": statistics.median(out["on"]), "off_spread_ms": max(out["off"]) - min(out["off"]),
            "launches_per_step": counts}


def steps_section():
    import vnext_amd.models  # noqa: F401
    from vnext_amd import train as T
    from vnext_amd import tuning
    from vnext_amd.registry import build_model, get_idol_cfg
    tuning.enable()
    torch.manual_seed(0)
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": "cuda:0"})).train()
    opt = T.build_optimizer(model, base_lr=1e-4)
    clips = T.synthetic_clips(1, 2, 720, 1280, "cuda:0", seed=8, num_instances=8)
    out = {"clips": 1, "frames": 2, "height": 720, "width": 1280, "instances": 8}
    for label, autocast in (("fp32", False), ("bf16", True)):
        out["train_step_" + label] = time_steps(model, opt, clips, autocast)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true", help="the fused path alone (for a rocprofv3 --kernel-trace run)")
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--steps", action="store_true", help="also train.train_step on the IDOL leg with the switch off / on")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_reid_loss.py: needs an MI355X (no CPU fallback for timings)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "shapes": []}
    for name, B, Q, C, counts in SHAPES:
        case = make_case(B, Q, C, counts, dev)
        paths = {}
        if not a.fused_only:
            paths["unfused"] = lambda: stage(False, *case)      # unfused first: the fused figure follows the one it is compared with
        paths["fused"] = lambda: stage(True, *case)
        for _ in range(a.warmup):
            for call in paths.values():
                call()
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        for _ in range(a.rounds):                       # alternating: one call of each per round
            for k, call in paths.items():
                times[k].append(timed(call))
        entry = {"name": name, "B": B, "Q": Q, "R": Q, "C": C, "J": sum(counts)}
        for k in paths:
            entry[k + "_fwd_bwd"] = stats(times[k])
        if not a.fused_only:
            ru, rf = paths["unfused"](), paths["fused"]()
            entry["max_abs_difference"] = {"loss_reid": float((ru[0] - rf[0]).abs()), "loss_reid_aux": float((ru[1] - rf[1]).abs()),
                                           "embeds_grad": float((ru[2] - rf[2]).abs().max())}
            entry["speedup_median"] = statistics.median(times["unfused"]) / statistics.median(times["fused"])
            entry["fused_median_below_unfused_min"] = statistics.median(times["fused"]) < min(times["unfused"])
            entry["rounds_fused_below_unfused"] = sum(1 for x, y in zip(times["unfused"], times["fused"]) if y < x)
        if not a.no_launch_count and not a.fused_only:
            try:
                entry["launches_fwd_bwd"] = {k: launches(call) for k, call in paths.items()}
            except Exception as e:                      # a profiler that does not start costs the count, not the timings
                entry["launches_fwd_bwd"] = "not measured: %s" % e
        res["shapes"].append(entry)
    if a.steps:
        res["steps"] = steps_section()
    res["timing"] = ("device events around one forward + backward of the reid stage (embedding views -> two loss scalars -> "
                     "embeds.grad), profiler off, paths alternating per round, unfused first")
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
