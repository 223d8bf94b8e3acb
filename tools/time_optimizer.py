"""Time the tail of a training step -- gradient clipping + AdamW -- on the eager chain and through the clipped AdamW op
(vnext_amd/ops/optim.py), on the parameter sets of SeqFormer-R50 and IDOL-R50.  MI355X only.

The models are built and their `.grad`s filled with fixed-seed noise (total norm far above the clip's 0.01); no forward runs.
Per model, in a process of its own under its own time limit:
(a) `clip_grad_norm_(params, 0.01)` + `build_optimizer`'s fused AdamW against `build_fused_optimizer`'s `ClippedAdamW.step()`,
    alternating in one process, every round kept: the HIP-event region around the tail, and the host time of the call (the
    wall clock until the call returns, before any synchronisation).  Medians, extremes and the spread (max - min) of the rounds.
(b) kernel launches and copies of both paths from torch.profiler, in a pass of their own, with the op's three kernels' own
    durations.
(c) the bytes the tail must move -- g read for the norm, then g, p, m, v read and p, m, v written: 32 B per parameter -- and
    the share of 6.3 TB/s the op's median region reaches.
The op counts as faster when its median lies below the eager median by more than the larger spread of the two.

    python tools/time_optimizer.py [--out FILE.json] [--rounds N] [--warmup N] [--models seqformer,idol] [--timeout S]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda:0"
HBM_BYTES_PER_S = 6.3e12
BYTES_PER_PARAMETER = 32


def stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "spread_ms": max(ts) - min(ts),
            "rounds_ms": list(ts)}


def child(name, rounds, warmup, out):
    import torch
    import vnext_amd.models  # noqa: F401
    from vnext_amd import train
    from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg
    torch.manual_seed(0)
    cfg = (get_idol_cfg if name == "idol" else get_seqformer_cfg)(**{"MODEL.DEVICE": DEV})
    model = build_model(cfg).train()
    eager, fused = train.build_optimizer(model), train.build_fused_optimizer(model)
    params = [p for g in eager.param_groups for p in g["params"]]
    gen = torch.Generator(device=DEV).manual_seed(1)

    def fill():
        for p in params:
            p.grad = torch.empty_like(p).normal_(generator=gen).mul_(1e-3)      # in the parameter's own strides

    def eager_tail():
        torch.nn.utils.clip_grad_norm_(params, 0.01)
        eager.step()

    def fused_tail():
        fused.step()

    def timed(call):
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
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize()
        kernels, copies, own = 0, 0, {}
        for ev in prof.events():
            if ev.device_type != torch.autograd.DeviceType.CUDA or ev.name.startswith("Optimizer.step#"):
                continue
            low = ev.name.lower()
            if low.startswith(("memcpy", "memset")):
                copies += 1
                continue
            kernels += 1
            if "adamw_" in low and "vnx" in low:
                key = low.split("adamw_")[1].split("(")[0]
                own[key] = own.get(key, 0.0) + ev.time_range.elapsed_us()
        return {"kernels": kernels, "copies_and_memsets": copies, **({"op_kernel_us": own} if own else {})}

    fill()
    times = {"eager": [], "op": []}
    for r in range(rounds + warmup):
        for key, call in (("eager", eager_tail), ("op", fused_tail)):
            t = timed(call)
            if r >= warmup:
                times[key].append(t)
    numel = sum(p.numel() for p in params)
    res = {"model": name, "parameter_tensors": len(params), "parameters": numel,
           "chunks": int(fused._chunks_host.shape[0]), "bytes_per_step": numel * BYTES_PER_PARAMETER}
    for key, v in times.items():
        res[key] = {"event_region": stats([t[0] for t in v]), "host_time_of_the_call": stats([t[1] for t in v])}
    try:
        res["eager"]["launches"] = counts(eager_tail)
        res["op"]["launches"] = counts(fused_tail)
    except Exception as e:      # no device tracer in this torch build: the counts are not measured
        res["launches_not_measured"] = repr(e)
    med_e, med_o = res["eager"]["event_region"]["median_ms"], res["op"]["event_region"]["median_ms"]
    spread = max(res["eager"]["event_region"]["spread_ms"], res["op"]["event_region"]["spread_ms"])
    res["op"]["share_of_6.3_TB_per_s"] = res["bytes_per_step"] / (med_o * 1e-3) / HBM_BYTES_PER_S
    res["eager"]["share_of_6.3_TB_per_s_on_the_same_bytes"] = res["bytes_per_step"] / (med_e * 1e-3) / HBM_BYTES_PER_S
    res["op_faster_beyond_the_spread"] = bool(med_e - med_o > spread)
    res["total_norm_after_the_rounds"] = float(fused.last_total_norm)
    with open(out, "w") as f:
        json.dump(res, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--models", default="seqformer,idol")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per model")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--part", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.rounds, a.warmup, a.part)
    res = {"rounds": a.rounds, "warmup": a.warmup, "models": {}}
    for name in a.models.split(","):
        # a fresh process per model, under its own time limit; after a failure nothing more is started
        with tempfile.TemporaryDirectory() as tmp:
            part = os.path.join(tmp, "part.json")
            cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--part", part, "--rounds", str(a.rounds),
                   "--warmup", str(a.warmup)]
            done = subprocess.run(cmd, timeout=a.timeout)
            if done.returncode != 0:
                raise SystemExit(f"time_optimizer.py: the {name} run ended with status {done.returncode}; stopping")
            with open(part) as f:
                res["models"][name] = json.load(f)
    res["timing"] = ("event_region: HIP events around clip_grad_norm_ + AdamW.step (eager: build_optimizer's fused AdamW) / "
                     "ClippedAdamW.step (op), the two alternating per round in one process, gradients of fixed-seed noise, no "
                     "forward; host_time_of_the_call: wall clock until the call returns, not synchronised; launches: "
                     "torch.profiler, a pass of their own; bytes_per_step: 32 B per parameter")
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
