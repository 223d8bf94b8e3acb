"""Time the class and box losses of the criteria: the ATen composition against the fused op.
MI355X only.

Both paths run forward + backward of the same expression -- per-layer focal sum over the logits against the implied
one-hot target, the matched boxes' L1 and GIoU sums, the argmax hits -- on the same logits [Ld, N, Q, K], boxes
[Ld, N, T, Q, 4] and pair list, alternating in one process: one round = one timed call of each, device events around the
call, medians over the rounds after warm-up, with min / max.  The ATen path is the lines of
`SetCriterion.forward_all_layers` (SeqFormer legs: `view` sums) or `IDOLCriterion.forward_all_layers` (IDOL leg:
`index_add_` segment sums); the fused path is `ops.set_loss.set_class_box_losses`.  Launch counts come from
torch.profiler in a separate pass after the timing (the profiler is off while timing).
--steps: also `train.train_step` un-instrumented on the bench's two legs (SeqFormer: one 5 x 360 x 640 clip, 4 instances;
IDOL: one 720 x 1280 pair, 8 objects), fp32 and bf16 autocast, switch off / on alternating three times, each figure the
median of 25 steps after 5 warm-up steps (the protocol of DESIGN sections 11 - 13), and the launches of one step each way.

    python tools/time_set_loss.py [--out FILE.json] [--rounds N] [--fused-only] [--steps]
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

SHAPES = [  # (name, Ld, N, T, Q, K, targets per clip, IDOL-shaped): the bench's two legs, then ten clips
    ("seqformer", 6, 2, 5, 300, 40, (2, 2), False),
    ("idol", 6, 2, 1, 300, 40, (4, 4), True),
    ("seqformer_N10", 6, 10, 5, 300, 40, (4,) * 10, False),
]


def make_case(Ld, N, T, Q, K, sizes, idol, dev, seed=0):
    """logits, boxes, the pair list (Hungarian-shaped: every target once per layer; IDOL-shaped: 2 - 5 queries per target,
    another count in every layer), labels, target boxes"""
    g = torch.Generator().manual_seed(seed)
    n_tot = sum(sizes)
    start = [0]
    for n in sizes:
        start.append(start[-1] + n)
    lay, clip, qry, tgt = [], [], [], []
    for l in range(Ld):
        for i, n in enumerate(sizes):
            if idol:
                t = torch.arange(n).repeat_interleave(torch.randint(2, 6, (n,), generator=g))
            else:
                t = torch.randperm(n, generator=g)
            q = torch.randperm(Q, generator=g)[:len(t)].sort().values
            lay.append(torch.full_like(q, l)); clip.append(torch.full_like(q, i)); qry.append(q); tgt.append(t + start[i])
    lay, clip, qry, tgt = (torch.cat(v).to(dev) for v in (lay, clip, qry, tgt))
    box = lambda *s: torch.cat([0.2 + 0.6 * torch.rand(*s, 2, generator=g), 0.05 + 0.4 * torch.rand(*s, 2, generator=g)], -1)   # noqa: E731
    return (torch.randn(Ld, N, Q, K, generator=g).to(dev) * 2 - 2, box(Ld, N, T, Q).to(dev), lay, clip, qry, tgt,
            torch.randint(0, K, (n_tot,), generator=g).to(dev), box(n_tot, T).to(dev))


def aten_sums(logits, boxes, lay, clip, qry, tgt, labels, tgt_boxes, idol, alpha=0.25):
    """the criteria's expression (their own term functions), from the logits to the per-layer sums [Ld, 4]"""
    from vnext_amd.models.criterion import box_terms, focal_term
    Ld, T = logits.shape[0], boxes.shape[2]
    onehot = torch.zeros_like(logits)
    onehot[lay, clip, qry, labels[tgt]] = torch.ones((), dtype=logits.dtype, device=logits.device)
    loss_ce = focal_term(logits, onehot, alpha).mean(2).sum((1, 2)) * logits.shape[2]
    l1, g = box_terms(boxes.transpose(2, 3)[lay, clip, qry], tgt_boxes[tgt])          # [R], [R, T]
    with torch.no_grad():
        hit = (logits[lay, clip, qry].argmax(-1) == labels[tgt]).float()
    if idol:
        seg = lambda v: torch.zeros(Ld, dtype=v.dtype, device=v.device).index_add_(0, lay, v)      # noqa: E731
        return torch.stack([loss_ce, seg(l1), seg(g.flatten()), seg(hit)], 1)
    n = len(lay) // Ld
    return torch.stack([loss_ce, l1.view(Ld, n).sum(1), g.view(Ld, n * T).sum(1), hit.view(Ld, n).sum(1)], 1)


def fused_sums(logits, boxes, lay, clip, qry, tgt, labels, tgt_boxes, idol):
    from vnext_amd.ops.set_loss import set_class_box_losses
    return set_class_box_losses(logits, boxes, lay, clip, qry, tgt, labels, tgt_boxes)


def step(fn, case, idol, w):
    x, b = case[0].detach().requires_grad_(True), case[1].detach().requires_grad_(True)
    out = fn(x, b, *case[2:], idol)
    (out[:, :3] * w).sum().backward()
    return out.detach(), x.grad, b.grad


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
    return len([e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA])


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
            T.enable_fused_set_loss(model, on)
            for _ in range(warmup):
                one()
            out[name].append(statistics.median([wall(one) for _ in range(steps)]))
    counts = {}
    for name, on in (("off", False), ("on", True)):
        T.enable_fused_set_loss(model, on)
        try:
            counts[name] = launches(one)
        except Exception as e:
            counts[name] = "not measured: %s" % e
    T.enable_fused_set_loss(model, False)
    return {"median_ms_of_25_steps_per_repeat": out, "off_median_ms": statistics.median(out["off"]),
            "on_median_ms": statistics.median(out["on"]), "launches_per_step": counts}


def steps_section():
    import vnext_amd.models  # noqa: F401
    from vnext_amd import train as T
    from vnext_amd import tuning
    from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg
    tuning.enable()
    out = {}
    for name, cfg, clips_args in (("seqformer", get_seqformer_cfg, (1, 5, 360, 640, 4)), ("idol", get_idol_cfg, (1, 2, 720, 1280, 8))):
        torch.manual_seed(0)
        model = build_model(cfg(**{"MODEL.DEVICE": "cuda:0"})).train()
        opt = T.build_optimizer(model, base_lr=1e-4)
        n, frames, h, w, objects = clips_args
        clips = T.synthetic_clips(n, frames, h, w, "cuda:0", seed=8, num_instances=objects)
        out[name] = {"clips": n, "frames": frames, "height": h, "width": w, "instances": objects}
        for label, autocast in (("fp32", False), ("bf16", True)):
            out[name]["train_step_" + label] = time_steps(model, opt, clips, autocast)
        del model, opt
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true", help="the fused op alone (for a rocprofv3 --kernel-trace run)")
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--steps", action="store_true", help="also train.train_step with the switch off / on (both models)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_set_loss.py: needs an MI355X (no CPU fallback for timings)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "shapes": []}
    for name, Ld, N, T, Q, K, sizes, idol in SHAPES:
        case = make_case(Ld, N, T, Q, K, sizes, idol, dev)
        w = torch.rand(Ld, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) + 0.5
        paths = {}
        if not a.fused_only:
            paths["aten"] = lambda: step(aten_sums, case, idol, w)       # ATen first: the fused figure follows the ATen one it is compared with
        paths["fused"] = lambda: step(fused_sums, case, idol, w)
        for _ in range(a.warmup):
            for call in paths.values():
                call()
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        for _ in range(a.rounds):                       # alternating: one call of each per round
            for k, call in paths.items():
                times[k].append(timed(call))
        entry = {"name": name, "Ld": Ld, "N": N, "T": T, "Q": Q, "K": K, "pairs": int(case[2].numel()),
                 "logits": Ld * N * Q * K}
        for k in paths:
            entry[k + "_fwd_bwd"] = stats(times[k])
        if not a.fused_only:
            ra, rf = paths["aten"](), paths["fused"]()
            entry["max_abs_difference"] = {"sums": float((ra[0] - rf[0]).abs().max()), "grad_logits": float((ra[1] - rf[1]).abs().max()),
                                           "grad_boxes": float((ra[2] - rf[2]).abs().max())}
            entry["speedup_median"] = statistics.median(times["aten"]) / statistics.median(times["fused"])
            entry["rounds_fused_below_aten"] = sum(1 for x, y in zip(times["aten"], times["fused"]) if y < x)
        if not a.no_launch_count and not a.fused_only:
            try:
                entry["launches_fwd_bwd"] = {k: launches(call) for k, call in paths.items()}
            except Exception as e:                      # a profiler that does not start costs the count, not the timings
                entry["launches_fwd_bwd"] = "not measured: %s" % e
        res["shapes"].append(entry)
    if a.steps:
        res["steps"] = steps_section()
    res["timing"] = ("device events around one forward + backward call (upstream weights applied, .backward() included), "
                     "profiler off, paths alternating per round, ATen first")
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
