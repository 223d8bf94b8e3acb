"""Where a SeqFormer training step spends its wall time (synchronising between phases, so the sum
exceeds the pipelined step).  python tools/step_breakdown.py [--graph] [--device-matching] [--fused-mask-loss]
[--fused-set-loss] [--idol [--fused-reid-loss]] [--fused-optimizer] [--clips N]

--device-matching: the same rows with SeqFormer's device-side matcher (train.enable_device_matching), so the "matching"
row and the step can be read side by side with the host matcher's.
--fused-mask-loss: the same rows with the criterion's mask losses from the fused kernel (train.enable_fused_mask_loss):
the "full forward" and "backward" rows carry the difference.
--fused-set-loss: likewise with the criterion's class and box losses from the fused op (train.enable_fused_set_loss).
--idol: the IDOL step instead (one 720 x 1280 pair, 8 objects: the bench's IDOL leg); its forward is one row, the trunk and
the matching are not timed apart.
--fused-reid-loss: with --idol, both reid losses from the fused op (train.enable_fused_reid_loss); SeqFormer has none.
--fused-optimizer: the clipped AdamW op (train.build_fused_optimizer) instead of clip_grad_norm_ + AdamW: the two tail rows
become one.
--clips N: SeqFormer clips per step (default 1; the bench's step has 2).
The last line is the kernel launches of one whole train_step (torch.profiler), in a pass of its own."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import vnext_amd.models  # noqa: F401,E402
from vnext_amd import train as T  # noqa: E402
from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--graph", action="store_true")
ap.add_argument("--device-matching", action="store_true")
ap.add_argument("--fused-mask-loss", action="store_true")
ap.add_argument("--fused-set-loss", action="store_true")
ap.add_argument("--fused-reid-loss", action="store_true")
ap.add_argument("--idol", action="store_true")
ap.add_argument("--fused-optimizer", action="store_true")
ap.add_argument("--clips", type=int, default=1)
ap.add_argument("--steps", type=int, default=8)
a = ap.parse_args()
dev = "cuda:0"
torch.manual_seed(0)
model = build_model((get_idol_cfg if a.idol else get_seqformer_cfg)(**{"MODEL.DEVICE": dev})).train()
model.graph_training = a.graph
if a.fused_reid_loss:
    T.enable_fused_reid_loss(model)       # raises for SeqFormer: it has no reid losses
if a.device_matching:
    T.enable_device_matching(model)
if a.fused_mask_loss:
    T.enable_fused_mask_loss(model)
if a.fused_set_loss:
    T.enable_fused_set_loss(model)
opt = T.build_fused_optimizer(model) if a.fused_optimizer else T.build_optimizer(model)
clips = T.synthetic_clips(1, 2, 720, 1280, dev, seed=8, num_instances=8) if a.idol else \
    T.synthetic_clips(a.clips, 5, 360, 640, dev, seed=100, num_instances=4)
for _ in range(3):
    T.train_step(model, opt, clips)

marks = {}


def tick(name, t0):
    torch.cuda.synchronize()
    t = time.perf_counter()
    marks[name] = marks.get(name, 0.0) + (t - t0) * 1e3
    return t


for _ in range(a.steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    targets = model.prepare_targets(clips)
    t = tick("prepare_targets", t)
    frames = [f for c in clips for f in c["image"]]
    if a.idol:
        pass
    elif a.graph:
        hs, logits, boxes, ref0, ref_rest, feats = model._graphed_train_trunk(torch.stack(frames))
    else:
        x, srcs, hs, memory, logits, boxes, refs = model._run(clips, want_refs=True)
        feats = model._mask_features(srcs, memory)
    if not a.idol:
        t = tick("trunk forward", t)
    if a.idol:
        pass
    elif a.device_matching:
        ind = model.criterion.matcher.match_all_layers_device(logits, boxes, targets)
        t = tick("matching (one kernel: cost + LSAP on the device)", t)
    else:
        ind = model.criterion.matcher.match_all_layers(logits, boxes, targets)
        t = tick("matching (cost + host LSAP)", t)
    losses = model(clips)
    t = tick("full forward (all of the above again + mask head + criterion)", t)
    total = sum(losses.values())
    opt.zero_grad(set_to_none=True)
    total.backward()
    t = tick("backward", t)
    if a.fused_optimizer:
        opt.step()
        t = tick("clip_grad_norm + AdamW step (one op)", t)
        continue
    params = [p for g in opt.param_groups for p in g["params"]]
    torch.nn.utils.clip_grad_norm_(params, 0.01)
    t = tick("clip_grad_norm", t)
    opt.step()
    t = tick("AdamW step", t)
for k, v in marks.items():
    print(f"{k:70s} {v / a.steps:8.2f} ms")

from torch.profiler import ProfilerActivity, profile  # noqa: E402
torch.cuda.synchronize()
with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
    T.train_step(model, opt, clips)
    torch.cuda.synchronize()
names = [e.name.lower() for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
kernels = [n for n in names if not n.startswith(("memcpy", "memset", "optimizer.step#"))]
print(f"{'kernel launches of one train_step':70s} {len(kernels):8d}    (+ {len(names) - len(kernels)} copies / memsets / annotations)")
