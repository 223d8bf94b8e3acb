"""Time the fused Swin glue (vnext_amd/ops/swin_glue.py) against the eager ATen chain it replaces, at Swin-L's four stage
shapes of SURVEY section 8(d) config C4 (5 frames of 736 x 1280, window 12): the residual site
`y = x + drop_path(a); n = norm(y)` (+ the cast the next Linear makes under autocast) and the PatchMerging site
(pad, 2x2 gather, norm), forward and forward + backward, under torch.autocast(bfloat16) and in fp32 -- medians of
HIP-event regions, the two variants ALTERNATING in one process.  Per site: the algorithmic bytes from the shapes (one
read of every input, one write of every output), the achieved bytes/s of the fused op and its share of the 6.3 TB/s
measured-copy rate; the launch counts of both variants (torch.profiler); the kernels' own times from a
`rocprofv3 --kernel-trace --stats` run of its own (a child process); and the SeqFormer Swin-L bf16 training step with
enable_bf16_window_attention on and enable_fused_swin_glue off / on, alternating, with the spread of the rounds.
One JSON line (profiles/swin_glue.json).

    python tools/time_swin_glue.py [--reps 20] [--model-reps 7] [--no-model] [--no-trace]
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from vnext_amd.models.swin import drop_path  # noqa: E402
from vnext_amd.ops import swin_glue as G  # noqa: E402

DEV = "cuda:0"
STAGES = [(184, 320, 192), (92, 160, 384), (46, 80, 768), (23, 40, 1536)]     # H, W, C at C4
FRAMES, RATE, COPY_RATE = 5, 0.2, 6.3e12
SWIN_L = {"MODEL.BACKBONE.NAME": "D2SwinTransformer", "MODEL.SWIN.EMBED_DIM": 192, "MODEL.SWIN.DEPTHS": [2, 2, 18, 2],
          "MODEL.SWIN.NUM_HEADS": [6, 12, 24, 48], "MODEL.SWIN.WINDOW_SIZE": 12, "MODEL.SWIN.DROP_PATH_RATE": 0.3,
          "MODEL.SWIN.PRETRAIN_IMG_SIZE": 384}
BF16, F32 = torch.bfloat16, torch.float32


def alternating(fns, reps, warmup=3):
    """HIP-event regions of several callables, taken in turn inside one loop -> {name: [ms, ..]}"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return ms


def launches(fn):
    """device kernels of one call"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and not e.name.startswith(("Memcpy", "Memset")))


def stream_types(mode, stage):
    """(x, a, n) types of the eager chain: fp32; under bf16 autocast an fp32 stream in stage 1, a bf16 stream after"""
    if mode == "fp32":
        return F32, F32, F32
    return (F32 if stage == 0 else BF16), BF16, BF16


def residual_site(stage, mode):
    H, W, C = STAGES[stage]
    tx, ta, tn = stream_types(mode, stage)
    torch.manual_seed(stage)
    x = torch.randn(FRAMES, H * W, C, device=DEV).to(tx).requires_grad_(True)
    a = torch.randn(FRAMES, H * W, C, device=DEV).to(ta).requires_grad_(True)
    gy, gn = torch.randn_like(x).detach(), torch.randn(FRAMES, H * W, C, device=DEV).to(tn)
    norm = torch.nn.LayerNorm(C).to(DEV)
    amp = mode == "bf16"

    def fused():
        with torch.autocast("cuda", dtype=BF16, enabled=amp):
            return G.residual_norm(x, a, G.drop_scale(a, RATE, True), norm)

    def eager():
        with torch.autocast("cuda", dtype=BF16, enabled=amp):
            y = x + drop_path(a, RATE, True)
            n = norm(y)
            return y, (n.to(BF16) if amp else n)             # the cast the next Linear makes

    def fwd(f):
        def g():
            with torch.no_grad():
                f()
        return g

    def fwd_bwd(f):
        def g():
            y, n = f()
            torch.autograd.backward([y, n], [gy, gn])
        return g
    with torch.autocast("cuda", dtype=BF16, enabled=amp):
        assert G.fused_applies(x, a, norm)
    el = x.numel()
    sx, sa, sn = x.element_size(), a.element_size(), gn.element_size()
    return dict(fused=fused, eager=eager, fwd=fwd, fwd_bwd=fwd_bwd, shape=[FRAMES * H * W, C],
                fwd_bytes=el * (2 * sx + sa + sn), bwd_bytes=el * (3 * sx + sn + sx + sa))


def merge_site(stage, mode):
    H, W, C = STAGES[stage]
    tx, _, tn = stream_types(mode, stage)
    torch.manual_seed(10 + stage)
    x = torch.randn(FRAMES, H * W, C, device=DEV).to(tx).requires_grad_(True)
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    gn = torch.randn(FRAMES, H2 * W2, 4 * C, device=DEV).to(tn)
    norm = torch.nn.LayerNorm(4 * C).to(DEV)
    amp = mode == "bf16"

    def fused():
        with torch.autocast("cuda", dtype=BF16, enabled=amp):
            return (G.merge_norm(x, H, W, norm),)

    def eager():
        with torch.autocast("cuda", dtype=BF16, enabled=amp):
            n = G.merge_norm_reference(x, H, W, norm)
            return ((n.to(BF16) if amp else n),)

    def fwd(f):
        def g():
            with torch.no_grad():
                f()
        return g

    def fwd_bwd(f):
        def g():
            f()[0].backward(gn)
        return g
    with torch.autocast("cuda", dtype=BF16, enabled=amp):
        assert G.merge_applies(x, norm)
    out_el = gn.numel()
    sx, sn = x.element_size(), gn.element_size()
    return dict(fused=fused, eager=eager, fwd=fwd, fwd_bwd=fwd_bwd, shape=[FRAMES * H2 * W2, 4 * C],
                fwd_bytes=x.numel() * sx + out_el * sn, bwd_bytes=2 * x.numel() * sx + out_el * sn)


def time_site(site, reps):
    row = {"rows_channels": site["shape"], "fwd_bytes": site["fwd_bytes"], "fwd_bwd_bytes": site["fwd_bytes"] + site["bwd_bytes"]}
    for leg, wrap, nbytes in (("fwd", site["fwd"], site["fwd_bytes"]),
                              ("fwd_bwd", site["fwd_bwd"], site["fwd_bytes"] + site["bwd_bytes"])):
        ms = alternating({"fused": wrap(site["fused"]), "eager": wrap(site["eager"])}, reps)
        for k, v in ms.items():
            row[f"{k}_{leg}_ms"] = round(statistics.median(v), 4)
            row[f"{k}_{leg}_launches"] = launches(wrap(site[k]))
        rate = nbytes / (statistics.median(ms["fused"]) * 1e-3)
        row[f"fused_{leg}_tb_s"] = round(rate / 1e12, 3)
        row[f"fused_{leg}_share_of_copy_rate"] = round(rate / COPY_RATE, 3)
        row[f"fused_faster_{leg}"] = statistics.median(ms["fused"]) < statistics.median(ms["eager"])
    torch.cuda.empty_cache()
    return row


def trace_child(reps):
    """run under rocprofv3: every residual and merge site, bf16 and fp32, fused forward + backward `reps` times"""
    for mode in ("bf16", "fp32"):
        for stage in range(len(STAGES)):
            sites = [residual_site(stage, mode)] + ([merge_site(stage, mode)] if stage < 3 else [])
            for site in sites:
                f = site["fwd_bwd"](site["fused"])
                for _ in range(reps + 2):
                    f()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()


def kernel_times(reps):
    """median duration in us of every swin_glue kernel instantiation, from a kernel trace of a child process"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = tempfile.mkdtemp(prefix="sg_trace_", dir=os.environ.get("VNX_TRACE_DIR"))
    try:
        subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
                        os.path.abspath(__file__), "--trace-child", "--reps", str(reps)],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=420)
        dur = {}
        for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for rec in csv.DictReader(f):
                    name = rec["Kernel_Name"]
                    if "swin_glue" in name:
                        key = name.split("(")[0].replace("void ", "").replace("vnx::(anonymous namespace)::", "")
                        key += " grid=" + rec.get("Grid_Size_X", rec.get("Grid_Size", "?"))
                        dur.setdefault(key, []).append((int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])) / 1e3)
        if not dur:
            raise RuntimeError("no swin_glue kernel in the trace under " + out)
        return {k: round(statistics.median(v[2:] or v), 2) for k, v in sorted(dur.items())}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def time_model(reps):
    from vnext_amd import train as T
    from vnext_amd.registry import build_model, get_seqformer_cfg
    torch.manual_seed(0)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": DEV, **SWIN_L})).train()
    T.enable_bf16_window_attention(model)
    opt = T.build_optimizer(model)
    clips = T.synthetic_clips(1, FRAMES, 720, 1280, DEV, seed=1)

    def step(on):
        def f():
            T.enable_fused_swin_glue(model, on)
            with torch.autocast("cuda", dtype=BF16):
                loss_dict = model(clips)
            opt.zero_grad(set_to_none=True)
            sum(loss_dict.values()).backward()
            opt.step()
        return f
    ms = alternating({"off": step(False), "on": step(True)}, reps, warmup=2)
    out = {}
    for k, v in ms.items():
        out[f"seqformer_swinl_bf16_step_glue_{k}_ms"] = round(statistics.median(v), 2)
        out[f"seqformer_swinl_bf16_step_glue_{k}_rounds_ms"] = [round(t, 2) for t in v]
    T.enable_fused_swin_glue(model, False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--model-reps", type=int, default=7)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.trace_child:
        return trace_child(args.reps)
    result = {"tool": "time_swin_glue", "frames": FRAMES, "drop_path_rate": RATE, "copy_rate_tb_s": COPY_RATE / 1e12,
              "residual": {}, "merge": {}}
    for mode in ("bf16", "fp32"):
        result["residual"][mode] = [time_site(residual_site(i, mode), args.reps) for i in range(len(STAGES))]
        result["merge"][mode] = [time_site(merge_site(i, mode), args.reps) for i in range(3)]
    if not args.no_trace:
        torch.cuda.empty_cache()
        result["kernel_us"] = kernel_times(min(args.reps, 10))
    if not args.no_model:
        result.update(time_model(args.model_reps))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
