"""Time the fused shifted-window attention (vnext_amd/ops/window_attention.py) against the reference ATen expression
(the same block with the kernel switched off, as VNX_FUSED_WINDOW_ATTN=0 does) at Swin-L's four stage shapes of SURVEY
section 8(d) config C4 (5 frames of 736 x 1280, window 12, SW-MSA blocks), forward and forward + backward, as the median of
HIP-event regions; then the SeqFormer Swin-L training step (fp32, one clip) with the switch on and off.  One JSON line.

    python tools/time_window_attention.py [--reps 20] [--no-model]

`--bf16`: the same four shapes under torch.autocast(bfloat16), three ways ALTERNATING in one process -- (a) the fp32 core
(the switch off: custom_fwd casts the bf16 qkv rows up), (b) the bf16 matrix-core core (WindowAttention.bf16_core), (c) the
ATen expression -- block forward and forward + backward; the core kernels' own times from `rocprofv3 --kernel-trace --stats`
runs of their own (one child process per stage, the median over its dispatches of each kernel name); and the SeqFormer
Swin-L bf16 training step with the switch off and on, alternating.  One JSON line (profiles/window_attention_bf16.json).

    python tools/time_window_attention.py --bf16 [--reps 20] [--no-model] [--no-trace]
"""
from __future__ import annotations

import argparse
import json
import os
import csv
import glob
import shutil
import statistics
import subprocess
import sys
import tempfile

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from vnext_amd.models.swin import WindowAttention  # noqa: E402
from vnext_amd.ops import window_attention as WA  # noqa: E402

DEV = "cuda:0"
STAGES = [(184, 320, 192, 6), (92, 160, 384, 12), (46, 80, 768, 24), (23, 40, 1536, 48)]     # H, W, C, heads at C4
FRAMES, WINDOW = 5, 12
SWIN_L = {"MODEL.BACKBONE.NAME": "D2SwinTransformer", "MODEL.SWIN.EMBED_DIM": 192, "MODEL.SWIN.DEPTHS": [2, 2, 18, 2],
          "MODEL.SWIN.NUM_HEADS": [6, 12, 24, 48], "MODEL.SWIN.WINDOW_SIZE": 12, "MODEL.SWIN.DROP_PATH_RATE": 0.3,
          "MODEL.SWIN.PRETRAIN_IMG_SIZE": 384}


def events(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def time_stage(H, W, C, heads, reps):
    torch.manual_seed(0)
    attn = WindowAttention(C, WINDOW, heads).to(DEV)
    x = torch.randn(FRAMES, H * W, C, device=DEV, requires_grad=True)
    go = torch.randn(FRAMES, H * W, C, device=DEV)
    row = {"grid": [H, W], "C": C, "heads": heads}
    for name, on in (("fused", True), ("aten", False)):
        WA.ENABLE = on
        fwd = events(lambda: WA.window_attention_block(x.detach(), H, W, attn, WINDOW, WINDOW // 2), reps)

        def step():
            y = WA.window_attention_block(x, H, W, attn, WINDOW, WINDOW // 2)
            y.backward(go)
        fb = events(step, reps)
        row[f"{name}_fwd_ms"], row[f"{name}_fwd_bwd_ms"] = round(fwd, 4), round(fb, 4)
        torch.cuda.empty_cache()
    WA.ENABLE = True
    # the core alone (no qkv / proj GEMMs): what the roofline figures of DESIGN section 10 are about
    qkv = torch.randn(FRAMES * H * W, 3 * C, device=DEV, requires_grad=True)
    bias, table = attn.qkv.bias.detach().clone().requires_grad_(True), attn.relative_position_bias_table
    gc = torch.randn(FRAMES * H * W, C, device=DEV)
    core = lambda: WA._WindowAttention.apply(qkv, bias, table, FRAMES, H, W, heads, WINDOW, WINDOW // 2, attn.scale)  # noqa
    row["kernel_fwd_ms"] = round(events(lambda: core(), reps), 4)
    row["kernel_fwd_bwd_ms"] = round(events(lambda: core().backward(gc), reps), 4)
    Hp, Wp = -(-H // WINDOW) * WINDOW, -(-W // WINDOW) * WINDOW
    flop = 2 * 2 * FRAMES * Hp * Wp * WINDOW * WINDOW * C            # q k^T and p v over the padded grid
    row["core_fwd_gflop"] = round(flop / 1e9, 2)
    row["kernel_fwd_tflops"] = round(flop / (row["kernel_fwd_ms"] * 1e-3) / 1e12, 2)
    return row


def time_model(reps):
    from vnext_amd import train as T
    from vnext_amd.registry import build_model, get_seqformer_cfg
    torch.manual_seed(0)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": DEV, **SWIN_L})).train()
    opt = T.build_optimizer(model)
    clips = T.synthetic_clips(1, FRAMES, 720, 1280, DEV, seed=1)
    out = {}
    for name, on in (("fused", True), ("aten", False)):
        WA.ENABLE = on
        out[f"seqformer_swinl_step_{name}_ms"] = round(events(lambda: T.train_step(model, opt, clips), reps, warmup=2), 2)
    WA.ENABLE = True
    return out


def alternating(fns, reps, warmup=3):
    """medians of HIP-event regions of several callables, taken in turn inside one loop"""
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
    return {k: statistics.median(v) for k, v in ms.items()}


def _bf16_stage_setup(H, W, C, heads):
    torch.manual_seed(0)
    attn = WindowAttention(C, WINDOW, heads).to(DEV)
    x = torch.randn(FRAMES, H * W, C, device=DEV, requires_grad=True)
    go = torch.randn(FRAMES, H * W, C, device=DEV)
    return attn, x, go


def _block_variant(attn, name):
    WA.ENABLE = name != "aten"
    attn.bf16_core = name == "bf16"


def time_stage_bf16(H, W, C, heads, reps):
    attn, x, go = _bf16_stage_setup(H, W, C, heads)
    row = {"grid": [H, W], "C": C, "heads": heads}

    def fwd(name):
        def f():
            _block_variant(attn, name)
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                WA.window_attention_block(x, H, W, attn, WINDOW, WINDOW // 2)
        return f

    def fwd_bwd(name):
        def f():
            _block_variant(attn, name)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = WA.window_attention_block(x, H, W, attn, WINDOW, WINDOW // 2)
            y.backward(go.to(y.dtype))
        return f
    names = ("fp32core", "bf16", "aten")
    for k, v in alternating({n: fwd(n) for n in names}, reps).items():
        row[f"{k}_fwd_ms"] = round(v, 4)
    for k, v in alternating({n: fwd_bwd(n) for n in names}, reps).items():
        row[f"{k}_fwd_bwd_ms"] = round(v, 4)
    WA.ENABLE = True
    Hp, Wp = -(-H // WINDOW) * WINDOW, -(-W // WINDOW) * WINDOW
    pairs = FRAMES * Hp * Wp * WINDOW * WINDOW * heads                # (query, key) pairs of the padded grid, all heads
    row["pairs_m"] = round(pairs / 1e6, 2)
    row["fwd_gflop"] = round(2 * 2 * pairs * WA.HEAD_DIM / 1e9, 2)         # 2 products forward, 5 backward
    row["bwd_gflop"] = round(5 * 2 * pairs * WA.HEAD_DIM / 1e9, 2)
    torch.cuda.empty_cache()
    return row


def trace_child(stage, reps):
    """run under rocprofv3: the two cores alone, forward + backward, `reps` times each at one stage"""
    H, W, C, heads = STAGES[stage]
    attn, _, _ = _bf16_stage_setup(H, W, C, heads)
    bias, table = attn.qkv.bias.detach().clone().requires_grad_(True), attn.relative_position_bias_table
    for fn, dt in ((WA._WindowAttention, torch.float32), (WA._WindowAttentionBF16, torch.bfloat16)):
        qkv = torch.randn(FRAMES * H * W, 3 * C, device=DEV, dtype=dt, requires_grad=True)
        gc = torch.randn(FRAMES * H * W, C, device=DEV, dtype=dt)
        for _ in range(reps + 2):
            fn.apply(qkv, bias, table, FRAMES, H, W, heads, WINDOW, WINDOW // 2, attn.scale).backward(gc)
    torch.cuda.synchronize()


def kernel_times(stage, reps):
    """median duration in us of every window_attn kernel at one stage, from a kernel trace of a child process"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = tempfile.mkdtemp(prefix="wa_trace_", dir=os.environ.get("VNX_TRACE_DIR"))
    try:
        subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
                        os.path.abspath(__file__), "--trace-child", str(stage), "--reps", str(reps)],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=300)
        dur = {}
        for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for rec in csv.DictReader(f):
                    name = rec["Kernel_Name"]
                    if "window_attn" in name:
                        key = name.split("(")[0].split("::")[-1].replace("void ", "")
                        dur.setdefault(key, []).append((int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])) / 1e3)
        if not dur:
            raise RuntimeError("no window_attn kernel in the trace under " + out)
        return {k: round(statistics.median(v[2:] or v), 2) for k, v in dur.items()}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def time_model_bf16(reps):
    from vnext_amd import train as T
    from vnext_amd.registry import build_model, get_seqformer_cfg
    torch.manual_seed(0)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": DEV, **SWIN_L})).train()
    opt = T.build_optimizer(model)
    clips = T.synthetic_clips(1, FRAMES, 720, 1280, DEV, seed=1)

    def step(on):
        def f():
            T.enable_bf16_window_attention(model, on)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss_dict = model(clips)
            opt.zero_grad(set_to_none=True)
            sum(loss_dict.values()).backward()
            opt.step()
        return f
    ms = alternating({"off": step(False), "on": step(True)}, reps, warmup=2)
    return {"seqformer_swinl_bf16_step_core_fp32_ms": round(ms["off"], 2),
            "seqformer_swinl_bf16_step_core_bf16_ms": round(ms["on"], 2)}


def main_bf16(args):
    result = {"tool": "time_window_attention --bf16", "frames": FRAMES, "window": WINDOW, "shift": WINDOW // 2,
              "stages": [time_stage_bf16(*s, args.reps) for s in STAGES]}
    if not args.no_trace:
        torch.cuda.empty_cache()
        for i, row in enumerate(result["stages"]):
            row["kernel_us"] = kernel_times(i, args.reps)
    if not args.no_model:
        result.update(time_model_bf16(args.model_reps))
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--model-reps", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.trace_child is not None:
        return trace_child(args.trace_child, args.reps)
    if args.bf16:
        return main_bf16(args)
    result = {"tool": "time_window_attention", "frames": FRAMES, "window": WINDOW, "shift": WINDOW // 2,
              "stages": [time_stage(*s, args.reps) for s in STAGES]}
    if not args.no_model:
        result.update(time_model(args.model_reps))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
