"""Time the fused shifted-window attention (vnext_amd/ops/window_attention.py) against the reference ATen expression
(the same block with the kernel switched off, as VNX_FUSED_WINDOW_ATTN=0 does) at Swin-L's four stage shapes of SURVEY
section 8(d) config C4 (5 frames of 736 x 1280, window 12, SW-MSA blocks), forward and forward + backward, as the median of
HIP-event regions; then the SeqFormer Swin-L training step (fp32, one clip) with the switch on and off.  One JSON line.

    python tools/time_window_attention.py [--reps 20] [--no-model]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--model-reps", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    result = {"tool": "time_window_attention", "frames": FRAMES, "window": WINDOW, "shift": WINDOW // 2,
              "stages": [time_stage(*s, args.reps) for s in STAGES]}
    if not args.no_model:
        result.update(time_model(args.model_reps))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
