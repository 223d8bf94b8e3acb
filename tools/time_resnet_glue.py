"""Time the fused element-wise glue of the ResNet trunk against the eager chain -> profiles/resnet_glue.json.

    python tools/time_resnet_glue.py [--out profiles/resnet_glue.json] [--rounds 7] [--quick]

Needs an MI355X (no fallback: without a GPU it exits with an error).  Three parts, all in one process so that the switch-off
and switch-on legs alternate round by round and see the same machine:

  sites    every site of the res2 .. res5 stages at the activations of 10 x 360 x 640 and 5 x 720 x 1280 inputs -- the shift +
           ReLU after conv1 / conv2, a block's tail with an identity and with a projection shortcut -- and the stem's shift +
           ReLU + max-pool; NCHW and NHWC, fp32 and bf16; the ops of vnext_amd/ops/resnet_glue.py against the eager
           expressions on the same tensors.
  trunks   the trunk forward (eval, NCHW) and forward + backward (training, channels-last after
           `vnext_amd.train.enable_channels_last()`), ResNet-50 and ResNet-101, fp32 and bf16 autocast, the switch off
           (= the parent commit's behaviour) and on.
  launches the kernels of one eval forward by torch's profiler, by family: with the switch on the trunk must launch exactly
           3 epilogues per block and one stem pass and no ATen element-wise or pooling kernel (asserted); the switch-off count
           is reported beside the 119 / 238 that one launch per bias, ReLU, add and pool would give.

Times are HIP events around `iters` back-to-back calls after a warm-up of every shape; per leg the median of the rounds and
their spread (min .. max).  The bar each leg is reported against: the switch-on median is not above the switch-off median by
more than the spread of the rounds.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vnext_amd import train as T  # noqa: E402
from vnext_amd.models.resnet import BLOCKS_PER_STAGE, ResNetTrunk  # noqa: E402
from vnext_amd.ops import resnet_glue as G  # noqa: E402

DEV = "cuda:0"
INPUTS = {"10x360x640": (10, 360, 640), "5x720x1280": (5, 720, 1280)}
STAGES = (("res2", 64, 256, 4), ("res3", 128, 512, 8), ("res4", 256, 1024, 16), ("res5", 512, 2048, 32))


def ceil_div(a, b):
    return -(-a // b)


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def alternate(legs, rounds, iters):
    """{name: fn} -> {name: {"median_ms", "min_ms", "max_ms"}}, the legs taking turns within every round"""
    for fn in legs.values():      # warm-up: code objects, algorithm choices, the allocator
        fn()
        fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            samples[k].append(timed(fn, iters))
    return {k: {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}
            for k, v in samples.items()}


def verdict(res, off="off", on="on"):
    spread = max(res[off]["max_ms"] - res[off]["min_ms"], res[on]["max_ms"] - res[on]["min_ms"])
    res["spread_ms"] = round(spread, 5)
    res["on_over_off"] = round(res[on]["median_ms"] / res[off]["median_ms"], 4)
    res["meets_bar"] = bool(res[on]["median_ms"] <= res[off]["median_ms"] + spread)
    return res


def site_legs(kind, shape, dtype, fmt):
    """the eager expression and the fused op of one site on the same tensors -> {"off": fn, "on": fn}, bytes moved by the op"""
    n, c, h, w = shape
    g = torch.Generator(device=DEV).manual_seed(1)
    new = lambda: torch.randn(shape, device=DEV, generator=g).to(dtype).contiguous(memory_format=fmt)      # noqa: E731
    y, b = new(), torch.randn(c, device=DEV, generator=g).to(dtype)
    bv = b.reshape(1, -1, 1, 1)
    size = y.numel() * y.element_size()
    if kind == "relu":
        return {"off": lambda: F.relu(y + bv), "on": lambda: G.conv_epilogue(y, b)}, 2 * size
    if kind == "tail_identity":
        r = new()
        return {"off": lambda: F.relu((y + bv) + r), "on": lambda: G.conv_epilogue(y, b, r)}, 3 * size
    if kind == "tail_projection":
        r, rb = new(), torch.randn(c, device=DEV, generator=g).to(dtype)
        rbv = rb.reshape(1, -1, 1, 1)
        return {"off": lambda: F.relu((y + bv) + (r + rbv)), "on": lambda: G.conv_epilogue(y, b, r, rb)}, 3 * size
    if kind == "stem_pool":
        out = n * c * ceil_div(h, 2) * ceil_div(w, 2) * y.element_size()
        return {"off": lambda: F.max_pool2d(F.relu(y + bv), 3, 2, 1), "on": lambda: G.stem_pool(y, b)}, size + out
    raise KeyError(kind)


def time_sites(rounds, quick):
    out = []
    with torch.no_grad():
        for tag, (n, H, W) in INPUTS.items():
            sites = [("stem_pool", (n, 64, ceil_div(H, 2), ceil_div(W, 2)))]
            for stage, mid, cout, stride in STAGES:
                h, w = ceil_div(H, stride), ceil_div(W, stride)
                sites += [(f"{stage}.relu", (n, mid, h, w)), (f"{stage}.tail_identity", (n, cout, h, w)),
                          (f"{stage}.tail_projection", (n, cout, h, w))]
            for name, shape in sites:
                for dtype in (torch.float32, torch.bfloat16):
                    for fmt, layout in ((torch.contiguous_format, "nchw"), (torch.channels_last, "nhwc")):
                        legs, nbytes = site_legs(name.split(".")[-1], shape, dtype, fmt)
                        res = verdict(alternate(legs, rounds, 5 if quick else 20))
                        res.update(input=tag, site=name, shape=list(shape), dtype=str(dtype).split(".")[-1], layout=layout,
                                   fused_bytes=nbytes,
                                   fused_gb_per_s=round(nbytes / (res["on"]["median_ms"] * 1e-3) / 1e9, 1))
                        out.append(res)
                        torch.cuda.empty_cache()
    return out


def make_trunk(depth):
    torch.manual_seed(depth)
    trunk = ResNetTrunk(depth).freeze(2).to(DEV)
    g = torch.Generator().manual_seed(depth)
    for m in trunk.modules():      # non-trivial frozen statistics: shifts that are not zero
        if hasattr(m, "running_var"):
            m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
            m.running_mean.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
            m.running_var.copy_(0.5 + torch.rand(m.bias.shape, generator=g))
    return trunk


def trunk_leg(trunk, x, training, autocast, on):
    def step():
        trunk.fused_glue = on
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            if not training:
                with torch.no_grad():
                    return trunk(x)
            outs = trunk(x)
        sum(o.float().mean() for o in outs).backward()
        trunk.zero_grad(set_to_none=True)
    return step


def time_trunks(rounds, quick):
    out = []
    for depth in (50, 101):
        trunk = make_trunk(depth)
        for tag, (n, H, W) in INPUTS.items():
            x = torch.randn(n, 3, H, W, device=DEV)
            for training in (False, True):
                trunk.train(training)
                for autocast in (False, True):
                    legs = {"off": trunk_leg(trunk, x, training, autocast, False),
                            "on": trunk_leg(trunk, x, training, autocast, True)}
                    res = verdict(alternate(legs, rounds, 2 if quick else 5))
                    res.update(depth=depth, input=tag, leg="forward+backward, training, channels-last" if training
                               else "forward, eval, NCHW", precision="bf16 autocast" if autocast else "fp32")
                    out.append(res)
                    print(json.dumps(res), flush=True)
        trunk.fused_glue = False
        del trunk
        torch.cuda.empty_cache()
    return out


FAMILIES = (("fused_glue", ("conv_epilogue_fwd_kernel", "stem_pool_fwd_kernel")),
            ("aten_elementwise", ("elementwise_kernel",)), ("aten_pool", ("max_pool",)),
            ("miopen_tensor_op", ("OpTensor", "Op1dTensor", "Op2dTensor", "Op3dTensor", "Op4dTensor", "Op5dTensor")))


def count_launches(trunk, x, on):
    from torch.profiler import ProfilerActivity, profile
    trunk.eval()
    trunk.fused_glue = on
    with torch.no_grad():
        trunk(x)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            trunk(x)
            torch.cuda.synchronize()
    names = {}
    for ev in prof.events():
        if getattr(ev, "device_type", None) is not None and "cuda" in str(ev.device_type).lower():
            names[ev.name] = names.get(ev.name, 0) + 1
    counts = {fam: 0 for fam, _ in FAMILIES}
    counts["other"] = 0
    for name, k in names.items():
        for fam, keys in FAMILIES:
            if any(key in name for key in keys):
                counts[fam] += k
                break
        else:
            counts["other"] += k
    counts["element_wise_total"] = counts["fused_glue"] + counts["aten_elementwise"] + counts["aten_pool"] + counts["miopen_tensor_op"]
    counts["kernels"] = sum(names.values())
    counts["names"] = {k[:120]: v for k, v in sorted(names.items(), key=lambda kv: -kv[1])[:12]}
    return counts


def launches():
    out = []
    x = torch.randn(2, 3, 256, 320, device=DEV)
    for depth in (50, 101):
        trunk = make_trunk(depth)
        blocks = sum(BLOCKS_PER_STAGE[depth])
        off, on = count_launches(trunk, x, False), count_launches(trunk, x, True)
        trunk.fused_glue = False
        expected_off = 7 * blocks + 4 + 3      # per block 3 shifts + 3 ReLUs + 1 add; 4 projections' shifts; the stem's 3
        expected_on = 3 * blocks + 1
        if off["kernels"]:      # (a profiler that sees no kernels gives nothing to hold the counts to)
            assert on["fused_glue"] == expected_on and on["aten_elementwise"] == 0 and on["aten_pool"] == 0 and \
                on["miopen_tensor_op"] == 0, (depth, on)
            assert off["fused_glue"] == 0, (depth, off)
        out.append({"depth": depth, "off": off, "on": on, "expected_off": expected_off, "expected_on": expected_on,
                    "off_matches_expected": off["element_wise_total"] == expected_off})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_glue.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="fewer iterations per round")
    ap.add_argument("--parts", default="launches,sites,trunks")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_resnet_glue: needs a GPU (nothing is timed or estimated without one)")
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": args.rounds,
              "channels_last": T.enable_channels_last(),
              "bar": "on.median_ms <= off.median_ms + spread_ms (the larger min..max of the two legs' rounds)"}
    for part, fn in (("sites", lambda: time_sites(args.rounds, args.quick)),
                     ("trunks", lambda: time_trunks(args.rounds, args.quick)), ("launches", launches)):
        if part in args.parts.split(","):
            result[part] = fn()
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:      # after every part: a later part that dies leaves the earlier ones
                json.dump(result, f, indent=1)
                f.write("\n")
    misses = [r for part in ("sites", "trunks") for r in result.get(part, []) if not r["meets_bar"]]
    print(f"{args.out}: {len(result.get('sites', []))} sites, {len(result.get('trunks', []))} trunk legs, "
          f"{len(misses)} miss the bar")


if __name__ == "__main__":
    main()
