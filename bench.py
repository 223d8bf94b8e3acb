"""bench.py -- headline measurement of the MI355X hot path.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Metric (BASELINE.json): MSDeformAttn fwd+bwd Gpoints/s at T=5, L=4, Q=300, H=8, K=4.
One step = one forward + one backward of the op over one T=5 360p clip folded
into the batch (B=5, Lq=300, S=5100, M=8, D=32, L=4, K=4; fp32; sampling
locations uniform in [0,1)^2, the reference's test convention, ops/test.py:34).
A point is one (b, q, head, level, k) bilinear sample: 192 000 per step.

Timed region: inputs are resident in HBM and ROTATE through more than 256 MiB of
distinct input sets, so neither the 256 MiB Infinity Cache nor the L2s hold a
step's inputs from the previous use ("cold" numbers).  The K steps are launched
as hipGraph replays (a step is three stream operations of a few microseconds;
launching them from Python one by one would time the interpreter), bracketed by
barrier + synchronize; exactly K steps are timed, ms_per_step = region / K; rank 0
prints one JSON line.

--dump-outputs DIR: after the timed region rank 0 writes what the last timed step
returned (output, grad_value, grad_sampling_loc, grad_attn_weight) as float32
DIR/<name>.npy, ~30 MB; the input sets are seeded, so two builds run with the same
arguments can be compared output for output.

N > 1: clips shard across ranks with no data-path collective (the op has no
exchange step) -- weak scaling, value = all ranks' points / max
time.  The gradient all-reduce of the model-level step lives with the model path.

A plain run stops there.  --full (minutes) adds, after the headline:
  repeats       --repeats more timed regions of K steps: median / min / p10 / p90
  model_step    the SeqFormer-R50 training step under DDP (clips/s), other_configs
  roofline      forward kernel (the kernel the north star sets the 60 % target on),
                algorithmic bytes / avg launch time measured here with events
  roofline_bwd  the same for the backward kernel (+ its zero-fill)
  op_cases, roofline_*  the other op shapes and kernel families
  cpu_baseline  the oracle (oracle/, "port") timed on the host cores on the same
                workload, plus the grid_sample fallback technique of the reference
--no-cpu / --no-model / --no-cases / --no-spans / --no-warm drop single legs of --full.
"""
from __future__ import annotations

import argparse
import gc
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md); ~6300 measured copy ceiling

SHAPES = {
    "360p": [(48, 80), (24, 40), (12, 20), (6, 10)],     # S = 5100
    "720p": [(92, 160), (46, 80), (23, 40), (12, 20)],   # S = 19560
}


def algorithmic_bytes(B, S, Lq, e=4, e_loc=4, M=8, D=32, L=4, K=4):
    """fwd = value + loc + attn + out; bwd = value + grad_value +
    grad_out + loc + attn + grad_loc + grad_attn."""
    fwd = B * (e * S * M * D + e_loc * Lq * M * L * K * 3 + e * Lq * M * D)
    bwd = B * (2 * e * S * M * D + e * Lq * M * D + 2 * e_loc * Lq * M * L * K * 3)
    return fwd, bwd


_LEVELS = {}


def make_set(res, B, Lq, seed, device, dist="U"):
    g = torch.Generator(device=device).manual_seed(seed)
    # the level geometry (two 32-byte int64 tensors) is ONE pair shared by every input set, as in the
    # models, where all 12 layers' calls pass the same tensors; what rotates is the data
    if (res, str(device)) not in _LEVELS:
        sh = torch.tensor(SHAPES[res], dtype=torch.long, device=device)
        _LEVELS[(res, str(device))] = (sh, torch.cat((sh.new_zeros((1,)), sh.prod(1).cumsum(0)[:-1])))
    shapes, lsi = _LEVELS[(res, str(device))]
    S = int(shapes.prod(1).sum())
    value = torch.randn(B, S, 8, 32, device=device, generator=g)
    if dist == "U":
        loc = torch.rand(B, Lq, 8, 4, 4, 2, device=device, generator=g)
    else:
        # SURVEY.md section 8d, "M": a reference point per query (decoder: random box centres; encoder, Lq == S: the
        # pixel-centre grid of deformable_transformer.py:183-190) + (dir_m (k + 1) + N(0, 1)) / (W_l, H_l), the
        # initialisation bias of ops/modules/ms_deform_attn.py:65-73
        if Lq == S:
            cells = []
            for h, w in SHAPES[res]:
                ys, xs = torch.meshgrid(torch.arange(h, device=device) + 0.5, torch.arange(w, device=device) + 0.5, indexing="ij")
                cells.append(torch.stack([xs.reshape(-1) / w, ys.reshape(-1) / h], -1))
            ref = torch.cat(cells, 0).view(1, S, 1, 1, 1, 2).expand(B, S, 1, 1, 1, 2)
        else:
            ref = torch.rand(B, Lq, 1, 1, 1, 2, device=device, generator=g)
        th = torch.arange(8, device=device) * (2 * math.pi / 8)
        dirs = torch.stack([th.cos(), th.sin()], -1)
        dirs = (dirs / dirs.abs().max(-1, keepdim=True)[0]).view(1, 1, 8, 1, 1, 2)
        steps = torch.arange(1, 5, device=device, dtype=torch.float32).view(1, 1, 1, 1, 4, 1)
        wh = torch.stack([shapes[:, 1], shapes[:, 0]], -1).float().view(1, 1, 1, 4, 1, 2)
        loc = (ref + (dirs * steps + torch.randn(B, Lq, 8, 4, 4, 2, device=device, generator=g)) / wh).contiguous()
    attn = torch.softmax(torch.randn(B, Lq, 8, 16, device=device, generator=g), -1).view(B, Lq, 8, 4, 4)
    grad_out = torch.randn(B, Lq, 256, device=device, generator=g)
    out = torch.empty(B, Lq, 256, device=device)
    gv, gl, ga = torch.empty_like(value), torch.empty_like(loc), torch.empty_like(attn)
    from vnext_amd import _lib
    ws_bytes = _lib.lib().vnx_msda_backward_workspace_bytes(0, 0, B, S, 8, 32, 4, Lq, 4, 1)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=device)
    return dict(ws=ws, ws_bytes=ws_bytes, shapes=shapes, lsi=lsi, value=value, loc=loc, attn=attn.contiguous(),
                grad_out=grad_out, out=out, gv=gv, gl=gl, ga=ga, S=S)


class Op:
    """Direct C-ABI launches into preallocated buffers (no allocation in the timed region)."""

    def __init__(self, device):
        from vnext_amd import _lib
        self.lib = _lib.lib()
        self._lib = _lib
        self.device = device

    def fwd(self, s, B, Lq):
        st = self.lib.vnx_msda_forward(
            s.get("vdt", 0), 0, s["value"].data_ptr(), s["shapes"].data_ptr(), s["lsi"].data_ptr(),
            s["loc"].data_ptr(), s["attn"].data_ptr(), s["out"].data_ptr(),
            B, s["S"], 8, 32, 4, Lq, 4, torch.cuda.current_stream().cuda_stream)
        self._lib.check(st)

    def bwd(self, s, B, Lq):
        st = self.lib.vnx_msda_backward(
            s.get("vdt", 0), 0, s["value"].data_ptr(), s["shapes"].data_ptr(), s["lsi"].data_ptr(),
            s["loc"].data_ptr(), s["attn"].data_ptr(), s["grad_out"].data_ptr(),
            s["gv"].data_ptr(), s["gl"].data_ptr(), s["ga"].data_ptr(),
            B, s["S"], 8, 32, 4, Lq, 4, 1, s["ws"].data_ptr(), s["ws_bytes"],
            torch.cuda.current_stream().cuda_stream)
        self._lib.check(st)


def capture(fns):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for f in fns[: min(len(fns), 4)]:
            f()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for f in fns:
            f()
    return graph


def prewarm(graph, seconds=0.06):
    """Replay until `seconds` of wall time have passed: the first tens of milliseconds of GPU work after an idle
    period run up to 10 % slow on this part (clock ramp; measured with tools/kbench.hip: 66.8 -> 59.9 us for the same
    encoder-shape launch over the first five measurements).  Untimed, outside every timed region."""
    t0 = time.perf_counter()
    while True:
        graph.replay()
        torch.cuda.synchronize()
        if time.perf_counter() - t0 >= seconds:
            return


def event_time_us(graph, launches, reps=15):
    """Median microseconds per launch, HIP events on the launch stream: (time of three back-to-back replays -
    time of one) / (2 x launches), i.e. the steady-state duration of a launch incl. the gap to the next one,
    without the one-off latency of starting a graph on an idle GPU (~10 us, which one replay of 24 launches
    would spread over them as +0.4 us each)."""
    prewarm(graph)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(k):
        ts = []
        for _ in range(reps):
            e0.record()
            for _ in range(k):
                graph.replay()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        ts.sort()
        return ts[len(ts) // 2]
    return (timed(3) - timed(1)) / (2 * launches)


def count_launches(step):
    """Device-side events (kernels, memsets, copies) of ONE more step, outside the timed region (torch.profiler;
    round 1: 5 696 by rocprofv3, profiles/r01_model_step_by_category.csv)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as e:      # a profiler problem must not cost the bench line
        return f"unavailable: {type(e).__name__}"


def model_step_leg(rank, local_rank, world, device, steps, warmup=3, clips_per_rank=2, bf16=False, count=False,
                   tuned_gemms=True, graph=False):
    """clips/s of the SeqFormer-R50 training step (BASELINE config: T=5 synthetic 360p clip, 300
    queries): forward + backward + RCCL gradient all-reduce + clipped AdamW step, two clips per
    rank -- the reference's per-GPU batch (IMS_PER_BATCH 16 on 8 GPUs, configs/base_ytvis.yaml:18) --
    weak scaling.  The loss is the reference's objective (clip-level Hungarian matching,
    focal / L1 / GIoU / mask focal + dice over the 6 decoder layers, vnext_amd/models/criterion.py)
    on 4 synthetic tracks per clip, with the fused dynamic mask head forward and backward.
    graph: the training trunk (backbone, transformer, heads; forward and backward) replayed from hipGraphs
    (train.capture_training_graphs; the clips of a step have one size).  Off for the figure this leg reports: the fp32 step
    is bound by its kernels and a replay of ~2 800 graph nodes is SLOWER than launching them (MI355X, same process: 59.2 ms
    eager, 62.5 replayed; round 6) -- the bf16 legs, whose kernels are shorter, are reported both ways by main()."""
    import torch.distributed as dist
    import vnext_amd.models  # noqa: F401
    from vnext_amd import train as T
    from vnext_amd import tuning
    from vnext_amd.registry import build_model, get_seqformer_cfg
    # the Linear / attention GEMMs are plain library GEMMs: take the rocBLAS / hipBLASLt solutions recorded offline for
    # these shapes on MI355X (vnext_amd/tuning, tuning itself off); tuned_gemms=False = the library's default heuristic
    gemms = tuning.enable() if tuned_gemms else (tuning.disable() or tuning.status())
    torch.manual_seed(0)
    cfg = get_seqformer_cfg(**{"MODEL.DEVICE": str(device)})
    model = build_model(cfg).train()
    timer = T.CommTimer() if world > 1 else None
    clips = T.synthetic_clips(clips_per_rank, 5, 360, 640, device, seed=100 + rank, num_instances=4)
    graph_state = (T.capture_training_graphs(model, clips, torch.bfloat16 if bf16 else None) if graph     # (before wrap_ddp)
                   else {"enabled": False, "why": "eager trunk"})
    ddp = T.wrap_ddp(model, local_rank, comm_timer=timer)
    opt = T.build_optimizer(model)
    def step():
        if bf16:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return T.train_step(ddp, opt, clips, comm_timer=timer)
        return T.train_step(ddp, opt, clips, comm_timer=timer)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    n_params = sum(p.numel() for p in model.parameters() if p.requires_grad)
    comm = timer.report() if timer is not None else None      # the last timed step's all-reduces (rank 0's view)
    launches = None
    if count:       # one more step on every rank (the gradient all-reduce needs them all); rank 0 counts its launches
        if rank == 0:
            launches = count_launches(step)
        else:
            step()
            torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
    T.release_training_graphs(model)
    del ddp, opt, model
    torch.cuda.empty_cache()
    return {"clips_per_s": world * clips_per_rank * steps / dt, "ms_per_step": dt * 1e3 / steps, "steps": steps,
            "launches_per_step": launches, "library_gemms": gemms, "graph_training": graph_state,
            "clips_per_rank": clips_per_rank, "n_gpus": world, "trainable_params": n_params,
            "grad_allreduce_MB_per_step": round(n_params * 4 / 1e6, 1),
            "ddp_bucket_cap_MB": T.ddp_bucket_mb() if world > 1 else None,
            "ddp_comm": comm,
            "config": "SeqFormer R50 (random init), T=5, 360x640 -> 384x640, 300 queries, 6+6 layers, fp32; "
                      "SetCriterion on 4 synthetic tracks per clip (matcher + focal/L1/GIoU/mask losses, deep supervision); DDP static_graph + gradient_as_bucket_view over RCCL"}


GRAPH_LEGS = {      # name -> (architecture, clips, frames per clip, height, width, instances, seed)
    "seqformer_360p_bf16": ("seqformer", 2, 5, 360, 640, 4, 100),
    "seqformer_720p_bf16": ("seqformer", 1, 5, 720, 1280, 4, 104),
    "idol_720p_bf16": ("idol", 1, 2, 720, 1280, 8, 8),
}


def graph_leg_child(name, steps):
    """`python bench.py --graph-leg <name>`: ONE bf16 training leg with its trunk replayed from hipGraphs
    (train.capture_training_graphs), in a process of its own -> one JSON object on stdout.  The parent bench runs these as child
    processes: a captured graph slows the eager steps of ITS process, and a fault inside a capture --
    there has been one kind, under DistributedDataParallel -- must not cost the bench its line."""
    import vnext_amd.models  # noqa: F401
    from vnext_amd import train as T
    from vnext_amd import tuning
    from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg
    arch, n_clips, frames, h, w, inst, seed = GRAPH_LEGS[name]
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    state = {"channels_last_trunk": T.enable_channels_last(), "conv_search": tuning.enable_conv_search(), "library_gemms": tuning.enable()}
    torch.manual_seed(0)
    if arch == "idol":
        model = build_model(get_idol_cfg(**{"MODEL.DEVICE": str(device)})).train()
        opt = T.build_optimizer(model, base_lr=1e-4)
    else:
        model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": str(device)})).train()
        opt = T.build_optimizer(model)
    clips = T.synthetic_clips(n_clips, frames, h, w, device, seed=seed, num_instances=inst)
    graph_state = T.capture_training_graphs(model, clips, torch.bfloat16)

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return T.train_step(model, opt, clips)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    print(json.dumps({"ms_per_step": ms, "clips_per_s": n_clips * 1e3 / ms, "steps": steps, "graph_training": graph_state, **state}))


def graph_leg(name, steps=10, timeout_s=420):
    """The graph-replayed bf16 leg `name`, measured by a child process (graph_leg_child) -> its dict, or {"error": ...}."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--graph-leg", name, "--model-steps", str(steps)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MIOPEN_USER_DB_PATH")}
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout_s, env=env)
        lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
        if r.returncode != 0 or not lines:
            return {"error": "child exited with %s: %s" % (r.returncode, (r.stderr or "").strip()[-300:])}
        out = json.loads(lines[-1])
        out["how"] = "measured in a child process (python bench.py --graph-leg %s): captured graphs stay out of this process" % name
        return out
    except (subprocess.TimeoutExpired, OSError, ValueError) as e:
        return {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}


def extra_model_legs(device):
    """Single-GPU legs for the other SURVEY section 8d configs (rank 0, N=1 only; a few seconds each):
    C2 SeqFormer-R50 whole-clip inference, C3-like IDOL-R50 key/reference training step, C5 IDOL-R50
    video inference with the tracker.  Random-init weights, synthetic frames / annotations, fp32."""
    import vnext_amd.models  # noqa: F401
    from vnext_amd import train as T
    from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg
    from vnext_amd import tuning
    tuning.enable()

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n
    out = {}
    torch.manual_seed(0)
    # Order: the eager training figures first, then the inference legs (whose trunks are replayed from hipGraphs); the
    # graph-replayed TRAINING forms run in child processes (graph_leg) -- a captured training graph slows the eager steps of its
    # process while it lives, and some of that outlasts it (round 6: SeqFormer step 56.1 ms before a capture, 57.1 after capture +
    # release).
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": str(device)})).train()
    opt = T.build_optimizer(model, base_lr=1e-4)
    pair = T.synthetic_clips(1, 2, 720, 1280, device, seed=8, num_instances=8)

    def idol_step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return T.train_step(model, opt, pair)
    for _ in range(3):
        idol_step()
    ms = timed(idol_step, 5)
    out["idol_train_step"] = {"ms_per_step": ms, "pairs_per_s": 1e3 / ms,
                              "config": "IDOL R50, one key/reference pair 720x1280, 8 objects, bf16 autocast (bf16 GEMMs and op "
                                        "value, fp32 locations / losses / reid kernels), simOTA + reid losses, AdamW"}
    del opt, model
    out["seqformer_train_step_720p"] = seqformer_720p_leg(device, timed)
    # -- the graph-replayed forms of the two bf16 legs above, each in a child process
    torch.cuda.empty_cache()
    out["idol_train_step"]["graphed_trunk"] = {
        **graph_leg("idol_720p_bf16", 5),
        "note": "the same step with the trunk replayed from hipGraphs (IDOL.graph_training): a key / reference pair is two frames, "
                "the eager step is bound by the host's launches"}
    out["seqformer_train_step_720p"]["bf16_autocast"]["graphed_trunk"] = graph_leg("seqformer_720p_bf16", 6)
    # -- inference (trunks replayed from hipGraphs)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": str(device)})).eval()
    clip = T.synthetic_clips(1, 5, 360, 640, device, seed=7, num_instances=0)
    for _ in range(2):
        model(clip)
    ms = timed(lambda: model(clip), 10)
    out["seqformer_inference"] = {"ms_per_clip": ms, "clips_per_s": 1e3 / ms, "frames_per_s": 5e3 / ms,
                                  "config": "SeqFormer R50, T=5, 360x640, 300 queries, trunk replayed from a hipGraph, "
                                            "top-10 masks at input resolution"}
    del model
    gc.collect()
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": str(device)})).eval()
    g = torch.Generator(device=device).manual_seed(1)
    for name, (h, w) in (("360p", (360, 640)), ("720p", (720, 1280))):
        video = [{"image": [torch.rand(3, h, w, device=device, generator=g) * 255 for _ in range(36)],
                  "height": h, "width": w}]
        model(video)
        ms = timed(lambda: model(video), 3)
        out[f"idol_video_inference_{name}"] = {"ms_per_video": ms, "frames_per_s": 36e3 / ms,
                                               "config": f"IDOL R50, 36 frames {h}x{w} in chunks of 10, tracker on"}
    del model
    torch.cuda.empty_cache()
    return out


def seqformer_720p_leg(device, timed):
    """BASELINE config 4 at N = 1: the SeqFormer training step on ONE T = 5 clip of 720 x 1280 frames per GPU (the per-GPU
    batch of projects/SeqFormer/configs/large_model/swin_ytvis.yaml on 8 GPUs; R50 trunk standing in for Swin-L, which
    SURVEY.md section 2 leaves out of scope): the 19 560-pixel encoder, 6 decoder layers x 5 frames of 720p mask-head
    training, the criterion and the optimiser together.  fp32 and bf16 autocast; ms / step, clips / s, launches, peak memory."""
    import vnext_amd.models  # noqa: F401
    from vnext_amd import train as T
    from vnext_amd.registry import build_model, get_seqformer_cfg
    res = {"config": "SeqFormer R50 (random init), T=5, 720x1280 -> 736x1280, 300 queries, 6+6 layers, 1 clip per GPU, 4 synthetic "
                     "tracks, SetCriterion + clipped AdamW; N = 1 point of BASELINE config 4 (R50 for Swin-L)"}
    for key, amp in (("fp32", False), ("bf16_autocast", True)):
        torch.manual_seed(0)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(device)
        model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": str(device)})).train()
        opt = T.build_optimizer(model)
        clips = T.synthetic_clips(1, 5, 720, 1280, device, seed=104, num_instances=4)

        def step(model=model, opt=opt, clips=clips, amp=amp):      # (bound now: the bf16 step outlives this loop, see below)
            if amp:
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    return T.train_step(model, opt, clips)
            return T.train_step(model, opt, clips)
        for _ in range(3):
            step()
        ms = timed(step, 6)
        res[key] = {"ms_per_step": ms, "clips_per_s": 1e3 / ms, "launches_per_step": count_launches(step),
                    "peak_memory_GiB": torch.cuda.max_memory_allocated(device) / 2**30}
        del model, opt, clips
    torch.cuda.empty_cache()
    return res


def latest_profile(suffix):
    """The newest committed summary profiles/rNN_<suffix> (tools/summarize_prof.py), or None."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_" + suffix)))
    if not files:
        return None
    try:
        with open(files[-1]) as f:
            return {"file": os.path.relpath(files[-1], ROOT), "data": json.load(f)}
    except (OSError, ValueError):
        return None


def latest_pmc_row(kernel, case=None):
    """The row of `kernel` in the newest committed profiles/rNN_backward_pmc.csv (tools/prof_backward_pmc.sh: rocprofv3 --pmc
    passes, counters per launch + the derived columns), as a dict of floats, or None."""
    import csv
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_backward_pmc.csv")))
    for path in reversed(files):
        try:
            with open(path) as f:
                rows = list(csv.DictReader(line for line in f if not line.startswith("#")))
        except OSError:
            continue
        for r in rows:
            if kernel in r.get("kernel", "") and (case is None or r.get("case") == case):
                out = {"source": os.path.relpath(path, ROOT)}
                for k, v in r.items():
                    try:
                        out[k] = float(v)
                    except (TypeError, ValueError):
                        out[k] = v
                return out
    return None


def valu_ceiling(entry, kernel):
    """The mask-head kernels are bound by vector-instruction ISSUE, not by the write roofline their bytes suggest:
    attach the committed counter evidence and say so.  valu_issue_frac = SQ_INSTS_VALU x 4 clk / 1 024 SIMDs / (duration x
    2.0 GHz) -- the share of all vector-issue slots the kernel's instructions occupy at 4 clocks each (an upper bound: packed
    and transcendental instructions differ), from the profiled run; the HBM figures stay beside it."""
    row = latest_pmc_row(kernel)
    if row is None:
        return entry
    entry["hbm_frac"] = entry["frac"]
    entry["bound"] = "valu"
    entry["valu_issue_frac"] = row.get("valu_issue_frac")
    entry["valu_insts_per_wave"] = row.get("valu_per_wave")
    entry["wait_frac"] = row.get("wait_frac")
    entry["valu_profiled_us"] = row.get("duration_us_rocprofv3")
    entry["valu_source"] = row["source"]
    entry["bound_note"] = ("vector-instruction issue: %.0f %% of the issue slots of the profiled launch (%s us) at 4 clk per instruction; "
                           "`frac` / `hbm_frac` = algorithmic bytes against the HBM write roofline, which is NOT what binds this kernel"
                           % (100 * (row.get("valu_issue_frac") or 0), row.get("duration_us_rocprofv3")))
    return entry


def largest_divisor_leq(n, cap):
    for d in range(min(n, cap), 0, -1):
        if n % d == 0:
            return d
    return 1


# ------------------------------------------------------------------------------------------------
# op-level rooflines beyond the headline (rank 0, N = 1): every BASELINE shape, both location
# distributions, the bf16 case of config 3, and the two other kernel families
# ------------------------------------------------------------------------------------------------
def pixel_centres(res, device):
    refs = []
    for h, w in SHAPES[res]:
        ys, xs = torch.meshgrid(torch.arange(h, device=device) + 0.5, torch.arange(w, device=device) + 0.5, indexing="ij")
        refs.append(torch.stack([xs.reshape(-1) / w, ys.reshape(-1) / h], -1))
    return torch.cat(refs, 0)


def make_case(res, B, Lq, dist, vdtype, seed, device):
    """One input set of an op-level case.  dist "U": locations uniform in [0,1)^2 (ops/test.py:34);
    "M": model-like -- reference point per query (encoder, Lq == S: the pixel centres of the pyramid,
    deformable_transformer.py:183-190; decoder: random box centres) + (head direction x (k+1) + N(0,1))
    pixels of every level (the module's initialisation, ops/modules/ms_deform_attn.py:65-73)."""
    g = torch.Generator(device=device).manual_seed(seed)
    if (res, str(device)) not in _LEVELS:
        sh = torch.tensor(SHAPES[res], dtype=torch.long, device=device)
        _LEVELS[(res, str(device))] = (sh, torch.cat((sh.new_zeros((1,)), sh.prod(1).cumsum(0)[:-1])))
    shapes, lsi = _LEVELS[(res, str(device))]
    S = int(shapes.prod(1).sum())
    value = torch.randn(B, S, 8, 32, device=device, generator=g).to(vdtype)
    if dist == "U":
        loc = torch.rand(B, Lq, 8, 4, 4, 2, device=device, generator=g)
    else:
        ref = pixel_centres(res, device).view(1, S, 1, 1, 1, 2) if Lq == S else \
            torch.rand(B, Lq, 1, 1, 1, 2, device=device, generator=g)
        th = torch.arange(8, device=device) * (2 * math.pi / 8)
        d = torch.stack([th.cos(), th.sin()], -1)
        d = d / d.abs().max(-1, keepdim=True)[0]
        k = torch.arange(1, 5, device=device).view(1, 1, 1, 1, 4, 1)
        offs = d.view(1, 1, 8, 1, 1, 2) * k + torch.randn(B, Lq, 8, 4, 4, 2, device=device, generator=g)
        wh = torch.stack([shapes[:, 1], shapes[:, 0]], -1).float().view(1, 1, 1, 4, 1, 2)
        loc = (ref + offs / wh).contiguous()
    attn = torch.softmax(torch.randn(B, Lq, 8, 16, device=device, generator=g), -1).view(B, Lq, 8, 4, 4).contiguous()
    grad_out = torch.randn(B, Lq, 256, device=device, generator=g).to(vdtype)
    out = torch.empty(B, Lq, 256, device=device, dtype=vdtype)
    gv, gl, ga = torch.empty_like(value), torch.empty_like(loc), torch.empty_like(attn)
    from vnext_amd import _lib
    vdt = _lib.VNX_F32 if vdtype == torch.float32 else _lib.VNX_BF16
    ws_bytes = _lib.lib().vnx_msda_backward_workspace_bytes(vdt, _lib.VNX_F32, B, S, 8, 32, 4, Lq, 4, 1)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=device)
    return dict(ws=ws, ws_bytes=ws_bytes, shapes=shapes, lsi=lsi, value=value, loc=loc, attn=attn, grad_out=grad_out,
                out=out, gv=gv, gl=gl, ga=ga, S=S, vdt=vdt)


def touched_rows(case, res):
    """Distinct (batch, pixel, head) rows of `value` the taps of this case's samples land on (counted on the device
    from the locations: floor, the in-map test of ms_deform_im2col_cuda.cuh:288 and the four corner tests :55-78)."""
    loc = case["loc"].float()                                   # [B, Lq, M, L, K, 2]
    B, Lq, M, L, K, _ = loc.shape
    S = case["S"]
    seen = torch.zeros(B * S * M, dtype=torch.bool, device=loc.device)
    bm = (torch.arange(B, device=loc.device).view(B, 1, 1, 1) * S * M + torch.arange(M, device=loc.device).view(1, 1, M, 1))
    start = 0
    for l, (H, W) in enumerate(SHAPES[res]):
        h = loc[:, :, :, l, :, 1] * H - 0.5
        w = loc[:, :, :, l, :, 0] * W - 0.5
        ok = (h > -1) & (w > -1) & (h < H) & (w < W)
        h0, w0 = h.floor().long(), w.floor().long()
        for dy in (0, 1):
            for dx in (0, 1):
                y, x = h0 + dy, w0 + dx
                inside = ok & (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
                idx = (bm + (start + y * W + x) * M)[inside]
                seen[idx] = True
        start += H * W
    return int(seen.sum())


def addressable_bytes(B, S, Lq, e=4, e_loc=4, M=8, D=32, L=4, K=4, rows=None):
    """SURVEY 8(d)'s byte count assumes the whole `value` is read.  A call with few queries on a large map cannot touch
    it all (decoder 720p: 768 K taps on 782 K rows reach 63 % of them).  -> (forward, backward) bytes with the value
    READ counted for the rows the samples really touch (`rows`, from touched_rows; at most min(4 * points, B S M));
    grad_value is still written in full: every row has an owner."""
    if rows is None:
        rows = min(4 * B * Lq * M * L * K, B * S * M)
    samples = B * Lq * M * L * K
    fwd = e * D * rows + e_loc * 3 * samples + e * B * Lq * M * D
    bwd = e * D * rows + e * D * B * S * M + e * B * Lq * M * D + e_loc * 6 * samples
    return fwd, bwd


OP_CASES = [
    # key, resolution, B, Lq (None = S: the encoder shape), distribution, value dtype, what it is
    ("decoder_360p_M", "360p", 5, 300, "M", torch.float32, "headline shape with model-like locations"),
    ("decoder_360p_U_B10", "360p", 10, 300, "U", torch.float32, "two clips per GPU folded (the reference's per-GPU batch)"),
    ("decoder_720p_U", "720p", 5, 300, "U", torch.float32, "decoder call, 720p"),
    ("decoder_720p_U_bf16", "720p", 5, 300, "U", torch.bfloat16, "config 3: bf16 value / grad, fp32 locations"),
    ("encoder_360p_M", "360p", 5, None, "M", torch.float32, "encoder call (94 % of a model's points), 360p"),
    ("encoder_720p_M", "720p", 2, None, "M", torch.float32, "encoder call, 720p, two frames"),
    ("encoder_360p_M_bf16", "360p", 5, None, "M", torch.bfloat16, "encoder call in bf16 (fp32 locations), 360p"),
    ("encoder_720p_M_bf16", "720p", 2, None, "M", torch.bfloat16, "config 3's largest call: encoder, 720p, bf16"),
]


def op_case_rooflines(op, device):
    out = {}
    for key, res, B, Lq, dist, vdtype, what in OP_CASES:
        S = sum(h * w for h, w in SHAPES[res])
        Lq = Lq or S
        e = 4 if vdtype == torch.float32 else 2
        probe = make_case(res, B, Lq, dist, vdtype, 1, device)
        in_bytes = sum(probe[k].numel() * probe[k].element_size() for k in ("value", "loc", "attn", "grad_out"))
        nsets = max(2, min(12, math.ceil(320 * 2**20 / in_bytes)))
        sets = [probe] + [make_case(res, B, Lq, dist, vdtype, 1 + i, device) for i in range(1, nsets)]
        inner = max(nsets, 8)
        nominal_fwd, nominal_bwd = algorithmic_bytes(B, S, Lq, e=e)
        rows_touched = touched_rows(probe, res)
        bytes_fwd, bytes_bwd = addressable_bytes(B, S, Lq, e=e, rows=rows_touched)
        g_fwd = capture([(lambda s=sets[i % nsets]: op.fwd(s, B, Lq)) for i in range(inner)])
        g_bwd = capture([(lambda s=sets[i % nsets]: op.bwd(s, B, Lq)) for i in range(inner)])
        us_f, us_b = event_time_us(g_fwd, inner, reps=9), event_time_us(g_bwd, inner, reps=9)
        points = 128 * B * Lq
        out[key] = {
            "what": what, "B": B, "Lq": Lq, "S": S, "loc": dist, "value_dtype": "f32" if e == 4 else "bf16",
            "points": points, "input_rotation_sets": nsets,
            "value_rows_touched": rows_touched, "value_rows": B * S * 8,
            # bytes = SURVEY 8(d)'s count with the value read limited to the rows this case's samples touch
            # (touched_rows / addressable_bytes); `nominal_*` = the count that assumes the whole `value` is read
            "fwd": {"us_per_launch": us_f, "algorithmic_bytes": bytes_fwd, "achieved_GBs": bytes_fwd / us_f / 1e3,
                    "frac_of_hbm_peak": bytes_fwd / us_f / 1e3 / HBM_PEAK_GBS, "gpoints_per_s": points / us_f / 1e3,
                    "nominal_bytes": nominal_fwd, "nominal_frac": nominal_fwd / us_f / 1e3 / HBM_PEAK_GBS},
            "bwd": {"us_per_launch": us_b, "algorithmic_bytes": bytes_bwd, "achieved_GBs": bytes_bwd / us_b / 1e3,
                    "frac_of_hbm_peak": bytes_bwd / us_b / 1e3 / HBM_PEAK_GBS,
                    "nominal_bytes": nominal_bwd, "nominal_frac": nominal_bwd / us_b / 1e3 / HBM_PEAK_GBS},
            "fwd_bwd_gpoints_per_s": points / (us_f + us_b) / 1e3,
        }
        del sets, probe, g_fwd, g_bwd
        torch.cuda.empty_cache()
    return out


def gather_ceiling(device):
    """What this memory system delivers for the forward's access pattern with no kernel around it: random
    128-B rows, 8 lanes x 16 B each (vnx_debug_row_gather_probe), cold (a 384 MiB table, > Infinity Cache)
    and from a 24 MiB table (the size of the headline `value`; L2 / Infinity Cache resident)."""
    from vnext_amd import _lib
    lib = _lib.lib()
    res = {}
    sink = torch.zeros(4, device=device)
    for name, mib in (("cold_384MiB", 384), ("cache_resident_24MiB", 24)):
        n_rows = mib * 2**20 // 128
        table = torch.empty(n_rows * 32, device=device).normal_()
        n_idx = 4 * 2**20
        idx = torch.randint(0, n_rows, (n_idx,), device=device, dtype=torch.int64).to(torch.int32)
        best = None
        for nf in (4, 8):
            def run(nf=nf):
                _lib.check(lib.vnx_debug_row_gather_probe(table.data_ptr(), n_rows, idx.data_ptr(), n_idx, nf,
                                                          sink.data_ptr(), torch.cuda.current_stream().cuda_stream))
            g = capture([run] * 4)
            us = event_time_us(g, 4, reps=7)
            gbs = n_idx * 128 / us / 1e3
            if best is None or gbs > best[0]:
                best = (gbs, nf, us)
        res[name] = {"GBs": best[0], "rows_in_flight_per_lane": best[1], "us": best[2], "rows": n_idx}
        del table, idx
        torch.cuda.empty_cache()
    return res


def head_rooflines(device):
    """The other two kernel families of the path: the fused dynamic mask head (output-write bound,
    bytes = 4 (8 HW + 171 n + 4 n HW) per frame) and the reid similarity on the matrix cores."""
    from vnext_amd import _lib
    from vnext_amd.heads import dynamic_mask_with_coords
    from vnext_amd.heads import reid as R
    lib = _lib.lib()
    out = {}
    for name, (H, W) in (("360p", (48, 80)), ("720p", (92, 160))):
        n = 300
        sets = []
        for i in range(8):
            g = torch.Generator(device=device).manual_seed(i)
            feats = torch.randn(1, 8, H, W, device=device, generator=g)
            ref = torch.rand(1, n, 2, device=device, generator=g) * torch.tensor([W * 8.0, H * 8.0], device=device)
            params = 0.3 * torch.randn(1, n, 169, device=device, generator=g)
            sets.append((feats, ref, params))
        with torch.no_grad():
            fns = [(lambda s=s: dynamic_mask_with_coords(s[0], s[1], s[2], [n], 8)) for s in sets] * 3
            us = event_time_us(capture(fns), len(fns), reps=9)
        nbytes = 4 * (8 * H * W + n * 171 + n * 4 * H * W)
        out[f"mask_head_fwd_{name}_n300"] = valu_ceiling({
            "bound": "hbm", "kernel": "dynamic_mask_head_runs_kernel", "us_per_launch": us, "algorithmic_bytes": nbytes,
            "achieved": nbytes / us / 1e3, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": nbytes / us / 1e3 / HBM_PEAK_GBS,
            "what": f"one {name} frame, 300 instances -> logits [300, {2 * H}, {2 * W}] fp32"}, "dynamic_mask_head_runs_kernel")
    # training shape: T = 5 frames x 6 decoder layers x 4 matched instances, forward + backward
    H, W, n_img, per = 48, 80, 5, 24
    n = n_img * per
    g = torch.Generator(device=device).manual_seed(5)
    feats = torch.randn(n_img, 8, H, W, device=device, generator=g).requires_grad_(True)
    ref = (torch.rand(1, n, 2, device=device, generator=g) * torch.tensor([W * 8.0, H * 8.0], device=device)).requires_grad_(True)
    params = (0.3 * torch.randn(1, n, 169, device=device, generator=g)).requires_grad_(True)
    gout = torch.randn(1, n, 2 * H, 2 * W, device=device, generator=g)

    def step():
        o = dynamic_mask_with_coords(feats, ref, params, [per] * n_img, 8)
        o.backward(gout)
        feats.grad = ref.grad = params.grad = None
    how = "hipGraph of 8 forward+backward steps through autograd"
    try:
        us = event_time_us(capture([step] * 8), 8, reps=9)
    except Exception as e:      # capture of the autograd backward not possible: time it eagerly (host-bound)
        how = f"eager ({type(e).__name__} during capture)"
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            step()
        e1.record()
        e1.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / 20
    nbytes = 4 * (2 * 8 * n_img * H * W + 2 * n * 171 + 2 * n * 4 * H * W)      # forward traffic + the same for the gradients
    out["mask_head_fwd_bwd_train_360p_n120"] = valu_ceiling({
        "bound": "hbm", "kernel": "dynamic_mask_head_runs_kernel + dynamic_mask_head_bwd_kernel", "timing": how,
        "us_per_step": us, "algorithmic_bytes": nbytes, "achieved": nbytes / us / 1e3, "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": nbytes / us / 1e3 / HBM_PEAK_GBS, "what": "5 frames x 24 matched instances (6 decoder layers x 4 tracks), 360p"},
        "dynamic_mask_head_bwd_kernel")
    # reid: 300 detections x 300 memory embeddings x 256 channels, dot and cosine, + bi-softmax
    a = torch.randn(300, 256, device=device)
    b = torch.randn(300, 256, device=device)
    with torch.no_grad():
        fns = [lambda: R.similarity(a, b)] * 16
        us_dot = event_time_us(capture(fns), 16, reps=9)
        a50, b50 = a[:50].contiguous(), b[:50].contiguous()     # a tracker frame: tens of detections x tens of tracklets
        fns = [lambda: R.match_scores(a50, b50, "bisoftmax")] * 16
        us_match = event_time_us(capture(fns), 16, reps=9)
    flops = 2.0 * 300 * 300 * 256
    out["reid_similarity_300x300x256"] = {
        "bound": "mfma", "kernel": "reid_similarity_kernel (v_mfma_f32_16x16x4_f32)", "us_per_launch": us_dot, "flops": flops,
        "achieved": flops / us_dot / 1e6, "peak": 157.3, "unit": "TFLOP/s", "frac": flops / us_dot / 1e6 / 157.3,
        "us_match_scores_bisoftmax_50x50": us_match,
        "what": "46 MFLOP: launch / latency bound by construction; MFMA utilisation is not the point, one launch per image is"}
    out["tracker_frame_360p_n20"] = tracker_frame_times(device)
    return out


def tracker_frame_times(device, n=20, frames=40):
    """IDOL's per-frame association on a synthetic video of `frames` frames with n
    detections each at the 360p mask size (90 x 160): wall-clock per frame of the device-resident tracker
    (vnx_tracker_frame: no host copy; ids read once at the end) against the host-steered IDOL_Tracker of round 1
    (two device->host copies per frame), same inputs, same ids."""
    from vnext_amd.models.tracker import DeviceTracker, IDOL_Tracker
    args = dict(init_score_thr=0.2, obj_score_thr=0.1, nms_thr_pre=0.5, nms_thr_post=0.05, addnew_score_thr=0.2,
                memo_tracklet_frames=10, memo_momentum=0.8, long_match=True, frame_weight=True, temporal_weight=True,
                memory_len=3)
    g = torch.Generator(device=device).manual_seed(11)
    ident = 3.0 * torch.randn(n, 256, device=device, generator=g)
    ys = torch.arange(90, device=device)[:, None]
    xs = torch.arange(160, device=device)[None, :]
    video = []
    for t in range(frames):
        masks = torch.stack([torch.where((xs >= 7 * k + t) & (xs < 7 * k + t + 12) & (ys >= 4 * k) & (ys < 4 * k + 9), 3.0, -3.0)
                             for k in range(n)])[:, None] + 0.5 * torch.randn(n, 1, 90, 160, device=device, generator=g)
        score = torch.linspace(0.95, 0.4, n, device=device)
        video.append((torch.cat([torch.rand(n, 4, device=device, generator=g), score[:, None]], 1),
                      torch.zeros(n, dtype=torch.long, device=device), masks,
                      ident + 0.4 * torch.randn(n, 256, device=device, generator=g)))
    res = {}
    ids = {}
    for name, cls in (("device", DeviceTracker), ("host_steered", IDOL_Tracker)):
        best = None
        for _ in range(3):
            tr = cls(**args)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "device":
                out = [tr.match_device(b, l, m, e, t) for t, (b, l, m, e) in enumerate(video)]
                out = torch.stack(out).cpu()
            else:
                out = torch.full((frames, n), -3, dtype=torch.long)
                for t, (b, l, m, e) in enumerate(video):
                    _, _, got, kept = tr.match(b, l, m, e, t, list(range(n)))
                    out[t, kept] = got
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / frames * 1e6
            best = dt if best is None else min(best, dt)
        res[f"us_per_frame_{name}"] = best
        ids[name] = out
    res["same_ids"] = bool(ids["device"].shape == ids["host_steered"].shape and torch.equal(ids["device"], ids["host_steered"]))
    res["host_copies_per_frame"] = {"device": 0, "host_steered": 2}
    res["what"] = f"{frames} frames x {n} detections, masks 90 x 160, 256-channel embeddings; wall clock incl. Python"
    return res


def cpu_baseline(B, Lq, res, budget_s=14.0):
    """The reference's pure-PyTorch fallback on the host cores, same workload, structured as SURVEY.md section 8(d)
    prescribes: `ms_deform_attn_core_pytorch` (ops/functions/ms_deform_attn_func.py:42-62: per-level grid_sample, the
    [N*M, D, Lq, L*P] stack, weighted sum) called once per frame as the module's loop does
    (ops/modules/ms_deform_attn.py:107-120) -- oracle/msda_torch_fallback.py: msda_core_frames, which equals the
    reference's own function bit for bit and runs within 10 % of its time where both can be run
    (oracle/time_reference_cpu.py -> profiles/rNN_cpu_reference_fn.json, attached as `reference_fn`).  Beside it the folded
    one-call form (rounds 1-4's figure) and the C oracle (oracle/msda_oracle.c)."""
    import numpy as np
    from oracle import msda_oracle as O
    from oracle.msda_torch_fallback import msda_core_frames, msda_grid_sample
    shapes = np.array(SHAPES[res], dtype=np.int64)
    sizes = [tuple(int(x) for x in hw) for hw in shapes]
    lsi = O.level_start_index(shapes)
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    rng = np.random.default_rng(3)
    value = rng.standard_normal((B, S, 8, 32)).astype(np.float32)
    loc = rng.random((B, Lq, 8, 4, 4, 2)).astype(np.float32)
    attn = rng.random((B, Lq, 8, 4, 4)).astype(np.float32)
    attn /= attn.sum((-1, -2), keepdims=True)
    go = rng.standard_normal((B, Lq, 256)).astype(np.float32)
    points = 128 * B * Lq
    cores = os.cpu_count() or 1
    tthreads = min(cores, 16)  # grid_sample does not scale past a few threads; avoid oversubscription
    torch.set_num_threads(tthreads)
    tv, tl, ta = (torch.from_numpy(x).requires_grad_(True) for x in (value, loc, attn))
    tg = torch.from_numpy(go)

    def frames():       # the B folded frames as one clip of T = B frames: one call per frame
        out = msda_core_frames(tv.unsqueeze(0), sizes, tl.unsqueeze(0), ta.unsqueeze(0))
        out.backward(tg.unsqueeze(0))

    def folded():
        msda_grid_sample(tv, shapes, tl, ta).backward(tg)

    def median(fn, budget):
        ts = []
        t_start = time.perf_counter()
        while len(ts) < 3 or (time.perf_counter() - t_start < budget and len(ts) < 25):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
            tv.grad = tl.grad = ta.grad = None
        return sorted(ts)[len(ts) // 2], len(ts)
    fmed, fn_ = median(frames, budget_s * 0.4)
    gmed, gn = median(folded, budget_s * 0.2)
    best = None
    for nt in sorted({1, min(cores, 32)}):
        ts = []
        t_start = time.perf_counter()
        while len(ts) < 3 or (time.perf_counter() - t_start < budget_s / 5 and len(ts) < 25):
            t0 = time.perf_counter()
            O.msda_forward(value, shapes, lsi, loc, attn, nthreads=nt)
            O.msda_backward(value, shapes, lsi, loc, attn, go, nthreads=nt)
            ts.append(time.perf_counter() - t0)
        med = sorted(ts)[len(ts) // 2]
        if best is None or med < best[0]:
            best = (med, nt, len(ts))
    med, nt, n = best
    ref = latest_profile("cpu_reference_fn.json")
    return {
        "value": points / fmed / 1e9, "unit": "Gpoints/s", "cores": tthreads, "kind": "port",
        "sample": f"{fn_} x (fwd+bwd) of the same B={B},Lq={Lq},{res} fp32 workload through the reference's pure-PyTorch "
                  f"fallback as the reference runs it: ms_deform_attn_core_pytorch's per-level grid_sample + [N*M, D, Lq, L*P] stack, "
                  f"one call per frame in the module's T-frame loop (oracle/msda_torch_fallback.py: msda_core_frames), autograd "
                  f"backward, median; torch intra-op threads = min(host cores, 16); host has {cores} cores",
        "ms_per_step": fmed * 1e3,
        # `value` changed its definition once: rounds 1-4 reported the folded call, rounds 5+ the reference's
        # per-frame loop -- a GPU / CPU ratio taken across that boundary compares two definitions, not two builds.  Both
        # figures sit at this level every round from here on, named by what they are.
        "definition_version": 2,
        "definitions": {"1": "rounds 1-4: T frames folded into ONE call (value_folded_call)",
                        "2": "rounds 5+: one call per frame, the reference module's loop (value_frame_loop = value)"},
        "value_frame_loop": points / fmed / 1e9,
        "value_folded_call": points / gmed / 1e9,
        "folded_call": {"value": points / gmed / 1e9, "unit": "Gpoints/s", "ms_per_step": gmed * 1e3,
                        "sample": f"{gn} x (fwd+bwd), the T frames folded into one call that accumulates per level (no stack): "
                                  "the figure rounds 1-4 reported as `value`"},
        "reference_fn": None if ref is None else {
            "source": ref["file"],
            "note": "the reference's own ms_deform_attn_core_pytorch imported from /root/reference, timed in the build container "
                    "(no /root/reference on the GPU box) next to this port on the same cores: equal bit for bit, time ratio "
                    "port / reference in `port_over_reference_time`",
            **{k: ref["data"].get(k) for k in ("host_cores", "torch_threads")},
            **{res_: {k: c.get(k) for k in ("reference_fn_frame_loop", "port_frame_loop", "port_over_reference_time",
                                            "port_equals_reference_bit_for_bit")}
               for res_, c in ref["data"].get("cases", {}).items()}},
        "c_oracle": {"value": points / med / 1e9, "unit": "Gpoints/s", "cores": nt, "ms_per_step": med * 1e3,
                     "sample": f"{n} x (fwd+bwd) through oracle/msda_oracle.c (OpenMP over (batch, head)), the faster of 1 and "
                               f"{min(cores, 32)} threads"},
    }


def timed_region(run, n, world, device):
    """EXACTLY n calls of `run` bracketed by barrier + synchronize on both sides; the maximum over
    ranks of the elapsed seconds (every rank returns the same number)."""
    import torch.distributed as dist
    on_gpu = device.type == "cuda"
    sync = torch.cuda.synchronize if on_gpu else (lambda: None)
    sync()
    if world > 1:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(n):
        run()
    sync()
    if world > 1:
        dist.barrier()
    sync()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    return elapsed


def headline_line(a, n_gpus, world_readback, ms_per_step, S, nsets, input_bytes, backend):
    points = 128 * a.batch * a.lq
    return {
        "metric": "MSDeformAttn fwd+bwd Gpoints/s (T=5,L=4,Q=300,H=8,K=4)",
        "value": points * n_gpus / (ms_per_step * 1e-3) / 1e9, "unit": "Gpoints/s", "n_gpus": n_gpus,
        "steps": a.steps, "warmup": a.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"SeqFormer-R50 T=5 {a.res} clip folded to B={a.batch}: MSDeformAttn "
                               f"decoder call, Lq={a.lq}, S={S}, M=8, D=32, L=4, K=4, "
                               f"loc~{'U[0,1)' if a.dist == 'U' else 'model-like'}; 1 step = fwd+bwd",
                   "points_per_step": points, "input_rotation_sets": nsets,
                   "input_rotation_MiB": round(nsets * input_bytes / 2**20, 1),
                   "parallelism": f"dp{n_gpus} (clips sharded, no data-path collective)"},
        # read back from the process group, not from the command line: 1 when no group exists
        "rccl_world_size": world_readback, "collective_backend": backend,
    }


def dump_outputs(dirname, arrays):
    """--dump-outputs: each tensor of `arrays` (name -> tensor) as float32 `dirname/<name>.npy`."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    for name, t in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), t.detach().float().cpu().numpy())


def stub_main(a, world, rank):
    """The multi-rank skeleton of main() on CPU tensors and gloo (see StubOp)."""
    import torch.distributed as dist
    device = torch.device("cpu")
    if world > 1:
        dist.init_process_group(a.backend)
    B, Lq = a.batch, a.lq
    S = sum(h * w for h, w in SHAPES[a.res])
    g = torch.Generator().manual_seed(rank)
    s = {"value": torch.randn(B, S, 8, 32, generator=g), "out": torch.empty(B, Lq, 256)}
    s["gv"] = torch.empty_like(s["value"])
    op = StubOp()

    def step():
        op.fwd(s, B, Lq)
        op.bwd(s, B, Lq)
    for _ in range(a.warmup):
        step()
    elapsed = timed_region(step, a.steps, world, device)
    readback = dist.get_world_size() if world > 1 else 1
    if rank == 0 and a.dump_outputs:
        dump_outputs(a.dump_outputs, {"output": s["out"], "grad_value": s["gv"]})
    if rank == 0:
        line = headline_line(a, world, readback, elapsed * 1e3 / a.steps, S, 1, s["value"].numel() * 4, a.backend)
        line["data"] = "stub op on CPU (launcher test only; not a measurement)"
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def self_launch(n, argv):
    """`python bench.py --gpus N` without a torchrun environment: start N ranks of this script, one
    process per GPU (the reference: detectron2/engine/launch.py:67-80, mp.spawn of one worker per GPU),
    through torch.distributed.run on the loopback address; rank 0 of the children prints the line."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on this host driver (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 1) // n)))
    return subprocess.call(cmd, env=env)


class StubOp:
    """CPU stand-in used ONLY by the launcher test (tests/test_bench_launcher.py, --stub-op): it moves
    the same tensors through torch so that the multi-rank plumbing of this script -- spawn, rendezvous,
    barrier, max-over-ranks timing, rank-0 line -- runs on gloo without a GPU.  Not a fallback: without
    --stub-op the script refuses to start when there is no GPU."""

    def fwd(self, s, B, Lq):
        s["out"].copy_(s["value"][:, :Lq].reshape(B, Lq, 256))

    def bwd(self, s, B, Lq):
        s["gv"].copy_(s["value"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="nccl = RCCL (the product); gloo: launcher test")
    ap.add_argument("--stub-op", action="store_true", help="launcher test on CPU: torch copies instead of the HIP op")
    ap.add_argument("--steps", type=int, default=200, help="timed steps: ms_per_step = their region / steps")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's output and gradients as float32 DIR/<name>.npy (rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: repeated regions, model legs, rooflines, other shapes, CPU baseline")
    ap.add_argument("--repeats", type=int, default=21,
                    help="--full: further timed regions of --steps steps each, for the median / min / p10 / p90 spread")
    ap.add_argument("--res", default="360p", choices=list(SHAPES))
    ap.add_argument("--lq", type=int, default=300)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--dist", default="U", choices=["U", "M"])
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baseline leg")
    ap.add_argument("--no-model", action="store_true", help="skip the model-level DDP step (clips/s) leg")
    ap.add_argument("--model-steps", type=int, default=10)
    ap.add_argument("--no-cases", action="store_true", help="skip the other op-level shapes and the mask-head / reid legs")
    ap.add_argument("--no-spans", action="store_true",
                    help="skip the stamped (kernel-span) replays: under rocprofv3 every traced launch is then a plain one")
    ap.add_argument("--no-warm", action="store_true",
                    help="skip the cache-warm forward leg (profiling runs: keeps rocprofv3's per-kernel average cold-only)")
    ap.add_argument("--graph-leg", default=None, choices=list(GRAPH_LEGS),
                    help="child mode: one bf16 training leg with its trunk replayed from hipGraphs -> a JSON object (graph_leg_child)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if a.graph_leg:
        return graph_leg_child(a.graph_leg, a.model_steps)
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(a.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != max(1, a.gpus):
        raise SystemExit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}")
    if a.stub_op:
        return stub_main(a, world, rank)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP library is the only implementation")
    if torch.cuda.device_count() < world:
        raise SystemExit(f"bench.py: {world} ranks but only {torch.cuda.device_count()} GPUs visible")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if a.full:
        from vnext_amd.train import enable_channels_last
        channels_last = enable_channels_last()      # before the process's first convolution (the model legs train in channels-last)
        from vnext_amd import tuning as _tuning
        conv_search = _tuning.enable_conv_search()  # (likewise: MIOpen reads MIOPEN_USER_DB_PATH at its first convolution)
    affinity = None
    if world > 1:
        import torch.distributed as dist
        from vnext_amd.train import set_rank_affinity
        # the ranks of THIS node share its cores (torchrun's LOCAL_WORLD_SIZE), not the whole job's
        affinity = set_rank_affinity(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", str(world))))
        dist.init_process_group("nccl", device_id=device)
    n_gpus = world if world > 1 else 1

    B, Lq, res = a.batch, a.lq, a.res
    op = Op(device)
    probe = make_set(res, B, Lq, 0, device, a.dist)
    S = probe["S"]
    bytes_fwd, bytes_bwd = algorithmic_bytes(B, S, Lq)
    set_bytes = sum(probe[k].numel() * probe[k].element_size()
                    for k in ("value", "loc", "attn", "grad_out", "out", "gv", "gl", "ga"))
    input_bytes = sum(probe[k].numel() * probe[k].element_size() for k in ("value", "loc", "attn", "grad_out"))
    nsets = max(2, math.ceil(320 * 2**20 / input_bytes))
    sets = [probe] + [make_set(res, B, Lq, 1000 * rank + i, device, a.dist) for i in range(1, nsets)]
    points = 128 * B * Lq

    def step_fns(i):
        s = sets[i % nsets]
        return [lambda: op.fwd(s, B, Lq), lambda: op.bwd(s, B, Lq)]

    # ---- the timed region: K steps as replays of a graph of `chunk` steps ------------
    chunk = largest_divisor_leq(a.steps, 100)
    fns = [f for i in range(chunk) for f in step_fns(i)]
    graph = capture(fns)
    prewarm(graph, 0.15)     # clocks up before the W warm-up steps (untimed either way)
    for _ in range(math.ceil(a.warmup / chunk)):
        graph.replay()
    # the region of EXACTLY K steps (barrier + synchronize on both sides, maximum over ranks): ms_per_step = region / K
    elapsed = timed_region(graph.replay, a.steps // chunk, world, device)
    ms_per_step = elapsed * 1e3 / a.steps
    if rank == 0 and a.dump_outputs:     # the last timed step is step chunk - 1 of the graph's last replay
        last = sets[(chunk - 1) % nsets]
        dump_outputs(a.dump_outputs, {"output": last["out"], "grad_value": last["gv"], "grad_sampling_loc": last["gl"],
                                      "grad_attn_weight": last["ga"]})
    line = headline_line(a, n_gpus, dist.get_world_size() if world > 1 else 1, ms_per_step, S, nsets, input_bytes,
                         "nccl (RCCL)")
    line["timing"] = ("one timed region of %d steps (a hipGraph of %d fwd+bwd steps replayed %d x), bracketed by barrier + "
                      "synchronize, maximum over ranks; ms_per_step = region / steps" % (a.steps, chunk, a.steps // chunk))
    line["rank_cpu_affinity"] = affinity      # rank 0's share of the host cores (None at one GPU: nothing pinned)
    if not a.full:
        if rank == 0:
            print(json.dumps(line), flush=True)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    # ---- --full: the same region timed `repeats` more times -- at --steps 20 one region is a single 0.6-ms graph replay,
    # too thin a sample to read much into; the median and min / p10 / p90 of the repeats ride along
    region_s = sorted(timed_region(graph.replay, a.steps // chunk, world, device) for _ in range(a.repeats))
    line["repeats"] = a.repeats
    line["timed_region_s"] = sum(region_s)
    line["ms_per_step_median_of_repeats"] = region_s[len(region_s) // 2] * 1e3 / a.steps
    line["ms_per_step_min_p10_p90"] = [region_s[0] * 1e3 / a.steps, region_s[int(0.1 * (len(region_s) - 1) + 0.5)] * 1e3 / a.steps,
                                       region_s[int(0.9 * (len(region_s) - 1) + 0.5)] * 1e3 / a.steps]
    line["channels_last_trunk"] = channels_last
    line["conv_search"] = conv_search           # MIOpen's algorithms by measurement, from the recorded find-db (tuning/miopen_userdb)

    # ---- model-level leg: SeqFormer-R50 T=5 360p training step under DDP (all ranks) ----------
    model_leg = None
    if not a.no_model:
        model_leg = model_step_leg(rank, local_rank, world, device, a.model_steps, count=True)
        if model_leg is not None and world == 1:
            one = model_step_leg(rank, local_rank, world, device, a.model_steps, clips_per_rank=1)
            model_leg["one_clip_per_rank"] = {k: one[k] for k in ("clips_per_s", "ms_per_step")}
            amp = model_step_leg(rank, local_rank, world, device, a.model_steps, bf16=True)
            plain = model_step_leg(rank, local_rank, world, device, a.model_steps, tuned_gemms=False)
            model_leg["library_default_gemms"] = {**{k: plain[k] for k in ("clips_per_s", "ms_per_step")},
                                                  "note": "the same step with TunableOp off: rocBLAS / hipBLASLt default heuristic"}
            from vnext_amd import tuning
            tuning.enable()
            model_leg["bf16_autocast"] = {**{k: amp[k] for k in ("clips_per_s", "ms_per_step")},
                                          "note": "same step under torch.autocast(bfloat16): bf16 GEMMs and op value, fp32 "
                                                  "locations / losses; the reference trains in fp32, so this is not the headline"}

    if rank == 0:
        if model_leg is not None:
            line["model_step"] = model_leg
            # the second half of BASELINE.json's metric ("clips/s at 1/2/4/8 GPU") and what bounds its scaling, as
            # top-level keys (details stay in `model_step`): whole-job clips/s of the SeqFormer-R50 training step at
            # this N, and the part of the RCCL gradient all-reduce no overlap with the backward can hide
            line["clips_per_s"] = model_leg["clips_per_s"]
            line["clips_per_s_config"] = "SeqFormer-R50 T=5 360p training step, %d clips per GPU, fp32, DDP over RCCL" % model_leg["clips_per_rank"]
            comm = model_leg.get("ddp_comm")
            line["exposed_allreduce_ms"] = comm.get("exposed_allreduce_ms") if isinstance(comm, dict) else None
            if world == 1:
                line["other_configs"] = extra_model_legs(device)
                # (the graph-replayed form of the bf16 step: a child process, graph_leg)
                model_leg["bf16_autocast"]["graphed_trunk"] = {
                    **graph_leg("seqformer_360p_bf16", a.model_steps),
                    "note": "the bf16 step with its trunk (backbone, transformer, heads; forward and backward) replayed from hipGraphs: "
                            "the bf16 kernels are short enough for the host's ~3 400 launches to bound the eager step"}
        # ---- per-kernel rooflines, measured live --------------------------------------------
        # `us_per_launch` (what `achieved` and `frac` are computed from): HIP events on the launch stream
        # around a hipGraph of back-to-back launches over the rotating (cold) input sets -- the figure the
        # committed rocprofv3 --kernel-trace --stats average of this same command agrees with (it includes
        # the ~1 us between dependent launches, so it never flatters the kernel).
        # `frac_kernel_span`: the same launches timed from inside (first wave start -> last wave end,
        # s_memrealtime stamps), a secondary figure.
        import ctypes
        inner = max(nsets, 24)
        L = op.lib
        # event-timed graphs: plain launches (no stamp argument) -- what rocprofv3 traces in tools/prof_bench.sh
        g_fwd = capture([(lambda s=sets[i % nsets]: op.fwd(s, B, Lq)) for i in range(inner)])
        g_bwd = capture([(lambda s=sets[i % nsets]: op.bwd(s, B, Lq)) for i in range(inner)])
        us_fwd_warm, g_fwd_warm = None, None
        if not a.no_warm:     # same launches on ONE input set: value / locations stay in L2 + Infinity Cache
            g_fwd_warm = capture([(lambda: op.fwd(sets[0], B, Lq)) for _ in range(inner)])
        us_fwd = event_time_us(g_fwd, inner)
        us_bwd = event_time_us(g_bwd, inner)
        if g_fwd_warm is not None:
            us_fwd_warm = event_time_us(g_fwd_warm, inner)
        # the same launches once more with a stamp region each (every workgroup stores its start and its last
        # wave's end: ~0.5-1 us of extra work per launch, which is why the event-timed graphs above are separate)
        n_regions = n_cold = 0
        max_regions = 6 * inner + 96
        kinds = (ctypes.c_int * max_regions)()
        offs = (ctypes.c_longlong * max_regions)()
        nblk = (ctypes.c_longlong * max_regions)()
        if not a.no_spans:
            # the stamp buffer is process-wide state, which the product library does not have: these replays (and only
            # these) go through the development build of the same sources (libvnext_hip_dev.so, variant 0 = automatic)
            DL = op._lib.dev_lib()
            op_dev = Op(device)
            op_dev.lib = DL
            n_words = (6 * inner + 96) * 2 * 8192    # <= 8 Ki workgroups per stamped launch
            stamps = torch.zeros(n_words, dtype=torch.int64, device=device)
            DL.vnx_debug_arm_stamps(stamps.data_ptr(), n_words)
            g_fwd = capture([(lambda s=sets[i % nsets]: op_dev.fwd(s, B, Lq)) for i in range(inner)])
            g_bwd = capture([(lambda s=sets[i % nsets]: op_dev.bwd(s, B, Lq)) for i in range(inner)])
            n_cold = DL.vnx_debug_stamp_regions(kinds, offs, nblk, max_regions)
            if not a.no_warm:
                g_fwd_warm = capture([(lambda: op_dev.fwd(sets[0], B, Lq)) for _ in range(inner)])
            n_regions = DL.vnx_debug_stamp_regions(kinds, offs, nblk, max_regions)
            DL.vnx_debug_arm_stamps(None, 0)
        khz = L.vnx_debug_wall_clock_khz()
        span = {1: [], 2: [], 3: [], 4: [], "warm": []}
        if khz > 0 and 0 < n_regions <= max_regions:
            for _ in range(10):
                stamps.zero_()
                g_fwd.replay()
                g_bwd.replay()
                if g_fwd_warm is not None:
                    g_fwd_warm.replay()
                torch.cuda.synchronize()
                for i in range(n_regions):
                    t = stamps[offs[i]:offs[i] + 2 * nblk[i]].view(-1, 2)
                    ran = t[:, 0] > 0                   # placeholder workgroups that returned at once still stamp
                    if bool(ran.any()) and (i >= n_cold or kinds[i] in span):
                        span["warm" if i >= n_cold else kinds[i]].append(float(t[ran, 1].max() - t[ran, 0].min()) / khz * 1e3)
        k_us = {k: (sum(v) / len(v) if v else None) for k, v in span.items()}

        def roof(nbytes, us_events, us_span, what):
            gbs = nbytes / us_events / 1e3
            r = {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                 "traffic": None, "kernel": what, "algorithmic_bytes_per_launch": nbytes, "us_per_launch": us_events,
                 "timing": "HIP events on the launch stream around hipGraphs of back-to-back launches on rotating inputs (cold): "
                           "(three replays - one replay) / (2 x launches), i.e. launch-to-launch time INCLUDING the gap between "
                           "consecutive launches; the rocprofv3 --kernel-trace average of this command (profiles/, attached as "
                           "rocprofv3_kernel_avg_us) counts the kernel alone and has come out 4 % above (round 5, a traced run on "
                           "another box) to 13 % below (round 6, the backward) this figure; us_kernel_span = first workgroup's start "
                           "to last workgroup's end by in-kernel stamps"}
            if us_span:
                r["us_kernel_span"] = us_span
                r["frac_kernel_span"] = nbytes / us_span / 1e3 / HBM_PEAK_GBS
            return r

        line["roofline"] = roof(bytes_fwd, us_fwd, k_us[1], "msda_fwd_d32_kernel (ms_deform_attn_forward)")
        if us_fwd_warm:
            line["roofline"]["warm_us_per_launch"] = us_fwd_warm
            line["roofline"]["warm_frac"] = bytes_fwd / us_fwd_warm / 1e3 / HBM_PEAK_GBS
            line["roofline"]["warm_note"] = "one input set replayed: value and locations stay in L2 / Infinity Cache; not an HBM fraction"
        line["roofline_bwd"] = roof(bytes_bwd, us_bwd, k_us[4],
                                    "msda_bwd_pair_kernel: one launch per ms_deform_attn_backward call, its workgroups either "
                                    "grad_value units (from the op's inputs) or eight grad_loc / grad_attn waves")
        line["roofline_bwd"]["alone_vs_in_step"] = (
            "us_per_launch is the backward replayed back to back (backward behind backward).  The unit split the launcher takes "
            "for this call -- the small levels cut in two, 815 workgroups for 768 resident -- was chosen on ms_per_step (backward "
            "behind forward: 24.8 against 25.7 us per step, the product library built both ways on one box); in backward-only "
            "sequences it is the slower split (23.4 against 21.2 us by these events; rocprofv3 18.6 against 18.5).  "
            "step_us_minus_forward_us = ms_per_step - the forward's us_per_launch: the backward's share of a step")
        line["roofline_bwd"]["step_us_minus_forward_us"] = line["ms_per_step"] * 1e3 - us_fwd
        if k_us[2]:
            line["roofline_bwd"]["us_grad_loc_kernel_span"] = k_us[2]
        if k_us[3]:
            line["roofline_bwd"]["us_grad_value_kernel_span"] = k_us[3]
        # the ceiling of this access pattern on this memory system, measured in the same run
        ceil = gather_ceiling(device)
        line["roofline"]["gather_ceiling_GBs"] = ceil["cold_384MiB"]["GBs"]
        line["roofline"]["gather_ceiling"] = ceil
        line["roofline"]["frac_of_gather_ceiling"] = line["roofline"]["achieved"] / ceil["cold_384MiB"]["GBs"]
        # what a cold launch of this size cannot beat: one memory latency before the first row arrives + its algorithmic
        # bytes at the gather rate measured above
        lat_us = 2.0
        floor_us = lat_us + bytes_fwd / ceil["cold_384MiB"]["GBs"] / 1e3
        line["roofline"]["floor_us"] = floor_us
        line["roofline"]["floor_frac"] = bytes_fwd / floor_us / 1e3 / HBM_PEAK_GBS
        line["roofline"]["floor_note"] = ("%.1f us of memory latency + algorithmic bytes / the row-gather rate of this run "
                                          "(%.0f GB/s): the ceiling for a cold call of this size, as a fraction of HBM peak "
                                          "= floor_frac" % (lat_us, ceil["cold_384MiB"]["GBs"]))
        # HBM bytes per launch cannot be counted from inside this process: they come from the committed
        # rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this same command (profiles/rNN_bench_pmc_hbm.json,
        # corrected as MI355X_MICROARCH.md section HBM says); the rocprofv3 kernel averages ride along
        pmc = latest_profile("bench_pmc_hbm.json")
        if pmc is not None and (B, Lq, res, a.dist) == (5, 300, "360p", "U"):
            for key, names in (("roofline", ["msda_fwd_d32_kernel"]),
                               ("roofline_bwd", ["msda_bwd_pair_kernel", "msda_bwd_d32_kernel", "msda_bwd_gv_rec_kernel", "msda_bwd_gv_sel_kernel",
                                                 "msda_bwd_gv_direct_kernel"])):
                vals = [v.get("hbm_bytes_per_launch_corrected") for k, v in pmc["data"].items() if any(n in k for n in names)]
                if vals and all(v is not None for v in vals):
                    line[key]["traffic"] = sum(vals)
                    line[key]["traffic_source"] = pmc["file"]
        prof = latest_profile("bench_kernel_avg_us.json")
        if prof is not None:
            line["rocprofv3_kernel_avg_us"] = {"source": prof["file"], **prof["data"]}
        line["fwd_gpoints_per_s"] = points / us_fwd / 1e3
        if not a.no_cases and world == 1:
            line["op_cases"] = op_case_rooflines(op, device)
            # the same floor as `roofline.floor_us` for the other decoder-shape forwards (B = 10 is the reference's
            # per-GPU batch: two clips x five frames): one memory latency + the case's bytes at this run's gather rate
            for key, c in line["op_cases"].items():
                if key.startswith("decoder_") and c["value_dtype"] == "f32":
                    fl = lat_us + c["fwd"]["nominal_bytes"] / ceil["cold_384MiB"]["GBs"] / 1e3
                    c["fwd"]["floor_us"] = fl
                    c["fwd"]["floor_frac"] = c["fwd"]["nominal_bytes"] / fl / 1e3 / HBM_PEAK_GBS
            line.update({"roofline_" + k: v for k, v in head_rooflines(device).items()})
        if not a.no_cpu and world == 1:     # the CPU leg runs at N = 1 only
            line["cpu_baseline"] = cpu_baseline(B, Lq, res)
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
