"""Clip-level data parallelism for the hot path (e).

The reference wraps the model in DistributedDataParallel(broadcast_buffers=False,
find_unused_parameters=True) (detectron2/engine/defaults.py:60-79,380), launches one process
per GPU with the NCCL backend (detectron2/engine/launch.py:27-126) and runs
`SimpleTrainer.run_step` (detectron2/engine/train_loop.py:258-294): loss dict -> sum ->
backward (bucketed gradient all-reduce overlapped with it) -> optimizer step; the optimizer is
AdamW with a 0.1 multiplier on the backbone and full-model gradient-norm clipping at 0.01
(projects/SeqFormer/train_net.py:85-119).

Here: the same step on RCCL (backend "nccl" on ROCm) with the host-side stalls removed --
static graph instead of the unused-parameter walk, gradients as bucket views, no per-step
`.item()` / gloo gather of the loss dict (train_loop.py:296-345) -- and synthetic clips made
on the device, one shard of clips per rank (rank r takes clips r, r+W, ...:
TrainingSampler semantics, projects/SeqFormer/seqformer/data/build.py:18-32).
"""
from __future__ import annotations

import os

import torch
import torch.distributed as dist
from torch.nn.parallel import DistributedDataParallel


def init_distributed(backend: str | None = None):
    """One process per GPU; reads RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the env."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not dist.is_initialized():
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        kw = {}
        if backend == "nccl":
            torch.cuda.set_device(local_rank)
            kw["device_id"] = torch.device("cuda", local_rank)
        dist.init_process_group(backend, **kw)
    return rank, local_rank, world


def shard_indices(num_items: int, rank: int, world: int):
    """Indices of this rank's clips: r, r+W, r+2W, ..."""
    return list(range(rank, num_items, world))


def synthetic_clips(num_clips: int, num_frames: int, height: int, width: int, device, seed: int = 0,
                    num_instances: int = 3, num_classes: int = 40):
    """Random frames plus `num_instances` synthetic tracks per clip in the dataset mapper's layout
    (per frame: gt_classes, gt_boxes xyxy pixels, gt_masks, gt_ids, image_size): a rectangle that
    drifts from frame to frame, its mask the filled rectangle."""
    g = torch.Generator(device=device).manual_seed(seed)
    clips = []
    for _ in range(num_clips):
        frames = [torch.rand(3, height, width, device=device, generator=g) * 255.0 for _ in range(num_frames)]
        clip = {"image": frames, "height": height, "width": width}
        if num_instances > 0:
            n = num_instances
            ctr = 0.25 + 0.5 * torch.rand(n, 2, device=device, generator=g)
            size = 0.1 + 0.25 * torch.rand(n, 2, device=device, generator=g)
            cls = torch.randint(0, num_classes, (n,), device=device, generator=g)
            wh = torch.tensor([width, height], device=device, dtype=torch.float32)
            ys = torch.arange(height, device=device)[None, :, None]
            xs = torch.arange(width, device=device)[None, None, :]
            inst = []
            for t in range(num_frames):
                c = (ctr + 0.02 * t).clamp(0.05, 0.95)
                lo, hi = ((c - size / 2).clamp(0, 1) * wh), ((c + size / 2).clamp(0, 1) * wh)
                masks = (xs >= lo[:, 0, None, None]) & (xs < hi[:, 0, None, None]) & \
                        (ys >= lo[:, 1, None, None]) & (ys < hi[:, 1, None, None])
                inst.append({"gt_classes": cls, "gt_boxes": torch.cat([lo, hi], 1), "gt_masks": masks,
                             "gt_ids": torch.arange(n, device=device), "image_size": (height, width)})
            clip["instances"] = inst
        clips.append(clip)
    return clips


# Gradient buckets.  xGMI is point to point (7 links x ~153 GB/s per GPU): a ring all-reduce of b bytes over 8 GPUs
# moves 2 * 7/8 * b over every link, ~11.4 us per MB, on top of ~30 us of launch + synchronisation per collective.
# SeqFormer-R50 has 188 MB of fp32 gradients per step and ~45 ms of backward to hide them under: 48 MB buckets =
# 4 collectives of ~0.55 ms each (DDP's default 25 MB would make 8; the FIRST bucket also closes later with larger
# buckets, but only the LAST one is exposed, and its size is what remains after the others -- the head's ~20 MB).
# VNX_DDP_BUCKET_MB overrides it for sweeps on hardware.
DEFAULT_BUCKET_MB = 48


def ddp_bucket_mb() -> int:
    return int(os.environ.get("VNX_DDP_BUCKET_MB", DEFAULT_BUCKET_MB))


class CommTimer:
    """DDP communication hook that times the gradient all-reduces: every bucket's span (hook call -> collective done,
    device events on GPU, wall clock on CPU) and the part of the communication nothing can hide -- from the moment the
    LAST bucket is ready (the backward has no gradient left to compute) to the end of the last all-reduce.
    `report()` after a synchronisation -> {"buckets", "allreduce_ms_sum", "exposed_allreduce_ms"} of the last step."""

    def __init__(self, process_group=None):
        self.group = process_group
        self.spans = []          # [(start, end)] of the current step: events or floats
        self._last = None

    def begin_step(self):
        self.spans = []

    def hook(self, state, bucket):
        import time
        buf = bucket.buffer()
        group = self.group if self.group is not None else dist.group.WORLD
        world = dist.get_world_size(group)
        on_gpu = buf.is_cuda
        if on_gpu:
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
        else:
            start, end = [time.perf_counter()], [None]
        buf.div_(world)
        fut = dist.all_reduce(buf, group=group, async_op=True).get_future()
        span = (start, end)
        self.spans.append(span)

        def done(f):
            if on_gpu:
                end.record()          # the future's callback runs ordered after the collective on its stream
            else:
                end[0] = time.perf_counter()
            return f.value()[0]
        return fut.then(done)

    def report(self):
        if not self.spans:
            return None
        first = self.spans[0][0]
        if isinstance(first, list):
            sums = sum((e[0] - s[0]) * 1e3 for s, e in self.spans if e[0] is not None)
            exposed = (self.spans[-1][1][0] - self.spans[-1][0][0]) * 1e3 if self.spans[-1][1][0] is not None else None
        else:
            sums = sum(s.elapsed_time(e) for s, e in self.spans)
            exposed = self.spans[-1][0].elapsed_time(self.spans[-1][1])
        return {"buckets": len(self.spans), "allreduce_ms_sum": round(sums, 3),
                "exposed_allreduce_ms": None if exposed is None else round(exposed, 3)}


def wrap_ddp(model, local_rank: int | None = None, bucket_cap_mb: int | None = None, comm_timer: CommTimer | None = None):
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return model
    on_gpu = next(model.parameters()).is_cuda
    ddp = DistributedDataParallel(
        model, device_ids=[local_rank] if on_gpu else None, broadcast_buffers=False,
        find_unused_parameters=False, static_graph=True, gradient_as_bucket_view=True,
        bucket_cap_mb=bucket_cap_mb if bucket_cap_mb is not None else ddp_bucket_mb())
    if comm_timer is not None:
        ddp.register_comm_hook(None, comm_timer.hook)
    return ddp


def set_rank_affinity(local_rank: int, local_world: int):
    """Pin this rank's host threads to the cores next to its GPU: the cores of the GPU's NUMA node (sysfs, through the
    device's PCI address), divided among the ranks whose GPUs share that node; all cores divided evenly when the
    topology cannot be read.  8 Python processes each issuing ~3 600 launches per step on one host are the first
    thing that bites at 8 GPUs (the reference leaves placement to the OS: detectron2/engine/launch.py:67-80).
    -> {"numa_node", "cpus"} for the bench line, or None when the platform has no sched_setaffinity."""
    if not hasattr(os, "sched_setaffinity"):
        return None
    allowed = sorted(os.sched_getaffinity(0))

    def node_of(idx):
        try:
            p = torch.cuda.get_device_properties(idx)
            bdf = f"{getattr(p, 'pci_domain_id', 0):04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}.0"
            with open(f"/sys/bus/pci/devices/{bdf}/numa_node") as f:
                return int(f.read().strip())
        except Exception:
            return -1

    def cpus_of(node):
        try:
            with open(f"/sys/devices/system/node/node{node}/cpulist") as f:
                out = []
                for part in f.read().strip().split(","):
                    lo, _, hi = part.partition("-")
                    out.extend(range(int(lo), int(hi or lo) + 1))
                return [c for c in out if c in allowed]
        except Exception:
            return []

    # one layout for all ranks: the NUMA pools only when EVERY rank's GPU and its node's cores can be read.  A rank
    # that fell back to the even split while another took its whole node overlapped it (a host that shows this process
    # fewer GPUs than ranks: tests/test_model_ddp.py::test_rank_affinity_partitions_the_allowed_cores).
    nodes = [node_of(r) for r in range(local_world)] if torch.cuda.is_available() else [-1]
    pools = {nd: cpus_of(nd) for nd in set(nodes) if nd >= 0}
    pool, node, share, slot = allowed, -1, local_world, local_rank
    if min(nodes) >= 0 and all(pools.values()) and local_rank < len(nodes):
        node = nodes[local_rank]
        mates = [r for r in range(local_world) if nodes[r] == node]
        pool, share, slot = pools[node], len(mates), mates.index(local_rank)
    per = max(1, len(pool) // max(1, share))
    mine = pool[slot * per:(slot + 1) * per] or pool
    try:
        os.sched_setaffinity(0, mine)
        torch.set_num_threads(max(1, min(len(mine), 16)))
    except OSError:
        return None
    return {"numa_node": node, "cpus": len(mine)}


def enable_tuned_gemms(path=None):
    """The rocBLAS / hipBLASLt solutions recorded offline for the models' GEMM shapes on MI355X (vnext_amd/tuning):
    SeqFormer-R50 training step 76.5 -> 66.6 ms.  Call once per process before training / inference; a no-op (with the
    reason in the returned dict) on other stacks."""
    from . import tuning
    return tuning.enable(path)


def enable_conv_search(db_dir=None) -> dict:
    """MIOpen's convolution algorithms by measurement instead of by heuristic, answered from the find-db recorded on MI355X
    (vnext_amd/tuning: `enable_conv_search`; SeqFormer-R50 step 59.0 -> 55.4 ms fp32, 54.0 -> 46.0 ms bf16).  Like
    `enable_channels_last`: once per process, BEFORE its first convolution."""
    from . import tuning
    return tuning.enable_conv_search(db_dir)


def enable_channels_last() -> dict:
    """Opt in to the channels-last ResNet trunk for TRAINING steps (vnext_amd/models/resnet.py: MIOpen's fp32 backward
    convolutions are NHWC kernels either way; given NCHW tensors it transposes around each: SeqFormer step 66.2 -> 64.3 ms).
    Two process-wide settings, which is why this is an explicit call and not an import side effect:
      * PYTORCH_MIOPEN_SUGGEST_NHWC=1 -- PyTorch hands MIOpen an NHWC problem only with it, and reads it ONCE: call this
        before the process runs its first convolution (a later call still flips the trunk's switch, but PyTorch has read
        the variable by then and the inputs are converted for nothing -- this function cannot see that; it is the caller's
        ordering to keep);
      * the trunk's switch `models.resnet.CHANNELS_LAST`.
    VNX_CHANNELS_LAST=0 or an explicit PYTORCH_MIOPEN_SUGGEST_NHWC=0 opt out.  -> {"enabled", "why"} for the bench line."""
    from .models import resnet
    if os.environ.get("VNX_CHANNELS_LAST", "1") == "0":
        return {"enabled": False, "why": "VNX_CHANNELS_LAST=0"}
    if not torch.cuda.is_available():
        return {"enabled": False, "why": "no GPU"}
    if os.environ.get("PYTORCH_MIOPEN_SUGGEST_NHWC", "1") != "1":
        return {"enabled": False, "why": "PYTORCH_MIOPEN_SUGGEST_NHWC is set to something else"}
    os.environ["PYTORCH_MIOPEN_SUGGEST_NHWC"] = "1"
    resnet.CHANNELS_LAST = True
    return {"enabled": True, "why": "PYTORCH_MIOPEN_SUGGEST_NHWC=1 set before the first convolution; training trunk in channels-last"}


def capture_training_graphs(model, clips, autocast_dtype=None) -> dict:
    """Opt in to the graph-replayed training trunk (`SeqFormer.graph_training` / `IDOL.graph_training`: backbone, transformer
    and heads -- forward AND backward -- as two hipGraphs per input shape) and capture it NOW, on `clips`: one forward +
    backward whose gradients are dropped.  For fixed-size inputs only (every new frame size is a new capture and a new static
    memory pool; Detectron2's multi-scale augmentation wants the eager trunk).

    Call it BEFORE `wrap_ddp`: captured inside DistributedDataParallel.forward, `torch.cuda.make_graphed_callables` dies in
    hipStreamEndCapture on this stack (round 6, one-rank RCCL group: segmentation fault; with the process group alone it
    captures fine).  Captured first, the replayed backward hands the trunk's gradients to the parameters' accumulators like any
    autograd node and DDP's bucket hooks fire there (tests/test_model_ddp.py) -- all of the trunk's buckets when the replayed
    backward returns, i.e. the all-reduce no longer overlaps the trunk's backward.

    What it buys is the host's time, and only where the host is the bound (MI355X, one GPU, the eager figure taken BEFORE the
    capture: a captured graph's private memory pool slows the eager steps that follow it by ~5 ms, which is how a first A/B
    of this misread the fp32 legs): IDOL 720p pair bf16 57.7 -> 49.6 ms, SeqFormer 720p clip bf16 68.9 -> 65.5, two 360p clips
    bf16 ~54 -> ~51; the fp32 SeqFormer steps are bound by their kernels and a replay of ~2 800 graph nodes is SLOWER than
    launching them (59.2 -> 62.5 ms, 720p 92.6 -> 95.5).  So: opt-in, for bf16 / small-batch steps.
    -> {"enabled", "why"} for the bench line."""
    if not hasattr(model, "graph_training"):
        return {"enabled": False, "why": "%s has no graph_training switch" % type(model).__name__}
    from .models.swin import SwinTransformer
    if any(isinstance(m, SwinTransformer) for m in model.modules()):
        # stochastic depth draws a fresh mask per step, which a replayed graph would freeze; not built
        raise NotImplementedError("capture_training_graphs: the Swin backbone trains eagerly (graph capture of its "
                                  "training trunk is not built)")
    if not torch.cuda.is_available() or not next(model.parameters()).is_cuda:
        return {"enabled": False, "why": "no GPU"}
    if dist.is_available() and dist.is_initialized() and isinstance(model, DistributedDataParallel):
        raise ValueError("capture_training_graphs: pass the bare model, before wrap_ddp")
    model.graph_training = True
    was_training = model.training
    model.train()
    with torch.autocast("cuda", dtype=autocast_dtype or torch.bfloat16, enabled=autocast_dtype is not None):
        losses = sum(model(clips).values())
    losses.backward()
    model.zero_grad(set_to_none=True)
    model.train(was_training)
    torch.cuda.synchronize()
    return {"enabled": True, "why": "training trunk captured (forward + backward hipGraphs) for %d input shape(s)"
                                    % len(getattr(model, "_train_trunks", {}))}


def release_training_graphs(model) -> None:
    """Back to the eager trunk, the captured graphs destroyed NOW (they sit in a reference cycle with the model: `del` alone leaves
    them to the collector).  While a captured training graph is alive, every EAGER step of the process is slower -- 58.6 -> 64.6
    ms on the SeqFormer step, back to 59.1 once the graphs are gone (MI355X, round 6) -- so a process that measures or runs
    both forms releases the graphs in between."""
    import gc
    if hasattr(model, "graph_training"):
        model.graph_training = False
    getattr(model, "_train_trunks", {}).clear()
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def enable_device_matching(model, on: bool = True) -> None:
    """Opt in to matching on the device (`SeqFormer.device_matching` / `IDOL.device_matching`).
    SeqFormer: Hungarian matching, cost and assignment of every (decoder layer, clip) in one kernel, the indices never
    leave the device -- `losses` then runs from `prepare_targets` to the loss dict without a device-to-host copy or a
    blocking upload.  The same pairs as the host matcher wherever the optimum is unique beyond fp32 rounding of the cost.
    IDOL: simOTA matching of every (decoder layer, key image) and the positive / negative sets of every reference image
    in one kernel; its compact result crosses to the host in one copy (the counts are needed there: the mask head's rows,
    `rng.sample`), so one synchronisation stays and the host arithmetic goes.  The same indices as the host matcher
    wherever no comparison is decided by fp32 rounding of the cost.  Raises for a model without the switch."""
    if not hasattr(model, "device_matching"):
        raise ValueError("enable_device_matching: %s has no device_matching switch" % type(model).__name__)
    model.device_matching = bool(on)


def enable_device_selection(model, on: bool = True) -> None:
    """Opt in to candidate selection on the device (`IDOL.device_selection`, vnext_amd/ops/det_select.py): the per-frame
    score threshold and class-aware box NMS of video inference by one kernel for the whole chunk, instead of a host copy
    of [F, Q, 6] floats and a NumPy loop per frame.  Only the picked indices cross to the host -- one copy, which is the
    one synchronisation that stays (the counts size the mask head's rows).  The same picks as the host loop wherever no
    comparison is decided by fp32 rounding of a sigmoid at the threshold; a shape the kernel refuses takes the host loop.
    The COCO pre-training branch (`IDOL.coco_inference`) uses the op whenever its tensors are CUDA, without this switch.
    Raises for a model without the switch."""
    if not hasattr(model, "device_selection"):
        raise ValueError("enable_device_selection: %s has no device_selection switch" % type(model).__name__)
    model.device_selection = bool(on)


def enable_device_clip_matching(model, on: bool = True) -> None:
    """Opt in to clip matching on the device (`SeqFormer.device_clip_matching`, vnext_amd/ops/clip_link.py): with
    `MODEL.SEQFORMER.CLIP_MATCHING` the clips of a long video are linked into tracks by three launches per clip on a state
    that stays in device memory -- mask sIoU against the stored clips, the assignment, new tracks, the running sums -- instead
    of a loop of small launches, two copies to the host and a scipy call per clip; the host no longer waits for the device
    between clips.  The same tracks as the host path wherever no assignment is decided by fp32 rounding of a score; a
    video beyond the kernels' limits (instances or frames of a clip, tracks of a video) is redone on the host path.
    Raises for a model without the switch (IDOL tracks frame by frame: `DeviceTracker`)."""
    if not hasattr(model, "device_clip_matching"):
        raise ValueError("enable_device_clip_matching: %s has no device_clip_matching switch" % type(model).__name__)
    model.device_clip_matching = bool(on)


def enable_device_ingest(model, on: bool = True) -> None:
    """Opt in to ingesting uint8 frames on the device (`SeqFormer.device_ingest` / `IDOL.device_ingest`,
    vnext_amd/ops/ingest.py): the mappers' uint8 CHW frames cross the bus as bytes in one pinned, non-blocking copy (not as
    floats, frame by frame, pageable), one kernel normalises, pads and writes the padding mask, and one more writes every
    pyramid level's padding mask and sine position -- instead of a cast, a subtract, a divide, a slice copy and a mask fill
    per frame and about 20 launches per level.  x and the masks are bit-identical to the eager path's; the positions agree to
    fp32 rounding of the sine's argument, and exactly on rows and columns without a valid pixel.  Float frames take the
    eager path whatever the switch says; the captured training trunks (`graph_training`) are unchanged.  Raises for a model
    without the switch."""
    if not hasattr(model, "device_ingest"):
        raise ValueError("enable_device_ingest: %s has no device_ingest switch" % type(model).__name__)
    model.device_ingest = bool(on)


def enable_device_resize(model, on: bool = True) -> None:
    """Opt in to the test-time resize on the device (`SeqFormer.device_resize` / `IDOL.device_resize`,
    vnext_amd/ops/resize.py): in eval mode, uint8 frames handed to `inference` / `inference_video` / `ytvis_results` at
    their DECODED size are resized to `ResizeShortestEdge(INPUT.MIN_SIZE_TEST, INPUT.MAX_SIZE_TEST)`'s target by the kernel
    that also normalises, pads and masks them -- byte for byte what Pillow's bilinear resize on the host gives, so the
    network sees the inputs it would have seen after the reference's test-time augmentation.  The input dict's optional
    "image_layout" ("chw", the default, or "hwc") names the frames' layout; "height" / "width" default to the source frame's
    size.  A video whose frames are already at their target takes the path it takes without the switch; float frames and
    training are unchanged.  Raises for a model without the switch."""
    if not hasattr(model, "device_resize"):
        raise ValueError("enable_device_resize: %s has no device_resize switch" % type(model).__name__)
    model.device_resize = bool(on)


def enable_device_masks(model, on: bool = True) -> None:
    """Opt in to dense result masks from the logits in one device pass (`SeqFormer.device_masks` / `IDOL.device_masks`,
    vnext_amd/ops/mask_dense.py): in eval mode the full-resolution masks `model(inputs)` returns -- SeqFormer's reported
    pairs, IDOL's tracks, and the `pred_masks` of IDOL's COCO-pretrain branch -- come from one kernel call per video (per
    distinct size pair for COCO) instead of the bilinear -> sigmoid -> crop -> nearest chain and its two full-resolution fp32
    tensors; the video branches then make one device-to-host copy.  Types, shapes and devices of the outputs are unchanged;
    the masks are the chain's wherever no pixel's bilinear value is within fp32 rounding of 0 (the device bit is value > 0,
    as in `ytvis_results`).  SeqFormer pairs of one query share memory.  CPU tensors and the RLE routes are unchanged.
    Raises for a model without the switch."""
    if not hasattr(model, "device_masks"):
        raise ValueError("enable_device_masks: %s has no device_masks switch" % type(model).__name__)
    model.device_masks = bool(on)


def enable_device_augment(model, on: bool = True) -> None:
    """Opt in to the training-time augmentation on the device (`SeqFormer.device_augment` / `IDOL.device_augment`,
    vnext_amd/ops/augment.py): in training mode, clips that `vnext_amd.data.clip_mapper.stage_clip` made -- SOURCE frames as
    decoded bytes, the drawn plan under "augment", ground-truth masks as their COCO run lengths -- are cropped, resized and
    flipped by one kernel that also normalises, pads and masks them (byte for byte Pillow's bilinear resize), and gt_masks,
    gt_boxes and gt_ids of the whole step come from one more call, straight from the run lengths with Pillow's NEAREST
    tables: what the reference's mapper computes with Pillow and numpy per frame and per mask on the host.  Clips without
    "augment", eval mode and the captured training trunks are unchanged; a plan beyond the kernels' range takes the host
    route of the same arithmetic.  Raises for a model without the switch."""
    if not hasattr(model, "device_augment"):
        raise ValueError("enable_device_augment: %s has no device_augment switch" % type(model).__name__)
    model.device_augment = bool(on)


def enable_fused_mask_loss(model, on: bool = True) -> None:
    """Opt in to the fused mask losses (`criterion.fused_mask_loss`, vnext_amd/ops/mask_loss.py): focal + dice of the
    matched instances' mask logits in one kernel pass each way, the ground truth read in place at image resolution --
    no sliced / padded / gathered float copy of it, and nothing of the logits' size kept for the backward.  SeqFormer
    and IDOL alike; same loss names and per-layer arithmetic, the sums reassociated.  CUDA only: with the switch on, a
    criterion given CPU tensors raises.  Raises for an object whose criterion has no such switch."""
    criterion = getattr(model, "criterion", None)
    if criterion is None or not hasattr(criterion, "fused_mask_loss"):
        raise ValueError("enable_fused_mask_loss: %s has no criterion with a fused_mask_loss switch" % type(model).__name__)
    criterion.fused_mask_loss = bool(on)


def enable_fused_set_loss(model, on: bool = True) -> None:
    """Opt in to the fused class and box losses (`criterion.fused_set_loss`, vnext_amd/ops/set_loss.py): the class focal
    loss over the logits of every decoder layer, the matched boxes' L1 and GIoU losses and (SeqFormer) `class_error` from
    one op -- two launches forward, one backward, no one-hot target, no gathers, nothing of the logits' size kept for the
    backward.  SeqFormer and IDOL alike; same loss names and normalisations, the sums reassociated.  CUDA only: with the
    switch on, a criterion given CPU tensors raises.  Raises for an object whose criterion has no such switch."""
    criterion = getattr(model, "criterion", None)
    if criterion is None or not hasattr(criterion, "fused_set_loss"):
        raise ValueError("enable_fused_set_loss: %s has no criterion with a fused_set_loss switch" % type(model).__name__)
    criterion.fused_set_loss = bool(on)


def enable_fused_reid_loss(model, on: bool = True) -> None:
    """Opt in to the fused reid losses (`criterion.fused_reid_loss`, vnext_amd/ops/reid_loss.py): IDOL's contrastive and
    auxiliary cosine losses of every image of a step from one op -- one packed upload, one launch forward and two backward
    whatever the batch, instead of a per-image loop of small launches.  Same loss names and numbers, the sums
    reassociated; the negatives are still drawn by the host generator.  Taken for CUDA embeddings; on the CPU the per-image
    path runs as before.  Raises for an object whose criterion has no such switch (SeqFormer has no reid losses)."""
    criterion = getattr(model, "criterion", None)
    if criterion is None or not hasattr(criterion, "fused_reid_loss"):
        raise ValueError("enable_fused_reid_loss: %s has no criterion with a fused_reid_loss switch" % type(model).__name__)
    criterion.fused_reid_loss = bool(on)


def enable_bf16_window_attention(model, on: bool = True) -> None:
    """Opt in to the bf16 window-attention core (`WindowAttention.bf16_core`, vnext_amd/ops/window_attention.py) on every
    Swin block of the model: under `torch.autocast(bfloat16)` on CUDA the core reads the bf16 qkv rows as the qkv GEMM
    left them, runs its products on the matrix cores and hands bf16 rows to proj -- no fp32 copy of qkv, no cast back.
    Scores, softmax and accumulators stay fp32.  Without bf16 autocast (fp32 input, fp16 autocast, CPU) the switch
    changes nothing.  Raises for a model without a WindowAttention (the ResNet trunks)."""
    from .models.swin import WindowAttention
    mods = [m for m in model.modules() if isinstance(m, WindowAttention)]
    if not mods:
        raise ValueError("enable_bf16_window_attention: %s has no WindowAttention" % type(model).__name__)
    for m in mods:
        m.bf16_core = bool(on)


def enable_fused_swin_glue(model, on: bool = True) -> None:
    """Opt in to the fused element-wise glue of the Swin stages (`BasicLayer.fused_glue`, `PatchMerging.fused_glue`,
    vnext_amd/ops/swin_glue.py): each residual add, with its stochastic depth, and the LayerNorm that follows it are one
    HIP pass each way -- the first block's norm1 a plain norm, each block's closing residual fused with the next block's
    norm1, the stage's last one a plain scaled add -- and PatchMerging's pad, 2x2 gather and LayerNorm are one pass
    without the padded and concatenated copies.  Under `torch.autocast(bfloat16)` the normalised rows leave as bf16, the
    cast the next Linear would make.  Same modules and state-dict names, the same masks under the same seed, the sums
    reassociated.  On the CPU, under fp16 autocast and for other types or widths the same expression runs through
    torch.  Raises for a model without a Swin backbone (the ResNet trunks)."""
    from .models.swin import BasicLayer, PatchMerging
    mods = [m for m in model.modules() if isinstance(m, (BasicLayer, PatchMerging))]
    if not mods:
        raise ValueError("enable_fused_swin_glue: %s has no Swin stage" % type(model).__name__)
    for m in mods:
        m.fused_glue = bool(on)


def enable_fused_resnet_glue(model, on: bool = True) -> None:
    """Opt in to the fused element-wise glue of the ResNet trunk (`ResNetTrunk.fused_glue`, vnext_amd/ops/resnet_glue.py):
    on CUDA the trunk's convolutions run without a bias and one HIP pass per site adds the folded batch norm's shift,
    applies the ReLU and, at a block's tail, adds the shortcut (with the projection's own shift) -- three launches per
    bottleneck instead of seven or eight; with a frozen stem or without grad, the stem's shift, ReLU and max-pool are one
    pass that writes only the pooled map.  fp32 results are the eager chain's wherever the convolution itself does not
    round its bias differently; under autocast each site rounds once instead of once per step -- except that a 16-bit
    TRAINING step keeps the eager chain at a block's tail (two fused sites per block: results bit-identical to the switch
    off).  Same modules and state-dict names.  CPU tensors and tensors in neither memory format keep the eager chain.  Raises for a model without
    a ResNet trunk (the Swin backbone)."""
    from .models.resnet import ResNetTrunk
    mods = [m for m in model.modules() if isinstance(m, ResNetTrunk)]
    if not mods:
        raise ValueError("enable_fused_resnet_glue: %s has no ResNet trunk" % type(model).__name__)
    for m in mods:
        m.fused_glue = bool(on)


def build_optimizer(model, base_lr=2e-4, backbone_multiplier=0.1, weight_decay=1e-4):
    """AdamW, backbone at base_lr * multiplier (train_net.py:85-113)."""
    backbone, rest = [], []
    for name, p in model.named_parameters():
        if p.requires_grad:
            (backbone if "backbone" in name else rest).append(p)
    on_gpu = bool(rest) and rest[0].is_cuda
    return torch.optim.AdamW([{"params": rest, "lr": base_lr},
                              {"params": backbone, "lr": base_lr * backbone_multiplier}],
                             lr=base_lr, weight_decay=weight_decay,
                             fused=True if on_gpu else None)   # one multi-tensor kernel chain per group


def build_fused_optimizer(model, base_lr=2e-4, backbone_multiplier=0.1, weight_decay=1e-4, clip_max_norm=0.01):
    """Opt in to the clipped AdamW step as one op (vnext_amd/ops/optim.py: `ClippedAdamW`): the two groups of
    `build_optimizer`, with the full-model gradient clipping at `clip_max_norm` inside `step()` -- norm, clip and update in
    three launches instead of the ~44 of clip_grad_norm_ + AdamW.  `train_step` sees `clips_gradients` and does not clip a
    second time.  Same arithmetic in fp32, the sums reassociated; state dicts cross with `build_optimizer`'s in both
    directions.  ONE difference: the gradients are not rescaled in place (after the step `.grad` holds the unclipped values).
    CUDA fp32 parameters only: on the CPU `step()` raises."""
    from .ops.optim import ClippedAdamW
    backbone, rest = [], []
    for name, p in model.named_parameters():
        if p.requires_grad:
            (backbone if "backbone" in name else rest).append(p)
    return ClippedAdamW([{"params": rest, "lr": base_lr},
                         {"params": backbone, "lr": base_lr * backbone_multiplier}],
                        lr=base_lr, weight_decay=weight_decay, max_norm=clip_max_norm)


def train_step(model, optimizer, clips, clip_max_norm: float = 0.01, comm_timer: CommTimer | None = None):
    """SimpleTrainer.run_step without the host synchronisations.  An optimizer that clips inside its step
    (`clips_gradients`: `build_fused_optimizer`) is not clipped here; its own max_norm holds."""
    if comm_timer is not None:
        comm_timer.begin_step()
    loss_dict = model(clips)
    losses = sum(loss_dict.values())
    optimizer.zero_grad(set_to_none=True)
    losses.backward()
    if getattr(optimizer, "clips_gradients", False):
        optimizer.step()
        return losses.detach()
    params = [p for g in optimizer.param_groups for p in g["params"]]
    torch.nn.utils.clip_grad_norm_(params, clip_max_norm)   # full-model clipping, train_net.py:115-119
    optimizer.step()
    return losses.detach()
