"""COCO pre-training pairs on the device, the whole step (vnext_amd/models/frames.py `augment_step` on `augment.ChainPlan`s;
DESIGN section 30): a tiny IDOL with `device_augment` sees bit-identical network inputs and targets to the host route of the
same plans, in the launches the design promises, and the same losses; and the two frame launches, captured in a hipGraph,
replay on other pixels and other plans.  The kernel alone is held to Pillow in tests/test_coco_pair.py.

The file's name sorts behind the tests that capture training trunks for the reason tests/test_train_augment_gpu.py gives: a
capture here must not be the first draw from torch's stream pool.
"""
import random

import numpy as np
import pytest
import torch

import vnext_amd.models  # noqa: F401  (registers the meta-archs)
from test_train_augment_gpu import TINY_IDOL, Spy, flat_targets, padded
from vnext_amd import train as T
from vnext_amd.data import clip_mapper
from vnext_amd.models import frames as frames_mod
from vnext_amd.ops import augment, poly_rle
from vnext_amd.ops.augment import ChainPlan, chain_full
from vnext_amd.registry import build_model, get_idol_cfg

DEV = "cuda:0"
STAR = [30.5, 20.25, 60.0, 31.5, 90.75, 22.0, 75.2, 50.0, 88.0, 80.5, 58.3, 66.6, 33.0, 84.0, 41.9, 52.2]
HOLE = [[100.0, 10.0, 150.0, 10.0, 150.0, 60.0, 100.0, 60.0], [110.0, 20.0, 140.0, 20.0, 140.0, 50.0, 110.0, 50.0]]


def xywh(polys):
    xs = np.concatenate([np.asarray(p)[0::2] for p in polys])
    ys = np.concatenate([np.asarray(p)[1::2] for p in polys])
    return [float(xs.min()), float(ys.min()), float(xs.max() - xs.min()), float(ys.max() - ys.min())]


def pairs(plans, seed):
    """two COCO images (96 x 160 and 80 x 120), each with a star, an object of two polygons, a box at the left edge (which
    a crop of the flipped key frame loses: id -1 there) and a crowd annotation (no slot)"""
    rng = np.random.default_rng(seed)
    out = []
    for c, ((h, w), plan) in enumerate(zip(((96, 160), (80, 120)), plans)):
        image = torch.from_numpy(rng.integers(0, 256, (3, h, w), dtype=np.uint8))
        s = w / 160.0
        scaled = lambda polys: [[v * s for v in p] for p in polys]      # noqa: E731
        annos = [{"category_id": 3 + c, "segmentation": scaled([STAR]), "bbox": xywh(scaled([STAR]))},
                 {"category_id": 9, "iscrowd": 1, "segmentation": scaled([STAR]), "bbox": xywh(scaled([STAR]))},
                 {"category_id": 5, "segmentation": scaled(HOLE), "bbox": xywh(scaled(HOLE))},
                 {"category_id": 7, "segmentation": [[2.0, 60.0 * s, 12.0, 60.0 * s, 12.0, 78.0 * s, 2.0, 78.0 * s]],
                  "bbox": [2.0, 60.0 * s, 10.0, 18.0 * s]}]
        out.append(clip_mapper.stage_coco_pair(image, annos, plan, 40))
    return out


CROPPED = [[ChainPlan(96, 160, True, 120, 200, 30, 10, 140, 100, 64, 90), chain_full(96, 160, 60, 100, False)],
           [ChainPlan(80, 120, False, 60, 90, 5, 4, 80, 50, 70, 112), ChainPlan(80, 120, True, 120, 180, 20, 30, 150, 88, 44, 75)]]
PLAIN = [[chain_full(96, 160, 60, 100, True), chain_full(96, 160, 72, 120, False)],
         [chain_full(80, 120, 64, 96, False), chain_full(80, 120, 48, 72, True)]]


@pytest.fixture(scope="module")
def idol():
    torch.manual_seed(6)
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": DEV, **TINY_IDOL})).train()
    T.enable_device_ingest(model)
    return model, Spy(model)


def step(model, spy, clips, route):
    torch.manual_seed(7)
    random.seed(7)
    np.random.seed(7)
    if route == "device":
        T.enable_device_augment(model)
        try:
            losses = model(clips)
        finally:
            T.enable_device_augment(model, on=False)
    else:
        losses = model(frames_mod.host_augmented(clips))
    torch.cuda.synchronize()
    return spy.take(), {k: v.detach().cpu() for k, v in losses.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cropped", "plain"])
def test_idol_step_on_coco_pairs_equals_the_host_route_bit_for_bit(idol, monkeypatch, name):
    model, spy = idol
    clips = pairs(CROPPED if name == "cropped" else PLAIN, seed=80)
    rasterised = []
    inner = poly_rle.polygons_to_runs
    monkeypatch.setattr(poly_rle, "polygons_to_runs", lambda *a, **k: rasterised.append(1) or inner(*a, **k))
    calls, bytes_calls = dict(augment.CALLS), augment.BYTES_CALLS["resize_window_bytes"]
    (seen_d, targets_d), loss_d = step(model, spy, clips, "device")
    # one launch of each op for the whole step; the first resample only where a frame is resampled twice
    assert augment.CALLS == {k: v + 1 for k, v in calls.items()} and rasterised == [1]
    assert augment.BYTES_CALLS["resize_window_bytes"] == bytes_calls + (1 if name == "cropped" else 0)
    calls, bytes_calls = dict(augment.CALLS), dict(augment.BYTES_CALLS)
    (seen_h, targets_h), loss_h = step(model, spy, clips, "host")
    assert augment.CALLS == calls and augment.BYTES_CALLS == bytes_calls and rasterised == [1]
    assert len(seen_d) == len(seen_h) > 0
    for a, b in zip(seen_d, seen_h):               # x, the level masks and positions
        assert a.dtype == b.dtype and torch.equal(a, b)
    td, th = flat_targets(targets_d), flat_targets(targets_h)
    assert len(td) == len(th) > 0
    for a, b in zip(td, th):                       # labels, boxes, masks, ids
        assert a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())
    assert set(loss_d) == set(loss_h)
    # the filled instance dicts themselves, and x and the padding mask against the host frames
    T.enable_device_augment(model)
    try:
        filled, pre = frames_mod.augment_step(model, clips)
    finally:
        T.enable_device_augment(model, on=False)
    host = frames_mod.host_augmented(clips)
    want = model._preprocess([f for clip in host for f in clip["image"]])
    assert torch.equal(pre[0], want[0]) and torch.equal(pre[1], want[1])
    lost = 0
    for got, ref in zip(filled, host):
        for g, r in zip(got["instances"], ref["instances"]):
            assert g["gt_masks"].is_cuda and g["gt_masks"].dtype == torch.bool and g["gt_ids"].dtype == torch.int64
            assert torch.equal(g["gt_masks"].cpu(), r["gt_masks"]) and torch.equal(g["gt_boxes"].cpu(), r["gt_boxes"])
            assert g["gt_boxes"].dtype == torch.float32 and torch.equal(g["gt_ids"].cpu(), r["gt_ids"])
            assert torch.equal(g["gt_classes"], r["gt_classes"]) and r["gt_ids"].numel() == 3
            lost += int((r["gt_ids"] == -1).sum())
    assert lost >= 1 if name == "cropped" else lost == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cropped", "plain"])
def test_idol_losses_on_coco_pairs_equal_the_host_route_bit_for_bit(idol, name):
    """The losses of the step above, device route against host route, compared exactly -- under torch's deterministic
    switches, because without them the tiny IDOL's losses are not reproducible run to run on ONE route.  Measured on an
    MI355X: the host route three times and the device route twice on the same clips and seeds, as the int32 bits of the fp32
    losses ("cropped"):
        loss_mask      host 1081000718, 1081000707, 1081000725   device 1081000770, 1081000754
        loss_dice      host 1081083451, 1081083450, 1081083454   device 1081083452, 1081083452
        loss_reid_aux  host 1067387186, 1067387184, 1067387186   device 1067387186, 1067387184
    (loss_ce, loss_bbox and loss_giou: the same bits in all five runs) -- the routes differ by no more than a route differs
    from itself, although every network input and target is bit-identical (the test above).  With
    `torch.use_deterministic_algorithms(True)` and `cudnn.deterministic` all five runs give the same bits for every loss of
    both steps (loss_mask 1081000738 five times).  The switches are restored afterwards."""
    model, spy = idol
    clips = pairs(CROPPED if name == "cropped" else PLAIN, seed=80)
    before = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
              torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        _, loss_d = step(model, spy, clips, "device")
        _, loss_h = step(model, spy, clips, "host")
    finally:
        torch.use_deterministic_algorithms(before[0], warn_only=before[1])
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = before[2:]
    assert set(loss_d) == set(loss_h)
    for k in sorted(loss_h):
        print(name, k, "device", loss_d[k].view(torch.int32).item(), "host", loss_h[k].view(torch.int32).item())
    for k in loss_h:
        assert torch.equal(loss_d[k], loss_h[k]), (k, float(loss_d[k]), float(loss_h[k]))


@pytest.mark.gpu
def test_the_two_frame_launches_captured_in_a_graph_replay_on_other_pixels_and_plans():
    """capture `vnx_resize_window_bytes` + `vnx_augment_frames` on static buffers, overwrite pixels and every table in place
    with ANOTHER step of the same padded sizes (another frame resampled twice, other sizes and windows), poison the outputs
    and the slots, replay: the eager result of that step, bit for bit"""
    from vnext_amd import _lib
    lib = _lib.lib()
    sizes = [(45, 70), (40, 40)]

    def host_step(seed, plans):
        g = torch.Generator().manual_seed(seed)
        frames = [torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g) for h, w in sizes]
        s = augment.stage_step(frames, plans, [], "cpu")
        assert s.size == (64, 64) and s.win_size == (64, 64) and s.win_table.shape[0] == 1
        return frames, plans, [s.pixels, s.src_table, s.dst_table, s.coeffs, s.win_table]

    first = host_step(91, [ChainPlan(45, 70, False, 60, 93, 7, 5, 64, 50, 50, 64), chain_full(40, 40, 21, 27, True)])
    second = host_step(92, [chain_full(45, 70, 33, 50, True), ChainPlan(40, 40, True, 64, 64, 3, 1, 60, 63, 64, 40)])
    room = [max(a.numel(), b.numel()) for a, b in zip(first[2], second[2])]
    bufs = [torch.zeros(n, dtype=t.dtype, device=DEV) for n, t in zip(room, first[2])]

    def load(tensors):
        for b, t in zip(bufs, tensors):
            b.fill_(0x77 if b.dtype == torch.uint8 else 0)      # (the slots of the step before are gone)
            b[:t.numel()].copy_(t.reshape(-1))

    x = torch.full((2, 3, 64, 64), float("nan"), device=DEV)
    mask = torch.full((2, 64, 64), 0xFF, dtype=torch.uint8, device=DEV)

    def launches(stream):
        _lib.check(lib.vnx_resize_window_bytes(bufs[0].data_ptr(), bufs[0].numel(), bufs[4].data_ptr(), bufs[3].data_ptr(),
                                               bufs[3].numel(), 1, 64, 64, 0, stream))
        _lib.check(lib.vnx_augment_frames(bufs[0].data_ptr(), bufs[0].numel(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                                          bufs[3].data_ptr(), bufs[3].numel(), 2, 64, 64, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0, 0,
                                          x.data_ptr(), mask.data_ptr(), stream))

    eager = []
    for frames, plans, tensors in (first, second):
        load(tensors)
        launches(_lib.current_stream(x))
        torch.cuda.synchronize()
        eager.append((x.clone(), mask.clone()))
        want, want_mask = padded(augment.reference_chain_frames(frames, plans), (64, 64))
        assert torch.equal(x.cpu(), want) and torch.equal(mask.cpu().bool(), want_mask)
    load(first[2])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches(_lib.current_stream(x))
    for k in (1, 0, 1):
        load((first, second)[k][2])
        x.fill_(float("nan"))
        mask.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(x, eager[k][0]) and torch.equal(mask, eager[k][1]), k
