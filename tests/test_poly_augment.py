"""Polygon ground truth in the device augmentation route: `clip_mapper.stage_clip(polygons=True)`, the coordinate transforms
of `augment.transform_polygons`, `frames.host_augmented` (CPU) and `frames.augment_step` (GPU), which must agree mask for mask."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from vnext_amd.data import clip_mapper
from vnext_amd.models import frames as frames_mod
from vnext_amd.ops import augment
from vnext_amd.ops import poly_rle as P
from vnext_amd.ops.augment import FramePlan
from vnext_amd.utils.ytvis_json import rle_counts

DEV = "cuda:0"
H, W = 96, 160
STAR = [30.5, 20.25, 60.0, 31.5, 90.75, 22.0, 75.2, 50.0, 88.0, 80.5, 58.3, 66.6, 33.0, 84.0, 41.9, 52.2]
HOLE = [[100.0, 10.0, 150.0, 10.0, 150.0, 60.0, 100.0, 60.0], [110.0, 20.0, 140.0, 20.0, 140.0, 50.0, 110.0, 50.0],
        [120.0, 55.0, 158.5, 70.0, 125.0, 90.0]]


def rectangle(y, x, dy, dx):
    m = np.zeros((H, W), dtype=np.uint8)
    m[y:y + dy, x:x + dx] = 1
    return rle_counts(m).tolist()


def clips(plans, seed=0):
    """per clip two frames of 96 x 160 with four instances: a star polygon, an object of three polygons, an RLE rectangle, and
    one present only in the first frame (as a box): the dummy polygon elsewhere; a crowd annotation is dropped"""
    rng = np.random.default_rng(seed)
    out = []
    for c, plan in enumerate(plans):
        frames = [torch.from_numpy(rng.integers(0, 256, (3, H, W), dtype=np.uint8)) for _ in plan]
        annos = []
        for t in range(len(plan)):
            shift = lambda p, d=3.5 * t: [v + d for v in p]                     # noqa: E731
            a = [{"id": 11, "category_id": 3 + c, "segmentation": [shift(STAR)]},
                 {"id": 12, "category_id": 5, "segmentation": [shift(p) for p in HOLE]},
                 {"id": 13, "category_id": 6, "segmentation": rectangle(20 + t, 40, 40, 60)},
                 {"id": 15, "category_id": 8, "iscrowd": 1, "segmentation": [shift(STAR)]}]
            if t == 0:
                a.append({"id": 14, "category_id": 7, "segmentation": [[4.0, 60.0, 10.0, 20.0]]})
            annos.append(a)
        out.append(clip_mapper.stage_clip(frames, annos, plan, 40, polygons=True))
    return out


PLANS = {
    "full": [[augment.full_plan(H, W, 60, 100)] * 2],
    "flipped": [[augment.full_plan(H, W, 60, 100, True), augment.full_plan(H, W, 72, 120, True)]],
    "cropped": [[FramePlan(16, 8, 120, 80, 64, 96, False), FramePlan(20, 12, 128, 80, 70, 112, True)]],
    "two clips": [[FramePlan(10, 0, 140, 88, 88, 140, False)] * 2, [augment.full_plan(H, W, 60, 100, True)] * 2],
}


def test_stage_clip_keeps_polygons_only_on_request():
    plan = PLANS["full"][0]
    clip = clips([plan])[0]
    for t, fr in enumerate(clip["instances"]):
        assert fr["gt_ids"].tolist() == ([11, 12, 13, -1, 14] if t == 0 else [11, 12, 13, -1, -1])
        assert fr["gt_classes"].tolist() == ([3, 5, 6, 40, 7] if t == 0 else [3, 5, 6, 40, 40])
        assert [q is None for q in fr["gt_poly"]] == [False, False, True, False, False]
        assert [c is None for c in fr["gt_rle"]] == [True, True, False, True, True]
        assert fr["gt_poly"][3] == [[0.0] * 6]                                  # the crowd's slot: the reference's dummy
        assert fr["gt_poly"][4] == ([[4.0, 60.0, 10.0, 20.0]] if t == 0 else [[0.0] * 6])
    frames = clip["image"]
    annos = [[{"id": 1, "category_id": 2, "segmentation": [STAR]}]] * 2
    with pytest.raises(ValueError, match="polygons go through frPyObjects to RLE first"):
        clip_mapper.stage_clip(frames, annos, plan, 40)
    rle_only = clip_mapper.stage_clip(frames, [[{"id": 1, "category_id": 2, "segmentation": rectangle(5, 5, 9, 9)}]] * 2, plan, 40)
    assert "gt_poly" not in rle_only["instances"][0]


def expected_mask(segmentation, p):
    """the coordinate transform and the rasterisation, written out"""
    polys = []
    for poly in P.object_polygons(segmentation):
        x, y = poly[0::2].copy(), poly[1::2].copy()
        x, y = x - p.x0, y - p.y0
        x, y = x * (p.nw * 1.0 / p.cw), y * (p.nh * 1.0 / p.ch)
        if p.flip:
            x = p.nw - x
        polys.append(np.stack((x, y), 1).reshape(-1))
    return P.counts_to_mask(P.object_counts_host(polys, p.nh, p.nw), p.nh, p.nw)


@pytest.mark.parametrize("name", list(PLANS))
def test_host_augmented_rasterises_the_transformed_polygons(name):
    staged = clips(PLANS[name])
    out = frames_mod.host_augmented(staged)
    assert len(out) == len(staged)
    filled = 0
    for clip, got, plan in zip(staged, out, PLANS[name]):
        rle_route = augment.reference_augment_masks(
            [(t, fr["gt_rle"][2]) for t, fr in enumerate(clip["instances"])], [(H, W)] * len(plan), plan)[0]
        for t, (fr, g, p) in enumerate(zip(clip["instances"], got["instances"], plan)):
            assert g["gt_masks"].shape == (5, p.nh, p.nw) and g["gt_masks"].dtype == torch.bool
            for s, q in enumerate(fr["gt_poly"]):
                want = rle_route[t] if q is None else expected_mask(q, p)
                assert np.array_equal(g["gt_masks"][s].numpy(), want), (name, t, s)
                box, nonempty = augment.mask_box(want)
                assert np.array_equal(g["gt_boxes"][s].numpy(), box)
                assert int(g["gt_ids"][s]) == (int(fr["gt_ids"][s]) if nonempty else -1)
                filled += int(nonempty)
            assert not g["gt_masks"][3].any() and int(g["gt_ids"][3]) == -1     # the dummy polygon is the empty mask
    assert filled >= 6 * len(staged)


def test_a_full_plan_at_source_size_is_the_plain_rasterisation():
    p = augment.full_plan(H, W, H, W)
    assert np.array_equal(augment.reference_polygon_mask(HOLE, p), P.counts_to_mask(P.object_counts_host(HOLE, H, W), H, W))
    flipped = augment.reference_polygon_mask([10.0, 20.0, 30.0, 40.0], augment.full_plan(H, W, H, W, True))
    want = np.zeros((H, W), bool)
    want[20:60, W - 40:W - 10] = True                                           # an integer box mirrors exactly
    assert np.array_equal(flipped, want)


def test_applies_says_no_beyond_the_caps():
    frames = [torch.zeros(3, H, W, dtype=torch.uint8)]
    plan = [augment.full_plan(H, W, 60, 100)]
    ok = ([[STAR]], [(60, 100)])
    big = ([[[float(v) for k in range(1100) for v in (k % 97, k % 61)]]], [(60, 100)])
    assert augment.applies(frames, plan, "cpu", polygons=ok) and augment.applies(frames, plan, "cpu")
    assert not augment.applies(frames, plan, "cpu", polygons=big)
    assert not augment.applies(frames, plan, "cpu", polygons=P.plan_objects(*big))


def stub_model():
    backbone = SimpleNamespace()
    return SimpleNamespace(device_augment=True, training=True, device=torch.device(DEV),
                           _pixel_stats=((123.675, 116.28, 103.53), (58.395, 57.12, 57.375)),
                           detr=SimpleNamespace(detr=SimpleNamespace(backbone=backbone)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PLANS))
def test_augment_step_equals_host_augmented(name):
    """masks, boxes and ids of polygon and RLE instances from ONE augment_masks call; the frames as without polygons"""
    staged = clips(PLANS[name])
    calls = dict(augment.CALLS)
    out, pre = frames_mod.augment_step(stub_model(), staged)
    assert pre is not None and augment.CALLS == {k: v + 1 for k, v in calls.items()}
    want = frames_mod.host_augmented(staged)
    for got, ref in zip(out, want):
        for g, r in zip(got["instances"], ref["instances"]):
            assert g["gt_masks"].is_cuda and g["gt_masks"].dtype == torch.bool
            assert torch.equal(g["gt_masks"].cpu(), r["gt_masks"])
            assert torch.equal(g["gt_boxes"].cpu(), r["gt_boxes"])
            assert torch.equal(g["gt_ids"].cpu(), r["gt_ids"]) and g["gt_ids"].dtype == torch.int64
            assert torch.equal(g["gt_classes"], r["gt_classes"])
    # the frames do not depend on the masks: the same step staged without polygons gives the same x
    plain = [{**c, "instances": [{k: v for k, v in fr.items() if k != "gt_poly"} | {"gt_rle": [[H * W]] * 5}
                                 for fr in c["instances"]]} for c in staged]
    _, pre_plain = frames_mod.augment_step(stub_model(), plain)
    assert torch.equal(pre[0], pre_plain[0]) and torch.equal(pre[1], pre_plain[1])


@pytest.mark.gpu
def test_a_step_beyond_the_caps_takes_the_host_route():
    staged = clips(PLANS["full"])
    rng = np.random.default_rng(1)
    big = np.empty(2 * 1500)
    big[0::2], big[1::2] = rng.uniform(0, W, 1500), rng.uniform(0, H, 1500)
    staged[0]["instances"][0]["gt_poly"][0] = [big.tolist()]
    calls = dict(augment.CALLS)
    out, pre = frames_mod.augment_step(stub_model(), staged)
    assert pre is None and augment.CALLS == calls
    assert out[0]["instances"][0]["gt_masks"].shape == (5, 60, 100)
