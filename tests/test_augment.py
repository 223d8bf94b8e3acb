"""Training-time augmentation, the host side (vnext_amd/ops/augment.py, vnext_amd/data/clip_mapper.py).

What is held to what, on the CPU:
* `reference_augment_frames` / `reference_augment_masks` -- numpy slicing, the integer restatement of Pillow's bilinear resize,
  Pillow's NEAREST index tables, `np.flip` -- equal Pillow's stored results of tests/golden/augment_pillow.npz
  (tools/make_golden_augment.py; no Pillow needed here) exactly.
* `nearest_table` equals the ramps Pillow produced for every (720 | 1280 -> config size) pair and 48 odd pairs.
* `sample_plan` draws what the configs allow; `stage_clip` keeps the reference mapper's bookkeeping.
* the CPU route of the ops (CPU tensors through `stage_step`) is the reference route.
The kernels are held to the same references in tests/test_train_augment_gpu.py.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from vnext_amd.data import clip_mapper
from vnext_amd.ops import augment, resize
from vnext_amd.utils.ytvis_json import counts_to_string, rle_counts


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN_DIR, "augment_pillow.npz")))


def cases(golden, kind):
    i = 0
    while "%s%d_plan" % (kind, i) in golden:
        yield i
        i += 1


def plan_of(row, flip=False):
    x0, y0, cw, ch, nh, nw = (int(v) for v in row)
    return augment.FramePlan(x0, y0, cw, ch, nh, nw, flip)


def test_reference_augment_frames_equals_pillow(golden):
    n = 0
    for i in cases(golden, "f"):
        src, want = golden["f%d_src" % i], golden["f%d_out" % i]
        for flip in (False, True):
            p = plan_of(golden["f%d_plan" % i], flip)
            expect = np.flip(want, axis=1) if flip else want
            got = augment.reference_augment_frames([src], [p], "hwc")[0]
            assert got.dtype == np.uint8 and np.array_equal(got, expect), (i, flip)
            chw = torch.from_numpy(np.ascontiguousarray(src.transpose(2, 0, 1)))
            got = augment.reference_augment_frames([chw], [p], "chw")[0]
            assert torch.is_tensor(got) and np.array_equal(got.numpy().transpose(1, 2, 0), expect), (i, flip)
        n += 1
    assert n >= 7


def test_reference_augment_masks_equals_pillow_and_boxes_are_the_bitmask_boxes(golden):
    n = 0
    for i in cases(golden, "m"):
        size, counts, want = tuple(golden["m%d_size" % i].tolist()), golden["m%d_counts" % i], golden["m%d_out" % i] != 0
        for flip in (False, True):
            p = plan_of(golden["m%d_plan" % i], flip)
            expect = np.flip(want, axis=1) if flip else want
            (got,), boxes, flags = augment.reference_augment_masks([(0, counts)], [size], [p])
            assert got.dtype == bool and np.array_equal(got, expect), (i, flip)
            ys, xs = np.nonzero(expect)              # BitMasks.get_bounding_boxes, the other way round
            if len(xs):
                assert boxes[0].tolist() == [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1] and flags[0]
            else:
                assert boxes[0].tolist() == [0, 0, 0, 0] and not flags[0]
        n += 1
    assert n >= 11


def test_nearest_table_equals_pillows_ramps(golden):
    pairs, starts, data = golden["ramp_pairs"].tolist(), golden["ramp_starts"], golden["ramp_data"]
    assert len(pairs) >= 60 and {720, 1280} <= {a for a, _ in pairs}
    closed_form_differs = 0
    for (n_in, n_out), s, e in zip(pairs, starts[:-1], starts[1:]):
        tab = augment.nearest_table(n_in, n_out)
        assert tab.dtype == np.int32 and tab.shape == (n_out,) and np.array_equal(tab, data[s:e]), (n_in, n_out)
        assert augment.nearest_table(n_in, n_out) is tab and not tab.flags.writeable      # cached, read-only
        closed = np.floor((np.arange(n_out) + 0.5) * n_in / n_out).astype(np.int32)
        closed_form_differs += not np.array_equal(closed, data[s:e])
    assert closed_form_differs > 0      # the accumulated table is not the closed form: the reason it is restated


def train_cfg(**inp):
    return SimpleNamespace(INPUT=SimpleNamespace(**inp))


IDOL_INPUT = dict(MIN_SIZE_TRAIN=(320, 352, 392, 416, 448, 480, 512, 544, 576, 608, 640), MAX_SIZE_TRAIN=768,
                  MIN_SIZE_TRAIN_SAMPLING="choice_by_clip", RANDOM_FLIP="flip_by_clip",
                  CROP=SimpleNamespace(ENABLED=True, TYPE="absolute_range", SIZE=(384, 600)))


def test_sample_plan_draws_what_the_config_allows():
    rng = np.random.default_rng(3)
    cfg = train_cfg(**IDOL_INPUT)
    sizes = [(720, 1280), (720, 1280), (400, 500)]
    cropped = flipped = 0
    shorts = set()
    for _ in range(200):
        plan = clip_mapper.sample_plan(cfg, sizes, 3, rng)
        assert len(plan) == 3 and len({p.flip for p in plan}) == 1                       # flip_by_clip
        crops = [(p.cw, p.ch) != (w, h) or (p.x0, p.y0) != (0, 0) for p, (h, w) in zip(plan, sizes)]
        for p, (h, w) in zip(plan, sizes):
            assert 0 <= p.x0 and 0 <= p.y0 and p.x0 + p.cw <= w and p.y0 + p.ch <= h       # inside the frame
            if (p.cw, p.ch) != (w, h):
                assert min(h, 384) <= p.ch <= min(h, 600) and min(w, 384) <= p.cw <= min(w, 600)
            # the target is ResizeShortestEdge's of the WINDOW for one of the configured short edges
            match = [s for s in cfg.INPUT.MIN_SIZE_TRAIN if resize.shortest_edge_size(p.ch, p.cw, s, 768) == (p.nh, p.nw)]
            assert match, p
            shorts.add(match[0])
        # choice_by_clip: ONE short edge fits all frames of the clip
        assert any(all(resize.shortest_edge_size(p.ch, p.cw, s, 768) == (p.nh, p.nw) for p in plan)
                   for s in cfg.INPUT.MIN_SIZE_TRAIN)
        cropped += any(crops)
        flipped += plan[0].flip
    assert 60 < cropped < 140 and 60 < flipped < 140 and len(shorts) > 5      # coins of 1/2 over 200 clips
    # per-frame forms, no crop, a range
    cfg = train_cfg(MIN_SIZE_TRAIN=(300, 340), MAX_SIZE_TRAIN=1333, MIN_SIZE_TRAIN_SAMPLING="range", RANDOM_FLIP="horizontal")
    seen_sizes, seen_flips = set(), set()
    for _ in range(50):
        plan = clip_mapper.sample_plan(cfg, [(720, 1280)] * 4, 4, rng)
        assert all((p.x0, p.y0, p.cw, p.ch) == (0, 0, 1280, 720) and 300 <= p.nh <= 340 for p in plan)
        seen_sizes.add(len({p.nh for p in plan}))
        seen_flips.add(len({p.flip for p in plan}))
    assert max(seen_sizes) > 1 and max(seen_flips) > 1
    assert not any(p.flip for p in clip_mapper.sample_plan(train_cfg(RANDOM_FLIP="none"), [(64, 64)], 1, rng))
    for bad in (dict(AUGMENTATIONS=["rotation"]), dict(RANDOM_FLIP="vertical"),
                dict(CROP=SimpleNamespace(ENABLED=True, TYPE="relative_range", SIZE=(0.9, 0.9)))):
        with pytest.raises(ValueError):
            clip_mapper.sample_plan(train_cfg(**bad), [(64, 64)], 1, rng)


def two_frame_clip():
    """ids 7 and 9 on frame 0; 9, a crowd annotation 4 and a new id 2 on frame 1"""
    g = torch.Generator().manual_seed(1)
    frames = [torch.randint(0, 256, (3, 20, 30), dtype=torch.uint8, generator=g) for _ in range(2)]
    def mask(y, x):
        m = np.zeros((20, 30), dtype=np.uint8)
        m[y:y + 5, x:x + 6] = 1
        return m
    m7, m9, m9b, m2 = mask(2, 3), mask(10, 20), mask(11, 19), mask(0, 0)
    annos = [[{"id": 7, "category_id": 3, "segmentation": rle_counts(m7).tolist()},
              {"id": 9, "category_id": 5, "segmentation": {"size": [20, 30], "counts": counts_to_string(rle_counts(m9))}}],
             [{"id": 9, "category_id": 5, "segmentation": counts_to_string(rle_counts(m9b))},
              {"id": 4, "category_id": 1, "iscrowd": 1, "segmentation": rle_counts(m7).tolist()},
              {"id": 2, "category_id": 8, "segmentation": rle_counts(m2).tolist()}]]
    plan = [augment.FramePlan(2, 1, 26, 18, 24, 35, True), augment.FramePlan(0, 0, 30, 20, 24, 36, True)]
    return frames, annos, plan, (m7, m9, m9b, m2)


def test_stage_clip_slot_order_dummy_annotation_and_iscrowd():
    frames, annos, plan, (m7, m9, m9b, m2) = two_frame_clip()
    entry = clip_mapper.stage_clip(frames, annos, plan, num_classes=40)
    assert entry["image"][0] is frames[0] and entry["augment"] == plan and "image_layout" not in entry
    f0, f1 = entry["instances"]
    # slots in order of first appearance: 7, 9, 4 (the crowd keeps its slot), 2
    assert f0["gt_ids"].tolist() == [7, 9, -1, -1] and f0["gt_classes"].tolist() == [3, 5, 40, 40]
    assert f1["gt_ids"].tolist() == [-1, 9, -1, 2] and f1["gt_classes"].tolist() == [40, 5, 40, 8]
    assert f0["image_size"] == (24, 35) and f1["image_size"] == (24, 36)
    assert f0["gt_rle"][0] == rle_counts(m7).tolist() and f0["gt_rle"][1] == rle_counts(m9).tolist()      # string -> counts
    assert f0["gt_rle"][2] == [600] and f1["gt_rle"][0] == [600] and f1["gt_rle"][2] == [600]              # the dummy: n_runs 1
    assert f1["gt_rle"][1] == rle_counts(m9b).tolist() and f1["gt_rle"][3] == rle_counts(m2).tolist()
    with pytest.raises(ValueError, match="frPyObjects"):
        clip_mapper.stage_clip(frames[:1], [[{"id": 1, "category_id": 1, "segmentation": [[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]]}]],
                               plan[:1], 40)


def test_the_cpu_route_of_the_ops_is_the_reference_route():
    frames, annos, plan, _ = two_frame_clip()
    entry = clip_mapper.stage_clip(frames, annos, plan, 40)
    listed = [(f, c) for f, fr in enumerate(entry["instances"]) for c in fr["gt_rle"]]
    ids = [i for fr in entry["instances"] for i in fr["gt_ids"].tolist()]
    staged = augment.stage_step(frames, plan, listed, "cpu", "chw", ids)
    assert staged.size == (32, 64) and staged.pixels.data_ptr() % 16 == 0 and staged.ids.tolist() == ids
    assert staged.src_table.tolist()[0][1:] == [20, 30, 2, 1, 26, 18, 1] and staged.dst_table.tolist() == [[0, 24, 35], [0, 24, 36]]
    assert staged.mask_rows[:, 1].tolist() == [len(c) for _, c in listed] and staged.mask_rows[:, 2].tolist() == [0] * 4 + [1] * 4
    words = staged.coeffs.numpy()
    for i, p in enumerate(plan):             # the nearest tables ride behind the bilinear ones
        assert np.array_equal(words[words[8 * i + 6]:][:p.nw], augment.nearest_table(p.cw, p.nw))
        assert np.array_equal(words[words[8 * i + 7]:][:p.nh], augment.nearest_table(p.ch, p.nh))
    mean, std = [1.0, 2.0, 3.0], [2.0, 4.0, 8.0]
    x, mask = augment.augment_frames(staged, mean, std)
    want = augment.reference_augment_frames(frames, plan, "chw")
    assert tuple(x.shape) == (2, 3, 32, 64) and mask.dtype == torch.bool
    for i, (w, p) in enumerate(zip(want, plan)):
        expect = (w.float() - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)
        assert torch.equal(x[i, :, :p.nh, :p.nw], expect) and not mask[i, :p.nh, :p.nw].any()
        assert mask[i, p.nh:].all() and mask[i, :, p.nw:].all() and (x[i, :, p.nh:] == 0).all()
    masks, boxes, nonempty = augment.augment_masks(staged)
    outs, want_boxes, flags = augment.reference_augment_masks(listed, [(20, 30)] * 2, plan)
    views = staged.mask_views(masks)
    assert [tuple(v.shape) for v in views] == [(4, 24, 35), (4, 24, 36)] and views[0].dtype == torch.bool
    assert all(np.array_equal(v.numpy(), o) for v, o in zip([m for v in views for m in v], outs))
    assert np.array_equal(boxes.numpy(), want_boxes) and nonempty.tolist() == flags.tolist() == [True, True, False, False,
                                                                                                False, True, False, True]
    # a window the bilinear kernel does not cover (10x): `applies` is false
    far = augment.FramePlan(0, 0, 30, 20, 2, 3, False)
    assert augment.applies(frames, plan, "cpu") and not augment.applies(frames, [far, far], "cpu")
    assert not augment.applies(frames, [plan[0]._replace(x0=5), plan[1]], "cpu")      # the window leaves the frame


def test_enable_device_augment_flips_both_models_and_raises_without_the_switch():
    import vnext_amd.models  # noqa: F401  (registers the meta-archs)
    from vnext_amd import train as T
    from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg
    tiny = {"ENC_LAYERS": 1, "DEC_LAYERS": 1, "NUM_OBJECT_QUERIES": 4, "DIM_FEEDFORWARD": 32}
    seq = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": "cpu", **{"MODEL.SeqFormer." + k: v for k, v in tiny.items()}}))
    idol = build_model(get_idol_cfg(**{"MODEL.DEVICE": "cpu", **{"MODEL.IDOL." + k: v for k, v in tiny.items()}}))
    for model in (seq, idol):
        assert model.device_augment is False
        T.enable_device_augment(model)
        assert model.device_augment is True
        T.enable_device_augment(model, on=False)
        assert model.device_augment is False
    with pytest.raises(ValueError, match="device_augment"):
        T.enable_device_augment(torch.nn.Linear(2, 2))


# ---- the models on the CPU: the switch takes the reference route of the ops, the wiring is the GPU's -------------------------
from test_resize import cpu_stand_ins  # noqa: E402,F401  (the PyTorch restatements of the HIP entry points the models call)


def test_seqformer_and_idol_training_steps_with_the_switch_on_cpu(cpu_stand_ins):  # noqa: F811
    import vnext_amd.models  # noqa: F401
    from test_train_augment_gpu import TINY_IDOL, TINY_SEQ, flat_targets, step_both_routes, training_clips
    from vnext_amd import train as T
    from vnext_amd.models import frames as frames_mod
    from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg
    torch.manual_seed(5)
    seq = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": "cpu", **TINY_SEQ})).train()
    plans = [[augment.full_plan(96, 160, 60, 100, True)] * 2, [augment.full_plan(96, 160, 60, 100, False)] * 2]
    step_both_routes(seq, training_clips(2, 2, plans, seed=50))
    idol = build_model(get_idol_cfg(**{"MODEL.DEVICE": "cpu", **TINY_IDOL})).train()
    plans = [[augment.FramePlan(16, 8, 120, 80, 64, 96, True), augment.FramePlan(0, 0, 160, 96, 60, 100, True)],
             [augment.FramePlan(10, 0, 140, 88, 88, 140, False), augment.FramePlan(20, 12, 128, 80, 70, 112, False)]]
    clips = training_clips(2, 2, plans, seed=60)      # (IDOL's reid loss has no CPU stand-in: the front end and the targets)
    T.enable_device_augment(idol)
    T.enable_device_ingest(idol)
    filled, pre = frames_mod.augment_step(idol, clips)
    host = frames_mod.host_augmented(clips)
    want = idol._preprocess([f for clip in host for f in clip["image"]])
    assert len(pre) == len(want) == 3 and torch.equal(pre[0], want[0]) and torch.equal(pre[1], want[1])
    assert torch.equal(pre[2][:, 1:], want[2][:, 1:])      # the tables: the same sizes (the ingest's also holds byte offsets)
    for a, b in zip(flat_targets(idol.prepare_targets(filled)), flat_targets(idol.prepare_targets(host))):
        assert a.dtype == b.dtype and torch.equal(a, b)
    # eval mode and clips without "augment" do not take the route
    T.enable_device_augment(seq)
    plain = frames_mod.host_augmented(training_clips(1, 2, plans[:1], seed=70))
    assert frames_mod.augment_step(seq, plain) == (plain, None)
    assert frames_mod.augment_step(seq.eval(), training_clips(1, 2, plans[:1], seed=70))[1] is None
