"""Colour augmentation, the host side (vnext_amd/ops/augment.py, vnext_amd/data/clip_mapper.py).

What is held to what, on the CPU:
* `reference_augment_frames` with colour weights in the plan equals tests/golden/augment_color.npz byte for byte: the three
  steps written out in numpy by tools/make_golden_augment_color.py (independently of the package) on frames Pillow resized.
* `sample_plan` draws a weight per frame and per listed step, leaves every other draw where it was, and keeps refusing
  "rotation"; `crop_size` gives `RandomCrop.get_crop_size`'s sizes for all four types.
* the colour table `stage_step` packs decodes to the weights bit for bit, a step without a weight stages what it always
  did, and the CPU route of the op is the reference route.
The kernels are held to the same fixture in tests/test_train_augment_color_gpu.py.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from vnext_amd.data import clip_mapper
from vnext_amd.ops import augment, resize
from vnext_amd.ops.augment import FramePlan

SUBSETS = list(range(1, 8))      # 1 brightness | 2 contrast | 4 saturation
NAMES = clip_mapper.COLOR_NAMES


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN_DIR, "augment_color.npz")))


def n_cases(golden):
    return sum(1 for k in golden if k.endswith("_plan"))


def plan_of(golden, i, subset):
    x0, y0, cw, ch, nh, nw, flip = (int(v) for v in golden["c%d_plan" % i])
    w = golden["c%d_weights" % i].tolist()
    return FramePlan(x0, y0, cw, ch, nh, nw, bool(flip), *(w[j] if subset >> j & 1 else None for j in range(3)))


def test_frame_plan_defaults_to_no_colour_and_keeps_its_positional_meaning():
    p = FramePlan(1, 2, 3, 4, 5, 6, True)
    assert p.color == (None, None, None) == augment.NO_COLOR and p[:7] == (1, 2, 3, 4, 5, 6, True)
    assert FramePlan(1, 2, 3, 4, 5, 6, True, 0.95).color == (0.95, None, None)
    assert augment.full_plan(4, 5, 6, 7).color == augment.NO_COLOR and augment.chain_full(4, 5, 6, 7).color == augment.NO_COLOR


def test_reference_augment_frames_equals_the_fixture_for_every_subset(golden):
    assert n_cases(golden) >= 7 and str(golden["numpy_version"]).startswith("2.")
    for i in range(n_cases(golden)):
        src = golden["c%d_src" % i]
        for subset in [0] + SUBSETS:
            p, want = plan_of(golden, i, subset), golden["c%d_s%d" % (i, subset)]
            got = augment.reference_augment_frames([src], [p], "hwc")[0]
            assert got.dtype == np.uint8 and np.array_equal(got, want), (i, subset)
            chw = torch.from_numpy(np.ascontiguousarray(src.transpose(2, 0, 1)))
            got = augment.reference_augment_frames([chw], [p], "chw")[0]
            assert torch.is_tensor(got) and np.array_equal(got.numpy().transpose(1, 2, 0), want), (i, subset)
    # the cases say what they are for: a clip at 255, an all-zero frame, one pixel
    assert (golden["c3_s0"] == 255).all() and (golden["c3_s1"] == 255).all() and (golden["c4_s7"] == 0).all()
    assert golden["c2_s7"].shape == (1, 1, 3)


def test_the_steps_are_the_issues_arithmetic_on_single_pixels():
    """values worked out by hand: truncation, the float32 product, the mean over ALL bytes, the gray sum's order"""
    one = np.array([[[10, 200, 255]]], dtype=np.uint8)
    assert augment.color_frame(one, 2, brightness=1.1).tolist() == [[[11, 220, 255]]]      # 280.5 clips
    assert augment.color_frame(one, 2, brightness=0.9).tolist() == [[[9, 180, 229]]]       # float32(0.9) * 255 = 229.5.. -> 229
    m = (10 + 200 + 255) / 3
    want = [int((1 - 0.9) * m + 0.9 * v) for v in (10, 200, 255)]
    assert augment.color_frame(one, 2, contrast=0.9).tolist() == [[want]]
    gray = 10 * 0.299 + 200 * 0.587 + 255 * 0.114
    want = [min(255, max(0, int((1 - 1.1) * gray + 1.1 * v))) for v in (10, 200, 255)]
    assert augment.color_frame(one, 2, saturation=1.1).tolist() == [[want]]
    chw = np.ascontiguousarray(one.transpose(2, 0, 1))
    assert augment.color_frame(chw, 0, saturation=1.1).reshape(-1).tolist() == want


def test_the_fixture_records_how_often_blas_disagrees_with_the_gray_sum(golden):
    n = int(golden["dot_disagreements"])
    assert 0 <= n <= 2 ** 24
    with open(os.path.join(os.path.dirname(os.path.dirname(GOLDEN_DIR)), "DESIGN.md")) as f:
        assert str(n) in f.read()      # DESIGN section 31 says it


# ---- the draws --------------------------------------------------------------------------------------------------------------
def train_cfg(**inp):
    return SimpleNamespace(INPUT=SimpleNamespace(**inp))


BASE = dict(MIN_SIZE_TRAIN=(320, 352, 392, 416), MAX_SIZE_TRAIN=768, MIN_SIZE_TRAIN_SAMPLING="choice_by_clip",
            RANDOM_FLIP="flip_by_clip", CROP=SimpleNamespace(ENABLED=True, TYPE="absolute_range", SIZE=(384, 600)))
SIZES = [(720, 1280), (720, 1280), (400, 500)]


@pytest.mark.parametrize("subset", SUBSETS)
def test_sample_plan_draws_a_weight_per_frame_for_each_listed_step(subset):
    listed = [n for j, n in enumerate(NAMES) if subset >> j & 1]
    cfg = train_cfg(AUGMENTATIONS=listed[::-1], **BASE)      # (the list's own order does not matter: build_augmentation's does)
    rng = np.random.default_rng(11)
    for _ in range(20):
        plan = clip_mapper.sample_plan(cfg, SIZES, 3, rng)
        assert len({p.flip for p in plan}) == 1                                  # flip_by_clip holds ...
        for j in range(3):
            weights = [p.color[j] for p in plan]
            if subset >> j & 1:
                assert all(isinstance(w, float) and 0.9 <= w <= 1.1 for w in weights)
                assert len(set(weights)) == 3                                    # ... and the weights differ all the same
            else:
                assert weights == [None] * 3


def test_the_other_draws_are_where_they_were():
    """an empty list: the parent's stream (restated here draw for draw); a full list: the same geometry up to the first
    frame's weights, which are drawn AFTER that frame's crop, size and flip"""
    for listed in ([], None):
        cfg = train_cfg(AUGMENTATIONS=listed, **BASE) if listed is not None else train_cfg(**BASE)
        plan = clip_mapper.sample_plan(cfg, SIZES, 3, np.random.default_rng(5))
        rng = np.random.default_rng(5)
        use_crop = not rng.random() > 0.5
        want, size, flip = [], None, False
        for i, (h, w) in enumerate(SIZES):
            x0, y0, cw, ch = 0, 0, w, h
            if use_crop:
                ch = int(rng.integers(min(h, 384), min(h, 600) + 1))
                cw = int(rng.integers(min(w, 384), min(w, 600) + 1))
                y0 = int(rng.integers(h - ch + 1))
                x0 = int(rng.integers(w - cw + 1))
            if size is None:
                size = int(rng.choice(BASE["MIN_SIZE_TRAIN"]))
            if i == 0:
                flip = bool(rng.random() < 0.5)
            want.append(FramePlan(x0, y0, cw, ch, *resize.shortest_edge_size(ch, cw, size, 768), flip))
        assert plan == want and all(p.color == augment.NO_COLOR for p in plan)
    for seed in range(6):
        plain = clip_mapper.sample_plan(train_cfg(**BASE), SIZES, 3, np.random.default_rng(seed))
        rng = np.random.default_rng(seed)
        full = clip_mapper.sample_plan(train_cfg(AUGMENTATIONS=list(NAMES), **BASE), SIZES, 3, rng)
        assert full[0][:7] == plain[0][:7]
        # the three weights follow the first frame's draws directly, in build_augmentation's order
        rng2 = np.random.default_rng(seed)
        clip_mapper.sample_plan(train_cfg(**BASE), SIZES[:1], 1, rng2)
        assert full[0].color == tuple(float(rng2.uniform(0.9, 1.1)) for _ in range(3))


def test_rotation_and_unknown_names_raise_naming_the_entry():
    rng = np.random.default_rng(0)
    for bad in ("rotation", "hue"):
        with pytest.raises(ValueError, match=bad):
            clip_mapper.sample_plan(train_cfg(AUGMENTATIONS=["brightness", bad]), [(64, 64)], 1, rng)
    with pytest.raises(ValueError):      # the COCO mapper never reads the key: unchanged
        clip_mapper.sample_coco_plan(train_cfg(AUGMENTATIONS=["brightness"]), (64, 64), rng)


class FixedRandom:
    """`rng.random(2)` of the relative_range draw, fixed"""

    def __init__(self, values):
        self.values = np.asarray(values, dtype=np.float64)

    def random(self, n):
        assert n == len(self.values)
        return self.values


def test_crop_size_gives_the_references_sizes():
    """RandomCrop.get_crop_size, restated from detectron2: edge values included"""
    for (h, w), size, want in [((480, 640), (0.5, 0.5), (240, 320)), ((481, 641), (0.5, 0.5), (241, 321)),      # x.5 rounds up
                               ((37, 53), (1.0, 1.0), (37, 53)), ((37, 53), (0.9, 0.3), (33, 16)), ((1, 1), (0.6, 0.4), (1, 0))]:
        assert clip_mapper.crop_size("relative", size, h, w, None) == (int(h * size[0] + 0.5), int(w * size[1] + 0.5)) == want
    for (h, w), size, want in [((480, 640), (384, 600), (384, 600)), ((300, 640), (384, 600), (300, 600)),      # larger than the image
                               ((300, 500), (384, 600), (300, 500)), ((384, 600), (384, 600), (384, 600))]:
        assert clip_mapper.crop_size("absolute", size, h, w, None) == want
    # relative_range: the fraction c + rand * (1 - c) with c in FLOAT32, as np.asarray(crop_size, dtype=np.float32) makes it
    for (h, w), size, rand in [((480, 640), (0.9, 0.9), (0.0, 1.0)), ((481, 641), (0.9, 0.7), (0.25, 0.5)),
                               ((37, 53), (1.0, 1.0), (0.3, 0.8)), ((720, 1280), (0.3, 0.6), (0.999, 0.001))]:
        c = np.asarray(size, dtype=np.float32)
        fh, fw = c + np.asarray(rand) * (1 - c)
        want = (int(h * fh + 0.5), int(w * fw + 0.5))
        assert clip_mapper.crop_size("relative_range", size, h, w, FixedRandom(rand)) == want
        assert want[0] <= h and want[1] <= w
    assert clip_mapper.crop_size("relative_range", (0.9, 0.9), 480, 640, FixedRandom((1.0, 1.0))) == (480, 640)      # fraction 1.0
    # float32(0.9) is not 0.9: at rand = 0 the fraction is the float32 value, and the size follows it
    assert clip_mapper.crop_size("relative_range", (0.9, 0.9), 10 ** 8, 5, FixedRandom((0.0, 0.0)))[0] == \
        int(10 ** 8 * float(np.float32(0.9)) + 0.5) != int(10 ** 8 * 0.9 + 0.5)
    rng = np.random.default_rng(2)
    for _ in range(50):
        ch, cw = clip_mapper.crop_size("absolute_range", (384, 600), 400, 1280, rng)
        assert 384 <= ch <= 400 and 384 <= cw <= 600
    with pytest.raises(ValueError):
        clip_mapper.crop_size("square", (1, 1), 4, 4, rng)


def test_sample_plan_takes_relative_and_absolute_crops():
    rng = np.random.default_rng(4)
    for crop_type, size, want in (("relative", (0.5, 0.25), (360, 320)), ("absolute", (384, 2000), (384, 1280))):
        cfg = train_cfg(**{**BASE, "CROP": SimpleNamespace(ENABLED=True, TYPE=crop_type, SIZE=size)})
        seen = set()
        for _ in range(40):
            for p in clip_mapper.sample_plan(cfg, [(720, 1280)] * 2, 2, rng):
                assert p.inside(720, 1280)
                seen.add((p.ch, p.cw))
        assert seen == {want, (720, 1280)}      # the clip's coin: the crop or the whole frame


# ---- staging ----------------------------------------------------------------------------------------------------------------
def test_color_words_hold_the_weights_bit_for_bit_and_a_plain_step_stages_what_it_did():
    plan = [FramePlan(0, 0, 30, 20, 24, 36, False, 0.9123456789, None, 1.0999999999),
            FramePlan(2, 1, 26, 18, 24, 35, True), FramePlan(0, 0, 30, 20, 10, 12, False, None, 1.05, None)]
    rows = augment.color_words(plan)
    assert rows.dtype == np.int32 and rows.shape == (3, 8) and rows[:, 0].tolist() == [5, 0, 2] and not rows[1].any()
    assert rows[0, 1] == np.array([0.9123456789], dtype=np.float32).view(np.int32)[0]
    assert np.array_equal(rows[2, 2:4], np.array([1.05], dtype="<f8").view(np.int32))
    got = [augment.color_of(r) for r in rows.tolist()]
    assert got[0] == (float(np.float32(0.9123456789)), None, 1.0999999999) and got[1] == augment.NO_COLOR
    assert got[2] == (None, 1.05, None)
    g = torch.Generator().manual_seed(3)
    frames = [torch.randint(0, 256, (3, 20, 30), dtype=torch.uint8, generator=g) for _ in plan]
    staged = augment.stage_step(frames, plan, [(1, [600])], "cpu")
    assert np.array_equal(staged.color.numpy(), rows) and staged.workspace == -1      # (the workspace exists on the device only)
    plain = augment.stage_step(frames, [FramePlan(*p[:7]) for p in plan], [(1, [600])], "cpu")
    assert plain.color is None and plain.workspace == -1
    for a, b in zip(staged[1:7], plain[1:7]):      # the tables of a coloured step are the plain step's, and so are the frames
        assert torch.equal(a, b)
    assert staged.pixels.numel() == plain.pixels.numel()
    for off, h, w in (r[:3] for r in plain.src_table.tolist()):      # (the bytes between two frames are nobody's)
        assert torch.equal(staged.pixels[off:off + 3 * h * w], plain.pixels[off:off + 3 * h * w])
    assert augment.color_workspace(3, 64, 96) == 3 * 3 * 64 * 96 + 4 * 3 * 2 * 3


def test_the_cpu_route_of_the_op_is_the_reference_route(golden):
    for j in (0, 1):
        cases = golden["batch%d" % j].tolist()
        plan = [plan_of(golden, i, 7) for i in cases]
        frames = [torch.from_numpy(golden["c%d_src" % i]) for i in cases]
        mean, std = golden["pixel_mean"].tolist(), golden["pixel_std"].tolist()
        for layout in ("hwc", "chw"):
            fs = [f if layout == "hwc" else f.permute(2, 0, 1).contiguous() for f in frames]
            assert augment.applies(fs, plan, "cpu", layout)
            calls = dict(augment.COLOR_CALLS)
            x, mask = augment.augment_frames(augment.stage_step(fs, plan, [], "cpu", layout), mean, std)
            assert augment.COLOR_CALLS == calls
            assert np.array_equal(mask.numpy(), golden["batch%d_mask" % j])
            assert np.array_equal(x.numpy(), golden["batch%d_x" % j])
