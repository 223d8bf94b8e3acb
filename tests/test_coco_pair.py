"""COCO pre-training pairs: the chain flip -> resize -> crop -> resize of IDOL's `COCO_CLIP_DatasetMapper` (vnext_amd/ops/augment.py,
vnext_amd/data/clip_mapper.py, vnext_amd/csrc/resize_body.h).

What is held to what:
* `reference_chain_frames` -- `np.flip`, the integer restatement of Pillow's bilinear resize, slicing, the restatement again --
  equals Pillow's stored results of tests/golden/coco_pair_pillow.npz (tools/make_golden_coco_pair.py) and, where Pillow
  imports, the literal PIL calls, byte for byte;
* `sample_coco_plan` draws what the mapper draws; `stage_coco_pair` keeps its bookkeeping;
* polygons, boxes and ids on a rectangle whose result is exact by hand;
* the CPU route of the ops (CPU tensors through `stage_step`, `resize_window_bytes`, `augment_frames`) is the reference route;
* GPU: `vnx_resize_window_bytes` through the C ABI into a guarded buffer equals the fixture byte for byte, and the second
  launch (`vnx_augment_frames` reading the slots) the fixture's final frames.
The whole training step and the hipGraph replay are in tests/test_train_coco_pair_gpu.py.

The cases (CASES below; each in CHW and HWC, flip off and on, every frame and slot at an odd byte offset):
  0  37 x 53 -> (45, 64), window (5, 3, 41, 35) -> (33, 39): two tiles on both axes of the window, an odd origin
  1  the window touches the right and bottom edges of (h1, w1)
  2  a 1 x 1 window
  3  w1 == w (the first horizontal pass is skipped) and nh == ch (the second vertical pass is skipped)
  4  an upscale followed by a downscale (three tiles across)
  5  a downscale followed by an upscale
  6  the side without a crop: no first resample, one launch
  7  (h1, w1) == (h, w) with a true crop: no first resample either, the mirrored window of the source itself
Cases 0, 1, 2 and 6 share one source; one launch holds all of them: frames with and without the first resample, four source
sizes.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from vnext_amd.data import clip_mapper
from vnext_amd.models import frames as frames_mod
from vnext_amd.ops import augment, resize
from vnext_amd.ops.augment import ChainPlan, FramePlan

DEV = "cuda:0"
GUARD = 64


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN_DIR, "coco_pair_pillow.npz")))


def cases(golden):
    """-> [(case, flip, source uint8 [h, w, 3], ChainPlan, mid uint8 [ch, cw, 3], out uint8 [nh, nw, 3])]"""
    out, i = [], 0
    while "c%d_plan" % i in golden:
        src = golden["src%d" % int(golden["c%d_src" % i])]
        h1, w1, x0, y0, cw, ch, nh, nw = (int(v) for v in golden["c%d_plan" % i])
        for flip in (0, 1):
            p = ChainPlan(src.shape[0], src.shape[1], bool(flip), h1, w1, x0, y0, cw, ch, nh, nw)
            out.append((i, flip, src, p, golden["c%d_mid%d" % (i, flip)], golden["c%d_out%d" % (i, flip)]))
        i += 1
    assert i == 8
    return out


def in_layout(hwc, layout):
    t = torch.from_numpy(np.array(hwc, order="C"))      # (a copy: a flipped 1 x 1 array keeps its negative stride otherwise)
    return t if layout == "hwc" else t.permute(2, 0, 1).contiguous()


def as_hwc(a, layout):
    a = a.numpy() if torch.is_tensor(a) else a
    return a if layout == "hwc" else a.transpose(1, 2, 0)


# ---- the plan ---------------------------------------------------------------------------------------------------------------
def coco_cfg(**over):
    inp = dict(MIN_SIZE_TRAIN=(320, 352, 392, 416, 448, 480, 512, 544, 576, 608, 640), MAX_SIZE_TRAIN=1333,
               MIN_SIZE_TRAIN_SAMPLING="choice", CROP=SimpleNamespace(ENABLED=True, TYPE="absolute_range", SIZE=(384, 600)),
               COCO_PRETRAIN=True, PRETRAIN_SAME_CROP=False)
    inp.update(over)
    return SimpleNamespace(INPUT=SimpleNamespace(**inp))


def test_sample_coco_plan_draws_what_the_mapper_draws():
    rng = np.random.default_rng(11)
    cfg = coco_cfg()
    shorts = cfg.INPUT.MIN_SIZE_TRAIN
    cropped = flipped = frames = 0
    first_edges, independent = set(), 0
    for n in range(2000):
        h, w = ((480, 640), (427, 640), (640, 480), (333, 500))[n % 4]
        plans = clip_mapper.sample_coco_plan(cfg, (h, w), rng)
        assert len(plans) == 2 and all(isinstance(p, ChainPlan) for p in plans)
        independent += plans[0] != plans[1]
        for p in plans:
            assert (p.h, p.w) == (h, w)
            assert 0 <= p.x0 and 0 <= p.y0 and p.cw >= 1 and p.ch >= 1 and p.x0 + p.cw <= p.w1 and p.y0 + p.ch <= p.h1
            crop = (p.h1, p.w1, p.x0, p.y0, p.cw, p.ch) != (h, w, 0, 0, w, h)
            if crop:
                edge = [s for s in (400, 500, 600) if resize.shortest_edge_size(h, w, s, 2 ** 62) == (p.h1, p.w1)]
                assert edge, p
                first_edges.add(edge[0])
                assert min(p.h1, 384) <= p.ch <= min(p.h1, 600) and min(p.w1, 384) <= p.cw <= min(p.w1, 600)
            assert any(resize.shortest_edge_size(p.ch, p.cw, s, 1333) == (p.nh, p.nw) for s in shorts), p
            cropped += crop
            flipped += p.flip
            frames += 1
    assert frames == 4000 and 0.45 * frames <= cropped <= 0.55 * frames and 0.45 * frames <= flipped <= 0.55 * frames
    assert first_edges == {400, 500, 600} and independent > 1900        # key and reference are two draws
    same = coco_cfg(PRETRAIN_SAME_CROP=True)
    for _ in range(50):
        a, b = clip_mapper.sample_coco_plan(same, (480, 640), rng)
        assert a == b
    off = coco_cfg(CROP=SimpleNamespace(ENABLED=False, TYPE="absolute_range", SIZE=(384, 600)))
    for _ in range(200):
        for p in clip_mapper.sample_coco_plan(off, (480, 640), rng):
            assert (p.h1, p.w1, p.x0, p.y0, p.cw, p.ch) == (480, 640, 0, 0, 640, 480) and not p.resamples_twice
    assert len(clip_mapper.sample_coco_plan(cfg, (480, 640), rng, frames=3)) == 3
    for bad in (dict(AUGMENTATIONS=["rotation"]), dict(RANDOM_FLIP="vertical"),
                dict(CROP=SimpleNamespace(ENABLED=True, TYPE="relative_range", SIZE=(0.9, 0.9))),
                dict(MIN_SIZE_TRAIN_SAMPLING="choice_by_clip")):
        with pytest.raises(ValueError):
            clip_mapper.sample_coco_plan(coco_cfg(**bad), (480, 640), rng)


# ---- frames -----------------------------------------------------------------------------------------------------------------
def test_reference_chain_frames_equals_the_fixture_and_pillow(golden):
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for i, flip, src, p, mid, want in cases(golden):
        for layout in resize.LAYOUTS:
            got = augment.reference_chain_frames([in_layout(src, layout)], [p], layout)[0]
            assert torch.is_tensor(got) and got.dtype == torch.uint8
            assert np.array_equal(as_hwc(got, layout), want), (i, flip, layout)
        assert np.array_equal(augment.reference_chain_frames([src], [p], "hwc")[0], want)       # arrays stay arrays
        if Image is not None:                      # the literal order, by Pillow itself
            a = np.ascontiguousarray(np.flip(src, axis=1)) if flip else src
            big = np.asarray(Image.fromarray(a).resize((p.w1, p.h1), Image.BILINEAR))
            crop = np.ascontiguousarray(big[p.y0:p.y0 + p.ch, p.x0:p.x0 + p.cw])
            assert np.array_equal(crop, mid), (i, flip)
            assert np.array_equal(np.asarray(Image.fromarray(crop).resize((p.nw, p.nh), Image.BILINEAR)), want), (i, flip)


def staged_batch(golden, layout, device):
    """every case, flip off and on, as ONE step (cases that share a source share the tensor)"""
    listed = cases(golden)
    tensors = {}
    frames = [tensors.setdefault(int(golden["c%d_src" % i]), in_layout(src, layout)) for i, _, src, _, _, _ in listed]
    plans = [p for _, _, _, p, _, _ in listed]
    return listed, frames, plans, augment.stage_step(frames, plans, [], device, layout)


def test_the_cpu_route_of_the_ops_is_the_reference_route(golden):
    mean, std = [1.0, 2.0, 3.0], [2.0, 4.0, 8.0]
    for layout in resize.LAYOUTS:
        listed, frames, plans, staged = staged_batch(golden, layout, "cpu")
        assert augment.applies(frames, plans, "cpu", layout)
        twice = [p for p in plans if p.resamples_twice]
        assert len(twice) == 12 and tuple(staged.win_table.shape) == (12, 16) and staged.win_size == (64, 96)
        # four distinct sources, each uploaded once: the rows of the frames that share one name the same offset
        sizes = [3 * 37 * 53, 3 * 40 * 50, 3 * 33 * 47, 3 * 90 * 120]
        offs = np.cumsum([0] + [(s + 15) // 16 * 16 for s in sizes])
        slots = sum((3 * p.ch * p.cw + 15) // 16 * 16 for p in twice)
        assert staged.pixels.numel() == offs[-1] + slots
        assert sorted(set(staged.win_table[:, 0].tolist())) == offs[:4].tolist()
        calls, bytes_calls = dict(augment.CALLS), dict(augment.BYTES_CALLS)
        augment.resize_window_bytes(staged)
        for (i, flip, _, p, mid, _), row in zip(listed, staged.src_table.tolist()):
            if p.resamples_twice:                  # the slot holds the window of the UNFLIPPED resized frame
                o, h, w = row[:3]
                assert (h, w) == (p.ch, p.cw) and o >= offs[-1] and row[3:] == [0, 0, p.cw, p.ch, flip]
                got = staged.pixels[o:o + 3 * h * w].view((3, h, w) if layout == "chw" else (h, w, 3))
                assert np.array_equal(as_hwc(got, layout), np.flip(mid, axis=1) if flip else mid), (i, flip, layout)
            else:
                assert row[1:] == [p.h, p.w, p.mirrored_x0, p.y0, p.cw, p.ch, flip]
        x, mask = augment.augment_frames(staged, mean, std)
        assert augment.CALLS == calls and augment.BYTES_CALLS == bytes_calls      # (CPU tensors: no launch)
        assert tuple(x.shape) == (16, 3) + staged.size and staged.size == (64, 96)
        for k, (i, flip, _, p, _, want) in enumerate(listed):
            expect = (torch.from_numpy(want.transpose(2, 0, 1).astype(np.float32)) - torch.tensor(mean).view(3, 1, 1)) \
                / torch.tensor(std).view(3, 1, 1)
            assert torch.equal(x[k, :, :p.nh, :p.nw], expect), (i, flip, layout)
            assert not mask[k, :p.nh, :p.nw].any() and mask[k, p.nh:].all() and mask[k, :, p.nw:].all()
    # beyond the kernel's range on EITHER resample, a plan of another frame, a window outside (h1, w1), mixed kinds
    f = [torch.zeros(3, 400, 400, dtype=torch.uint8)]
    ok = ChainPlan(400, 400, False, 200, 200, 0, 0, 100, 100, 50, 50)
    assert augment.applies(f, [ok], "cpu")
    assert not augment.applies(f, [ok._replace(h1=40, w1=40, cw=30, ch=30)], "cpu")           # 10x on the first
    assert not augment.applies(f, [ok._replace(nh=9, nw=9)], "cpu")                           # 11x on the second
    assert not augment.applies(f, [ok._replace(h=401)], "cpu") and not augment.applies(f, [ok._replace(x0=101)], "cpu")
    assert not augment.applies(f * 2, [ok, augment.full_plan(400, 400, 200, 200)], "cpu")


# ---- polygons, boxes, ids ---------------------------------------------------------------------------------------------------
def rect(x0, y0, x1, y1):
    return [[float(x0), float(y0), float(x1), float(y0), float(x1), float(y1), float(x0), float(y1)]]


def test_polygons_boxes_and_ids_on_a_rectangle_that_is_exact_by_hand():
    """40 x 60 source, x2 -> (80, 120), window (20, 10, 60, 40), x1/2 -> (20, 30)"""
    p = ChainPlan(40, 60, False, 80, 120, 20, 10, 60, 40, 20, 30)
    inside = {"category_id": 3, "bbox": [10, 5, 20, 20], "segmentation": rect(10, 5, 30, 25)}
    outside = {"category_id": 4, "bbox": [50, 30, 8, 8], "segmentation": rect(50, 30, 58, 38)}
    crowd = {"category_id": 5, "bbox": [1, 1, 5, 5], "iscrowd": 1, "segmentation": rect(1, 1, 6, 6)}
    # x: 10..30 -> 20..60 -> 0..40 -> 0..20;  y: 5..25 -> 10..50 -> 0..40 -> 0..20
    assert augment.transform_polygons(inside["segmentation"], p)[0].tolist() == [0, 0, 20, 0, 20, 20, 0, 20]
    want = np.zeros((20, 30), dtype=bool)
    want[0:20, 0:20] = True
    assert np.array_equal(augment.reference_polygon_mask(inside["segmentation"], p), want)
    assert augment.chain_boxes([[10, 5, 30, 25]], p).tolist() == [[0, 0, 20, 20]]
    # flipped: x -> 60 - x: 30..50 -> 60..100 -> 40..80 -> 20..40, clipped to the 30 columns
    q = p._replace(flip=True)
    assert augment.transform_polygons(inside["segmentation"], q)[0].tolist() == [40, 0, 20, 0, 20, 20, 40, 20]
    want_q = np.zeros((20, 30), dtype=bool)
    want_q[0:20, 20:30] = True
    assert np.array_equal(augment.reference_polygon_mask(inside["segmentation"], q), want_q)
    boxes = augment.chain_boxes([[10, 5, 30, 25]], q)
    assert boxes.dtype == np.float32 and boxes.tolist() == [[20, 0, 30, 20]]
    # wholly outside the crop: x 50..58 -> 100..116 -> 80..96 -> 40..48: zero width after the clip
    boxes = augment.chain_boxes([[50, 30, 58, 38]], p)
    assert boxes.tolist() == [[30, 20, 30, 20]] and augment.boxes_nonempty(boxes).tolist() == [False]
    assert not augment.reference_polygon_mask(outside["segmentation"], p).any()
    assert augment.chain_boxes(np.zeros((0, 4)), p).shape == (0, 4)
    # the pair through the host route: the crowd has no slot, ids are 1..n, -1 where the box (or the mask) is empty
    image = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (3, 40, 60), dtype=np.uint8))
    entry = clip_mapper.stage_coco_pair(image, [inside, crowd, outside], [p, q], num_classes=80)
    assert entry["image"][0] is image and entry["image"][1] is image and entry["augment"] == [p, q]
    for fr, plan in zip(entry["instances"], (p, q)):
        assert fr["gt_ids"].tolist() == [1, 2] and fr["gt_ids"].dtype == torch.int64 and fr["gt_classes"].tolist() == [3, 4]
        assert fr["gt_bbox"].dtype == np.float64 and fr["gt_bbox"].tolist() == [[10, 5, 30, 25], [50, 30, 58, 38]]
        assert fr["gt_poly"] == [inside["segmentation"], outside["segmentation"]] and fr["gt_rle"] == [None, None]
        assert fr["image_size"] == (plan.nh, plan.nw)
    key, ref = frames_mod.host_augmented([entry])[0]["instances"]
    assert key["gt_ids"].tolist() == [1, -1] and ref["gt_ids"].tolist() == [1, -1]
    assert key["gt_boxes"].dtype == torch.float32 and key["gt_boxes"].tolist() == [[0, 0, 20, 20], [30, 20, 30, 20]]
    assert ref["gt_boxes"].tolist() == [[20, 0, 30, 20], [0, 20, 0, 20]]
    assert np.array_equal(key["gt_masks"].numpy(), np.stack([want, np.zeros_like(want)]))
    assert np.array_equal(ref["gt_masks"].numpy(), np.stack([want_q, np.zeros_like(want)]))
    host = frames_mod.host_augmented([entry])[0]["image"]
    assert all(torch.equal(a, b) for a, b in zip(host, augment.reference_chain_frames([image, image], [p, q])))


def test_stage_coco_pair_shares_one_upload_and_rle_slots_and_mixed_steps_take_the_host_route():
    image = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (3, 40, 60), dtype=np.uint8))
    crop, plain = ChainPlan(40, 60, True, 80, 120, 20, 10, 60, 40, 20, 30), augment.chain_full(40, 60, 20, 30, True)
    entry = clip_mapper.stage_coco_pair(image, [], [crop, plain], 80)
    staged = augment.stage_step(entry["image"], entry["augment"], [], "cpu")
    # one source upload of 7200 bytes, one slot of 3 * 40 * 60 behind it; both rows start from offset 0
    assert staged.pixels.numel() == 7200 + 7200 and staged.win_table[:, [0, 9]].tolist() == [[0, 7200]]
    assert staged.win_table[0, :9].tolist() == [0, 40, 60, 80, 120, 120 - 20 - 60, 10, 60, 40]          # the mirrored window
    assert staged.src_table.tolist() == [[7200, 40, 60, 0, 0, 60, 40, 1], [0, 40, 60, 0, 0, 60, 40, 1]]
    none = augment.stage_step([image, image], [plain, plain], [], "cpu")
    assert none.pixels.numel() == 7200 and tuple(none.win_table.shape) == (0, 16)
    # an RLE segmentation under a ChainPlan, and a step that mixes the two kinds of plan: the host route
    dense = np.zeros((40, 60), dtype=np.uint8)
    dense[5:25, 10:30] = 1
    from vnext_amd.utils.ytvis_json import rle_counts
    rle = {"category_id": 3, "bbox": [10, 5, 20, 20], "segmentation": {"size": [40, 60], "counts": rle_counts(dense).tolist()}}
    pair = clip_mapper.stage_coco_pair(image, [rle], [crop._replace(flip=False), plain], 80)
    assert pair["instances"][0]["gt_poly"] == [None] and pair["instances"][0]["gt_rle"][0] == rle_counts(dense).tolist()
    model = SimpleNamespace(device_augment=True, training=True, device=torch.device("cpu"))
    calls = (dict(augment.CALLS), dict(augment.BYTES_CALLS))
    out, pre = frames_mod.augment_step(model, [pair])
    assert pre is None and (augment.CALLS, augment.BYTES_CALLS) == calls
    key = out[0]["instances"][0]
    want = np.zeros((20, 30), dtype=bool)
    want[0:20, 0:20] = True                        # the rectangle of the test above, through NEAREST twice
    assert np.array_equal(key["gt_masks"][0].numpy(), want) and key["gt_ids"].tolist() == [1]
    clip = clip_mapper.stage_clip([image, image], [[], []], [augment.full_plan(40, 60, 20, 30)] * 2, 80)
    out, pre = frames_mod.augment_step(model, [entry, clip])
    assert pre is None and len(out) == 2 and tuple(out[0]["image"][0].shape) == (3, 20, 30)


# ---- the kernel -------------------------------------------------------------------------------------------------------------
def packed(golden, layout):
    """One pixel buffer for every case and flip: guard bytes, the four sources and then the slots, EACH at an odd byte
    offset with 0xAB between them; slots pre-filled with 0xCD.  -> (buffer, win rows [12, 16] with the coefficient
    triples, coeffs, [(case row, slot offset or None, source offset)], expected buffer after the launch)"""
    listed = cases(golden)
    chunks, at, src_off = [], 1, {}
    for k in range(4):
        src = in_layout(golden["src%d" % k], layout).reshape(-1)
        src_off[k] = at
        chunks.append((at, src))
        at += src.numel() + 2 + src.numel() % 2      # the next offset is odd again
    rows, where = [], []
    for i, flip, src, p, mid, _ in listed:
        k = int(golden["c%d_src" % i])
        if not p.resamples_twice:
            where.append((None, src_off[k]))
            continue
        rows.append([src_off[k], p.h, p.w, p.h1, p.w1, p.mirrored_x0, p.y0, p.cw, p.ch, at] + [0] * 6)
        where.append((at, src_off[k]))
        at += 3 * p.ch * p.cw + 2 + (3 * p.ch * p.cw) % 2
    buf = torch.full((at + 3,), 0xAB, dtype=torch.uint8)
    for o, t in chunks:
        buf[o:o + t.numel()] = t
    expect = buf.clone()
    for (i, flip, _, p, mid, _), (slot, _) in zip(listed, where):
        if slot is not None:
            assert slot % 2 == 1
            buf[slot:slot + 3 * p.ch * p.cw] = 0xCD
            want = in_layout(np.flip(mid, axis=1) if flip else mid, layout).reshape(-1)
            expect[slot:slot + want.numel()] = want
    words, win = augment.window_words(np.zeros(0, dtype=np.int32), rows)
    return buf, torch.from_numpy(win), torch.from_numpy(words), listed, where, expect


def c_window_bytes(buf, win, coeffs, H, W, layout):
    """the entry point on a copy of `buf` with guard bytes around it -> the buffer afterwards, on the host"""
    from vnext_amd import _lib
    whole = torch.full((buf.numel() + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    whole[GUARD:GUARD + buf.numel()] = buf.to(DEV)
    win, coeffs = win.to(DEV).contiguous(), coeffs.to(DEV).contiguous()
    rc = _lib.lib().vnx_resize_window_bytes(whole[GUARD:].data_ptr(), buf.numel(), win.data_ptr(), coeffs.data_ptr(),
                                            coeffs.numel(), win.shape[0], H, W, int(layout == "hwc"), _lib.current_stream(whole))
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().vnx_last_error()
    assert (whole[:GUARD] == 0x5A).all() and (whole[-GUARD:] == 0x5A).all(), "a byte outside the buffer was written"
    return whole[GUARD:GUARD + buf.numel()].cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", resize.LAYOUTS)
def test_window_bytes_equal_the_fixture_and_nothing_else_is_written(golden, layout):
    buf, win, coeffs, listed, where, expect = packed(golden, layout)
    H, W = resize.padded_size([(p.ch, p.cw) for _, _, _, p, _, _ in listed if p.resamples_twice])
    assert (H, W) == (64, 96) and win.shape[0] == 12
    got = c_window_bytes(buf, win, coeffs, H, W, layout)
    for (i, flip, _, p, _, _), (slot, _) in zip(listed, where):
        if slot is not None:
            n = 3 * p.ch * p.cw
            assert torch.equal(got[slot:slot + n], expect[slot:slot + n]), (i, flip, layout)
    assert torch.equal(got, expect)                # the sources, the bytes between the slots, the ends of the buffer
    # the second launch reads the slots (and, without a first resample, the sources): the chain's frames
    from test_train_augment_gpu import c_frames
    src = torch.tensor([(slot, p.ch, p.cw, 0, 0, p.cw, p.ch, flip) if slot is not None else
                        (off, p.h, p.w, p.mirrored_x0, p.y0, p.cw, p.ch, flip)
                        for (_, flip, _, p, _, _), (slot, off) in zip(listed, where)], dtype=torch.int32)
    plans = [p for _, _, _, p, _, _ in listed]
    dst = torch.tensor([(0, p.nh, p.nw) for p in plans], dtype=torch.int32)
    H2, W2 = augment.padded_size(plans)
    x, mask = c_frames(got, src, dst, torch.from_numpy(augment.coeff_words(plans)), len(plans), H2, W2, False, layout)
    for k, (i, flip, _, p, _, want) in enumerate(listed):
        assert torch.equal(x[k, :, :p.nh, :p.nw].cpu(), torch.from_numpy(want.transpose(2, 0, 1).astype(np.float32))), (i, flip)
        assert not mask[k, :p.nh, :p.nw].any() and mask[k, p.nh:].all() and mask[k, :, p.nw:].all()


@pytest.mark.gpu
def test_a_malformed_row_leaves_its_slot_untouched(golden):
    from vnext_amd import _lib
    for layout in resize.LAYOUTS:
        buf, win, coeffs, listed, where, expect = packed(golden, layout)
        n = buf.numel()
        slot0, bytes0 = int(win[0, 9]), 3 * int(win[0, 8]) * int(win[0, 7])
        bad = {  # word of row 0 -> value
            "the window leaves w1": (5, int(win[0, 4]) - int(win[0, 7]) + 1), "the window leaves h1": (6, int(win[0, 3])),
            "a negative origin": (5, -1), "an empty window": (7, 0), "wider than the launch": (7, 97),
            "a huge window": (8, 2 ** 31 - 1), "the slot ends outside the buffer": (9, n - bytes0 + 1),
            "a negative slot": (9, -3), "the slot overlaps the source": (9, int(win[0, 0]) + 7),
            "the source leaves the buffer": (0, n - 10), "a huge source": (1, 2 ** 31 - 1), "ksize 18": (12, 18),
            "ksize 0 on an axis that changes": (15, 0), "bounds outside coeffs": (10, coeffs.numel() - 3),
            "weights outside coeffs": (14, coeffs.numel() - 5), "a negative table": (13, -8), "h1 0": (3, 0),
        }
        for why, (word, value) in bad.items():
            rows = win.clone()
            rows[0, word] = value
            got = c_window_bytes(buf, rows, coeffs, 64, 96, layout)
            want = expect.clone()
            want[slot0:slot0 + bytes0] = 0xCD      # row 0 wrote nothing; every other row did its work
            assert torch.equal(got, want), (why, layout)
    lib = _lib.lib()
    assert lib.vnx_resize_window_bytes(None, 0, None, None, 0, 0, 64, 96, 0, None) == 0          # no rows: no launch
    assert lib.vnx_resize_window_bytes(None, 0, None, None, 0, 1, 64, 96, 0, None) != 0          # null pointers
    assert lib.vnx_resize_window_bytes(None, 0, None, None, 0, 0, 64, 90, 0, None) != 0          # not a multiple of 32
