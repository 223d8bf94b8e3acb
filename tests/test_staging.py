"""The host side of the frame front end (vnext_amd/ops/{ingest,resize,augment}.py): the coefficient-table builder behind
`resize.coeff_words`, `augment.coeff_words` and `augment.window_words`, and the one pack-and-upload under `ingest.stage_frames`,
`resize.stage_sources` and `augment.stage_step`.

Every check reads the staged buffers back THROUGH their offsets, as the kernels do, and compares with `resize.pillow_coeffs`,
`augment.nearest_table` and the source frames -- not with the packers.  What the kernels make of these buffers is held to
Pillow in tests/test_resize.py, test_augment.py, test_coco_pair.py and their GPU counterparts; that a chain step's rows name
the shared sources and that its slots hold the resized windows is also asserted on the fixture in
tests/test_coco_pair.py::test_the_cpu_route_of_the_ops_is_the_reference_route."""
import numpy as np
import pytest
import torch

from vnext_amd.ops import augment, ingest, resize
from vnext_amd.ops.augment import ChainPlan, FramePlan

# windows (ch x cw) -> targets (nh x nw): 12 x 9 -> 8 x 6 twice (every table shared), 7 x 9 -> 7 x 6 (the vertical axis keeps
# its size: no pass, but a nearest table)
PLANS = [FramePlan(1, 2, 9, 12, 8, 6, False), FramePlan(0, 0, 9, 12, 8, 6, True), FramePlan(3, 1, 9, 7, 7, 6, False)]
BILINEAR = [(9, 6), (12, 8)]                 # the distinct resamples, and the nearest tables
NEAREST = [(9, 6), (12, 8), (7, 7)]


def bilinear_words(pairs):
    return sum(b.size + k.size for b, k in (resize.pillow_coeffs(*p) for p in pairs))


def check_triple(words, triple, n_in, n_out):
    """a row's {bounds offset, weights offset, ksize} followed into the buffer"""
    at_b, at_k, ksize = (int(v) for v in triple)
    if n_in == n_out:
        assert (at_b, at_k, ksize) == (0, 0, 0)
        return
    bounds, kk = resize.pillow_coeffs(n_in, n_out)
    assert ksize == kk.shape[1] == resize.kernel_size(n_in, n_out)
    assert np.array_equal(words[at_b:at_b + 2 * n_out].reshape(n_out, 2), bounds)
    assert np.array_equal(words[at_k:at_k + n_out * ksize].reshape(n_out, ksize), kk)


def test_augment_coeff_rows_lead_to_pillows_tables_and_each_table_is_placed_once():
    words = augment.coeff_words(PLANS)
    assert words.dtype == np.int32 and words.ndim == 1
    rows = words[:8 * len(PLANS)].reshape(len(PLANS), 8)
    for row, p in zip(rows, PLANS):
        for j, (n_in, n_out) in enumerate(((p.cw, p.nw), (p.ch, p.nh))):      # horizontal, vertical
            check_triple(words, row[3 * j:3 * j + 3], n_in, n_out)
            at = int(row[6 + j])
            assert at >= rows.size and np.array_equal(words[at:at + n_out], augment.nearest_table(n_in, n_out))
    assert rows[2, 3:6].tolist() == [0, 0, 0]                                 # 7 -> 7
    assert rows[0].tolist() == rows[1].tolist() and rows[2, :3].tolist() == rows[0, :3].tolist()
    assert words.size == rows.size + bilinear_words(BILINEAR) + sum(n_out for _, n_out in NEAREST)


def test_resize_coeff_rows_lead_to_pillows_tables_and_each_table_is_placed_once():
    sizes, targets = [(p.ch, p.cw) for p in PLANS], [(p.nh, p.nw) for p in PLANS]
    words = resize.coeff_words(sizes, targets)
    assert words.dtype == np.int32 and words.ndim == 1
    rows = words[:6 * len(sizes)].reshape(len(sizes), 6)
    for row, (h, w), (nh, nw) in zip(rows, sizes, targets):
        check_triple(words, row[0:3], w, nw)
        check_triple(words, row[3:6], h, nh)
    assert rows[2, 3:6].tolist() == [0, 0, 0] and rows[0].tolist() == rows[1].tolist()
    assert words.size == rows.size + bilinear_words(BILINEAR)


def test_window_words_appends_each_first_resample_once_behind_an_untouched_prefix():
    words = augment.coeff_words(PLANS)
    before = words.copy()
    # {source offset, h, w, h1, w1, x0, y0, cw, ch, slot offset, 6 zeros}: both resample w = 9 -> 15; 12 -> 20 and 12 -> 12
    win = [[0, 12, 9, 20, 15, 1, 2, 9, 12, 512] + [0] * 6, [0, 12, 9, 12, 15, 0, 0, 9, 7, 1024] + [0] * 6]
    out, rows = augment.window_words(words, win)
    assert np.array_equal(words, before) and np.array_equal(out[:words.size], before)
    assert rows.dtype == np.int32 and tuple(rows.shape) == (2, 16) and rows[:, :10].tolist() == [r[:10] for r in win]
    for row in rows:
        check_triple(out, row[10:13], int(row[2]), int(row[4]))
        check_triple(out, row[13:16], int(row[1]), int(row[3]))
        assert int(row[10]) >= words.size
    assert rows[0, 10:13].tolist() == rows[1, 10:13].tolist() and rows[1, 13:16].tolist() == [0, 0, 0]
    assert out.size == words.size + bilinear_words([(9, 15), (12, 20)])
    same, none = augment.window_words(words, [])
    assert np.array_equal(same, before) and tuple(none.shape) == (0, 16)


# ---- the upload -------------------------------------------------------------------------------------------------------------
SIZES = [(5, 7), (6, 4)]


def sources(layout, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (3, h, w) if layout == "chw" else (h, w, 3), dtype=torch.uint8, generator=g)
            for h, w in SIZES]


def check_sources(pixels, rows, frames):
    """every frame's bytes stand at its row's offset, 16-byte aligned, inside `pixels`; -> the end of the last one"""
    assert pixels.dtype == torch.uint8 and pixels.dim() == 1
    end = 0
    for (o, h, w), f in zip(rows, frames):
        assert o % 16 == 0 and o >= end and o + f.numel() <= pixels.numel() and 3 * h * w == f.numel()
        assert torch.equal(pixels[o:o + f.numel()].view(f.shape), f)
        end = o + f.numel()
    return end


def test_stage_frames_puts_every_frame_at_its_rows_offset():
    frames = sources("chw")
    pixels, table = ingest.stage_frames(frames, "cpu")
    assert table.dtype == torch.int32 and [r[1:] for r in table.tolist()] == [list(s) for s in SIZES]
    check_sources(pixels, table.tolist(), frames)
    assert ingest.padded_size(frames) == ingest.padded_hw(SIZES) == (32, 32)


@pytest.mark.parametrize("layout", resize.LAYOUTS)
def test_stage_sources_puts_every_frame_at_its_rows_offset(layout):
    frames, targets = sources(layout), [(10, 14), (6, 3)]
    pixels, src, dst, coeffs = resize.stage_sources(frames, targets, "cpu", layout)
    assert src.dtype == dst.dtype == coeffs.dtype == torch.int32
    assert [r[1:] for r in src.tolist()] == [list(s) for s in SIZES] and dst.tolist() == [[0, 10, 14], [0, 6, 3]]
    check_sources(pixels, src.tolist(), frames)
    assert np.array_equal(coeffs.numpy(), resize.coeff_words(SIZES, targets))
    assert resize.padded_size(targets) == (32, 32)


@pytest.mark.parametrize("layout", resize.LAYOUTS)
def test_stage_step_of_frame_plans_puts_every_frame_at_its_rows_offset(layout):
    frames = sources(layout)
    plan = [FramePlan(1, 0, 5, 4, 8, 10, True), FramePlan(0, 2, 4, 3, 3, 4, False)]
    s = augment.stage_step(frames, plan, [(1, [5, 7, 12])], "cpu", layout, ids=[9])
    check_sources(s.pixels, [r[:3] for r in s.src_table.tolist()], frames)
    assert [r[3:] for r in s.src_table.tolist()] == [[1, 0, 5, 4, 1], [0, 2, 4, 3, 0]]
    assert s.dst_table.tolist() == [[0, 8, 10], [0, 3, 4]] and np.array_equal(s.coeffs.numpy(), augment.coeff_words(plan))
    assert s.ends.tolist() == [5, 12, 24] and s.mask_rows.tolist() == [[0, 3, 1, 0]] and s.ids.tolist() == [9]
    assert s.groups == ((0, 0, 8, 10), (0, 1, 3, 4)) and s.mask_bytes == 12 and s.size == (32, 32) and s.layout == layout
    # the tables `augment_masks` and `resize_window_bytes` read are always there
    assert torch.equal(s.mask_src, s.src_table) and torch.equal(s.mask_dst, s.dst_table)
    assert tuple(s.win_table.shape) == (0, 16) and s.win_table.dtype == torch.int32


@pytest.mark.parametrize("layout", resize.LAYOUTS)
def test_stage_step_of_chain_plans_stores_a_tensor_once_and_its_slots_behind_the_sources(layout):
    first, second = sources(layout)
    frames = [first, first, second, first]                  # one tensor three times (a pair of one image, and again)
    plan = [ChainPlan(5, 7, False, 10, 14, 2, 1, 9, 6, 4, 6), ChainPlan(5, 7, True, 8, 11, 1, 0, 7, 5, 5, 7),
            augment.chain_full(6, 4, 9, 6, True), ChainPlan(5, 7, True, 5, 7, 1, 1, 4, 3, 6, 8)]      # the last two: no slot
    boxes = np.arange(8, dtype=np.float32).reshape(2, 4)
    s = augment.stage_step(frames, plan, [(0, [35]), (3, [0, 35])], "cpu", layout, ids=[1, 2], boxes=boxes)
    # the two distinct tensors, once each, where the rows of the frames without a first resample and the window rows say
    assert s.src_table[2, :3].tolist() == [112, 6, 4] and s.src_table[3, :3].tolist() == [0, 5, 7]
    sources_end = check_sources(s.pixels, [(0, 5, 7), (112, 6, 4)], [first, second])
    assert s.src_table[3, 3:].tolist() == [7 - 1 - 4, 1, 4, 3, 1]                       # the mirrored window of the source
    assert tuple(s.win_table.shape) == (2, 16) and s.win_table[:, :5].tolist() == [[0, 5, 7, 10, 14], [0, 5, 7, 8, 11]]
    assert s.win_table[:, 5:9].tolist() == [[2, 1, 9, 6], [11 - 1 - 7, 0, 7, 5]] and s.win_size == (32, 32)
    # every slot: named by its window row AND its frame's row, aligned, behind the last source byte, inside pixels, disjoint
    end = sources_end
    for row, p, slot in zip(s.src_table[:2].tolist(), plan[:2], s.win_table[:, 9].tolist()):
        assert row == [slot, p.ch, p.cw, 0, 0, p.cw, p.ch, int(p.flip)]
        assert slot % 16 == 0 and slot >= end and slot + 3 * p.ch * p.cw <= s.pixels.numel()
        end = slot + 3 * p.ch * p.cw
    assert s.pixels.numel() == 112 + 80 + 176 + 112                                     # 16-byte steps of 105, 72, 162, 105
    words = s.coeffs.numpy()
    for row in s.win_table.tolist():
        check_triple(words, row[10:13], row[2], row[4])
        check_triple(words, row[13:16], row[1], row[3])
    assert np.array_equal(words[:augment.coeff_words(plan).size], augment.coeff_words(plan))
    assert torch.equal(s.boxes, torch.from_numpy(boxes)) and s.ids.tolist() == [1, 2]
    assert torch.equal(s.mask_src, s.src_table) and torch.equal(s.mask_dst, s.dst_table)
