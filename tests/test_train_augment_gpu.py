"""Training-time augmentation on the device (vnext_amd/csrc/augment.hip, vnext_amd/ops/augment.py).

The kernels are held EXACTLY (integer arithmetic: no tolerance) to `reference_augment_frames` / `reference_augment_masks`,
which tests/test_augment.py holds to Pillow; through the C ABI into pre-filled outputs with guard words around them.  The
models with the switch on see bit-identical network inputs and targets to the host route of the same plan.  No test here
imports Pillow.

Why the file's name sorts late: DESIGN section 19 ("Open: the graphed IDOL training trunk and torch's stream pool").  Under the
name test_augment_gpu.py this file ran first among the GPU tests that capture a graph, so ITS capture created torch's shared
capture stream -- the first draw from the stream pool instead of a later one -- and
tests/test_model_ddp.py::test_ddp_wrapper_over_rccl_on_one_gpu[IDOL-True], which shares no code with these tests, then failed
on the gradient of `level_embed` (two runs of two; it passed in the run without this file).  Sorted behind the tests that
capture training trunks, this file draws no stream of its own and leaves the pool's history as it was.
"""
import random

import numpy as np
import pytest
import torch

import vnext_amd.models  # noqa: F401  (registers the meta-archs)
from vnext_amd import train as T
from vnext_amd.data import clip_mapper
from vnext_amd.models import frames as frames_mod
from vnext_amd.ops import augment, resize
from vnext_amd.ops.augment import FramePlan
from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg
from vnext_amd.utils.ytvis_json import rle_counts

DEV = "cuda:0"
GUARD = 64
TINY_SEQ = {"MODEL.SeqFormer.ENC_LAYERS": 1, "MODEL.SeqFormer.DEC_LAYERS": 2, "MODEL.SeqFormer.NUM_OBJECT_QUERIES": 12,
            "MODEL.SeqFormer.DIM_FEEDFORWARD": 64, "MODEL.SeqFormer.DROPOUT": 0.0, "INPUT.SAMPLING_FRAME_NUM": 2}
TINY_IDOL = {"MODEL.IDOL.ENC_LAYERS": 1, "MODEL.IDOL.DEC_LAYERS": 2, "MODEL.IDOL.NUM_OBJECT_QUERIES": 110,
             "MODEL.IDOL.DIM_FEEDFORWARD": 64, "MODEL.IDOL.DROPOUT": 0.0}

# (source h, w), window (x0, y0, cw, ch), target (nh, nw), why
FRAME_CASES = [
    ((45, 70), (3, 5, 37, 29), (50, 64), "odd origin, two tiles on both axes"),
    ((45, 70), (3, 5, 63, 29), (50, 33), "mixed: up-scale vertically, down-scale horizontally"),
    ((300, 280), (7, 11, 264, 272), (34, 33), "8x: the limit; nw = 33: a second tile that holds one column"),
    ((40, 70), (2, 1, 64, 36), (18, 32), "nw = 32 exactly"),
    ((40, 50), (5, 3, 40, 30), (15, 40), "window as wide as its target: the horizontal pass is skipped"),
    ((37, 53), (12, 14, 41, 23), (20, 30), "the window ends at the source's last row and column, the buffer with the frame"),
]


def sources(sizes, seed, layout="chw"):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (3, h, w) if layout == "chw" else (h, w, 3), dtype=torch.uint8, generator=g)
            for h, w in sizes]


def in_layout(hwc, layout):
    return hwc.contiguous() if layout == "hwc" else hwc.permute(2, 0, 1).contiguous()


def as_chw(t, layout):
    return t if layout == "chw" else t.permute(2, 0, 1)


def pack(frames, first=1, tail=3):
    """the frames' bytes in one host buffer, every frame at an ODD byte offset (`first` for the first), `tail` spare bytes"""
    offs, off = [], first
    for f in frames:
        offs.append(off)
        off += f.numel()
        off += 1 - off % 2
    end = offs[-1] + frames[-1].numel() + tail
    buf = torch.full((end,), 0xAB, dtype=torch.uint8)
    for f, o in zip(frames, offs):
        buf[o:o + f.numel()] = f.reshape(-1)
    return buf, offs


def tables(frames, plan, layout, offs):
    sizes = [resize.frame_size(f, layout) for f in frames]
    src = torch.tensor([(o, h, w, p.x0, p.y0, p.cw, p.ch, int(p.flip)) for o, (h, w), p in zip(offs, sizes, plan)],
                       dtype=torch.int32)
    dst = torch.tensor([(0, p.nh, p.nw) for p in plan], dtype=torch.int32)
    return src, dst, torch.from_numpy(augment.coeff_words(plan))


def c_frames(buf, src, dst, coeffs, B, H, W, channels_last, layout, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0),
             symbol="vnx_augment_frames"):
    """the entry point into NaN / 0xFF pre-filled outputs with guard words around them -> x [B, 3, H, W], mask uint8 [B, H, W]"""
    from vnext_amd import _lib
    buf, src, dst, coeffs = (t.to(DEV) for t in (buf, src, dst, coeffs))
    xs = torch.full((B * 3 * H * W + 2 * GUARD,), float("nan"), device=DEV)
    ms = torch.full((B * H * W + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    _lib.check(getattr(_lib.lib(), symbol)(
        buf.data_ptr(), buf.numel(), src.data_ptr(), dst.data_ptr(), coeffs.data_ptr(), coeffs.numel(), B, H, W,
        *mean, *std, int(channels_last), int(layout == "hwc"), xs[GUARD:].data_ptr(), ms[GUARD:].data_ptr(),
        _lib.current_stream(buf)))
    torch.cuda.synchronize()
    assert torch.isnan(xs[:GUARD]).all() and torch.isnan(xs[-GUARD:]).all(), "x: a guard word was written"
    assert (ms[:GUARD] == 0xFF).all() and (ms[-GUARD:] == 0xFF).all(), "mask: a guard byte was written"
    x, mask = xs[GUARD:-GUARD], ms[GUARD:-GUARD].view(B, H, W)
    assert not torch.isnan(x).any(), "x: an element was not written"
    assert (mask <= 1).all(), "mask: an element was not written"
    x = x.view(B, H, W, 3).permute(0, 3, 1, 2) if channels_last else x.view(B, 3, H, W)
    return x, mask


def padded(frames_chw, size):
    H, W = size
    x = torch.zeros(len(frames_chw), 3, H, W)
    mask = torch.ones(len(frames_chw), H, W, dtype=torch.bool)
    for i, f in enumerate(frames_chw):
        x[i, :, :f.shape[1], :f.shape[2]] = f.float()
        mask[i, :f.shape[1], :f.shape[2]] = False
    return x, mask


# ---- frames -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", FRAME_CASES, ids=["%dx%d_%dx%d" % (c[0] + c[2]) for c in FRAME_CASES])
def test_augmented_frames_are_exact(case):
    (h, w), (x0, y0, cw, ch), (nh, nw), why = case
    last = "buffer" in why
    hwc = sources([(h, w)], seed=31, layout="hwc")[0]
    H, W = resize.padded_size([(nh, nw)])
    for layout in resize.LAYOUTS:
        frame = in_layout(hwc, layout)
        buf, offs = pack([frame], first=2 if last else 1, tail=0 if last else 3)
        assert not last or (buf.numel() % 4 != 0 and offs[0] + frame.numel() == buf.numel())
        for flip in (False, True):
            plan = [FramePlan(x0, y0, cw, ch, nh, nw, flip)]
            want, want_mask = padded([as_chw(augment.reference_augment_frames([frame], plan, layout)[0], layout)], (H, W))
            src, dst, coeffs = tables([frame], plan, layout, offs)
            for channels_last in (False, True):
                x, mask = c_frames(buf, src, dst, coeffs, 1, H, W, channels_last, layout)
                assert torch.equal(x.cpu(), want), (layout, flip, channels_last)
                assert torch.equal(mask.cpu().bool(), want_mask), (layout, flip, channels_last)


@pytest.mark.gpu
def test_two_frames_with_different_windows_and_targets_and_a_window_outside_its_frame():
    sizes = [(45, 70), (40, 50), (33, 47), (33, 47)]
    plan = [FramePlan(3, 5, 37, 29, 50, 64, True), FramePlan(5, 3, 40, 30, 15, 40, False),
            FramePlan(20, 0, 28, 33, 20, 17, False),       # x0 + cw = 48 > 47: leaves the frame
            FramePlan(0, 2, 47, 32, 20, 29, True)]         # y0 + ch = 34 > 33
    for layout in resize.LAYOUTS:
        frames = sources(sizes, seed=32, layout=layout)
        buf, offs = pack(frames)
        src, dst, coeffs = tables(frames, plan, layout, offs)
        good = [as_chw(f, layout) for f in augment.reference_augment_frames(frames[:2], plan[:2], layout)]
        want, want_mask = padded(good, (64, 64))
        for channels_last in (False, True):
            x, mask = c_frames(buf, src, dst, coeffs, 4, 64, 64, channels_last, layout)
            assert torch.equal(x[:2].cpu(), want) and torch.equal(mask[:2].cpu().bool(), want_mask)
            assert (x[2:] == 0).all() and (mask[2:] == 1).all()               # all padding (the guards were checked)
        # negative origins and sizes, a window larger than the frame
        for bad in ((-1, 0, 10, 10), (0, -3, 10, 10), (0, 0, 0, 10), (0, 0, 71, 10), (2 ** 31 - 1, 0, 37, 29)):
            src2 = src.clone()
            src2[0, 3:7] = torch.tensor(bad, dtype=torch.int32)
            x, mask = c_frames(buf, src2, dst, coeffs, 4, 64, 64, False, layout)
            assert (x[0] == 0).all() and (mask[0] == 1).all() and torch.equal(x[1].cpu(), want[1])


@pytest.mark.gpu
def test_a_full_window_without_flip_equals_resize_ingest_frames_bit_for_bit():
    sizes, targets = [(37, 53), (19, 27), (33, 47), (150, 260)], [(19, 27), (37, 53), (33, 47), (75, 130)]
    cfg = get_seqformer_cfg(**{"MODEL.DEVICE": "cpu"})
    mean = torch.tensor(cfg.MODEL.PIXEL_MEAN, dtype=torch.float32).tolist()
    std = torch.tensor(cfg.MODEL.PIXEL_STD, dtype=torch.float32).tolist()
    H, W = resize.padded_size(targets)
    for layout in resize.LAYOUTS:
        frames = sources(sizes, seed=33, layout=layout)
        buf, offs = pack(frames)
        plan = [augment.full_plan(h, w, nh, nw) for (h, w), (nh, nw) in zip(sizes, targets)]
        src, dst, coeffs = tables(frames, plan, layout, offs)
        old_coeffs = torch.from_numpy(resize.coeff_words(sizes, targets))
        for channels_last in (False, True):
            x, mask = c_frames(buf, src, dst, coeffs, 4, H, W, channels_last, layout, mean, std)
            want, want_mask = c_frames(buf, src[:, :3].contiguous(), dst, old_coeffs, 4, H, W, channels_last, layout, mean, std,
                                       symbol="vnx_resize_ingest_frames")
            assert torch.equal(x, want) and torch.equal(mask, want_mask)


# ---- masks ------------------------------------------------------------------------------------------------------------------
def c_masks(ends, rows, src, dst, coeffs, H, W, mask_bytes):
    """vnx_augment_masks into pre-filled, guarded outputs -> (masks uint8 [mask_bytes], boxes [m, 4], nonempty uint8 [m]) on
    the host"""
    from vnext_amd import _lib
    lib = _lib.lib()
    ends, rows, src, dst, coeffs = (t.to(DEV) for t in (ends, rows, src, dst, coeffs))
    m = rows.shape[0]
    ms = torch.full((mask_bytes + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    bs = torch.full((4 * m + 2 * GUARD,), float("nan"), device=DEV)
    ns = torch.full((m + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    work = torch.full((int(lib.vnx_augment_masks_workspace(m, H, W)) + 2 * GUARD,), 0xCD, dtype=torch.uint8, device=DEV)
    _lib.check(lib.vnx_augment_masks(ends.data_ptr(), ends.numel(), rows.data_ptr(), m, src.data_ptr(), dst.data_ptr(),
                                     coeffs.data_ptr(), coeffs.numel(), src.shape[0], H, W, ms[GUARD:].data_ptr(), mask_bytes,
                                     bs[GUARD:].data_ptr(), ns[GUARD:].data_ptr(), work[GUARD:].data_ptr(),
                                     work.numel() - 2 * GUARD, _lib.current_stream(ends)))
    torch.cuda.synchronize()
    assert (ms[:GUARD] == 0xFF).all() and (ms[-GUARD:] == 0xFF).all(), "masks: a guard byte was written"
    assert torch.isnan(bs[:GUARD]).all() and torch.isnan(bs[-GUARD:]).all(), "boxes: a guard word was written"
    assert (ns[:GUARD] == 0xFF).all() and (ns[-GUARD:] == 0xFF).all(), "nonempty: a guard byte was written"
    assert (work[:GUARD] == 0xCD).all() and (work[-GUARD:] == 0xCD).all(), "workspace: a guard byte was written"
    return ms[GUARD:GUARD + mask_bytes].cpu(), bs[GUARD:GUARD + 4 * m].view(m, 4).cpu(), ns[GUARD:GUARD + m].cpu()


def mask_step(flip):
    """four frames: one with the edge cases, one with NO masks, the 40 x 40 checkerboard, a mask of 10 000 runs at 8x
    -> (sizes, plan, masks [(frame, counts)], names)"""
    sizes = [(45, 70), (33, 47), (40, 40), (300, 280)]
    plan = [FramePlan(3, 5, 37, 29, 50, 64, flip), FramePlan(0, 0, 47, 33, 20, 29, flip),
            FramePlan(4, 2, 33, 35, 21, 27, flip), FramePlan(7, 11, 264, 272, 34, 33, flip)]
    h, w = sizes[0]
    zero = np.zeros((h, w), dtype=np.uint8)
    corner, outside = zero.copy(), zero.copy()
    corner[5 + 29 - 1, 3 + 37 - 1] = 1                     # the window's last row and column
    outside[36:44, 45:69] = 1
    outside[0:4, 0:2] = 1
    span = [10 * h + 7, 6 * h + 13, h * w - 16 * h - 20]   # one run over columns 10 .. 16
    rng = np.random.default_rng(9)
    noise = (rng.random((h, w)) < 0.4).astype(np.uint8)
    noise[:, 0] = 1                                        # starts with a 1: the first count is 0
    nc = rle_counts(noise).tolist()
    assert nc[0] == 0
    gaps = nc[:7] + [0, 0] + nc[7:20] + [0, 0, 0, 0] + nc[20:]      # zero-length runs in the middle: the same mask
    yy, xx = np.mgrid[:40, :40]
    checker = rle_counts(((yy + xx) & 1).astype(np.uint8)).tolist()
    assert len(checker) > 1500
    big = (np.random.default_rng(10).random((300, 280)) < 0.5).astype(np.uint8)
    bigc = rle_counts(big).tolist()
    assert len(bigc) > 30000                               # a tile's slice is beyond what LDS holds: the search in memory
    masks = [(0, [h * w]), (0, [0, h * w]), (0, rle_counts(corner).tolist()), (0, rle_counts(outside).tolist()), (0, span),
             (0, nc), (0, gaps), (2, checker), (3, bigc), (3, [300 * 280])]
    names = ["n_runs 1", "full", "corner pixel", "outside the window", "a run over columns", "noise", "zero-length runs",
             "checkerboard", "30 000 runs", "empty at 8x"]
    return sizes, plan, masks, names


def mask_tables(sizes, plan, masks):
    src = torch.tensor([(0, h, w, p.x0, p.y0, p.cw, p.ch, int(p.flip)) for (h, w), p in zip(sizes, plan)], dtype=torch.int32)
    dst = torch.tensor([(0, p.nh, p.nw) for p in plan], dtype=torch.int32)
    rows, ends, e_at, o_at = [], [], 0, 0
    for f, counts in masks:
        e = np.cumsum(np.asarray(counts, dtype=np.int64)).astype(np.int32)
        rows.append((e_at, e.size, f, o_at))
        ends.append(e)
        e_at += e.size
        o_at += plan[f].nh * plan[f].nw
    return (torch.from_numpy(np.concatenate(ends)), torch.tensor(rows, dtype=torch.int32), src, dst,
            torch.from_numpy(augment.coeff_words(plan)), o_at)


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flipped"])
def test_augmented_masks_and_boxes_are_exact(flip):
    sizes, plan, masks, names = mask_step(flip)
    want, want_boxes, want_flags = augment.reference_augment_masks(masks, sizes, plan)
    assert want_flags.tolist() == [False, True, True, False, True, True, True, True, True, False]
    assert np.array_equal(want[5], want[6])                # the zero-length runs change nothing
    ends, rows, src, dst, coeffs, mask_bytes = mask_tables(sizes, plan, masks)
    H, W = resize.padded_size([(p.nh, p.nw) for p in plan])
    got, boxes, flags = c_masks(ends, rows, src, dst, coeffs, H, W, mask_bytes)
    assert (got <= 1).all(), "masks: a byte was not written"
    for name, (o, _, f, at), m in zip(names, rows.tolist(), want):
        nh, nw = plan[f].nh, plan[f].nw
        assert np.array_equal(got[at:at + nh * nw].view(nh, nw).numpy().astype(bool), m), name
    assert np.array_equal(boxes.numpy(), want_boxes) and flags.tolist() == want_flags.astype(int).tolist()
    assert boxes[3].tolist() == [0, 0, 0, 0] and flags[3] == 0      # outside the window: empty, a zero box (its id becomes -1)
    again, boxes2, flags2 = c_masks(ends, rows, src, dst, coeffs, H, W, mask_bytes)      # run twice: the same bytes
    assert torch.equal(got, again) and torch.equal(boxes.view(torch.int32), boxes2.view(torch.int32)) and torch.equal(flags, flags2)


@pytest.mark.gpu
def test_malformed_runs_are_empty_masks_and_no_masks_is_no_launch():
    from vnext_amd import _lib
    sizes, plan, masks, _ = mask_step(False)
    masks = masks[:5] + [(0, [100, 50])]                  # a last end that is not h * w, at the END of the buffer
    want, want_boxes, want_flags = augment.reference_augment_masks(masks, sizes, plan)
    assert not want_flags[5] and not want[5].any()
    ends, rows, src, dst, coeffs, mask_bytes = mask_tables(sizes, plan, masks)
    H, W = resize.padded_size([(p.nh, p.nw) for p in plan])
    rows[1, 1] = 10 ** 6                                   # runs that would end far outside `ends`
    rows[2, 0] = -5                                        # a negative offset
    got, boxes, flags = c_masks(ends, rows, src, dst, coeffs, H, W, mask_bytes)
    n = 50 * 64
    assert (got.view(6, n)[[1, 2, 5]] == 0).all() and flags[[1, 2, 5]].tolist() == [0, 0, 0] and (boxes[[1, 2, 5]] == 0).all()
    assert np.array_equal(got.view(6, n)[4].view(50, 64).numpy().astype(bool), want[4]) and flags[4] == 1
    # a row that names no frame / an output outside `masks`: nothing written for it (the guards were checked), a zero box
    rows2 = rows.clone()
    rows2[3, 2] = 9
    rows2[4, 3] = mask_bytes - 10
    got2, boxes2, flags2 = c_masks(ends, rows2, src, dst, coeffs, H, W, mask_bytes)
    assert (got2.view(6, n)[3] == 0xFF).all() and flags2[[3, 4]].tolist() == [0, 0] and (boxes2[[3, 4]] == 0).all()
    assert torch.equal(got2.view(6, n)[0], got.view(6, n)[0])
    # n = 0: VNX_OK with nothing to read or write
    assert _lib.lib().vnx_augment_masks(None, 0, None, 0, None, None, None, 0, 0, 64, 64, None, 0, None, None, None, 0, None) == 0


@pytest.mark.gpu
def test_the_python_ops_stage_one_buffer_and_count_their_calls():
    sizes, plan, masks, _ = mask_step(True)
    for layout in resize.LAYOUTS:
        frames = sources(sizes, seed=34, layout=layout)
        staged = augment.stage_step(frames, plan, masks, DEV, layout, ids=list(range(10, 20)))
        assert all(t.is_cuda for t in staged[:7]) and staged.size == (64, 64)
        calls = dict(augment.CALLS)
        x, mask = augment.augment_frames(staged, [0.0] * 3, [1.0] * 3)
        flat, boxes, nonempty = augment.augment_masks(staged)
        assert augment.CALLS == {"augment_frames": calls["augment_frames"] + 1, "augment_masks": calls["augment_masks"] + 1}
        want, want_mask = padded([as_chw(f, layout) for f in augment.reference_augment_frames(frames, plan, layout)], (64, 64))
        assert torch.equal(x.cpu(), want) and torch.equal(mask.cpu(), want_mask)
        outs, want_boxes, flags = augment.reference_augment_masks(masks, sizes, plan)
        views = staged.mask_views(flat)
        assert [v.shape[0] for v in views] == [7, 0, 1, 2]
        assert all(np.array_equal(m.cpu().numpy(), o) for m, o in zip([m for v in views for m in v], outs))
        assert np.array_equal(boxes.cpu().numpy(), want_boxes) and nonempty.cpu().tolist() == flags.tolist()
    empty = augment.stage_step(frames, plan, [], DEV, layout)      # a step without a single mask
    calls = augment.CALLS["augment_masks"]
    flat, boxes, nonempty = augment.augment_masks(empty)
    assert flat.numel() == 0 and tuple(boxes.shape) == (0, 4) and augment.CALLS["augment_masks"] == calls


@pytest.mark.gpu
def test_both_ops_captured_in_a_graph_replay_on_other_pixels_runs_and_plans():
    """one graph: capture a step, overwrite pixels, tables, coefficients and runs in place with ANOTHER step of the same
    padded size and buffer sizes, poison the outputs, replay"""
    from vnext_amd import _lib
    lib = _lib.lib()
    sizes = [(45, 70), (40, 40)]
    def step(seed, plan, shift):
        frames = sources(sizes, seed=seed)
        yy, xx = np.mgrid[:45, :70]
        a = (((yy + shift) // 7 + xx // 9) & 1).astype(np.uint8)
        b = ((np.mgrid[:40, :40][0] + shift) % 5 < 2).astype(np.uint8)
        masks = [(0, rle_counts(a).tolist()), (1, rle_counts(b).tolist()), (1, [1600])]
        return frames, plan, masks
    first = step(41, [FramePlan(3, 5, 37, 29, 50, 64, False), FramePlan(4, 2, 33, 35, 21, 27, True)], 0)
    second = step(42, [FramePlan(1, 2, 60, 40, 33, 50, True), FramePlan(0, 0, 40, 40, 64, 64, False)], 3)
    def staged_host(frames, plan, masks):
        s = augment.stage_step(frames, plan, masks, "cpu")
        return s, [s.pixels, s.src_table, s.dst_table, s.coeffs, s.ends, s.mask_rows]
    s1, t1 = staged_host(*first)
    s2, t2 = staged_host(*second)
    assert s1.size == s2.size == (64, 64)
    room = [max(a.numel(), b.numel()) for a, b in zip(t1, t2)]      # static buffers both steps fit in
    bufs = [torch.zeros(n, dtype=a.dtype, device=DEV) for n, a in zip(room, t1)]
    def load(tensors):
        for b, t in zip(bufs, tensors):
            b.zero_()
            b[:t.numel()].copy_(t.reshape(-1))
    m, mask_room = 3, max(s1.mask_bytes, s2.mask_bytes)
    x = torch.full((2, 3, 64, 64), float("nan"), device=DEV)
    mask = torch.full((2, 64, 64), 0xFF, dtype=torch.uint8, device=DEV)
    gm = torch.full((mask_room,), 0xFF, dtype=torch.uint8, device=DEV)
    boxes = torch.full((m, 4), float("nan"), device=DEV)
    flags = torch.full((m,), 0xFF, dtype=torch.uint8, device=DEV)
    work = torch.empty(int(lib.vnx_augment_masks_workspace(m, 64, 64)), dtype=torch.uint8, device=DEV)
    load(t1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stream = _lib.current_stream(x)
        _lib.check(lib.vnx_augment_frames(bufs[0].data_ptr(), bufs[0].numel(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                                          bufs[3].data_ptr(), bufs[3].numel(), 2, 64, 64, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0, 0,
                                          x.data_ptr(), mask.data_ptr(), stream))
        _lib.check(lib.vnx_augment_masks(bufs[4].data_ptr(), bufs[4].numel(), bufs[5].data_ptr(), m, bufs[1].data_ptr(),
                                         bufs[2].data_ptr(), bufs[3].data_ptr(), bufs[3].numel(), 2, 64, 64, gm.data_ptr(),
                                         gm.numel(), boxes.data_ptr(), flags.data_ptr(), work.data_ptr(), work.numel(), stream))
    for (frames, plan, masks), tensors, s in ((second, t2, s2), (first, t1, s1)):
        load(tensors)
        for t in (x, boxes):
            t.fill_(float("nan"))
        for t in (mask, gm, flags):
            t.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        want, want_mask = padded(augment.reference_augment_frames(frames, plan), (64, 64))
        assert torch.equal(x.cpu(), want) and torch.equal(mask.cpu().bool(), want_mask)
        outs, want_boxes, want_flags = augment.reference_augment_masks(masks, sizes, plan)
        got = gm.cpu()
        for (_, _, f, at), o in zip(s.mask_rows.tolist(), outs):
            assert np.array_equal(got[at:at + o.size].view(o.shape).numpy().astype(bool), o)
        assert np.array_equal(boxes.cpu().numpy(), want_boxes) and flags.cpu().tolist() == want_flags.astype(int).tolist()


# ---- the models -------------------------------------------------------------------------------------------------------------
class Spy:
    """what enters the backbone (x) and the transformer (masks, positions) on every forward, and what `prepare_targets` gave"""

    def __init__(self, model):
        self.seen, self.targets, self.hooks = [], [], []
        d = model.detr.detr
        self.hooks.append(d.backbone.register_forward_pre_hook(lambda m, args: self.seen.append(args[0].detach().clone())))
        self.hooks.append(d.transformer.register_forward_pre_hook(
            lambda m, args: self.seen.extend(t.detach().clone() for t in list(args[1]) + list(args[2]))))
        inner = model.prepare_targets

        def recording(batched_inputs):
            out = inner(batched_inputs)
            self.targets.append(out)
            return out
        model.prepare_targets = recording

    def take(self):
        out, self.seen, self.targets = (self.seen, self.targets), [], []
        return out


def flat_targets(t):
    """the tensors of a `prepare_targets` result, in order (lists / tuples / dicts of tensors)"""
    if torch.is_tensor(t):
        return [t]
    if isinstance(t, dict):
        return [v for k in sorted(t) for v in flat_targets(t[k])]
    if isinstance(t, (list, tuple)):
        return [v for item in t for v in flat_targets(item)]
    return []


def rectangle(h, w, y, x, dy, dx):
    m = np.zeros((h, w), dtype=np.uint8)
    m[y:y + dy, x:x + dx] = 1
    return rle_counts(m).tolist()


def training_clips(n_clips, n_frames, plans, seed):
    """clips of 96 x 160 source frames with two instances each (the second is absent from every frame but the first: the
    dummy annotation, n_runs 1, id -1; a crop that misses it on the first frame empties it there as well)"""
    clips = []
    for c in range(n_clips):
        frames = sources([(96, 160)] * n_frames, seed=seed + c)
        annos = []
        for t in range(n_frames):
            annos.append([{"id": 11, "category_id": 3 + c, "segmentation": rectangle(96, 160, 20 + t, 40 + 2 * t, 40, 60)},
                          {"id": 12, "category_id": 7, "segmentation": rectangle(96, 160, 60, 4, 20, 10 if t == 0 else 0)}])
        clips.append(clip_mapper.stage_clip(frames, annos, plans[c], 40))
    return clips


def step_both_routes(model, clips):
    """one training step through the device route and through the host route of the same plan -> the two loss dicts"""
    T.enable_device_ingest(model)
    spy = Spy(model)
    results = []
    for route in ("device", "host"):
        torch.manual_seed(7)
        random.seed(7)
        np.random.seed(7)
        calls = dict(augment.CALLS)
        if route == "device":
            T.enable_device_augment(model)
            losses = model(clips)
            T.enable_device_augment(model, on=False)
            ran = int(next(model.parameters()).is_cuda)      # (on the CPU the ops take their reference route: no launch)
            assert augment.CALLS == {k: v + ran for k, v in calls.items()}      # one call each for the whole step
        else:
            losses = model(frames_mod.host_augmented(clips))
            assert augment.CALLS == calls
        results.append((spy.take(), {k: float(v.detach()) for k, v in losses.items()}))
    ((seen_d, targets_d), loss_d), ((seen_h, targets_h), loss_h) = results
    assert len(seen_d) == len(seen_h) > 0
    for a, b in zip(seen_d, seen_h):
        assert a.dtype == b.dtype and torch.equal(a, b)                       # x, the level masks and positions
    td, th = flat_targets(targets_d), flat_targets(targets_h)
    assert len(td) == len(th) > 0
    for a, b in zip(td, th):
        assert a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())           # labels, boxes, masks, ids
    assert set(loss_d) == set(loss_h)
    for k in loss_h:      # the loss tolerance tests/test_ingest.py uses for its own on / off pair
        np.testing.assert_allclose(loss_d[k], loss_h[k], rtol=2e-4, atol=1e-5, err_msg=k)


@pytest.mark.gpu
def test_seqformer_training_step_with_the_switch_equals_the_host_route():
    torch.manual_seed(5)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": DEV, **TINY_SEQ})).train()
    plans = [[augment.full_plan(96, 160, 60, 100, True)] * 2, [augment.full_plan(96, 160, 60, 100, False)] * 2]
    step_both_routes(model, training_clips(2, 2, plans, seed=50))


@pytest.mark.gpu
def test_idol_training_step_with_the_switch_equals_the_host_route():
    torch.manual_seed(6)
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": DEV, **TINY_IDOL})).train()
    plans = [[FramePlan(16, 8, 120, 80, 64, 96, True), FramePlan(0, 0, 160, 96, 60, 100, True)],      # crops differ per frame
             [FramePlan(10, 0, 140, 88, 88, 140, False), FramePlan(20, 12, 128, 80, 70, 112, False)]]
    step_both_routes(model, training_clips(2, 2, plans, seed=60))
