"""Colour augmentation on the device (vnext_amd/csrc/augment.hip, resize_body.h; vnext_amd/ops/augment.py).

`vnx_augment_frames_color` is held EXACTLY -- no tolerance -- to tests/golden/augment_color.npz (the three steps in numpy on
Pillow-resized frames; tools/make_golden_augment_color.py), through the C ABI into pre-filled outputs with guards around
them and a pre-filled workspace: every subset of the three steps, both output layouts, both source layouts.  The shapes are
the smallest at which this can go wrong: three frames of different targets in one step (the mean must ignore the padding and
the other frames), 70 x 45 (six tiles feed one mean), 24 x 34 with crop and flip, one pixel, all 255 at w = 1.1, all zero,
the weights 0.9 and 1.1 exactly.  The file sorts next to tests/test_train_augment_gpu.py, for the reason given there.
"""
import os

import numpy as np
import pytest
import torch

import test_train_augment_gpu as base
from conftest import GOLDEN_DIR
from vnext_amd import train as T
from vnext_amd.ops import augment, resize
from vnext_amd.ops.augment import FramePlan
from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg

DEV = base.DEV
GUARD = base.GUARD
SUBSETS = list(range(1, 8))      # 1 brightness | 2 contrast | 4 saturation


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN_DIR, "augment_color.npz")))


def plan_of(golden, i, subset, weights=None):
    x0, y0, cw, ch, nh, nw, flip = (int(v) for v in golden["c%d_plan" % i])
    w = golden["c%d_weights" % i].tolist() if weights is None else weights
    return FramePlan(x0, y0, cw, ch, nh, nw, bool(flip), *(w[j] if subset >> j & 1 else None for j in range(3)))


def step_of(golden, cases, subset, layout, weights=None):
    """-> (frames of `layout`, plan)"""
    frames = [base.in_layout(torch.from_numpy(golden["c%d_src" % i]), layout) for i in cases]
    return frames, [plan_of(golden, i, subset, weights) for i in cases]


def host_tables(frames, plan, layout):
    """the frames at 16-byte offsets, the workspace behind them -> (buffer with GUARD bytes behind the workspace, pixel bytes,
    workspace offset, src, dst, coeffs, colour table)"""
    offs, off = [], 0
    for f in frames:
        offs.append(off)
        off += (f.numel() + 15) // 16 * 16
    H, W = resize.padded_size([(p.nh, p.nw) for p in plan])
    work = augment.color_workspace(len(frames), H, W)
    buf = torch.full((off + work + GUARD,), 0xCD, dtype=torch.uint8)      # the workspace starts as garbage: nothing relies on zeros
    for f, o in zip(frames, offs):
        buf[o:o + f.numel()] = f.reshape(-1)
    src, dst, coeffs = base.tables(frames, plan, layout, offs)
    return buf, off + work, off, src, dst, coeffs, torch.from_numpy(augment.color_words(plan))


def c_color(tabs, B, H, W, channels_last, layout, contrast, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
    """vnx_augment_frames_color into NaN / 0xFF pre-filled outputs with guards -> x [B, 3, H, W], mask uint8 [B, H, W]"""
    from vnext_amd import _lib
    buf, pixel_bytes, work_at, src, dst, coeffs, color = (t.to(DEV) if torch.is_tensor(t) else t for t in tabs)
    xs = torch.full((B * 3 * H * W + 2 * GUARD,), float("nan"), device=DEV)
    ms = torch.full((B * H * W + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().vnx_augment_frames_color(
        buf.data_ptr(), pixel_bytes, src.data_ptr(), dst.data_ptr(), coeffs.data_ptr(), coeffs.numel(), color.data_ptr(),
        B, H, W, *mean, *std, int(channels_last), int(layout == "hwc"), int(contrast), work_at, xs[GUARD:].data_ptr(),
        ms[GUARD:].data_ptr(), _lib.current_stream(buf)))
    torch.cuda.synchronize()
    assert torch.isnan(xs[:GUARD]).all() and torch.isnan(xs[-GUARD:]).all(), "x: a guard word was written"
    assert (ms[:GUARD] == 0xFF).all() and (ms[-GUARD:] == 0xFF).all(), "mask: a guard byte was written"
    assert (buf[pixel_bytes:] == 0xCD).all(), "pixels: a byte behind the workspace was written"
    assert torch.equal(buf[:work_at].cpu(), tabs[0][:work_at]), "pixels: a source byte was written"
    if not contrast:
        assert (buf[work_at:] == 0xCD).all(), "one launch: the workspace is not touched"
    x, mask = xs[GUARD:-GUARD], ms[GUARD:-GUARD].view(B, H, W)
    assert not torch.isnan(x).any(), "x: an element was not written"
    assert (mask <= 1).all(), "mask: an element was not written"
    x = x.view(B, H, W, 3).permute(0, 3, 1, 2) if channels_last else x.view(B, 3, H, W)
    return x, mask


def expected(golden, cases, subset, size):
    return base.padded([torch.from_numpy(golden["c%d_s%d" % (i, subset)]).permute(2, 0, 1) for i in cases], size)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", resize.LAYOUTS)
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("subset", SUBSETS)
def test_device_frames_equal_the_fixture_exactly(golden, subset, channels_last, layout):
    contrast = bool(subset & 2)
    for j in (0, 1):
        cases = golden["batch%d" % j].tolist()
        frames, plan = step_of(golden, cases, subset, layout)
        H, W = resize.padded_size([(p.nh, p.nw) for p in plan])
        tabs = host_tables(frames, plan, layout)
        x, mask = c_color(tabs, len(cases), H, W, channels_last, layout, contrast)
        want, want_mask = expected(golden, cases, subset, (H, W))
        assert torch.equal(mask.cpu().bool(), want_mask), (j, subset)
        for b, i in enumerate(cases):
            assert torch.equal(x[b].cpu(), want[b]), "case %d, subset %d" % (i, subset)
        again, _ = c_color(tabs, len(cases), H, W, channels_last, layout, contrast)      # two runs: the same bytes
        assert torch.equal(x.contiguous().view(torch.int32), again.contiguous().view(torch.int32))
        if not contrast:      # the two launches give the pointwise steps' result as well
            both, _ = c_color(tabs, len(cases), H, W, channels_last, layout, True)
            assert torch.equal(x.cpu(), both.cpu())
        if subset == 7:       # the final normalised tensor
            mean, std = golden["pixel_mean"].tolist(), golden["pixel_std"].tolist()
            x, mask = c_color(tabs, len(cases), H, W, channels_last, layout, True, mean, std)
            assert np.array_equal(x.cpu().numpy(), golden["batch%d_x" % j])
            assert np.array_equal(mask.cpu().numpy().astype(bool), golden["batch%d_mask" % j])


@pytest.mark.gpu
def test_a_plan_without_colour_gives_the_parents_output_bit_for_bit(golden):
    cases = golden["batch0"].tolist()
    mean, std = golden["pixel_mean"].tolist(), golden["pixel_std"].tolist()
    for layout in resize.LAYOUTS:
        frames, plan = step_of(golden, cases, 0, layout)
        tabs = host_tables(frames, plan, layout)
        assert not tabs[6].any()                                                # a table of zero rows
        for channels_last in (False, True):
            want, want_mask = base.c_frames(tabs[0][:tabs[1]], *tabs[3:6], 3, 96, 64, channels_last, layout, mean, std)
            for contrast in (False, True):
                x, mask = c_color(tabs, 3, 96, 64, channels_last, layout, contrast, mean, std)
                assert torch.equal(x.contiguous().view(torch.int32), want.contiguous().view(torch.int32))
                assert torch.equal(mask, want_mask)
        # the Python op: such a step stages no colour table and makes the launch it always made
        staged = augment.stage_step(frames, plan, [], DEV, layout)
        assert staged.color is None and staged.workspace == -1
        calls = dict(augment.COLOR_CALLS)
        x, mask = augment.augment_frames(staged, mean, std)
        assert augment.COLOR_CALLS == calls
        assert torch.equal(x.view(torch.int32), base.c_frames(tabs[0][:tabs[1]], *tabs[3:6], 3, 96, 64, False, layout, mean,
                                                              std)[0].view(torch.int32))


@pytest.mark.gpu
def test_malformed_colour_rows_are_empty_frames(golden):
    cases = golden["batch0"].tolist()
    frames, plan = step_of(golden, cases, 7, "hwc")
    tabs = list(host_tables(frames, plan, "hwc"))
    want, _ = expected(golden, cases, 7, (96, 64))
    nan32, inf32 = (int(np.array([v], dtype=np.float32).view(np.int32)[0]) for v in (np.nan, np.inf))
    nan64, inf64 = (np.array([v], dtype="<f8").view(np.int32).tolist() for v in (np.nan, -np.inf))
    for col, words in ((1, [nan32]), (1, [inf32]), (2, nan64), (2, inf64), (4, nan64), (4, inf64), (0, [15]), (0, [-1])):
        color = tabs[6].clone()
        color[1, col:col + len(words)] = torch.tensor(words, dtype=torch.int32)
        x, mask = c_color(tabs[:6] + [color], 3, 96, 64, False, "hwc", True)
        assert (x[1] == 0).all() and (mask[1] == 1).all(), (col, words)         # the empty frame: all padding
        assert torch.equal(x[0].cpu(), want[0]) and torch.equal(x[2].cpu(), want[2])
    # a weight that is not finite under a CLEAR flag is not read
    color = tabs[6].clone()
    color[1, 0] = 0
    color[1, 1] = nan32
    x, _ = c_color(tabs[:6] + [color], 3, 96, 64, False, "hwc", True)
    assert torch.equal(x[1].cpu(), expected(golden, cases, 0, (96, 64))[0][1])
    # one launch cannot honour contrast: such a row is malformed there
    x, mask = c_color(tabs, 3, 96, 64, False, "hwc", False)
    assert (x == 0).all() and (mask == 1).all()
    # a target of size zero, and a source frame that reaches into the workspace
    dst = tabs[4].clone()
    dst[0, 1] = 0
    x, mask = c_color(tabs[:4] + [dst] + tabs[5:], 3, 96, 64, False, "hwc", True)
    assert (x[0] == 0).all() and (mask[0] == 1).all() and torch.equal(x[1].cpu(), want[1])
    from vnext_amd import _lib
    lib = _lib.lib()
    assert lib.vnx_augment_color_workspace(3, 96, 64) == augment.color_workspace(3, 96, 64)
    buf = tabs[0].to(DEV)
    args = [tabs[3].to(DEV), tabs[4].to(DEV), tabs[5].to(DEV), tabs[6].to(DEV)]
    out = torch.zeros(3 * 3 * 96 * 64, device=DEV), torch.zeros(3 * 96 * 64, dtype=torch.uint8, device=DEV)
    def call(pixel_bytes, work_at, color_ptr=args[3].data_ptr(), batch=3):
        return lib.vnx_augment_frames_color(buf.data_ptr(), pixel_bytes, args[0].data_ptr(), args[1].data_ptr(),
                                            args[2].data_ptr(), args[2].numel(), color_ptr, batch, 96, 64, 0.0, 0.0, 0.0, 1.0,
                                            1.0, 1.0, 0, 1, 1, work_at, out[0].data_ptr(), out[1].data_ptr(), None)
    assert call(tabs[1], tabs[2]) == 0
    assert call(tabs[1] - 1, tabs[2]) != 0          # the workspace does not fit
    assert call(tabs[1], tabs[2] + 4) != 0          # not 16-byte aligned (and too far)
    assert call(tabs[1], tabs[2], color_ptr=None) != 0
    assert call(tabs[1], tabs[2], color_ptr=None, batch=0) == 0      # no frames: no launch
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_the_python_op_makes_one_launch_more_with_contrast_and_none_more_without(golden):
    cases = golden["batch0"].tolist()
    mean, std = golden["pixel_mean"].tolist(), golden["pixel_std"].tolist()
    for layout in resize.LAYOUTS:
        for subset, launches in ((5, 1), (1, 1), (4, 1), (2, 2), (7, 2)):
            frames, plan = step_of(golden, cases, subset, layout)
            staged = augment.stage_step(frames, plan, [(0, [100 * 64])], DEV, layout)
            assert staged.color.is_cuda and (staged.workspace >= 0) == (launches == 2)
            calls, colour = dict(augment.CALLS), dict(augment.COLOR_CALLS)
            x, mask = augment.augment_frames(staged, [0.0] * 3, [1.0] * 3)
            assert augment.CALLS == {**calls, "augment_frames": calls["augment_frames"] + 1}
            assert augment.COLOR_CALLS == {"augment_frames_color": colour["augment_frames_color"] + 1,
                                           "launches": colour["launches"] + launches}
            want, want_mask = expected(golden, cases, subset, (96, 64))
            assert torch.equal(x.cpu(), want) and torch.equal(mask.cpu(), want_mask)
            flat, boxes, nonempty = augment.augment_masks(staged)                 # the masks do not see the colour
            assert nonempty.tolist() == [False] and flat.numel() == 70 * 45
    frames, plan = step_of(golden, cases, 7, "chw")
    x, _ = augment.augment_frames(augment.stage_step(frames, plan, [], DEV), mean, std, channels_last=True)
    assert x.is_contiguous(memory_format=torch.channels_last) and np.array_equal(x.cpu().numpy(), golden["batch0_x"])


@pytest.mark.gpu
def test_the_two_launches_captured_in_a_graph_replay_on_other_pixels_and_weights(golden):
    """one graph on one stream: capture a step, overwrite the pixels and every table in place with ANOTHER step of the same
    batch and padded size (other frames in other slots, other weights), poison the outputs and the workspace, replay"""
    from vnext_amd import _lib
    lib = _lib.lib()
    first = step_of(golden, [0, 1, 2], 7, "chw")
    second = step_of(golden, [1, 2, 0], 7, "chw", weights=[1.1, 0.9, 1.0731])
    t1, t2 = host_tables(*first, "chw"), host_tables(*second, "chw")
    assert t1[1:3] == t2[1:3]      # (the same frames in another order: the same bytes in all, the same workspace offset)
    tensors = lambda t: [t[0], t[3], t[4], t[5], t[6]]
    room = [max(a.numel(), b.numel()) for a, b in zip(tensors(t1), tensors(t2))]
    bufs = [torch.zeros(n, dtype=a.dtype, device=DEV) for n, a in zip(room, tensors(t1))]
    def load(t):
        for b, a in zip(bufs, tensors(t)):
            b.zero_()
            b[:a.numel()].copy_(a.reshape(-1))
    x = torch.full((3, 3, 96, 64), float("nan"), device=DEV)
    mask = torch.full((3, 96, 64), 0xFF, dtype=torch.uint8, device=DEV)
    load(t1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.check(lib.vnx_augment_frames_color(bufs[0].data_ptr(), t1[1], bufs[1].data_ptr(), bufs[2].data_ptr(),
                                                bufs[3].data_ptr(), bufs[3].numel(), bufs[4].data_ptr(), 3, 96, 64, 0.0, 0.0,
                                                0.0, 1.0, 1.0, 1.0, 0, 0, 1, t1[2], x.data_ptr(), mask.data_ptr(),
                                                _lib.current_stream(x)))
    for (frames, plan), t in ((second, t2), (first, t1)):
        load(t)
        bufs[0][t[2]:].fill_(0x5A)
        x.fill_(float("nan"))
        mask.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        want, want_mask = base.padded(augment.reference_augment_frames(frames, plan), (96, 64))
        assert torch.equal(x.cpu(), want) and torch.equal(mask.cpu().bool(), want_mask)


# ---- the models -------------------------------------------------------------------------------------------------------------
def colored(plans, seed):
    rng = np.random.default_rng(seed)
    return [[p._replace(brightness=float(rng.uniform(0.9, 1.1)), contrast=float(rng.uniform(0.9, 1.1)),
                        saturation=float(rng.uniform(0.9, 1.1))) for p in clip] for clip in plans]


@pytest.mark.gpu
def test_seqformer_training_step_with_a_colour_plan_equals_the_host_route():
    torch.manual_seed(5)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": DEV, **base.TINY_SEQ})).train()
    plans = colored([[augment.full_plan(96, 160, 60, 100, True)] * 2, [augment.full_plan(96, 160, 60, 100, False)] * 2], 70)
    assert len({p.color for clip in plans for p in clip}) == 4                    # a weight per frame
    launches = augment.COLOR_CALLS["launches"]
    base.step_both_routes(model, base.training_clips(2, 2, plans, seed=50))
    assert augment.COLOR_CALLS["launches"] == launches + 2                        # the device route's, once


@pytest.mark.gpu
def test_idol_training_step_with_a_colour_plan_equals_the_host_route():
    torch.manual_seed(6)
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": DEV, **base.TINY_IDOL})).train()
    plans = colored([[FramePlan(16, 8, 120, 80, 64, 96, True), FramePlan(0, 0, 160, 96, 60, 100, True)],
                     [FramePlan(10, 0, 140, 88, 88, 140, False), FramePlan(20, 12, 128, 80, 70, 112, False)]], 71)
    plans[1][0] = plans[1][0]._replace(contrast=None)                            # a frame without one of the steps
    launches = augment.COLOR_CALLS["launches"]
    base.step_both_routes(model, base.training_clips(2, 2, plans, seed=60))
    assert augment.COLOR_CALLS["launches"] == launches + 2
