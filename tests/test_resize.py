"""Test-time resize on the device (vnext_amd/csrc/resize.hip, vnext_amd/ops/resize.py).

What is held to what:
* `reference_resize` -- the integer restatement of Pillow's 8-bit bilinear resample -- equals Pillow byte for byte: on the
  stored results of tests/golden/resize_pillow.npz (tools/make_golden_resize.py; no Pillow needed) and, where Pillow imports,
  on 200 random size pairs.
* the kernel equals `reference_resize` EXACTLY (integer arithmetic: no tolerance), through the C ABI, in both source and both
  output layouts, frames at odd byte offsets, outputs pre-filled and guarded; with the model's mean / std it is bit-identical
  to torch's `(u.float() - mean) / std` of the reference's bytes.
* the models with the switch on, fed sources, see bit-identical network inputs to the switch off fed host-resized frames.
No GPU test imports Pillow.
"""
import os

import numpy as np
import pytest
import torch

import vnext_amd.models  # noqa: F401  (registers the meta-archs)
from conftest import GOLDEN_DIR
from vnext_amd import train as T
from vnext_amd.models import idol as idol_mod
from vnext_amd.models import seqformer as sf
from vnext_amd.models import tracker as trk
from vnext_amd.ops import ingest, resize
from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg

DEV = "cuda:0"
GUARD = 64
TINY_SEQ = {"MODEL.SeqFormer.ENC_LAYERS": 1, "MODEL.SeqFormer.DEC_LAYERS": 2, "MODEL.SeqFormer.NUM_OBJECT_QUERIES": 12,
            "MODEL.SeqFormer.DIM_FEEDFORWARD": 64, "MODEL.SeqFormer.DROPOUT": 0.0, "INPUT.SAMPLING_FRAME_NUM": 2}
TINY_IDOL = {"MODEL.IDOL.ENC_LAYERS": 1, "MODEL.IDOL.DEC_LAYERS": 2, "MODEL.IDOL.NUM_OBJECT_QUERIES": 110,
             "MODEL.IDOL.DIM_FEEDFORWARD": 64, "MODEL.IDOL.DROPOUT": 0.0}
TEST_SIZE = {"INPUT.MIN_SIZE_TEST": 24, "INPUT.MAX_SIZE_TEST": 64}      # 48 x 80 sources -> 24 x 40
# (source, target, why): each the smallest shape that reaches its branch
CASES = [
    ((37, 53), (19, 27), "non-integer factor 1.95, ksize 5, taps clipped at all four borders"),
    ((48, 64), (24, 32), "exact 2x"),
    ((45, 63), (15, 21), "3x, ksize 7"),
    ((19, 27), (37, 53), "upscale, ksize 3"),
    ((40, 56), (40, 28), "vertical pass skipped"),
    ((40, 56), (20, 56), "horizontal pass skipped"),
    ((33, 47), (33, 47), "both skipped: the ingest kernel's result"),
    ((130, 70), (17, 9), "factor 7.7, ksize 17: the supported limit"),
    ((150, 260), (75, 130), "more than one tile on both axes, neither a multiple of the tile"),
]
EXTREMES = [CASES[0][:2], CASES[1][:2]]      # also as a 0/255 checkerboard and an all-255 frame: rounding at the extremes, the clamp
ALL_CASES = [(s, d, "random") for s, d, _ in CASES] + [(s, d, c) for s, d in EXTREMES for c in ("checker", "white")]


def case_name(src, dst, content):
    return "%dx%d_%dx%d_%s" % (src + dst + (content,))


@pytest.fixture(scope="module")
def golden():
    """name -> (source uint8 [h, w, 3], Pillow's result uint8 [nh, nw, 3]); read once"""
    g = np.load(os.path.join(GOLDEN_DIR, "resize_pillow.npz"))
    return {case_name(*c): (g[case_name(*c) + "_src"], g[case_name(*c) + "_out"]) for c in ALL_CASES}


def model_stats():
    cfg = get_seqformer_cfg(**{"MODEL.DEVICE": "cpu"})
    return [float(v) for v in cfg.MODEL.PIXEL_MEAN], [float(v) for v in cfg.MODEL.PIXEL_STD]


def as_f32(values):
    return torch.tensor(values, dtype=torch.float32).tolist()


def random_sources(sizes, seed, layout="chw"):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (3, h, w) if layout == "chw" else (h, w, 3), dtype=torch.uint8, generator=g)
            for h, w in sizes]


def in_layout(hwc, layout):
    """a uint8 [h, w, 3] array as a contiguous tensor of `layout`"""
    t = torch.from_numpy(np.ascontiguousarray(hwc))
    return t if layout == "hwc" else t.permute(2, 0, 1).contiguous()


def as_chw(t, layout):
    return t if layout == "chw" else t.permute(2, 0, 1)


@pytest.fixture
def cpu_stand_ins(monkeypatch):
    """PyTorch restatements (oracle/, tests only) of the HIP entry points the models call, so they run on CPU
    (as tests/test_ingest.py does)."""
    from oracle.heads_torch_fallback import dynamic_mask_head_torch
    from oracle.msda_torch_fallback import msda_grid_sample
    from vnext_amd.ops.modules import ms_deform_attn as mod

    class Fn:
        @staticmethod
        def apply(value, shapes, lsi, loc, attn, step):
            return msda_grid_sample(value, shapes, loc, attn)

    def with_coords(feats, ref, params, counts, stride):
        inst = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor([int(c) for c in counts]))
        return dynamic_mask_head_torch(feats, ref[0], params[0], inst.to(torch.int32), stride)[None]
    monkeypatch.setattr(mod, "MSDeformAttnFunction", Fn)
    monkeypatch.setattr(idol_mod, "dynamic_mask_head", dynamic_mask_head_torch)
    monkeypatch.setattr(sf, "dynamic_mask_head", dynamic_mask_head_torch)
    monkeypatch.setattr(sf, "dynamic_mask_with_coords", with_coords)
    monkeypatch.setattr(trk, "_pairwise_dot", lambda a, b: a @ b.t())
    monkeypatch.setattr(trk, "_match_scores", lambda e, m, metric: (
        ((e @ m.t()).softmax(1) + (e @ m.t()).softmax(0)) / 2 if metric == "bisoftmax" else (e @ m.t()).softmax(1)))


def same_video_result(a, b, score_rtol=1e-5, mask_frac=1e-3):
    """the comparison tests/test_ingest.py uses for its own on / off pair"""
    assert a["image_size"] == b["image_size"]
    assert a["pred_labels"] == b["pred_labels"]
    np.testing.assert_allclose(a["pred_scores"], b["pred_scores"], rtol=score_rtol)
    for ma, mb in zip(a["pred_masks"], b["pred_masks"]):
        if isinstance(ma, (list, tuple)):      # IDOL: per track, a list over frames (None where absent)
            for fa, fb in zip(ma, mb):
                assert (fa is None) == (fb is None)
                if fa is not None:
                    assert float((fa != fb).float().mean()) < mask_frac
        else:
            assert float((ma != mb).float().mean()) < mask_frac


# ---- CPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=[case_name(*c) for c in ALL_CASES])
def test_reference_resize_equals_the_stored_pillow_result(golden, case):
    (h, w), (nh, nw), _ = case
    src, want = golden[case_name(*case)]
    assert src.shape == (h, w, 3) and want.shape == (nh, nw, 3)
    for layout in resize.LAYOUTS:
        got = resize.reference_resize(in_layout(src, layout), nh, nw, layout)
        assert got.dtype == torch.uint8 and torch.equal(as_chw(got, layout), in_layout(want, "chw")), layout
    assert np.array_equal(resize.reference_resize(src, nh, nw, "hwc"), want)      # arrays in, arrays out


def test_reference_resize_equals_pillow_on_random_size_pairs():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(21)
    pairs = [((1, 1), (1, 1)), ((1, 40), (1, 7)), ((40, 1), (9, 1)), ((1, 5), (30, 1)), ((7, 1), (1, 60)),      # one-pixel sides
             ((31, 31), (31, 31)), ((20, 33), (20, 17)), ((20, 33), (11, 33)),                                   # equal sides
             ((80, 64), (10, 8)), ((80, 80), (11, 10)), ((72, 79), (9, 10)), ((8, 10), (64, 80))]               # factors up to 8
    while len(pairs) < 200:
        (h, w), (nh, nw) = rng.integers(1, 81, 2), rng.integers(1, 81, 2)
        pairs.append(((int(h), int(w)), (int(nh), int(nw))))
    for (h, w), (nh, nw) in pairs:
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        want = np.asarray(Image.fromarray(a).resize((nw, nh), Image.BILINEAR))
        assert np.array_equal(resize.reference_resize(a, nh, nw, "hwc"), want), ((h, w), (nh, nw))
        chw = resize.reference_resize(np.ascontiguousarray(a.transpose(2, 0, 1)), nh, nw, "chw")
        assert np.array_equal(chw.transpose(1, 2, 0), want), ((h, w), (nh, nw))


def test_shortest_edge_size_against_values_worked_by_hand():
    """short 360, max 640.  720 x 1280: scale 0.5 -> 360 x 640.  480 x 640: 0.75 -> 360 x 480.  300 x 1000: 1.2 -> 360 x 1200,
    over the maximum: x 640 / 1200 -> 192 x 640.  1080 x 1920: 1 / 3 -> 360 x 640.  101 x 77: 360 / 77 -> 472.2 x 360."""
    worked = {(720, 1280): (360, 640), (480, 640): (360, 480), (300, 1000): (192, 640), (1080, 1920): (360, 640),
              (101, 77): (472, 360)}
    for (h, w), want in worked.items():
        assert resize.shortest_edge_size(h, w, 360, 640) == want
        if min(want) == 360:      # the rule is idempotent on its own outputs that reached the short edge ...
            assert resize.shortest_edge_size(*want, 360, 640) == want
    # ... and on the capped one as well: 192 x 640 -> 360 x 1200 -> capped back to 192 x 640
    assert resize.shortest_edge_size(192, 640, 360, 640) == (192, 640)


def test_pillow_coeffs_rows_are_normalised_weights_inside_the_source():
    for n_in, n_out, ksize in ((64, 32, 5), (53, 27, 5), (63, 21, 7), (27, 53, 3), (19, 37, 3), (130, 17, 17), (1280, 640, 5),
                               (1, 9, 3), (9, 1, 19)):
        bounds, kk = resize.pillow_coeffs(n_in, n_out)
        assert bounds.dtype == np.int32 and kk.dtype == np.int32
        assert bounds.shape == (n_out, 2) and kk.shape == (n_out, ksize) and resize.kernel_size(n_in, n_out) == ksize
        assert (kk >= 0).all() and (kk < 2 ** 23).all()
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= n_in).all()
        assert (np.abs(kk.sum(1).astype(np.int64) - 2 ** 22) <= ksize).all()
        for (xmin, cnt), row in zip(bounds.tolist(), kk):
            assert (row[cnt:] == 0).all()
        assert resize.pillow_coeffs(n_in, n_out)[1] is kk      # cached per (in, out)
    assert resize.supported(130, 70, 17, 9) and not resize.supported(9, 9, 1, 9) and resize.supported(2, 2, 900, 900)


@pytest.mark.parametrize("layout", resize.LAYOUTS)
def test_stage_sources_round_trips_frames_of_unequal_sizes(layout):
    sizes, targets = [(7, 9), (1, 1), (16, 5), (12, 33)], [(4, 9), (3, 2), (16, 5), (24, 40)]
    frames = random_sources(sizes, seed=6, layout=layout)
    pixels, src, dst, coeffs = resize.stage_sources(frames, targets, "cpu", layout)
    assert pixels.dtype == torch.uint8 and pixels.data_ptr() % 16 == 0
    assert all(t.dtype == torch.int32 for t in (src, dst, coeffs)) and tuple(src.shape) == tuple(dst.shape) == (4, 3)
    assert dst.tolist() == [[0, nh, nw] for nh, nw in targets]
    words = coeffs.numpy()
    for i, (f, (o, h, w), (nh, nw)) in enumerate(zip(frames, src.tolist(), targets)):
        assert (h, w) == sizes[i] and o % 16 == 0 and torch.equal(pixels[o:o + 3 * h * w].view(f.shape), f)
        for j, (n_in, n_out) in enumerate(((w, nw), (h, nh))):
            b_off, k_off, ksize = words[6 * i + 3 * j:6 * i + 3 * j + 3].tolist()
            if n_in == n_out:
                assert ksize == 0
                continue
            bounds, kk = resize.pillow_coeffs(n_in, n_out)
            assert ksize == kk.shape[1]
            assert np.array_equal(words[b_off:b_off + bounds.size].reshape(bounds.shape), bounds)
            assert np.array_equal(words[k_off:k_off + kk.size].reshape(kk.shape), kk)
    x, mask = resize.resize_ingest_frames(pixels, src, dst, coeffs, 4, 32, 64, *model_stats(), layout=layout)
    resized = [as_chw(resize.reference_resize(f, nh, nw, layout), layout).contiguous() for f, (nh, nw) in zip(frames, targets)]
    want_x, want_mask = ingest.ingest_frames(*ingest.stage_frames(resized, "cpu"), 4, 32, 64, *model_stats())
    assert torch.equal(x, want_x) and torch.equal(mask, want_mask)


def test_enable_device_resize_flips_both_models_and_raises_without_the_switch():
    seq = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": "cpu", **TINY_SEQ}))
    idol = build_model(get_idol_cfg(**{"MODEL.DEVICE": "cpu", **TINY_IDOL}))
    assert seq._test_size == (360, 1333) and idol._test_size == (480, 1333)      # the reference's config files
    for model in (seq, idol):
        assert model.device_resize is False
        T.enable_device_resize(model)
        assert model.device_resize is True
        T.enable_device_resize(model, on=False)
        assert model.device_resize is False
    with pytest.raises(ValueError, match="device_resize"):
        T.enable_device_resize(torch.nn.Linear(2, 2))


def host_resized(frames, short, max_size, layout):
    """the parent's route: each frame through `reference_resize` to its ResizeShortestEdge target, as CHW"""
    out = []
    for f in frames:
        nh, nw = resize.shortest_edge_size(*resize.frame_size(f, layout), short, max_size)
        out.append(as_chw(resize.reference_resize(f, nh, nw, layout), layout).contiguous())
    return out


def test_seqformer_eval_with_the_switch_equals_host_resized_frames_on_cpu(cpu_stand_ins):
    torch.manual_seed(3)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": "cpu", **TINY_SEQ, **TEST_SIZE})).eval()
    for layout in resize.LAYOUTS:
        sources = random_sources([(48, 80)] * 2, seed=4, layout=layout)
        small = host_resized(sources, 24, 64, layout)
        assert [tuple(f.shape) for f in small] == [(3, 24, 40)] * 2
        off = model([{"image": small, "height": 48, "width": 80}])
        T.enable_device_resize(model)
        on = model([{"image": sources, "image_layout": layout}])      # height / width default to the SOURCE size
        again = model([{"image": small, "height": 48, "width": 80}])  # already at the target: the usual path
        T.enable_device_resize(model, on=False)
        assert tuple(on["image_size"]) == (48, 80)
        same_video_result(on, off, score_rtol=1e-6, mask_frac=1e-6)
        same_video_result(again, off, score_rtol=0, mask_frac=1e-9)


def test_idol_eval_with_the_switch_equals_host_resized_frames_on_cpu(cpu_stand_ins):
    torch.manual_seed(3)
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": "cpu", "MODEL.IDOL.BATCH_INFER_LEN": 2, **TINY_IDOL,
                                        **TEST_SIZE})).eval()
    for layout in resize.LAYOUTS:
        sources = random_sources([(48, 80)] * 3, seed=5, layout=layout)
        off = model([{"image": host_resized(sources, 24, 64, layout), "height": 48, "width": 80}])
        T.enable_device_resize(model)
        on = model([{"image": sources, "image_layout": layout}])
        T.enable_device_resize(model, on=False)
        assert tuple(on["image_size"]) == (48, 80)
        same_video_result(on, off, score_rtol=1e-6, mask_frac=1e-6)


def test_a_pair_beyond_the_kernels_range_takes_the_host_route():
    frames = random_sources([(90, 40)] * 2, seed=8)
    assert not resize.applies(frames, [(9, 4)] * 2, "cpu")                      # 10x: ksize 21
    out, plan, src = resize.plan_video(frames, "chw", 4, 64, "cpu")
    assert plan is None and src == (90, 40) and [tuple(f.shape) for f in out] == [(3, 9, 4)] * 2
    assert torch.equal(out[0], resize.reference_resize(frames[0], 9, 4))
    floats = [f.float() for f in frames]
    assert resize.plan_video(floats, "chw", 4, 64, "cpu") == (floats, None, None)


# ---- GPU, through the C ABI ------------------------------------------------------------------------------------------------
def pack_odd(frames, room=None):
    """the frames' bytes (whatever their layout) in one host buffer, every frame at an ODD byte offset
    -> (buffer uint8, rows [(offset, ...)])"""
    offs, off = [], 1
    for f in frames:
        offs.append(off)
        off += f.numel()
        off += 1 - off % 2
    buf = torch.full((room or off + 3,), 0xAB, dtype=torch.uint8)
    for f, o in zip(frames, offs):
        buf[o:o + f.numel()] = f.reshape(-1)
    return buf, offs


def tables(frames, targets, layout, offs):
    sizes = [resize.frame_size(f, layout) for f in frames]
    src = torch.tensor([(o, h, w) for o, (h, w) in zip(offs, sizes)], dtype=torch.int32)
    dst = torch.tensor([(0, nh, nw) for nh, nw in targets], dtype=torch.int32)
    return src, dst, torch.from_numpy(resize.coeff_words(sizes, targets))


def c_resize(buf, src, dst, coeffs, B, H, W, mean, std, channels_last, layout):
    """vnx_resize_ingest_frames into NaN / 0xFF pre-filled outputs with guard words around them -> x [B, 3, H, W] (a view
    of the layout asked for), mask uint8 [B, H, W]"""
    from vnext_amd import _lib
    buf, src, dst, coeffs = (t.to(DEV) for t in (buf, src, dst, coeffs))
    xs = torch.full((B * 3 * H * W + 2 * GUARD,), float("nan"), device=DEV)
    ms = torch.full((B * H * W + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().vnx_resize_ingest_frames(
        buf.data_ptr(), buf.numel(), src.data_ptr(), dst.data_ptr(), coeffs.data_ptr(), coeffs.numel(), B, H, W,
        *as_f32(mean), *as_f32(std), int(channels_last), int(layout == "hwc"), xs[GUARD:].data_ptr(), ms[GUARD:].data_ptr(),
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
    """uint8 CHW frames as floats padded to `size`, and the padding mask"""
    H, W = size
    x = torch.zeros(len(frames_chw), 3, H, W)
    mask = torch.ones(len(frames_chw), H, W, dtype=torch.bool)
    for i, f in enumerate(frames_chw):
        x[i, :, :f.shape[1], :f.shape[2]] = f.float()
        mask[i, :f.shape[1], :f.shape[2]] = False
    return x, mask


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL_CASES, ids=[case_name(*c) for c in ALL_CASES])
def test_the_resampled_bytes_are_exact(golden, case):
    """mean 0, std 1: x IS the resampled byte.  Against `reference_resize` and against Pillow's stored result"""
    (h, w), (nh, nw), _ = case
    src_hwc, pillow = golden[case_name(*case)]
    H, W = resize.padded_size([(nh, nw)])
    want, want_mask = padded([in_layout(pillow, "chw")], (H, W))
    for layout in resize.LAYOUTS:
        frame = in_layout(src_hwc, layout)
        ref = as_chw(resize.reference_resize(frame, nh, nw, layout), layout)
        assert torch.equal(ref, in_layout(pillow, "chw"))
        buf, offs = pack_odd([frame])
        assert offs[0] % 2 == 1
        src, dst, coeffs = tables([frame], [(nh, nw)], layout, offs)
        for channels_last in (False, True):
            x, mask = c_resize(buf, src, dst, coeffs, 1, H, W, [0.0] * 3, [1.0] * 3, channels_last, layout)
            assert torch.equal(x.cpu(), want), (layout, channels_last)
            assert torch.equal(mask.cpu().bool(), want_mask), (layout, channels_last)


@pytest.mark.gpu
def test_a_frame_at_its_target_size_equals_ingest_frames_bit_for_bit(golden):
    from vnext_amd import _lib
    src_hwc, _ = golden[case_name((33, 47), (33, 47), "random")]
    frame = in_layout(src_hwc, "chw")
    buf, offs = pack_odd([frame])
    src, dst, coeffs = tables([frame], [(33, 47)], "chw", offs)
    mean, std = model_stats()
    for channels_last in (False, True):
        x, mask = c_resize(buf, src, dst, coeffs, 1, 64, 64, mean, std, channels_last, "chw")
        fmt = torch.channels_last if channels_last else torch.contiguous_format
        want = torch.empty((1, 3, 64, 64), device=DEV, memory_format=fmt)
        want_mask = torch.empty((1, 64, 64), dtype=torch.bool, device=DEV)
        dbuf, dtab = buf.to(DEV), src.to(DEV)
        _lib.check(_lib.lib().vnx_ingest_frames(dbuf.data_ptr(), dbuf.numel(), dtab.data_ptr(), 1, 64, 64, *as_f32(mean),
                                                *as_f32(std), int(channels_last), want.data_ptr(), want_mask.data_ptr(),
                                                _lib.current_stream(dbuf)))
        torch.cuda.synchronize()
        assert torch.equal(x, want) and torch.equal(mask.bool(), want_mask)


@pytest.mark.gpu
def test_normalisation_is_torchs_expression_of_the_reference_bytes(golden):
    src_hwc, _ = golden[case_name((37, 53), (19, 27), "random")]
    mean, std = model_stats()
    m = torch.tensor(mean, device=DEV).view(3, 1, 1)
    s = torch.tensor(std, device=DEV).view(3, 1, 1)
    for layout in resize.LAYOUTS:
        frame = in_layout(src_hwc, layout)
        buf, offs = pack_odd([frame])
        src, dst, coeffs = tables([frame], [(19, 27)], layout, offs)
        ref = as_chw(resize.reference_resize(frame, 19, 27, layout), layout).to(DEV)
        want = (ref.float() - m) / s
        ieee = (ref.cpu().float() - m.cpu()) / s.cpu()
        x, mask = c_resize(buf, src, dst, coeffs, 1, 32, 32, mean, std, False, layout)
        assert torch.equal(x[0, :, :19, :27].cpu(), ieee)                    # the IEEE expression, as the ingest kernel
        ulps = (want.cpu().view(torch.int32).long() - ieee.contiguous().view(torch.int32).long()).abs().max()
        print(f"{layout}: ATen's device division differs from IEEE by at most {int(ulps)} ulp on these values")
        assert torch.equal(x[0, :, :19, :27], want)
        assert (x[0, :, 19:] == 0).all() and (x[0, :, :, 27:] == 0).all()


UNEQUAL = [((37, 53), (19, 27)), ((19, 27), (37, 53)), ((33, 47), (33, 47))]


def unequal_batch(layout="chw"):
    """three frames of unequal source and target sizes and a fourth row pointing outside the buffer, padded to 64 x 64
    -> (arguments of c_resize up to B, H, W; the three resized CHW frames)"""
    frames = random_sources([s for s, _ in UNEQUAL] + [(20, 20)], seed=12, layout=layout)
    targets = [d for _, d in UNEQUAL] + [(10, 10)]
    buf, offs = pack_odd(frames)
    src, dst, coeffs = tables(frames, targets, layout, offs)
    src[3, 0] = buf.numel() - 100                          # the fourth frame would end beyond the buffer
    resized = [as_chw(resize.reference_resize(f, nh, nw, layout), layout) for f, (nh, nw) in zip(frames[:3], targets)]
    return (buf, src, dst, coeffs, 4, 64, 64), resized


@pytest.mark.gpu
@pytest.mark.parametrize("layout", resize.LAYOUTS)
def test_a_batch_of_unequal_frames_and_a_row_outside_the_buffer(layout):
    args, resized = unequal_batch(layout)
    want, want_mask = padded(resized, (64, 64))
    for channels_last in (False, True):
        x, mask = c_resize(*args, [0.0] * 3, [1.0] * 3, channels_last, layout)
        assert torch.equal(x[:3].cpu(), want) and torch.equal(mask[:3].cpu().bool(), want_mask)
        assert (x[3] == 0).all() and (mask[3] == 1).all()                     # the bad row: all padding
    # rows the kernel must refuse without reading: a target beyond the padded size, a coefficient table outside its buffer
    buf, src, dst, coeffs, B, H, W = args
    dst2, coeffs2 = dst.clone(), coeffs.clone()
    dst2[0, 2] = 65
    coeffs2[6 * 1 + 1] = coeffs.numel() - 3
    x, mask = c_resize(buf, src, dst2, coeffs2, B, H, W, [0.0] * 3, [1.0] * 3, False, layout)
    assert (x[0] == 0).all() and (mask[0] == 1).all() and (x[1] == 0).all() and (mask[1] == 1).all()
    assert torch.equal(x[2].cpu(), want[2]) and torch.equal(mask[2].cpu().bool(), want_mask[2])


@pytest.mark.gpu
def test_level_constants_of_the_destination_table():
    """`level_constants` reads the DESTINATION table alone (h, w).  The three good frames: equal to `reference_levels` of the
    resize kernel's mask.  The fourth frame is refused by the resize kernel for its SOURCE row, which the level launch never
    sees: with the batch as it stands its level masks are those of the 10 x 10 target its destination row names; a caller
    that drops a frame says so in the destination row (nh = nw = 0), and then all four frames agree."""
    from test_ingest import check_positions
    (buf, src, dst, coeffs, B, H, W), _ = unequal_batch()
    levels, npf = [(8, 8), (4, 4), (2, 2), (1, 1)], 128
    _, mask = c_resize(buf, src, dst, coeffs, B, H, W, *model_stats(), False, "chw")
    assert (mask[3] == 1).all()
    masks, poss = ingest.level_constants(dst.to(DEV), B, H, W, levels, npf)
    named = mask.bool().clone()
    named[3, :10, :10] = False
    want_masks, want_poss = ingest.reference_levels(mask.bool(), levels, npf)
    named_masks, _ = ingest.reference_levels(named, levels, npf)
    for lvl, (a, b, c, p, q) in enumerate(zip(masks, want_masks, named_masks, poss, want_poss)):
        assert torch.equal(a[:3], b[:3]) and torch.equal(a[3], c[3])
        check_positions(b[:3], p[:3], q[:3], npf, f"level {lvl}")
    dst[3] = 0
    _, mask = c_resize(buf, src, dst, coeffs, B, H, W, *model_stats(), False, "chw")
    masks, poss = ingest.level_constants(dst.to(DEV), B, H, W, levels, npf)
    want_masks, want_poss = ingest.reference_levels(mask.bool(), levels, npf)
    for lvl, (a, b, p, q) in enumerate(zip(masks, want_masks, poss, want_poss)):
        assert torch.equal(a, b)
        check_positions(b, p, q, npf, f"all four, level {lvl}")


@pytest.mark.gpu
def test_a_captured_call_replays_on_new_pixels():
    """one graph, one branch: capture at 48 x 64 -> 24 x 32, overwrite the pixels in place, poison the outputs, replay"""
    from vnext_amd import _lib
    first, second = random_sources([(48, 64)], seed=14), random_sources([(48, 64)], seed=15)
    buf1, offs = pack_odd(first)
    buf2, _ = pack_odd(second)
    src, dst, coeffs = (t.to(DEV) for t in tables(first, [(24, 32)], "chw", offs))
    buf = buf1.to(DEV)
    x = torch.full((1, 3, 32, 32), float("nan"), device=DEV)
    mask = torch.full((1, 32, 32), 0xFF, dtype=torch.uint8, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.check(_lib.lib().vnx_resize_ingest_frames(
            buf.data_ptr(), buf.numel(), src.data_ptr(), dst.data_ptr(), coeffs.data_ptr(), coeffs.numel(), 1, 32, 32,
            0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0, 0, x.data_ptr(), mask.data_ptr(), _lib.current_stream(buf)))
    buf.copy_(buf2)
    x.fill_(float("nan"))
    mask.fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    want, want_mask = padded([resize.reference_resize(second[0], 24, 32)], (32, 32))
    assert torch.equal(x.cpu(), want) and torch.equal(mask.cpu().bool(), want_mask)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["cpu", DEV])
def test_the_python_op_stages_frames_from_the_host_and_from_the_device(where):
    """`stage_sources` + `resize_ingest_frames`: CPU frames (one pinned buffer, one copy) and frames already on the device
    (one cat, one small upload) give the same exact result, and the launch is counted"""
    sizes, targets = [(37, 53), (48, 64)], [(19, 27), (24, 32)]
    for layout in resize.LAYOUTS:
        frames = random_sources(sizes, seed=16, layout=layout)
        staged = resize.stage_sources([f.to(where) for f in frames], targets, DEV, layout)
        assert all(t.is_cuda for t in staged)
        calls = resize.CALLS["resize_ingest_frames"]
        x, mask = resize.resize_ingest_frames(*staged, 2, 32, 32, [0.0] * 3, [1.0] * 3, layout=layout)
        assert resize.CALLS["resize_ingest_frames"] == calls + 1
        want, want_mask = padded([as_chw(resize.reference_resize(f, nh, nw, layout), layout)
                                  for f, (nh, nw) in zip(frames, targets)], (32, 32))
        assert torch.equal(x.cpu(), want) and torch.equal(mask.cpu(), want_mask)


# ---- GPU, the models -------------------------------------------------------------------------------------------------------
class Spy:
    """what enters the backbone (x) and the transformer (masks, positions) on every forward"""

    def __init__(self, model):
        self.seen, self.hooks = [], []
        d = model.detr.detr
        self.hooks.append(d.backbone.register_forward_pre_hook(lambda m, args: self.seen.append(args[0].detach().clone())))
        self.hooks.append(d.transformer.register_forward_pre_hook(
            lambda m, args: self.seen.extend(t.detach().clone() for t in list(args[1]) + list(args[2]))))

    def take(self):
        out, self.seen = self.seen, []
        return out

    def remove(self):
        for h in self.hooks:
            h.remove()


def identical_network_inputs(on, off):
    assert len(on) == len(off) > 0
    for a, b in zip(on, off):
        assert a.dtype == b.dtype and torch.equal(a, b)


def run_models_on_gpu(model, n_frames):
    """switch on fed 48 x 80 sources (CHW and HWC) against switch off fed the host-resized frames, `device_ingest` on in both"""
    model.graph_inference = False
    T.enable_device_ingest(model)
    spy = Spy(model)
    results = {}
    for layout in resize.LAYOUTS:
        sources = random_sources([(48, 80)] * n_frames, seed=20, layout=layout)
        small = host_resized(sources, 24, 64, layout)
        off = model([{"image": small, "height": 48, "width": 80}])
        seen_off = spy.take()
        T.enable_device_resize(model)
        calls = resize.CALLS["resize_ingest_frames"]
        on = model([{"image": sources, "image_layout": layout}])
        seen_on = spy.take()
        assert resize.CALLS["resize_ingest_frames"] > calls                   # the op ran
        calls = resize.CALLS["resize_ingest_frames"]
        again = model([{"image": small, "height": 48, "width": 80}])          # frames already at their target
        spy.take()
        assert resize.CALLS["resize_ingest_frames"] == calls                  # ... it did not
        T.enable_device_resize(model, on=False)
        identical_network_inputs(seen_on, seen_off)
        same_video_result(on, off)
        same_video_result(again, off)
        results[layout] = (sources, off)
    spy.remove()
    return results


@pytest.mark.gpu
def test_seqformer_inference_with_the_switch_on_gpu():
    torch.manual_seed(5)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": DEV, **TINY_SEQ, **TEST_SIZE})).eval()
    results = run_models_on_gpu(model, 2)
    sources, off = results["hwc"]
    T.enable_device_resize(model)
    model.graph_inference = True
    video = [{"image": sources, "image_layout": "hwc"}]
    same_video_result(model(video), off)                 # captured ...
    same_video_result(model(video), off)                 # ... and replayed
    assert len(model._graphs) == 1
    key = next(iter(model._graphs))
    assert key[0] == "resize" and (48, 80) in key[3] and (24, 40) in key[4]      # keyed by source and target sizes


@pytest.mark.gpu
def test_idol_inference_with_the_switch_on_gpu():
    torch.manual_seed(6)
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": DEV, "MODEL.IDOL.BATCH_INFER_LEN": 2, **TINY_IDOL, **TEST_SIZE})).eval()
    results = run_models_on_gpu(model, 3)
    sources, off = results["chw"]
    T.enable_device_resize(model)
    model.graph_inference = True
    video = [{"image": sources}]
    same_video_result(model(video), off)                 # chunks of 2 + 1 frames: two graphs
    assert len(model._graphs) == 2 and all(k[0] == "resize" for k in model._graphs)
