"""uint8 frames ingested on the device (vnext_amd/csrc/ingest.hip, vnext_amd/ops/ingest.py): normalise + pad + padding mask
in one launch, the per-level masks and sine positions in one more, and the models' `device_ingest` switch.

CPU: the switch, the op as the reference expression, the staging buffer, the closed forms the kernel relies on.
GPU: the kernels through the C ABI with guard words around pre-poisoned outputs, then the models.

Positions are checked in two kinds.  (a) the coordinate's row / column normaliser is > 0: the kernel's absolute error against
the reference expression in float64 is at most max(2 x the eager GPU fp32 chain's error at the same positions, 3e-6) -- the
values lie in [-1, 1], and 3e-6 is the fp32 floor of tests/test_swin_glue.py.  (b) the normaliser is 0: the sine's argument is
about -3.1e6 / dim_t, so only `torch.equal` with the eager GPU chain means anything; the op's `degenerate` table makes it
possible.  Both kinds must occur in every batch below; a single level cannot always hold both (a 1 x 1 level of a batch
whose frames all have a pixel is valid everywhere), so emptiness is asserted per batch and on the named example."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vnext_amd.models  # noqa: F401  (registers the meta-archs)
from vnext_amd import train as T
from vnext_amd.models import idol as idol_mod
from vnext_amd.models import seqformer as sf
from vnext_amd.models import tracker as trk
from vnext_amd.models.seqformer import sine_position
from vnext_amd.ops import ingest
from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg

DEV = "cuda:0"
TINY_SEQ = {"MODEL.SeqFormer.ENC_LAYERS": 1, "MODEL.SeqFormer.DEC_LAYERS": 2, "MODEL.SeqFormer.NUM_OBJECT_QUERIES": 12,
            "MODEL.SeqFormer.DIM_FEEDFORWARD": 64, "MODEL.SeqFormer.DROPOUT": 0.0, "INPUT.SAMPLING_FRAME_NUM": 2}
TINY_IDOL = {"MODEL.IDOL.ENC_LAYERS": 1, "MODEL.IDOL.DEC_LAYERS": 2, "MODEL.IDOL.NUM_OBJECT_QUERIES": 110,
             "MODEL.IDOL.DIM_FEEDFORWARD": 64, "MODEL.IDOL.DROPOUT": 0.0}
ARBITRARY = ([0.1, 77.77, 200.3], [0.37, 3.0, 191.123])
BATCH_64 = ([(37, 50), (33, 64), (64, 33), (1, 1)], (64, 64), [(8, 8), (4, 4), (2, 2), (1, 1)])
BATCH_96 = ([(90, 150)], (96, 160), [(12, 20), (6, 10), (3, 5), (2, 3)])
BATCH_96_SMALL = ([(10, 10), (90, 150)], (96, 160), [(12, 20), (6, 10), (3, 5), (2, 3)])      # degenerate rows at every level
BATCH_WIDTHS = ([(5, 15), (5, 16), (5, 17)], (32, 32), [(4, 4), (2, 2), (1, 1)])
FP32_FLOOR = 3e-6


def model_stats():
    cfg = get_seqformer_cfg(**{"MODEL.DEVICE": "cpu"})
    return [float(v) for v in cfg.MODEL.PIXEL_MEAN], [float(v) for v in cfg.MODEL.PIXEL_STD]


def as_f32(values):
    """the float32 values of three numbers, as python floats"""
    return torch.tensor(values, dtype=torch.float32).tolist()


def random_frames(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g) for h, w in sizes]


def pack_odd(frames, room=None):
    """the frames' planes in one host buffer, every frame at an ODD byte offset -> (buffer uint8, table int32 [n, 3])"""
    rows, off = [], 1
    for f in frames:
        rows.append((off, f.shape[1], f.shape[2]))
        off += f.numel()
        off += 1 - off % 2
    buf = torch.full((room or off + 3,), 0xAB, dtype=torch.uint8)
    for f, (o, h, w) in zip(frames, rows):
        buf[o:o + f.numel()] = f.reshape(-1)
    return buf, torch.tensor(rows, dtype=torch.int32)


def eager_cpu(frames, size, mean, std):
    """the models' eager normalise + pad on the CPU (IEEE) -> x [B, 3, H, W], mask [B, H, W]"""
    H, W = size
    m, s = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1), torch.tensor(std, dtype=torch.float32).view(3, 1, 1)
    x = torch.zeros(len(frames), 3, H, W)
    mask = torch.ones(len(frames), H, W, dtype=torch.bool)
    for i, f in enumerate(frames):
        x[i, :, :f.shape[1], :f.shape[2]] = (f.float() - m) / s
        mask[i, :f.shape[1], :f.shape[2]] = False
    return x, mask


def sine_position64(mask, num_pos_feats, temperature=10000):
    """`sine_position` with every operation in float64"""
    not_mask = ~mask
    y_embed = not_mask.cumsum(1, dtype=torch.float64)
    x_embed = not_mask.cumsum(2, dtype=torch.float64)
    eps, scale = 1e-6, 2 * math.pi
    y_embed = (y_embed - 0.5) / (y_embed[:, -1:, :] + eps) * scale
    x_embed = (x_embed - 0.5) / (x_embed[:, :, -1:] + eps) * scale
    dim_t = torch.arange(num_pos_feats, dtype=torch.float64)
    dim_t = temperature ** (2 * (dim_t // 2) / num_pos_feats)
    pos_x = x_embed[:, :, :, None] / dim_t
    pos_y = y_embed[:, :, :, None] / dim_t
    pos_x = torch.stack((pos_x[..., 0::2].sin(), pos_x[..., 1::2].cos()), dim=4).flatten(3)
    pos_y = torch.stack((pos_y[..., 0::2].sin(), pos_y[..., 1::2].cos()), dim=4).flatten(3)
    return torch.cat((pos_y, pos_x), dim=3).permute(0, 3, 1, 2)


def degenerate_positions(level_mask, num_pos_feats):
    """bool [B, 2 npf, h, w]: the positions whose normaliser is 0 (pos_y: a column without a valid pixel; pos_x: a row)"""
    valid = ~level_mask.cpu()
    col, row = valid.any(1), valid.any(2)                     # [B, w], [B, h]
    B, h, w = valid.shape
    deg_y = (~col)[:, None, None, :].expand(B, num_pos_feats, h, w)
    deg_x = (~row)[:, None, :, None].expand(B, num_pos_feats, h, w)
    return torch.cat([deg_y, deg_x], 1)


def check_positions(level_mask, got, eager, num_pos_feats, what):
    """the two-kind position check of the module docstring -> (degenerate count, regular count)"""
    deg = degenerate_positions(level_mask, num_pos_feats)
    got, eager = got.detach().cpu(), eager.detach().cpu()
    assert got.shape == eager.shape == deg.shape
    assert torch.equal(got[deg], eager[deg]), f"{what}: degenerate positions differ from the eager chain"
    if (~deg).any():
        ref = sine_position64(level_mask.cpu(), num_pos_feats)
        err_kernel = float((got.double() - ref)[~deg].abs().max())
        err_eager = float((eager.double() - ref)[~deg].abs().max())
        print(f"{what}: kernel error {err_kernel:.3e}, eager fp32 chain error {err_eager:.3e}, "
              f"{int(deg.sum())} degenerate / {int((~deg).sum())} regular values")
        assert err_kernel <= max(2 * err_eager, FP32_FLOOR), (what, err_kernel, err_eager)
    return int(deg.sum()), int((~deg).sum())


@pytest.fixture
def cpu_stand_ins(monkeypatch):
    """PyTorch restatements (oracle/, tests only) of the HIP entry points the models call, so they run on CPU."""
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
    """the tolerance of tests/test_model_ddp.py::test_graph_replayed_inference_equals_eager_on_gpu"""
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
def test_enable_device_ingest_flips_both_models_and_raises_without_the_switch():
    seq = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": "cpu", **TINY_SEQ}))
    idol = build_model(get_idol_cfg(**{"MODEL.DEVICE": "cpu", **TINY_IDOL}))
    for model in (seq, idol):
        assert model.device_ingest is False
        T.enable_device_ingest(model)
        assert model.device_ingest is True
        T.enable_device_ingest(model, on=False)
        assert model.device_ingest is False
    with pytest.raises(ValueError, match="device_ingest"):
        T.enable_device_ingest(torch.nn.Linear(2, 2))


def test_the_build_keeps_correctly_rounded_fp32_division():
    """the pixel pass is exact only with IEEE division: hipcc's default, which no build flag may switch off"""
    from vnext_amd import build
    flags = " ".join(build.HIPCC_FLAGS)
    for opt_out in ("-ffast-math", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-freciprocal-math", "-Ofast",
                    "-funsafe-math-optimizations"):
        assert opt_out not in flags


def test_seqformer_eval_with_the_switch_equals_without_on_cpu(cpu_stand_ins):
    torch.manual_seed(3)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": "cpu", **TINY_SEQ})).eval()
    for sizes in ([(40, 70), (40, 70)], [(40, 70), (33, 50)]):      # the clip trunk, and the padded-batch path
        video = [{"image": random_frames(sizes, seed=4), "height": 40, "width": 70}]
        off = model(video)
        calls = dict(ingest.CALLS)
        T.enable_device_ingest(model)
        on = model(video)
        T.enable_device_ingest(model, on=False)
        assert ingest.CALLS == calls                    # on the CPU the op is the reference expression: no launch
        same_video_result(on, off, score_rtol=1e-6, mask_frac=1e-6)


def test_idol_eval_with_the_switch_equals_without_on_cpu(cpu_stand_ins):
    torch.manual_seed(3)
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": "cpu", "MODEL.IDOL.BATCH_INFER_LEN": 2, **TINY_IDOL})).eval()
    video = [{"image": random_frames([(40, 70)] * 3, seed=5), "height": 44, "width": 72}]
    off = model(video)
    T.enable_device_ingest(model)
    on = model(video)
    same_video_result(on, off, score_rtol=1e-6, mask_frac=1e-6)


def test_stage_frames_round_trips_frames_of_unequal_sizes():
    frames = random_frames([(7, 9), (1, 1), (16, 5), (3, 33)], seed=6)
    pixels, table = ingest.stage_frames(frames, "cpu")
    assert pixels.dtype == torch.uint8 and table.dtype == torch.int32 and tuple(table.shape) == (4, 3)
    assert pixels.data_ptr() % 16 == 0
    for f, (o, h, w) in zip(frames, table.tolist()):
        assert (h, w) == tuple(f.shape[1:]) and o % 16 == 0
        assert torch.equal(pixels[o:o + 3 * h * w].view(3, h, w), f)
    x, mask = ingest.ingest_frames(pixels, table, 4, 32, 64, *model_stats())
    want_x, want_mask = eager_cpu(frames, (32, 64), *model_stats())
    assert torch.equal(x, want_x) and torch.equal(mask, want_mask)


def test_closed_form_cumsums_equal_the_cumsums_for_every_rectangle():
    for vh in range(9):
        for vw in range(9):
            not_mask = torch.zeros(8, 8, dtype=torch.bool)
            not_mask[:vh, :vw] = True
            ys, xs = ingest.closed_form_embeds(8, 8, vh, vw)
            assert torch.equal(ys, not_mask.cumsum(0, dtype=torch.float32)), (vh, vw)
            assert torch.equal(xs, not_mask.cumsum(1, dtype=torch.float32)), (vh, vw)


def test_a_resized_rectangle_mask_is_a_rectangle_with_the_bisected_counts():
    """what the level pass relies on: torch's nearest resize of a top-left rectangle's complement is one again, with
    as many valid rows / columns as destination indices whose fp32 source index lies inside the frame"""
    def count(out, full, valid):
        scale = np.float32(full) / np.float32(out)
        src = np.minimum(np.floor(np.arange(out, dtype=np.float32) * scale).astype(np.int64), full - 1)
        assert (np.diff(src) >= 0).all()
        return int((src < valid).sum())
    for frames, (H, W), levels in (BATCH_64, BATCH_96, BATCH_96_SMALL, BATCH_WIDTHS, ([(360, 640), (300, 500)], (384, 640),
                                                                                   [(48, 80), (24, 40), (12, 20), (6, 10)])):
        mask = torch.ones(len(frames), H, W, dtype=torch.bool)
        for i, (h, w) in enumerate(frames):
            mask[i, :h, :w] = False
        for lh, lw in levels:
            mk = F.interpolate(mask[None].float(), size=(lh, lw)).to(torch.bool)[0]
            for i, (h, w) in enumerate(frames):
                want = torch.ones(lh, lw, dtype=torch.bool)
                want[:count(lh, H, h), :count(lw, W, w)] = False
                assert torch.equal(mk[i], want), (frames[i], (lh, lw))


# ---- GPU, through the C ABI ------------------------------------------------------------------------------------------------
GUARD = 64


def c_frames(buf, table, B, H, W, mean, std, channels_last):
    """vnx_ingest_frames into NaN / 0xFF pre-filled outputs with guard words around them -> x [B, 3, H, W] (a view of
    the layout asked for), mask uint8 [B, H, W]"""
    from vnext_amd import _lib
    xs = torch.full((B * 3 * H * W + 2 * GUARD,), float("nan"), device=DEV)
    ms = torch.full((B * H * W + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().vnx_ingest_frames(buf.data_ptr(), buf.numel(), table.data_ptr(), B, H, W, *as_f32(mean),
                                            *as_f32(std), int(channels_last), xs[GUARD:].data_ptr(), ms[GUARD:].data_ptr(),
                                            _lib.current_stream(buf)))
    torch.cuda.synchronize()
    assert torch.isnan(xs[:GUARD]).all() and torch.isnan(xs[-GUARD:]).all(), "x: a guard word was written"
    assert (ms[:GUARD] == 0xFF).all() and (ms[-GUARD:] == 0xFF).all(), "mask: a guard byte was written"
    x, mask = xs[GUARD:-GUARD], ms[GUARD:-GUARD].view(B, H, W)
    assert not torch.isnan(x).any(), "x: an element was not written"
    assert (mask <= 1).all(), "mask: an element was not written"
    x = x.view(B, H, W, 3).permute(0, 3, 1, 2) if channels_last else x.view(B, 3, H, W)
    return x, mask


def level_buffers(B, levels, npf):
    return ([torch.full((B * h * w + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=DEV) for h, w in levels],
            [torch.full((B * h * w * 2 * npf + 2 * GUARD,), float("nan"), device=DEV) for h, w in levels])


def c_levels(table, B, H, W, levels, npf, outs=None):
    """vnx_ingest_levels into pre-filled, guarded outputs -> (masks uint8 [B, h, w], positions [B, 2 npf, h, w] views).
    outs: the (mask buffers, position buffers) of an earlier call, to write into again"""
    from vnext_amd import _lib
    dim_t, degenerate = ingest.position_tables(DEV, npf)
    n = len(levels)
    mbuf, pbuf = outs = outs or level_buffers(B, levels, npf)
    sizes = (ctypes.c_int * (2 * n))(*[v for s in levels for v in s])
    mptr = (ctypes.c_void_p * n)(*[m[GUARD:].data_ptr() for m in mbuf])
    pptr = (ctypes.c_void_p * n)(*[p[GUARD:].data_ptr() for p in pbuf])
    _lib.check(_lib.lib().vnx_ingest_levels(table.data_ptr(), B, H, W, n, sizes, npf, dim_t.data_ptr(),
                                            degenerate.data_ptr(), mptr, pptr, _lib.current_stream(table)))
    return outs


def read_levels(outs, B, levels, npf):
    torch.cuda.synchronize()
    masks, poss = [], []
    for (h, w), m, p in zip(levels, *outs):
        assert (m[:GUARD] == 0xFF).all() and (m[-GUARD:] == 0xFF).all(), "level mask: a guard byte was written"
        assert torch.isnan(p[:GUARD]).all() and torch.isnan(p[-GUARD:]).all(), "positions: a guard word was written"
        mk, ps = m[GUARD:-GUARD].view(B, h, w), p[GUARD:-GUARD].view(B, h, w, 2 * npf)
        assert (mk <= 1).all(), "level mask: an element was not written"
        assert not torch.isnan(ps).any(), "positions: an element was not written"
        masks.append(mk)
        poss.append(ps.permute(0, 3, 1, 2))
    return masks, poss


@pytest.mark.gpu
@pytest.mark.parametrize("stats", ["model", "arbitrary"])
def test_every_byte_value_is_normalised_exactly(stats):
    """all 256 byte values x 3 channels against (u.float() - mean) / std on the CPU (IEEE), bit for bit"""
    mean, std = model_stats() if stats == "model" else ARBITRARY
    frame = torch.arange(256, dtype=torch.uint8).view(1, 16, 16).repeat(3, 1, 1)
    frame[1] = frame[1].flip(1)
    frame[2] = frame[2].t().clone()
    buf, table = pack_odd([frame])
    want, want_mask = eager_cpu([frame], (32, 32), mean, std)
    for channels_last in (False, True):
        x, mask = c_frames(buf.to(DEV), table.to(DEV), 1, 32, 32, mean, std, channels_last)
        assert torch.equal(x.cpu(), want) and torch.equal(mask.cpu().bool(), want_mask)
    m = torch.tensor(mean, device=DEV).view(3, 1, 1)
    s = torch.tensor(std, device=DEV).view(3, 1, 1)
    eager = ((frame.to(DEV).float() - m) / s).cpu()
    ulps = (eager.view(torch.int32).long() - want[0, :, :16, :16].contiguous().view(torch.int32).long()).abs().max()
    print(f"{stats}: ATen's device division differs from IEEE by at most {int(ulps)} ulp on the 768 values")


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [BATCH_64, BATCH_96, BATCH_WIDTHS], ids=["64x64", "96x160", "widths-15-16-17"])
def test_frames_at_odd_offsets_fill_both_layouts(batch):
    sizes, (H, W), _ = batch
    frames = random_frames(sizes, seed=11)
    buf, table = pack_odd(frames)
    assert all(o % 2 == 1 for o, _, _ in table.tolist())
    mean, std = model_stats()
    want, want_mask = eager_cpu(frames, (H, W), mean, std)
    for channels_last in (False, True):
        x, mask = c_frames(buf.to(DEV), table.to(DEV), len(frames), H, W, mean, std, channels_last)
        assert torch.equal(x.cpu(), want), f"channels_last={channels_last}"
        assert (x.cpu()[want_mask[:, None].expand_as(want)] == 0).all()
        assert torch.equal(mask.cpu().bool(), want_mask)
        again, mask_again = c_frames(buf.to(DEV), table.to(DEV), len(frames), H, W, mean, std, channels_last)
        assert torch.equal(again, x) and torch.equal(mask_again, mask)          # bit-identical run to run


@pytest.mark.gpu
def test_a_table_row_outside_the_buffer_is_an_empty_frame():
    frames = random_frames([(20, 20), (20, 20)], seed=12)
    buf, table = pack_odd(frames)
    table[1, 0] = buf.numel() - 100                      # the second frame's planes would end beyond the buffer
    x, mask = c_frames(buf.to(DEV), table.to(DEV), 2, 32, 32, *model_stats(), False)
    want, want_mask = eager_cpu(frames[:1], (32, 32), *model_stats())
    assert torch.equal(x[0].cpu(), want[0]) and torch.equal(mask[0].cpu().bool(), want_mask[0])
    assert (x[1] == 0).all() and (mask[1] == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [BATCH_64, BATCH_96, BATCH_96_SMALL], ids=["64x64", "96x160", "96x160-small"])
def test_level_masks_and_positions(batch):
    sizes, (H, W), levels = batch
    B, npf = len(sizes), 128
    table = torch.tensor([(0, h, w) for h, w in sizes], dtype=torch.int32, device=DEV)
    mask = torch.ones(B, H, W, dtype=torch.bool, device=DEV)
    for i, (h, w) in enumerate(sizes):
        mask[i, :h, :w] = False
    masks, poss = read_levels(c_levels(table, B, H, W, levels, npf), B, levels, npf)
    again = read_levels(c_levels(table, B, H, W, levels, npf), B, levels, npf)
    counts = []
    for (h, w), mk, ps, mk2, ps2 in zip(levels, masks, poss, *again):
        want = F.interpolate(mask[None].float(), size=(h, w)).to(torch.bool)[0]
        assert torch.equal(mk.bool(), want), (h, w)
        counts.append(check_positions(want, ps, sine_position(want, npf), npf, f"{H}x{W} level {h}x{w}"))
        assert torch.equal(mk2, mk) and torch.equal(ps2, ps)                       # bit-identical run to run
    assert sum(c[0] for c in counts) > 0 and sum(c[1] for c in counts) > 0         # both kinds occur in the batch
    if batch is BATCH_64:      # the 37 x 50 frame at (8, 8): 5 valid rows and 3 degenerate ones
        valid_rows = (~F.interpolate(mask[None].float(), size=(8, 8)).to(torch.bool)[0][0]).any(1).cpu()
        assert valid_rows.tolist() == [True] * 5 + [False] * 3
        assert counts[0][0] > 0 and counts[0][1] > 0
    if batch is BATCH_96_SMALL:
        assert all(c[0] > 0 and c[1] > 0 for c in counts)


@pytest.mark.gpu
def test_small_position_widths_and_the_reference_route():
    """num_pos_feats 16 (a tiny hidden size) through the kernel; a width it does not have through the reference expression"""
    sizes, (H, W), levels = BATCH_64
    frames = random_frames(sizes, seed=13)
    pixels, table = ingest.stage_frames(frames, DEV)
    _, mask = ingest.ingest_frames(pixels, table, len(frames), H, W, *model_stats())
    calls = ingest.CALLS["level_constants"]
    for npf, launched in ((16, 1), (6, 0)):
        masks, poss = ingest.level_constants(table, len(frames), H, W, levels, npf)
        assert ingest.CALLS["level_constants"] == calls + launched
        calls += launched
        for (h, w), mk, ps in zip(levels, masks, poss):
            want = F.interpolate(mask[None].float(), size=(h, w)).to(torch.bool)[0]
            assert torch.equal(mk, want) and tuple(ps.shape) == (len(frames), 2 * npf, h, w)
            check_positions(want, ps, sine_position(want, npf), npf, f"npf {npf} level {h}x{w}")


@pytest.mark.gpu
def test_a_captured_call_replays_on_new_pixels_and_new_sizes():
    """capture on one set of frames; overwrite pixels AND sizes in place (same H, W, other h_i, w_i); poison the outputs;
    replay; the result is the eager call's on the new set"""
    from vnext_amd import _lib
    (H, W), levels, npf, B = (64, 64), [(8, 8), (4, 4), (2, 2), (1, 1)], 128, 3
    first = random_frames([(37, 50), (64, 64), (20, 33)], seed=14)
    second = random_frames([(50, 37), (9, 64), (64, 1)], seed=15)
    room = 3 * B * H * W + 64
    buf1, table1 = pack_odd(first, room)
    buf2, table2 = pack_odd(second, room)
    mean, std = model_stats()
    buf, table = buf1.to(DEV), table1.to(DEV)
    ingest.position_tables(DEV, npf)                     # made outside the capture
    x = torch.full((B, 3, H, W), float("nan"), device=DEV)
    mask = torch.full((B, H, W), 0xFF, dtype=torch.uint8, device=DEV)
    outs = level_buffers(B, levels, npf)
    stats = as_f32(mean) + as_f32(std)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.check(_lib.lib().vnx_ingest_frames(buf.data_ptr(), buf.numel(), table.data_ptr(), B, H, W, *stats, 0,
                                                x.data_ptr(), mask.data_ptr(), _lib.current_stream(buf)))
        c_levels(table, B, H, W, levels, npf, outs)
    buf.copy_(buf2)
    table.copy_(table2)
    x.fill_(float("nan"))
    mask.fill_(0xFF)
    for t in outs[0]:
        t.fill_(0xFF)
    for t in outs[1]:
        t.fill_(float("nan"))
    graph.replay()
    masks, poss = read_levels(outs, B, levels, npf)
    want_x, want_mask = c_frames(buf, table, B, H, W, mean, std, False)
    eager_masks, eager_poss = read_levels(c_levels(table, B, H, W, levels, npf), B, levels, npf)
    cpu_x, cpu_mask = eager_cpu(second, (H, W), mean, std)
    assert torch.equal(x, want_x) and torch.equal(mask, want_mask)
    assert torch.equal(x.cpu(), cpu_x) and torch.equal(mask.cpu().bool(), cpu_mask)
    for a, b, c, d in zip(masks, eager_masks, poss, eager_poss):
        assert torch.equal(a, b) and torch.equal(c, d)
    second_mask = F.interpolate(cpu_mask[None].float(), size=(8, 8)).to(torch.bool)[0]
    assert torch.equal(masks[0].cpu().bool(), second_mask)


# ---- GPU, the models -------------------------------------------------------------------------------------------------------
class Spy:
    """what enters the backbone (x) and the transformer (masks, positions) on every forward"""

    def __init__(self, model):
        self.x, self.masks, self.poss, self.hooks = [], [], [], []
        d = model.detr.detr
        self.hooks.append(d.backbone.register_forward_pre_hook(lambda m, args: self.x.append(args[0].detach().clone())))
        self.hooks.append(d.transformer.register_forward_pre_hook(self._transformer))

    def _transformer(self, module, args):
        self.masks.append([m.detach().clone() for m in args[1]])
        self.poss.append([p.detach().clone() for p in args[2]])

    def take(self):
        out = (self.x, self.masks, self.poss)
        self.x, self.masks, self.poss = [], [], []
        return out

    def remove(self):
        for h in self.hooks:
            h.remove()


def compare_network_inputs(on, off, npf):
    (x_on, masks_on, poss_on), (x_off, masks_off, poss_off) = on, off
    assert len(x_on) == len(x_off) > 0
    for a, b in zip(x_on, x_off):
        assert torch.equal(a, b)
    for call, (ma, mb, pa, pb) in enumerate(zip(masks_on, masks_off, poss_on, poss_off)):
        for lvl, (a, b, p, q) in enumerate(zip(ma, mb, pa, pb)):
            assert torch.equal(a, b)
            level_mask = b.reshape(-1, *b.shape[-2:])
            check_positions(level_mask, p.reshape(-1, *p.shape[-3:]), q.reshape(-1, *q.shape[-3:]), npf,
                            f"forward {call} level {lvl}")


@pytest.mark.gpu
def test_seqformer_inference_with_the_switch_on_gpu():
    torch.manual_seed(5)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": DEV, **TINY_SEQ})).eval()
    videos = [[{"image": random_frames([(90, 150)] * 2, seed=20 + i), "height": 90, "width": 150}] for i in range(2)]
    videos += [[{"image": random_frames([(64, 120)] * 2, seed=30), "height": 64, "width": 120}]]
    mixed = [{"image": random_frames([(90, 150), (70, 100)], seed=31), "height": 90, "width": 150}]
    spy = Spy(model)
    model.graph_inference = False
    off = [model(v) for v in videos + [mixed]]
    seen_off = spy.take()
    T.enable_device_ingest(model)
    calls = dict(ingest.CALLS)
    on = [model(v) for v in videos + [mixed]]
    seen_on = spy.take()
    assert ingest.CALLS["ingest_frames"] == calls["ingest_frames"] + 4
    assert ingest.CALLS["level_constants"] == calls["level_constants"] + 4
    compare_network_inputs(seen_on, seen_off, 128)
    for a, b in zip(on, off):
        same_video_result(a, b)
    spy.remove()
    model.graph_inference = True
    graphed = [model(v) for v in videos]                 # two sizes: two graphs; the second video replays the first
    assert len(model._graphs) == 2 and all(k[1] == torch.uint8 for k in model._graphs)
    for a, b in zip(graphed, off):
        same_video_result(a, b)
    calls = dict(ingest.CALLS)                            # float frames: today's path whatever the switch says
    model.graph_inference = False
    floats = [{"image": [f.float() for f in videos[0][0]["image"]], "height": 90, "width": 150}]
    same_video_result(model(floats), off[0])
    assert ingest.CALLS == calls


@pytest.mark.gpu
def test_idol_inference_and_a_training_step_with_the_switch_on_gpu():
    torch.manual_seed(6)
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": DEV, **TINY_IDOL})).eval()
    frames = random_frames([(90, 150)] * 2, seed=40)

    def candidates():
        return model.inference_forward(frames)

    def same_candidates(a, b):
        assert len(a) == len(b)
        for fa, fb in zip(a, b):
            assert fa["indices"] == fb["indices"]
            np.testing.assert_allclose(fa["logits"].sigmoid().cpu().numpy(), fb["logits"].sigmoid().cpu().numpy(), rtol=1e-5)
            assert float(((fa["masks"] > 0) != (fb["masks"] > 0)).float().mean()) < 1e-3
    spy = Spy(model)
    model.graph_inference = False
    off = candidates()
    seen_off = spy.take()
    T.enable_device_ingest(model)
    calls = dict(ingest.CALLS)
    on = candidates()
    seen_on = spy.take()
    spy.remove()
    assert ingest.CALLS["ingest_frames"] == calls["ingest_frames"] + 1
    assert ingest.CALLS["level_constants"] == calls["level_constants"] + 1
    compare_network_inputs(seen_on, seen_off, 128)
    same_candidates(on, off)
    model.graph_inference = True
    same_candidates(candidates(), off)                   # captured ...
    same_candidates(candidates(), off)                   # ... and replayed
    assert len(model._graphs) == 1 and next(iter(model._graphs))[1] == torch.uint8

    def step(switch):
        import random
        torch.manual_seed(7)
        random.seed(7)
        np.random.seed(7)
        m = build_model(get_idol_cfg(**{"MODEL.DEVICE": DEV, **TINY_IDOL})).train()
        T.enable_device_ingest(m, switch)
        pairs = T.synthetic_clips(1, 2, 90, 150, DEV, seed=8, num_instances=2)
        for p in pairs:
            p["image"] = [f.to(torch.uint8).cpu() for f in p["image"]]
        before = ingest.CALLS["ingest_frames"]
        losses = m(pairs)
        assert ingest.CALLS["ingest_frames"] == before + int(switch)
        return {k: float(v.detach()) for k, v in losses.items()}
    want, got = step(False), step(True)
    assert set(want) == set(got)
    for k in want:      # the loss tolerance of tests/test_model_ddp.py's captured-trunk test
        np.testing.assert_allclose(got[k], want[k], rtol=2e-4, atol=1e-5, err_msg=k)
