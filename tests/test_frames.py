"""The front end both detectors share (vnext_amd/models/frames.py): frames -> network inputs, the pyramid levels' masks and
positions, the input kinds of an inference call and their graph keys, and the inference hipGraph cache.

CPU: the stack form against the list form, `level_inputs` with and without the table, `stage_chunk` for every input kind.
GPU: `replay_captured` through more shapes than the cache keeps, and the channels-last decision of the staged ingest."""
import pytest
import torch

from vnext_amd.models import frames as fr
from vnext_amd.models import resnet
from vnext_amd.ops import ingest, resize

DEV = "cuda:0"
STATS = ([123.675, 116.28, 103.53], [58.395, 57.12, 57.375])
MEAN, STD = (torch.tensor(v).view(3, 1, 1) for v in STATS)
LEVELS = [(8, 12), (4, 6), (2, 3), (1, 2)]


def float_frames(sizes, seed):
    """integer-valued float frames, as a decoder's bytes cast to float"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (3, h, w), generator=g).float() for h, w in sizes]


def sources(sizes, seed, layout="chw"):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (3, h, w) if layout == "chw" else (h, w, 3), dtype=torch.uint8, generator=g)
            for h, w in sizes]


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_stack_form_equals_list_form_on_same_sized_frames():
    frames = float_frames([(33, 65)] * 2, seed=1)      # padded 64 x 96: both axes padded, neither a multiple of 32
    x, mask = fr.pad_normalise(torch.stack(frames), MEAN, STD)
    lx, lmask = fr.pad_normalise_list(frames, MEAN, STD, "cpu")
    assert tuple(x.shape) == (2, 3, 64, 96) and tuple(mask.shape) == (2, 64, 96) and mask.dtype == torch.bool
    assert torch.equal(x, lx) and torch.equal(mask, lmask)
    assert not mask[:, :33, :65].any() and mask[:, 33:].all() and mask[:, :, 65:].all()


def test_list_form_pads_each_frame_of_unequal_sizes():
    sizes = [(33, 65), (40, 50)]
    frames = float_frames(sizes, seed=2)
    x, mask = fr.pad_normalise_list(frames, MEAN, STD, "cpu")
    assert tuple(x.shape) == (2, 3, 64, 96) and tuple(mask.shape) == (2, 64, 96)
    for i, (f, (h, w)) in enumerate(zip(frames, sizes)):
        want = torch.zeros(3, 64, 96)
        want[:, :h, :w] = (f - MEAN) / STD
        want_mask = torch.ones(64, 96, dtype=torch.bool)
        want_mask[:h, :w] = False
        assert torch.equal(x[i], want) and torch.equal(mask[i], want_mask)
        assert (x[i, :, h:] == 0).all() and (x[i, :, :, w:] == 0).all()


def test_level_inputs_with_the_table_equals_without():
    mask = torch.ones(2, 64, 96, dtype=torch.bool)
    mask[0, :33, :65] = False
    mask[1, :40, :50] = False
    table = torch.tensor([[0, 33, 65], [0, 40, 50]], dtype=torch.int32)
    srcs = [torch.zeros(2, 16, h, w) for h, w in LEVELS]
    masks, poss = fr.level_inputs(srcs, mask)
    tmasks, tposs = fr.level_inputs(srcs, mask, table)      # on the CPU the op is the reference expression
    assert len(masks) == len(poss) == len(tmasks) == len(tposs) == len(LEVELS)
    for (h, w), mk, ps, tmk, tps in zip(LEVELS, masks, poss, tmasks, tposs):
        assert tuple(mk.shape) == (2, h, w) and mk.dtype == torch.bool and tuple(ps.shape) == (2, 16, h, w)
        assert torch.equal(mk, tmk) and torch.equal(ps, tps)
        assert torch.equal(ps, ingest.sine_position(mk, 8))
    assert not masks[0].all() and masks[0].any()
    half = [s.to(torch.bfloat16) for s in srcs]             # the positions follow each level's dtype
    assert all(p.dtype == torch.bfloat16 for p in fr.level_inputs(half, mask)[1])
    assert all(p.dtype == torch.bfloat16 for p in fr.level_inputs(half, mask, table)[1])


def stage(frames, plan=None, device_ingest=False):
    return fr.stage_chunk(frames, plan, device_ingest, "cpu", STATS, MEAN, STD, None)


def test_stage_chunk_float_frames():
    frames = float_frames([(33, 65)] * 2, seed=3)
    s = stage(frames)
    assert s.key == (2, 3, 33, 65) and s.size == (64, 96) and len(s.tensors) == 1
    x, mask, table = s.to_net(*s.tensors)
    want = fr.pad_normalise(torch.stack(frames), MEAN, STD)
    assert table is None and torch.equal(x, want[0]) and torch.equal(mask, want[1])
    assert stage(float_frames([(33, 65), (40, 50)], seed=3)) is None      # unequal sizes: the eager list path


def test_stage_chunk_uint8_frames_with_and_without_the_switch():
    frames = sources([(33, 65)] * 2, seed=4)
    on = stage(frames, device_ingest=True)
    pixels, table = on.tensors
    assert len(on.tensors) == 2 and pixels.dtype == torch.uint8 and table.tolist() == [[0, 33, 65], [6448, 33, 65]]
    assert on.key == (tuple(pixels.shape), torch.uint8, 2, 64, 96) and on.size == (64, 96)
    off = stage(frames, device_ingest=False)                # switch off: the float stack
    assert off.key == (2, 3, 33, 65) and off.size == (64, 96) and len(off.tensors) == 1
    assert off.tensors[0].dtype == torch.float32
    x, mask, got_table = on.to_net(*on.tensors)
    fx, fmask, none = off.to_net(*off.tensors)
    assert got_table is table and none is None and torch.equal(x, fx) and torch.equal(mask, fmask)
    unequal = sources([(33, 65), (40, 50)], seed=4)
    assert stage(unequal, device_ingest=True) is None and stage(unequal, device_ingest=False) is None


@pytest.mark.parametrize("layout", resize.LAYOUTS)
def test_stage_chunk_resize_plan(layout):
    sizes = [(48, 80), (40, 72)]                            # staged whatever the sizes: the key carries them
    targets = [resize.shortest_edge_size(h, w, 24, 64) for h, w in sizes]
    assert targets == [(24, 40), (24, 43)]
    frames = sources(sizes, seed=5, layout=layout)
    s = stage(frames, (targets, layout))
    assert len(s.tensors) == 4 and s.size == (32, 64)
    assert s.key == ("resize", tuple(s.tensors[0].shape), layout, ((48, 80), (40, 72)), ((24, 40), (24, 43)), 32, 64)
    x, mask, table = s.to_net(*s.tensors)
    assert table is s.tensors[2] and table.tolist() == [[0, 24, 40], [0, 24, 43]]
    small = [resize.reference_resize(f, nh, nw, layout) for f, (nh, nw) in zip(frames, targets)]
    small = [f if layout == "chw" else f.permute(2, 0, 1) for f in small]
    want_x, want_mask = fr.pad_normalise_list(small, MEAN, STD, "cpu")
    assert torch.equal(x, want_x) and torch.equal(mask, want_mask)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_replay_captured_returns_each_calls_result_and_evicts_the_oldest():
    cache = {}
    fn = lambda a, b: (a * 2 + b,)      # noqa: E731
    g = torch.Generator().manual_seed(6)

    def call(k):
        a, b = (torch.randn(k, 8, generator=g).to(DEV) for _ in range(2))
        out, = fr.replay_captured(cache, k, (a, b), fn)
        assert torch.equal(out, a * 2 + b), k
    for k in range(1, 6):
        call(k)
        assert len(cache) == min(k, 4)
    call(5)                               # a replay with new values: the new result, not the captured one
    assert list(cache) == [2, 3, 4, 5]    # the oldest went at the fifth


@pytest.mark.gpu
def test_staged_ingest_is_channels_last_exactly_where_the_trunk_converts(monkeypatch):
    trunk = resnet.ResNet50Trunk().to(DEV)
    frames = sources([(32, 32)] * 2, seed=7)
    big = sources([(64, 64)] * 2, seed=8)

    def staged():
        x, _, _ = fr.ingest_staged(*ingest.stage_frames(frames, DEV), 2, 32, 32, STATS, trunk)
        rx, _, _ = fr.resize_staged(*resize.stage_sources(big, [(32, 32)] * 2, DEV), 2, 32, 32, "chw", STATS)
        assert tuple(x.shape) == tuple(rx.shape) == (2, 3, 32, 32) and rx.is_contiguous()      # the resize form: never
        return x
    with torch.enable_grad():
        monkeypatch.setattr(resnet, "CHANNELS_LAST", True)      # on the module, as train.enable_channels_last sets it
        trunk.train()
        x = staged()
        assert x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()
        trunk.eval()
        assert staged().is_contiguous()
        monkeypatch.setattr(resnet, "CHANNELS_LAST", False)
        trunk.train()
        assert staged().is_contiguous()
