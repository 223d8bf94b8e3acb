"""`device_masks` (train.enable_device_masks): the models' three dense mask sites -- `SeqFormer._report`,
`IDOL._track_masks`, `IDOL.coco_postprocess` -- through vnext_amd/ops/mask_dense.py, against the eager chain they replace.
The sites are called on fixed tensors, with no forward pass, so the comparison is exact."""
import numpy as np
import pytest
import torch

from test_mask_rle import BAND, IDOL_TINY, SEQ_TINY, _video, bilinear_f64, blob_logits
from vnext_amd import train as T
from vnext_amd.models.idol import IDOL
from vnext_amd.ops import mask_dense
from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg

H, W = 45, 80                      # stride-4 logit maps of a 180 x 320 input
IMAGE = (180, 320)
_MODELS = {}


def seqformer(device):
    if ("seq", device) not in _MODELS:
        torch.manual_seed(4)
        _MODELS["seq", device] = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": device, **SEQ_TINY})).eval()
    return _MODELS["seq", device]


def idol(device, coco=False):
    if ("idol", device, coco) not in _MODELS:
        torch.manual_seed(4)
        cfg = {"MODEL.DEVICE": device, "INPUT.COCO_PRETRAIN": coco, "MODEL.IDOL.BATCH_INFER_LEN": 2, **IDOL_TINY}
        _MODELS["idol", device, coco] = build_model(get_idol_cfg(**cfg)).eval()
    return _MODELS["idol", device, coco]


class Switched:
    """the model's switch held at a value inside a `with`"""

    def __init__(self, model, on):
        self.model, self.on = model, on

    def __enter__(self):
        self.keep = self.model.device_masks
        T.enable_device_masks(self.model, self.on)

    def __exit__(self, *exc):
        self.model.device_masks = self.keep


def assert_band_empty(logits, image, out):
    assert not (np.abs(bilinear_f64(logits.cpu(), 4, image, out)) < BAND).any(), (image, out)


# ---- the three sites on fixed tensors ----------------------------------------------------------------------------------
def report_case(device):
    """3 of 4 queries reported, query 0 under two classes; 2 frames"""
    model = seqformer(device)
    model.multi_cls, model.cls_thres = True, 0.5
    prob = torch.full((4, model.num_classes), 0.1)
    prob[0, 3], prob[0, 7], prob[1, 2], prob[3, 0] = 0.9, 0.8, 0.7, 0.6
    logits = blob_logits(8, H, W, seed=64).view(4, 2, H, W)
    return model, prob.to(device), logits.to(device)


def run_report(device, on, out):
    model, prob, logits = report_case(device)
    with Switched(model, on):
        return model._report(prob, logits, IMAGE, out)


def assert_same_report(a, b, out):
    assert a["pred_scores"] == b["pred_scores"] and a["pred_labels"] == b["pred_labels"] == [3, 7, 2, 0]
    assert a["image_size"] == b["image_size"] and len(a["pred_masks"]) == len(b["pred_masks"]) == 4
    for x, y in zip(a["pred_masks"], b["pred_masks"]):
        assert x.dtype == y.dtype == torch.bool and x.device == y.device == torch.device("cpu")
        assert tuple(x.shape) == tuple(y.shape) == (2,) + tuple(out)
        assert torch.equal(x, y)


def track_case(device):
    """3 tracks over 4 frames, absent from some; 7 seen frames"""
    maps = blob_logits(7, H, W, seed=64).to(device)
    present = [[True, False, True, True], [False, True, True, False], [True, True, False, False]]
    it = iter(maps)
    return [{"masks": [next(it)[None] if p else None for p in row]} for row in present], present


def run_tracks(device, on, out):
    tracks, present = track_case(device)
    return IDOL._track_masks(tracks, 4, IMAGE, out, device_masks=on), present


def assert_same_tracks(a, b, present, out):
    assert len(a) == len(b) == len(present)
    for ta, tb, row in zip(a, b, present):
        assert len(ta) == len(tb) == 4
        for x, y, p in zip(ta, tb, row):
            if not p:
                assert x is None and y is None
                continue
            assert x.dtype == y.dtype == torch.bool and x.device == y.device == torch.device("cpu")
            assert tuple(x.shape) == tuple(y.shape) == tuple(out) and torch.equal(x, y)


COCO_Q, COCO_K = 6, 5


def coco_case(device, sizes):
    """network outputs of len(sizes) images: every (query, class) pair is a candidate; a stub `masks_of` over blob logits"""
    B = len(sizes)
    g = torch.Generator().manual_seed(47)
    logits = torch.randn(B, COCO_Q, COCO_K, generator=g).to(device)
    cxcy = 0.3 + 0.4 * torch.rand(B, COCO_Q, 2, generator=g)
    boxes = torch.cat([cxcy, 0.1 + 0.3 * torch.rand(B, COCO_Q, 2, generator=g)], -1).to(device)
    bank = blob_logits(B * COCO_Q, H, W, seed=53).view(B, COCO_Q, H, W).to(device)
    return logits, boxes, (lambda image, queries: bank[image, queries]), bank


def run_coco(device, on, image_sizes, sizes_out):
    model = idol(device, coco=True)
    logits, boxes, masks_of, _ = coco_case(device, image_sizes)
    with Switched(model, on):
        return model.coco_postprocess(logits, boxes, masks_of, image_sizes, sizes_out)


def assert_same_coco(a, b, device, sizes_out):
    assert len(a) == len(b) == len(sizes_out)
    for ra, rb, out in zip(a, b, sizes_out):
        ia, ib = ra["instances"], rb["instances"]
        assert set(ia) == set(ib) and ia["image_size"] == ib["image_size"] == tuple(out)
        for k in ("pred_boxes", "scores", "pred_classes"):
            assert torch.equal(ia[k], ib[k])
        ma, mb = ia["pred_masks"], ib["pred_masks"]
        assert ma.dtype == mb.dtype == torch.uint8 and ma.device == mb.device == torch.device(device)
        assert tuple(ma.shape) == tuple(mb.shape) == (len(ia["scores"]),) + tuple(out) and len(ia["scores"]) > COCO_Q
        assert torch.equal(ma, mb)


COCO_IMAGES, COCO_OUTS = [(180, 320), (150, 290)], [(180, 320), (200, 300)]


# ---- CPU -----------------------------------------------------------------------------------------------------------
def test_enable_device_masks_sets_the_switch():
    for model in (seqformer("cpu"), idol("cpu")):
        assert model.device_masks is False
        T.enable_device_masks(model)
        assert model.device_masks is True
        T.enable_device_masks(model, on=False)
        assert model.device_masks is False
    with pytest.raises(ValueError, match="device_masks"):
        T.enable_device_masks(torch.nn.Linear(2, 2))


def test_cpu_sites_are_unchanged_by_the_switch():
    calls = dict(mask_dense.CALLS)
    out = (200, 300)
    assert_same_report(run_report("cpu", True, out), run_report("cpu", False, out), out)
    a, present = run_tracks("cpu", True, out)
    assert_same_tracks(a, run_tracks("cpu", False, out)[0], present, out)
    assert_same_coco(run_coco("cpu", True, COCO_IMAGES, COCO_OUTS), run_coco("cpu", False, COCO_IMAGES, COCO_OUTS), "cpu",
                     COCO_OUTS)
    assert mask_dense.CALLS == calls                           # CPU tensors: the host expression, no launch


# ---- GPU -----------------------------------------------------------------------------------------------------------
DEV = "cuda:0"
MIB = 1 << 20


def measured(fn):
    """fn() -> (its result, the op's launches, the peak of device memory over the call above what was allocated before)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base, calls = torch.cuda.memory_allocated(), mask_dense.CALLS["masks_from_logits"]
    result = fn()
    torch.cuda.synchronize()
    return result, mask_dense.CALLS["masks_from_logits"] - calls, torch.cuda.max_memory_allocated() - base


@pytest.mark.gpu
@pytest.mark.parametrize("out", [IMAGE, (200, 300)])
def test_report_site(out):
    _, _, logits = report_case("cpu")
    assert_band_empty(logits.flatten(0, 1), IMAGE, out)
    run_report(DEV, True, out)                                 # (first use: the library, the allocator's pools)
    on, calls, peak = measured(lambda: run_report(DEV, True, out))
    off, off_calls, off_peak = measured(lambda: run_report(DEV, False, out))
    assert calls == 1 and off_calls == 0
    assert_same_report(on, off, out)
    # the two pairs of query 0 are one piece of memory; without the switch each pair owns its masks
    assert on["pred_masks"][0].data_ptr() == on["pred_masks"][1].data_ptr()
    assert off["pred_masks"][0].data_ptr() != off["pred_masks"][1].data_ptr()
    if out == IMAGE:
        pixels = 3 * 2 * IMAGE[0] * IMAGE[1]                   # 3 distinct reported queries x 2 frames
        assert peak < 1.5 * pixels + MIB, (peak, pixels)
        assert off_peak >= 8 * pixels                          # (the instrument: the eager chain's two fp32 tensors)


@pytest.mark.gpu
@pytest.mark.parametrize("out", [IMAGE, (200, 300)])
def test_track_masks_site(out):
    assert_band_empty(blob_logits(7, H, W, seed=64), IMAGE, out)
    run_tracks(DEV, True, out)
    (on, present), calls, peak = measured(lambda: run_tracks(DEV, True, out))
    (off, _), off_calls, _ = measured(lambda: run_tracks(DEV, False, out))
    assert calls == 1 and off_calls == 0
    assert_same_tracks(on, off, present, out)
    if out == IMAGE:
        pixels = 7 * IMAGE[0] * IMAGE[1]
        # (the 7 logit maps the case itself uploads inside the call: pixels / 4 bytes, part of the 1.5)
        assert peak < 1.5 * pixels + MIB, (peak, pixels)
    assert IDOL._track_masks([], 4, IMAGE, out, device_masks=True) == []


@pytest.mark.gpu
def test_coco_postprocess_site():
    _, _, _, bank = coco_case("cpu", COCO_IMAGES)
    for b in range(2):
        assert_band_empty(bank[b], COCO_IMAGES[b], COCO_OUTS[b])
        assert_band_empty(bank[b], IMAGE, IMAGE)
    run_coco(DEV, True, COCO_IMAGES, COCO_OUTS)
    on, calls, _ = measured(lambda: run_coco(DEV, True, COCO_IMAGES, COCO_OUTS))
    off, off_calls, _ = measured(lambda: run_coco(DEV, False, COCO_IMAGES, COCO_OUTS))
    assert calls == 2 and off_calls == 0                       # one call per (image size, output size)
    assert_same_coco(on, off, DEV, COCO_OUTS)
    # two images of one size pair: one call; memory at out_size == image_size
    same = [IMAGE, IMAGE]
    run_coco(DEV, True, same, same)
    on, calls, peak = measured(lambda: run_coco(DEV, True, same, same))
    off, _, off_peak = measured(lambda: run_coco(DEV, False, same, same))
    assert calls == 1
    assert_same_coco(on, off, DEV, same)
    pixels = sum(len(r["instances"]["scores"]) for r in on) * IMAGE[0] * IMAGE[1]
    # the results themselves (boxes, scores, classes, pred_masks = `pixels` bytes) are alive at the end of the call
    assert peak < 1.5 * pixels + MIB, (peak, pixels)
    assert off_peak >= 8 * pixels // 2                         # (the instrument: the chain runs per image, half the pixels each)


# ---- one end-to-end run of each tiny model: structure and types -------------------------------------------------------------
@pytest.mark.gpu
def test_seqformer_end_to_end_with_the_switch():
    torch.manual_seed(6)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": DEV, "MODEL.SeqFormer.APPLY_CLS_THRES": 0.0, **SEQ_TINY})).eval()
    T.enable_device_masks(model)
    video = _video(3, 128, 192, 140, 200, DEV, seed=2)
    calls = mask_dense.CALLS["masks_from_logits"]
    res = model(video)
    assert mask_dense.CALLS["masks_from_logits"] == calls + 1
    assert tuple(res["image_size"]) == (140, 200)
    assert len(res["pred_scores"]) == len(res["pred_labels"]) == len(res["pred_masks"]) > 10
    for m in res["pred_masks"]:
        assert m.dtype == torch.bool and m.device.type == "cpu" and tuple(m.shape) == (3, 140, 200)
    assert any(bool(m.any()) for m in res["pred_masks"]) and not all(bool(m.all()) for m in res["pred_masks"])


@pytest.mark.gpu
def test_idol_end_to_end_with_the_switch():
    torch.manual_seed(7)
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": DEV, "MODEL.IDOL.BATCH_INFER_LEN": 2, **IDOL_TINY})).eval()
    T.enable_device_masks(model)
    video = _video(3, 128, 192, 140, 200, DEV, seed=3)
    calls = mask_dense.CALLS["masks_from_logits"]
    res = model(video)
    tracks = res["pred_masks"]
    assert len(res["pred_scores"]) == len(res["pred_labels"]) == len(tracks)
    assert mask_dense.CALLS["masks_from_logits"] == calls + (1 if tracks else 0)
    for per in tracks:
        assert len(per) == 3 and any(m is not None for m in per)
        for m in per:
            assert m is None or (m.dtype == torch.bool and m.device.type == "cpu" and tuple(m.shape) == (140, 200))
