"""IDOL's COCO pre-training evaluation branch (INPUT.COCO_PRETRAIN): `coco_postprocess` / `coco_results` on recorded
network outputs against the reference's `coco_inference` + `segmentation_postprocess`
(tools/make_golden_coco_inference.py -> tests/golden/coco_inference_idol.npz), and the model-level surface
(`forward` in eval mode, `coco_inference`, `train.enable_device_selection`)."""
import os

import numpy as np
import pytest
import torch

import vnext_amd.models  # noqa: F401
from conftest import GOLDEN_DIR
from vnext_amd import train as T
from vnext_amd.models import idol as idol_mod
from vnext_amd.registry import build_model, get_idol_cfg
from vnext_amd.utils.ytvis_json import rle_decode

TINY = {"MODEL.IDOL.ENC_LAYERS": 1, "MODEL.IDOL.DEC_LAYERS": 2, "MODEL.IDOL.NUM_OBJECT_QUERIES": 110,
        "MODEL.IDOL.DIM_FEEDFORWARD": 64, "MODEL.IDOL.DROPOUT": 0.0}
FIELDS = {"image_size", "pred_boxes", "scores", "pred_classes", "pred_masks"}


@pytest.fixture
def cpu_stand_ins(monkeypatch):
    """PyTorch restatements (oracle/, tests only) for the HIP entry points so the model runs on CPU."""
    from oracle.heads_torch_fallback import dynamic_mask_head_torch
    from oracle.msda_torch_fallback import msda_grid_sample
    from vnext_amd.ops.modules import ms_deform_attn as mod

    class Fn:
        @staticmethod
        def apply(value, shapes, lsi, loc, attn, step):
            return msda_grid_sample(value, shapes, loc, attn)
    monkeypatch.setattr(mod, "MSDeformAttnFunction", Fn)
    monkeypatch.setattr(idol_mod, "dynamic_mask_head", dynamic_mask_head_torch)


def _model(device, coco=True, **extra):
    torch.manual_seed(4)
    return build_model(get_idol_cfg(**{"MODEL.DEVICE": device, "INPUT.COCO_PRETRAIN": coco, **TINY, **extra})).eval()


_CACHE = {}


def _cached_model(device):
    """one tiny model per device for the tests that only use its post-processing"""
    if device not in _CACHE:
        _CACHE[device] = _model(device)
    return _CACHE[device]


def _fixture(device):
    g = dict(np.load(os.path.join(GOLDEN_DIR, "coco_inference_idol.npz")))
    step, shift = (float(x) for x in g["mask_scale"])
    masks = (torch.from_numpy(g["mask_q8"]).float() * step + shift).to(device)
    logits, boxes = torch.from_numpy(g["pred_logits"]).to(device), torch.from_numpy(g["pred_boxes"]).to(device)
    image_sizes = [tuple(int(v) for v in r) for r in g["image_sizes"]]
    out_sizes = [tuple(int(v) for v in r) for r in g["out_sizes"]]
    return g, logits, boxes, (lambda image, queries: masks[image, queries]), image_sizes, out_sizes


def _check_against_the_reference(device):
    model = _cached_model(device)
    g, logits, boxes, masks_of, image_sizes, out_sizes = _fixture(device)
    results = model.coco_postprocess(logits, boxes, masks_of, image_sizes, out_sizes)
    assert len(results) == len(image_sizes)
    inputs = [{"image_id": 10 + b, "height": oh, "width": ow} for b, (oh, ow) in enumerate(out_sizes)]
    model._coco_trunk = lambda batched_inputs: (logits, boxes, masks_of, image_sizes, out_sizes)     # the recorded outputs
    try:
        records = model.coco_results(inputs)
    finally:
        del model._coco_trunk
    at = 0
    for b, (res, (oh, ow)) in enumerate(zip(results, out_sizes)):
        inst = res["instances"]
        assert set(inst) == FIELDS and inst["image_size"] == (oh, ow)
        want = np.unpackbits(g[f"i{b}.masks"], axis=-1)[..., :ow].astype(bool)
        n = len(g[f"i{b}.scores"])
        assert n < 100, "the fixture drops rows with an empty box"
        np.testing.assert_array_equal(inst["pred_classes"].cpu().numpy(), g[f"i{b}.classes"])
        np.testing.assert_allclose(inst["scores"].cpu().numpy(), g[f"i{b}.scores"], rtol=1e-5)
        np.testing.assert_allclose(inst["pred_boxes"].cpu().numpy(), g[f"i{b}.boxes"], rtol=1e-5, atol=1e-5)
        masks = inst["pred_masks"]
        assert masks.dtype == torch.uint8 and tuple(masks.shape) == (n, oh, ow)
        assert float((masks.cpu().numpy().astype(bool) != want).mean()) < 2e-3
        for i in range(n):
            rec = records[at + i]
            assert rec["image_id"] == 10 + b and rec["category_id"] == int(g[f"i{b}.classes"][i])
            np.testing.assert_allclose(rec["score"], g[f"i{b}.scores"][i], rtol=1e-5)
            x0, y0, x1, y1 = g[f"i{b}.boxes"][i]
            np.testing.assert_allclose(rec["bbox"], [x0, y0, x1 - x0, y1 - y0], rtol=1e-5, atol=1e-4)
            assert rec["segmentation"]["size"] == [oh, ow]
        decoded = np.stack([rle_decode(records[at + i]["segmentation"]).astype(bool) for i in range(n)])
        assert float((decoded != want).mean()) < 2e-3
        at += n
    assert at == len(records)


def test_coco_postprocess_equals_the_reference_on_cpu():
    _check_against_the_reference("cpu")


@pytest.mark.gpu
def test_coco_postprocess_equals_the_reference_on_gpu():
    """selection by the kernel, masks through the device chain, RLE strings by the device encoder"""
    _check_against_the_reference("cuda:0")


def test_without_masks_there_is_no_pred_masks():
    model = _cached_model("cpu")
    _, logits, boxes, _, image_sizes, out_sizes = _fixture("cpu")
    results = model.coco_postprocess(logits, boxes, None, image_sizes, out_sizes)
    assert all(set(r["instances"]) == FIELDS - {"pred_masks"} for r in results)


def _images(device, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [{"image": (torch.rand(3, 64, 96, generator=g) * 255).to(device), "height": 70, "width": 100},
            {"image": (torch.rand(3, 48, 80, generator=g) * 255).to(device)}]


def _check_format(results, sizes):
    assert len(results) == len(sizes)
    for res, (h, w) in zip(results, sizes):
        inst = res["instances"]
        assert set(inst) == FIELDS and inst["image_size"] == (h, w)
        n = len(inst["scores"])
        assert 0 < n <= 100 and tuple(inst["pred_boxes"].shape) == (n, 4) and len(inst["pred_classes"]) == n
        assert inst["pred_masks"].dtype == torch.uint8 and tuple(inst["pred_masks"].shape) == (n, h, w)
        assert bool((inst["scores"][:-1] >= inst["scores"][1:]).all())


def test_tiny_model_in_eval_mode_returns_instances_with_coco_pretrain(cpu_stand_ins):
    model = _model("cpu")
    assert model.coco_pretrain and model.mask_on
    _check_format(model(_images("cpu")), [(70, 100), (48, 80)])
    model.mask_on = False
    assert all("pred_masks" not in r["instances"] for r in model(_images("cpu")))


def test_tiny_model_without_coco_pretrain_still_returns_the_video_dictionary(cpu_stand_ins):
    from vnext_amd.models import tracker as trk
    model = _model("cpu", coco=False, **{"MODEL.IDOL.BATCH_INFER_LEN": 2})
    assert not model.coco_pretrain
    g = torch.Generator().manual_seed(0)
    video = [{"image": [torch.rand(3, 64, 96, generator=g) * 255 for _ in range(2)], "height": 70, "width": 100}]
    import unittest.mock as mock
    with mock.patch.object(trk, "_pairwise_dot", lambda a, b: a @ b.t()), \
            mock.patch.object(trk, "_match_scores", lambda e, m, metric: ((e @ m.t()).softmax(1) + (e @ m.t()).softmax(0)) / 2
                              if metric == "bisoftmax" else (e @ m.t()).softmax(1)):
        res = model(video)
    assert set(res) == {"image_size", "pred_scores", "pred_labels", "pred_masks"}


def test_enable_device_selection_sets_and_clears_the_flag():
    model = _cached_model("cpu")
    assert model.device_selection is False
    T.enable_device_selection(model)
    assert model.device_selection is True
    T.enable_device_selection(model, on=False)
    assert model.device_selection is False
    with pytest.raises(ValueError, match="device_selection"):
        T.enable_device_selection(torch.nn.Linear(2, 2))


@pytest.mark.gpu
def test_tiny_model_on_gpu_equals_the_host_expression_on_the_same_trunk_outputs():
    model = _model("cuda:0")
    inputs = _images("cuda:0")
    results = model(inputs)
    _check_format(results, [(70, 100), (48, 80)])
    logits, boxes, masks_of, image_sizes, out_sizes = model._coco_trunk(inputs)
    assert image_sizes == [(64, 96), (48, 80)] and out_sizes == [(70, 100), (48, 80)]

    def masks_on_host(image, queries):
        return masks_of(image.cuda(), queries.cuda()).cpu()
    host = model.coco_postprocess(logits.cpu(), boxes.cpu(), masks_on_host, image_sizes, out_sizes)
    for got, want in zip(results, host):
        got, want = got["instances"], want["instances"]
        np.testing.assert_array_equal(got["pred_classes"].cpu().numpy(), want["pred_classes"].numpy())
        np.testing.assert_allclose(got["scores"].cpu().numpy(), want["scores"].numpy(), rtol=1e-5)
        np.testing.assert_allclose(got["pred_boxes"].cpu().numpy(), want["pred_boxes"].numpy(), rtol=1e-5, atol=1e-4)
        assert float((got["pred_masks"].cpu() != want["pred_masks"]).float().mean()) < 2e-3
    records = model.coco_results(inputs)
    assert len(records) == sum(len(r["instances"]["scores"]) for r in results)
    assert set(records[0]) == {"image_id", "category_id", "bbox", "score", "segmentation"}


@pytest.mark.gpu
def test_more_queries_than_the_kernel_holds_are_selected_on_the_host():
    """Q = 1500 is beyond the kernel's 1280: `coco_postprocess` on CUDA tensors takes the host expression, not an error"""
    from vnext_amd.ops import det_select as DS
    model = _cached_model("cpu")
    g = torch.Generator().manual_seed(4)
    logits = -4.0 + torch.randn(1, 1500, 2, generator=g)
    boxes = torch.cat([0.2 + 0.6 * torch.rand(1, 1500, 2, generator=g), 0.05 + 0.2 * torch.rand(1, 1500, 2, generator=g)], -1)
    with pytest.raises(DS.DetSelectUnsupported):
        DS.select_detections(logits.cuda(), boxes.cuda(), iou_thr=0.7, topk=100)
    got = model.coco_postprocess(logits.cuda(), boxes.cuda(), None, [(48, 80)], [(60, 90)])[0]["instances"]
    want = model.coco_postprocess(logits, boxes, None, [(48, 80)], [(60, 90)])[0]["instances"]
    assert len(want["scores"]) == 100
    np.testing.assert_array_equal(got["pred_classes"].cpu().numpy(), want["pred_classes"].numpy())
    np.testing.assert_allclose(got["scores"].cpu().numpy(), want["scores"].numpy(), rtol=1e-5)
    np.testing.assert_allclose(got["pred_boxes"].cpu().numpy(), want["pred_boxes"].numpy(), rtol=1e-5, atol=1e-4)
