"""COCO RLE strings encoded on the device (vnext_amd/csrc/mask_rle.hip, vnext_amd/ops/mask_rle.py) and the models'
`ytvis_results`: the strings of ytvis_json.rle_encode, the records of instances_to_coco_json_video."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vnext_amd.models  # noqa: F401
from conftest import GOLDEN_DIR
from vnext_amd import _lib
from vnext_amd.models import idol as idol_mod
from vnext_amd.models import seqformer as sf
from vnext_amd.models import tracker as trk
from vnext_amd.ops.mask_rle import encode_logits, encode_masks
from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg
from vnext_amd.utils.ytvis_json import instances_to_coco_json_video, rle_decode, rle_encode

IDOL_TINY = {"MODEL.IDOL.ENC_LAYERS": 1, "MODEL.IDOL.DEC_LAYERS": 2, "MODEL.IDOL.NUM_OBJECT_QUERIES": 110,
             "MODEL.IDOL.DIM_FEEDFORWARD": 64, "MODEL.IDOL.DROPOUT": 0.0}
SEQ_TINY = {"MODEL.SeqFormer.ENC_LAYERS": 1, "MODEL.SeqFormer.DEC_LAYERS": 2, "MODEL.SeqFormer.NUM_OBJECT_QUERIES": 12,
            "MODEL.SeqFormer.DIM_FEEDFORWARD": 64, "MODEL.SeqFormer.DROPOUT": 0.0}
BAND = 1e-5            # |bilinear value| below which the device bit may differ from sigmoid(value) > 0.5 on the host


def host_expression(logits, stride, image_size, out_size):
    """The models' mask step as it stands: bilinear x stride, sigmoid, crop, nearest, > 0.5 -> bool [M, oh, ow]."""
    h, w = logits.shape[-2:]
    m = F.interpolate(logits.float()[:, None], size=(h * stride, w * stride), mode="bilinear",
                      align_corners=False).sigmoid()
    return (F.interpolate(m[:, :, :image_size[0], :image_size[1]], size=tuple(out_size), mode="nearest") > 0.5)[:, 0]


def nearest_index(n_in, n_out):
    """ATen's nearest source index, fp32 scale in_size / out_size."""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def bilinear_f64(logits, stride, image_size, out_size):
    """Every output pixel's bilinear value in fp64 (indices and weights as ATen forms them) -> [M, oh, ow]."""
    M, h, w = logits.shape
    lg = logits.double().cpu().numpy()

    def axis(n, n_img, n_out):
        idx = nearest_index(n_img, n_out)
        scale = np.float32(n) / np.float32(n * stride)
        src = np.maximum(scale * (idx.astype(np.float32) + np.float32(0.5)) - np.float32(0.5), 0).astype(np.float64)
        i0 = src.astype(np.int64)
        i1 = np.where(i0 < n - 1, i0 + 1, i0)
        lam = src - i0
        return i0, i1, lam
    y0, y1, ly = axis(h, image_size[0], out_size[0])
    x0, x1, lx = axis(w, image_size[1], out_size[1])
    a, b = lg[:, y0][:, :, x0], lg[:, y0][:, :, x1]
    c, d = lg[:, y1][:, :, x0], lg[:, y1][:, :, x1]
    ly, lx = ly[None, :, None], lx[None, None, :]
    return (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * c + lx * d)


def blob_logits(M, h, w, seed):
    """Mask-like logit maps: a few Gaussian blobs minus an offset plus noise."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    out = torch.zeros(M, h, w)
    for m in range(M):
        for _ in range(3):
            cy, cx = float(torch.rand(1, generator=g)) * h, float(torch.rand(1, generator=g)) * w
            r = 2 + float(torch.rand(1, generator=g)) * max(h, w) / 4
            out[m] += 8 * torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
        out[m] += torch.randn(h, w, generator=g) - 2
    return out


# ---- CPU -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(1, 1), (1, 9), (7, 1), (37, 53), (64, 48)])
def test_cpu_encode_masks_is_rle_encode(hw):
    g = torch.Generator().manual_seed(hw[0] * 100 + hw[1])
    masks = torch.rand(3, *hw, generator=g) > 0.5
    masks[0] = False
    assert encode_masks(masks) == [rle_encode(m.numpy()) for m in masks]
    assert encode_masks(masks.to(torch.uint8)) == [rle_encode(m.numpy()) for m in masks]


@pytest.mark.parametrize("stride,hw,image,out", [(4, (6, 10), (24, 40), (30, 50)), (4, (6, 10), (21, 37), (21, 37)),
                                                 (8, (5, 7), (33, 50), (20, 31)), (4, (9, 16), (36, 64), (72, 128))])
def test_cpu_encode_logits_is_the_host_expression(stride, hw, image, out):
    logits = blob_logits(4, *hw, seed=stride + hw[0])
    want = [rle_encode(m.numpy()) for m in host_expression(logits, stride, image, out)]
    assert encode_logits(logits, stride, image, out) == want
    assert encode_logits(logits.double(), stride, image, out) == want       # other dtypes: cast to fp32


def test_abi_17_exports_the_encoder():
    assert _lib.ABI_VERSION == 17
    for name in ("vnx_mask_rle_measure", "vnx_mask_rle_write"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.product_lib(), name)
    assert _lib.product_lib().vnx_abi_version() == 17


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


def _video(frames, h, w, out_h, out_w, device="cpu", seed=0):
    g = torch.Generator().manual_seed(seed)
    return [{"video_id": 7, "image": [(torch.rand(3, h, w, generator=g) * 255).to(device) for _ in range(frames)],
             "height": out_h, "width": out_w, "length": frames}]


def _decoded_mismatch(got, want, score_rtol=0.0):
    """records of ytvis_results vs instances_to_coco_json_video: equal labels, scores within `score_rtol` (two forward
    passes of a model on the GPU agree to the last bits only: its kernels are not bitwise deterministic between calls)
    -> the worst fraction of differing mask pixels"""
    assert len(got) == len(want)
    worst = 0.0
    for a, b in zip(got, want):
        assert (a["video_id"], a["category_id"]) == (b["video_id"], b["category_id"])
        assert a["score"] == pytest.approx(b["score"], rel=score_rtol, abs=0)
        assert len(a["segmentations"]) == len(b["segmentations"])
        for sa, sb in zip(a["segmentations"], b["segmentations"]):
            assert sa["size"] == sb["size"]
            if sa["counts"] != sb["counts"]:
                worst = max(worst, float((rle_decode(sa) != rle_decode(sb)).mean()))
    return worst


def test_cpu_seqformer_ytvis_results_equal_the_host_writer(cpu_stand_ins):
    torch.manual_seed(4)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": "cpu", "MODEL.SeqFormer.APPLY_CLS_THRES": 0.0,
                                             **SEQ_TINY})).eval()
    video = _video(3, 64, 96, 70, 100)
    want = instances_to_coco_json_video(video, model(video))
    got = model.ytvis_results(video)
    assert got == want
    scores = [r["score"] for r in got]
    assert len(got) > len(set(id(r["segmentations"][0]) for r in got))     # queries reported under several classes
    assert len(scores) == len(got) > 10


def test_cpu_idol_ytvis_results_equal_the_host_writer(cpu_stand_ins):
    torch.manual_seed(3)
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": "cpu", "MODEL.IDOL.BATCH_INFER_LEN": 2, **IDOL_TINY})).eval()
    video = _video(3, 64, 96, 70, 100, seed=1)
    assert model.ytvis_results(video) == instances_to_coco_json_video(video, model(video))


def _golden_per_frame(g, v, device):
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": device, **IDOL_TINY})).eval()
    logits = torch.from_numpy(g[f"v{v}.pred_logits"]).to(device)
    boxes = torch.from_numpy(g[f"v{v}.pred_boxes"]).to(device)
    masks = torch.from_numpy(g[f"v{v}.pred_masks"]).to(device)
    embeds = torch.from_numpy(g[f"v{v}.pred_inst_embed"]).to(device)
    per_frame = []
    for f, c in enumerate(model.select_candidates(logits, boxes)):
        q = torch.from_numpy(c).to(device)
        per_frame.append({"indices": c.tolist(), "logits": logits[f, q], "boxes": boxes[f, q], "embeds": embeds[f, q],
                          "masks": masks[f, q]})
    args = dict(init_score_thr=0.2, obj_score_thr=0.1, nms_thr_pre=0.5, nms_thr_post=0.05, addnew_score_thr=0.2,
                memo_tracklet_frames=10, memo_momentum=0.8, long_match=True, frame_weight=True, temporal_weight=True,
                memory_len=3)
    return model, per_frame, args


@pytest.mark.parametrize("v", [0, 1])
def test_cpu_idol_rle_finishing_step_on_the_golden_video(v, cpu_stand_ins):
    """The reference fixture through `associate(rle=True)`: the records the host writer makes of the bool masks,
    absent frames (the empty mask's RLE) included."""
    g = dict(np.load(os.path.join(GOLDEN_DIR, "inference_idol.npz")))
    model, per_frame, args = _golden_per_frame(g, v, "cpu")
    oh, ow, ih, iw = (int(x) for x in g[f"v{v}.sizes"])
    res = model.associate(per_frame, trk.IDOL_Tracker(**args), (oh, ow), (ih, iw))
    rle = model.associate(per_frame, trk.IDOL_Tracker(**args), (oh, ow), (ih, iw), rle=True)
    assert not g[f"v{v}.present"].all()                # some track is absent from some frame
    inputs = [{"video_id": 1, "height": oh, "width": ow}]
    from vnext_amd.utils.ytvis_json import ytvis_records
    assert ytvis_records(inputs, rle) == instances_to_coco_json_video(inputs, res)


# ---- GPU -----------------------------------------------------------------------------------------------------------
DEV = "cuda:0"


def _dev_masks(masks):
    return encode_masks(torch.as_tensor(np.asarray(masks, dtype=np.uint8)).to(DEV))


@pytest.mark.gpu
def test_binary_mode_reproduces_the_pycocotools_strings():
    with open(os.path.join(GOLDEN_DIR, "rle_coco.json")) as f:
        cases = json.load(f)
    for c in cases:
        m = rle_decode(c)
        assert _dev_masks(m[None]) == [{"size": list(c["size"]), "counts": c["counts"]}], c.get("source")


def _edge_masks():
    rng = np.random.default_rng(5)
    one0 = np.zeros((9, 11), bool)
    one0[0, 0] = True
    yield "zeros", np.zeros((1, 9, 11), bool)
    yield "ones", np.ones((1, 9, 11), bool)
    yield "pixel0", one0[None]
    yield "1x1", np.array([[[True]], [[False]]])
    yield "1xW", rng.random((3, 1, 301)) > 0.5
    yield "Hx1", rng.random((3, 257, 1)) > 0.5
    yield "checker", (np.indices((173, 211)).sum(0) % 2 == 1)[None]
    yield "random37x53", rng.random((131, 37, 53)) > 0.5         # M not a multiple of any block size
    yield "random720p", rng.random((2, 720, 1280)) > 0.7


@pytest.mark.gpu
def test_binary_mode_edge_cases():
    for name, masks in _edge_masks():
        assert _dev_masks(masks) == [rle_encode(m) for m in masks], name
    assert _dev_masks(np.zeros((0, 5, 5), bool)) == []
    last = torch.zeros(1, 4000, 4000, dtype=torch.bool, device=DEV)
    last[0, -1, -1] = True                                   # one count of 16e6 - 1: a 5-character group
    got = encode_masks(last)
    assert got == [{"size": [4000, 4000], "counts": rle_encode(last[0].cpu().numpy())["counts"]}]
    assert len(got[0]["counts"]) == 6


def _check_logits(logits, stride, image, out):
    got = encode_logits(logits.to(DEV), stride, image, out)
    host = host_expression(logits.to(DEV), stride, image, out).cpu().numpy()
    v = bilinear_f64(logits, stride, image, out)
    band = np.abs(v) < BAND
    for i, (g, m) in enumerate(zip(got, host)):
        assert g["size"] == list(out)
        if not band[i].any():
            assert g["counts"] == rle_encode(m)["counts"], (i, stride, image, out)
        else:
            diff = rle_decode(g) != m
            assert not (diff & ~band[i]).any(), (i, stride, image, out)
    return band


@pytest.mark.gpu
@pytest.mark.parametrize("stride,hw", [(4, (23, 41)), (4, (90, 160)), (4, (180, 320)), (8, (23, 41)), (8, (45, 80))])
def test_logits_mode_matches_the_host_path(stride, hw):
    h, w = hw
    H, W = h * stride, w * stride
    logits = blob_logits(5, h, w, seed=h + stride)
    for image in [(H, W), (H - 3, W - 5), (H * 2 // 3, W * 3 // 4)]:
        for out in [image, (image[0] * 2, image[1] * 2), (image[0] * 3 // 2, image[1] * 3 // 2),
                    (max(1, image[0] // 3), max(1, image[1] // 2)), (image[0] + 7, image[1] - 11)]:
            _check_logits(logits, stride, image, out)


@pytest.mark.gpu
def test_logits_mode_at_the_product_resolutions():
    """360 -> 720 and 480 -> 720 upsampling of the model's output size, and a band case built on purpose."""
    logits = blob_logits(4, 90, 160, seed=11)
    _check_logits(logits, 4, (360, 640), (720, 1280))
    _check_logits(blob_logits(3, 120, 160, seed=12), 4, (480, 640), (720, 960))
    flat = torch.zeros(2, 10, 12)
    flat[1, 3:6, 4:9] = 1.0
    band = _check_logits(flat, 4, (40, 48), (40, 48))       # exact zeros: every zero pixel in the band
    assert band.any()


@pytest.mark.gpu
@pytest.mark.parametrize("n_in,n_out", [(40, 40), (40, 80), (40, 60), (48, 72), (37, 101), (97, 31), (720, 1280)])
def test_nearest_index_maps_equal_torch(n_in, n_out):
    ramp = torch.arange(n_in, dtype=torch.float32)[None, None, :, None]
    want = F.interpolate(ramp, size=(n_out, 1), mode="nearest")[0, 0, :, 0].long().numpy()
    assert (nearest_index(n_in, n_out) == want).all()
    # the kernel's own index map: stride 1 (bilinear = the map itself), a +-1 map, any wrong row / column flips a bit
    g = torch.Generator().manual_seed(n_in + n_out)
    sign = torch.where(torch.rand(3, n_in, 17, generator=g) > 0.5, 1.0, -1.0)
    got = encode_logits(sign.to(DEV), 1, (n_in, 17), (n_out, 23))
    want = F.interpolate(sign[:, None], size=(n_out, 23), mode="nearest")[:, 0] > 0
    assert got == [rle_encode(m.numpy()) for m in want]
    signt = sign.transpose(1, 2).contiguous()
    got = encode_logits(signt.to(DEV), 1, (17, n_in), (23, n_out))
    want = F.interpolate(signt[:, None], size=(23, n_out), mode="nearest")[:, 0] > 0
    assert got == [rle_encode(m.numpy()) for m in want]


def _raw(mode, data, M, h, w, s, ih, iw, oh, ow, guard=64, short=0):
    lib = _lib.lib()
    stream = _lib.current_stream(data)
    lengths = torch.empty(M, dtype=torch.int64, device=DEV)
    _lib.check(lib.vnx_mask_rle_measure(mode, data.data_ptr(), M, h, w, s, ih, iw, oh, ow, lengths.data_ptr(), stream))
    ends = lengths.cumsum(0)
    total = int(ends[-1])
    arena = torch.full((total + guard,), 0xAB, dtype=torch.uint8, device=DEV)
    _lib.check(lib.vnx_mask_rle_write(mode, data.data_ptr(), M, h, w, s, ih, iw, oh, ow, (ends - lengths).data_ptr(),
                                      arena.data_ptr(), total - short, stream))
    return lengths.cpu(), arena.cpu(), total


@pytest.mark.gpu
def test_deterministic_and_within_the_arena():
    logits = blob_logits(37, 45, 80, seed=3).to(DEV)
    a = _raw(_lib.MASK_RLE_LOGITS, logits, 37, 45, 80, 4, 180, 320, 360, 640)
    b = _raw(_lib.MASK_RLE_LOGITS, logits, 37, 45, 80, 4, 180, 320, 360, 640)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    total = a[2]
    assert (a[1][total:] == 0xAB).all()
    # an arena declared 5 bytes short: the strings stop there, nothing past it is written
    c = _raw(_lib.MASK_RLE_LOGITS, logits, 37, 45, 80, 4, 180, 320, 360, 640, short=5)
    assert torch.equal(c[1][:total - 5], a[1][:total - 5]) and (c[1][total - 5:] == 0xAB).all()
    masks = (torch.rand(19, 77, 131, device=DEV) > 0.5).to(torch.uint8)
    d = _raw(_lib.MASK_RLE_BINARY, masks, 19, 0, 0, 0, 0, 0, 77, 131)
    assert (d[1][d[2]:] == 0xAB).all()


@pytest.mark.gpu
def test_bad_sizes_are_refused_before_a_launch():
    lib = _lib.lib()
    x = torch.zeros(2, 8, 8, device=DEV)
    out = torch.empty(2, dtype=torch.int64, device=DEV)
    st = _lib.current_stream(x)

    def refused(*args, status=1):
        assert lib.vnx_mask_rle_measure(*args, out.data_ptr(), st) == status, args
        assert b"vnx_mask_rle_measure" in lib.vnx_last_error()
    L, B = _lib.MASK_RLE_LOGITS, _lib.MASK_RLE_BINARY
    refused(L, x.data_ptr(), -1, 8, 8, 4, 32, 32, 32, 32)                 # M < 0
    refused(L, None, 2, 8, 8, 4, 32, 32, 32, 32)                           # null input
    refused(L, x.data_ptr(), 2, 0, 8, 4, 32, 32, 32, 32)                   # non-positive sizes
    refused(L, x.data_ptr(), 2, 8, 8, 0, 32, 32, 32, 32)
    refused(L, x.data_ptr(), 2, 8, 8, 4, 32, 32, 0, 32)
    refused(L, x.data_ptr(), 2, 8, 8, 4, 33, 32, 32, 32)                   # crop larger than the upsampled map
    refused(L, x.data_ptr(), 2, 8, 8, 4, 32, 33, 32, 32)
    refused(L, x.data_ptr() + 2, 2, 8, 8, 4, 32, 32, 32, 32)               # misaligned logits
    refused(7, x.data_ptr(), 2, 8, 8, 4, 32, 32, 32, 32)                   # unknown mode
    refused(L, x.data_ptr(), 2, 8, 8, 4, 32, 32, 46341, 46341, status=2)   # oh * ow >= 2^31
    refused(B, x.data_ptr(), 2, 0, 0, 0, 0, 0, 65536, 32768, status=2)
    assert lib.vnx_mask_rle_measure(L, None, 0, 8, 8, 4, 32, 32, 32, 32, None, st) == 0      # M == 0: a no-op
    assert lib.vnx_mask_rle_write(L, x.data_ptr(), 2, 8, 8, 4, 32, 32, 32, 32, out.data_ptr(), out.data_ptr(), -1,
                                  st) == 1
    with pytest.raises(_lib.VnextHipError, match="crop|bad sizes"):
        encode_logits(x, 4, (40, 32), (32, 32))


def _idol_golden_rle(v, tracker_cls):
    g = dict(np.load(os.path.join(GOLDEN_DIR, "inference_idol.npz")))
    model, per_frame, args = _golden_per_frame(g, v, DEV)
    oh, ow, ih, iw = (int(x) for x in g[f"v{v}.sizes"])
    res = model.associate(per_frame, tracker_cls(**args), (oh, ow), (ih, iw))
    rle = model.associate(per_frame, tracker_cls(**args), (oh, ow), (ih, iw), rle=True)
    np.testing.assert_array_equal(np.array(rle["pred_labels"]), g[f"v{v}.labels"])
    np.testing.assert_allclose(np.array(rle["pred_scores"]), g[f"v{v}.scores"], rtol=1e-5)
    assert rle["pred_labels"] == res["pred_labels"] and rle["pred_scores"] == res["pred_scores"]
    present = g[f"v{v}.present"]
    want = np.unpackbits(g[f"v{v}.masks"], axis=-1)[..., :ow].astype(bool)
    empty = rle_encode(np.zeros((oh, ow), np.uint8))
    for i, (track, host) in enumerate(zip(rle["pred_masks"], res["pred_masks"])):
        for t, (r, m) in enumerate(zip(track, host)):
            if not present[i, t]:
                assert m is None and r == empty
                continue
            d = rle_decode(r)
            assert float((d != want[i, t]).mean()) < 2e-3, (i, t)
            assert float((d != m.numpy()).mean()) <= 1e-5, (i, t)


@pytest.mark.gpu
@pytest.mark.parametrize("v", [0, 1])
def test_idol_golden_through_the_rle_step_host_tracker(v):
    _idol_golden_rle(v, trk.IDOL_Tracker)


@pytest.mark.gpu
@pytest.mark.parametrize("v", [0, 1])
def test_idol_golden_through_the_rle_step_device_tracker(v):
    _idol_golden_rle(v, trk.DeviceTracker)


@pytest.mark.gpu
@pytest.mark.parametrize("clip_matching", [False, True])
def test_seqformer_ytvis_results_on_gpu(clip_matching):
    torch.manual_seed(6)
    cfg = {"MODEL.DEVICE": DEV, "MODEL.SeqFormer.APPLY_CLS_THRES": 0.0, "MODEL.SeqFormer.CLIP_MATCHING": clip_matching,
           "MODEL.SeqFormer.CLIP_LENGTH": 3, **SEQ_TINY}
    model = build_model(get_seqformer_cfg(**cfg)).eval()
    video = _video(5, 360, 640, 360, 640, DEV, seed=2)
    model(video)                                           # warm-up: the trunk's graph is captured
    got, want = model.ytvis_results(video), instances_to_coco_json_video(video, model(video))
    assert len(got) > 10
    assert _decoded_mismatch(got, want, score_rtol=1e-5) <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(360, 640, 360, 640), (360, 640, 720, 1280)])
def test_idol_ytvis_results_on_gpu(size):
    torch.manual_seed(7)
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": DEV, "MODEL.IDOL.BATCH_INFER_LEN": 2, **IDOL_TINY})).eval()
    video = _video(4, *size, DEV, seed=3)
    model(video)
    got, want = model.ytvis_results(video), instances_to_coco_json_video(video, model(video))
    assert _decoded_mismatch(got, want, score_rtol=1e-5) <= 1e-5
