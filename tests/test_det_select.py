"""Detection selection on the device (vnext_amd/csrc/det_select.hip, vnext_amd/ops/det_select.py): best class, score
threshold, class-aware greedy NMS and top-k of a batch of images against the host expression (`class_aware_nms` +
`torch.topk`) on the same fp32 inputs, through the C ABI with guard words behind every image's slice.

The randomised comparisons are exact on indices.  An image is LEFT OUT of them when a float64 recomputation shows that
an fp32 rounding decides a comparison of the host expression itself: a same-class IoU within 1e-6 of the threshold, a
best score within 1e-6 of the score threshold, or host fp32 sigmoid scores that are not strictly decreasing in logit
order (the kernel orders by the logit; among the `topk + 1` largest class scores in COCO mode).  At most 5 % of a test's
images may be left out; every test prints its count."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import vnext_amd.models  # noqa: F401
from conftest import GOLDEN_DIR
from vnext_amd import _lib
from vnext_amd.models import idol as idol_mod
from vnext_amd.models import tracker as trk
from vnext_amd.ops import det_select as DS
from vnext_amd.registry import build_model, get_idol_cfg

SHAPES = [(1, 1), (37, 3), (64, 1), (65, 3), (129, 2), (300, 80)]      # 64 / 65 / 129 cross the bit-matrix words
BATCH = 8
GUARD, SENTINEL = 8, 0x5A5A5A5A
TINY = {"MODEL.IDOL.ENC_LAYERS": 1, "MODEL.IDOL.DEC_LAYERS": 2, "MODEL.IDOL.NUM_OBJECT_QUERIES": 110,
        "MODEL.IDOL.DIM_FEEDFORWARD": 64, "MODEL.IDOL.DROPOUT": 0.0}


# ---- inputs, the host expression's own margins ------------------------------------------------------------------------
def make_inputs(seed, B, Q, K, iou_thr):
    """logits -4 + 0.5 N(0,1), centres U(0.2, 0.8), sizes U(0.05, 0.25); per image min(12, Q // 6) planted objects with a
    random class and 1-5 near-duplicate boxes (base + 0.012 d N(0,1) for the 0.7 threshold, base + 0.004 d for 0.9) whose
    logit on that class is 1.5 - 0.6 d + 0.5 N(0,1)"""
    g = torch.Generator().manual_seed(seed)
    logits = -4.0 + 0.5 * torch.randn(B, Q, K, generator=g)
    boxes = torch.cat([0.2 + 0.6 * torch.rand(B, Q, 2, generator=g), 0.05 + 0.2 * torch.rand(B, Q, 2, generator=g)], -1)
    for b in range(B):
        slots = torch.randperm(Q, generator=g).tolist()
        for _ in range(min(12, Q // 6)):
            cls = int(torch.randint(0, K, (1,), generator=g))
            base = torch.cat([0.2 + 0.6 * torch.rand(2, generator=g), 0.05 + 0.2 * torch.rand(2, generator=g)])
            for d in range(int(torch.randint(1, 6, (1,), generator=g))):
                q = slots.pop()
                boxes[b, q] = base + (0.012 * d * torch.randn(4, generator=g) if iou_thr < 0.8 else 0.004 * d)
                logits[b, q, cls] = 1.5 - 0.6 * d + 0.5 * torch.randn(1, generator=g).item()
    return logits, boxes


def fragile(logits, boxes, iou_thr, score_thr, topk):
    """True when an fp32 rounding decides a comparison of the host expression on this image (float64 recomputation)"""
    lo, bx = logits.double().numpy(), boxes.double().numpy()
    best32 = logits.sigmoid().max(-1)[0].numpy()
    label = lo.argmax(-1)
    best64 = 1.0 / (1.0 + np.exp(-lo.max(-1)))
    cand = np.ones(len(label), dtype=bool)
    if score_thr is not None:
        if np.any(np.abs(best64 - score_thr) < 1e-6):
            return True
        cand = best64 > score_thr
        if not cand.any():      # the single best query: the host takes the first maximum of the fp32 scores
            top = np.sort(best32)[::-1]
            return len(top) > 1 and top[0] == top[1] and np.sort(lo.max(-1))[-1] != np.sort(lo.max(-1))[-2]
    xy = np.concatenate([bx[:, :2] - 0.5 * bx[:, 2:], bx[:, :2] + 0.5 * bx[:, 2:]], -1)[cand]
    area = (xy[:, 2] - xy[:, 0]) * (xy[:, 3] - xy[:, 1])
    wh = np.clip(np.minimum(xy[:, None, 2:], xy[None, :, 2:]) - np.maximum(xy[:, None, :2], xy[None, :, :2]), 0, None)
    inter = wh[..., 0] * wh[..., 1]
    iou = inter / (area[:, None] + area[None, :] - inter)
    same = (label[cand][:, None] == label[cand][None, :]) & ~np.eye(int(cand.sum()), dtype=bool)
    if np.any(same & (np.abs(iou - iou_thr) < 1e-6)):
        return True
    order = np.lexsort((np.arange(len(label))[cand], -lo.max(-1)[cand]))
    if np.any(np.diff(best32[cand][order]) >= 0):
        return True
    if topk is not None:
        kept = DS.select_detections_host(logits[None], boxes[None], iou_thr=iou_thr, score_thr=score_thr).kept[0]
        flat = logits[torch.from_numpy(kept)].reshape(-1)
        top = torch.sort(flat, descending=True, stable=True)[0][:topk + 1].sigmoid().numpy()
        if np.any(np.diff(top) >= 0):
            return True
    return False


# ---- the C ABI with guard words -----------------------------------------------------------------------------------------
def run_abi(logits, boxes, score_thr, iou_thr, topk, expect=_lib.VNX_OK):
    """-> int32 [B, words] on the host; the GUARD words behind every image's slice must come back untouched"""
    lib = _lib.lib()
    B, Q, K = logits.shape
    words = lib.vnx_det_select_out_words(Q, topk)
    assert words == 4 + 2 * Q + 2 * topk
    stride = words + GUARD
    lo, bx = logits.cuda().contiguous(), boxes.cuda().contiguous()
    out = torch.full((B, stride), SENTINEL, dtype=torch.int32, device="cuda")
    status = lib.vnx_det_select(lo.data_ptr(), bx.data_ptr(), B, Q, K, ctypes.c_float(-1.0 if score_thr is None else score_thr),
                                ctypes.c_float(iou_thr), topk, out.data_ptr(), stride, _lib.current_stream(lo))
    torch.cuda.synchronize()
    assert status == expect, lib.vnx_last_error().decode()
    a = out.cpu().numpy()
    assert (a[:, words:] == SENTINEL).all(), "words of the stride beyond an image's result were written"
    if expect != _lib.VNX_OK:
        assert (a == SENTINEL).all(), "a refused call wrote to the output"
    return a[:, :words]


def unpack(a, Q, topk):
    kept = [row[4:4 + row[1]].astype(np.int64) for row in a]
    for row, k in zip(a, kept):
        assert row[3] == 0 and (row[4 + len(k):4 + Q] == -1).all()
        assert (row[4 + 2 * Q + 2 * row[2]:] == -1).all()
    labels = [row[4 + Q:4 + 2 * Q].astype(np.int64) for row in a]
    pairs = [row[4 + 2 * Q:4 + 2 * Q + 2 * row[2]].astype(np.int64).reshape(-1, 2) for row in a]
    return kept, labels, pairs


def _compare(mode):
    iou_thr, score_thr, topk = (0.7, None, 100) if mode == "coco" else (0.9, 0.1, None)
    left_out = total = suppressed = 0
    for s, (Q, K) in enumerate(SHAPES):
        logits, boxes = make_inputs(100 + s, BATCH, Q, K, iou_thr)
        want = DS.select_detections_host(logits, boxes, iou_thr=iou_thr, score_thr=score_thr, topk=topk)
        a = run_abi(logits, boxes, score_thr, iou_thr, topk or 0)
        assert (a[:, 0] == 0).all()
        kept, labels, pairs = unpack(a, Q, topk or 0)
        dev_logits, prob = logits.cuda(), logits.sigmoid()
        for b in range(BATCH):
            total += 1
            if fragile(logits[b], boxes[b], iou_thr, score_thr, topk):
                left_out += 1
                continue
            np.testing.assert_array_equal(kept[b], want.kept[b], err_msg=f"kept, Q={Q} K={K} image {b}")
            np.testing.assert_array_equal(labels[b], want.labels[b], err_msg=f"labels, Q={Q} K={K} image {b}")
            n_cand = Q if score_thr is None else int((prob[b].max(-1)[0] > score_thr).sum())
            suppressed += max(n_cand, 1) - len(kept[b])                     # what the NMS removed
            if topk:
                assert a[b, 2] == min(topk, len(kept[b]) * K)           # the count rule
                np.testing.assert_array_equal(pairs[b], want.topk[b], err_msg=f"top-k, Q={Q} K={K} image {b}")
                q, c = torch.from_numpy(pairs[b][:, 0]).cuda(), torch.from_numpy(pairs[b][:, 1]).cuda()
                # the scores a caller forms from the kernel's pairs against the eager ones at the host expression's pairs:
                # exactly on the device, and to the fixture tests' score tolerance against the host's fp32 sigmoid
                wq, wc = torch.from_numpy(want.topk[b][:, 0]), torch.from_numpy(want.topk[b][:, 1])
                scores = dev_logits[b, q, c].sigmoid()
                assert torch.equal(scores, dev_logits[b].sigmoid()[wq.cuda(), wc.cuda()])
                np.testing.assert_allclose(scores.cpu().numpy(), prob[b][wq, wc].numpy(), rtol=1e-5)
    print(f"[det_select {mode}] {left_out} of {total} images left out; the NMS removed {suppressed} candidates")
    assert left_out <= 0.05 * total
    return suppressed


@pytest.mark.gpu
def test_coco_mode_equals_the_host_expression():
    """no threshold, NMS at 0.7, top 100; the small shapes have kept * K < 100"""
    assert _compare("coco") > 0          # the suppression path ran


@pytest.mark.gpu
def test_video_mode_equals_the_host_expression():
    """score threshold 0.1, NMS at 0.9, no top-k"""
    assert _compare("video") > 0         # the suppression path ran


def _boxes(rows):
    return torch.tensor(rows, dtype=torch.float32)[None]


@pytest.mark.gpu
def test_hand_built_cases_are_exact():
    # a chain A-B-C of one class: IoU(A,B) = IoU(B,C) = 0.818 > 0.7 > IoU(A,C) = 0.667: B goes, and removes nothing
    logits = torch.tensor([[[2.0, -5.0], [1.0, -5.0], [0.0, -5.0]]])
    chain = _boxes([[0.30, 0.5, 0.2, 0.2], [0.32, 0.5, 0.2, 0.2], [0.34, 0.5, 0.2, 0.2]])
    kept, labels, _ = unpack(run_abi(logits, chain, None, 0.7, 0), 3, 0)
    assert kept[0].tolist() == [0, 2] and labels[0].tolist() == [0, 0, 0]
    # the same in the other query order: the order is the score's, not the index's
    kept, _, _ = unpack(run_abi(logits.flip(1), chain.flip(1), None, 0.7, 0), 3, 0)
    assert kept[0].tolist() == [2, 0]
    # identical boxes of different classes are all kept
    logits = torch.full((1, 3, 3), -5.0)
    logits[0, 0, 2], logits[0, 1, 0], logits[0, 2, 1] = 1.0, 3.0, 2.0
    same = _boxes([[0.5, 0.5, 0.2, 0.3]] * 3)
    kept, labels, _ = unpack(run_abi(logits, same, None, 0.7, 0), 3, 0)
    assert kept[0].tolist() == [1, 2, 0] and labels[0].tolist() == [2, 0, 1]
    # ... and of one class: only the best
    kept, _, _ = unpack(run_abi(logits[:, :, :1] + torch.tensor([0.0, 8.0, 7.0])[None, :, None], same, None, 0.7, 0), 3, 0)
    assert kept[0].tolist() == [1]
    # two zero-size boxes of one class: IoU is 0 / 0, which is not > thr
    kept, _, _ = unpack(run_abi(torch.tensor([[[1.0], [2.0]]]), _boxes([[0.5, 0.5, 0.0, 0.0]] * 2), None, 0.7, 0), 2, 0)
    assert kept[0].tolist() == [1, 0]
    # all-equal logits: index order, label 0, the top-k in flat order
    far = _boxes([[0.1 + 0.2 * i, 0.5, 0.05, 0.05] for i in range(5)])
    a = run_abi(torch.full((1, 5, 4), 0.25), far, None, 0.7, 100)
    kept, labels, pairs = unpack(a, 5, 100)
    assert kept[0].tolist() == [0, 1, 2, 3, 4] and labels[0].tolist() == [0] * 5 and a[0, 2] == 20
    assert pairs[0].tolist() == [[q, c] for q in range(5) for c in range(4)]
    # video mode, nothing above the threshold: exactly the best query, the lowest index on a tie, and no NMS
    logits = torch.tensor([[[-3.0, -2.0], [-2.5, -4.0], [-1.0, -6.0], [-7.0, -1.5], [-1.0, -1.0]]])
    a = run_abi(logits, _boxes([[0.5, 0.5, 0.2, 0.2]] * 5), 0.9, 0.9, 0)
    kept, labels, _ = unpack(a, 5, 0)
    assert kept[0].tolist() == [2] and a[0, 1] == 1 and labels[0].tolist() == [1, 0, 0, 1, 0]
    # a candidate exactly at score_thr (sigmoid(0) = 0.5) is not selected
    kept, _, _ = unpack(run_abi(torch.tensor([[[0.0, -1.0], [-2.0, 1.0], [0.0, 0.0]]]), far[:, :3], 0.5, 0.9, 0), 3, 0)
    assert kept[0].tolist() == [1]


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["nan_logit", "inf_box"])
def test_non_finite_input_sets_that_images_status_only(what):
    logits, boxes = make_inputs(5, 3, 37, 3, 0.7)
    clean = run_abi(logits, boxes, None, 0.7, 100)
    if what == "nan_logit":
        logits[1, 20, 2] = float("nan")
    else:
        boxes[1, 36, 3] = float("inf")
    a = run_abi(logits, boxes, None, 0.7, 100)
    assert a[:, 0].tolist() == [0, 1, 0]
    np.testing.assert_array_equal(a[[0, 2]], clean[[0, 2]])
    assert a[1, 1] == 0 and a[1, 2] == 0 and (a[1, 4:] == -1).all()
    with pytest.raises(_lib.VnextHipError, match="non-finite"):
        DS.select_detections(logits.cuda(), boxes.cuda(), iou_thr=0.7, topk=100)
    with pytest.raises(_lib.VnextHipError, match="non-finite"):
        DS.select_detections(logits, boxes, iou_thr=0.7, topk=100)


@pytest.mark.gpu
def test_shapes_beyond_the_limits_are_refused_before_any_launch():
    for Q, K, topk in ((4096, 1, 0), (1, 4097, 0), (4, 2, 257)):
        logits, boxes = make_inputs(1, 1, Q, K, 0.7)
        run_abi(logits, boxes, None, 0.7, topk, expect=_lib.VNX_ERR_UNSUPPORTED)
        assert "vnx_det_select" in _lib.lib().vnx_last_error().decode()
    # what must be supported at least: 1024 queries, 128 classes, top 128
    logits, boxes = make_inputs(2, 1, 1024, 128, 0.7)
    a = run_abi(logits, boxes, None, 0.7, 128)
    want = DS.select_detections_host(logits, boxes, iou_thr=0.7, topk=128)
    kept, _, pairs = unpack(a, 1024, 128)
    assert not fragile(logits[0], boxes[0], 0.7, None, 128)      # a property of the seeded input: the comparison runs
    np.testing.assert_array_equal(kept[0], want.kept[0])
    np.testing.assert_array_equal(pairs[0], want.topk[0])
    # B = 0: ok, nothing launched
    lib = _lib.lib()
    assert lib.vnx_det_select(None, None, 0, 300, 80, ctypes.c_float(-1.0), ctypes.c_float(0.7), 100, None, 0, None) == _lib.VNX_OK
    # the wrapper raises; select_candidates falls back to the host loop
    logits, boxes = make_inputs(3, 2, 4096, 2, 0.9)
    with pytest.raises(DS.DetSelectUnsupported):
        DS.select_detections(logits.cuda(), boxes.cuda(), iou_thr=0.9, score_thr=0.1)
    me = types.SimpleNamespace(device_selection=True, inference_select_thres=0.1)
    picks = idol_mod.IDOL.select_candidates(me, logits.cuda(), boxes.cuda())
    me.device_selection = False
    for got, want in zip(picks, idol_mod.IDOL.select_candidates(me, logits.cuda(), boxes.cuda())):
        np.testing.assert_array_equal(got, want)


@pytest.mark.gpu
def test_two_runs_are_byte_equal():
    logits, boxes = make_inputs(9, 4, 300, 80, 0.7)
    first = run_abi(logits, boxes, None, 0.7, 100)
    np.testing.assert_array_equal(first, run_abi(logits, boxes, None, 0.7, 100))
    first = run_abi(logits, boxes, 0.1, 0.9, 0)
    np.testing.assert_array_equal(first, run_abi(logits, boxes, 0.1, 0.9, 0))


# ---- the video fixture ------------------------------------------------------------------------------------------------------
def _video(v, device):
    g = dict(np.load(os.path.join(GOLDEN_DIR, "inference_idol.npz")))
    return g, {k: torch.from_numpy(g[f"v{v}.{k}"]).to(device) for k in ("pred_logits", "pred_boxes", "pred_masks", "pred_inst_embed")}


def _host_picks(logits, boxes, thr=0.1):
    me = types.SimpleNamespace(device_selection=False, inference_select_thres=thr)
    return idol_mod.IDOL.select_candidates(me, logits, boxes)


@pytest.mark.gpu
@pytest.mark.parametrize("v", [0, 1])
def test_video_fixture_selection_on_the_device_equals_the_host_picks(v):
    _, t = _video(v, "cuda:0")
    me = types.SimpleNamespace(device_selection=True, inference_select_thres=0.1)
    picks = idol_mod.IDOL.select_candidates(me, t["pred_logits"], t["pred_boxes"])
    want = _host_picks(t["pred_logits"], t["pred_boxes"])
    assert len(picks) == len(want)
    for got, ref in zip(picks, want):
        assert isinstance(got, np.ndarray) and got.dtype == np.int64
        np.testing.assert_array_equal(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("v", [0, 1])
def test_video_fixture_association_with_device_selection(v):
    """`associate` on the device's picks reproduces the reference's video output (the tolerances of test_idol_model.py)"""
    from vnext_amd import train as T
    g, t = _video(v, "cuda:0")
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": "cuda:0", **TINY})).eval()
    T.enable_device_selection(model)
    picks = model.select_candidates(t["pred_logits"], t["pred_boxes"])
    per_frame = []
    for f, c in enumerate(picks):
        q = torch.from_numpy(c).to("cuda:0")
        per_frame.append({"indices": c.tolist(), "logits": t["pred_logits"][f, q], "boxes": t["pred_boxes"][f, q],
                          "embeds": t["pred_inst_embed"][f, q], "masks": t["pred_masks"][f, q]})
    oh, ow, ih, iw = (int(x) for x in g[f"v{v}.sizes"])
    tracker = trk.IDOL_Tracker(init_score_thr=0.2, obj_score_thr=0.1, nms_thr_pre=0.5, nms_thr_post=0.05,
                               addnew_score_thr=0.2, memo_tracklet_frames=10, memo_momentum=0.8, long_match=True,
                               frame_weight=True, temporal_weight=True, memory_len=3)
    res = model.associate(per_frame, tracker, (oh, ow), (ih, iw))
    np.testing.assert_array_equal(np.array(res["pred_labels"]), g[f"v{v}.labels"])
    np.testing.assert_allclose(np.array(res["pred_scores"]), g[f"v{v}.scores"], rtol=1e-5)
    present = g[f"v{v}.present"]
    want = np.unpackbits(g[f"v{v}.masks"], axis=-1)[..., :ow].astype(bool)
    assert len(res["pred_masks"]) == present.shape[0]
    for i, track in enumerate(res["pred_masks"]):
        assert [m is not None for m in track] == present[i].tolist()
        for f, m in enumerate(track):
            if m is not None:
                assert float((m.numpy() != want[i, f]).mean()) < 2e-3, (i, f)


# ---- CPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [0, 1])
def test_select_detections_on_cpu_equals_class_aware_nms_on_the_video_fixture(v):
    _, t = _video(v, "cpu")
    logits, boxes = t["pred_logits"], t["pred_boxes"]
    sel = DS.select_detections(logits, boxes, iou_thr=0.9, score_thr=0.1)
    assert sel.topk is None and sel.counts.tolist() == [len(k) for k in sel.kept]
    for f, (got, ref) in enumerate(zip(sel.kept, _host_picks(logits, boxes))):
        np.testing.assert_array_equal(got, ref)
        np.testing.assert_array_equal(sel.labels[f], logits[f].argmax(-1).numpy())
    assert any(len(k) > 1 for k in sel.kept)


def test_the_input_recipe_leaves_few_images_out():
    """The margins are a property of the inputs alone: checked without a device."""
    for iou_thr, score_thr, topk in ((0.7, None, 100), (0.9, 0.1, None)):
        out = total = 0
        for s, (Q, K) in enumerate(SHAPES):
            logits, boxes = make_inputs(100 + s, BATCH, Q, K, iou_thr)
            out += sum(fragile(logits[b], boxes[b], iou_thr, score_thr, topk) for b in range(BATCH))
            total += BATCH
        print(f"[det_select inputs] iou_thr {iou_thr}: {out} of {total} images left out")
        assert out <= 0.05 * total
