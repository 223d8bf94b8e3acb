"""Detection selection on the device (vnext_amd/csrc/det_select.hip): every query's best class, the score threshold,
class-aware greedy box NMS and the top-k over (kept query, class), one launch for a batch of images, one workgroup per
image.  It serves IDOL's per-frame candidate selection (`IDOL.select_candidates`: `score_thr`, NMS at 0.9, no top-k) and
its COCO-pretrain inference (`IDOL.coco_postprocess`: no threshold, NMS at 0.7, top 100).

`select_detections` is the op.  CUDA tensors take the kernel; its compact int32 result crosses to the host in ONE copy.
That copy is the call's one synchronisation: the counts size what follows (the mask head's rows, the tracker's
detections), so they are needed on the host.  CPU tensors take the host expression -- `class_aware_nms` + `torch.topk`,
which is also what the tests compare the kernel with.

Scores are never produced here: a caller forms them as `logits[b, q, c].sigmoid()` with torch, so they equal the eager
expression by construction.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from .. import _lib


class DetSelectUnsupported(_lib.VnextHipError):
    """More queries than the kernel's LDS layout holds, or classes / topk beyond its limits: select on the host."""


class Detections(NamedTuple):
    """Per image (lists over the batch; host arrays): `kept` int64 [n_b] the queries that survive the NMS, in NMS order
    (max logit descending, query ascending); `labels` int64 [Q] every query's first-argmax class; `topk` int64 [m_b, 2]
    the (query, class) pairs of the `min(topk, n_b * K)` largest class logits of the kept queries, largest first (None
    without `topk`).  `counts` int64 [B] = the n_b."""
    kept: list
    counts: np.ndarray
    labels: list
    topk: list | None


def _check(status: int) -> None:
    if status == _lib.VNX_ERR_UNSUPPORTED:
        raise DetSelectUnsupported(_lib.lib().vnx_last_error().decode())
    _lib.check(status)


def out_words(queries: int, topk: int) -> int:
    """int32 words of one image's slice of the output buffer"""
    return int(_lib.lib().vnx_det_select_out_words(int(queries), int(topk)))


def box_cxcywh_to_xyxy_host(b):
    c, wh = b[..., :2], b[..., 2:]
    return np.concatenate([c - np.float32(0.5) * wh, c + np.float32(0.5) * wh], -1)


def class_aware_nms(boxes_xyxy, scores, classes, thr):
    """torchvision.ops.batched_nms restated on host arrays (published algorithm: boxes of
    different classes never suppress each other; greedy by descending score; returns the kept
    indices in descending-score order)."""
    order = np.argsort(-scores, kind="stable")
    b = boxes_xyxy[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    keep = np.ones(len(order), dtype=bool)
    for i in range(len(order)):
        if not keep[i]:
            continue
        lt = np.maximum(b[i, :2], b[i + 1:, :2])
        rb = np.minimum(b[i, 2:], b[i + 1:, 2:])
        wh = np.clip(rb - lt, 0, None)
        inter = wh[:, 0] * wh[:, 1]
        iou = inter / (area[i] + area[i + 1:] - inter)
        keep[i + 1:] &= ~((iou > thr) & (classes[order[i + 1:]] == classes[order[i]]))
    return order[keep]


def select_detections_host(logits, boxes, *, iou_thr, score_thr=None, topk=None):
    """The host expression on CPU tensors: the reference's arithmetic (fp32 sigmoid scores, `class_aware_nms`,
    `torch.topk` on the kept queries' scores)."""
    logits, boxes = logits.detach().float().cpu(), boxes.detach().float().cpu()
    if not bool(torch.isfinite(logits).all()) or not bool(torch.isfinite(boxes).all()):
        raise _lib.VnextHipError("select_detections: non-finite logits or boxes")
    prob = logits.sigmoid()
    best, label = prob.max(-1)
    xyxy = torch.cat([boxes[..., :2] - 0.5 * boxes[..., 2:], boxes[..., :2] + 0.5 * boxes[..., 2:]], -1).numpy()
    best, label_np = best.numpy(), label.numpy()
    kept, labels, pairs = [], [], []
    K = logits.shape[-1]
    for b in range(logits.shape[0]):
        score, cls = best[b], label_np[b].astype(np.int64)
        cand = np.arange(len(score)) if score_thr is None else np.nonzero(score > np.float32(score_thr))[0]
        if len(cand) == 0:
            cand = np.array([int(np.argmax(score))], dtype=np.int64)
        else:
            with np.errstate(invalid="ignore", divide="ignore"):      # 0 / 0 of two zero-size boxes: not > thr
                cand = cand[class_aware_nms(xyxy[b][cand], score[cand], cls[cand], iou_thr)]
        cand = cand.astype(np.int64)
        kept.append(cand)
        labels.append(cls)
        if topk is not None:
            flat = prob[b][torch.from_numpy(cand)].reshape(-1)
            idx = torch.topk(flat, min(int(topk), flat.numel()), dim=0)[1].numpy()
            pairs.append(np.stack([cand[idx // K], idx % K], 1).astype(np.int64).reshape(-1, 2))
    return Detections(kept, np.array([len(k) for k in kept], dtype=np.int64), labels, pairs if topk is not None else None)


def det_select_raw(logits, boxes, score_thr, iou_thr, topk):
    """The launch alone: fp32 contiguous CUDA logits [B, Q, K] and boxes [B, Q, 4] -> int32 [B, out_words(Q, topk)] on
    the device (layout: include/vnext_hip.h).  Neither synchronises nor copies."""
    B, Q, K = (int(v) for v in logits.shape)
    stride = out_words(Q, topk)
    with torch.cuda.device(logits.device):
        out = torch.empty(B, stride, dtype=torch.int32, device=logits.device)
        _check(_lib.lib().vnx_det_select(logits.data_ptr(), boxes.data_ptr(), B, Q, K, float(score_thr), float(iou_thr),
                                         int(topk), out.data_ptr(), stride, _lib.current_stream(logits)))
    return out


def select_detections(logits, boxes, *, iou_thr, score_thr=None, topk=None):
    """logits [B, Q, K] (pre-sigmoid) and boxes [B, Q, 4] (cxcywh) -> `Detections`.

    Per image: every query's label is the first argmax of its logits; the candidates are the queries whose best class
    score is `> score_thr` (all of them with `score_thr=None`; the single best query, and no NMS, when none passes);
    class-aware greedy NMS at `iou_thr` in (max logit descending, query ascending) order; with `topk` the largest
    `min(topk, kept * K)` class logits of the kept queries as (query, class) pairs.

    CUDA tensors: one kernel launch and one device-to-host copy of the compact result -- the one synchronisation of the
    call, which stays because the counts size what the caller does next.  16-bit inputs are converted with `.float()`.
    Raises `DetSelectUnsupported` for a shape the kernel refuses (the caller selects on the host) and `VnextHipError`
    when an image holds a non-finite logit or box.  CPU tensors: `select_detections_host`."""
    if logits.dim() != 3 or boxes.dim() != 3 or tuple(boxes.shape) != tuple(logits.shape[:2]) + (4,):
        raise ValueError(f"select_detections: logits {tuple(logits.shape)} / boxes {tuple(boxes.shape)} are not "
                         "[B, Q, K] / [B, Q, 4]")
    if not logits.is_cuda:
        return select_detections_host(logits, boxes, iou_thr=iou_thr, score_thr=score_thr, topk=topk)
    B, Q, K = (int(v) for v in logits.shape)
    k = 0 if topk is None else int(topk)
    if topk is not None and k < 1:
        raise ValueError("select_detections: topk must be positive")
    if Q < 1 or K < 1:
        raise ValueError("select_detections: no queries or no classes")
    raw = det_select_raw(logits.detach().float().contiguous(), boxes.detach().float().contiguous(),
                         -1.0 if score_thr is None else score_thr, iou_thr, k)
    a = raw.cpu().numpy()                                  # the one copy
    bad = np.nonzero(a[:, 0] != 0)[0] if B else []
    if len(bad):
        raise _lib.VnextHipError(f"select_detections: non-finite logits or boxes in image(s) {bad.tolist()}")
    kept = [a[b, 4:4 + int(a[b, 1])].astype(np.int64) for b in range(B)]
    labels = [a[b, 4 + Q:4 + 2 * Q].astype(np.int64) for b in range(B)]
    pairs = None
    if topk is not None:
        pairs = [a[b, 4 + 2 * Q:4 + 2 * Q + 2 * int(a[b, 2])].astype(np.int64).reshape(-1, 2) for b in range(B)]
    return Detections(kept, a[:, 1].astype(np.int64), labels, pairs)
