"""Clip-level set criterion of SeqFormer: Hungarian matching + focal / L1 / GIoU / mask losses.

Host-side mirror of the reference's training objective (same loss names, same numbers):
  matcher     projects/SeqFormer/seqformer/models/matcher.py:25-96
  criterion   projects/SeqFormer/seqformer/models/deformable_detr.py:231-439
  focal/dice  projects/SeqFormer/seqformer/models/segmentation_condInst.py:680-723
  GIoU loss   fvcore.nn.giou_loss (fvcore 0.1.5): 1 - GIoU, eps 1e-7 on union and hull
This is the caller of the hot path on the training side (it decides which instances the dynamic
mask head runs for), not a kernel.  Differences in *how*, not in *what*:
  * the cost matrices of all decoder layers are built in one batched pass and cross to the
    host in ONE copy (`match_all_layers`); the reference matches inside the layer loop -> 6
    device syncs per step (deformable_detr.py / segmentation_condInst.py:146-147);
  * the per-frame GIoU loop (matcher.py:69-72) is one broadcast over the frame axis;
  * `num_boxes` stays a tensor -- no `.item()` sync (deformable_detr.py:417-419);
  * opt-in (`match_all_layers_device`): cost and assignment of every (layer, clip) in ONE kernel on the device
    (vnext_amd/csrc/lsap.hip), the indices never leave it -- no copy to the host, no scipy, no upload.
  * opt-in (`fused_mask_loss`): focal + dice of the mask logits from one kernel pass each way (vnext_amd/csrc/mask_loss.hip),
    the ground truth read in place -- no sliced / padded / gathered float copy, nothing [R, M]-sized kept for the backward.
  * opt-in (`fused_set_loss`): the class focal loss, the boxes' L1 and GIoU losses and `class_error` of every decoder layer
    from one op (vnext_amd/csrc/set_loss.hip): no one-hot target, no gathers, two launches forward and one backward.
Shared with IDOL's criterion (idol_criterion.py, whose `IDOLCriterion` derives from `SetCriterion`), and written once:
  * the flat pair list `DeviceMatch(lay, clip, qry, tgt)` every all-layers expression and fused op consumes.  On the
    device-matching path the matcher returns it; everywhere else `flat_pairs` makes it from the host `indices_list` of
    either matcher.  The models call it once per step and pass the object on, so the rows of the mask head and the rows
    of the losses cannot fall out of step; `layer_counts` gives the host integers that go with it.
  * the loss terms before their reductions: `focal_term`, `dice_term`, `gt_canvas` (the ground truth as the mask logits
    see it), `box_terms`, `layer_suffixes`.  The reductions stay with each criterion: SeqFormer sums `view(Ld, n)`,
    IDOL segment-sums over unequal layer counts.  tools/time_set_loss.py and tools/time_mask_loss.py time these same
    functions as the ATen baseline of the fused ops.
"""
from __future__ import annotations

from collections import namedtuple
from itertools import accumulate

import torch
import torch.nn as nn
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment


def box_cxcywh_to_xyxy(b):
    c, wh = b[..., :2], b[..., 2:]
    return torch.cat([c - 0.5 * wh, c + 0.5 * wh], -1)


def box_xyxy_to_cxcywh(b):
    lo, hi = b[..., :2], b[..., 2:]
    return torch.cat([(lo + hi) / 2, hi - lo], -1)


def _area(b):
    return (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])


def pairwise_giou(a, b):
    """a [..., N, 4], b [..., M, 4] (xyxy, broadcastable leading axes) -> GIoU [..., N, M]
    (util/box_ops.py:65-86: eps only on the enclosing area)."""
    a, b = a[..., :, None, :], b[..., None, :, :]
    wh = (torch.minimum(a[..., 2:], b[..., 2:]) - torch.maximum(a[..., :2], b[..., :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = _area(a) + _area(b) - inter
    hull = (torch.maximum(a[..., 2:], b[..., 2:]) - torch.minimum(a[..., :2], b[..., :2])).clamp(min=0)
    hull = hull[..., 0] * hull[..., 1]
    return inter / union - (hull - union) / (hull + 1e-7)


def giou_loss(a, b, eps=1e-7):
    """element-wise 1 - GIoU of matched xyxy boxes (fvcore.nn.giou_loss, reduction 'none')."""
    lo, hi = torch.maximum(a[..., :2], b[..., :2]), torch.minimum(a[..., 2:], b[..., 2:])
    overlap = (hi > lo).all(-1)
    inter = torch.where(overlap, (hi - lo).prod(-1), torch.zeros_like(lo[..., 0]))
    union = _area(a) + _area(b) - inter
    hull = (torch.maximum(a[..., 2:], b[..., 2:]) - torch.minimum(a[..., :2], b[..., :2])).prod(-1)
    return 1 - (inter / (union + eps) - (hull - union) / (hull + eps))


def focal_term(logits, targets, alpha=0.25, gamma=2.0, p=None):
    """element-wise sigmoid focal term of logits against a 0/1 target (segmentation_condInst.py:698-720), before any
    reduction.  `p`: logits.sigmoid() where the caller holds it already (the mask branch shares it with `dice_term`)."""
    if p is None:
        p = logits.sigmoid()
    ce = F.binary_cross_entropy_with_logits(logits, targets, reduction="none")
    p_t = p * targets + (1 - p) * (1 - targets)
    loss = ce * (1 - p_t) ** gamma
    if alpha >= 0:
        loss = (alpha * targets + (1 - alpha) * (1 - targets)) * loss
    return loss


def sigmoid_focal_loss(logits, targets, num_boxes, alpha=0.25, gamma=2.0):
    """segmentation_condInst.py:698-723: mean over the last axis, summed, / num_boxes"""
    return focal_term(logits, targets, alpha, gamma).mean(1).sum() / num_boxes


def dice_term(p, targets):
    """per-row dice term of probabilities p [R, M] (the mask logits' sigmoid) against targets [R, M] -> [R]"""
    num = 2 * (p * targets).sum(1)
    den = p.sum(-1) + targets.sum(-1)
    return 1 - (num + 1) / (den + 1)


def dice_loss(logits, targets, num_boxes):
    """segmentation_condInst.py:680-695"""
    return dice_term(logits.sigmoid().flatten(1), targets).sum() / num_boxes


def gt_canvas(masks, stride, h, w, dtype):
    """Ground-truth masks as the mask logits see them (deformable_detr.py:353-362): per entry of `masks` ([..., H_i, W_i],
    one per clip or image) sampled at the centre of each stride-`stride` cell, cast, zero-padded to the /32-padded canvas
    (h, w), then concatenated along the first axis."""
    out = []
    for m in masks:
        m = m[..., stride // 2::stride, stride // 2::stride]
        assert m.shape[-2] <= h and m.shape[-1] <= w
        out.append(F.pad(m.to(dtype), (0, w - m.shape[-1], 0, h - m.shape[-2])))
    return torch.cat(out)


def box_terms(pred, want):
    """gathered pairs pred / want [R, ..., 4] (cxcywh) -> (L1 per pair [R], 1 - GIoU per box [R, ...])"""
    return (pred - want).abs().flatten(1).sum(1), giou_loss(box_cxcywh_to_xyxy(pred), box_cxcywh_to_xyxy(want))


def layer_suffixes(layers):
    """loss-name suffixes of deep supervision: `_0 ... _{Ld-2}` for the auxiliary layers, none for the last"""
    return [f"_{l}" for l in range(layers - 1)] + [""]


# What `HungarianMatcher.match_all_layers_device` returns and `SetCriterion.forward_all_layers` accepts in place of the host
# `indices_list`: int64 device tensors [Ld * n] each (n = all targets of the batch), layer-major, clips in order, a clip's
# pairs by ascending query.  lay / clip / qry index logits [Ld, N, Q, K]; tgt indexes the batch's concatenated targets.
DeviceMatch = namedtuple("DeviceMatch", ["lay", "clip", "qry", "tgt"])


def _target_offsets(sizes):
    """[0, n_0, n_0 + n_1, ...]: where each clip's targets begin among the batch's targets laid back to back"""
    return list(accumulate(sizes, initial=0))


def flat_pairs(indices_list, sizes, device=None, non_blocking=False):
    """host indices_list[layer][clip] -> DeviceMatch: THE place that lays the pairs out (everything that gathers by them
    -- controller, mask head rows, every loss -- takes its order from one call of this).  A clip's entry is either
    (query idx, target idx) (`HungarianMatcher`) or (selected [Q] bool, target idx of each selected query, ascending)
    (`OTAMatcher`); `sizes` are the clips' target counts.  One `cat` per field on the host, one transfer per field
    (`device` None: the vectors stay where the indices are)."""
    start = _target_offsets(sizes)
    lay, clip, qry, tgt = [], [], [], []
    for l, ind in enumerate(indices_list):
        for i, (q, j) in enumerate(ind):
            if q.dtype == torch.bool:
                q = torch.nonzero(q).flatten()
            lay.append(torch.full_like(q, l))
            clip.append(torch.full_like(q, i))
            qry.append(q)
            tgt.append(j.long() + start[i])                 # into the concatenated targets
    if not qry:                                             # no layer or no clip at all
        lay = clip = qry = tgt = [torch.zeros(0, dtype=torch.int64)]
    return DeviceMatch(*(torch.cat(v).to(device, non_blocking=non_blocking) for v in (lay, clip, qry, tgt)))


def layer_counts(indices_list):
    """pairs per layer of a host indices_list (either form), as host integers"""
    return [sum(len(j) for _, j in ind) for ind in indices_list]

_MATCH_CONSTANTS = {}


def _match_constants(sizes, layers, device):
    """What the host knows of a batch's matching from its target counts alone, as device tensors: clip offsets int32
    [N + 1], and per pair (layer-major) the layer, the clip and the clip's first target.  Made by device-side fills (no
    upload, so no blocking pageable copy) and kept per (target counts, layers, device), as `scale_tensor` keeps its
    constants."""
    key = (tuple(sizes), int(layers), str(device))
    c = _MATCH_CONSTANTS.get(key)
    if c is None:
        if len(_MATCH_CONSTANTS) > 256:
            _MATCH_CONSTANTS.clear()
        start = _target_offsets(sizes)
        offsets = torch.cat([torch.full((1,), v, dtype=torch.int32, device=device) for v in start])
        clip = torch.cat([torch.full((n,), i, dtype=torch.int64, device=device) for i, n in enumerate(sizes)])
        first = torch.cat([torch.full((n,), start[i], dtype=torch.int64, device=device) for i, n in enumerate(sizes)])
        lay = torch.arange(layers, dtype=torch.int64, device=device).repeat_interleave(start[-1], output_size=layers * start[-1])
        c = _MATCH_CONSTANTS[key] = (offsets, lay, clip.repeat(layers), first)
    return c


class HungarianMatcher(nn.Module):
    """One-to-one assignment of queries to ground-truth *clip* instances; a box cost is the
    distance over all frames of the clip (matcher.py:53-96)."""

    def __init__(self, multi_frame=True, cost_class=1.0, cost_bbox=1.0, cost_giou=1.0):
        super().__init__()
        assert cost_class != 0 or cost_bbox != 0 or cost_giou != 0, "all costs cant be 0"
        self.multi_frame = multi_frame
        self.cost_class, self.cost_bbox, self.cost_giou = cost_class, cost_bbox, cost_giou

    @torch.no_grad()
    def cost(self, logits, boxes, targets):
        """logits [..., bs, Q, K], boxes [..., bs, nf, Q, 4] (any leading layer axes) ->
        cost [..., bs, Q, sum n] on the device."""
        tgt_ids = torch.cat([t["labels"] for t in targets])
        nf = boxes.shape[-3]
        tgt = torch.cat([t["boxes"] for t in targets]).reshape(len(tgt_ids), nf, 4).to(boxes.dtype)
        if logits.dtype in (torch.bfloat16, torch.float16) or boxes.dtype in (torch.bfloat16, torch.float16):
            logits, boxes = logits.float(), boxes.float()                    # autocast outputs: fp32 costs
        prob = logits.sigmoid()
        out = boxes.transpose(-3, -2)                                        # [..., bs, Q, nf, 4]
        # Euclidean distance over the clip's nf*4 coordinates (torch.cdist default p=2, matcher.py:66)
        c_box = torch.cdist(out.flatten(-2), tgt.flatten(1))
        tgt = tgt.clamp(min=1e-7, max=1)                                     # matcher.py:68
        g = pairwise_giou(box_cxcywh_to_xyxy(out.transpose(-3, -2)),         # frames leading: [..., bs, nf, Q, n]
                          box_cxcywh_to_xyxy(tgt.transpose(0, 1)))
        c_giou = -g.mean(-3)
        alpha, gamma = 0.25, 2.0
        neg = (1 - alpha) * prob ** gamma * -(1 - prob + 1e-8).log()
        pos = alpha * (1 - prob) ** gamma * -(prob + 1e-8).log()
        c_cls = (pos - neg)[..., tgt_ids]
        return self.cost_bbox * c_box + self.cost_class * c_cls + self.cost_giou * c_giou

    @staticmethod
    def _solve(cost_cpu, sizes):
        """cost_cpu [bs, Q, sum n] on the host -> [(query idx, target idx)] per clip"""
        out, start = [], 0
        for i, n in enumerate(sizes):
            q, t = linear_sum_assignment(cost_cpu[i, :, start:start + n])
            out.append((torch.as_tensor(q, dtype=torch.int64), torch.as_tensor(t, dtype=torch.int64)))
            start += n
        return out

    def forward(self, outputs, targets, nf=None, valid_ratios=None):
        """The reference call: one layer's {'pred_logits', 'pred_boxes'} -> indices."""
        sizes = [len(t["labels"]) for t in targets]
        c = self.cost(outputs["pred_logits"], outputs["pred_boxes"], targets).cpu().numpy()
        return self._solve(c, sizes)

    def match_all_layers(self, logits, boxes, targets):
        """logits [Ld, bs, Q, K], boxes [Ld, bs, nf, Q, 4] -> indices_list (one entry per decoder
        layer); one device->host copy for all layers."""
        sizes = [len(t["labels"]) for t in targets]
        c = self.cost(logits, boxes, targets).cpu().numpy()
        return [self._solve(c[l], sizes) for l in range(c.shape[0])]

    @torch.no_grad()
    def match_all_layers_device(self, logits, boxes, targets):
        """`match_all_layers` without leaving the device: logits [Ld, bs, Q, K], boxes [Ld, bs, nf, Q, 4] -> DeviceMatch.
        One kernel computes the cost blocks and solves them (vnext_amd/ops/lsap.py); nothing is copied to the host and
        nothing is uploaded.  The same pairs as `match_all_layers` wherever the optimum is unique beyond the fp32
        rounding of the two cost evaluations.  A clip whose cost is not finite comes back with -1 indices: scipy
        raises there, this path does not look (looking is a synchronisation).
        A batch the kernel does not hold (a clip with more than ~128 targets at 300 queries, or more targets than
        queries) is matched on the host and uploaded."""
        from ..ops.lsap import LsapUnsupported, seqformer_match
        sizes = [len(t["labels"]) for t in targets]
        Ld = logits.shape[0]
        dev = logits.device
        if sum(sizes) == 0:                               # nobody has targets: nothing to launch
            empty = torch.empty(0, dtype=torch.int64, device=dev)
            return DeviceMatch(empty, empty, empty, empty)
        offsets, lay, clip, first = _match_constants(sizes, Ld, dev)
        labels = torch.cat([t["labels"] for t in targets]).to(dev)
        nf = boxes.shape[-3]
        tgt_boxes = torch.cat([t["boxes"] for t in targets]).reshape(len(labels), nf, 4).to(dev)
        try:
            qry, tgt = seqformer_match(logits, boxes, labels, tgt_boxes, offsets,
                                       (self.cost_class, self.cost_bbox, self.cost_giou), max_targets=max(sizes))
        except LsapUnsupported:
            return flat_pairs(self.match_all_layers(logits, boxes, targets), sizes, dev)
        return DeviceMatch(lay, clip, qry.flatten(), (tgt + first).flatten())


class SetCriterion(nn.Module):
    """labels (focal), boxes (L1 + GIoU over the clip's frames), masks (focal + dice)."""

    def __init__(self, num_classes, matcher, weight_dict, losses, focal_alpha=0.25, mask_out_stride=4, num_frames=1):
        super().__init__()
        self.num_classes, self.matcher, self.weight_dict, self.losses = num_classes, matcher, weight_dict, losses
        self.focal_alpha, self.mask_out_stride, self.num_frames = focal_alpha, mask_out_stride, num_frames
        # mask losses from the fused kernel (vnext_amd/ops/mask_loss.py): the ground truth read in place, one pass each
        # way (opt-in: train.enable_fused_mask_loss).  CUDA tensors only -- there is no fallback behind the switch
        self.fused_mask_loss = False
        # class focal + box L1 / GIoU + class_error of `forward_all_layers` from the fused op (vnext_amd/ops/set_loss.py;
        # opt-in: train.enable_fused_set_loss).  CUDA tensors only -- there is no fallback behind the switch
        self.fused_set_loss = False

    @staticmethod
    def _src_idx(indices):
        return (torch.cat([torch.full_like(s, i) for i, (s, _) in enumerate(indices)]),
                torch.cat([s for s, _ in indices]))

    @staticmethod
    def _tgt_idx(indices):
        return (torch.cat([torch.full_like(t, i) for i, (_, t) in enumerate(indices)]),
                torch.cat([t for _, t in indices]))

    def loss_labels(self, outputs, targets, indices, num_boxes, log=True):
        logits = outputs["pred_logits"]                                     # [bs, Q, K]
        b, q = self._src_idx(indices)
        cls = torch.cat([t["labels"][j.to(t["labels"].device)] for t, (_, j) in zip(targets, indices)])
        onehot = torch.zeros_like(logits)
        onehot[b.to(logits.device), q.to(logits.device), cls.to(logits.device)] = 1
        out = {"loss_ce": sigmoid_focal_loss(logits, onehot, num_boxes, self.focal_alpha, 2.0) * logits.shape[1]}
        if log:
            with torch.no_grad():
                sel = logits[b.to(logits.device), q.to(logits.device)]
                if cls.numel() == 0:
                    out["class_error"] = 100 - torch.zeros([], device=logits.device)
                else:
                    hit = (sel.argmax(-1) == cls.to(logits.device)).float().mean() * 100
                    out["class_error"] = 100 - hit
        return out

    def loss_boxes(self, outputs, targets, indices, num_boxes):
        b, q = self._src_idx(indices)
        pred = outputs["pred_boxes"].transpose(1, 2)[b.to(outputs["pred_boxes"].device), q.to(outputs["pred_boxes"].device)]
        nf = pred.shape[1] if pred.dim() == 3 else outputs["pred_boxes"].shape[1]
        tgt = torch.cat([t["boxes"].reshape(-1, nf, 4)[j.to(t["boxes"].device)] for t, (_, j) in zip(targets, indices)])
        tgt = tgt.to(pred)
        l1 = F.l1_loss(pred.flatten(1), tgt.flatten(1), reduction="none") / nf
        g = giou_loss(box_cxcywh_to_xyxy(pred.flatten(0, 1)), box_cxcywh_to_xyxy(tgt.flatten(0, 1))) / nf
        return {"loss_bbox": l1.sum() / num_boxes, "loss_giou": g.sum() / num_boxes}

    def loss_masks(self, outputs, targets, indices, num_boxes):
        """pred_masks: list over clips of [1, n_i, nf, H/4, W/4] (instances in matched order) or one
        tensor [sum n, nf, H/4, W/4]."""
        src = outputs["pred_masks"]
        if isinstance(src, (list, tuple)):
            src = torch.cat(list(src), 1)[0]
        nf, h, w = src.shape[1:]
        s = self.mask_out_stride
        if self.fused_mask_loss:
            return self._loss_masks_fused(src, targets, indices, num_boxes)
        picked = [t["masks"][j.to(t["masks"].device)] for t, (_, j) in zip(targets, indices)]   # [n_i, nf, H_i, W_i] each
        tgt = gt_canvas(picked, s, h, w, src.dtype) if picked else src.new_zeros((0, nf, h, w))
        if tgt.shape[0] == 0:
            zero = (src * 0).sum()
            return {"loss_mask": zero, "loss_dice": zero}
        src, tgt = src.flatten(1), tgt.flatten(1)
        return {"loss_mask": sigmoid_focal_loss(src, tgt, num_boxes), "loss_dice": dice_loss(src, tgt, num_boxes)}

    def _loss_masks_fused(self, src, targets, indices, num_boxes):
        """`loss_masks` through the fused kernel: the matched targets are named by index (into the clips' targets laid
        back to back: `flat_pairs` of the one layer) instead of gathered."""
        from ..ops.mask_loss import mask_focal_dice
        row_gt = flat_pairs([indices], [len(t["labels"]) for t in targets]).tgt
        if row_gt.numel() == 0:
            zero = (src * 0).sum()
            return {"loss_mask": zero, "loss_dice": zero}
        focal, dice = mask_focal_dice(src, [t["masks"] for t in targets], row_gt.to(src.device), self.mask_out_stride)
        return {"loss_mask": focal.sum() / num_boxes, "loss_dice": dice.sum() / num_boxes}

    # ---- all decoder layers in one pass ------------------------------------------------------
    def forward_all_layers(self, logits, boxes, masks, targets, indices_list, weighted=False):
        """`weighted`: return the terms already multiplied by `weight_dict` (what the model's forward returns,
        seqformer.py:140-144 of the reference): one multiply per loss type on the per-layer vectors and one
        `unbind` each, instead of a multiply and a `select` per (type, layer) -- 60 forward and ~110 backward
        launches fewer per step.

        `forward` for every decoder layer at once: logits [Ld, N, Q, K], boxes [Ld, N, T, Q, 4],
        masks [Ld * n, T, h, w] (the matched instances' mask logits, layer-major, clips in order,
        instances in matched order -- what the fused mask head returns), indices_list[layer][clip] =
        (query idx, target idx) on the host, or the `DeviceMatch` of `match_all_layers_device` (then nothing here
        touches the host: same names, same numbers).  Same names and numbers as `forward` with deep supervision; one set of
        kernels instead of one per layer (the Hungarian matching assigns every target in every layer,
        so each layer contributes the same number n of instances)."""
        Ld, N, Q, K = logits.shape
        T = boxes.shape[2]
        dev = logits.device
        num_boxes = torch.full((1,), float(sum(len(t["labels"]) for t in targets)), device=dev)   # a fill, not an upload
        world = 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(num_boxes)
            world = torch.distributed.get_world_size()
        num_boxes = torch.clamp(num_boxes / world, min=1)[0]
        if isinstance(indices_list, DeviceMatch):      # matched on the device: the index tensors are there already
            lay, clip, qry, tgt = indices_list
        else:                                          # stacked index tensors, built on the host, one transfer each
            lay, clip, qry, tgt = flat_pairs(indices_list, [len(t["labels"]) for t in targets], dev)
        n = len(qry) // Ld
        names = layer_suffixes(Ld)
        out = {}
        # labels (focal): mean over Q * Q = sum over Q
        all_labels = torch.cat([t["labels"] for t in targets]).to(dev)
        if self.fused_set_loss:
            from ..ops.set_loss import set_class_box_losses
            all_boxes = torch.cat([t["boxes"].reshape(-1, T, 4) for t in targets]).to(dev)
            sums = set_class_box_losses(logits, boxes, lay, clip, qry, tgt, all_labels, all_boxes, self.focal_alpha)   # [Ld, 4]
            loss_ce = sums[:, 0] / num_boxes
            l1 = sums[:, 1] / T / num_boxes
            g = sums[:, 2] / T / num_boxes
            out["class_error"] = 100 - sums.detach()[-1, 3] / max(n, 1) * 100
        else:
            onehot = torch.zeros_like(logits)
            onehot[lay, clip, qry, all_labels[tgt]] = torch.ones((), dtype=logits.dtype, device=dev)   # a Python 1 is uploaded
            loss_ce = focal_term(logits, onehot, self.focal_alpha).mean(2).sum((1, 2)) / num_boxes * Q
            with torch.no_grad():
                if n:
                    sel = logits[-1][clip[-n:], qry[-n:]]
                    out["class_error"] = 100 - (sel.argmax(-1) == all_labels[tgt[-n:]]).float().mean() * 100
                else:
                    out["class_error"] = 100 - torch.zeros([], device=dev)
            # boxes (L1 + GIoU over the clip's frames)
            pred = boxes.transpose(2, 3)[lay, clip, qry]                                   # [Ld*n, T, 4]
            all_boxes = torch.cat([t["boxes"].reshape(-1, T, 4) for t in targets]).to(pred)
            l1, g = box_terms(pred, all_boxes[tgt])                                        # [Ld*n], [Ld*n, T]
            l1 = l1.view(Ld, n).sum(1) / T / num_boxes
            g = g.view(Ld, n * T).sum(1) / T / num_boxes
        # masks (focal + dice)
        if n and self.fused_mask_loss:
            from ..ops.mask_loss import mask_focal_dice
            fm, dice = mask_focal_dice(masks, [t["masks"] for t in targets], tgt, self.mask_out_stride)   # [Ld*n] each
            loss_mask = fm.view(Ld, n).sum(1) / num_boxes
            loss_dice = dice.view(Ld, n).sum(1) / num_boxes
        elif n:
            h, w = masks.shape[-2:]
            gt = gt_canvas([t["masks"] for t in targets], self.mask_out_stride, h, w, masks.dtype)
            gt = gt.to(dev)[tgt].flatten(1)                                            # [Ld*n, T*h*w]
            src = masks.flatten(1)
            pm = src.sigmoid()                                                         # one sigmoid for both terms
            loss_mask = focal_term(src, gt, p=pm).mean(1).view(Ld, n).sum(1) / num_boxes
            loss_dice = dice_term(pm, gt).view(Ld, n).sum(1) / num_boxes
        else:
            loss_mask = loss_dice = (masks * 0).sum() + torch.zeros(Ld, device=dev)
        for kind, per_layer in (("loss_ce", loss_ce), ("loss_bbox", l1), ("loss_giou", g), ("loss_mask", loss_mask),
                                ("loss_dice", loss_dice)):
            if weighted:
                per_layer = per_layer * self._layer_weights(kind, names, dev)
            for suffix, term in zip(names, per_layer.unbind(0)):
                out[kind + suffix] = term
        return out

    def _layer_weights(self, kind, names, dev):
        """[Ld] tensor of weight_dict[kind + suffix] (1 where the dict has no entry), cached per device."""
        cache = self.__dict__.setdefault("_lw_cache", {})
        key = (kind, tuple(names), str(dev), tuple(self.weight_dict.get(kind + s, 1.0) for s in names))
        if key not in cache:
            cache[key] = torch.tensor(key[3], dtype=torch.float32, device=dev)
        return cache[key]

    def get_loss(self, loss, outputs, targets, indices, num_boxes, **kw):
        table = {"labels": self.loss_labels, "boxes": self.loss_boxes, "masks": self.loss_masks}
        assert loss in table, f"do you really want to compute {loss} loss?"
        return table[loss](outputs, targets, indices, num_boxes, **kw)

    def forward(self, outputs, targets, indices_list, valid_ratios=None):
        device = outputs["pred_logits"].device
        num_boxes = torch.as_tensor([float(sum(len(t["labels"]) for t in targets))], device=device)
        world = 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(num_boxes)
            world = torch.distributed.get_world_size()
        num_boxes = torch.clamp(num_boxes / world, min=1)[0]
        losses = {}
        for name in self.losses:
            losses.update(self.get_loss(name, outputs, targets, indices_list[-1], num_boxes))
        for i, aux in enumerate(outputs.get("aux_outputs", [])):
            for name in self.losses:
                kw = {"log": False} if name == "labels" else {}
                part = self.get_loss(name, aux, targets, indices_list[i], num_boxes, **kw)
                losses.update({f"{k}_{i}": v for k, v in part.items()})
        return losses
