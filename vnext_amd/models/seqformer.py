"""`SeqFormer` meta-architecture on the MI355X hot path (b).

Registered under the reference's name on the META_ARCH_REGISTRY surface
(projects/SeqFormer/seqformer/seqformer.py:74-75) with the same construction contract
`SeqFormer(cfg)` and the same `forward(batched_inputs)` I/O: a list of dicts with an "image"
list of T frames each; eval returns {"image_size", "pred_scores", "pred_labels", "pred_masks"}
(:403-408), training returns a dict of already-weighted losses (:221-225).

What is inside follows the reference's model tree (`detr` = CondInst_segm {`detr` =
DeformableDETR {transformer, class_embed, bbox_embed, query_embed, input_proj, backbone},
controller, mask_head}) where the hot path lives; what SURVEY section 2 marks out
of scope is deliberately thin:
  * backbone: a plain-PyTorch ResNet-50 trunk (convolutions run on MIOpen), frozen BN;
  * training loss: the reference's objective (vnext_amd/models/criterion.py: clip-level
    Hungarian matching, focal / L1 / GIoU / mask focal + dice with deep supervision), with the
    dynamic mask head of ALL decoder layers' matched instances on ALL frames in one fused
    forward launch and one fused backward launch (the reference: 6 layers x T frames x
    [MaskHeadSmallConv + repeat/cat + 3 grouped convs + pads/interpolate], and their autograd
    twins).  Clips without annotations ("instances" absent) train on an empty target set.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import nn

from ..heads import dynamic_mask_head, dynamic_mask_with_coords
from ..ops.ingest import sine_position  # noqa: F401  (its home; importable from here by name, as the three below)
from ..ops.mask_dense import masks_from_logits
from ..ops.mask_rle import encode_logits
from ..utils.ytvis_json import ytvis_records
from .criterion import HungarianMatcher, SetCriterion, box_xyxy_to_cxcywh, flat_pairs, layer_counts
from ..registry import META_ARCH_REGISTRY
from .frames import (TrainTrunk, augment_step, front_end, front_end_state, graphed_callable, level_inputs, plan_resize, preprocess,
                     replay_captured, stage_chunk, takes_bytes)
from .resnet import FrozenBatchNorm2d, ResNet50Trunk, build_backbone, conv_bn  # noqa: F401
from .seqformer_transformer import DeformableTransformer, inverse_sigmoid


_SCALES = {}


def scale_tensor(values, device):
    """A small constant tensor (image width / height factors) on `device`, built once per value
    and reused: `torch.tensor([...], device=cuda)` is a synchronous pageable host->device copy
    (~0.4 ms on this box) and the training step made ~20 of them."""
    key = (tuple(float(v) for v in values), str(device))
    t = _SCALES.get(key)
    if t is None:
        if len(_SCALES) > 256:
            _SCALES.clear()
        t = _SCALES[key] = torch.tensor(key[0], dtype=torch.float32, device=device)
    return t


class MLP(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        h = [hidden_dim] * (num_layers - 1)
        self.layers = nn.ModuleList(nn.Linear(n, k) for n, k in zip([input_dim] + h, h + [output_dim]))

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            x = F.relu(layer(x)) if i < len(self.layers) - 1 else layer(x)
        return x


class MaskHeadSmallConv(nn.Module):
    """segmentation_condInst.py:504-575 (fpns=None path): 3x3 convs on the stride-8/16/32 encoder
    memories, fused top-down at stride 8, down to 8 mask-feature channels."""

    def __init__(self, dim):
        super().__init__()
        self.lay1 = nn.Conv2d(dim, dim // 4, 3, padding=1)
        self.lay2 = nn.Conv2d(dim // 4, dim // 32, 3, padding=1)
        self.lay3 = nn.Conv2d(dim, dim // 4, 3, padding=1)
        self.lay4 = nn.Conv2d(dim, dim // 4, 3, padding=1)
        self.dcn = nn.Conv2d(dim // 4, dim // 4, 3, padding=1)

    def forward(self, feats):
        fused = F.relu(self.lay3(feats[-1]))
        fused = F.relu(self.lay4(feats[-2])) + F.interpolate(fused, size=feats[-2].shape[-2:], mode="nearest")
        fused = F.relu(self.lay1(feats[-3])) + F.interpolate(fused, size=feats[-3].shape[-2:], mode="nearest")
        return self.lay2(F.relu(self.dcn(fused)))


class DeformableDETR(nn.Module):
    def __init__(self, backbone, transformer, num_classes, num_frames, num_queries, num_feature_levels, hidden):
        super().__init__()
        self.backbone = backbone
        self.transformer = transformer
        self.num_frames, self.num_queries, self.num_feature_levels = num_frames, num_queries, num_feature_levels
        nd = transformer.decoder.num_layers
        self.class_embed = nn.ModuleList([nn.Linear(hidden, num_classes) for _ in range(nd)])
        self.bbox_embed = nn.ModuleList([MLP(hidden, hidden, 4, 3) for _ in range(nd)])
        self.query_embed = nn.Embedding(num_queries, hidden * 2)
        proj = [nn.Sequential(nn.Conv2d(c, hidden, 1), nn.GroupNorm(32, hidden)) for c in backbone.num_channels]
        cin = backbone.num_channels[-1]
        for _ in range(num_feature_levels - len(proj)):  # deformable_detr.py:66-76
            proj.append(nn.Sequential(nn.Conv2d(cin, hidden, 3, 2, 1), nn.GroupNorm(32, hidden)))
            cin = hidden
        self.input_proj = nn.ModuleList(proj)
        bias_value = -math.log((1 - 0.01) / 0.01)
        for ce in self.class_embed:
            ce.bias.data.fill_(bias_value)
        for be in self.bbox_embed:
            nn.init.constant_(be.layers[-1].weight.data, 0)
            nn.init.constant_(be.layers[-1].bias.data, 0)
        nn.init.constant_(self.bbox_embed[0].layers[-1].bias.data[2:], -2.0)
        self.transformer.decoder.bbox_embed = self.bbox_embed   # iterative box refinement (:95-103)


class CondInstSegm(nn.Module):
    def __init__(self, detr, hidden):
        super().__init__()
        self.detr = detr
        self.controller = MLP(hidden, hidden, 169, 3)
        self.mask_head = MaskHeadSmallConv(hidden)


@META_ARCH_REGISTRY.register()
class SeqFormer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        m = cfg.MODEL.SeqFormer
        self.device = torch.device(cfg.MODEL.DEVICE)
        self.num_frames = cfg.INPUT.SAMPLING_FRAME_NUM
        self.num_classes = m.NUM_CLASSES
        self.mask_stride = m.MASK_STRIDE
        hidden = m.HIDDEN_DIM
        transformer = DeformableTransformer(
            d_model=hidden, nhead=m.NHEADS, num_encoder_layers=m.ENC_LAYERS, num_decoder_layers=m.DEC_LAYERS,
            dim_feedforward=m.DIM_FEEDFORWARD, dropout=m.DROPOUT, activation="relu", return_intermediate_dec=True,
            num_frames=self.num_frames, num_feature_levels=m.NUM_FEATURE_LEVELS, dec_n_points=m.DEC_N_POINTS,
            enc_n_points=m.ENC_N_POINTS)
        detr = DeformableDETR(build_backbone(cfg), transformer, m.NUM_CLASSES, self.num_frames, m.NUM_OBJECT_QUERIES,
                              m.NUM_FEATURE_LEVELS, hidden)
        self.detr = CondInstSegm(detr, hidden)
        weights = {"loss_ce": m.CLASS_WEIGHT, "loss_bbox": m.L1_WEIGHT, "loss_giou": m.GIOU_WEIGHT,
                   "loss_mask": m.MASK_WEIGHT, "loss_dice": m.DICE_WEIGHT}
        if m.DEEP_SUPERVISION:   # seqformer.py:183-187
            weights.update({f"{k}_{i}": v for i in range(m.DEC_LAYERS - 1) for k, v in list(weights.items())})
        matcher = HungarianMatcher(multi_frame=True, cost_class=m.SET_COST_CLASS, cost_bbox=m.SET_COST_BOX,
                                   cost_giou=m.SET_COST_GIOU)
        self.criterion = SetCriterion(m.NUM_CLASSES, matcher, weights, ["labels", "boxes", "masks"],
                                      mask_out_stride=m.MASK_STRIDE, focal_alpha=m.FOCAL_ALPHA,
                                      num_frames=self.num_frames)
        self.deep_supervision = m.DEEP_SUPERVISION
        self.multi_cls, self.cls_thres = m.MULTI_CLS_ON, m.APPLY_CLS_THRES
        self.clip_matching, self.clip_length, self.clip_stride = m.CLIP_MATCHING, m.CLIP_LENGTH, m.CLIP_STRIDE
        self.graph_inference = True     # replay the inference trunk from a hipGraph (per clip shape)
        self.graph_training = False     # capture the training trunk's forward and backward (opt-in)
        self.device_matching = False    # match queries to targets on the device: no host round trip in `losses` (opt-in)
        self.device_clip_matching = False     # CLIP_MATCHING inference: link the clips on the device, no host copy per clip (opt-in)
        # uint8 frames are uploaded as bytes and normalised, padded and masked by one kernel; the level masks and positions
        # come from one more (vnext_amd/ops/ingest.py; opt-in: train.enable_device_ingest).  Float frames: unchanged
        self.device_ingest = False
        # eval mode, uint8 frames at their decoded size: ResizeShortestEdge(MIN_SIZE_TEST, MAX_SIZE_TEST) by the kernel that
        # also ingests them, byte for byte Pillow's (vnext_amd/ops/resize.py; opt-in: train.enable_device_resize)
        self.device_resize = False
        # training mode, clips staged by `data.clip_mapper.stage_clip`: crop, resize and flip of the source frames AND of their
        # run-length ground truth on the device (vnext_amd/ops/augment.py; opt-in: train.enable_device_augment)
        self.device_augment = False
        # eval mode, `model(inputs)`: the full-resolution bool masks from the logits by one kernel (vnext_amd/ops/mask_dense.py)
        # instead of the bilinear -> sigmoid -> nearest chain (opt-in: train.enable_device_masks); CUDA tensors only
        self.device_masks = False
        self._pixel_stats, self._test_size, self._graphs, self._train_trunks = front_end_state(cfg, 360)
        self.register_buffer("pixel_mean", torch.tensor(cfg.MODEL.PIXEL_MEAN).view(3, 1, 1), persistent=False)
        self.register_buffer("pixel_std", torch.tensor(cfg.MODEL.PIXEL_STD).view(3, 1, 1), persistent=False)
        self.to(self.device)

    # ---- shared trunk -------------------------------------------------------------------------
    def _preprocess(self, batched_inputs):
        """normalise + pad to a multiple of 32 (seqformer.py:413-429, util/misc.py:298-302) -> (x, mask); with
        `device_ingest` and uint8 frames -> (x, mask, table) from the ingest kernel (`_features` takes the table)."""
        return preprocess([f for clip in batched_inputs for f in clip["image"]], *front_end(self))

    def _features(self, x, mask, table=None):
        """table: the frames' geometry on the device when x, mask came from the ingest kernel (`level_inputs`)"""
        d = self.detr.detr
        T = self.num_frames
        N = x.shape[0] // T
        feats = d.backbone(x)
        srcs = []
        for l, f in enumerate(feats):
            srcs.append(d.input_proj[l](f))
        for l in range(len(feats), d.num_feature_levels):
            srcs.append(d.input_proj[l](feats[-1] if l == len(feats) else srcs[-1]))
        masks, poss = level_inputs(srcs, mask, table)
        fold = lambda t: t.reshape(N, T, *t.shape[1:])  # noqa: E731
        return [fold(s) for s in srcs], [fold(mk) for mk in masks], [fold(p) for p in poss]

    def _heads(self, hs, hs_box, init_reference, inter_references, inter_boxes=None):
        """Class logits [Ld, N, Q, K] and boxes [Ld, N, T, Q, 4] of every decoder layer (deformable_detr.py:195-213).
        inter_boxes: the box predictions the decoder's refinement loop already made with these same box heads and
        references (seqformer_transformer.py) -- then only the class heads run here."""
        d = self.detr.detr
        if inter_boxes is not None and d.transformer.decoder.bbox_embed is d.bbox_embed:
            return torch.stack([d.class_embed[lvl](h) for lvl, h in enumerate(hs.unbind(0))]), inter_boxes
        classes, coords = [], []
        for lvl, (h, h_box) in enumerate(zip(hs.unbind(0), hs_box.unbind(0))):   # unbind: ONE stack in the backward
            reference = init_reference if lvl == 0 else inter_references[lvl - 1]
            reference = inverse_sigmoid(reference)
            classes.append(d.class_embed[lvl](h))
            tmp = d.bbox_embed[lvl](h_box)
            if reference.shape[-1] == 4:
                tmp = tmp + reference
            else:
                tmp[..., :2] = tmp[..., :2] + reference
            coords.append(tmp.sigmoid())
        return torch.stack(classes), torch.stack(coords)

    def _run(self, batched_inputs, want_refs=False, pre=None):
        """pre: (x, mask, table) the front end already made (`device_augment`)"""
        pre = self._preprocess(batched_inputs) if pre is None else pre
        x = pre[0]
        srcs, masks, poss = self._features(*pre)
        hs, hs_box, memory, init_ref, inter_refs, inter_boxes, _, _ = self.detr.detr.transformer(
            srcs, masks, poss, self.detr.detr.query_embed.weight)
        logits, boxes = self._heads(hs, hs_box, init_ref, inter_refs, inter_boxes)
        if want_refs:  # the (pre-sigmoid) reference each decoder layer refined, [N, T, Q, 2 or 4]
            refs = [inverse_sigmoid(init_ref if l == 0 else inter_refs[l - 1]) for l in range(hs.shape[0])]
            return x, srcs, hs, memory, logits, boxes, refs
        return x, srcs, hs, memory, logits, boxes

    # ---- training -----------------------------------------------------------------------------
    def prepare_targets(self, batched_inputs):
        """Clip-level targets (seqformer.py:268-299).  A clip's "instances" is a list over frames
        of objects with gt_classes [n], gt_boxes (xyxy pixels; `.tensor` or a tensor), gt_masks
        (`.tensor` or a tensor) [n, H, W], gt_ids [n] (-1 = not visible) and image_size (h, w) --
        detectron2 `Instances` or anything with those attributes / keys."""
        def field(o, k):
            v = o[k] if isinstance(o, dict) else getattr(o, k)
            return getattr(v, "tensor", v)
        targets = []
        for clip in batched_inputs:
            frames = clip.get("instances")
            if not frames:
                h, w = clip["image"][0].shape[-2:]
                T = len(clip["image"])
                targets.append({"labels": torch.zeros(0, dtype=torch.int64, device=self.device),
                                "boxes": torch.zeros(0, T, 4, device=self.device),
                                "masks": torch.zeros(0, T, h, w, dtype=torch.bool, device=self.device),
                                "size": torch.as_tensor([h, w], dtype=torch.long)})     # host: only the host reads it
                continue
            boxes, masks, classes = [], [], []
            for fr in frames:
                h, w = field(fr, "image_size")
                scale = scale_tensor([w, h, w, h], self.device)
                boxes.append(box_xyxy_to_cxcywh(field(fr, "gt_boxes").to(self.device, torch.float32) / scale))
                masks.append(field(fr, "gt_masks").to(self.device))
                classes.append(field(fr, "gt_classes").to(self.device) * (field(fr, "gt_ids").to(self.device) != -1))
            targets.append({"labels": torch.stack(classes, 0).max(0)[0], "boxes": torch.stack(boxes, 1),
                            "masks": torch.stack(masks, 1),
                            "size": torch.as_tensor([h, w], dtype=torch.long)})
        return targets

    def _mask_features(self, srcs, memory):
        """[N, T, S, C] encoder memory -> stride-8 mask features of every frame [N*T, 8, H/8, W/8]
        (forward_mask_head_train's per-frame MaskHeadSmallConv calls, batched over N*T and run
        ONCE instead of once per decoder layer)."""
        N, T = memory.shape[:2]
        mem, start = [], 0
        for s in srcs[:3]:
            h, w = s.shape[-2:]
            mem.append(memory[:, :, start:start + h * w].reshape(N * T, h, w, -1).permute(0, 3, 1, 2))
            start += h * w
        return self.detr.mask_head(mem).float().contiguous()

    def _train_trunk(self, x, mask):
        """Padded frames -> what `losses` needs from the network, as a flat tuple of tensors: the shape-static, sync-free
        part of a training step (`frames.TrainTrunk` captures it)."""
        srcs, masks, poss = self._features(x, mask)
        d = self.detr.detr
        hs, hs_box, memory, init_ref, inter_refs, inter_boxes, _, _ = d.transformer(srcs, masks, poss, d.query_embed.weight)
        logits, boxes = self._heads(hs, hs_box, init_ref, inter_refs, inter_boxes)
        return (hs, logits, boxes, inverse_sigmoid(init_ref), inverse_sigmoid(inter_refs),
                self._mask_features(srcs, memory))

    def _graphed_train_trunk(self, stack):
        """Forward + backward hipGraphs of the training trunk for this clip batch shape, captured
        on first use (3 eager warm-up iterations on a side stream, then capture -- what
        make_graphed_callables does)."""
        return graphed_callable(self._train_trunks, lambda: TrainTrunk(self).train(), stack)

    def losses(self, batched_inputs):
        """CondInst_segm.forward (segmentation_condInst.py:69-207) + SetCriterion."""
        batched_inputs, pre = augment_step(self, batched_inputs)      # `device_augment`: pre = (x, mask, table), else None
        targets = self.prepare_targets(batched_inputs)
        frames = [f for clip in batched_inputs for f in clip["image"]]
        if pre is None and self.graph_training and frames[0].is_cuda and all(f.shape == frames[0].shape for f in frames):
            hs, logits, boxes, ref0, ref_rest, feats = self._graphed_train_trunk(
                torch.stack([f.to(self.device, torch.float32) for f in frames]))
            refs = [ref0] + list(ref_rest[:hs.shape[0] - 1])
        else:
            x, srcs, hs, memory, logits, boxes, refs = self._run(batched_inputs, want_refs=True, pre=pre)
            feats = self._mask_features(srcs, memory)
        return self._losses_after_trunk(targets, hs, logits, boxes, refs, feats)

    def _losses_after_trunk(self, targets, hs, logits, boxes, refs, feats):
        """Matching, the matched instances' masks and the criterion.  With `device_matching` nothing here copies to the
        host or uploads (tests/test_device_matching.py runs it under torch's sync-debug mode)."""
        Ld, N, T = boxes.shape[:3]
        if self.device_matching and self.deep_supervision and logits.is_cuda:
            # cost + assignment of every (layer, clip) in one kernel; the indices stay on the device
            match = self.criterion.matcher.match_all_layers_device(logits, boxes, targets)
        else:
            indices_list = self.criterion.matcher.match_all_layers(logits, boxes, targets)
            match = flat_pairs(indices_list, [len(t["labels"]) for t in targets], self.device)
        lay, clip, qry = match.lay, match.clip, match.qry         # the one pair list: these rows are the criterion's rows
        # the matched instances of every decoder layer, on every frame of their clip: one gather, one
        # controller call, one mask-head launch (the reference: a Python loop over layers x clips x frames)
        params = self.detr.controller(hs[lay, clip, qry])                         # [Ld*n, 169]
        ref_xy = torch.stack([r[..., :2] for r in refs])                          # [Ld, N, T, Q, 2] pre-sigmoid
        sizes = torch.stack([scale_tensor(t["size"].flip(0).tolist(), self.device) for t in targets])   # [N, (w, h)]
        points = ref_xy[lay, clip, :, qry].sigmoid() * sizes[clip][:, None, :]    # [Ld*n, T, 2] image pixels
        image = (clip * T)[:, None] + torch.arange(T, device=self.device)[None, :]
        params = params[:, None].expand(-1, T, -1).flatten(0, 1)                   # [(l, i, inst, t), 169]
        points = points.flatten(0, 1)
        image = image.flatten().to(torch.int32)
        masks = dynamic_mask_head(feats, points.float(), params.float(), image, 8)  # [sum, H/4, W/4]
        masks = masks.view(-1, T, *masks.shape[-2:])
        if masks.shape[0] == 0:  # nothing matched anywhere: keep the mask branch in the autograd graph
            masks = masks + 0 * (feats.sum() + sum(p.sum() for p in self.detr.controller.parameters()))
        if self.deep_supervision:   # every decoder layer's losses in one pass over stacked tensors
            return self.criterion.forward_all_layers(logits, boxes, masks, targets, match, weighted=True)
        else:                       # (matched on the host: the device matching is for deep supervision only)
            n_last = layer_counts(indices_list)[-1]
            outputs = {"pred_logits": logits[-1], "pred_boxes": boxes[-1], "pred_masks": masks[masks.shape[0] - n_last:]}
            loss = self.criterion(outputs, targets, indices_list)
        w = self.criterion.weight_dict
        return {k: v * w[k] if k in w else v for k, v in loss.items()}

    # ---- the two branches -----------------------------------------------------------------------
    def forward(self, batched_inputs):
        if self.training:
            return self.losses(batched_inputs)
        return self.inference(batched_inputs)

    # ---- inference --------------------------------------------------------------------------
    def _clip_trunk_tail(self, x, mask, table=None):
        """Padded frames of ONE clip -> what `inference` needs from the network: class
        logits and (pre-sigmoid) reference of the last decoder layer, its query states and the
        stride-8 mask features.  Shape-static and free of host synchronisation, so it can be
        captured into a hipGraph; boxes of the other layers are not computed (whole-video
        inference never reads them, seqformer.py:351-410)."""
        srcs, masks, poss = self._features(x, mask, table)
        d = self.detr.detr
        hs, _, memory, init_ref, inter_refs, _, _, _ = d.transformer(srcs, masks, poss, d.query_embed.weight)
        last = hs.shape[0] - 1
        ref = inverse_sigmoid(init_ref if last == 0 else inter_refs[last - 1])
        return d.class_embed[last](hs[last]), ref, hs[last], self._mask_features(srcs, memory)

    def _top_instances(self, frames, rz=None):
        """Frames of one clip (any length; the reference sets `num_frames` to it, seqformer.py:231,249)
        -> class probabilities [10, K] of the 10 best queries and their mask logits
        [10, T, H/4, W/4] at a quarter of the padded input size (`inference_clip`, :302-326).
        rz = (targets, layout) (`device_resize`): the frames are uint8 sources, resized to their targets by the ingest."""
        T = len(frames)
        keep, self.num_frames = self.num_frames, T
        try:
            staged = stage_chunk(frames, rz, *front_end(self))
            if staged is None:      # frames of different sizes: the general (eager, padded-batch) path
                x, srcs, hs, memory, logits_all, _, refs = self._run([{"image": frames}], want_refs=True)
                logits, ref_last, hs_last, feats = logits_all[-1], refs[-1], hs[-1], self._mask_features(srcs, memory)
            elif self.graph_inference and staged.tensors[0].is_cuda:      # one hipGraph per clip shape and input kind
                logits, ref_last, hs_last, feats = replay_captured(
                    self._graphs, staged.key, staged.tensors, lambda *t: self._clip_trunk_tail(*staged.to_net(*t)))
            else:
                logits, ref_last, hs_last, feats = self._clip_trunk_tail(*staged.to_net(*staged.tensors))
        finally:
            self.num_frames = keep
        ih, iw = frames[0].shape[-2:] if rz is None else rz[0][0]             # size fed to the network
        prob = logits[0].sigmoid()                                            # [Q, classes]
        query = prob.max(1)[0].topk(min(10, prob.shape[0]))[1]
        params = self.detr.controller(hs_last[0, query])                     # [10, 169]
        scale = scale_tensor([iw, ih], self.device)
        ref = ref_last[0][:, query, :2].sigmoid() * scale                     # [T, 10, 2] image pixels
        n = len(query)
        logits_m = dynamic_mask_with_coords(feats, ref.reshape(1, T * n, 2).float(),
                                            params.float().repeat(T, 1)[None], [n] * T, 8)
        return prob[query], logits_m.view(T, n, *logits_m.shape[-2:]).transpose(0, 1)

    def _report(self, prob, mask_logits, image_size, out_size, rle=False):
        """class probabilities [n, K] + mask logits [n, T, H/4, W/4] -> the output dict
        (`whole_video_inference` :351-410 == `clip_matching_postprocess` :328-349).  `rle=True`: "pred_masks" holds
        each reported pair's T COCO RLE dicts instead of bool masks; every query is encoded once, on the device
        (vnext_amd/ops/mask_rle.py), and a query reported under several classes shares its strings.
        `device_masks` (CUDA tensors, `rle=False`): the bool masks [T, oh, ow] of the distinct reported queries come from
        one kernel call (vnext_amd/ops/mask_dense.py) and cross to the host in one copy; the pairs of one query, reported
        under several classes, are then views of the SAME memory (without the switch each pair owns a copy)."""
        if prob.shape[0] == 0:
            return {"image_size": out_size, "pred_scores": [], "pred_labels": [], "pred_masks": []}
        if self.multi_cls:
            who, label = torch.where(prob > self.cls_thres)
            score = prob[who, label]
        else:
            score, label = prob.max(-1)
            who = None
        if rle or (self.device_masks and mask_logits.is_cuda):
            n, T, h, w = mask_logits.shape
            rows = list(range(n)) if who is None else who.tolist()
            used = sorted(set(rows))
            at = {q: j for j, q in enumerate(used)}
            picked = mask_logits[used].reshape(len(used) * T, h, w)
            if rle:
                strings = encode_logits(picked, self.mask_stride, image_size, out_size)
                masks = [strings[at[q] * T:(at[q] + 1) * T] for q in rows]
            else:
                host = masks_from_logits(picked, self.mask_stride, image_size, out_size).cpu()
                masks = [host[at[q] * T:(at[q] + 1) * T] for q in rows]
        else:
            h, w = mask_logits.shape[-2:]
            masks = F.interpolate(mask_logits, size=(h * self.mask_stride, w * self.mask_stride), mode="bilinear",
                                  align_corners=False).sigmoid()
            if who is not None:
                masks = masks[who]
            masks = F.interpolate(masks[:, :, :image_size[0], :image_size[1]], size=out_size, mode="nearest") > 0.5
            masks = [m for m in masks.cpu()]
        return {"image_size": out_size, "pred_scores": score.tolist(), "pred_labels": label.tolist(),
                "pred_masks": masks}

    @torch.no_grad()
    def ytvis_results(self, batched_inputs):
        """One video -> its YTVIS result records {"video_id", "score", "category_id", "segmentations"}: the records of
        `instances_to_coco_json_video(batched_inputs, self(batched_inputs))`, with the masks encoded from the logits on
        the device (`_report(rle=True)`) instead of copied to the host as bool masks."""
        return ytvis_records(batched_inputs, self.inference(batched_inputs, rle=True))

    def _linked_clips(self, frames, on_device, rz=None):
        """CLIP_MATCHING: the video's overlapping clips, linked into tracks -> (class probabilities [N, K], mask logits
        [N, L, H/4, W/4]).  `on_device`: through `DeviceVideos`, whose per-clip call copies nothing to the host (and
        needs neither `prob.max(-1)` nor the sigmoid copy a `Clips` object makes)."""
        from types import SimpleNamespace
        from .clip_matching import Clips, DeviceVideos, Videos
        n_frames, merged, clips = len(frames), None, []
        for start in range(0, n_frames, self.clip_stride):
            end, last = start + self.clip_length, False
            if end >= n_frames:
                start, end, last = max(0, n_frames - self.clip_length), n_frames, True
            clips.append(list(range(start, end)))
            if last:
                break
        for idx in clips:
            clip = [frames[i] for i in idx]
            prob, mask_logits = (self._top_instances(clip) if rz is None else
                                 self._top_instances(clip, ([rz[0][i] for i in idx], rz[1])))
            if merged is None and on_device:      # the clip count bounds the tracks the state needs room for
                merged = DeviceVideos(self.clip_length, n_frames, self.num_classes, mask_logits.shape[-2:], self.device,
                                      max_instances=prob.shape[0], num_clips=len(clips))
            elif merged is None:
                merged = Videos(self.clip_length, n_frames, self.num_classes, mask_logits.shape[-2:], self.device)
            if on_device:
                merged.update_logits(idx, prob, mask_logits)
            else:
                score, label = prob.max(-1)
                merged.update(Clips(idx, SimpleNamespace(pred_classes=label, scores=score, cls_probs=prob,
                                                         pred_masks=mask_logits)))
        return merged.get_result()

    @torch.no_grad()
    def inference(self, batched_inputs, rle=False):
        """One video (seqformer.py:227-264).  Default: the whole video as one clip -- the 10 queries
        with the best class score, their masks on every frame, every (query, class) pair above
        APPLY_CLS_THRES reported (the reference runs the mask head for all 300 queries of all 6 decoder
        layers and keeps 10 of the last).  With CLIP_MATCHING: overlapping clips of CLIP_LENGTH frames
        every CLIP_STRIDE, linked by mask sIoU (vnext_amd/models/clip_matching.py), tracks averaged."""
        assert len(batched_inputs) == 1
        video = batched_inputs[0]
        frames, rz, src_size = plan_resize(self.device_resize and not self.training, video, self._test_size, self.device)
        if rz is None and not takes_bytes(frames, self.device_ingest, self.device):      # uint8 frames stay bytes until the kernel
            frames = [f.to(self.device, torch.float32) for f in frames]
        ih, iw = frames[0].shape[-2:] if rz is None else rz[0][0]      # the size the network sees: with `device_resize` the target
        sh, sw = (ih, iw) if src_size is None else src_size
        out_size = (video.get("height", sh), video.get("width", sw))
        if not self.clip_matching:
            prob, mask_logits = self._top_instances(frames) if rz is None else self._top_instances(frames, rz)
            return self._report(prob, mask_logits, (ih, iw), out_size, rle)
        if self.device_clip_matching and (frames[0].is_cuda or (frames[0].dtype == torch.uint8 and self.device.type == "cuda")):
            from ..ops.clip_link import ClipLinkUnsupported
            try:
                cls, mask_logits = self._linked_clips(frames, on_device=True, rz=rz)
            except ClipLinkUnsupported:      # a clip beyond the kernels' limits, or more tracks than the state holds
                cls, mask_logits = self._linked_clips(frames, on_device=False, rz=rz)
        else:
            cls, mask_logits = self._linked_clips(frames, on_device=False, rz=rz)
        return self._report(cls, mask_logits, (ih, iw), out_size, rle)
