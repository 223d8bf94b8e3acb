"""`IDOL` meta-architecture on the MI355X hot path (b).

Registered under the reference's name (projects/IDOL/idol/idol.py:71-72), built as `IDOL(cfg)`,
same `forward(batched_inputs)` I/O: training takes key/reference frame pairs (each item's
"image" / "instances" lists hold 2 frames) and returns the weighted loss dict (:228-232);
inference takes one video and returns {"image_size", "pred_scores", "pred_labels",
"pred_masks"} (:466-471).  Model tree (`detr` = CondInst_segm {`detr` = DeformableDETR {...},
controller, mask_head, reid_embed_head}) and parameter names follow the reference so its
checkpoints load.

Mapping onto the machine (the arithmetic and the decisions are the reference's):
  * key and reference frames go through backbone + transformer in ONE batch of 2*bz frames
    (the reference runs the transformer twice, segmentation_condInst.py:142-143);
  * matching for all decoder layers in one host round-trip (idol_criterion.OTAMatcher);
  * the dynamic mask head of all layers' matched queries in one fused launch (forward and
    backward), mask features computed once instead of once per layer (:157-200);
  * reid losses: one similarity launch per image on the matrix cores (heads.loss_reid);
  * inference: per-frame candidate selection for the whole chunk from one host copy, mask
    head only for the selected queries (the reference evaluates all 300 per frame, :296-318),
    tracker with one mask-IoU matrix and one association matrix per frame (models/tracker.py);
  * COCO pre-training evaluation (INPUT.COCO_PRETRAIN, idol.py:235-248, 488-531): images in, per-image instances out;
    NMS and the top 100 by one kernel for the whole batch (ops/det_select.py), the mask head for the picked queries
    only (`coco_inference`, `coco_postprocess`, `coco_results`).
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from ..heads import dynamic_mask_head, loss_reid
from ..registry import META_ARCH_REGISTRY
from .criterion import box_cxcywh_to_xyxy, box_xyxy_to_cxcywh, flat_pairs, layer_counts
from .idol_criterion import IDOLCriterion, OTAMatcher, reid_terms, reid_terms_fused, sample_aux_masks, select_pos_neg_masks
from .frames import (TrainTrunk, augment_step, front_end, front_end_state, graphed_callable, level_inputs, plan_resize, preprocess,
                     replay_captured, stage_chunk)
from .idol_transformer import DeformableTransformer
from .resnet import build_backbone
from .seqformer import MLP, DeformableDETR, MaskHeadSmallConv, scale_tensor
from .seqformer_transformer import inverse_sigmoid
from .tracker import DeviceTracker, IDOL_Tracker
from ..ops.det_select import DetSelectUnsupported, class_aware_nms, select_detections, select_detections_host  # noqa: F401 (class_aware_nms: the host NMS, re-exported)
from ..ops.mask_dense import masks_from_logits
from ..ops.mask_rle import encode_logits
from ..utils.ytvis_json import rle_encode, ytvis_records

COCO_NMS_THR, COCO_TOPK, VIDEO_NMS_THR = 0.7, 100, 0.9      # idol.py:502, 507, 340


class CondInstSegmIDOL(nn.Module):
    def __init__(self, detr, hidden):
        super().__init__()
        self.detr = detr
        self.controller = MLP(hidden, hidden, 169, 3)
        for layer in self.controller.layers:     # segmentation_condInst.py:68-70
            nn.init.xavier_uniform_(layer.weight)
            nn.init.zeros_(layer.bias)
        self.mask_head = MaskHeadSmallConv(hidden)
        self.reid_embed_head = MLP(hidden, hidden, hidden, 3)


@META_ARCH_REGISTRY.register()
class IDOL(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        m = cfg.MODEL.IDOL
        self.device = torch.device(cfg.MODEL.DEVICE)
        self.num_frames = cfg.INPUT.SAMPLING_FRAME_NUM
        self.num_classes, self.mask_stride = m.NUM_CLASSES, m.MASK_STRIDE
        self.is_multi_cls, self.apply_cls_thres = m.MULTI_CLS_ON, m.APPLY_CLS_THRES
        self.temporal_score_type = m.TEMPORAL_SCORE_TYPE
        self.inference_select_thres = m.INFERENCE_SELECT_THRES
        self.inference_fw, self.inference_tw = m.INFERENCE_FW, m.INFERENCE_TW
        self.memory_len, self.nms_pre, self.add_new_score = m.MEMORY_LEN, m.NMS_PRE, m.ADD_NEW_SCORE
        self.batch_infer_len = m.BATCH_INFER_LEN
        self.coco_pretrain = bool(cfg.INPUT.COCO_PRETRAIN)      # eval mode: image-level `coco_inference` (idol.py:235)
        self.mask_on = bool(cfg.MODEL.MASK_ON)
        hidden = m.HIDDEN_DIM
        transformer = DeformableTransformer(
            d_model=hidden, nhead=m.NHEADS, num_encoder_layers=m.ENC_LAYERS, num_decoder_layers=m.DEC_LAYERS,
            dim_feedforward=m.DIM_FEEDFORWARD, dropout=m.DROPOUT, activation="relu", return_intermediate_dec=True,
            num_frames=self.num_frames, num_feature_levels=m.NUM_FEATURE_LEVELS, dec_n_points=m.DEC_N_POINTS,
            enc_n_points=m.ENC_N_POINTS)
        detr = DeformableDETR(build_backbone(cfg), transformer, m.NUM_CLASSES, self.num_frames, m.NUM_OBJECT_QUERIES,
                              m.NUM_FEATURE_LEVELS, hidden)
        self.detr = CondInstSegmIDOL(detr, hidden)
        weights = {"loss_ce": m.CLASS_WEIGHT, "loss_bbox": m.L1_WEIGHT, "loss_giou": m.GIOU_WEIGHT,
                   "loss_reid": m.REID_WEIGHT, "loss_reid_aux": m.REID_WEIGHT * 1.5,
                   "loss_mask": m.MASK_WEIGHT, "loss_dice": m.DICE_WEIGHT}
        if m.DEEP_SUPERVISION:   # idol.py:183-187
            weights.update({f"{k}_{i}": v for i in range(m.DEC_LAYERS - 1) for k, v in list(weights.items())})
        matcher = OTAMatcher(multi_frame=True, cost_class=m.SET_COST_CLASS, cost_bbox=m.SET_COST_BOX,
                             cost_giou=m.SET_COST_GIOU)
        self.criterion = IDOLCriterion(m.NUM_CLASSES, matcher, weights, ["labels", "boxes", "masks", "reid"],
                                       mask_out_stride=m.MASK_STRIDE, focal_alpha=m.FOCAL_ALPHA,
                                       num_frames=self.num_frames)
        self.deep_supervision = m.DEEP_SUPERVISION
        self.graph_inference = True      # replay the per-chunk inference trunk from a hipGraph
        self.graph_training = False      # capture the training trunk's forward and backward (opt-in: the trunk's gradients then
        #                                  reach DDP's buckets together, at the end of the replayed backward)
        # simOTA matching and the contrastive sets by one kernel (vnext_amd/ops/ota_match.py) instead of on the host
        # (opt-in: train.enable_device_matching); CUDA tensors only, the host matcher otherwise
        self.device_matching = False
        # per-frame candidate selection (score threshold + class-aware NMS) by one kernel for the whole chunk
        # (vnext_amd/ops/det_select.py) instead of the host loop (opt-in: train.enable_device_selection); CUDA tensors only
        self.device_selection = False
        # uint8 frames are uploaded as bytes and normalised, padded and masked by one kernel; the level masks and positions
        # come from one more (vnext_amd/ops/ingest.py; opt-in: train.enable_device_ingest).  Float frames: unchanged
        self.device_ingest = False
        # eval mode, uint8 video frames at their decoded size: ResizeShortestEdge(MIN_SIZE_TEST, MAX_SIZE_TEST) by the kernel
        # that also ingests them, byte for byte Pillow's (vnext_amd/ops/resize.py; opt-in: train.enable_device_resize)
        self.device_resize = False
        # training mode, clips staged by `data.clip_mapper.stage_clip`: crop, resize and flip of the source frames AND of their
        # run-length ground truth on the device (vnext_amd/ops/augment.py; opt-in: train.enable_device_augment)
        self.device_augment = False
        # eval mode, `model(inputs)`: the full-resolution masks of the tracks (and of COCO-pretrain detections) from the logits
        # by one kernel (vnext_amd/ops/mask_dense.py) instead of the bilinear -> sigmoid -> nearest chain (opt-in:
        # train.enable_device_masks); CUDA tensors only
        self.device_masks = False
        self._pixel_stats, self._test_size, self._graphs, self._train_trunks = front_end_state(cfg, 480)
        self.register_buffer("pixel_mean", torch.tensor(cfg.MODEL.PIXEL_MEAN).view(3, 1, 1), persistent=False)
        self.register_buffer("pixel_std", torch.tensor(cfg.MODEL.PIXEL_STD).view(3, 1, 1), persistent=False)
        self.to(self.device)

    # ---- shared trunk -------------------------------------------------------------------------
    def _preprocess(self, frames):
        """normalise + pad to a multiple of 32 (idol.py:473-482, util/misc.py nested tensor) -> (x, mask); with
        `device_ingest` and uint8 frames -> (x, mask, table) from the ingest kernel (`_encode_decode` takes the table)."""
        return preprocess(list(frames), *front_end(self))

    def _encode_decode(self, x, mask, table=None):
        """-> srcs, hs [Ld, N, Q, C], memory [N, S, C], per-layer pre-sigmoid references, the refined references, and the box
        predictions of the decoder's refinement loop (what _box_heads would compute again; None if it used other heads).
        table: the frames' geometry on the device when x, mask came from the ingest kernel (`level_inputs`)"""
        d = self.detr.detr
        feats = d.backbone(x)
        srcs = [d.input_proj[l](f) for l, f in enumerate(feats)]
        for l in range(len(feats), d.num_feature_levels):
            srcs.append(d.input_proj[l](feats[-1] if l == len(feats) else srcs[-1]))
        masks, poss = level_inputs(srcs, mask, table)
        hs, memory, init_ref, inter_refs, _, inter_boxes, _ = d.transformer(srcs, masks, poss, d.query_embed.weight)
        refs = [inverse_sigmoid(init_ref if l == 0 else inter_refs[l - 1]) for l in range(hs.shape[0])]
        if d.transformer.decoder.bbox_embed is not d.bbox_embed:
            inter_boxes = None        # the decoder's loop did not use the detector's box heads: they run in _box_heads
        return srcs, hs, memory, refs, inter_refs, inter_boxes        # inter_boxes [Ld, N, Q, 4] with their graph | None

    def _box_heads(self, hs, refs, layers, loop_boxes=None):
        """Class logits and boxes of the decoder layers `layers`.  loop_boxes [Ld, ...]: the box predictions the decoder's
        refinement loop made with these box heads and references (idol_transformer.py) -- then only the class heads run."""
        d = self.detr.detr
        if loop_boxes is not None:
            layers = list(layers)      # (plain indexing: a list index would copy an index tensor to the device -- not under capture)
            picked = loop_boxes if layers == list(range(loop_boxes.shape[0])) else torch.stack([loop_boxes[l] for l in layers])
            return torch.stack([d.class_embed[l](hs[l]) for l in layers]), picked
        logits, boxes = [], []
        for l in layers:
            tmp = d.bbox_embed[l](hs[l])
            if refs[l].shape[-1] == 4:
                tmp = tmp + refs[l]
            else:
                tmp[..., :2] = tmp[..., :2] + refs[l]
            logits.append(d.class_embed[l](hs[l]))
            boxes.append(tmp.sigmoid())
        return torch.stack(logits), torch.stack(boxes)

    def _mask_features(self, srcs, memory):
        """[N, S, C] memory -> stride-8 mask features [N, 8, H/8, W/8] (forward_mask_head_train :330-345)"""
        mem, start = [], 0
        for s in srcs[:3]:
            h, w = s.shape[-2:]
            mem.append(memory[:, start:start + h * w].reshape(memory.shape[0], h, w, -1).permute(0, 3, 1, 2))
            start += h * w
        return self.detr.mask_head(mem).float().contiguous()

    def _train_trunk(self, x, mask, table=None):
        """Padded frames of the key / reference pairs (key frames at even positions) -> everything `losses` needs from the
        network, as a flat tuple of tensors: query states of every decoder layer [Ld, N, Q, C]; class logits and boxes of every
        layer on the KEY frames; the layers' pre-sigmoid reference xy on the key frames [Ld, bz, Q, 2]; the last layer's
        refined references on the REFERENCE frames; the key frames' stride-8 mask features; the reference frames' class logits
        (last layer); the reid embeddings of all frames."""
        srcs, hs, memory, refs, inter_refs, inter_boxes = self._encode_decode(x, mask, table)
        loop_boxes = None if inter_boxes is None else inter_boxes[:, 0::2]
        logits, boxes = self._box_heads(hs[:, 0::2], [r[0::2] for r in refs], range(hs.shape[0]), loop_boxes)
        feats = self._mask_features([s[0::2] for s in srcs], memory[0::2])
        ref_xy = torch.stack([r[0::2, :, :2] for r in refs])
        ref_logits = self.detr.detr.class_embed[-1](hs[-1, 1::2])
        embeds = self.detr.reid_embed_head(hs[-1])
        return hs, logits, boxes, ref_xy, inter_refs[-1, 1::2], feats, ref_logits, embeds

    def _graphed_train_trunk(self, stack):
        """Forward + backward hipGraphs of `_train_trunk` for this batch shape (and autocast dtype), captured on first use
        (`torch.cuda.make_graphed_callables`: eager warm-up iterations on a side stream, then capture).  Under torch.autocast
        the capture runs with autocast's weight cache OFF: a cast cached before the capture would be a tensor outside the
        graph's memory pool."""
        return graphed_callable(self._train_trunks, lambda: TrainTrunk(self).train(), stack)

    # ---- training -----------------------------------------------------------------------------
    def prepare_targets(self, batched_inputs):
        """-> (det_targets, ref_targets): key / reference frame of every pair (idol.py:283-311)."""
        def field(o, k):
            v = o[k] if isinstance(o, dict) else getattr(o, k)
            return getattr(v, "tensor", v)
        per_frame = []
        for video in batched_inputs:
            for fr in video["instances"]:
                h, w = field(fr, "image_size")
                scale = scale_tensor([w, h, w, h], self.device)
                ids = field(fr, "gt_ids").to(self.device)
                per_frame.append({"labels": field(fr, "gt_classes").to(self.device),
                                  "boxes": box_xyxy_to_cxcywh(field(fr, "gt_boxes").to(self.device, torch.float32) / scale),
                                  "masks": field(fr, "gt_masks").to(self.device), "inst_id": ids, "valid": ids != -1})
        det, ref = per_frame[0::2], per_frame[1::2]
        for d_t, r_t in zip(det, ref):     # objects absent from the key frame are dropped from both
            if not bool(d_t["valid"].all()):
                keep = d_t["valid"].clone()
                for t in (d_t, r_t):
                    for k in list(t):
                        t[k] = t[k][keep]
        return det, ref

    def losses(self, batched_inputs):
        """CondInst_segm.forward (segmentation_condInst.py:78-231) + SetCriterion."""
        batched_inputs, pre = augment_step(self, batched_inputs)      # `device_augment`: pre = (x, mask, table), else None
        det_t, ref_t = self.prepare_targets(batched_inputs)
        frames = [f for video in batched_inputs for f in video["image"]]
        sizes = [tuple(f.shape[-2:]) for f in frames][0::2]
        if pre is not None:      # the frames are still the sources: the network saw their targets
            sizes = [tuple(fr["image_size"]) for video in batched_inputs for fr in video["instances"]][0::2]
            hs, logits, boxes, ref_xy, ref_last, feats, ref_logits, embeds = self._train_trunk(*pre)
        elif self.graph_training and frames[0].is_cuda and all(f.shape == frames[0].shape for f in frames):
            hs, logits, boxes, ref_xy, ref_last, feats, ref_logits, embeds = self._graphed_train_trunk(
                torch.stack([f.to(self.device, torch.float32) for f in frames]))
        else:
            hs, logits, boxes, ref_xy, ref_last, feats, ref_logits, embeds = self._train_trunk(*self._preprocess(frames))
        Ld, bz = hs.shape[0], len(det_t)
        pos_neg = None
        if self.device_matching and logits.is_cuda:
            indices_list, matched, pos_neg = self.criterion.matcher.match_all_layers_device(
                logits, boxes, det_t, ref=(ref_last, ref_logits.detach().sigmoid(), ref_t))
        else:
            indices_list, matched = self.criterion.matcher.match_all_layers(logits, boxes, det_t)
        # the selected queries of every decoder layer on every key frame: one gather, one controller
        # call, one mask-head launch
        counts = layer_counts(indices_list)
        match = flat_pairs(indices_list, [len(t["labels"]) for t in det_t], self.device, non_blocking=True)
        lay, img, qry = match.lay, match.clip, match.qry          # the one pair list: these rows are the criterion's rows
        key_hs = hs[:, 0::2]                                                            # [Ld, bz, Q, C]
        scale = torch.stack([scale_tensor([sizes[i][1], sizes[i][0]], self.device) for i in range(bz)])   # [bz, (w, h)]
        params = self.detr.controller(key_hs[lay, img, qry])
        points = ref_xy[lay, img, qry].sigmoid() * scale[img]
        masks = dynamic_mask_head(feats, points.float(), params.float(), img.to(torch.int32), 8)
        if masks.shape[0] == 0:  # nothing matched: keep the mask branch in the autograd graph
            masks = masks + 0 * (feats.sum() + sum(p.sum() for p in self.detr.controller.parameters()))
        masks = masks[:, None]                                                          # [n, 1, H/4, W/4]
        # contrastive sets on the reference frames (last decoder layer), embeddings of both frames
        if pos_neg is None:
            selections = select_pos_neg_masks(ref_last, ref_logits.sigmoid(), ref_t)
        else:                    # matched on the device above: the sampling loop alone
            selections = sample_aux_masks(pos_neg)
        if self.criterion.fused_reid_loss and embeds.is_cuda:     # both reid losses of all images from one op
            qd = reid_terms_fused(embeds[0::2], embeds[1::2], matched, selections)
        else:
            qd = reid_terms(embeds[0::2], embeds[1::2], matched, selections, loss_reid)
        if self.deep_supervision:   # every decoder layer's losses in one pass over stacked tensors
            loss = self.criterion.forward_all_layers(logits, boxes, masks, det_t, match, qd, counts=counts)
        else:
            n_last = counts[-1]
            outputs = {"pred_logits": logits[-1], "pred_boxes": boxes[-1], "pred_masks": masks[masks.shape[0] - n_last:],
                       "pred_qd": qd}
            loss = self.criterion(outputs, det_t, ref_t, indices_list)
        if qd["count"] == 0:     # keep the reid head in the graph (static DDP graph)
            loss["loss_reid"] = loss["loss_reid"] + embeds.sum() * 0
        w = self.criterion.weight_dict
        return {k: v * w[k] if k in w else v for k, v in loss.items()}

    def forward(self, batched_inputs):
        if self.training:
            return self.losses(batched_inputs)
        if self.coco_pretrain:
            return self.coco_inference(batched_inputs)
        return self.inference_video(batched_inputs)

    @torch.no_grad()
    def ytvis_results(self, batched_inputs):
        """One video -> its YTVIS result records {"video_id", "score", "category_id", "segmentations"}: the records of
        `instances_to_coco_json_video(batched_inputs, self(batched_inputs))`, with the masks encoded from the tracks'
        logits on the device (`_track_masks`, vnext_amd/ops/mask_rle.py) instead of copied to the host as bool masks."""
        return ytvis_records(batched_inputs, self.inference_video(batched_inputs, rle=True))

    # ---- inference ----------------------------------------------------------------------------
    @torch.no_grad()
    def select_candidates(self, logits, boxes):
        """logits [F, Q, K], boxes [F, Q, 4] -> per frame the query indices that enter the tracker
        (idol.py:331-343): best class score above INFERENCE_SELECT_THRES (the top-1 query if none),
        then class-aware box NMS at 0.9; one host copy for the whole chunk.  With `device_selection` and CUDA tensors the
        selection itself runs on the device (ops/det_select.py) and only the picked indices cross; a shape the kernel
        refuses takes the host loop."""
        if self.device_selection and logits.is_cuda:
            try:
                return list(select_detections(logits, boxes, iou_thr=VIDEO_NMS_THR,
                                              score_thr=self.inference_select_thres).kept)
            except DetSelectUnsupported:
                pass
        best, label = logits.sigmoid().max(-1)
        host = torch.cat([best[..., None], label[..., None].to(best.dtype), box_cxcywh_to_xyxy(boxes)], -1).cpu().numpy()
        picks = []
        for f in range(host.shape[0]):
            score, cls, bx = host[f, :, 0], host[f, :, 1].astype(np.int64), host[f, :, 2:]
            cand = np.nonzero(score > self.inference_select_thres)[0]
            if len(cand) == 0:
                cand = np.array([int(np.argmax(score))])
            else:
                cand = cand[class_aware_nms(bx[cand], score[cand], cls[cand], VIDEO_NMS_THR)]
            picks.append(cand)
        return picks

    # ---- COCO pre-training evaluation ------------------------------------------------------------
    @torch.no_grad()
    def _coco_trunk(self, batched_inputs):
        """-> logits, boxes, a `masks_of(image, queries)` callable (None with MASK_ON false), image sizes, output sizes"""
        images = [x["image"] for x in batched_inputs]      # (`_preprocess` uploads them: as floats, or as bytes for the kernel)
        image_sizes = [tuple(int(v) for v in im.shape[-2:]) for im in images]
        out_sizes = [(int(x.get("height", s[0])), int(x.get("width", s[1]))) for x, s in zip(batched_inputs, image_sizes)]
        logits, boxes, hs_last, ref_last, feats = self._chunk_trunk(*self._preprocess(images))
        scale = torch.stack([scale_tensor([w, h], self.device) for h, w in image_sizes])      # [B, (w, h)]: each image's own

        def masks_of(image, queries):
            """image, queries int64 [n] on the device -> mask logits [n, H/4, W/4] of those queries"""
            sel_hs = hs_last[image, queries]
            points = ref_last[image, queries, :2].sigmoid() * scale[image]
            return dynamic_mask_head(feats, points.float(), self.detr.controller(sel_hs).float(), image.to(torch.int32), 8)
        return logits, boxes, masks_of if self.mask_on else None, image_sizes, out_sizes

    @torch.no_grad()
    def _coco_select(self, logits, boxes, masks_of, image_sizes, out_sizes):
        """The part of `coco_inference` + `segmentation_postprocess` before the masks are formed: per image the output
        boxes, scores, classes of the rows with a non-empty box, and (with masks) the stride-4 mask logits of those rows."""
        try:
            sel = select_detections(logits, boxes, iou_thr=COCO_NMS_THR, topk=COCO_TOPK)
        except DetSelectUnsupported:      # more queries or classes than the kernel holds: the host expression
            sel = select_detections_host(logits, boxes, iou_thr=COCO_NMS_THR, topk=COCO_TOPK)
        dev = logits.device
        counts = [len(p) for p in sel.topk]
        image = torch.from_numpy(np.repeat(np.arange(len(counts)), counts)).to(dev)
        pairs = torch.from_numpy(np.concatenate(sel.topk).reshape(-1, 2)).to(dev)
        query, cls = pairs[:, 0], pairs[:, 1]
        scores = logits[image, query, cls].sigmoid()                      # = prob[keep].view(-1)[topk]
        xyxy = box_cxcywh_to_xyxy(boxes[image, query].float())
        mask_logits = None
        if masks_of is not None:     # the mask head once, for the distinct picked queries of all images
            flat = image * logits.shape[1] + query
            uniq, inverse = torch.unique(flat, return_inverse=True)
            mask_logits = masks_of(torch.div(uniq, logits.shape[1], rounding_mode="floor"), uniq % logits.shape[1])[inverse]
        out, start = [], 0
        for b, n in enumerate(counts):
            sl = slice(start, start + n)
            start += n
            (ih, iw), (oh, ow) = image_sizes[b], out_sizes[b]
            bx = xyxy[sl] * scale_tensor([iw, ih, iw, ih], dev)           # Boxes.scale(image size)
            sx, sy = ow / iw, oh / ih
            bx = bx * scale_tensor([sx, sy, sx, sy], dev)                 # segmentation_postprocess: scale, clip, drop empty
            bx = torch.stack([bx[:, 0].clamp(0, ow), bx[:, 1].clamp(0, oh), bx[:, 2].clamp(0, ow), bx[:, 3].clamp(0, oh)], 1)
            keep = ((bx[:, 2] - bx[:, 0]) > 0) & ((bx[:, 3] - bx[:, 1]) > 0)
            out.append({"pred_boxes": bx[keep], "scores": scores[sl][keep], "pred_classes": cls[sl][keep],
                        "mask_logits": None if mask_logits is None else mask_logits[sl][keep]})
        return out

    @torch.no_grad()
    def coco_postprocess(self, logits, boxes, masks_of, image_sizes, out_sizes):
        """`coco_inference` (idol.py:488-531) + `segmentation_postprocess` (segmentation_condInst.py:748-788) on network
        outputs: logits [B, Q, K], boxes [B, Q, 4] (cxcywh), `masks_of(image, queries) -> [n, H/4, W/4]` mask logits of
        the named queries (None: no masks), the images' sizes (h, w) before padding and the sizes to report at.
        -> per image {"instances": {"image_size", "pred_boxes" [n, 4], "scores", "pred_classes", "pred_masks" uint8
        [n, height, width]}}: plain tensors under the reference's field names.  Selection: ops/det_select.py (the
        kernel for CUDA tensors; the host expression for a shape it refuses).  Masks: bilinear x4, sigmoid > 0.5, crop to the image, nearest to the output size.
        `device_masks` (CUDA tensors): the masks come from ops/mask_dense.py, one call per distinct (image size, output
        size) as in `coco_records`; no full-resolution float is formed."""
        results = []
        selected = self._coco_select(logits, boxes, masks_of, image_sizes, out_sizes)
        dense = self._coco_device_masks(selected, image_sizes, out_sizes) if self.device_masks and logits.is_cuda else {}
        for b, r in enumerate(selected):
            inst = {"image_size": tuple(out_sizes[b]), "pred_boxes": r["pred_boxes"], "scores": r["scores"],
                    "pred_classes": r["pred_classes"]}
            if b in dense:
                inst["pred_masks"] = dense[b]
            elif r["mask_logits"] is not None:
                m = r["mask_logits"][:, None].float()
                h, w = m.shape[-2:]
                ih, iw = image_sizes[b]
                if m.shape[0]:
                    m = F.interpolate(m, size=(h * 4, w * 4), mode="bilinear", align_corners=False).sigmoid() > 0.5
                    m = F.interpolate(m[:, :, :ih, :iw].float(), size=tuple(out_sizes[b]), mode="nearest")[:, 0]
                else:
                    m = m.new_zeros((0,) + tuple(out_sizes[b]))
                inst["pred_masks"] = m.to(torch.uint8)
            results.append({"instances": inst})
        return results

    @staticmethod
    def _coco_device_masks(selected, image_sizes, out_sizes):
        """`_coco_select`'s rows -> {image: uint8 [n, height, width] on the device}, the masks of the stride-4 logits by one
        kernel call per distinct (image size, output size); an image without detections keeps the host expression's empty."""
        groups = {}
        for b, r in enumerate(selected):
            if r["mask_logits"] is not None and r["mask_logits"].shape[0]:
                groups.setdefault((tuple(image_sizes[b]), tuple(out_sizes[b])), []).append(b)
        dense = {}
        for (isz, osz), members in groups.items():
            parts = [selected[b]["mask_logits"] for b in members]
            masks = masks_from_logits(parts[0] if len(parts) == 1 else torch.cat(parts), 4, isz, osz).view(torch.uint8)
            start = 0
            for b, p in zip(members, parts):
                dense[b] = masks[start:start + p.shape[0]]
                start += p.shape[0]
        return dense

    @torch.no_grad()
    def coco_inference(self, batched_inputs):
        """Eval mode with INPUT.COCO_PRETRAIN (idol.py:235-248): [{"image": [3, h, w], "height", "width"}, ...], one dict
        per image (sizes may differ) -> [{"instances": {...}}, ...] as `coco_postprocess` forms them.  The mask head runs
        once, for the distinct picked queries of all images (the reference runs it for all Q)."""
        return self.coco_postprocess(*self._coco_trunk(batched_inputs))

    @torch.no_grad()
    def coco_results(self, batched_inputs):
        """Images -> their COCO result records {"image_id", "category_id", "bbox" (xywh), "score", "segmentation" (RLE)}:
        the counterpart of `ytvis_results`.  The RLE strings are encoded from the mask logits on the device
        (ops/mask_rle.py), one call per distinct (image size, output size); no full-resolution mask is formed."""
        logits, boxes, masks_of, image_sizes, out_sizes = self._coco_trunk(batched_inputs)
        return self.coco_records(batched_inputs, self._coco_select(logits, boxes, masks_of, image_sizes, out_sizes),
                                 image_sizes, out_sizes)

    @staticmethod
    def coco_records(batched_inputs, selected, image_sizes, out_sizes):
        """`_coco_select`'s rows -> COCO result records, the masks as RLE of the stride-4 logits"""
        rles = [None] * len(selected)
        groups = {}
        for b, r in enumerate(selected):
            if r["mask_logits"] is not None:
                groups.setdefault((tuple(image_sizes[b]), tuple(out_sizes[b])), []).append(b)
        for (isz, osz), members in groups.items():
            strings = encode_logits(torch.cat([selected[b]["mask_logits"] for b in members]), 4, isz, osz)
            start = 0
            for b in members:
                n = selected[b]["mask_logits"].shape[0]
                rles[b] = strings[start:start + n]
                start += n
        records = []
        for b, (x, r) in enumerate(zip(batched_inputs, selected)):
            bx = r["pred_boxes"].cpu()
            xywh = torch.stack([bx[:, 0], bx[:, 1], bx[:, 2] - bx[:, 0], bx[:, 3] - bx[:, 1]], 1).tolist()
            for i, (score, label) in enumerate(zip(r["scores"].tolist(), r["pred_classes"].tolist())):
                rec = {"image_id": x.get("image_id", b), "category_id": int(label), "bbox": xywh[i], "score": float(score)}
                if rles[b] is not None:
                    rec["segmentation"] = rles[b][i]
                records.append(rec)
        return records

    def _chunk_trunk(self, x, mask, table=None):
        """Padded frames -> (logits [F,Q,K], boxes [F,Q,4], query states, pre-sigmoid reference of the
        last decoder layer, stride-8 mask features): the shape-static, sync-free part of inference."""
        srcs, hs, memory, refs, _, inter_boxes = self._encode_decode(x, mask, table)
        last = hs.shape[0] - 1
        logits, boxes = self._box_heads(hs, refs, [last], inter_boxes)
        return logits[0], boxes[0], hs[last], refs[last], self._mask_features(srcs, memory)

    @torch.no_grad()
    def inference_forward(self, frames, rz=None):
        """One chunk of frames -> per-frame candidates (inference_forward :234-321 + the selection of
        idol.py:331-349): list over frames of dicts {indices, logits [n,K], boxes [n,4], embeds
        [n,C], masks [n,1,H/4,W/4]} for the queries that survive the score threshold and the
        class-aware box NMS (0.9).
        rz = (targets, layout) (`device_resize`): the frames are uint8 sources, resized to their targets by the ingest."""
        frames = list(frames)
        staged = stage_chunk(frames, rz, *front_end(self))
        if staged is None:      # frames of different sizes: the eager, padded-batch path
            logits, boxes, hs_last, ref_last, feats = self._chunk_trunk(*self._preprocess(frames))
        elif self.graph_inference and staged.tensors[0].is_cuda:      # one hipGraph per chunk shape and input kind
            logits, boxes, hs_last, ref_last, feats = replay_captured(
                self._graphs, staged.key, staged.tensors, lambda *t: self._chunk_trunk(*staged.to_net(*t)))
        else:
            logits, boxes, hs_last, ref_last, feats = self._chunk_trunk(*staged.to_net(*staged.tensors))
        picks = self.select_candidates(logits, boxes)
        frame_of = torch.from_numpy(np.concatenate([np.full(len(c), f) for f, c in enumerate(picks)])).to(self.device)
        query = torch.from_numpy(np.concatenate(picks)).to(self.device)
        sel_hs = hs_last[frame_of, query]
        ih, iw = frames[0].shape[-2:] if rz is None else rz[0][0]
        scale = scale_tensor([iw, ih], self.device)
        points = ref_last[frame_of, query, :2].sigmoid() * scale              # = inter_references[-2][..., :2]
        masks = dynamic_mask_head(feats, points.float(), self.detr.controller(sel_hs).float(),
                                  frame_of.to(torch.int32), 8)
        embeds = self.detr.reid_embed_head(sel_hs)
        out, start = [], 0
        for f, c in enumerate(picks):
            sl = slice(start, start + len(c))
            out.append({"indices": c.tolist(), "logits": logits[f, query[sl]], "boxes": boxes[f, query[sl]],
                        "embeds": embeds[sl], "masks": masks[sl][:, None]})
            start += len(c)
        return out

    @torch.no_grad()
    def inference_video(self, batched_inputs, rle=False):
        """idol.py:236-281: chunks of BATCH_INFER_LEN frames through the network, then the tracker."""
        video, rz, src_size = plan_resize(self.device_resize and not self.training, batched_inputs[0], self._test_size,
                                          self.device)
        per_frame = []
        for s in range(0, len(video), self.batch_infer_len):
            e = s + self.batch_infer_len
            per_frame.extend(self.inference_forward(video[s:e]) if rz is None else
                             self.inference_forward(video[s:e], (rz[0][s:e], rz[1])))
        args = dict(init_score_thr=0.2, obj_score_thr=0.1, nms_thr_pre=self.nms_pre, nms_thr_post=0.05,
                    addnew_score_thr=self.add_new_score, memo_tracklet_frames=10, memo_momentum=0.8,
                    long_match=self.inference_tw, frame_weight=(self.inference_tw | self.inference_fw),
                    temporal_weight=self.inference_tw, memory_len=self.memory_len)
        most = max((len(fr["indices"]) for fr in per_frame), default=0)
        on_device = self.device.type == "cuda" and DeviceTracker.supports(memory_len=self.memory_len, max_dets=most)
        tracker = (DeviceTracker if on_device else IDOL_Tracker)(**args)
        ih, iw = video[0].shape[-2:] if rz is None else rz[0][0]      # the size the network sees: with `device_resize` the target
        sh, sw = (ih, iw) if src_size is None else src_size
        oh, ow = batched_inputs[0].get("height", sh), batched_inputs[0].get("width", sw)
        return self.associate(per_frame, tracker, (oh, ow), (ih, iw), host_factory=lambda: IDOL_Tracker(**args), rle=rle)

    @staticmethod
    def _track_masks(tracks, n_frames, image_size, ori_size, rle=False, device_masks=False):
        """The final mask step of `associate`: each track's remembered stride-4 logits [1, H/4, W/4] (None where the
        track is absent) -> per track, a list over frames of bool masks of `ori_size` on the host (None where absent) or,
        with `rle`, of their COCO RLE dicts (the empty mask's RLE where absent, as the YTVIS writer puts it).  The RLE
        form encodes the seen frames of ALL tracks in one device call; no full-resolution mask is formed.
        `device_masks` (the model's switch; CUDA logits, `rle=False`): the bool masks of the seen frames of ALL tracks come
        from one kernel call (vnext_amd/ops/mask_dense.py) and one copy to the host, instead of one chain and one copy
        per track; a track's masks are rows of that one host tensor."""
        seen = [[i for i, m in enumerate(v["masks"]) if m is not None] for v in tracks]
        logits = [v["masks"][i][0] for v, idx in zip(tracks, seen) for i in idx] if device_masks and not rle else []
        if logits and logits[0].is_cuda:
            m = torch.stack(logits)                                                   # [sum k, H/4, W/4]
            rows = iter(masks_from_logits(m, 4, image_size, ori_size).cpu())
            masks_out = []
            for idx in seen:
                per = [None] * n_frames
                for i in idx:
                    per[i] = next(rows)
                masks_out.append(per)
            return masks_out
        if rle:
            out = []
            if tracks:
                m = torch.cat([torch.stack([v["masks"][i] for i in idx]) for v, idx in zip(tracks, seen)])[:, 0]
                strings = iter(encode_logits(m, 4, image_size, ori_size))
                empty = rle_encode(np.zeros(tuple(ori_size), dtype=np.uint8))
                for idx in seen:
                    per = [empty] * n_frames
                    for i in idx:
                        per[i] = next(strings)
                    out.append(per)
            return out
        masks_out = []
        for v, idx in zip(tracks, seen):
            m = torch.stack([v["masks"][i] for i in idx])                         # [k, 1, H/4, W/4]: one pass per track
            h, w = m.shape[-2:]
            m = F.interpolate(m, size=(h * 4, w * 4), mode="bilinear", align_corners=False).sigmoid()
            m = (F.interpolate(m[:, :, :image_size[0], :image_size[1]], size=ori_size, mode="nearest") > 0.5)[:, 0].cpu()
            per = [None] * n_frames
            for j, i in enumerate(idx):
                per[i] = m[j]
            masks_out.append(per)
        return masks_out

    @torch.no_grad()
    def associate(self, per_frame, tracker, ori_size, image_size, host_factory=None, rle=False):
        """IDOL.inference (idol.py:313-471) on the pre-selected candidates of every frame.

        With a `DeviceTracker` the association of the whole video is enqueued without a host round trip:
        every frame leaves its ids in device memory, they are read ONCE after the last frame, and the
        per-track bookkeeping (which only needs the ids) runs on that copy.  With the host-side
        `IDOL_Tracker` (CPU, differential tests) the ids arrive frame by frame, as in the reference.

        The device tracker has fixed limits (slots alive at a time, detections per frame, memory_len): a video that
        outgrows its slots is associated AGAIN by `host_factory()` (the host-side tracker, no limits) instead of
        being lost -- a tracklet that found no slot is never remembered, so the device ids up to that point may
        already differ from the reference's and are discarded as a whole.

        `rle=True`: "pred_masks" holds each track's COCO RLE dicts instead of bool masks (`_track_masks`)."""
        n_frames = len(per_frame)
        on_device = isinstance(tracker, DeviceTracker)
        probs, frame_ids = [], []
        for t, fr in enumerate(per_frame):
            prob = fr["logits"].sigmoid()
            score, label = prob.max(1)
            det = torch.cat([fr["boxes"], score[:, None]], 1)
            probs.append(prob)
            if on_device:
                frame_ids.append(tracker.match_device(det, label, fr["masks"], fr["embeds"], t))
            else:
                _, _, ids, kept = tracker.match(bboxes=det, labels=label, masks=fr["masks"], track_feats=fr["embeds"],
                                                frame_id=t, indices=list(range(len(fr["indices"]))))
                full = torch.full((det.shape[0],), -3, dtype=torch.long)
                full[torch.tensor(kept, dtype=torch.long)] = ids
                frame_ids.append(full)
        if on_device and frame_ids:
            sizes = [len(x) for x in frame_ids]
            frame_ids = list(torch.cat(frame_ids).cpu().split(sizes))      # the one copy of the video
            if tracker.counters()[1]:
                if host_factory is None:
                    raise RuntimeError("DeviceTracker: more simultaneous tracklets than slots; raise `capacity`")
                return self.associate(per_frame, host_factory(), ori_size, image_size, rle=rle)
        video = {}
        for t, (fr, ids) in enumerate(zip(per_frame, frame_ids)):
            for row, k in enumerate(ids.tolist()):
                if k < 0:
                    continue
                v = video.setdefault(k, {"masks": [None] * t, "scores": [None] * t, "valid": 0})
                v["masks"].append(fr["masks"][row])
                v["scores"].append(probs[t][row])
                v["valid"] += 1
            for v in video.values():
                if len(v["masks"]) < t + 1:
                    v["masks"].append(None)
                    v["scores"].append(None)
            if t > 8:      # drop short noisy sequences (:386-393)
                for k in [k for k, v in video.items() if v["masks"][-1] is None and v["masks"][-2] is None and v["valid"] < 3]:
                    video.pop(k)
        cls = []
        for v in video.values():
            s = torch.stack([x for x in v["scores"] if x is not None])
            cls.append(s.mean(0) if self.temporal_score_type == "mean" else s.max(0)[0])
        masks_out = self._track_masks(list(video.values()), n_frames, image_size, ori_size, rle, self.device_masks)
        if not cls:
            return {"image_size": ori_size, "pred_scores": [], "pred_labels": [], "pred_masks": []}
        cls = torch.stack(cls)
        if self.is_multi_cls:
            who, label = torch.where(cls > self.apply_cls_thres)
            score, masks_out = cls[who, label], [masks_out[i] for i in who.tolist()]
        else:
            score, label = cls.max(-1)
        return {"image_size": ori_size, "pred_scores": score.tolist(), "pred_labels": label.tolist(),
                "pred_masks": masks_out}
