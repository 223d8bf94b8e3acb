"""YTVIS AP, locally: the YouTube-VIS cocoapi fork's `YTVOS.loadRes` + `YTVOSeval` (reference:
projects/InstMove/MinVIS_motion/minvis/data_video/datasets/ytvis_api/ytvos.py:218-266, ytvoseval.py:88-130, 176-190,
267-345, 347-452, 459-503, 534-545) and the evaluator protocol around it (minvis/data_video/ytvis_eval.py), for the
records `model.ytvis_results(inputs)` returns.

The video mask IoU -- the reference's Python double loop of RLE merges -- is taken as integer sums over run tables
(vnext_amd/ops/video_iou.py: on the device for a CUDA `device`, in numpy otherwise) and is bit-identical to the
reference's; the matching, the accumulation and the summary are restated here in numpy on the host, with the numpy
calls the reference's numbers depend on (`argsort(kind="mergesort")`, `cumsum`, `np.spacing(1)`,
`searchsorted(side="left")`).
"""
from __future__ import annotations

import json
import os
import time
from collections import defaultdict

import numpy as np

from .. import _lib
from ..ops import video_iou as V
from ..ops.poly_rle import polygons_to_runs

STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")
AREA_LABELS = ("all", "small", "medium", "large")


def _default_device():
    try:
        import torch
        return "cuda" if torch.cuda.is_available() and os.path.exists(_lib.LIB_PATH) else None
    except Exception:
        return None


def _avg_area(areas):
    """the reference's `avg_area`: the mean of the non-zero frame areas, 0 if none"""
    l = [a for a in areas if a]
    return np.array(l).mean() if l else 0


class YTVISEval:
    """`YTVISEval(gt).add(records)`, then `.evaluate()` -> the numbers of YTVOSeval.evaluate / accumulate / summarize.

    gt: the annotation JSON (a dict or a path): `videos`, `categories`, `annotations` with per-frame `segmentations`
    (uncompressed RLE, compressed RLE or None), `areas` and `iscrowd`.  polygons: False (the default) = polygon ground
    truth raises ValueError; True = a frame's list segmentation (polygons or boxes, as frPyObjects takes them) is rasterised
    at the video's `height` x `width` by `ops.poly_rle.polygons_to_runs`, on the evaluator's device (the kernel) or on the
    host, and joins the RLE ground truth in one table; `areas` stay what the annotation states.
    device: a CUDA device for the kernels; None = CUDA when this process has one and the library is built, else the
    numpy path; "cpu" = the numpy path.  iou_thrs, rec_thrs, max_dets, area_rng: the reference's Params (defaults: 0.5 :
    0.05 : 0.95, 0 : 0.01 : 1, [1, 10, 100], all / small / medium / large at 128^2 and 256^2).
    device_matching: with a CUDA device, the matching of every (video, category) goes through the kernel of
    ops/ap_match.py (one launch) instead of the Python loop of `_evaluate_vid`; the results are identical.
    """

    def __init__(self, gt, device=None, iou_thrs=None, rec_thrs=None, max_dets=(1, 10, 100), area_rng=None,
                 device_matching=False, polygons=False):
        if isinstance(gt, (str, os.PathLike)):
            with open(gt) as f:
                gt = json.load(f)
        if not isinstance(gt, dict):
            raise ValueError(f"YTVISEval: annotation format {type(gt)} not supported")
        self.gt = gt
        self.polygons = bool(polygons)
        self.device = _default_device() if device is None else (None if str(device) == "cpu" else device)
        self.iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True) if iou_thrs is None \
            else np.asarray(iou_thrs, dtype=np.float64)
        self.rec_thrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True) if rec_thrs is None \
            else np.asarray(rec_thrs, dtype=np.float64)
        self.max_dets = sorted(int(m) for m in max_dets)
        self.area_rng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 128 ** 2], [128 ** 2, 256 ** 2], [256 ** 2, 1e5 ** 2]] \
            if area_rng is None else [list(a) for a in area_rng]
        if len(self.area_rng) != len(AREA_LABELS):
            raise ValueError("YTVISEval: area_rng needs the four ranges all / small / medium / large")
        self.videos = {v["id"]: v for v in gt.get("videos", [])}
        self.categories = {c["id"]: c for c in gt.get("categories", [])}
        self.vid_ids = [v.item() for v in np.unique(list(self.videos))] if self.videos else []
        self.cat_ids = [c.item() for c in np.unique(list(self.categories))] if self.categories else []
        for ann in gt.get("annotations") or []:
            for f, seg in enumerate(ann["segmentations"]):
                if isinstance(seg, list) and seg and not self.polygons:
                    raise ValueError(f"YTVISEval: annotation {ann.get('id')} frame {f} is a polygon; only RLE ground "
                                     "truth is supported")
        self.records = []
        self.device_matching = bool(device_matching) and self.device is not None

    def add(self, records):
        """records: what `model.ytvis_results(inputs)` returns ({"video_id", "score", "category_id", "segmentations"});
        may be called once per video."""
        for r in records:
            if r["video_id"] not in self.videos:
                raise ValueError(f"YTVISEval: record {len(self.records)} names video {r['video_id']!r}, which the "
                                 "annotations do not have")
            self.records.append(r)
        return self

    # ---- masks -> run tables --------------------------------------------------------------------------------------
    def _size_of(self, seg, video, label):
        size = seg.get("size")
        if size is None:
            size = [video["height"], video["width"]]
        size = [int(size[0]), int(size[1])]
        if "height" in video and "width" in video and size != [int(video["height"]), int(video["width"])]:
            raise ValueError(f"YTVISEval: mask-size mismatch: {label} is {size[0]} x {size[1]}, its video "
                             f"{video['height']} x {video['width']}")
        return size

    def _tables(self, tracks):
        """tracks: [(label, video, segmentations[, is ground truth])] -> (tables, frame_mask, track rows); one mask per
        present frame"""
        polys, poly_sizes, poly_slots = [], [], []
        counts, counts_sizes, counts_slots = [], [], []
        strings, string_sizes, string_slots, labels = [], [], [], []
        frame_mask, rows = [], []
        for label, video, segs, *is_gt in tracks:
            rows.append((len(frame_mask), len(segs)))
            for f, seg in enumerate(segs):
                if not seg:
                    frame_mask.append(-1)
                    continue
                where = f"{label} frame {f}"
                if self.polygons and is_gt and is_gt[0] and isinstance(seg, list):
                    if "height" not in video or "width" not in video:
                        raise ValueError(f"YTVISEval: {where} is a polygon and its video states no height / width")
                    polys.append(seg)
                    poly_sizes.append((int(video["height"]), int(video["width"])))
                    poly_slots.append(len(frame_mask))
                    frame_mask.append(0)
                    continue
                size = self._size_of(seg, video, where)
                c = seg["counts"]
                if isinstance(c, (str, bytes)):
                    strings.append(c)
                    string_sizes.append(size)
                    string_slots.append(len(frame_mask))
                    labels.append(where)
                else:
                    counts.append(c)
                    counts_sizes.append(size)
                    counts_slots.append(len(frame_mask))
                frame_mask.append(0)
        frame_mask = np.array(frame_mask, dtype=np.int32).reshape(-1)
        try:
            t_counts = V.runs_from_counts(counts, counts_sizes)
        except ValueError as e:
            raise ValueError(f"YTVISEval: malformed uncompressed RLE in the ground truth: {e}") from None
        t_strings = V.decode_strings(strings, string_sizes, device=self.device, labels=labels)
        if self.device is not None:
            t_counts = t_counts.to(t_strings.rows.device)
        tables = V.concat_tables(t_counts, t_strings)
        frame_mask[counts_slots] = np.arange(len(counts), dtype=np.int32)
        frame_mask[string_slots] = len(counts) + np.arange(len(strings), dtype=np.int32)
        if polys:
            try:
                t_polys = polygons_to_runs(polys, poly_sizes, device=self.device)
            except ValueError as e:
                raise ValueError(f"YTVISEval: malformed polygon ground truth: {e}") from None
            tables = V.concat_tables(tables, t_polys)
            frame_mask[poly_slots] = len(counts) + len(strings) + np.arange(len(polys), dtype=np.int32)
        return tables, frame_mask, np.array(rows, dtype=np.int32).reshape(-1, 2)

    # ---- YTVOSeval.evaluate ---------------------------------------------------------------------------------------
    def evaluate(self):
        """-> {"AP", "AP50", ..., "ARl" (the 12 numbers of `summarize`; -1 where the reference leaves -1), "stats"
        float64 [12], "per_category" {name: AP in percent, as `_derive_coco_results` forms it}, "precision" [T, R, K,
        A, M], "recall" [T, K, A, M], "scores" [T, R, K, A, M], "ious" {(video, category): [D, G] or []}, "eval_vids"
        (the reference's `evalImgs`: one dict or None per (category, area range, video))}."""
        cats = set(self.cat_ids)
        gts, dts = defaultdict(list), defaultdict(list)
        by_video = defaultdict(list)
        for ann in self.gt.get("annotations") or []:
            by_video[ann["video_id"]].append(ann)
        for v in self.vid_ids:
            for ann in by_video.get(v, []):
                if ann["category_id"] in cats:
                    gts[v, ann["category_id"]].append(
                        {"id": ann["id"], "ann": ann, "ignore": bool(ann.get("iscrowd")),
                         "iscrowd": int(ann.get("iscrowd", 0)), "avg_area": _avg_area(ann["areas"])})
        by_video = defaultdict(list)
        for i, r in enumerate(self.records):
            by_video[r["video_id"]].append((i + 1, r))
        for v in self.vid_ids:
            for i, r in by_video.get(v, []):
                if r["category_id"] in cats:
                    dts[v, r["category_id"]].append({"id": i, "rec": r, "score": r["score"]})
        max_det = self.max_dets[-1]
        for key, dt in dts.items():                         # sorted by score (stable), cut to the last maxDets
            inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
            dts[key] = [dt[i] for i in inds][:max_det]
        groups = [(v, c) for v in self.vid_ids for c in self.cat_ids if (v, c) in gts or (v, c) in dts]
        tracks, pairs = [], []
        for key in groups:
            video = self.videos[key[0]]
            for d in dts.get(key, []):
                d["track"] = len(tracks)
                tracks.append((f"record {d['id'] - 1} (video {key[0]!r})", video, d["rec"]["segmentations"]))
            for g in gts.get(key, []):
                g["track"] = len(tracks)
                tracks.append((f"annotation {g['id']!r} (video {key[0]!r})", video, g["ann"]["segmentations"], True))
            pairs += [(d["track"], g["track"]) for d in dts.get(key, []) for g in gts.get(key, [])]
        t0 = time.perf_counter()
        tables, frame_mask, track_rows = self._tables(tracks)
        area = tables.rows[:, 3].cpu().numpy() if tables.is_cuda else tables.rows[:, 3]
        for key in groups:
            for d in dts.get(key, []):
                first, frames = track_rows[d["track"]]
                masks = frame_mask[first:first + frames]
                # loadRes: the areas of the present masks as pycocotools gives them (uint32), None for absent frames
                d["avg_area"] = _avg_area(list(area[masks[masks >= 0]].astype(np.uint32)))
        pairs = np.array(pairs, dtype=np.int32).reshape(-1, 2)
        t1 = time.perf_counter()
        sums = V.pair_sums(tables, frame_mask, track_rows, pairs)
        t2 = time.perf_counter()
        bad = np.flatnonzero(sums[:, 3])
        if len(bad):
            d, g = pairs[bad[0]]
            what = {_lib.VIDEO_IOU_FRAMES: "differ in frame count", _lib.VIDEO_IOU_PIXELS: "have masks of different "
                    "sizes in one frame (mask-size mismatch)"}.get(int(sums[bad[0], 3]), "point outside the run tables")
            raise ValueError(f"YTVISEval: {tracks[d][0]} and {tracks[g][0]} {what}")
        iou = V.ious_from_sums(sums)
        ious, at = {}, 0
        for v in self.vid_ids:
            for c in self.cat_ids:
                D, G = len(dts.get((v, c), [])), len(gts.get((v, c), []))
                if D == 0 and G == 0:
                    ious[v, c] = []
                else:
                    ious[v, c] = iou[at:at + D * G].reshape(D, G).copy()
                    at += D * G
        if self.device_matching:
            eval_vids = self._evaluate_vids_device(groups, gts, dts, iou, max_det)
        else:
            eval_vids = [self._evaluate_vid(gts.get((v, c), []), dts.get((v, c), []), ious[v, c], v, c, a, max_det)
                         for c in self.cat_ids for a in self.area_rng for v in self.vid_ids]
        t3 = time.perf_counter()
        out = self._accumulate(eval_vids)
        # host clock, seconds: run tables (decode included), pair sums (copies included), matching, accumulation
        self.timings = {"tables_s": t1 - t0, "sums_s": t2 - t1, "match_s": t3 - t2, "accumulate_s": time.perf_counter() - t3,
                        "masks": len(tables), "pairs": len(pairs), "device_matching": self.device_matching}
        out["stats"] = self._summarize(out["precision"], out["recall"])
        out.update({n: float(s) for n, s in zip(STAT_NAMES, out["stats"])})
        out["per_category"] = {}
        for k, c in enumerate(self.cat_ids):
            p = out["precision"][:, :, k, 0, -1]
            p = p[p > -1]
            out["per_category"][str(self.categories[c].get("name", c))] = float(np.mean(p) * 100) if p.size \
                else float("nan")
        out["ious"] = ious
        out["eval_vids"] = eval_vids
        return out

    # ---- YTVOSeval.evaluateVid ------------------------------------------------------------------------------------
    def _evaluate_vid(self, gt, dt, ious, vid, cat, rng, max_det):
        if len(gt) == 0 and len(dt) == 0:
            return None
        ig = [1 if (g["ignore"] or (g["avg_area"] < rng[0] or g["avg_area"] > rng[1])) else 0 for g in gt]
        gtind = np.argsort(ig, kind="mergesort")
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in dtind[0:max_det]]
        iscrowd = [g["iscrowd"] for g in gt]
        ious = ious[:, gtind] if len(ious) > 0 else ious
        T, G, D = len(self.iou_thrs), len(gt), len(dt)
        gtm, dtm = np.zeros((T, G)), np.zeros((T, D))
        gt_ig = np.array([ig[i] for i in gtind])
        dt_ig = np.zeros((T, D))
        if not len(ious) == 0:
            rows = ious.tolist()
            for tind, t in enumerate(self.iou_thrs):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    row = rows[dind]
                    for gind in range(G):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:       # matched already, and not a crowd
                            continue
                        if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:   # matched to a regular gt, now on ignored ones
                            break
                        if row[gind] < iou:
                            continue
                        iou = row[gind]
                        m = gind
                    if m == -1:
                        continue
                    dt_ig[tind, dind] = gt_ig[m]
                    dtm[tind, dind] = gt[m]["id"]
                    gtm[tind, m] = d["id"]
        a = np.array([d["avg_area"] < rng[0] or d["avg_area"] > rng[1] for d in dt]).reshape((1, len(dt)))
        dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {"video_id": vid, "category_id": cat, "aRng": rng, "maxDet": max_det,
                "dtIds": [d["id"] for d in dt], "gtIds": [g["id"] for g in gt], "dtMatches": dtm, "gtMatches": gtm,
                "dtScores": [d["score"] for d in dt], "gtIgnore": gt_ig, "dtIgnore": dt_ig}

    def _evaluate_vids_device(self, groups, gts, dts, iou, max_det):
        """`_evaluate_vid` for every (category, area range, video) from one launch of the matching kernel: `groups` in
        the order of the flat IoU array, the detections already in score order and cut to `max_det`."""
        import torch
        from ..ops import ap_match as M
        rows, n_dt, n_gt, n_iou = {}, 0, 0, 0
        for key in groups:
            D, G = len(dts.get(key, [])), len(gts.get(key, []))
            rows[key] = (D, G, n_dt, n_gt, n_iou)
            n_dt, n_gt, n_iou = n_dt + D, n_gt + G, n_iou + D * G
        all_g = [g for key in groups for g in gts.get(key, [])]
        all_d = [d for key in groups for d in dts.get(key, [])]
        dev = torch.device(self.device)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(dev)   # noqa: E731
        table = np.array([rows[key] for key in groups], dtype=np.int64).reshape(-1, 5)
        m = M.ap_match(up(table, np.int64), up(iou, np.float64).reshape(-1), up([g["iscrowd"] for g in all_g], np.uint8),
                       up([g["avg_area"] for g in all_g], np.float64), up([d["avg_area"] for d in all_d], np.float64),
                       up(self.area_rng, np.float64).reshape(-1, 2), up(self.iou_thrs, np.float64)).numpy()
        out = []
        for c in self.cat_ids:
            for a, rng in enumerate(self.area_rng):
                for v in self.vid_ids:
                    if (v, c) not in rows:
                        out.append(None)
                        continue
                    D, G, dof, gof, _ = rows[v, c]
                    gt, dt = gts.get((v, c), []), dts.get((v, c), [])
                    ig = m.gt_ignore[a, gof:gof + G].astype(np.int64)
                    gtind = np.argsort(ig, kind="mergesort")            # the reference's order: ignored last, stable
                    gt_ids = np.array([g["id"] for g in gt], dtype=np.float64)
                    dt_ids = np.array([d["id"] for d in dt], dtype=np.float64)
                    dm, gm = m.dt_match[a, :, dof:dof + D], m.gt_match[a, :, gof:gof + G]
                    dtm = np.where(dm >= 0, gt_ids[np.maximum(dm, 0)], 0.0) if G else np.zeros(dm.shape)
                    gtm = np.where(gm >= 0, dt_ids[np.maximum(gm, 0)], 0.0) if D else np.zeros(gm.shape)
                    outside = np.array([d["avg_area"] < rng[0] or d["avg_area"] > rng[1] for d in dt]).reshape((1, D))
                    dt_ig = np.logical_or(m.dt_ignore[a, :, dof:dof + D] != 0, np.logical_and(dtm == 0, outside))
                    out.append({"video_id": v, "category_id": c, "aRng": rng, "maxDet": max_det,
                                "dtIds": [d["id"] for d in dt], "gtIds": [gt[i]["id"] for i in gtind], "dtMatches": dtm,
                                "gtMatches": gtm[:, gtind], "dtScores": [d["score"] for d in dt], "gtIgnore": ig[gtind],
                                "dtIgnore": dt_ig})
        return out

    # ---- YTVOSeval.accumulate -------------------------------------------------------------------------------------
    def _accumulate(self, eval_vids):
        T, R, K, A, M = len(self.iou_thrs), len(self.rec_thrs), len(self.cat_ids), len(self.area_rng), len(self.max_dets)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        scores = -np.ones((T, R, K, A, M))
        I0 = len(self.vid_ids)
        for k in range(K):
            for a in range(A):
                for m, max_det in enumerate(self.max_dets):
                    E = [e for e in eval_vids[(k * A + a) * I0:(k * A + a + 1) * I0] if e is not None]
                    if len(E) == 0:
                        continue
                    dt_scores = np.concatenate([e["dtScores"][0:max_det] for e in E])
                    inds = np.argsort(-dt_scores, kind="mergesort")
                    sorted_scores = dt_scores[inds]
                    dtm = np.concatenate([e["dtMatches"][:, 0:max_det] for e in E], axis=1)[:, inds]
                    dt_ig = np.concatenate([e["dtIgnore"][:, 0:max_det] for e in E], axis=1)[:, inds]
                    gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                    npig = np.count_nonzero(gt_ig == 0)
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dt_ig))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                    fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        recall[t, k, a, m] = rc[-1] if nd else 0
                        pr = np.maximum.accumulate(pr[::-1])[::-1]      # pr[i - 1] = max(pr[i - 1], pr[i]), from the end
                        at = np.searchsorted(rc, self.rec_thrs, side="left")
                        ok = at < nd                                     # the reference's loop stops at the first miss
                        q, ss = np.zeros((R,)), np.zeros((R,))
                        q[ok] = pr[at[ok]]
                        ss[ok] = sorted_scores[at[ok]]
                        precision[t, :, k, a, m] = q
                        scores[t, :, k, a, m] = ss
        return {"precision": precision, "recall": recall, "scores": scores, "counts": [T, R, K, A, M]}

    # ---- YTVOSeval.summarize --------------------------------------------------------------------------------------
    def _summarize(self, precision, recall):
        return summarize(precision, recall, self.iou_thrs, self.max_dets)


def summarize(precision, recall, iou_thrs, max_dets):
    """The 12 numbers of `summarize` from precision [T, R, K, A, M] and recall [T, K, A, M]; -1 where nothing is defined."""
    def one(ap=1, iou_thr=None, area="all", max_det=100):
        aind = [i for i, lbl in enumerate(AREA_LABELS) if lbl == area]
        mind = [i for i, m in enumerate(max_dets) if m == max_det]
        s = precision if ap == 1 else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == iou_thrs)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
    md = max_dets
    last = md[2] if len(md) > 2 else -1
    stats = np.zeros((12,))
    stats[0] = one(1)
    stats[1] = one(1, iou_thr=.5, max_det=last)
    stats[2] = one(1, iou_thr=.75, max_det=last)
    stats[3] = one(1, area="small", max_det=last)
    stats[4] = one(1, area="medium", max_det=last)
    stats[5] = one(1, area="large", max_det=last)
    stats[6] = one(0, max_det=md[0])
    stats[7] = one(0, max_det=md[1] if len(md) > 1 else -1)
    stats[8] = one(0, max_det=last)
    stats[9] = one(0, area="small", max_det=last)
    stats[10] = one(0, area="medium", max_det=last)
    stats[11] = one(0, area="large", max_det=last)
    return stats


class YTVISEvaluator:
    """The reference evaluators' protocol (`reset()` / `process(inputs, outputs)` / `evaluate()`) around `YTVISEval`,
    without detectron2.

    `outputs` is a model's output dict -- `model.ytvis_results`-style, "pred_masks" holding RLE dicts (through
    `utils.ytvis_json.ytvis_records`), or `model(inputs)` with mask arrays (through `instances_to_coco_json_video`) -- or
    a list of result records.  `evaluate()` returns {"segm": {...}}: the numbers of `summarize` in percent under the
    reference's names (NaN where the reference has -1: `_derive_coco_results`; AR100 / ARs / ARm / ARl beside the
    eight it lists) and "AP-<category>" per category when there is more than one.

    The evaluator scores the records this process has seen.  Gathering records across ranks stays the caller's
    `gather_object` (call `process(None, gathered_records)` on the main rank, or merge the lists before `evaluate`).
    """

    def __init__(self, gt, device=None, **params):
        self._args = (gt, device, params)
        self.reset()

    def reset(self):
        gt, device, params = self._args
        self._eval = YTVISEval(gt, device=device, **params)
        self._args = (self._eval.gt, device, params)            # a path is read once

    def process(self, inputs, outputs):
        from ..utils.ytvis_json import instances_to_coco_json_video, ytvis_records
        if isinstance(outputs, dict):
            first = next((m for track in outputs["pred_masks"] for m in track if m is not None), None)
            outputs = ytvis_records(inputs, outputs) if isinstance(first, dict) \
                else instances_to_coco_json_video(inputs, outputs)
        self._eval.add(outputs)

    def evaluate(self):
        if not self._eval.records:
            return {"segm": {n: float("nan") for n in STAT_NAMES}}
        res = self._eval.evaluate()
        segm = {n: float(res[n] * 100 if res[n] >= 0 else "nan") for n in STAT_NAMES}
        if len(res["per_category"]) > 1:
            segm.update({"AP-" + name: ap for name, ap in res["per_category"].items()})
        self.results = res
        return {"segm": segm}
