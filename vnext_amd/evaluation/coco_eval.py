"""COCO AP (bbox, segm), locally: `COCO.loadRes` + `COCOeval.evaluate / accumulate / summarize` for the records
`IDOL.coco_results(images)` returns, and the `COCOEvaluator` protocol of the reference's COCO-pretrain stage
(detectron2/evaluation/coco_evaluation.py) around it, without pycocotools or detectron2.

It is the arithmetic of `YTVISEval` (ytvis_eval.py, restated from the YouTube-VIS cocoapi fork) on one-frame
"videos", with what COCO adds: the unit is the image; `area` (the annotation's for ground truth; w * h of a result box
for "bbox", the mask's pixel count for "segm", whatever `bbox` a record carries) takes the place of `avg_area`; the
box IoU; the crowd IoU, whose union is the detection's area alone; area ranges at 32^2 and 96^2.

IoU, in float64: box  w = min(dx + dw, gx + gw) - max(dx, gx), h likewise, 0 if w <= 0 or h <= 0, else i = w * h and
u = crowd ? d_area : d_area + g_area - i;  mask  i = the intersection's pixel count (ops/video_iou.pair_sums with one
frame per track: the kernel for a CUDA device, numpy otherwise), u = crowd ? area(dt) : area(dt) + area(gt) - i.  The
quotient is one IEEE double division on the host, 0 where u is 0, so both routes give the same bits.

The state is flat: detections and ground truths sorted by (category, image) -- detections by score inside a group
(stable) and cut to the last `max_dets` -- and one row {D, G, offsets} per (image, category) that has either.  The
matching is ops/ap_match.py: the kernel for a CUDA device (one launch), `match_vectorised` without one, `match_host`
(plain Python, the readable form) for device="cpu".  The accumulation slices a category's detections out of the flat
arrays; no step of the matching or the accumulation loops over images, detections or ground truths in Python.
"""
from __future__ import annotations

import json
import os
import time
from collections.abc import Mapping

import numpy as np

from .. import _lib
from ..ops import ap_match as M
from ..ops import video_iou as V
from ..ops.poly_rle import polygons_to_runs
from .ytvis_eval import AREA_LABELS, STAT_NAMES, _default_device, summarize

MATCHING = ("device", "vectorised", "host")


class _Ious(Mapping):
    """`COCOeval.ious`: {(image, category): float64 [D, G], or [] where the pair has neither} over the flat array."""

    def __init__(self, img_ids, cat_ids, keys, table, flat):
        self._imgs = {v: i for i, v in enumerate(img_ids)}
        self._cats = {c: k for k, c in enumerate(cat_ids)}
        self._img_ids, self._cat_ids, self._keys, self._table, self._flat = img_ids, cat_ids, keys, table, flat

    def __getitem__(self, key):
        i, k = self._imgs[key[0]], self._cats[key[1]]
        want = k * len(self._img_ids) + i
        p = int(np.searchsorted(self._keys, want))
        if p == len(self._keys) or self._keys[p] != want:
            return []
        D, G, _, _, off = self._table[p].tolist()
        return self._flat[off:off + D * G].reshape(D, G).copy()

    def __iter__(self):
        return ((v, c) for v in self._img_ids for c in self._cat_ids)

    def __len__(self):
        return len(self._img_ids) * len(self._cat_ids)


def _group_offsets(D):
    D = np.asarray(D, dtype=np.int64)
    return np.cumsum(D) - D


def _within(counts):
    """[3, 2] -> [0, 1, 2, 0, 1]"""
    counts = np.asarray(counts, dtype=np.int64)
    return np.arange(int(counts.sum()), dtype=np.int64) - np.repeat(_group_offsets(counts), counts)


class COCOEval:
    """`COCOEval(gt, iou_type).add(records)`, then `.evaluate()` -> the numbers of COCOeval.evaluate / accumulate /
    summarize.

    gt: the annotation JSON (a dict or a path): `images`, `categories`, `annotations` with `bbox` (xywh), `area`,
    `iscrowd` and, for "segm", `segmentation` as an RLE dict (compressed or not).  polygons: False (the default) = a
    polygon segmentation raises ValueError; True = a list segmentation (polygons or boxes, as frPyObjects takes them) is
    rasterised at its image's `height` x `width` by `ops.poly_rle.polygons_to_runs`, on the evaluator's device (the
    kernel) or on the host, and joins the RLE ground truth in one table.  `area` stays what the annotation states (COCO's
    polygon areas differ from pixel counts, and COCOeval uses the stated one); "bbox" ignores the segmentation.
    iou_type: "bbox" or "segm".  device: a CUDA device for the kernels; None = CUDA when this process has one and the
    library is built; "cpu" = numpy and `match_host`.  matching: "device" / "vectorised" / "host" overrides the route of
    the matching alone.  iou_thrs, rec_thrs, max_dets, area_rng: COCOeval's Params (0.5 : 0.05 : 0.95, 0 : 0.01 : 1,
    [1, 10, 100], all / small / medium / large at 32^2 and 96^2).
    """

    def __init__(self, gt, iou_type, device=None, iou_thrs=None, rec_thrs=None, max_dets=(1, 10, 100), area_rng=None,
                 matching=None, polygons=False):
        if isinstance(gt, (str, os.PathLike)):
            with open(gt) as f:
                gt = json.load(f)
        if not isinstance(gt, dict):
            raise ValueError(f"COCOEval: annotation format {type(gt)} not supported")
        if iou_type not in ("bbox", "segm"):
            raise ValueError(f"COCOEval: iou_type {iou_type!r} (bbox or segm; keypoints are out of scope)")
        self.gt, self.iou_type = gt, iou_type
        self.polygons = bool(polygons)
        self.device = _default_device() if device is None else (None if str(device) == "cpu" else device)
        if matching is None:
            matching = "device" if self.device is not None else "host" if device is not None else "vectorised"
        if matching not in MATCHING or (matching == "device" and self.device is None):
            raise ValueError(f"COCOEval: matching {matching!r} (one of {MATCHING}; 'device' needs a CUDA device)")
        self.matching = matching
        self.iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True) if iou_thrs is None \
            else np.asarray(iou_thrs, dtype=np.float64)
        self.rec_thrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True) if rec_thrs is None \
            else np.asarray(rec_thrs, dtype=np.float64)
        self.max_dets = sorted(int(m) for m in max_dets)
        self.area_rng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]] \
            if area_rng is None else [list(a) for a in area_rng]
        if len(self.area_rng) != len(AREA_LABELS):
            raise ValueError("COCOEval: area_rng needs the four ranges all / small / medium / large")
        self.images = {v["id"]: v for v in gt.get("images", [])}
        self.categories = {c["id"]: c for c in gt.get("categories", [])}
        self.img_ids = [v.item() for v in np.unique(list(self.images))] if self.images else []
        self.cat_ids = [c.item() for c in np.unique(list(self.categories))] if self.categories else []
        for ann in gt.get("annotations") or []:
            seg = ann.get("segmentation")
            if isinstance(seg, list) and seg:
                if not self.polygons:
                    raise ValueError(f"COCOEval: annotation {ann.get('id')} is a polygon; only RLE ground truth is supported")
                continue
            if iou_type == "segm" and not isinstance(seg, dict):
                raise ValueError(f"COCOEval: annotation {ann.get('id')} has no RLE segmentation")
        self.records = []

    def add(self, records):
        """records: what `IDOL.coco_results(images)` returns ({"image_id", "category_id", "score", "bbox" xywh and / or
        "segmentation" RLE}); may be called once per batch.  Ids are index + 1 in the order added."""
        need = "bbox" if self.iou_type == "bbox" else "segmentation"
        for r in records:
            if r["image_id"] not in self.images:
                raise ValueError(f"COCOEval: record {len(self.records)} names image {r['image_id']!r}, which the "
                                 "annotations do not have")
            if need not in r:
                raise ValueError(f"COCOEval: record {len(self.records)} has no {need!r} ({self.iou_type} evaluation)")
            self.records.append(r)
        return self

    # ---- flat state -------------------------------------------------------------------------------------------------
    def _flatten(self):
        I = len(self.img_ids)
        img_at = {v: i for i, v in enumerate(self.img_ids)}
        cat_at = {c: k for k, c in enumerate(self.cat_ids)}
        anns = [a for a in self.gt.get("annotations") or [] if a["category_id"] in cat_at and a["image_id"] in img_at]
        g_key = np.array([cat_at[a["category_id"]] * I + img_at[a["image_id"]] for a in anns], dtype=np.int64)
        order = np.argsort(g_key, kind="stable")             # (category, image), the annotations' order inside
        g = {"key": g_key[order], "ann": [anns[i] for i in order]}
        g["id"] = np.array([a["id"] for a in g["ann"]], dtype=np.int64)
        g["crowd"] = np.array([1 if a.get("iscrowd") else 0 for a in g["ann"]], dtype=np.uint8)
        g["area"] = np.array([a["area"] for a in g["ann"]], dtype=np.float64)
        recs = [(i + 1, r) for i, r in enumerate(self.records) if r["category_id"] in cat_at]
        d_key = np.array([cat_at[r["category_id"]] * I + img_at[r["image_id"]] for _, r in recs], dtype=np.int64)
        score = np.array([r["score"] for _, r in recs], dtype=np.float64)
        order = np.lexsort((-score, d_key))                  # stable: (category, image), then the score, then arrival
        key = d_key[order]
        first = np.flatnonzero(np.concatenate(([True], key[1:] != key[:-1]))) if len(key) else np.zeros(0, np.int64)
        counts = np.diff(np.concatenate((first, [len(key)])))
        rank = _within(counts)
        keep = rank < self.max_dets[-1]                      # the cut to the last maxDets
        order = order[keep]
        d = {"key": key[keep], "rank": rank[keep], "score": score[order], "rec": [recs[i][1] for i in order],
             "id": np.array([recs[i][0] for i in order], dtype=np.int64)}
        keys = np.union1d(g["key"], d["key"])
        D = np.searchsorted(d["key"], keys, side="right") - np.searchsorted(d["key"], keys, side="left")
        G = np.searchsorted(g["key"], keys, side="right") - np.searchsorted(g["key"], keys, side="left")
        table = np.stack((D, G, _group_offsets(D), _group_offsets(G), _group_offsets(D * G)), 1).astype(np.int64)
        return g, d, keys, table.reshape(-1, 5)

    def _pairs(self, table):
        """-> (detection index, ground-truth index) of every IoU element, in the flat array's order"""
        D, G, dof, gof, _ = table.T
        n = D * G
        local = _within(n)
        Gp = np.repeat(G, n)
        return np.repeat(dof, n) + local // np.maximum(Gp, 1), np.repeat(gof, n) + local % np.maximum(Gp, 1)

    def _box_ious(self, g, d, table):
        gb = np.array([a["bbox"] for a in g["ann"]], dtype=np.float64).reshape(-1, 4)
        db = np.array([r["bbox"] for r in d["rec"]], dtype=np.float64).reshape(-1, 4)
        d_area = db[:, 2] * db[:, 3]
        di, gi = self._pairs(table)
        a, b = db[di], gb[gi]
        w = np.minimum(a[:, 0] + a[:, 2], b[:, 0] + b[:, 2]) - np.maximum(a[:, 0], b[:, 0])
        h = np.minimum(a[:, 1] + a[:, 3], b[:, 1] + b[:, 3]) - np.maximum(a[:, 1], b[:, 1])
        hit = (w > 0) & (h > 0)
        i = np.where(hit, w * h, 0.0)
        u = np.where(g["crowd"][gi] != 0, d_area[di], d_area[di] + gb[gi, 2] * gb[gi, 3] - i)
        return np.divide(i, u, out=np.zeros(len(i), dtype=np.float64), where=hit & (u > 0)), d_area

    def _size_of(self, seg, image, label):
        size = [int(seg["size"][0]), int(seg["size"][1])]
        if "height" in image and "width" in image and size != [int(image["height"]), int(image["width"])]:
            raise ValueError(f"COCOEval: mask-size mismatch: {label} is {size[0]} x {size[1]}, its image "
                             f"{image['height']} x {image['width']}")
        return size

    def _mask_ious(self, g, d, table):
        masks = [(f"record {i - 1} (image {r['image_id']!r})", self.images[r["image_id"]], r["segmentation"])
                 for i, r in zip(d["id"].tolist(), d["rec"])]
        masks += [(f"annotation {a['id']!r} (image {a['image_id']!r})", self.images[a["image_id"]], a["segmentation"])
                  for a in g["ann"]]
        counts, counts_sizes, counts_at, strings, string_sizes, string_at, labels = [], [], [], [], [], [], []
        polys, poly_sizes, poly_at = [], [], []
        for m, (label, image, seg) in enumerate(masks):
            if self.polygons and m >= len(d["rec"]) and isinstance(seg, list) and seg:
                if "height" not in image or "width" not in image:
                    raise ValueError(f"COCOEval: {label} is a polygon and its image states no height / width")
                polys.append(seg)
                poly_sizes.append((int(image["height"]), int(image["width"])))
                poly_at.append(m)
                continue
            if not isinstance(seg, dict):
                raise ValueError(f"COCOEval: {label} has no RLE segmentation")
            size = self._size_of(seg, image, label)
            if isinstance(seg["counts"], (str, bytes)):
                strings.append(seg["counts"])
                string_sizes.append(size)
                string_at.append(m)
                labels.append(label)
            else:
                counts.append(seg["counts"])
                counts_sizes.append(size)
                counts_at.append(m)
        try:
            t_counts = V.runs_from_counts(counts, counts_sizes)
        except ValueError as e:
            raise ValueError(f"COCOEval: malformed uncompressed RLE: {e}") from None
        t_strings = V.decode_strings(strings, string_sizes, device=self.device, labels=labels)
        if self.device is not None:
            t_counts = t_counts.to(t_strings.rows.device)
        tables = V.concat_tables(t_counts, t_strings)
        if polys:
            try:
                t_polys = polygons_to_runs(polys, poly_sizes, device=self.device)
            except ValueError as e:
                raise ValueError(f"COCOEval: malformed polygon ground truth ({masks[poly_at[0]][0]} is object 0): {e}") from None
            tables = V.concat_tables(tables, t_polys)
        row_of = np.zeros(len(masks), dtype=np.int32)        # one frame per track: track m's mask is row_of[m]
        row_of[counts_at] = np.arange(len(counts), dtype=np.int32)
        row_of[string_at] = len(counts) + np.arange(len(strings), dtype=np.int32)
        row_of[poly_at] = len(counts) + len(strings) + np.arange(len(polys), dtype=np.int32)
        tracks = np.stack((np.arange(len(masks)), np.ones(len(masks))), 1).astype(np.int32).reshape(-1, 2)
        di, gi = self._pairs(table)
        pairs = np.stack((di, len(d["rec"]) + gi), 1).astype(np.int32).reshape(-1, 2)
        t1 = time.perf_counter()
        sums = V.pair_sums(tables, row_of, tracks, pairs)
        bad = np.flatnonzero(sums[:, 3])
        if len(bad):
            a, b = pairs[bad[0]]
            what = "have masks of different sizes (mask-size mismatch)" if int(sums[bad[0], 3]) == _lib.VIDEO_IOU_PIXELS \
                else "point outside the run tables"
            raise ValueError(f"COCOEval: {masks[a][0]} and {masks[b][0]} {what}")
        area = (tables.rows[:, 3].cpu().numpy() if tables.is_cuda else tables.rows[:, 3])[row_of[:len(d["rec"])]]
        i = sums[:, 0].astype(np.float64)
        u = np.where(g["crowd"][gi] != 0, sums[:, 1], sums[:, 1] + sums[:, 2] - sums[:, 0]).astype(np.float64)
        return np.divide(i, u, out=np.zeros(len(i), dtype=np.float64), where=u > 0), area.astype(np.float64), t1

    # ---- COCOeval.evaluate ------------------------------------------------------------------------------------------
    def evaluate(self, eval_imgs=False):
        """-> {"AP", "AP50", ..., "ARl" (the 12 numbers of `summarize`; -1 where the reference leaves -1), "stats"
        float64 [12], "per_category" {name: AP in percent, as `_derive_coco_results` forms it}, "precision" [T, R, K,
        A, M], "recall" [T, K, A, M], "scores" [T, R, K, A, M], "ious" {(image, category): [D, G] or []}}; with
        `eval_imgs=True` also "eval_imgs", the reference's `evalImgs` (one dict or None per (category, area range,
        image); a Python loop over them)."""
        t0 = time.perf_counter()
        g, d, keys, table = self._flatten()
        if self.iou_type == "bbox":
            ious, d_area = self._box_ious(g, d, table)
            t1 = time.perf_counter()
        else:
            ious, d_area, t1 = self._mask_ious(g, d, table)
        t2 = time.perf_counter()
        area_rng = np.array(self.area_rng, dtype=np.float64).reshape(-1, 2)
        m = self._match(table, ious, g["crowd"], g["area"], d_area, area_rng)
        t3 = time.perf_counter()
        # indices -> ids; the reference's `dtm == 0` sees an id of 0 as no match
        gof_of_dt = np.repeat(table[:, 3], table[:, 0])
        dof_of_gt = np.repeat(table[:, 2], table[:, 1])
        dtm = np.where(m.dt_match >= 0, g["id"][np.clip(gof_of_dt + m.dt_match, 0, max(len(g["id"]) - 1, 0))]
                       if len(g["id"]) else 0, 0)
        gtm = np.where(m.gt_match >= 0, d["id"][np.clip(dof_of_gt + m.gt_match, 0, max(len(d["id"]) - 1, 0))]
                       if len(d["id"]) else 0, 0)
        outside = (d_area[None, :] < area_rng[:, 0:1]) | (d_area[None, :] > area_rng[:, 1:2])
        dt_ig = (m.dt_ignore != 0) | ((dtm == 0) & outside[:, None, :])
        flat = {"g": g, "d": d, "keys": keys, "table": table, "dtm": dtm, "gtm": gtm, "dt_ig": dt_ig,
                "gt_ig": m.gt_ignore}
        out = self._accumulate(flat)
        self.timings = {"tables_s": t1 - t0, "sums_s": t2 - t1, "match_s": t3 - t2, "accumulate_s": time.perf_counter() - t3,
                        "problems": int(len(table)), "detections": int(len(d["id"])), "ground_truths": int(len(g["id"])),
                        "pairs": int(len(ious)), "matching": self.matching, "host_fallback": bool(m.host_fallback)}
        out["stats"] = summarize(out["precision"], out["recall"], self.iou_thrs, self.max_dets)
        out.update({n: float(s) for n, s in zip(STAT_NAMES, out["stats"])})
        out["per_category"] = {}
        for k, c in enumerate(self.cat_ids):
            p = out["precision"][:, :, k, 0, -1]
            p = p[p > -1]
            out["per_category"][str(self.categories[c].get("name", c))] = float(np.mean(p) * 100) if p.size \
                else float("nan")
        out["ious"] = _Ious(self.img_ids, self.cat_ids, keys, table, ious)
        if eval_imgs:
            out["eval_imgs"] = self._eval_imgs(flat)
        return out

    def _match(self, table, ious, gt_crowd, gt_area, dt_area, area_rng):
        if self.matching == "host":
            return M.match_host(table, ious, gt_crowd, gt_area, dt_area, area_rng, self.iou_thrs)
        if self.matching == "vectorised":
            return M.match_vectorised(table, ious, gt_crowd, gt_area, dt_area, area_rng, self.iou_thrs)
        import torch
        dev = torch.device(self.device)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(dev)   # noqa: E731
        return M.ap_match(up(table, np.int64), up(ious, np.float64), up(gt_crowd, np.uint8), up(gt_area, np.float64),
                          up(dt_area, np.float64), up(area_rng, np.float64), up(self.iou_thrs, np.float64),
                          max_gt=int(table[:, 1].max()) if len(table) else 0).numpy()

    # ---- COCOeval.accumulate ----------------------------------------------------------------------------------------
    def _accumulate(self, flat):
        T, R, K, A, M_ = len(self.iou_thrs), len(self.rec_thrs), len(self.cat_ids), len(self.area_rng), len(self.max_dets)
        precision = -np.ones((T, R, K, A, M_))
        recall = -np.ones((T, K, A, M_))
        scores = -np.ones((T, R, K, A, M_))
        I = len(self.img_ids)
        d, g = flat["d"], flat["g"]
        d_cut = np.searchsorted(d["key"], np.arange(K + 1) * I)      # a category's detections: one slice, images in order
        g_cut = np.searchsorted(g["key"], np.arange(K + 1) * I)
        for k in range(K):
            ds, gs = slice(d_cut[k], d_cut[k + 1]), slice(g_cut[k], g_cut[k + 1])
            if d_cut[k] == d_cut[k + 1] and g_cut[k] == g_cut[k + 1]:
                continue
            for a in range(A):
                gt_ig = flat["gt_ig"][a, gs]
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                for m, max_det in enumerate(self.max_dets):
                    sel = np.flatnonzero(d["rank"][ds] < max_det)
                    dt_scores = d["score"][ds][sel]
                    inds = np.argsort(-dt_scores, kind="mergesort")
                    sorted_scores = dt_scores[inds]
                    dtm = flat["dtm"][a, :, ds][:, sel[inds]]
                    dt_ig = flat["dt_ig"][a, :, ds][:, sel[inds]]
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
        return {"precision": precision, "recall": recall, "scores": scores, "counts": [T, R, K, A, M_]}

    # ---- evalImgs, on request ---------------------------------------------------------------------------------------
    def _eval_imgs(self, flat):
        """The reference's `evalImgs` from the flat state: ground truths in its order (ignored last, stable)."""
        I = len(self.img_ids)
        g, d, keys, table = flat["g"], flat["d"], flat["keys"], flat["table"]
        at = {int(k): p for p, k in enumerate(keys)}
        out = []
        for k, c in enumerate(self.cat_ids):
            for a, rng in enumerate(self.area_rng):
                for i, v in enumerate(self.img_ids):
                    p = at.get(k * I + i)
                    if p is None:
                        out.append(None)
                        continue
                    D, G, dof, gof, _ = table[p].tolist()
                    ig = flat["gt_ig"][a, gof:gof + G].astype(np.int64)
                    order = np.argsort(ig, kind="mergesort")
                    out.append({"image_id": v, "category_id": c, "aRng": rng, "maxDet": self.max_dets[-1],
                                "dtIds": d["id"][dof:dof + D].tolist(), "gtIds": g["id"][gof:gof + G][order].tolist(),
                                "dtMatches": flat["dtm"][a, :, dof:dof + D].astype(np.float64),
                                "gtMatches": flat["gtm"][a, :, gof:gof + G][:, order].astype(np.float64),
                                "dtScores": d["score"][dof:dof + D].tolist(), "gtIgnore": ig[order],
                                "dtIgnore": flat["dt_ig"][a, :, dof:dof + D]})
        return out


class COCOEvaluator:
    """detectron2's `COCOEvaluator` protocol (`reset()` / `process(inputs, outputs)` / `evaluate()`) around `COCOEval`.

    `outputs` is `model(inputs)`'s [{"instances": {"pred_boxes" xyxy, "scores", "pred_classes", "pred_masks"}}] of the
    COCO branch (boxes go to xywh, masks through `utils.ytvis_json.rle_encode`; `category_ids[class]` is the dataset's
    category id, the class index itself when None), or a list of `coco_results` records.  `evaluate()` returns {"bbox":
    {...}, "segm": {...}} in percent under detectron2's names (AP, AP50, AP75, APs, APm, APl, NaN where the reference has
    -1, and "AP-<name>" per category when there is more than one); "segm" is absent when no record carries a mask
    (MASK_ON false).  Gathering records across ranks stays the caller's `gather_object`.
    """
    NAMES = STAT_NAMES[:6]

    def __init__(self, gt, device=None, category_ids=None, **params):
        if isinstance(gt, (str, os.PathLike)):
            with open(gt) as f:
                gt = json.load(f)
        self._args = (gt, device, params)
        self.category_ids = category_ids
        self.reset()

    def reset(self):
        self.records = []

    def process(self, inputs, outputs):
        from ..utils.ytvis_json import rle_encode
        if not (len(outputs) and isinstance(outputs[0], dict) and "instances" in outputs[0]):
            self.records.extend(outputs)
            return
        host = lambda x: np.asarray(x.cpu() if hasattr(x, "cpu") else x)                 # noqa: E731
        for b, (x, o) in enumerate(zip(inputs, outputs)):
            inst = o["instances"]
            boxes = host(inst["pred_boxes"]).reshape(-1, 4).astype(np.float64)
            masks = host(inst["pred_masks"]) if inst.get("pred_masks") is not None else None
            for i, (score, label) in enumerate(zip(host(inst["scores"]).tolist(), host(inst["pred_classes"]).tolist())):
                x0, y0, x1, y1 = boxes[i].tolist()
                rec = {"image_id": x.get("image_id", b), "score": float(score), "bbox": [x0, y0, x1 - x0, y1 - y0],
                       "category_id": int(label) if self.category_ids is None else self.category_ids[int(label)]}
                if masks is not None:
                    rec["segmentation"] = rle_encode(masks[i])
                self.records.append(rec)

    def evaluate(self):
        gt, device, params = self._args
        types = ["bbox"] + (["segm"] if any("segmentation" in r for r in self.records) else [])
        if not self.records:
            return {"bbox": {n: float("nan") for n in self.NAMES}}
        out, self.results = {}, {}
        for iou_type in types:
            res = COCOEval(gt, iou_type, device=device, **params).add(self.records).evaluate()
            one = {n: float(res[n] * 100 if res[n] >= 0 else "nan") for n in self.NAMES}
            if len(res["per_category"]) > 1:
                one.update({"AP-" + name: ap for name, ap in res["per_category"].items()})
            out[iou_type], self.results[iou_type] = one, res
        return out
