"""The AP evaluation that `COCOEval` (coco_eval.py) and `YTVISEval` (ytvis_eval.py) share: cocoapi's `loadRes` +
`evaluate / accumulate / summarize`, which the YouTube-VIS fork copied, stated once.  A unit is an image or a video, a
mask a track of frames (one frame for an image); a class says what its unit is called, where a track's masks are, what
an area is and how pair sums become an IoU, and nothing else.

The state is flat: detections and ground truths sorted by (category, unit) -- detections by score inside a group
(stable) and cut to the last `max_dets` -- and one row {D, G, offsets} per (unit, category) that has either.  The mask
IoU is taken as integer sums over run tables (ops/video_iou.py: the kernel for a CUDA device, numpy otherwise) and one
IEEE double division on the host, so both routes give the same bits.  The matching is ops/ap_match.py: the kernel (one
launch), `match_vectorised`, or `match_host` (plain Python, the readable form).  The accumulation slices a category's
detections out of the flat arrays, with the numpy calls the reference's numbers depend on (`argsort(kind="mergesort")`,
`cumsum`, the spacing of 1.0, `searchsorted(side="left")`); no step of the matching or the accumulation loops over units,
detections or ground truths in Python.
"""
from __future__ import annotations

import functools
import json
import os
import time
from collections.abc import Mapping

import numpy as np

from .. import _lib
from ..ops import ap_match as M
from ..ops import video_iou as V
from ..ops.poly_rle import polygons_to_runs

STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")
AREA_LABELS = ("all", "small", "medium", "large")
MATCHING = ("device", "vectorised", "host")


def _default_device():
    try:
        import torch
        return "cuda" if torch.cuda.is_available() and os.path.exists(_lib.LIB_PATH) else None
    except Exception:
        return None


def load_json(gt):
    """an annotation document: the dict itself, or the path of its JSON file"""
    if isinstance(gt, (str, os.PathLike)):
        with open(gt) as f:
            return json.load(f)
    return gt


class _Ious(Mapping):
    """`COCOeval.ious`: {(unit, category): float64 [D, G], or [] where the pair has neither} over the flat array."""

    def __init__(self, unit_ids, cat_ids, keys, table, flat):
        self._units = {v: i for i, v in enumerate(unit_ids)}
        self._cats = {c: k for k, c in enumerate(cat_ids)}
        self._unit_ids, self._cat_ids, self._keys, self._table, self._flat = unit_ids, cat_ids, keys, table, flat

    def __getitem__(self, key):
        i, k = self._units[key[0]], self._cats[key[1]]
        want = k * len(self._unit_ids) + i
        p = int(np.searchsorted(self._keys, want))
        if p == len(self._keys) or self._keys[p] != want:
            return []
        D, G, _, _, off = self._table[p].tolist()
        return self._flat[off:off + D * G].reshape(D, G).copy()

    def __iter__(self):
        return ((v, c) for v in self._unit_ids for c in self._cat_ids)

    def __len__(self):
        return len(self._unit_ids) * len(self._cat_ids)


class _Lazy:
    """a sequence whose element m is made when it is asked for: the masks' labels, which only an error reads"""

    def __init__(self, make):
        self._make = make

    def __getitem__(self, m):
        return self._make(m)


def _group_offsets(D):
    D = np.asarray(D, dtype=np.int64)
    return np.cumsum(D) - D


def _within(counts):
    """[3, 2] -> [0, 1, 2, 0, 1]"""
    counts = np.asarray(counts, dtype=np.int64)
    return np.arange(int(counts.sum()), dtype=np.int64) - np.repeat(_group_offsets(counts), counts)


class APEval:
    """`Eval(gt, ...).add(records)`, then `.evaluate()`.  A class states:

    UNIT         "image" / "video": records and annotations name theirs under UNIT + "_id", the document lists them
                 under UNIT + "s", and messages call them that
    EVAL_KEY     the name of the reference's `evalImgs` in the result
    AREA_RNG     the default area ranges all / small / medium / large
    FRAMES       a track is a list of per-frame masks: labels name the frame, and a frame may be without a mask (None);
                 False = a track is one mask, which must be there
    STATUS_TEXT  what a pair's non-zero status (ops/video_iou.py) says in an error
    `_masks_of(items)`, `_gt_area(ann)`, `_dt_areas(...)`, `_ious_from_sums(sums, crowd)`: below

    Parameters: gt: the annotation JSON (a dict or a path).  device: a CUDA device for the kernels; None = CUDA when this
    process has one and the library is built; "cpu" = numpy.  matching: "device" / "vectorised" / "host", the route of the
    matching alone (`_default_matching` without one).  iou_thrs, rec_thrs, max_dets, area_rng: the reference's Params
    (0.5 : 0.05 : 0.95, 0 : 0.01 : 1, [1, 10, 100], the class's ranges).  polygons: False = polygon ground truth raises
    ValueError; True = a list segmentation (polygons or boxes, as frPyObjects takes them) is rasterised at its unit's
    `height` x `width` by `ops.poly_rle.polygons_to_runs`, on the evaluator's device (the kernel) or on the host, and
    joins the RLE ground truth in one table; areas stay what the annotation states.
    """
    UNIT = EVAL_KEY = AREA_RNG = None
    FRAMES = False
    STATUS_TEXT = {_lib.VIDEO_IOU_PIXELS: "have masks of different sizes (mask-size mismatch)"}
    need = None                                             # a key every record must carry

    def __init__(self, gt, device=None, iou_thrs=None, rec_thrs=None, max_dets=(1, 10, 100), area_rng=None,
                 matching=None, polygons=False):
        self.name, self.key = type(self).__name__, self.UNIT + "_id"
        gt = load_json(gt)
        if not isinstance(gt, dict):
            raise ValueError(f"{self.name}: annotation format {type(gt)} not supported")
        self.gt, self.polygons = gt, bool(polygons)
        self.device = _default_device() if device is None else (None if str(device) == "cpu" else device)
        if matching is None:
            matching = self._default_matching(device)
        if matching not in MATCHING or (matching == "device" and self.device is None):
            raise ValueError(f"{self.name}: matching {matching!r} (one of {MATCHING}; 'device' needs a CUDA device)")
        self.matching = matching
        self.iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True) if iou_thrs is None \
            else np.asarray(iou_thrs, dtype=np.float64)
        self.rec_thrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True) if rec_thrs is None \
            else np.asarray(rec_thrs, dtype=np.float64)
        self.max_dets = sorted(int(m) for m in max_dets)
        self.area_rng = [list(a) for a in (self.AREA_RNG if area_rng is None else area_rng)]
        if len(self.area_rng) != len(AREA_LABELS):
            raise ValueError(f"{self.name}: area_rng needs the four ranges all / small / medium / large")
        self.units = {v["id"]: v for v in gt.get(self.UNIT + "s", [])}
        self.categories = {c["id"]: c for c in gt.get("categories", [])}
        self.unit_ids = [v.item() for v in np.unique(list(self.units))] if self.units else []
        self.cat_ids = [c.item() for c in np.unique(list(self.categories))] if self.categories else []
        anns = gt.get("annotations") or []
        for seg, t, f in zip(*self._frames(anns)[:3]):
            if isinstance(seg, list) and seg and not self.polygons:
                raise ValueError(f"{self.name}: annotation {anns[t].get('id')}{f' frame {f}' if self.FRAMES else ''} is a "
                                 "polygon; only RLE ground truth is supported")
        self.records = []

    def _default_matching(self, device):
        """the kernel with a CUDA device, `match_host` for device="cpu", `match_vectorised` where None found no device"""
        return "device" if self.device is not None else "host" if device is not None else "vectorised"

    def add(self, records):
        """records: the model's result records ({UNIT + "_id", "category_id", "score", ...}); may be called once per
        batch.  Ids are index + 1 in the order added."""
        for r in records:
            if r[self.key] not in self.units:
                raise ValueError(f"{self.name}: record {len(self.records)} names {self.UNIT} {r[self.key]!r}, which the "
                                 "annotations do not have")
            if self.need is not None and self.need not in r:
                raise ValueError(f"{self.name}: record {len(self.records)} has no {self.need!r}")
            self.records.append(r)
        return self

    # ---- what a class states ----------------------------------------------------------------------------------------
    def _masks_of(self, items):
        """annotations or records -> (the masks of their tracks, one per frame and None for a frame without one, as one
        list; the tracks' lengths)"""
        raise NotImplementedError

    def _gt_area(self, ann):
        raise NotImplementedError

    def _dt_areas(self, area, frame_mask, rows):
        """area: every mask's pixel count; frame_mask, rows: the detections' tracks -> the detections' areas"""
        raise NotImplementedError

    def _ious_from_sums(self, sums, crowd):
        """int64 [P, 4] pair sums, the crowd flag of each pair's ground truth -> float64 [P]"""
        raise NotImplementedError

    # ---- flat state -------------------------------------------------------------------------------------------------
    def _flatten(self):
        I = len(self.unit_ids)
        unit_at = {v: i for i, v in enumerate(self.unit_ids)}
        cat_at = {c: k for k, c in enumerate(self.cat_ids)}
        anns = [a for a in self.gt.get("annotations") or [] if a["category_id"] in cat_at and a[self.key] in unit_at]
        g_key = np.array([cat_at[a["category_id"]] * I + unit_at[a[self.key]] for a in anns], dtype=np.int64)
        order = np.argsort(g_key, kind="stable")             # (category, unit), the annotations' order inside
        g = {"key": g_key[order], "ann": [anns[i] for i in order]}
        g["id"] = np.array([a["id"] for a in g["ann"]], dtype=np.int64)
        g["crowd"] = np.array([1 if a.get("iscrowd") else 0 for a in g["ann"]], dtype=np.uint8)
        g["area"] = np.array([self._gt_area(a) for a in g["ann"]], dtype=np.float64)
        recs = [(i + 1, r) for i, r in enumerate(self.records) if r["category_id"] in cat_at]
        d_key = np.array([cat_at[r["category_id"]] * I + unit_at[r[self.key]] for _, r in recs], dtype=np.int64)
        score = np.array([r["score"] for _, r in recs], dtype=np.float64)
        order = np.lexsort((-score, d_key))                  # stable: (category, unit), then the score, then arrival
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

    # ---- masks -> run tables -> IoU ---------------------------------------------------------------------------------
    def _size_of(self, seg, unit, where, slot):
        if not isinstance(seg, dict):
            raise ValueError(f"{self.name}: {where(slot)} has no RLE segmentation")
        size = [int(seg["size"][0]), int(seg["size"][1])]
        if "height" in unit and "width" in unit and size != [int(unit["height"]), int(unit["width"])]:
            raise ValueError(f"{self.name}: mask-size mismatch: {where(slot)} is {size[0]} x {size[1]}, its {self.UNIT} "
                             f"{unit['height']} x {unit['width']}")
        return size

    def _frames(self, items):
        """-> (every mask of the items' tracks in order, its track's index, its frame's index, the tracks' lengths)"""
        masks, lengths = self._masks_of(items)
        return masks, np.repeat(np.arange(len(items)), lengths).tolist(), _within(lengths).tolist(), lengths

    def _tables(self, label, items, first_gt):
        """items: records, then (from `first_gt`) annotations; label(t, f): what an error calls frame f of item t ->
        (tables, frame_mask, track rows); one mask per present frame, by kind: uncompressed counts, then compressed
        strings, then polygons"""
        counts, strings, polys = (([], [], []) for _ in range(3))            # of a kind: masks, sizes, frame_mask slots
        frame_mask = []
        polygons = self.polygons
        units = [self.units[x[self.key]] for x in items]
        masks, track_of, frame_of, lengths = self._frames(items)
        where = lambda slot: label(track_of[slot], frame_of[slot])           # noqa: E731  (made on error only)
        for seg, t in zip(masks, track_of):
            if not seg:
                if not self.FRAMES:
                    raise ValueError(f"{self.name}: {where(len(frame_mask))} has no RLE segmentation")
                frame_mask.append(-1)
                continue
            unit = units[t]
            if polygons and t >= first_gt and isinstance(seg, list):
                if "height" not in unit or "width" not in unit:
                    raise ValueError(f"{self.name}: {where(len(frame_mask))} is a polygon and its {self.UNIT} states no "
                                     "height / width")
                kind, mask, size = polys, seg, (int(unit["height"]), int(unit["width"]))
            else:
                size, mask = self._size_of(seg, unit, where, len(frame_mask)), seg["counts"]
                kind = strings if isinstance(mask, (str, bytes)) else counts
            kind[0].append(mask)
            kind[1].append(size)
            kind[2].append(len(frame_mask))
            frame_mask.append(0)
        try:
            parts = [V.runs_from_counts(counts[0], counts[1])]
        except ValueError as e:
            raise ValueError(f"{self.name}: malformed uncompressed RLE: {e}") from None
        parts.append(V.decode_strings(strings[0], strings[1], device=self.device,
                                      labels=_Lazy(lambda m: where(strings[2][m]))))
        if self.device is not None:
            parts[0] = parts[0].to(parts[1].rows.device)
        if polys[0]:
            try:
                parts.append(polygons_to_runs(polys[0], polys[1], device=self.device))
            except ValueError as e:
                raise ValueError(f"{self.name}: malformed polygon ground truth ({where(polys[2][0])} is object 0): "
                                 f"{e}") from None
        tables = functools.reduce(V.concat_tables, parts)
        frame_mask = np.array(frame_mask, dtype=np.int32).reshape(-1)
        frame_mask[np.array(counts[2] + strings[2] + polys[2], dtype=np.int64)] = np.arange(len(tables), dtype=np.int32)
        return tables, frame_mask, np.stack((_group_offsets(lengths), lengths), 1).astype(np.int32).reshape(-1, 2)

    def _ious(self, g, d, di, gi):
        """the IoU of every pair -> (float64 [P], the detections' areas, masks in the tables, the time the sums began)"""
        n_dt, items = len(d["rec"]), d["rec"] + g["ann"]

        def label(t, f=None):
            """what an error calls item t, or frame f of it; made then, since a label per mask costs as much as the
            rest of the loop over the masks"""
            what = f"record {d['id'][t] - 1}" if t < n_dt else f"annotation {items[t]['id']!r}"
            frame = f" frame {f}" if self.FRAMES and f is not None else ""
            return f"{what} ({self.UNIT} {items[t][self.key]!r}){frame}"
        tables, frame_mask, rows = self._tables(label, items, n_dt)
        pairs = np.stack((di, n_dt + gi), 1).astype(np.int32).reshape(-1, 2)
        t1 = time.perf_counter()
        sums = V.pair_sums(tables, frame_mask, rows, pairs)
        bad = np.flatnonzero(sums[:, 3])
        if len(bad):
            a, b = pairs[bad[0]]
            why = self.STATUS_TEXT.get(int(sums[bad[0], 3]), "point outside the run tables")
            raise ValueError(f"{self.name}: {label(a)} and {label(b)} {why}")
        area = tables.rows[:, 3].cpu().numpy() if tables.is_cuda else tables.rows[:, 3]
        return self._ious_from_sums(sums, g["crowd"][gi]), self._dt_areas(area, frame_mask, rows[:n_dt]), len(tables), t1

    # ---- evaluate ---------------------------------------------------------------------------------------------------
    def evaluate(self, eval_imgs=False):
        """-> {"AP", "AP50", ..., "ARl" (the 12 numbers of `summarize`; -1 where the reference leaves -1), "stats"
        float64 [12], "per_category" {name: AP in percent, as `_derive_coco_results` forms it}, "precision" [T, R, K,
        A, M], "recall" [T, K, A, M], "scores" [T, R, K, A, M], "ious" {(unit, category): [D, G] or []}}; with
        `eval_imgs=True` also EVAL_KEY, the reference's `evalImgs` (one dict or None per (category, area range, unit);
        a Python loop over them).  `timings` holds the stages on the host clock, in seconds: flat state and run tables
        (decode included), pair sums (copies included), matching, accumulation."""
        t0 = time.perf_counter()
        g, d, keys, table = self._flatten()
        ious, d_area, masks, t1 = self._ious(g, d, *self._pairs(table))
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
                        "pairs": int(len(ious)), "masks": int(masks), "matching": self.matching,
                        "host_fallback": bool(m.host_fallback)}
        out["stats"] = summarize(out["precision"], out["recall"], self.iou_thrs, self.max_dets)
        out.update({n: float(s) for n, s in zip(STAT_NAMES, out["stats"])})
        out["per_category"] = {}
        for k, c in enumerate(self.cat_ids):
            p = out["precision"][:, :, k, 0, -1]
            p = p[p > -1]
            out["per_category"][str(self.categories[c].get("name", c))] = float(np.mean(p) * 100) if p.size \
                else float("nan")
        out["ious"] = _Ious(self.unit_ids, self.cat_ids, keys, table, ious)
        if eval_imgs:
            out[self.EVAL_KEY] = self._eval_imgs(flat)
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

    # ---- accumulate -------------------------------------------------------------------------------------------------
    def _accumulate(self, flat):
        T, R, K, A, M_ = len(self.iou_thrs), len(self.rec_thrs), len(self.cat_ids), len(self.area_rng), len(self.max_dets)
        precision = -np.ones((T, R, K, A, M_))
        recall = -np.ones((T, K, A, M_))
        scores = -np.ones((T, R, K, A, M_))
        I = len(self.unit_ids)
        d, g = flat["d"], flat["g"]
        d_cut = np.searchsorted(d["key"], np.arange(K + 1) * I)      # a category's detections: one slice, units in order
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

    # ---- evalImgs ---------------------------------------------------------------------------------------------------
    def _eval_imgs(self, flat):
        """The reference's `evalImgs` from the flat state: ground truths in its order (ignored last, stable)."""
        I = len(self.unit_ids)
        g, d, keys, table = flat["g"], flat["d"], flat["keys"], flat["table"]
        at = {int(k): p for p, k in enumerate(keys)}
        out = []
        for k, c in enumerate(self.cat_ids):
            for a, rng in enumerate(self.area_rng):
                for i, v in enumerate(self.unit_ids):
                    p = at.get(k * I + i)
                    if p is None:
                        out.append(None)
                        continue
                    D, G, dof, gof, _ = table[p].tolist()
                    ig = flat["gt_ig"][a, gof:gof + G].astype(np.int64)
                    order = np.argsort(ig, kind="mergesort")
                    out.append({self.key: v, "category_id": c, "aRng": rng, "maxDet": self.max_dets[-1],
                                "dtIds": d["id"][dof:dof + D].tolist(), "gtIds": g["id"][gof:gof + G][order].tolist(),
                                "dtMatches": flat["dtm"][a, :, dof:dof + D].astype(np.float64),
                                "gtMatches": flat["gtm"][a, :, gof:gof + G][:, order].astype(np.float64),
                                "dtScores": d["score"][dof:dof + D].tolist(), "gtIgnore": ig[order],
                                "dtIgnore": flat["dt_ig"][a, :, dof:dof + D]})
        return out


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


def in_percent(res, names):
    """What the evaluator classes return for one IoU type: `names` of an `evaluate()` result in percent (NaN where the
    reference has -1: `_derive_coco_results`) and "AP-<category>" per category when there is more than one; `res=None`
    (nothing to score): NaN throughout."""
    if res is None:
        return {n: float("nan") for n in names}
    out = {n: float(res[n] * 100 if res[n] >= 0 else "nan") for n in names}
    if len(res["per_category"]) > 1:
        out.update({"AP-" + name: ap for name, ap in res["per_category"].items()})
    return out
