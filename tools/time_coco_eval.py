"""Time the local COCO evaluator at val2017's scale.  MI355X only.

A synthetic set: `--images` images of 480 x 640 (default 5 000), 80 categories, 100 detections and about 7 ground
truths per image, every mask a compressed RLE string.  The masks come from a pool of ellipses (`--clusters` base
shapes, each with jittered variants, encoded once on the host): an image takes a handful of clusters, its ground
truths are their base shapes, its detections variants of them (some from other clusters, some under another
category), so the IoUs, the ties and the share of matches are of the usual kind while the set builds in seconds.
Distinct records share mask strings; the evaluator does not know and decodes every one.  Reported, per IoU type:

  device       COCOEval(device="cuda").evaluate(): the total and the stages on the host clock, ending in a device
               synchronise (tables = flat state + upload + decode, sums = pair sums + copy back, matching = upload +
               the one launch + copy back, accumulation); median of `--iters` runs after a warm-up run
  cpu          the same class with device="cpu" (numpy tables and sums, `match_host`): one run
  matchers     the matching alone on the evaluation's own flat arrays: the kernel by device events (median),
               `match_vectorised` and `match_host` on the host clock
  launches     launches of this package's kernels in one device evaluate()
  fallback     the share of problems that took the host fallback (must be 0 here), the largest G

Both routes must return identical arrays.  `--rehearse` runs the cpu route alone at the given size, without a GPU, and
writes nothing: it checks the tool, it measures nothing.

    python tools/time_coco_eval.py [--images 5000] [--out profiles/coco_eval.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

H, W, CATS, DETS, VARIANTS = 480, 640, 80, 100, 12


def build_pool(clusters, rng):
    """-> per cluster: category, [(rle, tight box, area)] with the base shape first"""
    from vnext_amd.utils.ytvis_json import rle_encode
    yy, xx = np.mgrid[0:H, 0:W]
    pool = []
    for _ in range(clusters):
        cy, cx = rng.uniform(40, H - 40), rng.uniform(40, W - 40)
        ry, rx = np.exp(rng.uniform(np.log(8), np.log(150), 2))          # areas on both sides of 32^2 and 96^2
        shapes = []
        for j in range(1 + VARIANTS):
            spread = 0.0 if j == 0 else 0.05 * j
            dy, dx = rng.uniform(-1, 1, 2) * spread * np.array([ry, rx])
            s = 1 + rng.uniform(-1, 1) * spread * 0.5
            m = ((yy - cy - dy) / (ry * s)) ** 2 + ((xx - cx - dx) / (rx * s)) ** 2 <= 1.0
            ys, xs = np.nonzero(m)
            box = [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]
            shapes.append((rle_encode(m), box, float(m.sum())))
        pool.append((int(rng.integers(1, CATS + 1)), shapes))
    return pool


def build_set(images, clusters, seed=0):
    rng = np.random.default_rng(seed)
    pool = build_pool(clusters, rng)
    gt = {"images": [{"id": i + 1, "height": H, "width": W} for i in range(images)],
          "categories": [{"id": c, "name": f"c{c}"} for c in range(1, CATS + 1)], "annotations": []}
    records = []
    for i in range(images):
        mine = rng.choice(clusters, size=int(np.clip(rng.poisson(7), 1, 15)), replace=False)
        for k in mine:
            cat, shapes = pool[k]
            seg, box, area = shapes[0]
            gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": i + 1, "category_id": cat,
                                      "iscrowd": int(rng.random() < 0.03), "segmentation": seg, "bbox": box, "area": area})
        near = rng.random(DETS) < 0.8
        which = np.where(near, rng.choice(mine, DETS), rng.integers(0, clusters, DETS))
        variant = rng.integers(0, 1 + VARIANTS, DETS)
        other = rng.random(DETS) < 0.15
        scores = rng.random(DETS)
        for j in range(DETS):
            cat, shapes = pool[which[j]]
            seg, box, _ = shapes[variant[j]]
            records.append({"image_id": i + 1, "category_id": int(rng.integers(1, CATS + 1)) if other[j] else cat,
                            "bbox": box, "score": float(scores[j]), "segmentation": seg})
    return gt, records


def same(a, b):
    return bool(all(a[k].tobytes() == b[k].tobytes() for k in ("precision", "recall", "scores", "stats")) and
                a["ious"]._flat.tobytes() == b["ious"]._flat.tobytes())


def timed_evaluate(ev, sync):
    sync()
    t0 = time.perf_counter()
    res = ev.evaluate()
    sync()
    return res, dict(ev.timings, total_s=time.perf_counter() - t0)


def one_type(gt, records, iou_type, iters, rehearse):
    from vnext_amd.evaluation import COCOEval
    from vnext_amd.ops import ap_match as M
    from vnext_amd.ops import video_iou as V
    out = {}
    kept = {}
    inner = COCOEval._match

    def keep_inputs(self, *args):                            # the flat arrays the matching sees, for the matchers below
        kept["args"] = args + (self.iou_thrs,)
        return inner(self, *args)
    COCOEval._match = keep_inputs
    try:
        if not rehearse:
            import torch
            launches = {"n": 0}
            counted = {"match_into": (M, 1), "pair_sums_device": (V, 1), "decode_strings_device": (V, 2)}
            originals = {name: getattr(mod, name) for name, (mod, _) in counted.items()}

            def counting(name, n):
                def call(*a, **k):
                    launches["n"] += n
                    return originals[name](*a, **k)
                return call
            ev = COCOEval(gt, iou_type, device="cuda").add(records)
            for name, (mod, n) in counted.items():
                setattr(mod, name, counting(name, n))
            try:
                dev_res, _ = timed_evaluate(ev, torch.cuda.synchronize)                  # warm-up, launches counted
            finally:
                for name, (mod, _) in counted.items():
                    setattr(mod, name, originals[name])
            runs = [timed_evaluate(ev, torch.cuda.synchronize)[1] for _ in range(iters)]
            out["device"] = {k: statistics.median(r[k] for r in runs) for k in
                             ("tables_s", "sums_s", "match_s", "accumulate_s", "total_s")}
            out["device"]["total_s_all"] = [r["total_s"] for r in runs]
            out["device"].update({k: runs[0][k] for k in ("problems", "detections", "ground_truths", "pairs", "matching")})
            out["launches"] = launches["n"]
            table = kept["args"][0]
            out["fallback"] = {"share_of_problems": 1.0 if runs[0]["host_fallback"] else 0.0,
                               "largest_G": int(table[:, 1].max()), "largest_D": int(table[:, 0].max()),
                               "limit_G": M.MAX_GT}
            # the kernel alone, device events
            up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).cuda()   # noqa: E731
            dts = (np.int64, np.float64, np.uint8, np.float64, np.float64, np.float64, np.float64)
            d_args = [up(a, dt) for a, dt in zip(kept["args"], dts)]
            m = M.ap_match(*d_args)
            status = torch.zeros(1, dtype=torch.int32, device="cuda")
            times = []
            for it in range(3 + 20):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                M.match_into(*d_args, m, status)
                b.record()
                b.synchronize()
                if it >= 3:
                    times.append(a.elapsed_time(b))
            assert int(status) == 0
            out["matchers"] = {"kernel_ms_median": statistics.median(times), "kernel_ms_all": times,
                               "timing": "device events around the one launch, outputs preallocated, 3 warm-up launches"}
        ev = COCOEval(gt, iou_type, device="cpu").add(records)
        cpu_res, out["cpu"] = timed_evaluate(ev, lambda: None)
        out["cpu"]["what"] = "this package's own host route (numpy tables and sums, match_host), not pycocotools"
        t0 = time.perf_counter()
        vec = M.match_vectorised(*kept["args"])
        out.setdefault("matchers", {})["match_vectorised_s"] = time.perf_counter() - t0
        out["matchers"]["match_host_s"] = out["cpu"]["match_s"]
        if rehearse:
            host = M.match_host(*kept["args"])
            assert all((getattr(vec, n) == getattr(host, n)).all() for n in ("dt_match", "dt_ignore", "gt_match", "gt_ignore"))
        if not rehearse:
            out["identical_arrays"] = same(dev_res, cpu_res)
            dm = m.numpy()
            out["matchers"]["vectorised_equals_kernel"] = bool(all(
                (getattr(vec, n) == getattr(dm, n)).all() for n in ("dt_match", "dt_ignore", "gt_match", "gt_ignore")))
        out["AP"], out["AP50"], out["AR100"] = cpu_res["AP"], cpu_res["AP50"], cpu_res["AR100"]
    finally:
        COCOEval._match = inner
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--clusters", type=int, default=240)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--types", default="bbox,segm")
    ap.add_argument("--rehearse", action="store_true", help="the cpu route alone, no GPU, nothing written")
    a = ap.parse_args()
    res = {"images": a.images, "size": [H, W], "categories": CATS, "detections_per_image": DETS,
           "mask_pool": {"clusters": a.clusters, "shapes_per_cluster": 1 + VARIANTS}}
    if not a.rehearse:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("time_coco_eval.py: needs an MI355X (no CPU fallback for timings)")
        res["device"] = torch.cuda.get_device_name(0)
    t0 = time.perf_counter()
    gt, records = build_set(a.images, a.clusters)
    res["ground_truths_per_image"] = len(gt["annotations"]) / a.images
    print(f"set built in {time.perf_counter() - t0:.1f} s: {len(records)} records, {len(gt['annotations'])} annotations",
          flush=True)
    for t in a.types.split(","):
        res[t] = one_type(gt, records, t, a.iters, a.rehearse)
        print(t, json.dumps(res[t])[:600], flush=True)
    text = json.dumps(res, indent=1)
    if a.rehearse:
        print("rehearsal only: nothing measured, nothing written")
        return
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
