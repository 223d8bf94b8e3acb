"""Time polygons -> run tables (vnext_amd/ops/poly_rle.py, vnext_amd/csrc/poly_rle.hip) on a synthetic set at the scale of
COCO val2017: 36 000 objects of 1 - 3 polygons with 10 - 200 vertices on 480 x 640 canvases.  MI355X only.

(a) one `polygons_to_runs` call: the kernel launch alone (tables on the device; HIP-event region, median of the rounds), the
    whole call from Python lists to device tables (host wall clock: planning, packing, the upload and the launch), and the
    host route (`device="cpu"`) on a sample of the objects, scaled.
(b) `COCOEval(polygons=True).evaluate()` on a document with these polygons as ground truth, beside the same ground truth
    pre-converted to RLE; one detection per ground truth (its own mask, a random score).

Nothing is asserted about the times: the parent commit has no polygon path to compare with.  The device tables are compared
with the host's on the sample.

    python tools/time_poly_rle.py [--out FILE.json] [--objects N] [--rounds N] [--host-sample N]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vnext_amd import _lib  # noqa: E402
from vnext_amd.evaluation import COCOEval  # noqa: E402
from vnext_amd.ops import poly_rle as P  # noqa: E402

DEV = "cuda:0"
H, W = 480, 640


def workload(n, seed=0):
    rng = np.random.default_rng(seed)
    objects = []
    for _ in range(n):
        polys = []
        for _ in range(int(rng.integers(1, 4))):
            k = int(rng.integers(10, 201))
            th = np.sort(rng.uniform(0, 2 * np.pi, k))
            r = rng.uniform(8, 110) * (1 + 0.15 * np.sin(rng.integers(2, 9) * th + rng.uniform(0, 6)))
            xy = np.empty(2 * k)
            xy[0::2] = rng.uniform(0, W) + r * np.cos(th)
            xy[1::2] = rng.uniform(0, H) + r * np.sin(th)
            polys.append(np.round(xy, 2).tolist())               # COCO stores two decimals
        objects.append(polys)
    return objects


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)),
            "rounds_ms": [float(v) for v in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_rle.json"))
    ap.add_argument("--objects", type=int, default=36000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--host-sample", type=int, default=400)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "an MI355X is needed"
    objects = workload(args.objects)
    sizes = [(H, W)] * len(objects)

    # ---- (a) the op ----
    t0 = time.perf_counter()
    planned = P.plan_objects(objects, sizes)
    plan_s = time.perf_counter() - t0
    polys, slots, fits = planned
    dev_polys = [ps if fits[m] else [] for m, ps in enumerate(polys)]
    coords, prow, orow, total = P.pack_tables(dev_polys, sizes, np.where(fits, slots, 1))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)          # noqa: E731
    c, p, o = up(coords), up(prow), up(orow)
    for _ in range(3):
        tables, status = P.poly_rle_device(c, p, o, total)
    torch.cuda.synchronize()
    kernel_ms = []
    for _ in range(args.rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tables, status = P.poly_rle_device(c, p, o, total)
        b.record()
        torch.cuda.synchronize()
        kernel_ms.append(a.elapsed_time(b))
    assert not status.cpu().numpy().any()
    call_ms = []
    for _ in range(max(3, args.rounds // 3)):
        t0 = time.perf_counter()
        tables = P.polygons_to_runs(objects, sizes, device=DEV)
        torch.cuda.synchronize()
        call_ms.append((time.perf_counter() - t0) * 1e3)
    sample = np.linspace(0, len(objects) - 1, min(args.host_sample, len(objects))).astype(int)
    t0 = time.perf_counter()
    host = P.polygons_to_runs([objects[i] for i in sample], [sizes[i] for i in sample])
    host_s = time.perf_counter() - t0
    got = tables.numpy()
    equal = all(np.array_equal(got.ends[got.rows[i, 0]:got.rows[i, 0] + got.rows[i, 1]],
                               host.ends[host.rows[j, 0]:host.rows[j, 0] + host.rows[j, 1]])
                and got.rows[i, 3] == host.rows[j, 3] for j, i in enumerate(sample))
    runs = int(got.rows[:, 1].sum())
    out = {"device": torch.cuda.get_device_name(0), "objects": len(objects), "polygons": int(len(prow)),
           "vertices": int(len(coords) // 2), "canvas": [H, W], "objects_on_the_host_route": int((~fits).sum()),
           "run_slots": int(total), "runs": runs, "rounds": args.rounds,
           "caps": {"vertices": _lib.POLY_RLE_MAX_VERTICES, "crossings": _lib.POLY_RLE_MAX_CROSSINGS,
                    "points": _lib.POLY_RLE_MAX_POINTS, "polygons": _lib.POLY_RLE_MAX_POLYGONS},
           "kernel_event_region": stats(kernel_ms), "polygons_to_runs_wall_clock": stats(call_ms),
           "host_planning_s": plan_s, "host_route_sample": {"objects": int(len(sample)), "seconds": host_s,
                                                            "scaled_to_all_objects_s": host_s * len(objects) / len(sample)},
           "device_equals_host_on_the_sample": bool(equal)}

    # ---- (b) the evaluator ----
    per_image = 8
    images = [{"id": i + 1, "height": H, "width": W} for i in range((len(objects) + per_image - 1) // per_image)]
    cats = [{"id": k + 1, "name": f"c{k + 1}"} for k in range(80)]
    rng = np.random.default_rng(1)
    cat_of = rng.integers(1, 81, len(objects))
    rle = [{"size": [H, W], "counts": np.diff(got.ends[r[0]:r[0] + r[1]], prepend=0).tolist()} for r in got.rows]
    base = [{"id": m + 1, "image_id": m // per_image + 1, "category_id": int(cat_of[m]), "iscrowd": 0,
             "area": float(got.rows[m, 3]), "bbox": [0.0, 0.0, 1.0, 1.0]} for m in range(len(objects))]
    gt_poly = {"images": images, "categories": cats, "annotations": [dict(a, segmentation=objects[m]) for m, a in enumerate(base)]}
    gt_rle = {"images": images, "categories": cats, "annotations": [dict(a, segmentation=rle[m]) for m, a in enumerate(base)]}
    scores = rng.random(len(objects))
    dt = [{"image_id": a["image_id"], "category_id": a["category_id"], "score": float(scores[m]), "segmentation": rle[m]}
          for m, a in enumerate(base)]
    ev = {}
    for name, gt, kw in (("rle_ground_truth", gt_rle, {}), ("polygon_ground_truth", gt_poly, {"polygons": True})):
        ms, res = [], None
        for _ in range(3):
            t0 = time.perf_counter()
            e = COCOEval(gt, "segm", device=DEV, **kw).add(dt)
            res = e.evaluate()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        ev[name] = {"evaluate_wall_clock": stats(ms), "AP": float(res["AP"]), "timings": e.timings}
    out["coco_eval_segm"] = ev
    out["timing"] = ("kernel: HIP events around one vnx_poly_rle launch with its four output allocations, tables resident; "
                     "polygons_to_runs: Python lists to device tables, host wall clock to a device synchronise; the host "
                     "route on an evenly spaced sample, scaled; COCOEval: construction + add + evaluate, three rounds each. "
                     "No time is asserted: the parent commit has no polygon path")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "coco_eval_segm"}, indent=1))
    print({k: (v["evaluate_wall_clock"]["median_ms"], v["AP"]) for k, v in ev.items()})


if __name__ == "__main__":
    main()
