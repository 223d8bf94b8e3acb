"""Write tests/golden/ytvis_eval.npz: a small synthetic YTVIS annotation set and result records, scored by the
reference's own evaluator (the YouTube-VIS cocoapi fork under
projects/InstMove/MinVIS_motion/minvis/data_video/datasets/ytvis_api: `YTVOS.loadRes` + `YTVOSeval`).

The reference's two modules are imported from a VNext checkout as they stand.  What they need and this machine lacks
is stood in for here: `pycocotools.mask` by tools/pycocotools_standin.py (numpy, on this repository's RLE functions),
`np.float` by `float`, matplotlib by an empty module when it is missing.  The fixture holds data only -- the two JSON
documents as strings, every `ious[(video, category)]`, per `evalImgs` entry `dtMatches` / `gtMatches` / `dtIgnore` /
`gtIgnore`, `precision`, `recall`, `scores`, `stats` and the area ranges used -- no reference text.  Rerunning gives
the same arrays.

    python tools/make_golden_ytvis_eval.py [--vnext /root/reference] [--out tests/golden/ytvis_eval.npz]
"""
from __future__ import annotations

import argparse
import contextlib
import copy
import importlib.util
import io
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from vnext_amd.utils.ytvis_json import rle_counts, rle_encode  # noqa: E402

API = "projects/InstMove/MinVIS_motion/minvis/data_video/datasets/ytvis_api"
# the reference's area ranges (128^2, 256^2 for 720p videos) scaled to masks of 24 x 40 and 37 x 53
AREA_RNG = [[0, 1e5 ** 2], [0, 150], [150, 450], [450, 1e5 ** 2]]
VIDEOS = [(1, 24, 40, 6), (2, 37, 53, 9), (3, 24, 40, 7), (4, 37, 53, 8)]          # id, height, width, frames
CATEGORIES = [(1, "person"), (2, "dog"), (3, "car")]
# ground truth: video, category, centre (y, x), velocity, radii, absent frames, crowd, uncompressed
OBJECTS = [
    (1, 1, (8, 8), (1.0, 3.0), (4, 5), (0,), 0, False),
    (1, 1, (14, 28), (0.5, -2.0), (7, 9), (), 0, True),
    (1, 2, (12, 20), (0.0, 0.5), (10, 16), (5,), 0, False),
    (2, 1, (18, 24), (0.3, 1.0), (14, 18), (), 0, False),
    (2, 1, (10, 38), (1.5, -1.0), (8, 12), (2,), 1, True),
    (2, 2, (30, 8), (-1.0, 2.0), (4, 4), (3, 4), 0, False),
    (2, 3, (12, 12), (1.0, 2.5), (9, 9), (), 0, True),
    (3, 1, (10, 12), (0.5, 2.0), (7, 8), (6,), 0, False),
    (3, 3, (16, 30), (-0.5, -1.5), (4, 5), (), 0, False),
    (4, 1, (20, 26), (-0.5, 0.5), (15, 17), (), 0, True),
    (4, 2, (14, 14), (1.0, 3.0), (9, 10), (0, 7), 0, False),
    (4, 3, (28, 40), (-1.0, -1.0), (4, 5), (), 0, False),
]
NO_DETECTIONS = {(4, 3)}                 # a (video, category) with ground truth and no detection
ONLY_DETECTIONS = (3, 2)                 # and one the other way round
CROWDED = (1, 1)                         # the (video, category) that gets more than 100 detections


def ellipse(h, w, cy, cx, ry, rx):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0


def build_dataset():
    """-> (annotation dict, result records): plain JSON-able Python"""
    rng = np.random.default_rng(20)
    sizes = {v: (h, w, t) for v, h, w, t in VIDEOS}
    gt = {"videos": [{"id": v, "height": h, "width": w, "length": t} for v, h, w, t in VIDEOS],
          "categories": [{"id": c, "name": n} for c, n in CATEGORIES], "annotations": []}
    records = []

    def track_masks(v, centre, vel, radii, absent, dy=0.0, dx=0.0, scale=1.0):
        h, w, t = sizes[v]
        return [None if f in absent else
                ellipse(h, w, centre[0] + vel[0] * f + dy, centre[1] + vel[1] * f + dx, radii[0] * scale, radii[1] * scale)
                for f in range(t)]

    def record(v, c, score, masks, empty_for_absent):
        h, w, _ = sizes[v]
        segs = []
        for m in masks:
            if m is None:
                segs.append(rle_encode(np.zeros((h, w), np.uint8)) if empty_for_absent else None)
            else:
                segs.append(rle_encode(m))
        records.append({"video_id": v, "score": score, "category_id": c, "segmentations": segs})

    for i, (v, c, centre, vel, radii, absent, crowd, uncompressed) in enumerate(OBJECTS):
        h, w, t = sizes[v]
        masks = track_masks(v, centre, vel, radii, absent)
        segs = [None if m is None else
                ({"size": [h, w], "counts": [int(x) for x in rle_counts(m)]} if uncompressed else rle_encode(m))
                for m in masks]
        gt["annotations"].append({"id": i + 1, "video_id": v, "category_id": c, "iscrowd": crowd, "segmentations": segs,
                                  "areas": [None if m is None else int(m.sum()) for m in masks]})
        if (v, c) in NO_DETECTIONS:
            continue
        for j in range(6):                               # detections around the object, from tight to loose
            spread = 0.12 * (j + 1)
            dy, dx = (rng.uniform(-1, 1, 2) * spread * np.array(radii)).tolist()
            scale = float(1 + rng.uniform(-1, 1) * spread * 0.5)
            gone = tuple(int(f) for f in rng.choice(t, size=int(rng.integers(0, 3)), replace=False)) if j % 2 else absent
            score = float(np.round(0.95 - 0.1 * j + rng.uniform(-0.15, 0.15), 2))
            record(v, c, score, track_masks(v, centre, vel, radii, gone, dy, dx, scale), empty_for_absent=j != 3)
    # false positives: ellipses that follow nothing, in every video; one (video, category) without ground truth
    for v, h, w, t in VIDEOS:
        for j in range(5):
            c = int(rng.integers(1, 4)) if (v, j) != (ONLY_DETECTIONS[0], 0) else ONLY_DETECTIONS[1]
            if (v, c) in NO_DETECTIONS:
                c = 1
            centre = (float(rng.uniform(4, h - 4)), float(rng.uniform(4, w - 4)))
            radii = (float(rng.uniform(3, h / 3)), float(rng.uniform(3, w / 3)))
            vel = tuple(rng.uniform(-1.5, 1.5, 2).tolist())
            record(v, c, float(np.round(rng.uniform(0.05, 0.7), 2)), track_masks(v, centre, vel, radii, ()), True)
    # one (video, category) with more than 100 detections, most of them low-score noise around its two objects
    v, c = CROWDED
    h, w, t = sizes[v]
    for j in range(100):
        o = OBJECTS[j % 2]
        dy, dx = (rng.uniform(-1.2, 1.2, 2) * np.array(o[4])).tolist()
        record(v, c, float(np.round(rng.uniform(0.01, 0.45), 2)),
               track_masks(v, o[2], o[3], o[4], (), dy, dx, float(rng.uniform(0.6, 1.4))), True)
    records[1]["score"] = records[0]["score"]            # two detections of one group with equal scores
    return gt, records


@contextlib.contextmanager
def reference_modules(vnext):
    """The reference's ytvos / ytvoseval modules, imported from the checkout with the stand-ins in place; on exit
    `sys.modules` and `np.float` are as they were (the tests call this inside a pytest process)."""
    names = ("pycocotools", "pycocotools.mask", "matplotlib", "matplotlib.pyplot", "matplotlib.collections",
             "matplotlib.patches")
    before = {n: sys.modules.get(n) for n in names}
    had_float = hasattr(np, "float")
    try:
        yield _load_reference(vnext)
    finally:
        for n, mod in before.items():
            if n.startswith("matplotlib") and not getattr(sys.modules.get(n), "_stand_in", False):
                continue                                 # the real matplotlib, imported on the way: it stays
            if mod is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = mod
        if not had_float and hasattr(np, "float"):
            del np.float


def _load_reference(vnext):
    import pycocotools_standin
    pkg = types.ModuleType("pycocotools")
    pkg.mask = pycocotools_standin
    sys.modules["pycocotools"], sys.modules["pycocotools.mask"] = pkg, pycocotools_standin
    if not hasattr(np, "float"):
        np.float = float
    try:
        import matplotlib.pyplot  # noqa: F401
        import matplotlib.collections  # noqa: F401
        import matplotlib.patches  # noqa: F401
    except Exception:
        for name, attrs in (("matplotlib", ()), ("matplotlib.pyplot", ()), ("matplotlib.collections", ("PatchCollection",)),
                            ("matplotlib.patches", ("Polygon",))):
            mod = types.ModuleType(name)
            mod._stand_in = True
            for a in attrs:
                setattr(mod, a, object)
            sys.modules[name] = mod
    mods = []
    for name in ("ytvos", "ytvoseval"):
        spec = importlib.util.spec_from_file_location("_ref_" + name, os.path.join(vnext, API, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


def generate(vnext):
    """-> the fixture as a dict of arrays"""
    gt, records = build_dataset()
    gt_json, dt_json = json.dumps(gt), json.dumps(records)
    with reference_modules(vnext) as (ytvos, ytvoseval), contextlib.redirect_stdout(io.StringIO()):
        api = ytvos.YTVOS()
        api.dataset = json.loads(gt_json)
        api.createIndex()
        res = api.loadRes(json.loads(dt_json))
        E = ytvoseval.YTVOSeval(api, res)
        E.params.areaRng = copy.deepcopy(AREA_RNG)
        E.evaluate()
        E.accumulate()
        E.summarize()
    fx = {"gt_json": np.array(gt_json), "dt_json": np.array(dt_json), "area_rng": np.array(AREA_RNG, dtype=np.float64),
          "vid_ids": np.array(E.params.vidIds, dtype=np.int64), "cat_ids": np.array(E.params.catIds, dtype=np.int64)}
    for (v, c), iou in E.ious.items():
        fx[f"ious_{v}_{c}"] = np.zeros(0) if isinstance(iou, list) else np.asarray(iou, dtype=np.float64)
    fx["eval_none"] = np.array([e is None for e in E.evalImgs])
    for n, e in enumerate(E.evalImgs):
        if e is not None:
            fx[f"ev{n}_dtm"] = np.asarray(e["dtMatches"], dtype=np.float64)
            fx[f"ev{n}_gtm"] = np.asarray(e["gtMatches"], dtype=np.float64)
            fx[f"ev{n}_dtig"] = np.asarray(e["dtIgnore"], dtype=bool)
            fx[f"ev{n}_gtig"] = np.asarray(e["gtIgnore"], dtype=np.int64)
    for k in ("precision", "recall", "scores"):
        fx[k] = np.asarray(E.eval[k], dtype=np.float64)
    fx["stats"] = np.asarray(E.stats, dtype=np.float64)
    return fx


def fixture_conditions(fx):
    """What the fixture must exercise -> {condition: bool}; checked here and asserted again by the test."""
    gt, recs = json.loads(str(fx["gt_json"])), json.loads(str(fx["dt_json"]))
    rng = fx["area_rng"]
    groups_gt, groups_dt = {}, {}
    for a in gt["annotations"]:
        groups_gt.setdefault((a["video_id"], a["category_id"]), []).append(a)
    for r in recs:
        groups_dt.setdefault((r["video_id"], r["category_id"]), []).append(r)

    def avg(a):
        l = [x for x in a["areas"] if x]
        return float(np.mean(l)) if l else 0.0
    ious = np.concatenate([fx[k].reshape(-1) for k in fx if k.startswith("ious_")])
    thrs = np.linspace(0.5, 0.95, 10)
    per_interval = [int(((ious > lo) & (ious < hi)).sum()) for lo, hi in zip(thrs[:-1], thrs[1:])]
    return {
        "0.2 < AP < 0.9": bool(0.2 < fx["stats"][0] < 0.9),
        "every area range holds a non-ignored ground truth": all(
            any(not a["iscrowd"] and lo <= avg(a) <= hi for a in gt["annotations"]) for lo, hi in rng),
        "every AP and AR of the summary is defined": bool((fx["stats"] > -1).all()),
        "a crowd ground truth": any(a["iscrowd"] for a in gt["annotations"]),
        "detections without ground truth": any(k not in groups_gt for k in groups_dt),
        "ground truth without detections": any(k not in groups_dt for k in groups_gt),
        "more than 100 detections in a group": any(len(v) > 100 for v in groups_dt.values()),
        "equal scores in a group": any(len({r["score"] for r in v}) < len(v) for v in groups_dt.values()),
        "absent frames in the ground truth": any(s is None for a in gt["annotations"] for s in a["segmentations"]),
        "absent frames in the results (None and the empty mask)":
            any(s is None for r in recs for s in r["segmentations"]) and
            any(s is not None and len(s["counts"]) <= 3 for r in recs for s in r["segmentations"]),
        "uncompressed and compressed ground truth": len({isinstance(s["counts"], list) for a in gt["annotations"]
                                                         for s in a["segmentations"] if s}) == 2,
        "three IoU values inside each of two threshold intervals": sum(n >= 3 for n in per_interval) >= 2,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vnext", default="/root/reference", help="root of a VNext checkout (the reference)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ytvis_eval.npz"))
    a = ap.parse_args()
    fx = generate(a.vnext)
    cond = fixture_conditions(fx)
    for k, ok in cond.items():
        print(("ok   " if ok else "FAIL ") + k)
    print("stats", np.round(fx["stats"], 4).tolist())
    if not all(cond.values()):
        raise SystemExit("the fixture does not meet its conditions; nothing written")
    np.savez_compressed(a.out, **fx)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
