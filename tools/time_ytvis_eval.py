"""Time the local YTVIS evaluator at a realistic size.  MI355X only.

A synthetic set: `--videos` videos of 36 frames at 720 x 1280, 100 detections and `--gts` ground truths per video in
one category each, masks of a few ellipses (a few hundred runs), drawn and RLE-encoded on the device
(vnext_amd/ops/mask_rle.py encode_masks).  Reported:

  decode_ms    the two launches of the run-table decode (vnx_rle_runs_measure / _write) and the scan between them, over
               every string of the set, arenas preallocated; median of device-event times
  sums_ms      vnx_video_iou_sums over every (detection, ground truth) pair of the set; device events
  evaluate     YTVISEval(device="cuda").evaluate() by stage on the host clock (tables = flat state + upload + decode,
               sums = upload + kernel + copy back, matching, accumulation)
  numpy_path   the same evaluate() on THIS PACKAGE'S OWN numpy path (device="cpu": string decode and pair sums in
               numpy / Python) -- not the reference's evaluator, which needs pycocotools and cannot run here; both paths
               must return identical arrays

    python tools/time_ytvis_eval.py [--videos 4] [--gts 4] [--out profiles/ytvis_eval.json]
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
import torch  # noqa: E402

H, W, FRAMES, DETS = 720, 1280, 36, 100


def event_ms(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), times


def track_strings(n_tracks, anchors, jitter, dev, g):
    """n_tracks tracks of FRAMES ellipse-cluster masks around `anchors` [n_tracks, 2] -> [[str] * FRAMES] * n_tracks"""
    from vnext_amd.ops.mask_rle import encode_masks
    yy = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    xx = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    out = []
    for t in range(n_tracks):
        m = torch.zeros(FRAMES, H, W, dtype=torch.bool, device=dev)
        vel = (torch.rand(2, device=dev, generator=g) - 0.5) * 8
        f = torch.arange(FRAMES, device=dev, dtype=torch.float32)[:, None, None]
        for _ in range(3):
            off = (torch.rand(2, device=dev, generator=g) - 0.5) * jitter
            ry, rx = (40 + torch.rand(2, device=dev, generator=g) * 120).tolist()
            cy, cx = anchors[t, 0] + off[0] + vel[0] * f, anchors[t, 1] + off[1] + vel[1] * f
            m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        out.append([r["counts"] for r in encode_masks(m)])
    return out


def build_set(videos, gts, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    gt = {"videos": [], "categories": [{"id": 1, "name": "object"}], "annotations": []}
    records = []
    for v in range(1, videos + 1):
        gt["videos"].append({"id": v, "height": H, "width": W, "length": FRAMES})
        anchors = torch.rand(gts, 2, device=dev, generator=g) * torch.tensor([H, W], device=dev)
        for i, track in enumerate(track_strings(gts, anchors, 0.0, dev, g)):
            segs = [{"size": [H, W], "counts": s} for s in track]
            gt["annotations"].append({"id": len(gt["annotations"]) + 1, "video_id": v, "category_id": 1, "iscrowd": 0,
                                      "segmentations": segs, "areas": [1.0] * FRAMES})
        det_anchor = anchors[torch.arange(DETS, device=dev) % gts]
        scores = torch.rand(DETS, device=dev, generator=g).tolist()
        for i, track in enumerate(track_strings(DETS, det_anchor, 160.0, dev, g)):
            records.append({"video_id": v, "category_id": 1, "score": scores[i],
                            "segmentations": [{"size": [H, W], "counts": s} for s in track]})
    return gt, records


def kernel_legs(gt, records, iters, dev):
    from vnext_amd import _lib
    from vnext_amd.ops import video_iou as V
    from vnext_amd.utils.ytvis_json import string_to_counts
    strings = [s["counts"] for a in gt["annotations"] for s in a["segmentations"]]
    n_gt = len(strings)
    strings += [s["counts"] for r in records for s in r["segmentations"]]
    arena, offsets, lengths = V._string_arena(strings)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    d_arena, d_off, d_len = up(arena), up(offsets), up(lengths)
    d_px = torch.full((len(strings),), H * W, dtype=torch.int32, device=dev)
    tables, status = V.decode_strings_device(d_arena, d_off, d_len, d_px)
    assert not bool(status.any())
    lib = _lib.lib()
    M, total = len(strings), int(tables.ends.shape[0])
    runs = torch.empty(M, dtype=torch.int32, device=dev)
    ends, ones = torch.empty(total, dtype=torch.int32, device=dev), torch.empty(total, dtype=torch.int32, device=dev)
    rows, st = torch.empty(M, 4, dtype=torch.int32, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
    stream = _lib.current_stream(runs)

    def decode():
        _lib.check(lib.vnx_rle_runs_measure(d_arena.data_ptr(), len(arena), d_off.data_ptr(), d_len.data_ptr(), M,
                                            runs.data_ptr(), stream))
        run_off = (runs.cumsum(0, dtype=torch.int64) - runs).to(torch.int32)
        _lib.check(lib.vnx_rle_runs_write(d_arena.data_ptr(), len(arena), d_off.data_ptr(), d_len.data_ptr(),
                                          d_px.data_ptr(), run_off.data_ptr(), runs.data_ptr(), M, ends.data_ptr(),
                                          ones.data_ptr(), total, rows.data_ptr(), st.data_ptr(), stream))
    decode_ms, decode_all = event_ms(decode, iters)
    assert torch.equal(ends, tables.ends) and torch.equal(rows, tables.rows)
    # tracks: the ground truths of every video first, then the detections; every pair of one video
    gts = n_gt // FRAMES // len(gt["videos"])
    tracks = np.stack((np.arange(M // FRAMES) * FRAMES, np.full(M // FRAMES, FRAMES)), 1).astype(np.int32)
    pairs = np.array([(n_gt // FRAMES + (v * DETS) + d, v * gts + j) for v in range(len(gt["videos"]))
                      for d in range(DETS) for j in range(gts)], dtype=np.int32)
    d_fm = torch.arange(M, dtype=torch.int32, device=dev)
    d_tr, d_pr = up(tracks), up(pairs)
    sums_ms, sums_all = event_ms(lambda: V.pair_sums_device(tables, d_fm, d_tr, d_pr), iters)
    sample = [len(string_to_counts(s)) for s in strings[:: max(1, M // 48)]]
    return {"strings": M, "string_bytes": int(len(arena)), "runs_total": total,
            "runs_per_mask_sampled": {"min": min(sample), "median": statistics.median(sample), "max": max(sample)},
            "decode_ms_median": decode_ms, "decode_ms_all": decode_all,
            "pairs": int(len(pairs)), "pair_frames": int(len(pairs)) * FRAMES,
            "sums_ms_median": sums_ms, "sums_ms_all": sums_all,
            "timing": "device events; decode = measure + scan + write with the arenas preallocated; sums = the one launch"}


def evaluate_legs(gt, records):
    from vnext_amd.evaluation import YTVISEval
    out, results = {}, {}
    for name, device in (("evaluate_cuda", "cuda"), ("numpy_path", "cpu")):
        ev = YTVISEval(gt, device=device).add(records)
        if device == "cuda":
            ev.evaluate()                                    # warm-up: library load, allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        results[name] = ev.evaluate()
        out[name] = dict(ev.timings, total_s=time.perf_counter() - t0)
    out["numpy_path"]["what"] = "this package's own numpy path (device='cpu'), not the reference's evaluator"
    a, b = results["evaluate_cuda"], results["numpy_path"]
    out["identical_arrays"] = bool(all((a[k] == b[k]).all() for k in ("precision", "recall", "scores", "stats")) and
                                   all((a["ious"][k] == b["ious"][k]).all() for k in a["ious"]))
    out["AP"] = a["AP"]
    out["timing"] = "host clock per stage of evaluate(): tables (upload + decode), sums (upload + kernel + copy back), " \
                    "matching, accumulation"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--videos", type=int, default=4)
    ap.add_argument("--gts", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ytvis_eval.py: needs an MI355X (no CPU fallback for timings)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "videos": a.videos, "frames": FRAMES, "size": [H, W],
           "detections_per_video": DETS, "ground_truths_per_video": a.gts}
    gt, records = build_set(a.videos, a.gts, dev)
    res["kernels"] = kernel_legs(gt, records, a.iters, dev)
    res["evaluate"] = evaluate_legs(gt, records)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
