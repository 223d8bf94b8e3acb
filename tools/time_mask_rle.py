"""Time the YTVIS output stage: mask logits -> COCO RLE strings.  MI355X only.

  (a) the device encoder alone (vnext_amd/ops/mask_rle.py encode_logits): M masks of h x w logits -> out_h x out_w,
      median of device-event times; `--encoder-only` runs just this leg (for a rocprofv3 --kernel-trace --stats run)
  (b) the output stage end to end on the same logits: the host path (bilinear + sigmoid + crop + nearest + > 0.5 on the
      device, `.cpu()` of the bool masks, ytvis_json.rle_encode per mask; copy and encoding timed apart) against
      encode_logits (two launches, one scan, one copy of the strings, the Python str split)
  (c) model level: `ytvis_results(video)` against `instances_to_coco_json_video(video, model(video))` for IDOL R50 on
      36 frames at 720p (bench.py's idol_video_inference_720p input) and SeqFormer R50 on T = 5 at 720p.  Random-init
      weights keep few or degenerate masks: (a) and (b) are the representative figures.

    python tools/time_mask_rle.py [--out FILE.json] [--encoder-only] [--skip-models]
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

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def logit_field(M, h, w, device, seed=0):
    """Mask-like logits: 2-6 Gaussian blobs per map, an offset and unit noise (a few thousand runs per 720p mask)."""
    g = torch.Generator(device=device).manual_seed(seed)
    yy = torch.arange(h, device=device, dtype=torch.float32)[None, :, None]
    xx = torch.arange(w, device=device, dtype=torch.float32)[None, None, :]
    out = torch.randn(M, h, w, device=device, generator=g) - 2.0
    for _ in range(4):
        cy = torch.rand(M, 1, 1, device=device, generator=g) * h
        cx = torch.rand(M, 1, 1, device=device, generator=g) * w
        r = 4 + torch.rand(M, 1, 1, device=device, generator=g) * (h / 5)
        on = (torch.rand(M, 1, 1, device=device, generator=g) > 0.3).float()
        out += on * 9 * torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
    return out.contiguous()


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


def wall_ms(fn, iters, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times), times


def encoder_leg(M, h, w, stride, out_size, iters, dev):
    from vnext_amd import _lib
    from vnext_amd.ops.mask_rle import encode_logits
    from vnext_amd.utils.ytvis_json import string_to_counts
    logits = logit_field(M, h, w, dev)
    image = (h * stride, w * stride)
    rles = encode_logits(logits, stride, image, out_size)
    runs = [len(string_to_counts(r["counts"])) for r in rles[:: max(1, M // 24)]]
    # the two launches and the scan between them, with the arena preallocated (what a captured graph would replay)
    lib = _lib.lib()
    stream = _lib.current_stream(logits)
    lengths = torch.empty(M, dtype=torch.int64, device=dev)
    total = sum(len(r["counts"]) for r in rles)
    arena = torch.empty(total, dtype=torch.uint8, device=dev)
    args = (_lib.MASK_RLE_LOGITS, logits.data_ptr(), M, h, w, stride, image[0], image[1], out_size[0], out_size[1])

    def kernels():
        _lib.check(lib.vnx_mask_rle_measure(*args, lengths.data_ptr(), stream))
        ends = lengths.cumsum(0)
        _lib.check(lib.vnx_mask_rle_write(*args, (ends - lengths).data_ptr(), arena.data_ptr(), total, stream))
    ms_k, all_k = event_ms(kernels, iters)
    ms_call, all_call = event_ms(lambda: encode_logits(logits, stride, image, out_size), iters)
    px = M * out_size[0] * out_size[1]
    return logits, {
        "masks": M, "logits": [h, w], "stride": stride, "out": list(out_size),
        "runs_per_mask_sampled": {"min": min(runs), "median": statistics.median(runs), "max": max(runs)},
        "string_bytes_total": total,
        "kernels_ms_median": ms_k, "kernels_ms_all": all_k,
        "encode_logits_ms_median": ms_call, "encode_logits_ms_all": all_call,
        "masks_per_s": M / (ms_call * 1e-3), "output_pixels_per_s": px / (ms_call * 1e-3),
        "timing": "device events around the call; kernels_ms = measure + cumsum + write launches only, "
                  "encode_logits_ms = the op end to end (launches, scan, total copy, arena copy, str split)"}


def output_stage_leg(logits, stride, out_size, iters):
    from vnext_amd.ops.mask_rle import encode_logits
    from vnext_amd.utils.ytvis_json import rle_encode
    M, h, w = logits.shape
    image = (h * stride, w * stride)

    def device_masks():
        m = F.interpolate(logits[:, None], size=(h * stride, w * stride), mode="bilinear", align_corners=False).sigmoid()
        return (F.interpolate(m[:, :, :image[0], :image[1]], size=out_size, mode="nearest") > 0.5)[:, 0]
    t_int, t_copy, t_enc, t_host = [], [], [], []
    for i in range(iters + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = device_masks()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        host = [x for x in m.cpu()]                      # the models' `.cpu()` of the bool masks
        t2 = time.perf_counter()
        recs = [rle_encode(x.numpy()) for x in host]
        t3 = time.perf_counter()
        if i:
            t_int.append(1e3 * (t1 - t0)); t_copy.append(1e3 * (t2 - t1)); t_enc.append(1e3 * (t3 - t2))
            t_host.append(1e3 * (t3 - t0))
    ms_dev, all_dev = wall_ms(lambda: encode_logits(logits, stride, image, out_size), iters)
    same = encode_logits(logits, stride, image, out_size) == recs
    return {"host_path_ms_median": statistics.median(t_host),
            "host_interpolate_ms_median": statistics.median(t_int), "host_copy_ms_median": statistics.median(t_copy),
            "host_encode_ms_median": statistics.median(t_enc), "host_path_ms_all": t_host,
            "device_path_ms_median": ms_dev, "device_path_ms_all": all_dev,
            "speedup": statistics.median(t_host) / ms_dev, "identical_strings": bool(same),
            "timing": "host clock, each stage ending in a synchronise; both paths return the same Python records"}


def model_leg(iters, dev):
    import vnext_amd.models  # noqa: F401  (registers the meta-architectures)
    from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg
    from vnext_amd.utils.ytvis_json import instances_to_coco_json_video
    out = {}
    g = torch.Generator(device=dev).manual_seed(1)
    model = build_model(get_idol_cfg(**{"MODEL.DEVICE": str(dev)})).eval()
    video = [{"video_id": 1, "image": [torch.rand(3, 720, 1280, device=dev, generator=g) * 255 for _ in range(36)],
              "height": 720, "width": 1280}]
    out["idol_36x720p"] = _model_pair(model, video, iters, instances_to_coco_json_video)
    del model
    torch.cuda.empty_cache()
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": str(dev)})).eval()
    clip = [{"video_id": 1, "image": [torch.rand(3, 720, 1280, device=dev, generator=g) * 255 for _ in range(5)],
             "height": 720, "width": 1280}]
    out["seqformer_T5_720p"] = _model_pair(model, clip, iters, instances_to_coco_json_video)
    out["note"] = "random-init weights: few or degenerate masks; (a) and (b) are the representative figures"
    return out


def _model_pair(model, video, iters, writer):
    recs = model.ytvis_results(video)
    ms_host, _ = wall_ms(lambda: writer(video, model(video)), iters)
    ms_dev, _ = wall_ms(lambda: model.ytvis_results(video), iters)
    return {"records": len(recs), "segmentations": sum(len(r["segmentations"]) for r in recs),
            "model_then_host_writer_ms_median": ms_host, "ytvis_results_ms_median": ms_dev,
            "timing": "host clock around the whole call, ending in a synchronise"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--masks", type=int, default=360)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--encoder-only", action="store_true")
    ap.add_argument("--skip-models", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mask_rle.py: needs an MI355X (no CPU fallback for timings)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0)}
    logits, res["a_encoder"] = encoder_leg(a.masks, 180, 320, 4, (720, 1280), a.iters, dev)
    if not a.encoder_only:
        res["b_output_stage"] = output_stage_leg(logits, 4, (720, 1280), max(3, a.iters // 2))
        if not a.skip_models:
            res["c_models"] = model_leg(3, dev)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
