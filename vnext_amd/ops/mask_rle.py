"""COCO RLE strings of result masks, encoded on the device (vnext_amd/csrc/mask_rle.hip).

A YTVIS results file holds one `{"size": [h, w], "counts": str}` per (instance, frame): the compressed RLE of
vnext_amd/utils/ytvis_json.py `rle_encode` (pycocotools' rleEncode + rleToString).  The models produce those masks from
stride-4 logits as

    m = F.interpolate(logits, size=(h * s, w * s), mode="bilinear", align_corners=False).sigmoid()
    m = F.interpolate(m[:, :, :ih, :iw], size=(oh, ow), mode="nearest") > 0.5

and `encode_logits` returns the strings of those masks without forming them: per output pixel the kernel takes the
nearest index on the crop and ONE bilinear sample of the logit map there, and sets the bit where that value is > 0 (=
sigmoid > 0.5 outside a band of |value| within fp32 rounding of 0).  Two launches (measure the string lengths, write
the strings at their offsets); the lengths' scan and the one device-to-host copy of the byte arena are the only host
work.  `encode_masks` is the same encoder on uint8 / bool masks.

CUDA tensors take the kernel; CPU tensors take the host expression above and `rle_encode` (the reference the tests
compare against; it also keeps the CPU model tests running).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from ..utils.ytvis_json import rle_encode
from .mask_dense import host_masks


def _records(lengths_end, arena, oh, ow):
    """int64 string ends [M] + the byte arena (host) -> [{"size", "counts"}]"""
    text = arena.tobytes().decode("ascii")
    ends = lengths_end.tolist()
    starts = [0] + ends[:-1]
    return [{"size": [oh, ow], "counts": text[a:b]} for a, b in zip(starts, ends)]


def _encode_device(mode, data, M, h, w, stride, ih, iw, oh, ow):
    lib = _lib.lib()
    if M == 0:
        return []
    dev = data.device
    with torch.cuda.device(dev):
        stream = _lib.current_stream(data)
        lengths = torch.empty(M, dtype=torch.int64, device=dev)
        _lib.check(lib.vnx_mask_rle_measure(mode, data.data_ptr(), M, h, w, stride, ih, iw, oh, ow,
                                            lengths.data_ptr(), stream))
        ends = lengths.cumsum(0)
        ends_host = ends.cpu()                          # sizes the arena: the call's one synchronisation before the copy
        total = int(ends_host[-1])
        arena = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        offsets = ends - lengths
        _lib.check(lib.vnx_mask_rle_write(mode, data.data_ptr(), M, h, w, stride, ih, iw, oh, ow, offsets.data_ptr(),
                                          arena.data_ptr(), total, stream))
        host = arena[:total].cpu()
    return _records(ends_host.numpy(), host.numpy(), oh, ow)


def _sizes(image_size, out_size):
    ih, iw = (int(v) for v in image_size)
    oh, ow = (int(v) for v in out_size)
    return ih, iw, oh, ow


def encode_logits(logits, stride, image_size, out_size):
    """logits [M, h, w] (mask logits, one map per (instance, frame)), the upsampling factor `stride`, the crop
    `image_size` (ih, iw) on the [h * stride, w * stride] grid and the output size (oh, ow) -> M dicts
    {"size": [oh, ow], "counts": str}, the RLE of the thresholded masks the host expression forms."""
    if logits.dim() != 3:
        raise ValueError(f"encode_logits: logits must be [M, h, w], got {tuple(logits.shape)}")
    M, h, w = (int(v) for v in logits.shape)
    ih, iw, oh, ow = _sizes(image_size, out_size)
    stride = int(stride)
    if not logits.is_cuda:
        if M == 0:
            return []
        return [rle_encode(x) for x in host_masks(logits, stride, (ih, iw), (oh, ow)).numpy()]
    return _encode_device(_lib.MASK_RLE_LOGITS, logits.float().contiguous(), M, h, w, stride, ih, iw, oh, ow)


def encode_masks(masks):
    """masks [M, H, W] bool / uint8 (a pixel is set when non-zero) -> M dicts {"size": [H, W], "counts": str}."""
    if masks.dim() != 3:
        raise ValueError(f"encode_masks: masks must be [M, H, W], got {tuple(masks.shape)}")
    M, H, W = (int(v) for v in masks.shape)
    if not masks.is_cuda:
        return [rle_encode(np.asarray(x != 0, dtype=np.uint8)) for x in masks.numpy()]
    data = (masks != 0).to(torch.uint8).contiguous() if masks.dtype not in (torch.bool, torch.uint8) else \
        masks.contiguous().view(torch.uint8)
    return _encode_device(_lib.MASK_RLE_BINARY, data, M, 0, 0, 0, 0, 0, H, W)
