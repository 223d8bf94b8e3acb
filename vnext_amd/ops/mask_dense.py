"""Dense result masks from the mask logits in one device pass (vnext_amd/csrc/mask_dense.hip).

`model(inputs)` returns full-resolution masks.  The models form them from stride-s logits as

    m = F.interpolate(logits, size=(h * s, w * s), mode="bilinear", align_corners=False).sigmoid()
    m = F.interpolate(m[:, :, :ih, :iw], size=(oh, ow), mode="nearest") > 0.5

which writes two fp32 tensors of the upsampled size before any bit exists.  `masks_from_logits` returns those masks
without the intermediates: per output pixel the kernel takes the nearest index on the crop and ONE bilinear sample of the
logit map there -- the device code `ops.mask_rle.encode_logits` runs (csrc/mask_sample.h), so the two agree on every pixel.

The zero band.  The device bit is `value > 0`, not `sigmoid(value) > 0.5`: the two differ only where |value| is within
fp32 rounding of 0 (the kernel's single sample and ATen's two passes round differently there, and `sigmoid` rounds
values below about 6e-8 to exactly 0.5).  Exactly as for `encode_logits`.

Two forms.  `bits=False`: bool [M, oh, ow] (one byte per pixel; what the models return).  `bits=True`: uint8
[M, oh, pitch], pitch = 8 * ceil(ow / 64), pixel x in bit x & 7 of byte x >> 3 (`np.packbits(..., bitorder="little")`),
padding zero -- for callers that store or ship one bit per pixel; `unpack_bits` is its inverse.  A caller that wants bool
masks on the host should copy the byte form: unpacking on the host costs more than the copy it saves.

CUDA tensors take the kernel; CPU tensors take the host expression above (the reference the tests compare against; it
also keeps the CPU model tests running).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from .. import _lib

CALLS = {"masks_from_logits": 0}           # device launches (tests count them)


def bits_pitch(width: int) -> int:
    """bytes per row of the `bits` form"""
    return 8 * ((int(width) + 63) // 64)


def host_masks(logits, stride, image_size, out_size):
    """The models' eager chain -> bool [M, oh, ow] (any device)."""
    h, w = logits.shape[-2:]
    m = F.interpolate(logits.float()[:, None], size=(h * stride, w * stride), mode="bilinear",
                      align_corners=False).sigmoid()
    return (F.interpolate(m[:, :, :image_size[0], :image_size[1]], size=tuple(out_size), mode="nearest") > 0.5)[:, 0]


def pack_bits(masks):
    """bool [M, oh, ow] on the host -> uint8 [M, oh, pitch] (the `bits` form)"""
    M, oh, ow = masks.shape
    out = np.zeros((M, oh, bits_pitch(ow)), dtype=np.uint8)
    out[:, :, :(ow + 7) // 8] = np.packbits(masks.numpy(), axis=-1, bitorder="little")
    return torch.from_numpy(out)


def unpack_bits(packed, width):
    """uint8 [..., pitch] of the `bits` form (any device) -> bool [..., width]"""
    if packed.shape[-1] * 8 < width:
        raise ValueError(f"unpack_bits: rows of {packed.shape[-1]} bytes hold fewer than {width} pixels")
    shifts = torch.arange(8, dtype=torch.uint8, device=packed.device)
    bits = (packed.to(torch.uint8)[..., None] >> shifts) & 1
    return bits.flatten(-2)[..., :width].to(torch.bool)


def masks_from_logits(logits, stride, image_size, out_size, bits=False):
    """logits [M, h, w] (mask logits, one map per (instance, frame)), the upsampling factor `stride`, the crop
    `image_size` (ih, iw) on the [h * stride, w * stride] grid and the output size (oh, ow) -> the thresholded masks the
    host expression forms, on the logits' device: bool [M, oh, ow], or with `bits` uint8 [M, oh, 8 * ceil(ow / 64)].

    On the device a pixel is set where its bilinear value is > 0; the host expression sets it where sigmoid(value) > 0.5.
    The two may differ where |value| is within fp32 rounding of 0 (the zero band), and nowhere else."""
    if logits.dim() != 3:
        raise ValueError(f"masks_from_logits: logits must be [M, h, w], got {tuple(logits.shape)}")
    M, h, w = (int(v) for v in logits.shape)
    ih, iw = (int(v) for v in image_size)
    oh, ow = (int(v) for v in out_size)
    stride = int(stride)
    if not logits.is_cuda:
        m = host_masks(logits, stride, (ih, iw), (oh, ow)) if M else torch.zeros((0, oh, ow), dtype=torch.bool)
        return pack_bits(m) if bits else m
    data = logits.float().contiguous()
    shape = (M, oh, bits_pitch(ow)) if bits else (M, oh, ow)
    out = torch.empty(shape, dtype=torch.uint8, device=data.device)
    with torch.cuda.device(data.device):
        _lib.check(_lib.lib().vnx_mask_dense(_lib.MASK_DENSE_BITS if bits else _lib.MASK_DENSE_U8, data.data_ptr(), M, h, w,
                                             stride, ih, iw, oh, ow, out.data_ptr(), out.numel(),
                                             _lib.current_stream(data)))
    CALLS["masks_from_logits"] += 1
    return out if bits else out.view(torch.bool)
