"""uint8 frames to network inputs on the device (vnext_amd/csrc/ingest.hip).

Detectron2's mappers hand the models uint8 CHW frames on the CPU.  Instead of a float cast on the host, a pageable upload of
four times the bytes and a chain of small launches per frame and per pyramid level:

`stage_frames(frames, device) -> (pixels, table)`: the frames' bytes in ONE device buffer and an int32 table with a row
{byte offset of the frame's first plane, h, w} per frame.  CPU frames are packed into one pinned buffer (table first, each
frame's planes 16-byte aligned behind it) and cross the bus in one `non_blocking` copy; the buffer comes from torch's pinned
allocator, which holds the block back until the copy that reads it has finished.  uint8 frames already on the device: one
`cat` of their flattened planes and a small table upload.
`pack_upload(ints, uploads, nbytes, device, extra) -> (int32 views, pixels)`: that one buffer and one copy, for any list of
int32 tables in front of the frames; `resize.stage_sources` and `augment.stage_step` stage through it as well.
`padded_hw(sizes) -> (H, W)`: the largest (h, w), rounded up to multiples of 32 -- what `padded_size` of all three ops is.
`ingest_frames(pixels, table, B, H, W, mean, std, channels_last) -> (x, mask)`: x fp32 [B, 3, H, W] (contiguous or
channels-last) = (u - mean) / std inside each frame and 0 outside, mask bool [B, H, W] = True outside: one launch, no memset.
`level_constants(table, B, H, W, level_sizes, num_pos_feats, temperature) -> (masks, poss)`: per level the nearest-resized
padding mask [B, h, w] and `sine_position` of it, [B, 2 * num_pos_feats, h, w] as the permuted view of [B, h, w, C] the eager
function returns: one launch for all levels.

The kernels read the geometry from the table in device memory: the launches can be captured and replayed on other pixels and
other frame sizes of the same padded shape.  On the CPU both functions ARE the reference expression, evaluated by torch (as
`swin_glue.fused_applies` routes); on the GPU a position width the kernel does not have (num_pos_feats not a multiple of 4,
or above 128) or more than 8 levels takes the reference expression too.  `CALLS` counts the kernel launches made here.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch
import torch.nn.functional as F

from .. import _lib

CALLS = {"ingest_frames": 0, "level_constants": 0}      # launches through the C ABI (tests: the op ran / did not run)

_TABLES = {}


def applies(frames, device) -> bool:
    """All frames are uint8 [3, h, w] tensors (CPU or on `device`)."""
    return bool(frames) and all(torch.is_tensor(f) and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[0] == 3
                                and f.numel() > 0 and (not f.is_cuda or f.device == torch.device(device)) for f in frames)


def padded_hw(sizes):
    """(H, W): the largest of the (h, w) `sizes`, rounded up to multiples of 32"""
    H = max(int(s[0]) for s in sizes)
    W = max(int(s[1]) for s in sizes)
    return (H + 31) // 32 * 32, (W + 31) // 32 * 32


def padded_size(frames):
    """(H, W): the largest frame, rounded up to multiples of 32"""
    return padded_hw([f.shape[-2:] for f in frames])


def _align16(n: int) -> int:
    return (n + 15) // 16 * 16


def pack_upload(ints, uploads, nbytes: int, device, extra: int = 0):
    """int32 arrays, [(uint8 tensor, byte offset)] and the byte count of the pixel area -> (the arrays as int32 views on
    `device`, pixels uint8 [nbytes + extra]).  ONE host buffer -- the arrays back to back, padded to 16 bytes, then every
    tensor at its offset (the caller keeps them 16-byte aligned) -- pinned for a CUDA device, and ONE `non_blocking` copy.
    `extra` bytes behind the pixels are allocated on the device in the same block and not uploaded."""
    device = torch.device(device)
    cuts = np.cumsum([0] + [a.size for a in ints]).tolist()
    head = _align16(4 * cuts[-1])
    buf = torch.empty(head + nbytes, dtype=torch.uint8, pin_memory=device.type == "cuda")
    buf[:4 * cuts[-1]].view(torch.int32).copy_(torch.from_numpy(np.concatenate([a.reshape(-1) for a in ints])))
    for f, o in uploads:
        buf[head + o:head + o + f.numel()].view(f.shape).copy_(f)
    if extra:
        whole = torch.empty(head + nbytes + extra, dtype=torch.uint8, device=device)
        whole[:head + nbytes].copy_(buf, non_blocking=True)
    else:
        whole = buf.to(device, non_blocking=True)
    words = whole[:4 * cuts[-1]].view(torch.int32)
    return [words[a:b].view(arr.shape) for arr, a, b in zip(ints, cuts[:-1], cuts[1:])], whole[head:]


def stage_frames(frames, device):
    """uint8 [3, h, w] frames -> (pixels uint8 [bytes], table int32 [n, 3]) on `device`; see the module docstring."""
    on_device = frames[0].is_cuda
    rows, off = [], 0
    for f in frames:
        rows.append((off, f.shape[-2], f.shape[-1]))
        off += f.numel() if on_device else _align16(f.numel())
    table = np.array(rows, dtype=np.int32)
    if on_device:
        pixels = torch.cat([f.reshape(-1) for f in frames])
        return pixels, torch.from_numpy(table).pin_memory().to(device, non_blocking=True)
    (table,), pixels = pack_upload([table], [(f, o) for f, (o, _, _) in zip(frames, rows)], off, device)
    return pixels, table


def closed_form_embeds(h: int, w: int, vh: int, vw: int):
    """The two cumsums of `sine_position` for a mask whose valid pixels are the top-left vh x vw rectangle of h x w, in
    closed form (what the kernel computes): y_embed = min(y + 1, vh) on the valid columns and 0 elsewhere, x_embed likewise."""
    ys = torch.arange(1, h + 1).clamp(max=vh)[:, None] * (torch.arange(w) < vw)[None, :]
    xs = torch.arange(1, w + 1).clamp(max=vw)[None, :] * (torch.arange(h) < vh)[:, None]
    return ys.float(), xs.float()


def reference_ingest(pixels, table, B, H, W, mean, std, channels_last=False):
    """`ingest_frames` by torch: the models' eager normalise + pad, frame by frame"""
    mean = torch.as_tensor(mean, dtype=torch.float32, device=pixels.device).view(3, 1, 1)
    std = torch.as_tensor(std, dtype=torch.float32, device=pixels.device).view(3, 1, 1)
    x = torch.zeros(B, 3, H, W, dtype=torch.float32, device=pixels.device)
    mask = torch.ones(B, H, W, dtype=torch.bool, device=pixels.device)
    for i, (o, h, w) in enumerate(table.tolist()):
        f = pixels[o:o + 3 * h * w].view(3, h, w)
        x[i, :, :h, :w] = (f.to(torch.float32) - mean) / std
        mask[i, :h, :w] = False
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    return x, mask


def sine_position(mask, num_pos_feats=128, temperature=10000):
    """models/position_encoding.py:35-55 with normalize=True."""
    not_mask = ~mask
    y_embed = not_mask.cumsum(1, dtype=torch.float32)
    x_embed = not_mask.cumsum(2, dtype=torch.float32)
    eps, scale = 1e-6, 2 * math.pi
    y_embed = (y_embed - 0.5) / (y_embed[:, -1:, :] + eps) * scale
    x_embed = (x_embed - 0.5) / (x_embed[:, :, -1:] + eps) * scale
    dim_t = torch.arange(num_pos_feats, dtype=torch.float32, device=mask.device)
    dim_t = temperature ** (2 * (dim_t // 2) / num_pos_feats)
    pos_x = x_embed[:, :, :, None] / dim_t
    pos_y = y_embed[:, :, :, None] / dim_t
    pos_x = torch.stack((pos_x[..., 0::2].sin(), pos_x[..., 1::2].cos()), dim=4).flatten(3)
    pos_y = torch.stack((pos_y[..., 0::2].sin(), pos_y[..., 1::2].cos()), dim=4).flatten(3)
    return torch.cat((pos_y, pos_x), dim=3).permute(0, 3, 1, 2)


def reference_levels(mask, level_sizes, num_pos_feats, temperature=10000):
    """`level_constants` by torch from the padding mask [B, H, W]: the expression of the models' eager path"""
    masks = [F.interpolate(mask[None].float(), size=tuple(s)).to(torch.bool)[0] for s in level_sizes]
    return masks, [sine_position(mk, num_pos_feats, temperature) for mk in masks]


def _stats(v):
    """three python floats from a sequence or a (host or device) tensor; the models pass the cfg's host values"""
    v = v.flatten().tolist() if torch.is_tensor(v) else list(v)
    assert len(v) == 3
    return [float(t) for t in v]


def ingest_frames(pixels, table, B, H, W, mean, std, channels_last=False):
    """-> (x fp32 [B, 3, H, W], mask bool [B, H, W]); see the module docstring.  mean, std: three values each."""
    if not pixels.is_cuda:
        return reference_ingest(pixels, table, B, H, W, _stats(mean), _stats(std), channels_last)
    assert pixels.dtype == torch.uint8 and pixels.is_contiguous() and table.dtype == torch.int32 and table.is_contiguous()
    assert tuple(table.shape) == (B, 3) and table.device == pixels.device
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    x = torch.empty((B, 3, H, W), dtype=torch.float32, device=pixels.device, memory_format=fmt)
    mask = torch.empty((B, H, W), dtype=torch.bool, device=pixels.device)
    with torch.cuda.device(pixels.device):
        _lib.check(_lib.lib().vnx_ingest_frames(pixels.data_ptr(), pixels.numel(), table.data_ptr(), B, H, W,
                                                *_stats(mean), *_stats(std), int(bool(channels_last)), x.data_ptr(),
                                                mask.data_ptr(), _lib.current_stream(pixels)))
    CALLS["ingest_frames"] += 1
    return x, mask


def position_tables(device, num_pos_feats: int, temperature=10000):
    """(dim_t, degenerate) fp32 [num_pos_feats] on `device`, made once per (device, num_pos_feats, temperature) by the eager
    expression itself: `dim_t` as `sine_position` forms it, `degenerate` = `sine_position` of a one-element mask with no
    valid pixel -- the values ATen gives every row / column whose normaliser is 0, by construction.  (First use allocates
    and launches: not under stream capture; the models' warm-up runs make it.)"""
    device = torch.device(device)
    key = (str(device), int(num_pos_feats), float(temperature))
    t = _TABLES.get(key)
    if t is None:
        with torch.no_grad():
            dim_t = torch.arange(num_pos_feats, dtype=torch.float32, device=device)
            dim_t = temperature ** (2 * (dim_t // 2) / num_pos_feats)
            empty = torch.ones(1, 1, 1, dtype=torch.bool, device=device)
            degenerate = sine_position(empty, num_pos_feats, temperature)[0, :num_pos_feats, 0, 0].contiguous()
        t = _TABLES[key] = (dim_t.contiguous(), degenerate)
    return t


def levels_apply(table, level_sizes, num_pos_feats) -> bool:
    return (table.is_cuda and len(level_sizes) <= _lib.INGEST_MAX_LEVELS and num_pos_feats % 4 == 0
            and 0 < num_pos_feats <= _lib.INGEST_MAX_POS_FEATS)


def level_constants(table, B, H, W, level_sizes, num_pos_feats, temperature=10000):
    """-> (masks, poss): per level the padding mask bool [B, h, w] and the position fp32 [B, 2 * num_pos_feats, h, w] (a
    permuted view of [B, h, w, C], as `sine_position` returns it); see the module docstring."""
    level_sizes = [(int(h), int(w)) for h, w in level_sizes]
    if not levels_apply(table, level_sizes, num_pos_feats):
        mask = torch.ones(B, H, W, dtype=torch.bool, device=table.device)
        for i, (_, h, w) in enumerate(table.tolist()):
            mask[i, :h, :w] = False
        return reference_levels(mask, level_sizes, num_pos_feats, temperature)
    assert table.dtype == torch.int32 and table.is_contiguous() and tuple(table.shape) == (B, 3)
    dim_t, degenerate = position_tables(table.device, num_pos_feats, temperature)
    n = len(level_sizes)
    masks = [torch.empty((B, h, w), dtype=torch.bool, device=table.device) for h, w in level_sizes]
    poss = [torch.empty((B, h, w, 2 * num_pos_feats), dtype=torch.float32, device=table.device) for h, w in level_sizes]
    sizes = (ctypes.c_int * (2 * n))(*[v for s in level_sizes for v in s])
    mptr = (ctypes.c_void_p * n)(*[m.data_ptr() for m in masks])
    pptr = (ctypes.c_void_p * n)(*[p.data_ptr() for p in poss])
    with torch.cuda.device(table.device):
        _lib.check(_lib.lib().vnx_ingest_levels(table.data_ptr(), B, H, W, n, sizes, num_pos_feats, dim_t.data_ptr(),
                                                degenerate.data_ptr(), mptr, pptr, _lib.current_stream(table)))
    CALLS["level_constants"] += 1
    return masks, [p.permute(0, 3, 1, 2) for p in poss]
