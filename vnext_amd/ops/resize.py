"""Test-time resize of uint8 frames on the device, bit-exact with Pillow (vnext_amd/csrc/resize.hip).

The reference's test-time augmentation is `ResizeShortestEdge(MIN_SIZE_TEST, MAX_SIZE_TEST, "choice")` and nothing else; on a
uint8 frame it is `Image.fromarray(img).resize((nw, nh), Image.BILINEAR)`.  Pillow's 8-bit resample is integer arithmetic on
coefficient tables, restated here:

`shortest_edge_size(h, w, short, max_size) -> (nh, nw)`: the target size, in Python floats as the reference computes it.
`pillow_coeffs(n_in, n_out) -> (bounds int32 [n_out, 2], kk int32 [n_out, ksize])`: per output index the first source index and
the tap count, and the taps' weights in 22-bit fixed point -- out of IEEE double arithmetic, cached per (n_in, n_out).
`nearest_table(n_in, n_out) -> int32 [n_out]`: Pillow's NEAREST source indices, what `ops.augment` resamples masks with.
`CoeffTables(first)`: the builder of every `coeffs` buffer -- `bilinear(n_in, n_out) -> (bounds offset, weights offset, ksize)`
((0, 0, 0) where the axis keeps its size), `nearest(n_in, n_out) -> offset`, each distinct table placed once, `words(front)`
the finished buffer; `coeff_words(sizes, targets)` writes this op's 6-word rows with it, `augment.coeff_words` and
`augment.window_words` theirs.
`reference_resize(frame_u8, nh, nw, layout)`: the two passes by numpy on the CPU (horizontal first, rounded to uint8, then
vertical; a pass whose axis keeps its size is skipped).  It is the CPU route of the op and the oracle of the GPU tests; Pillow
is not imported.
`stage_sources(frames, targets, device, layout) -> (pixels, src_table, dst_table, coeffs)`: tables, coefficients and frame bytes
in ONE pinned buffer and one `non_blocking` copy (as `ingest.stage_frames`); uint8 frames already on the device take one `cat`
and one small upload.  `src_table` int32 [n, 3] = {byte offset, h, w}, `dst_table` int32 [n, 3] = {0, nh, nw} -- what
`ingest.level_constants` takes as its table, so the level masks and positions of the resized batch come from the existing
launch.  `coeffs` int32: n rows {bounds offset, weights offset, ksize} x {horizontal, vertical} (offsets in int32 words from
the start of `coeffs`, ksize 0 = the pass is skipped), then the tables themselves.
`resize_ingest_frames(pixels, src_table, dst_table, coeffs, B, H, W, mean, std, channels_last, layout) -> (x, mask)`: the same
outputs as `ingest.ingest_frames`, of the RESIZED frames, in one launch.

layout: "chw" ([3, h, w] planes, what the mappers give) or "hwc" ([h, w, 3] interleaved, what decoders give): always an
explicit argument, never guessed from a shape.  The kernel covers ksize <= 17 on both axes (a downscale of up to 8x, any
upscale); `applies` says so and the caller takes the host route beyond.  `CALLS` counts the kernel launches made here.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from .. import _lib
from . import ingest

CALLS = {"resize_ingest_frames": 0}      # launches through the C ABI (tests: the op ran / did not run)

PRECISION_BITS = 22                      # Pillow's 8-bit resample: weights in 22-bit fixed point, 2^21 added before the shift
LAYOUTS = ("chw", "hwc")


def shortest_edge_size(h: int, w: int, short: int, max_size: int):
    """`ResizeShortestEdge.get_output_shape`: the short edge becomes `short`, the long edge scales with it, both shrink
    together if the larger would exceed `max_size`; int(v + 0.5) of each."""
    h, w = int(h), int(w)
    size = short * 1.0
    scale = size / min(h, w)
    if h < w:
        newh, neww = size, scale * w
    else:
        newh, neww = scale * h, size
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh = newh * scale
        neww = neww * scale
    return int(newh + 0.5), int(neww + 0.5)


def kernel_size(n_in: int, n_out: int) -> int:
    """taps per output index of the bilinear filter, n_in -> n_out"""
    return int(math.ceil(max(n_in / n_out, 1.0))) * 2 + 1


@functools.lru_cache(maxsize=256)
def _coeffs(n_in: int, n_out: int):
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    kk = np.zeros((n_out, ksize), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), n_in) - xmin
        ws, total = [], 0.0
        for x in range(cnt):
            w = max(0.0, 1.0 - abs((x + xmin - center + 0.5) / fs))
            ws.append(w)
            total += w                   # left to right, as the C loop sums
        for x, w in enumerate(ws):
            if total != 0.0:
                w = w / total
            kk[xx, x] = int(0.5 + w * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, cnt)
    bounds.setflags(write=False)
    kk.setflags(write=False)
    return bounds, kk


def pillow_coeffs(n_in: int, n_out: int):
    """-> (bounds int32 [n_out, 2] = (xmin, cnt), kk int32 [n_out, ksize]); read-only arrays, cached per (n_in, n_out)"""
    return _coeffs(int(n_in), int(n_out))


@functools.lru_cache(maxsize=256)
def _nearest(n_in: int, n_out: int):
    a = n_in / n_out
    xo = a * 0.5
    tab = np.empty(n_out, dtype=np.int32)
    for i in range(n_out):
        tab[i] = int(xo)
        xo += a
    np.minimum(tab, n_in - 1, out=tab)      # (Pillow skips a sample outside the image; none is on these tables)
    tab.setflags(write=False)
    return tab


def nearest_table(n_in: int, n_out: int):
    """-> int32 [n_out], read-only, cached per (n_in, n_out): Pillow's `resize(..., NEAREST)` source indices (what the masks
    of `ops.augment` are resampled with; see its module docstring)"""
    return _nearest(int(n_in), int(n_out))


class CoeffTables:
    """The tables behind the rows of a `coeffs` buffer: the next free word, the parts so far, what is already placed.
    `first`: the words in front of the first table (the rows, or a buffer that is being extended)."""

    def __init__(self, first: int):
        self.at, self.parts, self.placed = int(first), [], {}

    def _place(self, key, tables, value):
        if key not in self.placed:
            self.placed[key] = value
            self.parts += [t.reshape(-1) for t in tables]
            self.at += sum(t.size for t in tables)
        return self.placed[key]

    def bilinear(self, n_in: int, n_out: int):
        """-> (bounds offset, weights offset, ksize) of `pillow_coeffs(n_in, n_out)`, placed once; (0, 0, 0) for
        n_in == n_out: the pass is skipped"""
        if n_in == n_out:
            return 0, 0, 0
        bounds, kk = pillow_coeffs(n_in, n_out)
        return self._place(("bilinear", n_in, n_out), (bounds, kk), (self.at, self.at + bounds.size, kk.shape[1]))

    def nearest(self, n_in: int, n_out: int) -> int:
        """-> the offset of `nearest_table(n_in, n_out)`, placed once"""
        return self._place(("nearest", n_in, n_out), (nearest_table(n_in, n_out),), self.at)

    def words(self, front):
        """`front` (the `first` words) and every placed table behind it, as one int32 array"""
        return np.concatenate([np.asarray(front, dtype=np.int32).reshape(-1)] + self.parts)


def _pass(src, bounds, kk):
    """one resample pass along axis 1 of uint8 [rows, n_in, ...] -> uint8 [rows, n_out, ...]"""
    out = np.empty((src.shape[0], bounds.shape[0]) + src.shape[2:], dtype=np.uint8)
    wide = src.astype(np.int64)
    for xx, (xmin, cnt) in enumerate(bounds.tolist()):
        k = kk[xx, :cnt].astype(np.int64).reshape((1, cnt) + (1,) * (src.ndim - 2))
        acc = (1 << (PRECISION_BITS - 1)) + (wide[:, xmin:xmin + cnt] * k).sum(1)
        out[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def _hw_axes(layout: str):
    if layout not in LAYOUTS:
        raise ValueError("layout must be 'chw' or 'hwc', not %r" % (layout,))
    return (1, 2) if layout == "chw" else (0, 1)


def frame_size(frame, layout: str):
    ah, aw = _hw_axes(layout)
    return int(frame.shape[ah]), int(frame.shape[aw])


def reference_resize(frame_u8, nh: int, nw: int, layout: str = "chw"):
    """Pillow's `resize((nw, nh), BILINEAR)` of a uint8 frame (tensor or array, `layout`), by integer numpy on the CPU; the
    result has the input's kind and layout."""
    ah, aw = _hw_axes(layout)
    is_tensor = torch.is_tensor(frame_u8)
    a = frame_u8.detach().cpu().numpy() if is_tensor else np.asarray(frame_u8)
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[3 - ah - aw] == 3
    h, w = a.shape[ah], a.shape[aw]
    if nw != w:                          # horizontal first; its result is bytes
        a = np.moveaxis(_pass(np.moveaxis(a, aw, 1), *pillow_coeffs(w, nw)), 1, aw)
    if nh != h:
        a = np.moveaxis(_pass(np.moveaxis(a, ah, 1), *pillow_coeffs(h, nh)), 1, ah)
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.copy() if not a.flags.writeable else a) if is_tensor else a


def axis_supported(n_in: int, n_out: int) -> bool:
    """the kernel's range on one axis: at most VNX_RESIZE_MAX_KSIZE taps"""
    return min(n_in, n_out) >= 1 and kernel_size(n_in, n_out) <= _lib.RESIZE_MAX_KSIZE


def supported(h: int, w: int, nh: int, nw: int) -> bool:
    """the kernel's range: at most VNX_RESIZE_MAX_KSIZE taps on both axes"""
    return min(h, w, nh, nw) >= 1 and axis_supported(h, nh) and axis_supported(w, nw)


def applies(frames, targets, device, layout: str = "chw") -> bool:
    """All frames are uint8 tensors of `layout` (CPU or on `device`) and every (source, target) pair is in the kernel's range"""
    ah, aw = _hw_axes(layout)
    c = 3 - ah - aw
    if not frames or len(frames) != len(targets):
        return False
    cuda = frames[0].is_cuda if torch.is_tensor(frames[0]) else False
    for f, (nh, nw) in zip(frames, targets):
        if not (torch.is_tensor(f) and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[c] == 3 and f.numel() > 0):
            return False
        if f.is_cuda != cuda or (f.is_cuda and f.device != torch.device(device)):
            return False
        if not supported(f.shape[ah], f.shape[aw], nh, nw):
            return False
    return True


def plan_video(frames, layout: str, short: int, max_size: int, device):
    """What a model with `device_resize` does with one video's frames -> (frames, plan, source size of frame 0).
    plan = (targets, layout): hand `frames` as they are to `stage_sources` / `resize_ingest_frames`.
    plan = None: hand `frames` to the path the model takes without the switch -- they are not uint8 tensors of `layout`
    (float frames: returned untouched, source size None), they are CHW and already at their targets (the rule is idempotent on
    its own outputs), or a pair is outside the kernel's range: the host route, `reference_resize` frame by frame to CHW."""
    ah, aw = _hw_axes(layout)
    if not frames or not all(torch.is_tensor(f) and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[3 - ah - aw] == 3
                             and f.numel() > 0 for f in frames):
        return frames, None, None
    sizes = [frame_size(f, layout) for f in frames]
    targets = [shortest_edge_size(h, w, short, max_size) for h, w in sizes]
    if layout == "chw" and targets == sizes:
        return frames, None, sizes[0]
    if applies(frames, targets, device, layout):
        return frames, (targets, layout), sizes[0]
    out = []
    for f, (nh, nw) in zip(frames, targets):
        r = reference_resize(f, nh, nw, layout)
        out.append(r if layout == "chw" else r.permute(2, 0, 1).contiguous())
    return out, None, sizes[0]


padded_size = ingest.padded_hw           # (H, W): the largest target (nh, nw), rounded up to multiples of 32


def coeff_words(sizes, targets):
    """the `coeffs` buffer of a batch as one int32 array: the per-frame rows, then each distinct axis table once"""
    tables = CoeffTables(6 * len(sizes))
    rows = [tables.bilinear(w, nw) + tables.bilinear(h, nh) for (h, w), (nh, nw) in zip(sizes, targets)]
    return tables.words(np.array(rows, dtype=np.int32).reshape(len(sizes), 6))


_coeff_words = coeff_words               # (the name it had while it was private: callers written against it keep working)


def stage_sources(frames, targets, device, layout: str = "chw"):
    """uint8 frames of `layout` and their target sizes [(nh, nw)] -> (pixels uint8 [bytes], src_table int32 [n, 3],
    dst_table int32 [n, 3], coeffs int32 [words]) on `device`; see the module docstring."""
    n = len(frames)
    sizes = [frame_size(f, layout) for f in frames]
    on_device = frames[0].is_cuda
    rows, off = [], 0
    for h, w in sizes:
        rows.append((off, h, w))
        off += 3 * h * w if on_device else ingest._align16(3 * h * w)
    ints = [np.array(rows, dtype=np.int32), np.array([(0, int(nh), int(nw)) for nh, nw in targets], dtype=np.int32),
            coeff_words(sizes, targets)]
    if on_device:
        pixels = torch.cat([f.reshape(-1) for f in frames])
        dev = torch.from_numpy(np.concatenate([a.reshape(-1) for a in ints])).pin_memory().to(device, non_blocking=True)
        return pixels, dev[:3 * n].view(n, 3), dev[3 * n:6 * n].view(n, 3), dev[6 * n:]
    (src, dst, words), pixels = ingest.pack_upload(ints, [(f, o) for f, (o, _, _) in zip(frames, rows)], off, device)
    return pixels, src, dst, words


def reference_resize_ingest(pixels, src_table, dst_table, coeffs, B, H, W, mean, std, channels_last=False, layout="chw"):
    """`resize_ingest_frames` on the CPU: `reference_resize` frame by frame, then the models' eager normalise + pad"""
    _hw_axes(layout)
    parts, rows, off = [], [], 0
    for (o, h, w), (_, nh, nw) in zip(src_table.tolist(), dst_table.tolist()):
        f = pixels[o:o + 3 * h * w].view((3, h, w) if layout == "chw" else (h, w, 3))
        r = reference_resize(f, nh, nw, layout)
        r = r if layout == "chw" else r.permute(2, 0, 1)
        parts.append(r.reshape(-1))
        rows.append((off, nh, nw))
        off += 3 * nh * nw
    return ingest.reference_ingest(torch.cat(parts), torch.tensor(rows, dtype=torch.int32), B, H, W, mean, std, channels_last)


def resize_ingest_frames(pixels, src_table, dst_table, coeffs, B, H, W, mean, std, channels_last=False, layout="chw"):
    """-> (x fp32 [B, 3, H, W], mask bool [B, H, W]) of the resized frames; see the module docstring."""
    _hw_axes(layout)
    if not pixels.is_cuda:
        return reference_resize_ingest(pixels, src_table, dst_table, coeffs, B, H, W, ingest._stats(mean),
                                       ingest._stats(std), channels_last, layout)
    assert pixels.dtype == torch.uint8 and pixels.is_contiguous()
    for t in (src_table, dst_table):
        assert t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (B, 3) and t.device == pixels.device
    assert coeffs.dtype == torch.int32 and coeffs.is_contiguous() and coeffs.device == pixels.device
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    x = torch.empty((B, 3, H, W), dtype=torch.float32, device=pixels.device, memory_format=fmt)
    mask = torch.empty((B, H, W), dtype=torch.bool, device=pixels.device)
    with torch.cuda.device(pixels.device):
        _lib.check(_lib.lib().vnx_resize_ingest_frames(
            pixels.data_ptr(), pixels.numel(), src_table.data_ptr(), dst_table.data_ptr(), coeffs.data_ptr(), coeffs.numel(),
            B, H, W, *ingest._stats(mean), *ingest._stats(std), int(bool(channels_last)), int(layout == "hwc"),
            x.data_ptr(), mask.data_ptr(), _lib.current_stream(pixels)))
    CALLS["resize_ingest_frames"] += 1
    return x, mask
