"""Training-time augmentation on the device: crop, resize, horizontal flip of uint8 source frames AND of their ground-truth
masks, with the masks' boxes (vnext_amd/csrc/augment.hip).

The reference trains every config with RandomCrop("absolute_range") (IDOL), ResizeShortestEdge and RandomFlip, applied by
Pillow and numpy in a data-loader worker to the frames and, mask by mask, to the decoded ground truth.  Here the host only
draws the random numbers (`vnext_amd/data/clip_mapper.py`); frames cross the bus as decoded bytes and masks as their COCO run
lengths, and a few launches produce (x, mask) and every mask, box and `nonempty` flag.

`FramePlan(x0, y0, cw, ch, nh, nw, flip)`: one frame's draw: the crop window inside the source, the target size, the flip.
A plan answers for itself: `inside(h, w)`, `resamples()` (the (n_in, n_out) pairs `supported` checks), `coords(xy)` (polygon
and box coordinates, in float64), `frame(...)` and `mask(dense)` (the host route of one frame and one mask), `truth(masks,
bboxes)` (a frame's boxes and keep flags); `ChainPlan` below has the same methods, so nothing outside the two asks which
kind a plan is.
`nearest_table(n_in, n_out) -> int32 [n_out]` (`resize.nearest_table`): Pillow's `resize(..., NEAREST)` source indices.  Pillow
takes its affine path for NEAREST and ACCUMULATES in double -- xo = 0.5 * a, then tab[i] = int(xo); xo += a with
a = n_in / n_out -- which is not `floor((i + 0.5) * n_in / n_out)` (they differ on about a fifth of the size pairs).  Python
floats, cached per pair.
`reference_augment_frames(frames, plan, layout)`: numpy slicing, `resize.reference_resize`, `np.flip` -> uint8 frames.
`reference_augment_masks(masks, sizes, plan)`: `rle_decode`, slicing, the index tables, `np.flip` (`reference_rle_mask`), then
the box as `BitMasks.get_bounding_boxes` computes it.  Both are the CPU route of the ops and the oracle of the GPU tests.
`coeff_words(plan)`, `window_words(words, rows)`: the `coeffs` buffer of a step and the first resamples' tables behind it;
each distinct bilinear and nearest table once (`resize.CoeffTables`).
`stage_step(frames, plan, masks, device, layout) -> Staged`: the tables, the coefficients, the masks' run END positions (one
cumsum each), their rows and ids, and the frame bytes in ONE pinned buffer and one `non_blocking` copy
(`ingest.pack_upload`): the sources' layout of its kind of plan, the mask rows, the upload.
`augment_frames(staged, mean, std, channels_last) -> (x, mask)`: one launch; the outputs of `resize.resize_ingest_frames`.
`augment_masks(staged) -> (masks uint8 [bytes], boxes fp32 [m, 4], nonempty bool [m])`: two launches; `staged.mask_views(masks)`
gives each frame's bool [n_inst, nh, nw] as a view.

The bilinear range is the resize kernel's (ksize <= 17 on both axes, of the WINDOW to the target); `applies` says so and the
caller takes the host route beyond.  `CALLS` counts the launches made here.

Polygon ground truth: `transform_polygons(segmentation, p)` applies a frame's plan to the coordinates on
the host (crop, resize, flip, in the reference's order and with its expressions), `ops.poly_rle.polygons_to_runs` rasterises
them at the TARGET size on the device, and `stage_step` takes such a mask as a `PolyRuns(offset, size)` -- its slot of the
device-resident run ends -- and gives it a pseudo-frame row (the target as its own source: the full window, no flip, identity
nearest tables), so ONE `augment_masks` call makes gt_masks, boxes and `nonempty` of RLE and polygon masks alike.

The COCO pre-training chain: IDOL's `COCO_CLIP_DatasetMapper` applies flip -> resize to (h1, w1) -> crop ->
resize to (nh, nw), two resamples through a byte-rounded intermediate image.  `ChainPlan` is one frame's draw of it;
`ChainPlan.frame` / `mask` / `coords` and `chain_boxes` are the literal host route; `reference_augment_frames` (also under
the name `reference_chain_frames`), `reference_rle_mask`, `transform_polygons` and `reference_polygon_mask` take either kind
of plan.  `stage_step` takes a step of ChainPlans: a source tensor that is listed
more than once is uploaded once, every frame that needs the first resample gets a slot behind the source frames in the SAME
device allocation, and `resize_window_bytes(staged)` -- one launch of `vnx_resize_window_bytes`, none when no frame needs it --
fills the slots with the (mirrored, where the frame is flipped) crop window of the resized frame; `augment_frames` then reads a
slot as a source frame.  Pillow's 8-bit bilinear resize commutes with a horizontal flip, so flip-first equals the mirrored
window with the flip applied last -- which is what the kernels do, and what the tests hold to the literal order.
`BYTES_CALLS` counts those launches.

Colour: a FramePlan may carry `brightness`, `contrast`, `saturation` -- the weights detectron2's
RandomBrightness / RandomContrast / RandomSaturation drew for THIS frame, None where the step is off (the default: every
positional construction keeps its meaning).  `color_frame` is the three steps in numpy, literally, on the resized and flipped
bytes; `FramePlan.frame` ends with it, so `reference_augment_frames` and `host_augmented` take them.  `stage_step` packs the
weights of a step that has any into a colour table [n, 8] (`color_words`: the float as its bit pattern, the doubles as two
words) in the same upload, and with contrast reserves the kernels' workspace behind the frames in the same allocation;
`augment_frames` then calls `vnx_augment_frames_color`: one launch, two with contrast (the mean of a whole frame after
brightness needs a pass of its own).  A step without a weight stages the tables and makes the launch it always did.
`COLOR_CALLS` counts those calls and their launches.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from .. import _lib
from ..utils.ytvis_json import counts_to_string, rle_decode
from . import ingest, poly_rle, resize

CALLS = {"augment_frames": 0, "augment_masks": 0}      # calls through the C ABI (tests: the ops ran / did not run)
BYTES_CALLS = {"resize_window_bytes": 0}               # (a dict of its own: tests compare CALLS as a whole)
COLOR_CALLS = {"augment_frames_color": 0, "launches": 0}      # (likewise; every such call also counts as an augment_frames)
SRC_WORDS, COEFF_WORDS, MASK_ROW_WORDS, WIN_WORDS, COLOR_WORDS = 8, 8, 4, 16, 8
BRIGHTNESS, CONTRAST, SATURATION = 1, 2, 4             # the flags of a colour row
NO_COLOR = (None, None, None)


nearest_table = resize.nearest_table


def _window(a, p, ah: int, aw: int):
    """the plan's crop window {x0, y0, cw, ch} of an array whose rows and columns are axes (ah, aw)"""
    sl = [slice(None)] * a.ndim
    sl[ah], sl[aw] = slice(p.y0, p.y0 + p.ch), slice(p.x0, p.x0 + p.cw)
    return np.ascontiguousarray(a[tuple(sl)])


def _window_inside(p, h: int, w: int) -> bool:
    return p.x0 >= 0 and p.y0 >= 0 and p.cw >= 1 and p.ch >= 1 and p.x0 + p.cw <= w and p.y0 + p.ch <= h


def _to_bytes(x):
    """what every BlendTransform returns: `np.clip(x, 0, 255).astype(np.uint8)` (the conversion truncates)"""
    return np.clip(x, 0, 255).astype(np.uint8)


def color_frame(a, ac: int, brightness=None, contrast=None, saturation=None):
    """detectron2's RandomBrightness, RandomContrast, RandomSaturation with the weights they drew (None: the step is off), in
    `build_augmentation`'s order, on a uint8 frame whose channels are axis `ac`; every step returns bytes, so the next one
    sees bytes.  numpy 2 types: brightness in float32, one rounding; contrast and saturation in float64, every product and
    every sum rounded on its own.  The gray value is the left-to-right sum of three rounded products on the channels in stored
    order (this package's statement of `image.dot([0.299, 0.587, 0.114])`, whose rounding is the BLAS's).  The oracle of the
    kernels."""
    if brightness is not None:
        a = _to_bytes(np.float32(brightness) * a.astype(np.float32))
    if contrast is not None:
        w = float(contrast)
        a = _to_bytes((1 - w) * a.mean() + w * a.astype(np.float64))
    if saturation is not None:
        w = float(saturation)
        c = np.moveaxis(a, ac, 0).astype(np.float64)
        gray = c[0] * 0.299 + c[1] * 0.587 + c[2] * 0.114
        a = _to_bytes((1 - w) * np.expand_dims(gray, ac) + w * a.astype(np.float64))
    return a


class FramePlan(NamedTuple):
    """One frame's draw of crop -> resize -> flip: the window {x0, y0, cw, ch} inside the source, the target, the flip; then
    the colour weights drawn for this frame, None where the step is off"""
    x0: int
    y0: int
    cw: int
    ch: int
    nh: int
    nw: int
    flip: bool
    brightness: float = None
    contrast: float = None
    saturation: float = None

    @property
    def color(self):
        return (self.brightness, self.contrast, self.saturation)

    def inside(self, h: int, w: int) -> bool:
        """the window lies inside a source of h x w"""
        return _window_inside(self, h, w)

    def resamples(self):
        """the (n_in, n_out) pairs the kernels resample, horizontal first"""
        return [(self.cw, self.nw), (self.ch, self.nh)]

    def coords(self, xy):
        """flat float64 [x, y, x, y, ...] (changed in place) in the reference's order and with its expressions: crop
        `x -= x0, y -= y0`; resize `x * (nw * 1.0 / cw), y * (nh * 1.0 / ch)` (ResizeTransform.apply_coords); flip
        `x = nw - x` (HFlipTransform.apply_coords)"""
        xy[0::2] -= self.x0
        xy[1::2] -= self.y0
        xy[0::2] = xy[0::2] * (self.nw * 1.0 / self.cw)
        xy[1::2] = xy[1::2] * (self.nh * 1.0 / self.ch)
        if self.flip:
            xy[0::2] = self.nw - xy[0::2]
        return xy

    def frame(self, a, ah: int, aw: int, layout: str):
        """a uint8 source array -> the augmented one: slicing, `resize.reference_resize`, `np.flip`, `color_frame`"""
        a = resize.reference_resize(_window(a, self, ah, aw), self.nh, self.nw, layout)
        a = np.flip(a, axis=aw) if self.flip else a
        return a if self.color == NO_COLOR else color_frame(a, 3 - ah - aw, *self.color)

    def mask(self, dense):
        """a bool [h, w] mask at the source size -> bool [nh, nw]: slicing, the index tables, `np.flip`"""
        m = _window(dense, self, 0, 1)[nearest_table(self.ch, self.nh)][:, nearest_table(self.cw, self.nw)]
        return np.flip(m, axis=1) if self.flip else m

    def truth(self, masks, bboxes=None):
        """a frame's augmented masks -> (their boxes float32 [n, 4] as `BitMasks.get_bounding_boxes` computes them, the
        instances `filter_empty_instances` keeps bool [n]); the annotations' boxes are not read"""
        return mask_boxes(masks)


class ChainPlan(NamedTuple):
    """One frame's draw of flip -> resize -> crop -> resize: the source size (h, w), the flip, the first resize's target
    (h1, w1), the crop window {x0, y0, cw, ch} inside the FLIPPED and resized h1 x w1 image, the final target (nh, nw).
    The side without a crop is the same record with (h1, w1) = (h, w) and the full window (`chain_full`)."""
    h: int
    w: int
    flip: bool
    h1: int
    w1: int
    x0: int
    y0: int
    cw: int
    ch: int
    nh: int
    nw: int

    color = NO_COLOR      # (the COCO mapper builds its own list and never reads INPUT.AUGMENTATIONS)

    @property
    def resamples_twice(self) -> bool:
        """the first resample exists (an identity resize is skipped, not run)"""
        return (self.h1, self.w1) != (self.h, self.w)

    @property
    def mirrored_x0(self) -> int:
        """the window's origin in the UNFLIPPED resized image"""
        return self.w1 - self.x0 - self.cw if self.flip else self.x0

    def inside(self, h: int, w: int) -> bool:
        """the plan is of THIS frame (h x w), and its window lies inside the resized image"""
        return (self.h, self.w) == (h, w) and min(self.h1, self.w1, self.nh, self.nw) >= 1 and \
            _window_inside(self, self.h1, self.w1)

    def resamples(self):
        """the (n_in, n_out) pairs the kernels resample: the first resize (where it exists), then the second"""
        first = [(self.w, self.w1), (self.h, self.h1)] if self.resamples_twice else []
        return first + [(self.cw, self.nw), (self.ch, self.nh)]

    def coords(self, xy):
        """flat float64 [x, y, x, y, ...] (changed in place) in the reference's order and with its expressions:
        `x = w - x` on a flip (HFlipTransform.apply_coords); `x * (w1 * 1.0 / w), y * (h1 * 1.0 / h)`
        (ResizeTransform.apply_coords); `x -= x0, y -= y0` (CropTransform); `x * (nw * 1.0 / cw), y * (nh * 1.0 / ch)`"""
        if self.flip:
            xy[0::2] = self.w - xy[0::2]
        xy[0::2] = xy[0::2] * (self.w1 * 1.0 / self.w)
        xy[1::2] = xy[1::2] * (self.h1 * 1.0 / self.h)
        xy[0::2] -= self.x0
        xy[1::2] -= self.y0
        xy[0::2] = xy[0::2] * (self.nw * 1.0 / self.cw)
        xy[1::2] = xy[1::2] * (self.nh * 1.0 / self.ch)
        return xy

    def frame(self, a, ah: int, aw: int, layout: str):
        """a uint8 source array through the chain in the LITERAL order: `np.flip`, `resize.reference_resize` to (h1, w1),
        slicing, `resize.reference_resize` to (nh, nw)"""
        if self.flip:
            a = np.ascontiguousarray(np.flip(a, axis=aw))
        a = resize.reference_resize(a, self.h1, self.w1, layout)
        return resize.reference_resize(_window(a, self, ah, aw), self.nh, self.nw, layout)

    def mask(self, dense):
        """a bool [h, w] mask at the source size as the reference's `apply_segmentation` does it: `np.flip`, Pillow's
        NEAREST to (h1, w1), slicing, NEAREST to (nh, nw) -> bool [nh, nw]"""
        m = np.flip(dense, axis=1) if self.flip else dense
        m = _window(m[nearest_table(self.h, self.h1)][:, nearest_table(self.w, self.w1)], self, 0, 1)
        return m[nearest_table(self.ch, self.nh)][:, nearest_table(self.cw, self.nw)]

    def truth(self, masks, bboxes):
        """a frame's augmented masks and its annotations' boxes (XYXY) -> (`chain_boxes`, the instances the mapper keeps:
        the box AND the mask are not empty)"""
        boxes = chain_boxes(bboxes, self)
        return boxes, boxes_nonempty(boxes) & np.array([bool(m.any()) for m in masks], dtype=bool)


def chain_full(h: int, w: int, nh: int, nw: int, flip: bool = False) -> ChainPlan:
    """the side of the coin without a crop: flip, one resize"""
    return ChainPlan(int(h), int(w), bool(flip), int(h), int(w), 0, 0, int(w), int(h), int(nh), int(nw))


class PolyRuns(NamedTuple):
    """a mask whose run ends are on the device already (a slot of `polygons_to_runs`' ends, at the frame's TARGET size)"""
    offset: int
    size: int


def full_plan(h: int, w: int, nh: int, nw: int, flip: bool = False) -> FramePlan:
    """the whole frame as the window"""
    return FramePlan(0, 0, int(w), int(h), int(nh), int(nw), bool(flip))


# ---- the CPU route and oracle -----------------------------------------------------------------------------------------------
def reference_augment_frames(frames, plan, layout: str = "chw"):
    """uint8 frames (tensors or arrays of `layout`) -> each through its plan's `frame` (a FramePlan: cropped, resized and
    flipped; a ChainPlan: the chain in its literal order), same kind and layout.  The CPU route of the ops and the oracle of
    the GPU tests."""
    ah, aw = resize._hw_axes(layout)
    out = []
    for f, p in zip(frames, plan):
        is_tensor = torch.is_tensor(f)
        a = f.detach().cpu().numpy() if is_tensor else np.asarray(f)
        assert p.inside(a.shape[ah], a.shape[aw])
        a = np.ascontiguousarray(p.frame(a, ah, aw, layout))
        out.append(torch.from_numpy(a) if is_tensor else a)
    return out


reference_chain_frames = reference_augment_frames      # (the name the chain's tests and callers use)


def _dense(counts, h: int, w: int):
    """COCO counts -> bool [h, w]; counts that do not sum to h * w, or a negative one, are the empty mask"""
    counts = [int(c) for c in counts]
    if sum(counts) == h * w and min(counts) >= 0:
        return rle_decode({"size": [h, w], "counts": counts_to_string(counts)}).astype(bool)
    return np.zeros((h, w), dtype=bool)


def reference_rle_mask(counts, size, p):
    """One RLE mask (COCO counts at the source `size` = (h, w)) through a plan of either kind (`p.mask`) -> bool [nh, nw]"""
    return np.ascontiguousarray(p.mask(_dense(counts, *size)))


def chain_boxes(bboxes, p: ChainPlan):
    """The annotations' boxes (XYXY, float64 [n, 4]) through a ChainPlan as `transform_instance_annotations` takes them: the
    four corners through the coordinates' chain, their min / max, `clip(min=0)`, the minimum with (nw, nh, nw, nh) -- all in
    float64 -- then float32 [n, 4], as `Boxes` holds them."""
    b = np.asarray(bboxes, dtype=np.float64).reshape(-1, 4)
    if b.shape[0] == 0:
        return np.zeros((0, 4), dtype=np.float32)
    corners = b[:, [0, 1, 2, 1, 0, 3, 2, 3]].reshape(-1)       # (x0, y0), (x1, y0), (x0, y1), (x1, y1), box by box
    xy = p.coords(corners.copy()).reshape(-1, 4, 2)
    lo, hi = xy.min(axis=1), xy.max(axis=1)
    out = np.concatenate((lo, hi), axis=1).clip(min=0)
    return np.minimum(out, np.array([p.nw, p.nh, p.nw, p.nh], dtype=np.float64)).astype(np.float32)


def boxes_nonempty(boxes, threshold: float = 1e-5):
    """`Boxes.nonempty(threshold)` of float32 [n, 4]: width and height above the threshold"""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    return ((boxes[:, 2] - boxes[:, 0]) > threshold) & ((boxes[:, 3] - boxes[:, 1]) > threshold)


def transform_polygons(segmentation, p):
    """One annotation's polygons (or boxes, as their 4-vertex polygons) through the frame's plan, in float64 and in the
    reference's order (`FramePlan.coords`: crop, resize, flip; `ChainPlan.coords`: flip, resize, crop, resize).  The shifted
    polygon is NOT clipped to the window (the reference clips with shapely first, which is not installed): the rasteriser
    drops columns outside the canvas and clamps rows.
    -> a list of flat float64 polygons for a canvas of nh x nw."""
    return [p.coords(poly.copy()) for poly in poly_rle.object_polygons(segmentation)]


def reference_polygon_mask(segmentation, p):
    """the host route of one polygon mask: `transform_polygons`, `object_counts_host` at (nh, nw) -> bool [nh, nw]"""
    counts = poly_rle.object_counts_host(transform_polygons(segmentation, p), p.nh, p.nw)
    return np.ascontiguousarray(poly_rle.counts_to_mask(counts, p.nh, p.nw))


def mask_box(m):
    """`BitMasks.get_bounding_boxes` of one bool [h, w] array -> ([x0, y0, x1 + 1, y1 + 1] float32, nonempty)"""
    xs, ys = np.flatnonzero(m.any(0)), np.flatnonzero(m.any(1))
    if xs.size == 0:
        return np.zeros(4, dtype=np.float32), False
    return np.array([xs[0], ys[0], xs[-1] + 1, ys[-1] + 1], dtype=np.float32), True


def mask_boxes(masks):
    """`mask_box` of each -> (boxes float32 [m, 4], nonempty bool [m])"""
    found = [mask_box(m) for m in masks]
    return (np.array([b for b, _ in found], dtype=np.float32).reshape(len(masks), 4),
            np.array([k for _, k in found], dtype=bool))


def reference_augment_masks(masks, sizes, plan):
    """masks: [(frame index, COCO counts)]; sizes: the frames' source (h, w); plan: the frames' FramePlan
    -> ([bool array [nh, nw] per mask], boxes float32 [m, 4], nonempty bool [m]).  Counts that do not sum to h * w are the
    empty mask."""
    outs = [reference_rle_mask(counts, sizes[f], plan[f]) for f, counts in masks]
    return (outs, *mask_boxes(outs))


# ---- staging ----------------------------------------------------------------------------------------------------------------
def supported(p) -> bool:
    """every resample of the plan (both of a ChainPlan, the one of a FramePlan) is in the kernel's range"""
    return all(resize.axis_supported(n_in, n_out) for n_in, n_out in p.resamples())


def applies(frames, plan, device, layout: str = "chw", polygons=None) -> bool:
    """All frames are uint8 CPU tensors of `layout`, the plans are of one kind, every window lies inside its frame and every
    (window, target) pair is in the kernel's range; polygons: (objects, sizes) of the step's transformed polygon masks, or
    what `poly_rle.plan_objects` made of them -- every one inside the caps of vnx_poly_rle"""
    ah, aw = resize._hw_axes(layout)
    if not frames or len(frames) != len(plan) or len({type(p) for p in plan}) > 1:
        return False
    if polygons is not None:
        fits = polygons[2] if len(polygons) == 3 else poly_rle.plan_objects(*polygons)[2]
        if not bool(np.all(fits)):
            return False
    for f, p in zip(frames, plan):
        if not (torch.is_tensor(f) and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[3 - ah - aw] == 3 and not f.is_cuda):
            return False
        if not (p.inside(f.shape[ah], f.shape[aw]) and supported(p)):
            return False
    return True


def padded_size(plan):
    return ingest.padded_hw([(p.nh, p.nw) for p in plan])


def coeff_words(plan):
    """the `coeffs` buffer of a step as one int32 array: a row of 8 per frame ({bounds offset, weights offset, ksize} x
    {horizontal, vertical}, then the two nearest tables' offsets), then each distinct bilinear and nearest table once"""
    tables = resize.CoeffTables(COEFF_WORDS * len(plan))
    rows = np.zeros((len(plan), COEFF_WORDS), dtype=np.int32)
    for row, p in zip(rows, plan):
        for j, pair in enumerate(((p.cw, p.nw), (p.ch, p.nh))):
            row[3 * j:3 * j + 3] = tables.bilinear(*pair)
            row[6 + j] = tables.nearest(*pair)
    return tables.words(rows)


def window_words(words, win):
    """`resize_window_bytes`' rows (lists of 16, the triples still zero) and a step's `coeffs` words -> (the words with each
    distinct table of (w -> w1) and (h -> h1) appended once, int32 [k, 16] rows that name them)"""
    win = np.asarray(win, dtype=np.int32).reshape(-1, WIN_WORDS)
    tables = resize.CoeffTables(words.size)
    for row in win:
        row[10:13] = tables.bilinear(int(row[2]), int(row[4]))
        row[13:16] = tables.bilinear(int(row[1]), int(row[3]))
    return tables.words(words), win


def color_words(plan):
    """the colour table of a step: int32 [n, 8] = {flags, brightness as the float's bit pattern, contrast as a double's two
    words (low, high), saturation likewise, 0, 0}; a frame without a weight is a row of zeros"""
    rows = np.zeros((len(plan), COLOR_WORDS), dtype=np.int32)
    for row, p in zip(rows, plan):
        wb, wc, ws = p.color
        row[0] = BRIGHTNESS * (wb is not None) | CONTRAST * (wc is not None) | SATURATION * (ws is not None)
        row[1:2] = np.array([0.0 if wb is None else wb], dtype=np.float32).view(np.int32)
        row[2:6] = np.array([0.0 if wc is None else wc, 0.0 if ws is None else ws], dtype="<f8").view(np.int32)
    return rows


def color_of(row):
    """a colour row (a list of 8) -> (brightness, contrast, saturation), None where the flag is clear"""
    words = np.array(row, dtype=np.int32)
    wb, (wc, ws) = float(words[1:2].view(np.float32)[0]), words[2:6].view("<f8").tolist()
    return (wb if row[0] & BRIGHTNESS else None, wc if row[0] & CONTRAST else None, ws if row[0] & SATURATION else None)


def color_workspace(n: int, H: int, W: int) -> int:
    """the bytes `vnx_augment_frames_color` wants behind the frames when contrast is on: the post-brightness bytes
    [n, 3, H, W] and a uint32 per (frame, 32 x 32 tile) (vnx_augment_color_workspace)"""
    return n * 3 * H * W + 4 * n * (H // 32) * (W // 32)


_coeff_words, _window_words = coeff_words, window_words      # (their names while private: callers written against them keep working)


class Staged(NamedTuple):
    pixels: torch.Tensor        # uint8 [bytes]
    src_table: torch.Tensor     # int32 [n, 8] = {byte offset, h, w, x0, y0, cw, ch, flip}
    dst_table: torch.Tensor     # int32 [n, 3] = {0, nh, nw}: what `ingest.level_constants` takes
    coeffs: torch.Tensor        # int32 [words]
    ends: torch.Tensor          # int32 [sum of runs] (at least one word)
    mask_rows: torch.Tensor     # int32 [m, 4] = {ends offset, n_runs, frame index, output byte offset}
    ids: torch.Tensor           # int32 [m]: the masks' instance ids
    size: tuple                 # (H, W) the step is padded to
    layout: str
    mask_bytes: int
    groups: tuple               # per frame (first mask, masks, nh, nw): the masks of a frame are consecutive
    mask_src: torch.Tensor      # src_table / dst_table of the frames AND the pseudo-frames of polygon masks (the rows
    mask_dst: torch.Tensor      # mask_rows index); src_table and dst_table above are their first n rows
    win_table: torch.Tensor     # int32 [k, 16], the rows of `resize_window_bytes`: k = 0 unless a step of ChainPlans needs it
    win_size: tuple             # (H1, W1) that launch is padded to
    boxes: object = None        # a step of ChainPlans: fp32 [m, 4], the masks' boxes the caller computed (`chain_boxes`)
    color: object = None        # a step with a colour weight: int32 [n, 8] (`color_words`); None: the plain launch
    workspace: int = -1         # ... with contrast, on the device: the byte offset inside `pixels` of the kernels' workspace

    def mask_views(self, masks):
        """the flat output of `augment_masks` -> per frame bool [n_inst, nh, nw] (views)"""
        rows, out, off = masks.view(torch.bool), [], 0
        for _, k, nh, nw in self.groups:
            out.append(rows[off:off + k * nh * nw].view(k, nh, nw))
            off += k * nh * nw
        return out


def _frame_sources(frames, sizes, plan):
    """a step of FramePlans -> (src rows, [(tensor, byte offset)], source bytes, window rows, slot bytes): every frame at
    the next 16-byte offset, its window in its row"""
    src, off = np.zeros((len(plan), SRC_WORDS), dtype=np.int32), 0
    for row, (h, w), p in zip(src, sizes, plan):
        row[:] = (off, h, w, p.x0, p.y0, p.cw, p.ch, int(p.flip))
        off += ingest._align16(3 * h * w)
    return src, list(zip(frames, src[:, 0].tolist())), off, [], 0


def _chain_sources(frames, sizes, plan):
    """a step of ChainPlans -> the same: a source listed twice (the pair of one image) is placed once; a frame that is
    resampled twice gets a window row and a slot behind the sources, which its src row then names as its source"""
    placed, off = {}, 0
    for f, (h, w) in zip(frames, sizes):
        if id(f) not in placed:
            placed[id(f)] = (f, off)
            off += ingest._align16(3 * h * w)
    src, win, slot = np.zeros((len(plan), SRC_WORDS), dtype=np.int32), [], off
    for row, f, (h, w), p in zip(src, frames, sizes, plan):
        assert p.inside(h, w), "stage_step: a ChainPlan of another frame, or a window outside (h1, w1)"
        at = placed[id(f)][1]
        if p.resamples_twice:                # the window of the unflipped resized frame -> its slot; the flip comes last
            win.append([at, h, w, p.h1, p.w1, p.mirrored_x0, p.y0, p.cw, p.ch, slot] + [0] * 6)
            row[:] = (slot, p.ch, p.cw, 0, 0, p.cw, p.ch, int(p.flip))
            slot += ingest._align16(3 * p.ch * p.cw)
        else:                                # one resample: the (mirrored) window of the source itself
            row[:] = (at, h, w, p.mirrored_x0, p.y0, p.cw, p.ch, int(p.flip))
    return src, list(placed.values()), off, win, slot - off


def _mask_rows(masks, plan):
    """-> (mask rows int32 [m, 4], the staged run ends, groups, {frame: row of its pseudo-frame}, the output's bytes); a
    PolyRuns mask names its pseudo-frame, and its ends offset counts from the END of the staged ones"""
    n = len(plan)
    rows, ends, e_at, o_at = np.zeros((len(masks), MASK_ROW_WORDS), dtype=np.int32), [], 0, 0
    groups, pseudo, last = [[0, 0, p.nh, p.nw] for p in plan], {}, -1
    for i, (f, counts) in enumerate(masks):
        assert f >= last, "stage_step: the masks of a frame are consecutive, the frames ascending"
        if f != last:
            groups[f][0] = i
        last = f
        groups[f][1] += 1
        if isinstance(counts, PolyRuns):
            rows[i] = (counts.offset, counts.size, pseudo.setdefault(f, n + len(pseudo)), o_at)
        else:
            e = np.cumsum(np.asarray(counts, dtype=np.int64))
            assert e.size >= 1 and e[-1] <= 0x7fffffff
            rows[i] = (e_at, e.size, f, o_at)
            ends.append(e.astype(np.int32))
            e_at += e.size
        o_at += plan[f].nh * plan[f].nw
    ends = np.concatenate(ends) if ends else np.zeros(1, dtype=np.int32)
    rows[rows[:, 2] >= n, 0] += ends.size    # the device-resident ends follow the staged ones
    return rows, ends, tuple(tuple(g) for g in groups), pseudo, int(o_at)


_SOURCES = {FramePlan: (_frame_sources, False), ChainPlan: (_chain_sources, True)}      # (layout, the boxes ride along)


def stage_step(frames, plan, masks, device, layout: str = "chw", ids=None, poly_ends=None, boxes=None) -> Staged:
    """frames: uint8 CPU tensors of `layout`; plan: a FramePlan per frame; masks: [(frame index, COCO counts)] with the masks
    of a frame CONSECUTIVE and the frames ascending; ids: the masks' instance ids (default 0).  A mask may be a
    `PolyRuns(offset, size)` instead of counts: its run ends are words [offset, offset + size) of `poly_ends` (int32 on
    `device`, at the frame's target size).  plan may be a ChainPlan per frame instead (its masks are PolyRuns; boxes: the
    masks' boxes, fp32 [m, 4], packed into the same upload).  See the module docstring."""
    device = torch.device(device)
    n, m = len(frames), len(masks)
    kinds = {type(p) for p in plan} or {FramePlan}
    assert len(kinds) == 1, "stage_step: ChainPlans or FramePlans, not both"
    sources, with_boxes = _SOURCES[kinds.pop()]
    src, uploads, nbytes, win, slots = sources(frames, [resize.frame_size(f, layout) for f in frames], plan)
    rows, ends, groups, pseudo, mask_bytes = _mask_rows(masks, plan)
    assert not pseudo or (poly_ends is not None and poly_ends.is_cuda and device.type == "cuda"), \
        "stage_step: polygon masks take device-resident run ends"
    # a pseudo-frame: the target as its own source (the full window, no flip); the mask kernel reads no pixels
    full = [full_plan(plan[f].nh, plan[f].nw, plan[f].nh, plan[f].nw) for f in pseudo]
    src = np.concatenate([src] + [np.array([(0, p.ch, p.cw, 0, 0, p.cw, p.ch, 0)], dtype=np.int32) for p in full])
    dst = np.array([(0, p.nh, p.nw) for p in list(plan) + full], dtype=np.int32).reshape(n + len(full), 3)
    words, win = window_words(coeff_words(list(plan) + full), win)      # the first resample's tables ride behind the others
    idv = np.zeros(m, dtype=np.int32) if ids is None else np.asarray(ids, dtype=np.int32).reshape(m)
    ints = [src, dst, words, ends, rows, idv, win]
    colored = any(p.color != NO_COLOR for p in plan)
    workspace = -1
    if colored:                              # (never a chain step: the table rides last, nothing else moves)
        ints.append(color_words(plan))
        if device.type == "cuda" and any(p.contrast is not None for p in plan):
            workspace, slots = nbytes + slots, slots + color_workspace(n, *padded_size(plan))
    if with_boxes:
        box_bits = np.zeros((m, 4), dtype=np.float32) if boxes is None else np.asarray(boxes, dtype=np.float32).reshape(m, 4)
        ints.append(box_bits.view(np.int32))
    (src_d, dst_d, words_d, ends_d, rows_d, ids_d, win_d, *rest), pixels = ingest.pack_upload(
        ints, uploads, nbytes, device, extra=slots)
    color_d, box_d = (rest[0], rest[1:]) if colored else (None, rest)
    if pseudo:
        ends_d = torch.cat((ends_d, poly_ends.to(torch.int32)))
    win_size = ingest.padded_hw([(r[8], r[7]) for r in win.tolist()] or [(1, 1)])
    return Staged(pixels, src_d[:n], dst_d[:n], words_d, ends_d, rows_d, ids_d, padded_size(plan), layout, mask_bytes, groups,
                  src_d, dst_d, win_d, win_size, box_d[0].view(torch.float32) if box_d else None, color_d, workspace)


def _plan_of(staged: Staged):
    n = staged.src_table.shape[0]
    colors = [NO_COLOR] * n if staged.color is None else [color_of(r) for r in staged.color.tolist()]
    return [FramePlan(x0, y0, cw, ch, nh, nw, bool(fl), *c) for (_, _, _, x0, y0, cw, ch, fl), (_, nh, nw), c
            in zip(staged.src_table.tolist(), staged.dst_table.tolist(), colors)]


# ---- the ops ----------------------------------------------------------------------------------------------------------------
def resize_window_bytes(staged: Staged) -> None:
    """The first resample of a step of ChainPlans: every row of `staged.win_table` -> the bytes of its slot inside
    `staged.pixels` (in place).  One launch on the current stream, before `augment_frames`; none when the step has no such
    frame (or is not a chain step)."""
    win, pixels, layout = staged.win_table, staged.pixels, staged.layout
    if win.shape[0] == 0:
        return
    if not pixels.is_cuda:
        ah, aw = resize._hw_axes(layout)
        for o, h, w, h1, w1, x0, y0, cw, ch, d in (r[:10] for r in win.tolist()):
            f = pixels[o:o + 3 * h * w].view((3, h, w) if layout == "chw" else (h, w, 3))
            sl = [slice(None)] * 3
            sl[ah], sl[aw] = slice(y0, y0 + ch), slice(x0, x0 + cw)
            pixels[d:d + 3 * ch * cw].copy_(resize.reference_resize(f, h1, w1, layout)[tuple(sl)].reshape(-1))
        return
    H1, W1 = staged.win_size
    with torch.cuda.device(pixels.device):
        _lib.check(_lib.lib().vnx_resize_window_bytes(
            pixels.data_ptr(), pixels.numel(), win.data_ptr(), staged.coeffs.data_ptr(), staged.coeffs.numel(),
            win.shape[0], H1, W1, int(layout == "hwc"), _lib.current_stream(pixels)))
    BYTES_CALLS["resize_window_bytes"] += 1


def augment_frames(staged: Staged, mean, std, channels_last: bool = False):
    """-> (x fp32 [B, 3, H, W], mask bool [B, H, W]) of the augmented frames; one launch -- with a colour table the launch
    that also applies brightness and saturation, and one more when a frame asks for contrast"""
    pixels, layout, (H, W) = staged.pixels, staged.layout, staged.size
    B = staged.src_table.shape[0]
    if not pixels.is_cuda:
        frames = [pixels[o:o + 3 * h * w].view((3, h, w) if layout == "chw" else (h, w, 3))
                  for o, h, w in (r[:3] for r in staged.src_table.tolist())]
        out = [f if layout == "chw" else f.permute(2, 0, 1).contiguous()
               for f in reference_augment_frames(frames, _plan_of(staged), layout)]
        return ingest.ingest_frames(*ingest.stage_frames(out, "cpu"), B, H, W, mean, std, channels_last)
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    x = torch.empty((B, 3, H, W), dtype=torch.float32, device=pixels.device, memory_format=fmt)
    mask = torch.empty((B, H, W), dtype=torch.bool, device=pixels.device)
    with torch.cuda.device(pixels.device):
        if staged.color is None:
            _lib.check(_lib.lib().vnx_augment_frames(
                pixels.data_ptr(), pixels.numel(), staged.src_table.data_ptr(), staged.dst_table.data_ptr(),
                staged.coeffs.data_ptr(), staged.coeffs.numel(), B, H, W, *ingest._stats(mean), *ingest._stats(std),
                int(bool(channels_last)), int(layout == "hwc"), x.data_ptr(), mask.data_ptr(), _lib.current_stream(pixels)))
        else:
            contrast = staged.workspace >= 0
            _lib.check(_lib.lib().vnx_augment_frames_color(
                pixels.data_ptr(), pixels.numel(), staged.src_table.data_ptr(), staged.dst_table.data_ptr(),
                staged.coeffs.data_ptr(), staged.coeffs.numel(), staged.color.data_ptr(), B, H, W, *ingest._stats(mean),
                *ingest._stats(std), int(bool(channels_last)), int(layout == "hwc"), int(contrast),
                max(staged.workspace, 0), x.data_ptr(), mask.data_ptr(), _lib.current_stream(pixels)))
            COLOR_CALLS["augment_frames_color"] += 1
            COLOR_CALLS["launches"] += 1 + contrast
    CALLS["augment_frames"] += 1
    return x, mask


def augment_masks(staged: Staged):
    """-> (masks uint8 [mask_bytes], boxes fp32 [m, 4], nonempty bool [m]); two launches (none for m == 0)"""
    m, dev = staged.mask_rows.shape[0], staged.ends.device
    if not staged.ends.is_cuda:
        ends, rows = staged.ends.numpy(), staged.mask_rows.tolist()
        listed = [(f, np.diff(ends[o:o + k], prepend=0)) for o, k, f, _ in rows]
        sizes = [tuple(r[1:3]) for r in staged.src_table.tolist()]
        outs, boxes, flags = reference_augment_masks(listed, sizes, _plan_of(staged))
        flat = np.concatenate([o.reshape(-1) for o in outs]) if outs else np.zeros(0, dtype=bool)
        return torch.from_numpy(flat.astype(np.uint8)), torch.from_numpy(boxes), torch.from_numpy(flags)
    H, W = staged.size
    masks = torch.empty(max(staged.mask_bytes, 1), dtype=torch.uint8, device=dev)[:staged.mask_bytes]
    boxes = torch.empty((m, 4), dtype=torch.float32, device=dev)
    nonempty = torch.empty(m, dtype=torch.bool, device=dev)
    if m == 0:
        return masks, boxes, nonempty
    lib = _lib.lib()
    work = torch.empty(int(lib.vnx_augment_masks_workspace(m, H, W)), dtype=torch.uint8, device=dev)
    src, dst = staged.mask_src, staged.mask_dst
    with torch.cuda.device(dev):
        _lib.check(lib.vnx_augment_masks(
            staged.ends.data_ptr(), staged.ends.numel(), staged.mask_rows.data_ptr(), m, src.data_ptr(),
            dst.data_ptr(), staged.coeffs.data_ptr(), staged.coeffs.numel(), src.shape[0], H, W,
            masks.data_ptr(), masks.numel(), boxes.data_ptr(), nonempty.data_ptr(), work.data_ptr(), work.numel(),
            _lib.current_stream(staged.ends)))
    CALLS["augment_masks"] += 1
    return masks, boxes, nonempty
