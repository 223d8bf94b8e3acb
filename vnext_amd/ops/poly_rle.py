"""COCO polygons to run tables (vnext_amd/csrc/poly_rle.hip): pycocotools' `frPyObjects` + `merge` for polygon and box
segmentations, on the device or in numpy.

`poly_counts_host` restates `rleFrPoly` of the COCO mask API step by step (upsample the vertices by 5, walk every edge as a
dense point sequence, take the column crossings, sort, difference, fold the zero differences), `merge_counts_host` is
`rleMerge` with intersect = 0 (the union) and `object_counts_host` what `frPyObjects` + `merge` give for one annotation.
They are the CPU route and the oracle of the kernel, which is held to them count for count.  pycocotools itself was not
available where this was written: the restatement is checked on its own merits (tests/test_poly_rle.py), not against the
package.

`polygons_to_runs` turns a list of annotations into `RunTables` (vnext_amd/ops/video_iou.py) -- with a CUDA device one
launch of vnx_poly_rle, the run arena sized on the host from the coordinates (no device-to-host read); objects beyond the
kernel's caps go through the host functions and are spliced in.
"""
from __future__ import annotations

import numpy as np

from .. import _lib
from .video_iou import RunTables, _pixels, runs_from_counts

SCALE = 5.0                                   # rleFrPoly's upsampling factor
COORD_LIMIT = float(2 ** 24)                  # |coordinate| beyond this is refused (the kernel's int32 arithmetic)

STATUS_TEXT = {_lib.POLY_RLE_BAD_COORD: "a coordinate that is not finite or beyond 2^24 in magnitude",
               _lib.POLY_RLE_FEW_VERTICES: "a polygon of fewer than 3 vertices",
               _lib.POLY_RLE_BAD_SIZE: "height * width outside [1, 2^31)",
               _lib.POLY_RLE_CAP: "more vertices, dense points, crossings or polygons than the kernel's caps",
               _lib.POLY_RLE_BAD_SLOT: "a row or a run slot outside its arena, or a slot too small"}


def status_text(status):
    return "; ".join(t for bit, t in STATUS_TEXT.items() if status & bit) or "ok"


def _check_size(h, w):
    h, w = int(h), int(w)
    if h < 1 or w < 1 or h * w >= 2 ** 31:
        raise ValueError(f"polygon masks need 1 <= height * width < 2^31, got {h} x {w}")
    return h, w


def _flat_polygon(xy):
    xy = np.asarray(xy, dtype=np.float64).reshape(-1)
    if len(xy) < 6 or len(xy) % 2:
        raise ValueError(f"a polygon is a flat [x0, y0, x1, y1, ...] of at least 6 and an even number of values, got {len(xy)}")
    if not np.isfinite(xy).all() or (np.abs(xy) > COORD_LIMIT).any():
        raise ValueError("a polygon coordinate is not finite or beyond 2^24 in magnitude")
    return xy


def upsampled_vertices(xy):
    """The integer vertices of rleFrPoly: (int)(5 * c + 0.5), the cast truncating toward zero -> (X, Y) int64 [k]."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1)
    q = np.trunc(SCALE * xy + 0.5).astype(np.int64)
    return q[0::2], q[1::2]


def dense_points(X, Y, fused=False):
    """The dense point sequence (u, v) of the closed ring X, Y (int64 [k]).  `fused=True` evaluates the two line
    expressions as a contracted build would: ys + s * t as ONE rounding (a fused multiply-add), then + 0.5 -- the form
    the kernel must NOT take; the tests use it to prove that they can tell the two apart."""
    xs, ys = X, Y
    xe, ye = np.roll(X, -1), np.roll(Y, -1)
    dx, dy = np.abs(xe - xs), np.abs(ys - ye)
    xmaj = dx >= dy
    flip = (xmaj & (xs > xe)) | (~xmaj & (ys > ye))
    xs, xe = np.where(flip, xe, xs), np.where(flip, xs, xe)
    ys, ye = np.where(flip, ye, ys), np.where(flip, ys, ye)
    n = np.maximum(dx, dy)
    num = np.where(xmaj, ye - ys, xe - xs).astype(np.float64)
    # a zero-length edge has s = 0 / 0 in the original; its one point's v is never read (u equals both neighbours'), so 0
    s = np.divide(num, n.astype(np.float64), out=np.zeros(len(n), dtype=np.float64), where=n > 0)
    cnt = n + 1
    first = np.cumsum(cnt) - cnt
    e = np.repeat(np.arange(len(cnt)), cnt)
    d = np.arange(int(cnt.sum()), dtype=np.int64) - first[e]
    t = np.where(flip[e], n[e] - d, d)
    base = np.where(xmaj, ys, xs)[e]
    mac = base.astype(np.float64) + s[e] * t.astype(np.float64)                    # a product, then an addition
    if fused:
        # exact rational arithmetic rounded once, where one rounding more or less can move the truncation at all: the two
        # forms differ by at most one unit in the last place, so only sums that close to an integer are redone
        from fractions import Fraction
        near = np.flatnonzero(np.abs((mac + 0.5) - np.rint(mac + 0.5)) <= 4 * np.spacing(np.abs(mac) + 1.0))
        for i in near:
            mac[i] = float(Fraction(float(s[e[i]])) * int(t[i]) + int(base[i]))
    line = mac + 0.5
    r = np.trunc(line).astype(np.int64)
    lin = t + np.where(xmaj, xs, ys)[e]
    u = np.where(xmaj[e], lin, r)
    v = np.where(xmaj[e], r, lin)
    return u, v


def column_of(xd):
    """Integer form of step 3's column test: the pixel column of upsampled x `xd`, or None when (xd + 0.5) / 5 - 0.5 is
    not an integer.  Equal to the floating form for every residue and sign (tests/test_poly_rle.py)."""
    return (xd - 2) // 5 if (xd - 2) % 5 == 0 else None


def row_of(yd, h):
    """Integer form of step 3's row: ceil of (yd + 0.5) / 5 - 0.5 clamped to [0, h]."""
    return min(max(-((2 - yd) // 5), 0), h)


def crossings(u, v, h, w):
    """Step 3 in the floating form of the original -> the positions xd * h + yd (int64, unsorted)."""
    i = np.flatnonzero(u[1:] != u[:-1]) + 1
    xd = np.where(u[i] < u[i - 1], u[i], u[i] - 1).astype(np.float64)
    xd = (xd + 0.5) / SCALE - 0.5
    keep = (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
    yd = np.minimum(v[i], v[i - 1]).astype(np.float64)
    yd = (yd + 0.5) / SCALE - 0.5
    yd = np.ceil(np.minimum(np.maximum(yd, 0.0), float(h)))
    return (xd[keep] * h + yd[keep]).astype(np.int64)


def runs_of_positions(pos, h, w):
    """Step 4, as the original writes it: append h * w, sort, difference, fold the zero differences."""
    a = np.sort(np.concatenate((np.asarray(pos, dtype=np.int64), [h * w])))
    a = np.diff(a, prepend=0).tolist()
    b, j, k = [a[0]], 1, len(a)
    while j < k:
        if a[j] > 0:
            b.append(a[j])
            j += 1
        else:
            j += 1
            if j < k:
                b[-1] += a[j]
                j += 1
    return b


def poly_counts_host(xy, h, w, fused=False):
    """One polygon, flat [x0, y0, x1, y1, ...] (float64, at least 3 vertices) -> its COCO counts on an h x w canvas."""
    h, w = _check_size(h, w)
    X, Y = upsampled_vertices(_flat_polygon(xy))
    u, v = dense_points(X, Y, fused=fused)
    return runs_of_positions(crossings(u, v, h, w), h, w)


def merge_counts_host(list_of_counts, h, w):
    """The union of several masks given as COCO counts: `mask.merge(rles)` with intersect = 0.  One list comes back as it is."""
    h, w = _check_size(h, w)
    hw = h * w
    if len(list_of_counts) == 0:
        return [hw]
    if len(list_of_counts) == 1:
        return [int(c) for c in list_of_counts[0]]
    starts, stops = [], []
    for c in list_of_counts:
        if sum(int(x) for x in c) != hw:
            raise ValueError(f"merge_counts_host: runs that sum to {sum(c)}, not to height * width = {hw}")
        e = np.cumsum(np.asarray(c, dtype=np.int64))
        s, t = e[0::2], e[1::2]
        starts.append(s[:len(t)])                  # the set runs [s, t); a last even-indexed end is h * w itself
        stops.append(t)
    pos = np.concatenate(starts + stops)
    delta = np.concatenate([np.ones(len(s), np.int64) for s in starts] + [-np.ones(len(t), np.int64) for t in stops])
    order = np.argsort(pos, kind="stable")
    pos, delta = pos[order], delta[order]
    upos, first = np.unique(pos, return_index=True)
    cover = np.cumsum(np.add.reduceat(delta, first)) if len(pos) else np.zeros(0, np.int64)
    state = cover > 0
    change = state != np.concatenate(([False], state[:-1]))
    tog = upos[change]
    tog = tog[(tog < hw)]
    # set runs of zero length cannot arise from canonical inputs; an input [0, n, ...] toggles at 0 and gives b[0] = 0
    return np.diff(np.concatenate(([0], tog, [hw]))).astype(np.int64).tolist()


def _box_polygon(b):
    xs, ys, bw, bh = (float(x) for x in b)
    xe, ye = xs + bw, ys + bh
    return [xs, ys, xs, ye, xe, ye, xe, ys]


def object_polygons(segmentation):
    """One annotation's segmentation -> the list of flat float64 polygons frPyObjects would rasterise: a list of polygons,
    one flat polygon, a box [x, y, w, h] (exactly 4 numbers) or a list of boxes.  ValueError for anything else."""
    if isinstance(segmentation, np.ndarray):
        segmentation = segmentation.tolist() if segmentation.ndim > 1 else [segmentation]
    if isinstance(segmentation, dict) or isinstance(segmentation, (str, bytes)) or not hasattr(segmentation, "__len__"):
        raise ValueError("object_polygons: a polygon list, one flat polygon or a box [x, y, w, h] is needed")
    if len(segmentation) == 0:
        return []
    if not hasattr(segmentation[0], "__len__"):
        segmentation = [segmentation]                                  # one flat polygon or one box
    polys = []
    for p in segmentation:
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        polys.append(_flat_polygon(_box_polygon(p) if len(p) == 4 else p))
    return polys


def object_counts_host(segmentation, h, w):
    """frPyObjects + merge for one annotation (see object_polygons); an empty polygon list is the empty mask."""
    h, w = _check_size(h, w)
    return merge_counts_host([poly_counts_host(p, h, w) for p in object_polygons(segmentation)], h, w)


def counts_to_mask(counts, h, w):
    """COCO counts -> bool [h, w] (column-major runs, zeros first)."""
    bits = np.repeat(np.arange(len(counts)) & 1, np.asarray(counts, dtype=np.int64)).astype(bool)
    return bits.reshape(w, h).T


def mask_to_counts(mask):
    """bool [h, w] -> canonical COCO counts."""
    flat = np.asarray(mask, dtype=bool).T.reshape(-1)
    tog = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    if len(flat) and flat[0]:
        tog = np.concatenate(([0], tog))
    return np.diff(np.concatenate(([0], tog, [len(flat)]))).astype(np.int64).tolist()


# ---- the device route ----------------------------------------------------------------------------------------------

def crossing_bound(X, w):
    """The host's bound on one polygon's crossings from its integer vertices: sum over the edges of
    min(|X[j+1] - X[j]| / 5 + 1, w), plus 1."""
    dX = np.abs(np.roll(X, -1) - X)
    return int(np.minimum(dX // 5 + 1, w).sum()) + 1


def _dense_count(X, Y):
    return int((np.maximum(np.abs(np.roll(X, -1) - X), np.abs(np.roll(Y, -1) - Y)) + 1).sum())


def plan_objects(objects, sizes):
    """The host half of the device route: per object its polygons, its run-slot size (the sum of the polygons' crossing
    bounds + 1) and whether it fits the kernel's caps.  -> (polys: list of lists of float64 arrays, slots int64 [M],
    fits bool [M]).  ValueError, naming the object, for what no route takes."""
    polys, slots, fits = [], np.zeros(len(objects), np.int64), np.ones(len(objects), bool)
    for m, (seg, (h, w)) in enumerate(zip(objects, sizes)):
        try:
            ps = object_polygons(seg)
        except ValueError as e:
            raise ValueError(f"object {m}: {e}") from None
        bound, dense = 0, 0
        for p in ps:
            X, Y = upsampled_vertices(p)
            b = crossing_bound(X, int(w))
            bound += b
            dense += _dense_count(X, Y)
            fits[m] &= len(X) <= _lib.POLY_RLE_MAX_VERTICES and b <= _lib.POLY_RLE_MAX_CROSSINGS
        fits[m] &= (bound <= _lib.POLY_RLE_MAX_CROSSINGS and dense <= _lib.POLY_RLE_MAX_POINTS
                    and len(ps) <= _lib.POLY_RLE_MAX_POLYGONS)
        slots[m] = bound + 1
        polys.append(ps)
    return polys, slots, fits


def fits_caps(objects, sizes):
    """True when every object stays inside the kernel's caps (what `augment.applies` asks for a polygon step)."""
    return bool(plan_objects(objects, sizes)[2].all())


def pack_tables(polys, sizes, slots):
    """numpy tables of vnx_poly_rle for objects that all run on the device: (coords float64 [C], poly_rows int32 [P, 4] =
    {coordinate offset, vertices, object, 0}, obj_rows int32 [M, 6] = {first polygon, polygons, run-slot offset, slot
    size, h, w}, total run slots)."""
    coords, prow, orow, off, coff = [], [], [], 0, 0
    for m, (ps, (h, w)) in enumerate(zip(polys, sizes)):
        orow.append((len(prow), len(ps), off, int(slots[m]), int(h), int(w)))
        for p in ps:
            prow.append((coff, len(p) // 2, m, 0))
            coords.append(p)
            coff += len(p)
        off += int(slots[m])
    if off >= 2 ** 31 or coff >= 2 ** 31:
        raise ValueError("polygons_to_runs: 2^31 run slots or coordinates in one call (int32 offsets)")
    return (np.concatenate(coords) if coords else np.zeros(0, np.float64),
            np.asarray(prow, dtype=np.int32).reshape(-1, 4), np.asarray(orow, dtype=np.int32).reshape(-1, 6), off)


def poly_rle_device(coords, poly_rows, obj_rows, run_slots):
    """vnx_poly_rle on device tensors -> (RunTables, status int32 [M]) on that device; no synchronisation."""
    import torch
    lib = _lib.lib()
    dev = obj_rows.device
    M = int(obj_rows.shape[0])
    ends = torch.empty(max(run_slots, 1), dtype=torch.int32, device=dev)
    ones = torch.empty(max(run_slots, 1), dtype=torch.int32, device=dev)
    rows = torch.empty(M, 4, dtype=torch.int32, device=dev)
    status = torch.empty(M, dtype=torch.int32, device=dev)
    if M:
        with torch.cuda.device(dev):
            _lib.check(lib.vnx_poly_rle(coords.data_ptr(), int(coords.shape[0]), poly_rows.data_ptr(),
                                        int(poly_rows.shape[0]), obj_rows.data_ptr(), M, ends.data_ptr(), ones.data_ptr(),
                                        int(run_slots), rows.data_ptr(), status.data_ptr(), _lib.current_stream(rows)))
    return RunTables(ends[:run_slots], ones[:run_slots], rows), status


def polygons_to_runs(objects, sizes, device=None, check=True, planned=None):
    """objects[m]: one annotation's segmentation (a polygon list, one flat polygon, a box or a list of boxes), sizes[m] =
    (h, w) -> RunTables with one mask per object, in order, and the per-object status in its `.status` attribute (all
    zeros on the host route, which raises instead; a device tensor on the device route).

    With a CUDA `device` the kernel runs and the tables stay there; an object's run slot is sized from the host's crossing
    bound and padded with ends = h * w (rows[., 1] holds the true run count), so nothing is read back.  Objects beyond the
    kernel's caps go through the host functions and are spliced in.  `check=True` reads the status once and raises
    ValueError, naming the object; `check=False` leaves that to the caller (no device-to-host read at all).  `planned`:
    what `plan_objects(objects, sizes)` returned, when the caller has it.  The tables' `.slot_rows` (numpy int64 [M, 2] =
    {offset, words} of each object's slot of ends / ones, known on the host) lets a consumer address the padded slots."""
    objects, sizes = list(objects), [(int(h), int(w)) for h, w in sizes]
    if len(objects) != len(sizes):
        raise ValueError(f"polygons_to_runs: {len(objects)} objects, {len(sizes)} sizes")
    _pixels(sizes)
    if device is None or str(device) == "cpu":
        counts = []
        for m, (seg, (h, w)) in enumerate(zip(objects, sizes)):
            try:
                counts.append(object_counts_host(seg, h, w))
            except ValueError as e:
                raise ValueError(f"object {m}: {e}") from None
        tables = runs_from_counts(counts, sizes)
        tables.status = np.zeros(len(objects), dtype=np.int32)
        tables.slot_rows = tables.rows[:, :2].astype(np.int64)
        return tables
    import torch
    dev = torch.device(device)
    polys, slots, fits = plan_objects(objects, sizes) if planned is None else planned
    host = np.flatnonzero(~fits)
    dev_polys = [ps if fits[m] else [] for m, ps in enumerate(polys)]          # a host-route object: an empty device slot
    dev_slots = np.where(fits, slots, 1)
    coords, prow, orow, total = pack_tables(dev_polys, sizes, dev_slots)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a) if a.size else np.zeros((1,) + a.shape[1:], a.dtype)).to(dev)  # noqa: E731
    tables, status = poly_rle_device(up(coords)[:len(coords)], up(prow)[:len(prow)], up(orow)[:len(orow)], total)
    slot_rows = orow[:, 2:4].astype(np.int64)
    if len(host):
        extra = runs_from_counts([object_counts_host(objects[m], *sizes[m]) for m in host], [sizes[m] for m in host])
        rows_h = extra.rows.copy()
        rows_h[:, 0] += total
        if total + len(extra.ends) >= 2 ** 31:
            raise ValueError("polygons_to_runs: 2^31 run slots in one call (int32 offsets)")
        rows = tables.rows.index_copy(0, up(host.astype(np.int64)), up(rows_h))
        slot_rows[host] = rows_h[:, :2]
        tables = RunTables(torch.cat((tables.ends, up(extra.ends))), torch.cat((tables.ones, up(extra.ones))), rows)
    if check and len(objects):
        st = status.cpu().numpy()
        bad = np.flatnonzero(st)
        if len(bad):
            raise ValueError(f"polygons_to_runs: object {int(bad[0])}: {status_text(int(st[bad[0]]))}"
                             + (f" ({len(bad)} such objects)" if len(bad) > 1 else ""))
    tables.status, tables.slot_rows = status, slot_rows
    return tables
