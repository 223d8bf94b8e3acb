"""A numpy stand-in for the four `pycocotools.mask` calls the YouTube-VIS cocoapi fork makes (`area`, `merge`,
`frPyObjects`, `toBbox`), built on vnext_amd/utils/ytvis_json.py.  pycocotools is a compiled third-party package that
is not installed here; tools/make_golden_ytvis_eval.py registers this module under its name to run the reference's
evaluator.  An RLE object is {"size": [h, w], "counts": str or bytes}, as pycocotools has it.

Only what that evaluator needs: no `iou`, no `encode` / `decode`.  `frPyObjects` also takes polygons and boxes, through
this package's restatement of `rleFrPoly` (vnext_amd/ops/poly_rle.py poly_counts_host) -- a restatement, never compared with
the compiled package.
"""
from __future__ import annotations

import numpy as np

from vnext_amd.ops.poly_rle import object_polygons, poly_counts_host
from vnext_amd.utils.ytvis_json import counts_to_string, rle_counts, string_to_counts


def _counts(rle):
    c = rle["counts"]
    if isinstance(c, bytes):
        c = c.decode("ascii")
    return string_to_counts(c) if isinstance(c, str) else [int(x) for x in c]


def _flat(rle):
    """the mask as a flat column-major 0/1 array"""
    counts = np.asarray(_counts(rle), dtype=np.int64)
    h, w = rle["size"]
    assert (counts >= 0).all() and int(counts.sum()) == h * w, "malformed RLE"
    return np.repeat(np.arange(len(counts)) & 1, counts).astype(np.uint8)


def _from_flat(flat, size):
    h, w = size
    return {"size": [int(h), int(w)], "counts": counts_to_string(rle_counts(flat.reshape((h, w), order="F")))}


def area(rles):
    """set pixels: a uint32 scalar for one RLE object, a uint32 array for a list"""
    if isinstance(rles, dict):
        return area([rles])[0]
    return np.array([sum(_counts(r)[1::2]) for r in rles], dtype=np.uint32)


def merge(rles, intersect=False):
    """union (intersect false) or intersection of RLE objects of one size"""
    size = list(rles[0]["size"])
    out = _flat(rles[0])
    for r in rles[1:]:
        if list(r["size"]) != size:
            raise ValueError("merge: masks of different sizes")
        out = (out & _flat(r)) if intersect else (out | _flat(r))
    return _from_flat(out, size)


def frPyObjects(obj, h, w):
    """uncompressed RLE ({"size", "counts": list}) -> RLE object; a list of them -> a list.  A list of polygons or of boxes
    -> a list of RLE objects, one per polygon / box (merge them for the annotation's mask); one flat polygon or one box
    [x, y, w, h] -> one RLE object."""
    if isinstance(obj, list) and all(isinstance(o, dict) for o in obj):
        return [frPyObjects(o, h, w) for o in obj]
    if isinstance(obj, dict) and "counts" in obj:
        assert list(obj["size"]) == [h, w]
        return {"size": [int(h), int(w)], "counts": counts_to_string(obj["counts"])}
    if isinstance(obj, (list, tuple, np.ndarray)) and len(obj):
        rles = [{"size": [int(h), int(w)], "counts": counts_to_string(poly_counts_host(p, h, w))} for p in object_polygons(obj)]
        return rles if isinstance(obj[0], (list, tuple, np.ndarray)) else rles[0]
    raise NotImplementedError("pycocotools stand-in: uncompressed RLE, polygons or boxes")


def toBbox(rles):
    """[x, y, w, h] of the set pixels (zeros for an empty mask)"""
    if isinstance(rles, dict):
        return toBbox([rles])[0]
    out = np.zeros((len(rles), 4), dtype=np.float64)
    for i, r in enumerate(rles):
        h, w = r["size"]
        ys, xs = np.nonzero(_flat(r).reshape((h, w), order="F"))
        if len(ys):
            out[i] = (xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1)
    return out
