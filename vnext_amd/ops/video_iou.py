"""Video mask IoU from run lengths (vnext_amd/csrc/video_iou.hip): the expensive part of the YTVIS evaluator.

`YTVOSeval.computeIoU` forms, for a detection track d and a ground-truth track g of one video,

    iou = sum_f |d_f & g_f| / sum_f |d_f | g_f|          (an absent mask is the empty set; 0.0 when the union is empty)

with two RLE merges and two areas per frame in a Python double loop.  Both sums are integers, so here they are taken
from run tables and come out exact: iou = I / (A_d + A_g - I) with I, A_d, A_g the frame sums of the intersection and
of the two areas, one double division on the host.

Run tables: a mask is a slice of two int32 arenas, `ends[k]` = the column-major pixel index at which run k ends (the
cumulative sum of the COCO counts, run 0 counts zeros) and `ones[k]` = the set pixels below `ends[k]`; a row per mask
holds {arena offset, runs, pixel count, area}.  A pixel's bit is the parity of the upper bound of its index in `ends`.

`runs_from_counts` builds the tables in numpy (uncompressed ground truth; the CPU path; the oracle of the decode
kernel), `decode_strings` from compressed strings on the device (CUDA) or through `string_counts_checked` (CPU);
`pair_sums` is the kernel (tables on a CUDA device) or `pair_sums_host` (numpy tables).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .. import _lib

STATUS_TEXT = {_lib.RLE_RUNS_BAD_BYTE: "a byte outside 48..111", _lib.RLE_RUNS_TRUNCATED: "the string ends inside a count",
               _lib.RLE_RUNS_NEGATIVE: "a negative count (or one of more than 7 characters)",
               _lib.RLE_RUNS_BAD_SUM: "the runs do not sum to height * width",
               _lib.RLE_RUNS_BAD_SLOT: "the string or its run slot lies outside its arena"}


def status_text(status):
    return "; ".join(t for bit, t in STATUS_TEXT.items() if status & bit) or "ok"


@dataclass
class RunTables:
    """ends, ones: int32 [R]; rows: int32 [M, 4] = {offset, runs, pixels, area}.  numpy arrays or tensors of one device."""
    ends: object
    ones: object
    rows: object

    @property
    def is_cuda(self):
        return bool(getattr(self.rows, "is_cuda", False))

    def __len__(self):
        return int(self.rows.shape[0])

    def to(self, device):
        import torch
        if self.is_cuda:
            return RunTables(self.ends.to(device), self.ones.to(device), self.rows.to(device))
        return RunTables(*(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (self.ends, self.ones, self.rows)))

    def numpy(self):
        if not self.is_cuda:
            return self
        return RunTables(*(a.cpu().numpy() for a in (self.ends, self.ones, self.rows)))


def _pixels(sizes):
    px = np.array([int(h) * int(w) for h, w in sizes], dtype=np.int64).reshape(-1)
    if (px < 1).any() or (px >= 2 ** 31).any():
        raise ValueError("run tables: every mask needs 1 <= height * width < 2^31 (int32 run ends)")
    return px


def runs_from_counts(counts, sizes):
    """counts: a list of COCO count lists (run lengths over the column-major mask, the first run counts zeros), sizes: a
    list of (height, width) -> RunTables (numpy).  ValueError for a negative count or runs that do not sum to h * w."""
    px = _pixels(sizes)
    if len(counts) != len(px):
        raise ValueError(f"runs_from_counts: {len(counts)} count lists, {len(px)} sizes")
    rows = np.zeros((len(px), 4), dtype=np.int32)
    ends, ones, off = [], [], 0
    for m, c in enumerate(counts):
        c = np.asarray(c, dtype=np.int64).reshape(-1)
        if (c < 0).any():
            raise ValueError(f"runs_from_counts: mask {m} has a negative count")
        e = np.cumsum(c, dtype=np.int64)
        if (e[-1] if len(e) else 0) != px[m]:
            raise ValueError(f"runs_from_counts: the runs of mask {m} sum to {int(e[-1]) if len(e) else 0}, "
                             f"not to height * width = {int(px[m])}")
        s = c.copy()
        s[0::2] = 0
        o = np.cumsum(s, dtype=np.int64)
        rows[m] = (off, len(c), px[m], o[-1])
        ends.append(e.astype(np.int32))
        ones.append(o.astype(np.int32))
        off += len(c)
        if off >= 2 ** 31:
            raise ValueError("run tables: 2^31 runs or more in one table (int32 offsets)")
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int32)   # noqa: E731
    return RunTables(cat(ends), cat(ones), rows)


def concat_tables(a, b):
    """The tables of a's masks followed by b's (numpy or one device)."""
    if a.is_cuda != b.is_cuda:
        raise ValueError("concat_tables: one table is on the host, the other on a device")
    if a.is_cuda:
        import torch
        rows_b = b.rows.clone()
        rows_b[:, 0] += int(a.ends.shape[0])
        return RunTables(torch.cat((a.ends, b.ends)), torch.cat((a.ones, b.ones)), torch.cat((a.rows, rows_b)))
    rows_b = b.rows.copy()
    rows_b[:, 0] += len(a.ends)
    return RunTables(np.concatenate((a.ends, b.ends)), np.concatenate((a.ones, b.ones)), np.concatenate((a.rows, rows_b)))


def string_counts_checked(s, pixels):
    """A compressed string -> (counts, status): `ytvis_json.string_to_counts` with the checks of the decode kernel (the
    same status bits); counts is [] when the status is non-zero."""
    data = s.encode("latin-1", "replace") if isinstance(s, str) else bytes(s)
    counts, status, p, n = [], 0, 0, len(data)
    while p < n:
        x, k, more = 0, 0, True
        while more:
            if p >= n:
                return [], status | _lib.RLE_RUNS_TRUNCATED
            c = data[p] - 48
            if c < 0 or c > 63:
                status |= _lib.RLE_RUNS_BAD_BYTE
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if k > 7:
            status |= _lib.RLE_RUNS_NEGATIVE
        if len(counts) > 2:
            x += counts[-2]
        if x < 0:
            status |= _lib.RLE_RUNS_NEGATIVE
        counts.append(x)
    if sum(counts) != pixels:
        status |= _lib.RLE_RUNS_BAD_SUM
    return ([], status) if status else (counts, 0)


def _raise_bad(status, labels):
    bad = np.flatnonzero(status)
    if len(bad):
        m = int(bad[0])
        where = labels[m] if labels is not None else f"mask {m}"
        raise ValueError(f"malformed RLE string of {where}: {status_text(int(status[m]))}"
                         + (f" ({len(bad)} such masks)" if len(bad) > 1 else ""))


def _string_arena(strings):
    data = [s.encode("latin-1", "replace") if isinstance(s, str) else bytes(s) for s in strings]
    lengths = np.array([len(d) for d in data], dtype=np.int64)
    offsets = np.cumsum(lengths) - lengths
    return np.frombuffer(b"".join(data), dtype=np.uint8).copy(), offsets, lengths


def decode_strings_device(arena, offsets, lengths, pixels):
    """The two launches on device tensors (uint8 [B], int64 [M], int64 [M], int32 [M]) -> (RunTables, status int32 [M]),
    all on that device.  One host read (the total number of runs) sizes the run arenas."""
    import torch
    lib = _lib.lib()
    dev = offsets.device
    M = int(offsets.shape[0])
    if M == 0:
        z = torch.zeros(0, dtype=torch.int32, device=dev)
        return RunTables(z, z.clone(), torch.zeros(0, 4, dtype=torch.int32, device=dev)), z.clone()
    with torch.cuda.device(dev):
        stream = _lib.current_stream(offsets)
        runs = torch.empty(M, dtype=torch.int32, device=dev)
        _lib.check(lib.vnx_rle_runs_measure(arena.data_ptr(), int(arena.shape[0]), offsets.data_ptr(),
                                            lengths.data_ptr(), M, runs.data_ptr(), stream))
        run_ends = runs.cumsum(0, dtype=torch.int64)
        total = int(run_ends[-1])
        if total >= 2 ** 31:
            raise ValueError("run tables: 2^31 runs or more in one table (int32 offsets)")
        run_offsets = (run_ends - runs).to(torch.int32)
        ends = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
        ones = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
        rows = torch.empty(M, 4, dtype=torch.int32, device=dev)
        status = torch.empty(M, dtype=torch.int32, device=dev)
        _lib.check(lib.vnx_rle_runs_write(arena.data_ptr(), int(arena.shape[0]), offsets.data_ptr(), lengths.data_ptr(),
                                          pixels.data_ptr(), run_offsets.data_ptr(), runs.data_ptr(), M, ends.data_ptr(),
                                          ones.data_ptr(), total, rows.data_ptr(), status.data_ptr(), stream))
    return RunTables(ends[:total], ones[:total], rows), status


def decode_strings(strings, sizes, device=None, labels=None):
    """Compressed COCO RLE strings + their (height, width) -> RunTables, on `device` (a CUDA device: the decode kernel)
    or in numpy (None / "cpu").  ValueError for a malformed string, naming `labels[m]` where given."""
    px = _pixels(sizes)
    if len(strings) != len(px):
        raise ValueError(f"decode_strings: {len(strings)} strings, {len(px)} sizes")
    if device is None or str(device) == "cpu":
        counts, status = [], np.zeros(len(px), dtype=np.int32)
        for m, s in enumerate(strings):
            c, status[m] = string_counts_checked(s, int(px[m]))
            counts.append(c)
        _raise_bad(status, labels)
        return runs_from_counts(counts, sizes)
    import torch
    arena, offsets, lengths = _string_arena(strings)
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    tables, status = decode_strings_device(up(arena) if len(arena) else torch.zeros(1, dtype=torch.uint8, device=dev),
                                           up(offsets), up(lengths), up(px.astype(np.int32)))
    _raise_bad(status.cpu().numpy(), labels)
    return tables


def _below(ends, ones, x):
    """set pixels of the mask (its slices of the arenas) below the pixel indices x"""
    if len(ends) == 0:
        return np.zeros(len(x), dtype=np.int64)
    u = np.searchsorted(ends, x, side="right")
    prev = np.maximum(u - 1, 0)
    base = np.where(u > 0, ones[prev].astype(np.int64), 0)
    return base + np.where((u & 1) == 1, x.astype(np.int64) - ends[prev], 0)


def _tracks_and_pairs(frame_mask, tracks, pairs):
    frame_mask = np.ascontiguousarray(np.asarray(frame_mask, dtype=np.int32).reshape(-1))
    tracks = np.ascontiguousarray(np.asarray(tracks, dtype=np.int32).reshape(-1, 2))
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    return frame_mask, tracks, pairs


def pair_sums_host(tables, frame_mask, tracks, pairs):
    """The sums of vnx_video_iou_sums in numpy: int64 [P, 4] = {sum I, sum A_d, sum A_g, status}."""
    t = tables.numpy()
    frame_mask, tracks, pairs = _tracks_and_pairs(frame_mask, tracks, pairs)
    out = np.zeros((len(pairs), 4), dtype=np.int64)
    M, T, F, R = len(t.rows), len(tracks), len(frame_mask), len(t.ends)

    def table(m):
        off, n = int(t.rows[m, 0]), int(t.rows[m, 1])
        if off < 0 or n < 0 or off + n > R:
            return None
        return t.ends[off:off + n], t.ones[off:off + n]
    for p, (d, g) in enumerate(pairs):
        if not (0 <= d < T and 0 <= g < T):
            out[p, 3] = _lib.VIDEO_IOU_BAD_TABLE
            continue
        (fd, nd), (fg, ng) = tracks[d], tracks[g]
        if min(fd, nd, fg, ng) < 0 or fd + nd > F or fg + ng > F:
            out[p, 3] = _lib.VIDEO_IOU_BAD_TABLE
            continue
        if nd != ng:
            out[p, 3] = _lib.VIDEO_IOU_FRAMES
            continue
        acc, status = [0, 0, 0], 0
        for f in range(nd):
            md, mg = int(frame_mask[fd + f]), int(frame_mask[fg + f])
            if md >= M or mg >= M:
                status = _lib.VIDEO_IOU_BAD_TABLE
                break
            ta = table(md) if md >= 0 else ()
            tb = table(mg) if mg >= 0 else ()
            if ta is None or tb is None:
                status = _lib.VIDEO_IOU_BAD_TABLE
                break
            if md >= 0 and mg >= 0:
                if t.rows[md, 2] != t.rows[mg, 2]:
                    status = _lib.VIDEO_IOU_PIXELS
                    break
                if len(tb[0]) < len(ta[0]):
                    ta, tb = tb, ta
                s, e = ta[0][0:-1:2], ta[0][1::2]              # the set runs [s, e) of the mask with fewer runs
                s = s[:len(e)]
                acc[0] += int((_below(*tb, e) - _below(*tb, s)).sum())
            acc[1] += int(t.rows[md, 3]) if md >= 0 else 0
            acc[2] += int(t.rows[mg, 3]) if mg >= 0 else 0
        out[p] = (0, 0, 0, status) if status else (*acc, 0)
    return out


def pair_sums_device(tables, frame_mask, tracks, pairs):
    """vnx_video_iou_sums on device tensors -> int64 [P, 4] on that device (no synchronisation)."""
    import torch
    lib = _lib.lib()
    dev = tables.rows.device
    P = int(pairs.shape[0])
    out = torch.empty(P, 4, dtype=torch.int64, device=dev)
    if P == 0:
        return out
    with torch.cuda.device(dev):
        _lib.check(lib.vnx_video_iou_sums(tables.ends.data_ptr(), tables.ones.data_ptr(), int(tables.ends.shape[0]),
                                          tables.rows.data_ptr(), int(tables.rows.shape[0]), frame_mask.data_ptr(),
                                          int(frame_mask.shape[0]), tracks.data_ptr(), int(tracks.shape[0]),
                                          pairs.data_ptr(), P, out.data_ptr(), _lib.current_stream(out)))
    return out


def pair_sums(tables, frame_mask, tracks, pairs):
    """tables (RunTables), frame_mask int32 [F] (mask index per (track, frame), -1 = no mask), tracks int32 [T, 2] =
    {first, frames}, pairs int32 [P, 2] = {detection track, ground-truth track} -> numpy int64 [P, 4] = {sum of the
    intersections, of the detection's areas, of the ground truth's areas, status}.  Tables on a CUDA device take the
    kernel, numpy tables `pair_sums_host`."""
    frame_mask, tracks, pairs = _tracks_and_pairs(frame_mask, tracks, pairs)
    if not tables.is_cuda:
        return pair_sums_host(tables, frame_mask, tracks, pairs)
    import torch
    dev = tables.rows.device
    up = lambda a: (torch.from_numpy(a) if a.size else torch.zeros((1,) + a.shape[1:], dtype=torch.int32)).to(dev)  # noqa: E731
    fm, tr, pr = up(frame_mask), up(tracks), up(pairs)
    out = pair_sums_device(RunTables(tables.ends.contiguous(), tables.ones.contiguous(), tables.rows.contiguous()),
                           fm[:len(frame_mask)], tr[:len(tracks)], pr[:len(pairs)])
    return out.cpu().numpy()


def ious_from_sums(sums):
    """int64 [P, 4] -> float64 [P]: I / (A_d + A_g - I), 0.0 where that denominator is 0 (the reference's iou_seq)."""
    i = sums[:, 0].astype(np.float64)
    u = (sums[:, 1] + sums[:, 2] - sums[:, 0]).astype(np.float64)
    return np.divide(i, u, out=np.zeros(len(sums), dtype=np.float64), where=u > 0)
