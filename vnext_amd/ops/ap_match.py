"""The greedy matching of the AP evaluators (vnext_amd/csrc/ap_match.hip): COCOeval.evaluateImg / YTVOSeval.evaluateVid
for every (image, category) problem of an evaluation, all area ranges and all IoU thresholds at once.

A problem is a row {D, G, detection offset, ground-truth offset, IoU offset} of an int64 table into flat arrays: the
detections' areas, the ground truths' crowd flags and areas, and the problems' row-major [D, G] IoU matrices (float64),
detections already in score order and cut to the last `max_dets`.  The results are problem-local indices, -1 for none:

    dt_match  int32 [A, T, sum D]   the ground truth a detection took
    dt_ignore uint8 [A, T, sum D]   that ground truth's ignore flag; without a match: the detection's area is outside
    gt_match  int32 [A, T, sum G]   the last detection that took a ground truth
    gt_ignore uint8 [A, sum G]      crowd, or area outside the range

The caller maps indices to ids, which keeps the reference's `dtm == 0` behaviour for an id of 0 where it belongs.

`match_host` is the readable statement of the decisions (plain Python, the reference's loop on indices);
`match_vectorised` makes the same decisions in numpy, one step per (detection rank, ground-truth rank) over all
problems, area ranges and thresholds; `ap_match` is the kernel, for CUDA tensors.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .. import _lib

MAX_GT, MAX_LANES = _lib.AP_MATCH_MAX_GT, _lib.AP_MATCH_MAX_LANES


@dataclass
class Matches:
    dt_match: object
    dt_ignore: object
    gt_match: object
    gt_ignore: object
    host_fallback: bool = False        # ap_match only: a problem beyond the kernel's limits sent the call to match_host

    def numpy(self):
        if isinstance(self.dt_match, np.ndarray):
            return self
        return Matches(*(a.cpu().numpy() for a in (self.dt_match, self.dt_ignore, self.gt_match, self.gt_ignore)),
                       host_fallback=self.host_fallback)


def _host_inputs(table, ious, gt_crowd, gt_area, dt_area, area_rng, thrs):
    table = np.ascontiguousarray(np.asarray(table, dtype=np.int64).reshape(-1, 5))
    f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))       # noqa: E731
    ious, gt_area, dt_area, thrs = f(ious), f(gt_area), f(dt_area), f(thrs)
    gt_crowd = np.ascontiguousarray(np.asarray(gt_crowd).reshape(-1) != 0).astype(np.uint8)
    area_rng = np.ascontiguousarray(np.asarray(area_rng, dtype=np.float64).reshape(-1, 2))
    if len(gt_crowd) != len(gt_area):
        raise ValueError(f"ap_match: {len(gt_crowd)} crowd flags, {len(gt_area)} ground-truth areas")
    D, G, dof, gof, iof = table.T if len(table) else np.zeros((5, 0), np.int64)
    if (table < 0).any() or (dof + D > len(dt_area)).any() or (gof + G > len(gt_area)).any() or \
            (iof + D * G > len(ious)).any():
        raise ValueError("ap_match: a row of the problem table points outside its arrays")
    return table, ious, gt_crowd, gt_area, dt_area, area_rng, thrs


def _empty(A, T, n_dt, n_gt):
    return Matches(np.full((A, T, n_dt), -1, np.int32), np.zeros((A, T, n_dt), np.uint8),
                   np.full((A, T, n_gt), -1, np.int32), np.zeros((A, n_gt), np.uint8))


def match_host(table, ious, gt_crowd, gt_area, dt_area, area_rng, thrs):
    """The reference's evaluateImg on indices, in plain Python: numpy inputs -> Matches of numpy arrays."""
    table, ious, gt_crowd, gt_area, dt_area, area_rng, thrs = _host_inputs(table, ious, gt_crowd, gt_area, dt_area,
                                                                           area_rng, thrs)
    A, T = len(area_rng), len(thrs)
    out = _empty(A, T, len(dt_area), len(gt_area))
    rows = ious.tolist()
    for D, G, dof, gof, iof in table.tolist():
        crowd = gt_crowd[gof:gof + G].tolist()
        for a, (lo, hi) in enumerate(area_rng.tolist()):
            ig = [1 if (crowd[g] or gt_area[gof + g] < lo or gt_area[gof + g] > hi) else 0 for g in range(G)]
            out.gt_ignore[a, gof:gof + G] = ig
            order = [g for g in range(G) if not ig[g]] + [g for g in range(G) if ig[g]]   # ignored last, stable
            for t, thr in enumerate(thrs.tolist()):
                taken = [False] * G
                for d in range(D):
                    iou = min([thr, 1 - 1e-10])
                    m = -1
                    for g in order:
                        if taken[g] and not crowd[g]:                  # matched already, and not a crowd
                            continue
                        if m > -1 and ig[m] == 0 and ig[g] == 1:       # holds a regular match, now on ignored ones
                            break
                        v = rows[iof + d * G + g]
                        if v < iou:
                            continue
                        iou = v
                        m = g
                    if m == -1:                                        # unmatched: ignored when its area is outside
                        out.dt_ignore[a, t, dof + d] = dt_area[dof + d] < lo or dt_area[dof + d] > hi
                        continue
                    taken[m] = True
                    out.dt_match[a, t, dof + d] = m
                    out.dt_ignore[a, t, dof + d] = ig[m]
                    out.gt_match[a, t, gof + m] = d
    return out


def match_vectorised(table, ious, gt_crowd, gt_area, dt_area, area_rng, thrs):
    """`match_host`'s decisions in numpy: the loops run over the detection rank and the ground-truth rank (twice: the
    ground truths a lane does not ignore, then the ignored ones for lanes without a match), each step over every
    problem that is that deep, every area range and every threshold."""
    table, ious, gt_crowd, gt_area, dt_area, area_rng, thrs = _host_inputs(table, ious, gt_crowd, gt_area, dt_area,
                                                                           area_rng, thrs)
    A, T = len(area_rng), len(thrs)
    out = _empty(A, T, len(dt_area), len(gt_area))
    lo, hi = area_rng[:, 0:1], area_rng[:, 1:2]
    gt_ig = gt_crowd.astype(bool)[None, :] | (gt_area[None, :] < lo) | (gt_area[None, :] > hi)          # [A, sum G]
    dt_out = (dt_area[None, :] < lo) | (dt_area[None, :] > hi)                                         # [A, sum D]
    D, G, dof, gof, iof = table.T if len(table) else np.zeros((5, 0), np.int64)
    own = np.zeros(len(gt_area), bool)                      # ground truths some problem owns
    if len(table):
        own[np.repeat(gof, G) + (np.arange(int(G.sum())) - np.repeat(np.cumsum(G) - G, G))] = True
    out.gt_ignore[:] = gt_ig & own[None, :]
    taken = np.zeros((A, T, len(gt_area)), bool)
    crowd = gt_crowd.astype(bool)
    thr = np.minimum(thrs, 1 - 1e-10)
    dt_match, gt_match = out.dt_match, out.gt_match
    for d in range(int(D.max()) if len(table) else 0):
        P = np.flatnonzero(D > d)                           # problems with a detection of this rank
        best = np.broadcast_to(thr[None, None, :], (len(P), A, T)).copy()
        m = np.full((len(P), A, T), -1, np.int64)
        for second in (False, True):
            for g in range(int(G[P].max())):
                sub = np.flatnonzero(G[P] > g)              # rows of P with a ground truth of this rank
                if not len(sub):
                    break
                q = P[sub]
                gi = gof[q] + g
                v = ious[iof[q] + d * G[q] + g][:, None, None]
                ig = gt_ig[:, gi].T[:, :, None]                              # [n, A, 1]
                tk = taken[:, :, gi].transpose(2, 0, 1)                      # [n, A, T]
                if second:                                  # a taken crowd stays free
                    ok = ig & second_open[sub] & ~(tk & ~crowd[gi][:, None, None])
                else:                                       # not ignored, so not a crowd
                    ok = ~ig & ~tk
                ok = ok & ~(v < best[sub])
                best[sub] = np.where(ok, v, best[sub])
                m[sub] = np.where(ok, g, m[sub])
            if not second:
                second_open = m == -1                       # the reference's break: no ignored ones after a regular match
        n, a_i, t_i = np.nonzero(m >= 0)
        gi = gof[P[n]] + m[n, a_i, t_i]
        taken[a_i, t_i, gi] = True
        gt_match[a_i, t_i, gi] = d
        di = dof[P] + d
        dt_match[:, :, di] = m.transpose(1, 2, 0)
        matched_ig = gt_ig[a_i, gi]
        ign = np.broadcast_to(dt_out[:, di].T[:, :, None], m.shape).copy()
        ign[n, a_i, t_i] = matched_ig
        out.dt_ignore[:, :, di] = ign.transpose(1, 2, 0)
    return out


def ap_match(table, ious, gt_crowd, gt_area, dt_area, area_rng, thrs, max_gt=None):
    """The kernel.  CUDA tensors: table int64 [P, 5], ious float64 [sum D * G], gt_crowd uint8 [sum G], gt_area float64
    [sum G], dt_area float64 [sum D], area_rng float64 [A, 2], thrs float64 [T] -> Matches of tensors on that device.
    CPU tensors raise.  A problem with more than MAX_GT ground truths, or A * T above MAX_LANES, takes `match_host`
    for the whole call (`host_fallback`); `max_gt` is the largest G when the caller knows it (it saves the read)."""
    import torch
    tensors = (table, ious, gt_crowd, gt_area, dt_area, area_rng, thrs)
    for x in tensors:
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("ap_match: Not implemented on the CPU (CUDA tensors only; the host form is match_host)")
    dev = table.device
    want = (torch.int64, torch.float64, torch.uint8, torch.float64, torch.float64, torch.float64, torch.float64)
    names = ("table", "ious", "gt_crowd", "gt_area", "dt_area", "area_rng", "thrs")
    for x, dt, name in zip(tensors, want, names):
        if x.dtype != dt or x.device != dev or not x.is_contiguous():
            raise ValueError(f"ap_match: {name} must be a contiguous {dt} tensor on {dev}")
    if table.dim() != 2 or table.shape[1] != 5 or area_rng.dim() != 2 or area_rng.shape[1] != 2:
        raise ValueError("ap_match: table is [P, 5], area_rng [A, 2]")
    if gt_crowd.numel() != gt_area.numel():
        raise ValueError(f"ap_match: {gt_crowd.numel()} crowd flags, {gt_area.numel()} ground-truth areas")
    P, A, T = int(table.shape[0]), int(area_rng.shape[0]), int(thrs.numel())
    n_dt, n_gt = int(dt_area.numel()), int(gt_area.numel())
    if max_gt is None:
        max_gt = int(table[:, 1].max()) if P else 0
    if max_gt > MAX_GT or A * T > MAX_LANES:
        host = match_host(*(x.cpu().numpy() for x in tensors))
        up = lambda a: torch.from_numpy(a).to(dev)                       # noqa: E731
        return Matches(up(host.dt_match), up(host.dt_ignore), up(host.gt_match), up(host.gt_ignore), host_fallback=True)
    out = Matches(torch.full((A, T, n_dt), -1, dtype=torch.int32, device=dev),
                  torch.zeros((A, T, n_dt), dtype=torch.uint8, device=dev),
                  torch.full((A, T, n_gt), -1, dtype=torch.int32, device=dev),
                  torch.zeros((A, n_gt), dtype=torch.uint8, device=dev))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    match_into(table, ious, gt_crowd, gt_area, dt_area, area_rng, thrs, out, status)
    st = int(status)
    if st:
        raise ValueError("ap_match: a row of the problem table points outside its arrays" if st == _lib.AP_MATCH_BAD_TABLE
                         else f"ap_match: a problem has more than {MAX_GT} ground truths")
    return out


def match_into(table, ious, gt_crowd, gt_area, dt_area, area_rng, thrs, out, status):
    """One launch of vnx_ap_match into preallocated outputs (`out`: Matches of tensors, `status` int32 [1], zeroed by
    the caller); no checks beyond the library's, no synchronisation."""
    import torch
    with torch.cuda.device(table.device):
        _lib.check(_lib.lib().vnx_ap_match(
            table.data_ptr(), int(table.shape[0]), ious.data_ptr(), int(ious.numel()), gt_crowd.data_ptr(),
            gt_area.data_ptr(), int(gt_area.numel()), dt_area.data_ptr(), int(dt_area.numel()), area_rng.data_ptr(),
            int(area_rng.shape[0]), thrs.data_ptr(), int(thrs.numel()), out.dt_match.data_ptr(), out.dt_ignore.data_ptr(),
            out.gt_match.data_ptr(), out.gt_ignore.data_ptr(), status.data_ptr(), _lib.current_stream(table)))
