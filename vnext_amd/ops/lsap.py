"""Linear sum assignment on the device (vnext_amd/csrc/lsap.hip): one wave64 per problem, no host round trip.

`seqformer_match` is SeqFormer's Hungarian matching of every (decoder layer, clip) of a step in one launch: the kernel
computes each cost block (`HungarianMatcher.cost`) and solves it.  `lsap_solve` is the solver alone on cost matrices
that already sit in device memory -- `scipy.optimize.linear_sum_assignment`, batched.  Shortest augmenting paths with
fp64 duals on fp32 costs: on the same matrix the assignment is scipy's whenever the optimum is unique.

Neither call synchronises, copies to the host or allocates anything but its outputs.  A problem with a non-finite cost
gets -1 in every output slot (scipy raises there; nothing on the device can): `HungarianMatcher.match_all_layers_device`
does not look, a caller that may see such costs has to.

CUDA tensors only, like the other kernels of this package: there is no CPU implementation behind these calls (the CPU
form of the matching is `HungarianMatcher.match_all_layers`).
"""
from __future__ import annotations

import torch

from .. import _lib


class LsapUnsupported(_lib.VnextHipError):
    """The problem's state does not fit the LDS of a CU (or has more targets than queries): solve it on the host."""


def _check(status: int) -> None:
    if status == _lib.VNX_ERR_UNSUPPORTED:
        raise LsapUnsupported(_lib.lib().vnx_last_error().decode())
    _lib.check(status)


def _f32(t):
    return t.to(torch.float32).contiguous()


def seqformer_match(logits, boxes, labels, tgt_boxes, offsets, weights, return_cost=False, max_targets=None):
    """logits [Ld, N, Q, K], boxes [Ld, N, T, Q, 4] (cxcywh; bf16 / fp16 are cast to fp32 as `HungarianMatcher.cost`
    does), labels int64 [n_tot] and tgt_boxes [n_tot, T, 4] (the clips' targets back to back), offsets int32 [N + 1]
    on the device, weights = (cost_class, cost_bbox, cost_giou) -> (qry, tgt) int64 [Ld, n_tot]: at a clip's offset
    its matched queries ascending and the clip-local target of each.  `max_targets`: the largest clip's target count
    when the host knows it (it sizes the kernel's LDS; default n_tot, which is always enough).  `return_cost`: also the
    cost the kernel solved, [Ld, N, Q, n_tot] fp32, NaN where a column is not one of the clip's own targets.
    Raises LsapUnsupported when a problem does not fit the kernel."""
    if not logits.is_cuda:
        raise RuntimeError("seqformer_match: Not implemented on the CPU (HungarianMatcher.match_all_layers is the host form)")
    if logits.dim() != 4 or boxes.dim() != 5 or boxes.shape[-1] != 4 or boxes.shape[:2] != logits.shape[:2] or \
            boxes.shape[3] != logits.shape[2]:
        raise ValueError(f"seqformer_match: logits {tuple(logits.shape)} / boxes {tuple(boxes.shape)} are not "
                         "[Ld, N, Q, K] / [Ld, N, T, Q, 4]")
    Ld, N, Q, K = (int(v) for v in logits.shape)
    T = int(boxes.shape[2])
    n_tot = int(labels.shape[0])
    if tuple(tgt_boxes.shape) != (n_tot, T, 4) or tuple(offsets.shape) != (N + 1,) or offsets.dtype != torch.int32 or \
            labels.dtype != torch.int64:
        raise ValueError("seqformer_match: labels int64 [n], tgt_boxes [n, T, 4], offsets int32 [N + 1] expected")
    n_max = n_tot if max_targets is None else int(max_targets)
    w_class, w_bbox, w_giou = (float(w) for w in weights)
    dev = logits.device
    with torch.cuda.device(dev):
        logits, boxes, tgt_boxes = _f32(logits.detach()), _f32(boxes.detach()), _f32(tgt_boxes.detach())
        labels, offsets = labels.contiguous(), offsets.contiguous()
        qry = torch.empty(Ld, n_tot, dtype=torch.int64, device=dev)
        tgt = torch.empty(Ld, n_tot, dtype=torch.int64, device=dev)
        cost = torch.full((Ld, N, Q, n_tot), float("nan"), dtype=torch.float32, device=dev) if return_cost else None
        _check(_lib.lib().vnx_seqformer_match(
            logits.data_ptr(), boxes.data_ptr(), labels.data_ptr(), tgt_boxes.data_ptr(), offsets.data_ptr(),
            Ld, N, T, Q, K, n_tot, n_max, w_class, w_bbox, w_giou, qry.data_ptr(), tgt.data_ptr(),
            cost.data_ptr() if return_cost else None, _lib.current_stream(logits)))
    return (qry, tgt, cost) if return_cost else (qry, tgt)


def lsap_solve(cost, maximize=False):
    """cost [rows, cols] or [batch, rows, cols] on the device (any strides; cast to fp32) -> (row_ind, col_ind) int64
    [min(rows, cols)] or [batch, min(rows, cols)]: `scipy.optimize.linear_sum_assignment` of every matrix, rows
    ascending.  Raises LsapUnsupported when a matrix does not fit the LDS of a CU."""
    if not cost.is_cuda:
        raise RuntimeError("lsap_solve: Not implemented on the CPU (scipy.optimize.linear_sum_assignment is the host form)")
    if cost.dim() not in (2, 3):
        raise ValueError(f"lsap_solve: cost must be [rows, cols] or [batch, rows, cols], got {tuple(cost.shape)}")
    single = cost.dim() == 2
    c = cost.detach()
    if c.dtype != torch.float32:
        c = c.to(torch.float32)
    if single:
        c = c[None]
    batch, rows, cols = (int(v) for v in c.shape)
    k = min(rows, cols)
    dev = c.device
    with torch.cuda.device(dev):
        row_ind = torch.empty(batch, k, dtype=torch.int64, device=dev)
        col_ind = torch.empty(batch, k, dtype=torch.int64, device=dev)
        sb, sr, sc = (int(v) for v in c.stride())
        _check(_lib.lib().vnx_lsap_solve(c.data_ptr(), batch, rows, cols, sb, sr, sc, int(bool(maximize)),
                                         row_ind.data_ptr(), col_ind.data_ptr(), _lib.current_stream(c)))
    return (row_ind[0], col_ind[0]) if single else (row_ind, col_ind)
