"""IDOL's simOTA matching and contrastive sets on the device (vnext_amd/csrc/ota_match.hip): one launch for every
(decoder layer, key image) and every reference image of a step, one workgroup per problem.

`idol_match` is the op: device tensors in, one device buffer out.  It neither synchronises nor copies to the host.
`unpack` turns the buffer, once it has been brought to the host, into the structures `OTAMatcher.match_all_layers` and
`select_pos_neg_masks` return (`OTAMatcher.match_all_layers_device` does both).

CUDA tensors only, like the other kernels of this package: there is no CPU implementation behind these calls (the CPU
form is `OTAMatcher.match_all_layers` + `select_pos_neg_masks` of vnext_amd/models/idol_criterion.py).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib


class OtaUnsupported(_lib.VnextHipError):
    """A problem has more targets than the kernel's LDS layout holds, or fewer queries than the matching's top-k asks
    for: match on the host."""


def _check(status: int) -> None:
    if status == _lib.VNX_ERR_UNSUPPORTED:
        raise OtaUnsupported(_lib.lib().vnx_last_error().decode())
    _lib.check(status)


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def max_targets(queries: int) -> int:
    """targets of one problem at most for this many queries (the kernel's LDS layout in the 160 KB of a CU): 105 at 300"""
    return int(_lib.lib().vnx_idol_match_max_targets(int(queries)))


def out_words(max_targets: int, queries: int) -> int:
    """int32 words of one problem's slice of the output buffer"""
    return int(_lib.lib().vnx_idol_match_out_words(int(max_targets), int(queries)))


def idol_match(det_prob, det_boxes, target_boxes, labels, problems, max_targets, ref_prob=None, ref_boxes=None,
               valid=None, valid_first=None):
    """det_prob [Pd, Q, K] class probabilities and det_boxes [Pd, Q, 4] (cxcywh) of the detection problems, ref_prob
    [Pr, Q, K] / ref_boxes [Pr, Q, 4] of the selection problems (or None); target_boxes [n_tot, 4] and labels int64
    [n_tot]: the targets of all images back to back, those of the selection problems from `valid_first` on, with their
    flags in valid uint8 / bool [n_tot - valid_first]; problems int32 [Pd + Pr, 2] = (first target, count) on the
    device; max_targets: the largest count (known on the host; it sizes the kernel's LDS).
    -> int32 [Pd + Pr, out_words(max_targets, Q)] on the device (layout: include/vnext_hip.h, `unpack`).
    Raises OtaUnsupported when a problem does not fit the kernel."""
    if not det_prob.is_cuda:
        raise RuntimeError("idol_match: Not implemented on the CPU (OTAMatcher.match_all_layers and select_pos_neg_masks "
                           "are the host form)")
    if det_prob.dim() != 3 or det_boxes.dim() != 3 or det_boxes.shape != det_prob.shape[:2] + (4,):
        raise ValueError(f"idol_match: det_prob {tuple(det_prob.shape)} / det_boxes {tuple(det_boxes.shape)} are not "
                         "[P, Q, K] / [P, Q, 4]")
    Pd, Q, K = (int(v) for v in det_prob.shape)
    Pr = 0 if ref_prob is None else int(ref_prob.shape[0])
    if Pr and (ref_boxes is None or tuple(ref_prob.shape[1:]) != (Q, K) or tuple(ref_boxes.shape) != (Pr, Q, 4)):
        raise ValueError("idol_match: ref_prob [P, Q, K] and ref_boxes [P, Q, 4] with the detection problems' Q and K expected")
    n_tot = int(labels.shape[0])
    first = n_tot if valid_first is None else int(valid_first)
    if tuple(target_boxes.shape) != (n_tot, 4) or labels.dtype != torch.int64 or problems.dtype != torch.int32 or \
            tuple(problems.shape) != (Pd + Pr, 2) or (n_tot > first and (valid is None or valid.numel() != n_tot - first)):
        raise ValueError("idol_match: target_boxes [n, 4], labels int64 [n], problems int32 [P, 2], valid [n - valid_first] expected")
    dev = det_prob.device
    with torch.cuda.device(dev):
        det_prob, det_boxes, target_boxes = _f32(det_prob), _f32(det_boxes), _f32(target_boxes)
        if Pr:
            ref_prob, ref_boxes = _f32(ref_prob), _f32(ref_boxes)
        if valid is not None:
            valid = valid.contiguous()
            valid = valid.view(torch.uint8) if valid.dtype == torch.bool else valid.to(torch.uint8)
        labels, problems = labels.contiguous(), problems.contiguous()
        stride = out_words(max_targets, Q)
        out = torch.empty(Pd + Pr, stride, dtype=torch.int32, device=dev)
        _check(_lib.lib().vnx_idol_match(
            det_prob.data_ptr(), det_boxes.data_ptr(), ref_prob.data_ptr() if Pr else None,
            ref_boxes.data_ptr() if Pr else None, target_boxes.data_ptr(), labels.data_ptr(),
            valid.data_ptr() if valid is not None and valid.numel() else None, problems.data_ptr(), Pd, Pr, Q, K, n_tot,
            first, int(max_targets), out.data_ptr(), stride, _lib.current_stream(det_prob)))
    return out


def unpack(out, det_problems, queries, max_targets):
    """The buffer of `idol_match` ON THE HOST -> (status int32 [P], detection [(selected [Q] bool, gt idx int64,
    matched int64)], selection [(inst int64 [I], pos [Q, I] bool, neg [Q, I] bool)])"""
    assert not out.is_cuda
    Q, cap = int(queries), int(max_targets)
    a = out.numpy()                                   # a handful of slices per problem: numpy's are cheaper than torch's
    det, sel = [], []
    for p in range(a.shape[0]):
        n = int(a[p, 1])
        if p < det_problems:
            gt = a[p, 2:2 + Q]
            selected = gt >= 0
            det.append((torch.from_numpy(selected), torch.from_numpy(gt[selected].astype("int64")),
                        torch.from_numpy(a[p, 2 + Q:2 + Q + n].astype("int64"))))
        else:
            bits = np.ascontiguousarray(a[p, 2 + cap:].view("uint8")[:n * Q].reshape(n, Q).T)
            sel.append((torch.from_numpy(a[p, 2:2 + n].astype("int64")), torch.from_numpy((bits & 1) != 0),
                        torch.from_numpy((bits & 2) != 0)))
    return out[:, 0], det, sel
