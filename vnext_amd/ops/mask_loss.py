"""The mask losses of both criteria, fused (vnext_amd/csrc/mask_loss.hip): sigmoid focal + dice of the matched instances'
mask logits against the ground truth, one pass each way.

`mask_focal_dice` returns the two per-row vectors the criteria sum (`sigmoid_focal_loss` before its `.sum() / num_boxes`,
`dice_loss` likewise).  The ground truth is read IN PLACE, at image resolution, through the criteria's stride: no sliced,
padded, cast, concatenated or gathered copy, and the forward keeps nothing of the logits' size for the backward, which
recomputes from the logits.  The clips' base pointers and shapes travel in the launch arguments, so nothing is uploaded.

The call never synchronises and allocates only its outputs, the per-piece partial sums and (backward) the gradient,
through torch's allocator: it can be captured in a graph.  No atomics: two calls on the same input are bit-identical.

CUDA tensors only, like the other kernels of this package: there is no CPU implementation behind this call (the CPU form
is the ATen expression in `SetCriterion.forward_all_layers`).
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn.functional as F

from .. import _lib


def _clip_table(gt_list, frames, device):
    """per-clip ground truth -> (MaskLossClips, the tensors it points into).  Clips without targets are left out; more
    clips than the table holds are merged (see `mask_focal_dice`)."""
    clips = []
    for m in gt_list:
        if m.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"mask_focal_dice: ground truth must be bool or uint8, got {m.dtype}")
        if m.dim() == 3:                                   # IDOL: [n, H, W]
            m = m[:, None]
        if m.dim() != 4 or (m.shape[0] and m.shape[1] != frames):
            raise ValueError(f"mask_focal_dice: ground truth {tuple(m.shape)} is not [n, {frames}, H, W]")
        if m.shape[0] == 0:
            continue
        if m.device != device:
            m = m.to(device)
        clips.append(m)
    if len(clips) > _lib.MASK_LOSS_MAX_CLIPS:              # neighbours of one size first: a cat without padding
        merged = [[clips[0]]]
        for m in clips[1:]:
            if m.shape[2:] == merged[-1][0].shape[2:]:
                merged[-1].append(m)
            else:
                merged.append([m])
        clips = [g[0] if len(g) == 1 else torch.cat(g) for g in merged]
    if len(clips) > _lib.MASK_LOSS_MAX_CLIPS:              # still too many: one zero-padded tensor (a missing pixel is target 0)
        H, W = max(m.shape[2] for m in clips), max(m.shape[3] for m in clips)
        clips = [torch.cat([F.pad(m, (0, W - m.shape[3], 0, H - m.shape[2])) for m in clips])]
    clips = [m.contiguous() for m in clips]
    table = _lib.MaskLossClips()
    first = 0
    for i, m in enumerate(clips):
        table.masks[i] = m.data_ptr()
        table.height[i], table.width[i], table.first[i] = int(m.shape[2]), int(m.shape[3]), first
        first += int(m.shape[0])
    table.count, table.total = len(clips), first
    return table, clips


class _MaskFocalDice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, row_gt, table, keep, stride, alpha, gamma):
        R, frames, h, w = (int(v) for v in logits.shape)
        dev = logits.device
        pieces = -(-(frames * h * w) // _lib.MASK_LOSS_PIECE)
        with torch.cuda.device(dev):
            focal = torch.empty(R, dtype=torch.float32, device=dev)
            dice = torch.empty(R, dtype=torch.float32, device=dev)
            sums = torch.empty(R, 3, dtype=torch.float32, device=dev)
            partial = torch.empty(R, pieces, 4, dtype=torch.float32, device=dev)
            _lib.check(_lib.lib().vnx_mask_loss_forward(
                logits.data_ptr(), ctypes.byref(table), row_gt.data_ptr(), R, frames, h, w, stride, alpha, gamma,
                partial.data_ptr(), partial.numel() * 4, focal.data_ptr(), dice.data_ptr(), sums.data_ptr(),
                _lib.current_stream(logits)))
        ctx.save_for_backward(logits, row_gt, sums)
        ctx.table, ctx.keep, ctx.args = table, keep, (stride, alpha, gamma)      # `keep` holds the tensors the table points into
        return focal, dice

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_focal, grad_dice):
        logits, row_gt, sums = ctx.saved_tensors
        R, frames, h, w = (int(v) for v in logits.shape)
        stride, alpha, gamma = ctx.args
        with torch.cuda.device(logits.device):
            grad_focal = grad_focal.to(torch.float32).contiguous()
            grad_dice = grad_dice.to(torch.float32).contiguous()
            grad = torch.empty_like(logits)
            _lib.check(_lib.lib().vnx_mask_loss_backward(
                logits.data_ptr(), ctypes.byref(ctx.table), row_gt.data_ptr(), R, frames, h, w, stride, alpha, gamma,
                sums.data_ptr(), grad_focal.data_ptr(), grad_dice.data_ptr(), grad.data_ptr(),
                _lib.current_stream(logits)))
        return grad, None, None, None, None, None, None


def mask_focal_dice(logits, gt_list, row_gt, stride, alpha=0.25, gamma=2.0):
    """logits [R, F, h, w] (fp32; bf16 / fp16 are cast to fp32), gt_list: per clip (image) a bool / uint8 tensor
    [n_i, F, H_i, W_i] (or [n_i, H_i, W_i] when F = 1) at image resolution -- `t["masks"]` as `prepare_targets` leaves
    it --, row_gt int64 [R] on the device: the row's target, counted over the clips' targets laid back to back
    (`DeviceMatch.tgt`) -> (focal [R], dice [R]) fp32.

    The target of logit (r, f, y, x) is `gt[row_gt[r]][f, y * stride + stride // 2, x * stride + stride // 2]` where
    that pixel exists and 0 where it does not: the criteria's "slice `[s // 2::s]`, then zero-pad to the canvas".
    focal[r] = mean over the row of alpha_t * ce * (1 - p_t) ** gamma; dice[r] = 1 - (2 sum(p t) + 1) / (sum(p) + sum(t)
    + 1).  Differentiable in `logits`, once.  A row whose `row_gt` is outside the targets has target 0 everywhere.

    The ground truth is read in place.  Exceptions, each a copy at image resolution: a clip tensor that is not
    contiguous (or not on the logits' device) is made so, and a batch of more than 16 clips with targets -- what the
    launch arguments hold -- is concatenated: neighbouring clips of one size first, and if that is not enough all of
    them, zero-padded to the largest, into one tensor.  Clips without targets do not count.

    Never synchronises; allocates its outputs, the partial sums [R, ceil(F h w / 4096), 4] and, in the backward, the
    gradient.  R == 0 launches nothing."""
    if not logits.is_cuda:
        raise RuntimeError("mask_focal_dice: Not implemented on the CPU (the ATen expression of "
                           "SetCriterion.forward_all_layers is the host form)")
    if logits.dim() != 4:
        raise ValueError(f"mask_focal_dice: logits {tuple(logits.shape)} are not [R, F, h, w]")
    if row_gt.dtype != torch.int64 or tuple(row_gt.shape) != (logits.shape[0],):
        raise ValueError(f"mask_focal_dice: row_gt must be int64 [{logits.shape[0]}], got {row_gt.dtype} {tuple(row_gt.shape)}")
    stride = int(stride)
    if stride < 1:
        raise ValueError(f"mask_focal_dice: stride {stride}")
    if logits.dtype != torch.float32:
        logits = logits.to(torch.float32)
    logits = logits.contiguous()
    if logits.shape[0] == 0:
        empty = logits.sum((1, 2, 3))                      # [0], in the graph
        return empty, empty
    if row_gt.device != logits.device:
        row_gt = row_gt.to(logits.device)
    table, keep = _clip_table(gt_list, int(logits.shape[1]), logits.device)
    return _MaskFocalDice.apply(logits, row_gt.contiguous(), table, keep, stride, float(alpha), float(gamma))
