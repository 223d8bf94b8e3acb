"""The class and box losses of both criteria, fused (vnext_amd/csrc/set_loss.hip): the sigmoid focal loss over all logits
of every decoder layer against the one-hot target the matched pairs imply, the matched boxes' L1 and GIoU losses and the
count of matched queries whose argmax is their label -- two launches forward, one backward.

`set_class_box_losses` returns the per-layer sums `[Ld, 4]` the criteria normalise (`/ num_boxes`, `/ T`; IDOL: `/ denom`,
`* present`).  The one-hot target is never materialised, nothing is gathered, and the forward keeps nothing of the
logits' size for the backward, which recomputes from the inputs and writes every element of both gradients itself (zeros
at unmatched queries): no memset, no scatter.

The call never synchronises and allocates only its output, the per-piece partial sums and (backward) the two gradients,
through torch's allocator: it can be captured in a graph.  No atomics: two calls on the same input are bit-identical.

CUDA tensors only, like the other kernels of this package: there is no CPU implementation behind this call (the CPU form
is the ATen expression in `SetCriterion.forward_all_layers`).
"""
from __future__ import annotations

import torch

from .. import _lib


def _pieces(queries: int, classes: int) -> int:
    """pieces per (layer, clip): include/vnext_hip.h, vnx_set_loss_forward"""
    rows = max(1, min(_lib.SET_LOSS_MAX_ROWS, _lib.SET_LOSS_PIECE // classes))
    return -(-queries // rows)


class _SetLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, boxes, lay, clip, qry, tgt, labels, tgt_boxes, alpha):
        Ld, N, T, Q = (int(v) for v in boxes.shape[:4])
        K = int(logits.shape[3])
        dev = logits.device
        with torch.cuda.device(dev):
            out = torch.empty(Ld, 4, dtype=torch.float32, device=dev)
            partial = torch.empty(Ld, N * _pieces(Q, K), 4, dtype=torch.float32, device=dev)
            _lib.check(_lib.lib().vnx_set_loss_forward(
                logits.data_ptr(), boxes.data_ptr(), lay.data_ptr(), clip.data_ptr(), qry.data_ptr(), tgt.data_ptr(),
                labels.data_ptr(), tgt_boxes.data_ptr(), Ld, N, T, Q, K, int(qry.numel()), int(labels.numel()), alpha,
                partial.data_ptr(), partial.numel() * 4, out.data_ptr(), _lib.current_stream(logits)))
        ctx.save_for_backward(logits, boxes, lay, clip, qry, tgt, labels, tgt_boxes)
        ctx.alpha = alpha
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        logits, boxes, lay, clip, qry, tgt, labels, tgt_boxes = ctx.saved_tensors
        Ld, N, T, Q = (int(v) for v in boxes.shape[:4])
        K = int(logits.shape[3])
        with torch.cuda.device(logits.device):
            grad_out = grad_out.to(torch.float32).contiguous()
            grad_logits = torch.empty_like(logits)
            grad_boxes = torch.empty_like(boxes)
            _lib.check(_lib.lib().vnx_set_loss_backward(
                logits.data_ptr(), boxes.data_ptr(), lay.data_ptr(), clip.data_ptr(), qry.data_ptr(), tgt.data_ptr(),
                labels.data_ptr(), tgt_boxes.data_ptr(), Ld, N, T, Q, K, int(qry.numel()), int(labels.numel()), ctx.alpha,
                grad_out.data_ptr(), grad_logits.data_ptr(), grad_boxes.data_ptr(), _lib.current_stream(logits)))
        return grad_logits, grad_boxes, None, None, None, None, None, None, None


def set_class_box_losses(logits, boxes, lay, clip, qry, tgt, labels, tgt_boxes, alpha=0.25):
    """logits [Ld, N, Q, K] and boxes [Ld, N, T, Q, 4] in cxcywh (fp32; bf16 / fp16 are cast to fp32 and the gradients
    come back in the inputs' types), the pair list lay / clip / qry / tgt int64 [R] on the device (`DeviceMatch`'s layout:
    query `qry[r]` of (layer `lay[r]`, clip `clip[r]`) is matched to target `tgt[r]`, counted over the clips' targets laid
    back to back), labels int64 [n_tot], tgt_boxes [n_tot, T, 4] -> fp32 [Ld, 4], per layer:

      [:, 0]  the sum over (n, q, k) of the sigmoid focal term (gamma 2; `alpha < 0`: no class weighting) against the
              one-hot target that is 1 at (clip, qry, labels[tgt]) of the layer's pairs;
      [:, 1]  the sum over the layer's pairs, frames and coordinates of |pred - want|;
      [:, 2]  the sum over the layer's pairs and frames of `criterion.giou_loss` (1 - GIoU; eps 1e-7 on union and hull);
      [:, 3]  the number of the layer's pairs whose argmax over K equals the label (a tie goes to the lowest index, as
              `torch.argmax`).  Not differentiable.

    Differentiable in `logits` and `boxes`, once.  Away from ties the gradients are ATen's; at an exact tie a maximum /
    minimum splits its gradient evenly between its operands and sign(0) = 0, also as ATen does.

    Preconditions: every (lay, clip, qry) triple appears at most once (Hungarian pairs are one-to-one; `OTAMatcher._one`
    returns each selected query once) -- with a duplicate, which pair the query keeps is not defined.  A pair with a
    negative `qry` or `tgt` (the device Hungarian matcher's answer for a clip whose cost is not finite), or with an index
    outside its array, contributes nothing.

    Never synchronises; allocates its output, the partial sums [Ld, N * pieces, 4] and, in the backward, the two
    gradients.  R == 0 is valid: column 0 and `grad_logits` are computed, the other columns and `grad_boxes` are zero."""
    if not (logits.is_cuda and boxes.is_cuda):
        raise RuntimeError("set_class_box_losses: Not implemented on the CPU (the ATen expression of "
                           "SetCriterion.forward_all_layers is the host form)")
    if logits.dim() != 4 or boxes.dim() != 5 or boxes.shape[-1] != 4 or boxes.shape[:2] != logits.shape[:2] \
            or boxes.shape[3] != logits.shape[2]:
        raise ValueError(f"set_class_box_losses: logits {tuple(logits.shape)} / boxes {tuple(boxes.shape)} are not "
                         "[Ld, N, Q, K] / [Ld, N, T, Q, 4]")
    if min(logits.shape) < 1 or boxes.shape[2] < 1:
        raise ValueError(f"set_class_box_losses: empty logits {tuple(logits.shape)} / boxes {tuple(boxes.shape)}")
    dev = logits.device
    pairs = [lay, clip, qry, tgt]
    if any(p.dim() != 1 or p.numel() != qry.numel() or p.dtype != torch.int64 for p in pairs):
        raise ValueError("set_class_box_losses: lay, clip, qry, tgt must be int64 [R]")
    lay, clip, qry, tgt = (p.to(dev).contiguous() for p in pairs)
    T = int(boxes.shape[2])
    if labels.dtype != torch.int64 or labels.dim() != 1 or tuple(tgt_boxes.shape) != (labels.numel(), T, 4):
        raise ValueError(f"set_class_box_losses: labels {labels.dtype} {tuple(labels.shape)} / tgt_boxes "
                         f"{tuple(tgt_boxes.shape)} are not int64 [n] / [n, {T}, 4]")
    labels = labels.to(dev).contiguous()
    tgt_boxes = tgt_boxes.detach().to(dev, torch.float32).contiguous()
    if logits.dtype != torch.float32:
        logits = logits.to(torch.float32)
    if boxes.dtype != torch.float32:
        boxes = boxes.to(torch.float32)
    return _SetLoss.apply(logits.contiguous(), boxes.contiguous(), lay, clip, qry, tgt, labels, tgt_boxes, float(alpha))
