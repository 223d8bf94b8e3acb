"""IDOL's two re-identification losses, fused (vnext_amd/csrc/reid_loss.hip): the contrastive loss and the auxiliary cosine
loss of every instance of every image of a step -- one launch forward, two backward.

`reid_contrastive_losses` returns the per-instance terms `[J, 2]` that `idol_criterion.reid_terms_fused` sums and the
criterion divides by the instance count.  Nothing is gathered or normalised into a copy: the key rows are named by index,
both embedding tensors are read in place (the two interleaved halves `embeds[0::2]` / `embeds[1::2]` of one tensor
included), and the forward keeps `dot [J, R]`, `|ref_r| [J, R]` and eight floats per instance for the backward, which
writes every element of both gradients itself: no memset, no scatter.

The call never synchronises and allocates only its output, those saved statistics and (backward) the two gradients,
through torch's allocator: it can be captured in a graph.  No atomics: two calls on the same input are bit-identical.

CUDA tensors only, like the other kernels of this package: there is no CPU implementation behind this call (the CPU form
is `vnext_amd.heads.loss_reid`'s expression, per image).
"""
from __future__ import annotations

import torch

from .. import _lib


def supported(key_rows: int, ref_rows: int, channels: int) -> bool:
    """the sizes the kernels take (include/vnext_hip.h, vnx_reid_loss_forward); anything else is VNX_ERR_UNSUPPORTED"""
    return key_rows >= 1 and channels >= 1 and 1 <= ref_rows <= _lib.REID_LOSS_MAX_ROWS


def _rows_in_place(x):
    """[B, rows, C] with contiguous rows and any image stride is read where it is; anything else through a copy"""
    B, rows, C = x.shape
    ok = x.stride(2) == 1 and x.stride(1) == C and (B == 1 or x.stride(0) >= rows * C)
    return x if ok else x.contiguous()


def _geometry(key, ref):
    B, Q, C = (int(v) for v in key.shape)
    return (key.data_ptr(), int(key.stride(0)) if B > 1 else Q * C, Q,
            ref.data_ptr(), int(ref.stride(0)) if B > 1 else int(ref.shape[1]) * C, int(ref.shape[1]), C, B)


class _ReidLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, key, ref, img, key_query, flags):
        J, R = int(img.numel()), int(ref.shape[1])
        dev = key.device
        with torch.cuda.device(dev):
            out = torch.empty(J, 2, dtype=torch.float32, device=dev)
            dot = torch.empty(J, R, dtype=torch.float32, device=dev)
            ref_norm = torch.empty(J, R, dtype=torch.float32, device=dev)
            stats = torch.empty(J, 8, dtype=torch.float32, device=dev)
            _lib.check(_lib.lib().vnx_reid_loss_forward(
                *_geometry(key, ref), img.data_ptr(), key_query.data_ptr(), flags.data_ptr(), J, out.data_ptr(),
                dot.data_ptr(), ref_norm.data_ptr(), stats.data_ptr(), _lib.current_stream(key)))
        ctx.save_for_backward(key, ref, img, key_query, flags, dot, ref_norm, stats)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        key, ref, img, key_query, flags, dot, ref_norm, stats = ctx.saved_tensors
        with torch.cuda.device(key.device):
            grad_out = grad_out.to(torch.float32).contiguous()
            grad_key = torch.empty(key.shape, dtype=torch.float32, device=key.device)
            grad_ref = torch.empty(ref.shape, dtype=torch.float32, device=key.device)
            _lib.check(_lib.lib().vnx_reid_loss_backward(
                *_geometry(key, ref), img.data_ptr(), key_query.data_ptr(), flags.data_ptr(), int(img.numel()),
                dot.data_ptr(), ref_norm.data_ptr(), stats.data_ptr(), grad_out.data_ptr(), grad_key.data_ptr(),
                grad_ref.data_ptr(), _lib.current_stream(key)))
        return grad_key, grad_ref, None, None, None


def reid_contrastive_losses(key_embeds, ref_embeds, img, key_query, flags):
    """key_embeds [B, Q, C] and ref_embeds [B, R, C] (fp32; bf16 / fp16 are cast to fp32 and the gradients come back in
    the inputs' types; views with contiguous rows, such as `embeds[0::2]`, are read in place), the instance list `img`,
    `key_query` int32 [J] on the device (instance j: row `key_query[j]` of key image `img[j]` against every row of
    reference image `img[j]`; `img` non-decreasing) and `flags` uint8 [J, R] (bit 0 positive, bit 1 negative, bit 2 aux
    sample) -> fp32 [J, 2]:

      [:, 0]  softplus(logsumexp over the negatives of dot + logsumexp over the positives of -dot), dot_r = <ref_r, key>;
              exactly 0 when either set is empty;
      [:, 1]  the mean over the aux samples of (cos_r - [r positive])^2, cos with both norms clamped at 1e-12 as
              `F.normalize` does; 0 without aux samples.

    Differentiable in both embedding tensors, once.  An instance whose `img` or `key_query` is out of range reads
    nothing, gives (0, 0) and contributes no gradient.  Two instances may share a key row: their gradients add.

    Sizes: any C >= 1 (16-byte loads where C % 4 == 0), 1 <= R <= 1024, any B, Q, J (`supported`); outside them the
    library returns a status before anything is launched and this call raises.  J == 0 is valid: an empty result, no
    launch, zero gradients.  Never synchronises; allocates its output, dot / |ref_r| [J, R], stats [J, 8] and, in the
    backward, the two gradients."""
    if not (key_embeds.is_cuda and ref_embeds.is_cuda):
        raise RuntimeError("reid_contrastive_losses: Not implemented on the CPU (vnext_amd.heads.loss_reid's expression "
                           "per image is the host form)")
    if key_embeds.dim() != 3 or ref_embeds.dim() != 3 or key_embeds.shape[0] != ref_embeds.shape[0] \
            or key_embeds.shape[2] != ref_embeds.shape[2]:
        raise ValueError(f"reid_contrastive_losses: key {tuple(key_embeds.shape)} / ref {tuple(ref_embeds.shape)} are not "
                         "[B, Q, C] / [B, R, C]")
    dev = key_embeds.device
    J, R = int(img.numel()), int(ref_embeds.shape[1])
    if img.dtype != torch.int32 or key_query.dtype != torch.int32 or img.dim() != 1 or key_query.shape != img.shape:
        raise ValueError("reid_contrastive_losses: img and key_query must be int32 [J]")
    if flags.dtype != torch.uint8 or tuple(flags.shape) != (J, R):
        raise ValueError(f"reid_contrastive_losses: flags {flags.dtype} {tuple(flags.shape)} are not uint8 [{J}, {R}]")
    img, key_query, flags = (v.to(dev).contiguous() for v in (img, key_query, flags))
    if key_embeds.dtype != torch.float32:
        key_embeds = key_embeds.to(torch.float32)
    if ref_embeds.dtype != torch.float32:
        ref_embeds = ref_embeds.to(torch.float32)
    return _ReidLoss.apply(_rows_in_place(key_embeds), _rows_in_place(ref_embeds), img, key_query, flags)
