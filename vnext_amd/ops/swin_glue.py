"""The element-wise glue of a Swin stage in one HIP pass each way (vnext_amd/csrc/swin_glue.hip).

`residual_norm(x, a, scale, norm) -> (y, n)`:  y = x + scale[b] * a  (the residual add with stochastic depth: `scale` is
the per-sample `mask / keep` of `drop_path`, fp32 [B], or None), n = norm(y) (an nn.LayerNorm, or None).  Swin is pre-norm,
so y stays the residual stream and n feeds the next branch: the in-block site is `(x, attn_out) -> (y, norm2(y))`, the
between-block site `(y, mlp_out) -> (x', norm1_next(x'))`.  `a is None` is the plain LayerNorm that opens a stage (y is x
itself), `norm is None` the plain scaled add that closes it (n is None).
`merge_norm(x, H, W, norm) -> n`: PatchMerging up to its `reduction`: pad to even H and W, the four 2x2 phases side by
side, LayerNorm over 4C -- without the padded copy and the concatenated copy.

On the GPU, for the three type combinations of the kernel (fp32 everywhere; under bf16 autocast an fp32 or a bf16 stream
with a bf16 branch and a bf16 n -- the cast the next Linear would make) and widths that are multiples of 8 from 32 to
3072, each is one launch forward, and one (two with a LayerNorm: its parameter gradients) backward.  Everywhere else (CPU,
fp16 autocast, other types or widths) `fused_applies` says no and the functions ARE the reference expression, evaluated by
torch.  Saved for the backward: y (alive anyway as the next site's input), the row statistics and the scale.  No host
synchronisation and no allocation inside the C calls.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import _lib

MIN_CHANNELS, MAX_CHANNELS = 32, 3072


def _code(dtype):
    return _lib.VNX_BF16 if dtype == torch.bfloat16 else _lib.VNX_F32


def _bf16_autocast(x) -> bool:
    return x.is_cuda and torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16


def _fp16_autocast(x) -> bool:
    return x.is_cuda and torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.float16


def _norm_ok(norm, channels) -> bool:
    return (isinstance(norm, torch.nn.LayerNorm) and tuple(norm.normalized_shape) == (channels,)
            and norm.weight is not None and norm.bias is not None and norm.weight.dtype == torch.float32
            and norm.bias.dtype == torch.float32)


def _width_ok(channels) -> bool:
    return MIN_CHANNELS <= channels <= MAX_CHANNELS and channels % 8 == 0


def norm_dtype(x, a=None):
    """The type the fused op gives n -- a row of the kernel's type table -- or None when (x, a) is in no row.
    fp32 stream, fp32 branch: fp32.  Under bf16 autocast, fp32 or bf16 stream with a bf16 branch: bf16."""
    if x.dtype == torch.float32 and (a is None or a.dtype == torch.float32) and not _bf16_autocast(x):
        return torch.float32
    if _bf16_autocast(x) and x.dtype in (torch.float32, torch.bfloat16) and (a is None or a.dtype == torch.bfloat16):
        return torch.bfloat16
    return None


def fused_applies(x, a, norm) -> bool:
    """CUDA, a width and a type combination the kernel has, no fp16 autocast, an fp32 LayerNorm over the last dimension."""
    if not x.is_cuda or _fp16_autocast(x) or not _width_ok(x.shape[-1]) or norm_dtype(x, a) is None:
        return False
    if a is not None and (a.shape != x.shape or a.device != x.device):
        return False
    return norm is None or _norm_ok(norm, x.shape[-1])


def merge_applies(x, norm) -> bool:
    return (x.is_cuda and not _fp16_autocast(x) and x.shape[-1] % 8 == 0 and _width_ok(4 * x.shape[-1])
            and norm_dtype(x) is not None and _norm_ok(norm, 4 * x.shape[-1]))


class _ResidualNorm(torch.autograd.Function):
    """(x, a or None, scale or None, gamma or None, beta) -> (y or None, n or None)"""

    @staticmethod
    def forward(ctx, x, a, scale, gamma, beta, eps, n_dtype):
        lib = _lib.lib()
        x = x.contiguous()
        C = x.shape[-1]
        rows = x.numel() // C
        rows_per_sample = max(1, rows // max(1, x.shape[0]))
        y = n = stats = None
        if a is not None:
            a = a.contiguous()
            y = torch.empty_like(x)
        if gamma is not None:
            n = torch.empty_like(x, dtype=n_dtype)
            stats = torch.empty(rows, 2, dtype=torch.float32, device=x.device)
        a_dtype = a.dtype if a is not None else n_dtype
        ctx.codes = (_code(x.dtype), _code(a_dtype), _code(n_dtype))
        ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
        with torch.cuda.device(x.device):
            _lib.check(lib.vnx_swin_residual_norm_forward(
                *ctx.codes, x.data_ptr(), ptr(a), ptr(scale), ptr(gamma), ptr(beta), ptr(y), ptr(n), ptr(stats), rows, C,
                rows_per_sample, float(eps), _lib.current_stream(x)))
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(y if y is not None else x, stats, scale, gamma)
        ctx.has_a, ctx.a_dtype, ctx.rows_per_sample = a is not None, a_dtype, rows_per_sample
        return y, n

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y, grad_n):
        lib = _lib.lib()
        y, stats, scale, gamma = ctx.saved_tensors
        C = y.shape[-1]
        rows = y.numel() // C
        if grad_y is not None:
            grad_y = grad_y.to(y.dtype).contiguous()
        if grad_n is not None:
            grad_n = grad_n.contiguous()
        grad_x = torch.empty_like(y)
        grad_a = torch.empty_like(y, dtype=ctx.a_dtype) if ctx.has_a else None
        grad_gamma = grad_beta = partial = None
        nbytes = 0
        if gamma is not None:
            grad_gamma, grad_beta = torch.empty_like(gamma), torch.empty_like(gamma)
            nbytes = lib.vnx_swin_glue_partial_bytes(rows, C)
            partial = torch.empty(nbytes, dtype=torch.uint8, device=y.device)
        ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
        with torch.cuda.device(y.device):
            _lib.check(lib.vnx_swin_residual_norm_backward(
                *ctx.codes, ptr(grad_y), ptr(grad_n), y.data_ptr(), ptr(stats), ptr(gamma), ptr(scale), grad_x.data_ptr(),
                ptr(grad_a), ptr(grad_gamma), ptr(grad_beta), ptr(partial), nbytes, rows, C, ctx.rows_per_sample,
                _lib.current_stream(y)))
        return grad_x, grad_a, None, grad_gamma, grad_beta, None, None


class _MergeNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, n_dtype):
        lib = _lib.lib()
        x = x.contiguous()                                   # [B, H, W, C]
        B, H, W, C = x.shape
        rows = B * ((H + 1) // 2) * ((W + 1) // 2)
        n = torch.empty(B, rows // max(1, B), 4 * C, dtype=n_dtype, device=x.device)
        stats = torch.empty(rows, 2, dtype=torch.float32, device=x.device)
        ctx.codes = (_code(x.dtype), _code(n_dtype))
        with torch.cuda.device(x.device):
            _lib.check(lib.vnx_swin_merge_norm_forward(*ctx.codes, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                                       n.data_ptr(), stats.data_ptr(), B, H, W, C, float(eps),
                                                       _lib.current_stream(x)))
        ctx.save_for_backward(x, stats, gamma)
        return n

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_n):
        lib = _lib.lib()
        x, stats, gamma = ctx.saved_tensors
        B, H, W, C = x.shape
        grad_n = grad_n.contiguous()
        grad_x = torch.empty_like(x)
        grad_gamma, grad_beta = torch.empty_like(gamma), torch.empty_like(gamma)
        nbytes = lib.vnx_swin_glue_partial_bytes(stats.shape[0], 4 * C)
        partial = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.vnx_swin_merge_norm_backward(*ctx.codes, grad_n.data_ptr(), x.data_ptr(), stats.data_ptr(),
                                                        gamma.data_ptr(), grad_x.data_ptr(), grad_gamma.data_ptr(),
                                                        grad_beta.data_ptr(), partial.data_ptr(), nbytes, B, H, W, C,
                                                        _lib.current_stream(x)))
        return grad_x, grad_gamma, grad_beta, None, None


def drop_scale(a, p: float, training: bool):
    """The per-sample scale `mask / keep` of models.swin.drop_path as fp32 [B], or None (eval mode, rate 0).  The mask is
    drawn by the same torch.rand call -- shape (B, 1, .., 1), the branch's dtype and device -- so under one seed the fused
    and the unfused path drop the same samples."""
    if p == 0.0 or not training:
        return None
    keep = 1.0 - p
    mask = (keep + torch.rand((a.shape[0],) + (1,) * (a.dim() - 1), dtype=a.dtype, device=a.device)).floor_()
    return (mask.reshape(-1).to(torch.float64 if a.dtype == torch.float64 else torch.float32) / keep)


def residual_norm_reference(x, a, scale, norm):
    """the reference expression, by torch"""
    y = x
    if a is not None:
        y = x + (a if scale is None else a * scale.to(a.dtype).view((-1,) + (1,) * (a.dim() - 1)))
    return y, (norm(y) if norm is not None else None)


def residual_norm(x, a, scale, norm):
    """-> (y, n): y = x + scale[b] * a (a None: x itself), n = norm(y) (norm None: None).  See the module docstring."""
    if a is None and norm is None:
        return x, None
    if not fused_applies(x, a, norm):
        return residual_norm_reference(x, a, scale, norm)
    if scale is not None:
        scale = scale.to(torch.float32).contiguous()
    gamma, beta, eps = (norm.weight, norm.bias, norm.eps) if norm is not None else (None, None, 0.0)
    y, n = _ResidualNorm.apply(x, a, scale, gamma, beta, eps, norm_dtype(x, a))
    return (x if a is None else y), n


def merge_norm_reference(x, H, W, norm):
    B, L, C = x.shape
    x = x.view(B, H, W, C)
    if H % 2 == 1 or W % 2 == 1:
        x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    x = torch.cat([x[:, 0::2, 0::2, :], x[:, 1::2, 0::2, :], x[:, 0::2, 1::2, :], x[:, 1::2, 1::2, :]], -1)
    return norm(x.view(B, -1, 4 * C))


def merge_norm(x, H, W, norm):
    """x [B, H*W, C] -> norm(cat of the four 2x2 phases of the zero-padded grid) [B, ceil(H/2) * ceil(W/2), 4C]"""
    B, L, C = x.shape
    assert L == H * W, "input feature has wrong size"
    if not merge_applies(x, norm):
        return merge_norm_reference(x, H, W, norm)
    return _MergeNorm.apply(x.reshape(B, H, W, C), norm.weight, norm.bias, norm.eps, norm_dtype(x))
