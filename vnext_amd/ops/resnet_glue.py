"""The element-wise glue of the ResNet trunk in one HIP pass per site (vnext_amd/csrc/resnet_glue.hip).

`conv_epilogue(y, bias, res=None, res_bias=None) -> y`:  y <- relu((y + bias[c]) + (res + res_bias[c])), IN PLACE on the
output of a convolution that ran without its bias (the shift of a folded frozen batch norm).  Without `res` it is the
shift + ReLU after a bottleneck's first two convolutions, with `res` the block's tail: an identity shortcut passes the
block's input, a projection shortcut the raw output of its convolution and that convolution's shift.
`stem_pool(y, bias) -> out`:  max_pool2d(relu(y + bias[c]), 3, 2, 1), the stem after its convolution; forward only.

The layout is the tensor's own: contiguous (NCHW) or channels-last contiguous (NHWC); `res` must have y's layout.  fp32
results equal the eager chain's bit for bit; 16-bit results are the fp32 sum rounded once.  Backward of the epilogue:
grad = y > 0 ? grad_y : 0, ONE tensor handed to the convolution's output and to `res` alike; the shifts are constants of a
frozen norm and get none.  Saved: y alone, alive anyway as the next convolution's input.  CUDA tensors only: these ops have
no other implementation (models/resnet.py keeps the eager chain for everything they do not take).  No host synchronisation
and no allocation inside the C calls.
"""
from __future__ import annotations

import torch

from .. import _lib

_CODES = {torch.float32: _lib.VNX_F32, torch.bfloat16: _lib.VNX_BF16, torch.float16: _lib.VNX_F16}


def layout_of(x):
    """LAYOUT_NCHW for a contiguous [N, C, H, W] tensor, LAYOUT_NHWC for a channels-last contiguous one (a tensor that is
    both -- C or H * W of 1 -- is NCHW), None for anything else"""
    if x.dim() != 4:
        return None
    if x.is_contiguous():
        return _lib.LAYOUT_NCHW
    if x.is_contiguous(memory_format=torch.channels_last):
        return _lib.LAYOUT_NHWC
    return None


def _check(name, y, bias):
    if not y.is_cuda:
        raise RuntimeError(f"{name}: Not implemented on the CPU")
    if y.dtype not in _CODES:
        raise TypeError(f"{name}: float32, bfloat16 or float16 (got {y.dtype})")
    layout = layout_of(y)
    if layout is None:
        raise ValueError(f"{name}: a [N, C, H, W] tensor, contiguous or channels-last contiguous")
    if bias.shape != (y.shape[1],) or bias.dtype != y.dtype or bias.device != y.device or not bias.is_contiguous():
        raise ValueError(f"{name}: the shift is a contiguous [{y.shape[1]}] tensor of y's type and device")
    return layout


def _like(t, y):
    """t in y's memory layout (itself when it already is)"""
    return t if t.stride() == y.stride() else torch.empty_like(y).copy_(t)


class _ConvEpilogue(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, bias, res, res_bias):
        layout = _check("conv_epilogue", y, bias)
        if res is not None:
            if res.shape != y.shape or res.dtype != y.dtype or res.device != y.device:
                raise ValueError("conv_epilogue: res has y's shape, type and device")
            res = _like(res, y)
            if res_bias is not None:
                _check("conv_epilogue", y, res_bias)
        elif res_bias is not None:
            raise ValueError("conv_epilogue: res_bias goes with res")
        N, C, H, W = y.shape
        ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
        with torch.cuda.device(y.device):
            _lib.check(_lib.lib().vnx_conv_epilogue_forward(_CODES[y.dtype], layout, y.data_ptr(), bias.data_ptr(), ptr(res),
                                                            ptr(res_bias), N, C, H * W, _lib.current_stream(y)))
        ctx.mark_dirty(y)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        (y,) = ctx.saved_tensors
        grad_y = _like(grad_y.to(y.dtype), y)
        grad_in = torch.empty_like(y)
        with torch.cuda.device(y.device):
            _lib.check(_lib.lib().vnx_conv_epilogue_backward(_CODES[y.dtype], grad_y.data_ptr(), y.data_ptr(),
                                                             grad_in.data_ptr(), y.numel(), _lib.current_stream(y)))
        return (grad_in if ctx.needs_input_grad[0] else None, None, grad_in if ctx.needs_input_grad[2] else None, None)


def conv_epilogue(y, bias, res=None, res_bias=None):
    """y <- relu((y + bias[c]) + (res + res_bias[c])) in place; -> y.  See the module docstring."""
    return _ConvEpilogue.apply(y, bias, res, res_bias)


def conv_epilogue_reference(y, bias, res=None, res_bias=None):
    """the eager chain, by torch (out of place)"""
    v = y + bias.reshape(1, -1, 1, 1)
    if res is not None:
        v = v + (res if res_bias is None else res + res_bias.reshape(1, -1, 1, 1))
    return torch.relu(v)


def stem_pool(y, bias):
    """max_pool2d(relu(y + bias[c]), 3, 2, 1) in one pass, in y's layout.  The kernel is forward only: a y that wants a
    gradient takes the eager chain."""
    if torch.is_grad_enabled() and y.requires_grad:      # an unfrozen stem: the eager chain, which has a backward
        return stem_pool_reference(y, bias)
    layout = _check("stem_pool", y, bias)
    N, C, H, W = y.shape
    fmt = torch.channels_last if layout == _lib.LAYOUT_NHWC else torch.contiguous_format
    out = torch.empty((N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=y.dtype, device=y.device, memory_format=fmt)
    with torch.cuda.device(y.device):
        _lib.check(_lib.lib().vnx_stem_pool_forward(_CODES[y.dtype], layout, y.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                                    N, C, H, W, _lib.current_stream(y)))
    return out


def stem_pool_reference(y, bias):
    import torch.nn.functional as F
    return F.max_pool2d(F.relu(y + bias.reshape(1, -1, 1, 1)), 3, 2, 1)
