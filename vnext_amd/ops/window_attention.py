"""The (shifted-)window attention of a Swin Transformer block, fused (vnext_amd/csrc/window_attn.hip).

Reference (projects/SeqFormer/seqformer/backbone/swin.py:129-169 WindowAttention.forward, :233-293 the block's pad / roll /
partition / reverse / crop around it, :404-438 the SW-MSA mask of BasicLayer.forward):

    x = F.pad(norm1(x).view(B, H, W, C), (0, 0, 0, pad_r, 0, pad_b))
    x = torch.roll(x, (-s, -s), (1, 2)) if s > 0 else x
    x = window_partition(x, w).view(-1, w * w, C)
    x = attn(x, mask)               # qkv Linear, scale, q k^T + relative-position bias (+ mask), softmax, attn_drop, @ v, proj
    x = window_reverse(x, w, Hp, Wp); inverse roll; crop to H x W

`window_attention_block` computes the same function as

    qkv = x Wqkv^T                  (library GEMM on the UNPADDED, UNSHIFTED tokens, no bias: the Linear acts token by token)
    o   = all windows, all heads    ONE launch (vnx_window_attention_forward: pad, roll, partition, bias, scale, relative-
                                    position bias, mask, softmax, context, reverse, crop -- as index arithmetic; no mask
                                    tensor, no gathered bias, the scores never stored)
    y   = o Wproj^T + bproj         (library GEMM), proj_drop

and a backward of one attention launch (+ one fixed-order reduction of the table / padded-token partials) and the GEMMs'.
The qkv bias gradient is the column sum of grad_qkv over the real tokens PLUS the k / v gradients of the padded tokens
(whose q / k / v are the bias itself): the kernel returns that second part.

Same module, same parameters (vnext_amd/models/swin.py WindowAttention).  Everywhere the kernel does not apply -- CPU
tensors, VNX_FUSED_WINDOW_ATTN=0 (the A/B switch), head_dim != 32, window > 12, more than 48 heads, and attention dropout
(`attn_drop > 0` while training: the kernel has no dropout; every reference config uses 0.0) -- the block IS the reference
expression, evaluated by torch.  Under torch.autocast the qkv GEMM runs in the autocast dtype and the attention core in fp32
(custom_fwd casts its inputs).

Opt-in, `WindowAttention.bf16_core` (train.enable_bf16_window_attention): when the switch is on, the tensors are on CUDA,
autocast is enabled with dtype bfloat16 and the qkv GEMM's output is bf16, the core is `_WindowAttentionBF16` instead --
the same entry points with dtype VNX_BF16 (vnext_amd/csrc/window_attn_mfma.hip): bf16 qkv in as the GEMM left it, bf16
context out for proj, every product on the matrix cores, scores / softmax / lse / accumulators fp32, no fp32 copy of qkv
anywhere.  In every other case (fp32 input, fp16 autocast, CPU, the cases above) the switch changes nothing.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from .. import _lib

HEAD_DIM = 32
MAX_WINDOW = 12
MAX_HEADS = 48
ENABLE = os.environ.get("VNX_FUSED_WINDOW_ATTN", "1") != "0"     # A/B switch: off = the reference expression, by torch


class _WindowAttention(torch.autograd.Function):
    """qkv [B * H * W, 3 C] (the qkv GEMM without bias, image-row order), qkv_bias [3 C] or None, table [(2w-1)^2, heads]
    -> the attention context [B * H * W, C] (before proj)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, qkv, qkv_bias, table, B, H, W, heads, window, shift, scale):
        lib = _lib.lib()
        qkv = qkv.contiguous()
        table = table.contiguous()
        C = qkv.shape[1] // 3
        out = torch.empty(qkv.shape[0], C, dtype=torch.float32, device=qkv.device)
        lse = torch.empty(qkv.shape[0], heads, dtype=torch.float32, device=qkv.device)
        with torch.cuda.device(qkv.device):
            _lib.check(lib.vnx_window_attention_forward(
                _lib.VNX_F32, qkv.data_ptr(), qkv_bias.data_ptr() if qkv_bias is not None else None, table.data_ptr(),
                out.data_ptr(), lse.data_ptr(), B, H, W, heads, HEAD_DIM, 3 * C, window, shift, float(scale),
                _lib.current_stream(qkv)))
        ctx.save_for_backward(qkv, qkv_bias, table, out, lse)
        ctx.dims = (B, H, W, heads, window, shift, float(scale))
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        lib = _lib.lib()
        qkv, qkv_bias, table, out, lse = ctx.saved_tensors
        B, H, W, heads, window, shift, scale = ctx.dims
        grad_out = grad_out.float().contiguous()
        C = qkv.shape[1] // 3
        g = torch.empty_like(qkv)
        g_table = torch.empty_like(table)
        g_pad = torch.empty(3 * C, dtype=torch.float32, device=qkv.device) if qkv_bias is not None else None
        nbytes = lib.vnx_window_attention_partial_bytes(B, H, W, heads, window)
        partial = torch.empty(max(1, nbytes // 4), dtype=torch.float32, device=qkv.device)
        with torch.cuda.device(qkv.device):
            _lib.check(lib.vnx_window_attention_backward(
                _lib.VNX_F32, qkv.data_ptr(), qkv_bias.data_ptr() if qkv_bias is not None else None, table.data_ptr(),
                out.data_ptr(), lse.data_ptr(), grad_out.data_ptr(), g.data_ptr(), g_table.data_ptr(),
                g_pad.data_ptr() if g_pad is not None else None, partial.data_ptr(), partial.numel() * 4,
                B, H, W, heads, HEAD_DIM, 3 * C, window, shift, scale, _lib.current_stream(qkv)))
        g_bias = g.sum(0) + g_pad if qkv_bias is not None else None
        return g, g_bias, g_table, None, None, None, None, None, None, None


class _WindowAttentionBF16(torch.autograd.Function):
    """The bf16 core: qkv bf16 [B * H * W, 3 C] as the qkv GEMM left it (no bias), qkv_bias / table fp32 -> the context
    bf16 [B * H * W, C].  No cast_inputs: called under bf16 autocast, it keeps the types it is given."""

    @staticmethod
    def forward(ctx, qkv, qkv_bias, table, B, H, W, heads, window, shift, scale):
        lib = _lib.lib()
        qkv = qkv.contiguous()
        table = table.contiguous()
        C = qkv.shape[1] // 3
        out = torch.empty(qkv.shape[0], C, dtype=torch.bfloat16, device=qkv.device)
        lse = torch.empty(qkv.shape[0], heads, dtype=torch.float32, device=qkv.device)
        with torch.cuda.device(qkv.device):
            _lib.check(lib.vnx_window_attention_forward(
                _lib.VNX_BF16, qkv.data_ptr(), qkv_bias.data_ptr() if qkv_bias is not None else None, table.data_ptr(),
                out.data_ptr(), lse.data_ptr(), B, H, W, heads, HEAD_DIM, 3 * C, window, shift, float(scale),
                _lib.current_stream(qkv)))
        ctx.save_for_backward(qkv, qkv_bias, table, out, lse)
        ctx.dims = (B, H, W, heads, window, shift, float(scale))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        lib = _lib.lib()
        qkv, qkv_bias, table, out, lse = ctx.saved_tensors
        B, H, W, heads, window, shift, scale = ctx.dims
        grad_out = grad_out.to(torch.bfloat16).contiguous()
        C = qkv.shape[1] // 3
        g = torch.empty_like(qkv)
        g_table = torch.empty_like(table)
        g_pad = torch.empty(3 * C, dtype=torch.float32, device=qkv.device) if qkv_bias is not None else None
        nbytes = lib.vnx_window_attention_partial_bytes(B, H, W, heads, window)
        partial = torch.empty(max(1, nbytes // 4), dtype=torch.float32, device=qkv.device)
        with torch.cuda.device(qkv.device):
            _lib.check(lib.vnx_window_attention_backward(
                _lib.VNX_BF16, qkv.data_ptr(), qkv_bias.data_ptr() if qkv_bias is not None else None, table.data_ptr(),
                out.data_ptr(), lse.data_ptr(), grad_out.data_ptr(), g.data_ptr(), g_table.data_ptr(),
                g_pad.data_ptr() if g_pad is not None else None, partial.data_ptr(), partial.numel() * 4,
                B, H, W, heads, HEAD_DIM, 3 * C, window, shift, scale, _lib.current_stream(qkv)))
        # the column sum in fp32: a bf16 sum over the tokens would lose the bias gradient
        g_bias = g.sum(0, dtype=torch.float32) + g_pad if qkv_bias is not None else None
        return g, g_bias, g_table, None, None, None, None, None, None, None


def window_partition(x, w):
    """[B, H, W, C] -> [B * nW, w, w, C] (swin.py window_partition)."""
    B, H, W, C = x.shape
    x = x.view(B, H // w, w, W // w, w, C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, w, w, C)


def window_reverse(windows, w, H, W):
    """[B * nW, w, w, C] -> [B, H, W, C] (swin.py window_reverse)."""
    B = int(windows.shape[0] / (H * W / w / w))
    x = windows.view(B, H // w, W // w, w, w, -1)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(B, H, W, -1)


def shift_mask(Hp, Wp, w, s, device, dtype=torch.float32):
    """The SW-MSA mask [nW, w*w, w*w] of BasicLayer.forward: -100.0 between different regions of the shifted grid."""
    img_mask = torch.zeros((1, Hp, Wp, 1), device=device, dtype=dtype)
    cnt = 0
    for hs in (slice(0, -w), slice(-w, -s), slice(-s, None)):
        for ws in (slice(0, -w), slice(-w, -s), slice(-s, None)):
            img_mask[:, hs, ws, :] = cnt
            cnt += 1
    mw = window_partition(img_mask, w).view(-1, w * w)
    mask = mw.unsqueeze(1) - mw.unsqueeze(2)
    return mask.masked_fill(mask != 0, -100.0).masked_fill(mask == 0, 0.0)


def _window_attention_reference(windows, attn, mask):
    """WindowAttention.forward, as the reference writes it: windows [B_, N, C] -> [B_, N, C]."""
    B_, N, C = windows.shape
    heads = attn.num_heads
    qkv = attn.qkv(windows).reshape(B_, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    q = q * attn.scale
    a = q @ k.transpose(-2, -1)
    bias = attn.relative_position_bias_table[attn.relative_position_index.view(-1)].view(N, N, -1)
    a = a + bias.permute(2, 0, 1).contiguous().unsqueeze(0)
    if mask is not None:
        nW = mask.shape[0]
        a = a.view(B_ // nW, nW, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)
        a = a.view(-1, heads, N, N)
    a = attn.attn_drop(a.softmax(dim=-1))
    x = (a @ v).transpose(1, 2).reshape(B_, N, C)
    return attn.proj_drop(attn.proj(x))


def reference_block(x, H, W, attn, window, shift):
    """The block's attention branch by torch: x [B, H*W, C] (after norm1) -> [B, H*W, C] (before drop_path)."""
    B, L, C = x.shape
    x = x.view(B, H, W, C)
    pad_r = (window - W % window) % window
    pad_b = (window - H % window) % window
    x = F.pad(x, (0, 0, 0, pad_r, 0, pad_b))
    _, Hp, Wp, _ = x.shape
    if shift > 0:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
        mask = shift_mask(Hp, Wp, window, shift, x.device, x.dtype)
    else:
        mask = None
    xw = window_partition(x, window).view(-1, window * window, C)
    aw = _window_attention_reference(xw, attn, mask).view(-1, window, window, C)
    x = window_reverse(aw, window, Hp, Wp)
    if shift > 0:
        x = torch.roll(x, shifts=(shift, shift), dims=(1, 2))
    if pad_r > 0 or pad_b > 0:
        x = x[:, :H, :W, :].contiguous()
    return x.view(B, H * W, C)


def fused_applies(x, attn, window) -> bool:
    C = x.shape[-1]
    heads = attn.num_heads
    return (ENABLE and x.is_cuda and x.dim() == 3 and C == heads * HEAD_DIM and 1 <= window <= MAX_WINDOW
            and 1 <= heads <= MAX_HEADS and attn.qkv.weight.dtype == torch.float32
            and attn.relative_position_bias_table.dtype == torch.float32
            and (x.dtype == torch.float32 or torch.is_autocast_enabled())
            and not (attn.attn_drop.p > 0 and attn.training))


def window_attention_block(x, H, W, attn, window, shift):
    """The attention branch of a Swin block: x [B, H*W, C] (after norm1) -> attn's output over the shifted windows, merged
    back, [B, H*W, C] (before drop_path).  `attn` is a WindowAttention (vnext_amd/models/swin.py).  The fused kernel runs
    on CUDA tensors; on CPU, with VNX_FUSED_WINDOW_ATTN=0, attention dropout while training, or shapes outside the kernel's
    (see the module docstring) this is the reference expression by torch."""
    if not fused_applies(x, attn, window):
        return reference_block(x, H, W, attn, window, shift)
    B, L, C = x.shape
    qkv = F.linear(x.reshape(B * L, C), attn.qkv.weight)
    if (getattr(attn, "bf16_core", False) and torch.is_autocast_enabled()
            and torch.get_autocast_dtype("cuda") == torch.bfloat16 and qkv.dtype == torch.bfloat16):
        ctxt = _WindowAttentionBF16.apply(qkv, attn.qkv.bias, attn.relative_position_bias_table, B, H, W,
                                          attn.num_heads, window, shift, attn.scale)
        return attn.proj_drop(attn.proj(ctxt)).view(B, L, C)
    ctxt = _WindowAttention.apply(qkv, attn.qkv.bias, attn.relative_position_bias_table, B, H, W, attn.num_heads, window,
                                  shift, attn.scale)
    return attn.proj_drop(attn.proj(ctxt)).view(B, L, C)
