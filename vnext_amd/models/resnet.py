"""The ResNet trunk both detectors use by default (depth 50; 101 and 152 by `MODEL.RESNETS.DEPTH`): plain PyTorch (the
convolutions run on MIOpen), frozen batch norm folded into the convolutions' filters, optionally channels-last for training
steps, optionally with the element-wise steps after each convolution fused (ops/resnet_glue.py).  `build_backbone(cfg)`
picks between it and the Swin backbone (models/swin.py)."""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F
from torch import nn

from .swin import D2SwinTransformer, is_swin

# TRAINING steps run the ResNet trunk in channels-last memory format on the GPU: MIOpen's fp32 convolutions of these shapes
# are NHWC implicit-GEMM kernels in the backward either way, and given NCHW tensors it transposes in and out around each of
# them (156 + 88 transpose / sub-tensor launches, ~2.2 ms of a 66 ms SeqFormer step on MI355X).  PyTorch only hands MIOpen an
# NHWC problem when PYTORCH_MIOPEN_SUGGEST_NHWC is set.  Measured on one box (bench.py model legs, ms per step, NCHW -> this):
# SeqFormer fp32 two clips 66.2 -> 64.3, one clip 52.4 -> 50.6, bf16 autocast 76.9 -> 74.3, IDOL bf16 pair 67.1 -> 65.8.
# Inference keeps NCHW (forward-only NHWC is slower: SeqFormer 12.0 -> 12.9 ms per clip, IDOL 720p 185 -> 172 frames/s),
# which is why the filters stay NCHW (channels-last filters select NHWC whatever the input is).  A training-only process can
# set VNX_CHANNELS_LAST_WEIGHTS=1 to store the filters channels-last as well (no per-call filter conversion: IDOL pair
# 65.8 -> 60.7 ms, bf16 autocast 74.3 -> 69.7; fp32 SeqFormer unchanged).
# OFF unless the process asks for it: vnext_amd.train.enable_channels_last() sets the MIOpen variable and this switch
# together (importing this module changes nothing process-wide; until round 4 it did both at import time).
# Set after import: read it as this module's attribute at call time, never through `from .resnet import CHANNELS_LAST`.
CHANNELS_LAST = False


class FrozenBatchNorm2d(nn.Module):
    """models/backbone.py:27-64: fixed statistics and affine parameters.  As a standalone module it
    is `x * scale + shift`; inside the trunk below the two constants are folded into the preceding
    convolution instead (`folded()`), which removes two full-resolution elementwise passes per
    convolution from the forward and one from the backward."""

    def __init__(self, n):
        super().__init__()
        self.register_buffer("weight", torch.ones(n))
        self.register_buffer("bias", torch.zeros(n))
        self.register_buffer("running_mean", torch.zeros(n))
        self.register_buffer("running_var", torch.ones(n))
        self._fold = None

    def folded(self):
        """(scale [C], shift [C]), recomputed only when a buffer changed (load_state_dict, .to())."""
        key = tuple((t.data_ptr(), t._version) for t in (self.weight, self.bias, self.running_mean, self.running_var))
        if self._fold is None or self._fold[0] != key:
            with torch.no_grad():
                scale = self.weight * (self.running_var + 1e-5).rsqrt()
                self._fold = (key, scale, self.bias - self.running_mean * scale)
        return self._fold[1], self._fold[2]

    def expanded_scale(self, weight):
        """the scale broadcast to the shape of the preceding convolution's filters (a cached constant: the
        multi-tensor multiply of `fold_all` wants equal shapes)"""
        scale, _ = self.folded()
        cached = getattr(self, "_expanded", None)
        if cached is None or cached[0] is not scale or cached[1].shape != weight.shape or cached[1].device != weight.device:
            fmt = torch.channels_last if weight.dim() == 4 and weight.is_contiguous(memory_format=torch.channels_last) \
                and not weight.is_contiguous() else torch.contiguous_format
            cached = self._expanded = (scale, scale.reshape(-1, 1, 1, 1).expand_as(weight).contiguous(memory_format=fmt))
        return cached[1]

    def forward(self, x):
        scale, shift = self.folded()
        return x * scale.reshape(1, -1, 1, 1) + shift.reshape(1, -1, 1, 1)


def conv_bn(x, conv, bn, folded_weight=None):
    """bn(conv(x)) for a frozen bn: one convolution with scaled filters and the shift as its bias
    (the filters stay trainable: the scaling is a differentiable [Cout,1,1,1] multiply on the weights).
    `folded_weight`: the scaled filters -- or a (filters, shift) pair -- when the caller has folded all convolutions at
    once (`fold_all`)."""
    if isinstance(folded_weight, tuple):
        folded_weight, shift = folded_weight
    else:
        scale, shift = bn.folded()
        if folded_weight is None:
            folded_weight = conv.weight * scale.reshape(-1, 1, 1, 1)
    return F.conv2d(x, folded_weight, shift, conv.stride, conv.padding)


class _FoldScales(torch.autograd.Function):
    """weights[i] * scales[i] for a list of filters in one multi-tensor launch (and one in the backward)
    instead of one small launch per convolution: 53 + 43 launches -> a handful per training step."""

    @staticmethod
    def forward(ctx, scales, out_dtype, *weights):
        ctx.scales = scales
        ctx.set_materialize_grads(False)
        return tuple(_cast_all(torch._foreach_mul(list(weights), scales), out_dtype))

    @staticmethod
    def backward(ctx, *grads):
        live = [i for i, g in enumerate(grads) if g is not None]
        out = [None] * len(grads)
        if live:
            gs = _cast_all([grads[i] for i in live], torch.float32)      # (16-bit under autocast: one multi-tensor cast back)
            for i, g in zip(live, torch._foreach_mul(gs, [ctx.scales[i] for i in live])):
                out[i] = g
        return (None, None, *out)


def _cast_all(tensors, dtype):
    """the list in `dtype` with ONE multi-tensor launch (torch._foreach_copy_ converts), itself when it already is"""
    if dtype is None or not tensors or all(t.dtype == dtype for t in tensors):
        return list(tensors)
    out = [torch.empty_like(t, dtype=dtype) for t in tensors]
    torch._foreach_copy_(out, list(tensors))
    return out


def fold_all(pairs):
    """[(conv, frozen bn)] -> {conv: scaled filters}.  Trainable filters go through `_FoldScales`
    (differentiable), frozen ones through a plain multi-tensor multiply.  Under torch.autocast the filters come out in the
    autocast dtype (round 6): autocast would otherwise cast every convolution's filters at its call -- 53 launches forward and
    53 casts of their gradients backward per step where two multi-tensor launches do."""
    out = {}
    adt = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() and pairs and pairs[0][0].weight.is_cuda else None
    for trainable in (True, False):
        group = [(c, b) for c, b in pairs if c.weight.requires_grad == trainable]
        if not group:
            continue
        scales = [b.expanded_scale(c.weight) for c, b in group]
        weights = [c.weight for c, _ in group]
        if trainable and torch.is_grad_enabled():
            scaled = _FoldScales.apply(scales, adt, *weights)
        else:
            with torch.no_grad():
                scaled = _cast_all(torch._foreach_mul(weights, scales), adt)
        out.update({c: w for (c, _), w in zip(group, scaled)})
    if adt is not None:      # the shifts (the convolutions' biases) too: one multi-tensor cast instead of one per convolution
        convs = [c for c, _ in pairs]
        with torch.no_grad():
            shifts = _cast_all([b.folded()[1] for _, b in pairs], adt)
        out = {c: (out[c], sh) for c, sh in zip(convs, shifts)}
    return out


class _Bottleneck(nn.Module):
    def __init__(self, cin, mid, cout, stride, stride_in_1x1=False):
        super().__init__()
        s1, s3 = (stride, 1) if stride_in_1x1 else (1, stride)      # detectron2 resnet.py:147
        self.conv1 = nn.Conv2d(cin, mid, 1, s1, bias=False); self.bn1 = FrozenBatchNorm2d(mid)
        self.conv2 = nn.Conv2d(mid, mid, 3, s3, 1, bias=False); self.bn2 = FrozenBatchNorm2d(mid)
        self.conv3 = nn.Conv2d(mid, cout, 1, bias=False); self.bn3 = FrozenBatchNorm2d(cout)
        self.down = None
        if stride != 1 or cin != cout:
            self.down = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), FrozenBatchNorm2d(cout))

    def pairs(self):
        out = [(self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3)]
        return out + ([(self.down[0], self.down[1])] if self.down is not None else [])

    def forward(self, x, folded=None, fused=False):
        w = (lambda c: folded[c]) if folded is not None else (lambda c: None)
        if fused and glue_applies(x):
            return self._forward_fused(x, w)
        y = F.relu(conv_bn(x, self.conv1, self.bn1, w(self.conv1)))
        y = F.relu(conv_bn(y, self.conv2, self.bn2, w(self.conv2)))
        y = conv_bn(y, self.conv3, self.bn3, w(self.conv3))
        return F.relu(y + (x if self.down is None else conv_bn(x, self.down[0], self.down[1], w(self.down[0]))))

    def _forward_fused(self, x, w):
        """the same block with the convolutions called without a bias and every element-wise step after them in
        ops/resnet_glue.py: three launches (bias + ReLU twice, the tail once) instead of seven or eight"""
        from ..ops.resnet_glue import conv_epilogue
        y, b = conv_raw(x, self.conv1, self.bn1, w(self.conv1))
        y = conv_epilogue(y, b)
        y, b = conv_raw(y, self.conv2, self.bn2, w(self.conv2))
        y = conv_epilogue(y, b)
        y, b = conv_raw(y, self.conv3, self.bn3, w(self.conv3))
        r, rb = (x, None) if self.down is None else conv_raw(x, self.down[0], self.down[1], w(self.down[0]))
        if y.dtype != torch.float32 and torch.is_grad_enabled():
            # A 16-bit TRAINING step keeps the eager tail.  After conv1 / conv2 the kernel's one rounding of (output + shift)
            # is the eager chain's own, so those sites are bit-identical either way; at the tail the kernel rounds the fp32
            # sum once where the chain rounds two or three times, and that other rounding realisation has not been shown to
            # stay within the project's margin for the bf16 weight gradients.  fp32 is bit-identical
            # everywhere; without grad the fused tail runs in every type.
            y = y + b.reshape(1, -1, 1, 1)
            return F.relu(y + (r if rb is None else r + rb.reshape(1, -1, 1, 1)))
        return conv_epilogue(y, b, r, rb)


def conv_raw(x, conv, bn, folded_weight=None):
    """`conv_bn` without the shift: (the convolution with scaled filters and NO bias, the shift) -- the fused glue adds
    the shift in the pass that also applies the ReLU and the residual"""
    if isinstance(folded_weight, tuple):
        folded_weight, shift = folded_weight
    else:
        scale, shift = bn.folded()
        if folded_weight is None:
            folded_weight = conv.weight * scale.reshape(-1, 1, 1, 1)
    y = F.conv2d(x, folded_weight, None, conv.stride, conv.padding)
    return y, (shift if shift.dtype == y.dtype else shift.to(y.dtype))


def glue_applies(x) -> bool:
    """the fused glue takes CUDA tensors of the kernels' three types that are contiguous or channels-last contiguous;
    everything else runs the eager chain"""
    return (x.is_cuda and x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16, torch.float16)
            and (x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last)))


BLOCKS_PER_STAGE = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}


class ResNetTrunk(nn.Module):
    """res3/res4/res5 features (strides 8/16/32, 512/1024/2048 channels) of a bottleneck ResNet: depth 50, 101 or 152
    (detectron2's `ResNet.make_default_stages`).  `stride_in_1x1` puts a stage's stride on its first block's conv1 (the
    MSRA models) instead of conv2."""
    strides = (8, 16, 32)
    num_channels = (512, 1024, 2048)

    def __init__(self, depth=50, stride_in_1x1=False):
        super().__init__()
        if depth not in BLOCKS_PER_STAGE:
            raise ValueError("MODEL.RESNETS.DEPTH: %r is not a bottleneck ResNet this trunk builds (50, 101, 152)" % (depth,))
        self.depth, self.stride_in_1x1 = depth, bool(stride_in_1x1)
        self.fused_glue = False      # vnext_amd.train.enable_fused_resnet_glue
        self.stem = nn.Sequential(nn.Conv2d(3, 64, 7, 2, 3, bias=False), FrozenBatchNorm2d(64), nn.ReLU(),
                                  nn.MaxPool2d(3, 2, 1))
        def stage(cin, mid, cout, n, stride):
            return nn.Sequential(*[_Bottleneck(cin if i == 0 else cout, mid, cout, stride if i == 0 else 1, stride_in_1x1)
                                   for i in range(n)])
        n2, n3, n4, n5 = BLOCKS_PER_STAGE[depth]
        self.res2 = stage(64, 64, 256, n2, 1)
        self.res3 = stage(256, 128, 512, n3, 2)
        self.res4 = stage(512, 256, 1024, n4, 2)
        self.res5 = stage(1024, 512, 2048, n5, 2)
        if CHANNELS_LAST and os.environ.get("VNX_CHANNELS_LAST_WEIGHTS", "0") == "1":
            self.to(memory_format=torch.channels_last)

    def freeze(self, freeze_at=2):
        """detectron2's MODEL.BACKBONE.FREEZE_AT (default 2, kept by the reference's configs): the
        stem and res2 are not trained, so the backward stops at res3's input."""
        stages = [self.stem, self.res2, self.res3, self.res4, self.res5]
        for stage in stages[:freeze_at]:
            for p in stage.parameters():
                p.requires_grad_(False)
        return self

    def wants_channels_last(self) -> bool:
        """this call of `forward` would convert its input to channels-last: a training step with the switch on.  Whoever
        makes the input (models/frames.py) asks, and writes it channels-last in the first place."""
        return CHANNELS_LAST and self.training and torch.is_grad_enabled()

    def _stem_fused(self, x) -> bool:
        """the fused stem is forward only: taken when nothing upstream of the pool wants a gradient"""
        return not (torch.is_grad_enabled() and (x.requires_grad or self.stem[0].weight.requires_grad))

    def forward(self, x):
        if self.wants_channels_last():
            x = x.contiguous(memory_format=torch.channels_last)
        blocks = [b for stage in (self.res2, self.res3, self.res4, self.res5) for b in stage]
        folded = fold_all([(self.stem[0], self.stem[1])] + [p for b in blocks for p in b.pairs()])
        fused = self.fused_glue and x.is_cuda
        if fused and glue_applies(x) and self._stem_fused(x):
            from ..ops.resnet_glue import stem_pool
            y, b = conv_raw(x, self.stem[0], self.stem[1], folded[self.stem[0]])
            x = stem_pool(y, b)
        else:
            x = F.max_pool2d(F.relu(conv_bn(x, self.stem[0], self.stem[1], folded[self.stem[0]])), 3, 2, 1)
        outs = []
        for stage in (self.res2, self.res3, self.res4, self.res5):
            for b in stage:
                x = b(x, folded, fused)
            outs.append(x)
        return outs[1:]


ResNet50Trunk = ResNetTrunk      # the name the trunk had before its depth was an option: `ResNet50Trunk()` is depth 50


# MODEL.RESNETS keys whose value must be the one this trunk implements
_FIXED_RESNETS = (("NORM", "FrozenBN"), ("RES5_DILATION", 1), ("NUM_GROUPS", 1), ("WIDTH_PER_GROUP", 64),
                  ("RES2_OUT_CHANNELS", 256), ("STEM_OUT_CHANNELS", 64))


def resnet_from_cfg(cfg):
    """the ResNet trunk `MODEL.RESNETS` / `MODEL.BACKBONE.FREEZE_AT` describe (detectron2's `build_resnet_backbone`); a
    value this trunk does not implement raises ValueError naming its key"""
    r = cfg.MODEL.RESNETS
    for key, want in _FIXED_RESNETS:
        got = getattr(r, key, want)
        if got != want:
            raise ValueError("MODEL.RESNETS.%s: %r is not built (this trunk implements %r)" % (key, got, want))
    if any(getattr(r, "DEFORM_ON_PER_STAGE", [False] * 4)):
        raise ValueError("MODEL.RESNETS.DEFORM_ON_PER_STAGE: deformable stages are not built")
    depth = getattr(r, "DEPTH", 50)
    if depth not in BLOCKS_PER_STAGE:
        raise ValueError("MODEL.RESNETS.DEPTH: %r is not built (bottleneck depths 50, 101, 152)" % (depth,))
    out = list(getattr(r, "OUT_FEATURES", ["res3", "res4", "res5"]))
    if not all(f in out for f in ("res3", "res4", "res5")) or any(f not in ("res2", "res3", "res4", "res5") for f in out):
        raise ValueError("MODEL.RESNETS.OUT_FEATURES: %r must contain res3, res4 and res5 (the levels the detectors read)" % (out,))
    freeze_at = getattr(getattr(cfg.MODEL, "BACKBONE", None), "FREEZE_AT", 2)
    return ResNetTrunk(depth, bool(getattr(r, "STRIDE_IN_1X1", False))).freeze(freeze_at)


def build_backbone(cfg):
    """MODEL.BACKBONE.NAME "D2SwinTransformer": the Swin backbone (models/swin.py); otherwise the ResNet trunk that
    MODEL.RESNETS describes -- without that node the ResNet-50 trunk with its stem and res2 frozen."""
    if is_swin(cfg):
        return D2SwinTransformer(cfg)
    if getattr(cfg.MODEL, "RESNETS", None) is None:
        return ResNet50Trunk().freeze(2)
    return resnet_from_cfg(cfg)
