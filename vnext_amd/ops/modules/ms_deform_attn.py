"""`MSDeformAttn` modules of both projects, on the MI355X op.

Two classes, because the reference has two (same name, different forward):

* `MSDeformAttnIDOL`  <- projects/IDOL/idol/models/ops/modules/ms_deform_attn.py:30-116
  `forward(query, reference_points, input_flatten, spatial_shapes, level_start_index,
  padding_mask) -> (output, sampling_locations, attention_weights)`
* `MSDeformAttnSeqFormer` <- projects/SeqFormer/seqformer/models/ops/modules/ms_deform_attn.py:32-217
  `mode='encode'|'decode'`, clip tensors `[N, T, ...]`, extra `output_proj_box`.

Both offer `encode_forward(query, reference_points, input_flatten, spatial_shapes, level_start_index,
padding_mask) -> output`: what the shared encoder layer (vnext_amd/models/transformer_common.py) calls.

Parameter names, shapes and initialisation are the reference's (checkpoints load
unchanged).  What differs is the mapping onto the machine: the
reference loops over the T frames of a clip in Python and launches the op once per frame
(`:107-120, :153-167, :198-211`); here the frame axis is folded into the op's batch axis, so
a layer is ONE launch whatever T is, and no per-frame `contiguous()` / `cat` copies are made.
The arithmetic that builds `sampling_locations` keeps the reference's expression order so
fp32 results match bit for bit up to the op.
"""
from __future__ import annotations

import math
import warnings

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.init import constant_, xavier_uniform_

from ... import msda_ext
from ..fused_ffn import autocast_once, linear_masked
from ..functions import MSDeformAttnFunction, MSDeformAttnFusedFunction, check_flattened_length


def _is_power_of_2(n):
    if (not isinstance(n, int)) or (n < 0):
        raise ValueError("invalid input for _is_power_of_2: {} (type: {})".format(n, type(n)))
    return (n & (n - 1) == 0) and n != 0


class _MSDeformAttnBase(nn.Module):
    def __init__(self, d_model=256, n_levels=4, n_heads=8, n_points=4):
        super().__init__()
        if d_model % n_heads != 0:
            raise ValueError("d_model must be divisible by n_heads, but got {} and {}".format(d_model, n_heads))
        if not _is_power_of_2(d_model // n_heads):
            warnings.warn("MSDeformAttn: a power-of-two head dimension (32 for the tuned kernels) is faster.")
        self.im2col_step = 64
        self.d_model = d_model
        self.n_levels = n_levels
        self.n_heads = n_heads
        self.n_points = n_points
        self.sampling_offsets = nn.Linear(d_model, n_heads * n_levels * n_points * 2)
        self.attention_weights = nn.Linear(d_model, n_heads * n_levels * n_points)
        self.value_proj = nn.Linear(d_model, d_model)
        self.output_proj = nn.Linear(d_model, d_model)
        # set by a transformer layer that adds the output projections' biases itself, in the pass that follows
        # (`add_dropout_norm(..., r_bias=...)`: the bias gradient then falls out of the LayerNorm backward instead of a
        # reduction launch per projection): the module then returns `output_proj` / `output_proj_box` WITHOUT bias
        self.defer_output_bias = False

    def _project_output(self, x, proj):
        return F.linear(x, proj.weight) if self.defer_output_bias else proj(x)

    def _reset_parameters(self):
        # reference :62-75 (IDOL) / :65-80 (SeqFormer): zero offset weights, bias = the head's unit
        # direction (max-norm normalised) times (k+1); uniform attention; xavier projections
        constant_(self.sampling_offsets.weight.data, 0.)
        thetas = torch.arange(self.n_heads, dtype=torch.float32) * (2.0 * math.pi / self.n_heads)
        grid_init = torch.stack([thetas.cos(), thetas.sin()], -1)
        grid_init = (grid_init / grid_init.abs().max(-1, keepdim=True)[0]).view(
            self.n_heads, 1, 1, 2).repeat(1, self.n_levels, self.n_points, 1)
        for i in range(self.n_points):
            grid_init[:, :, i, :] *= i + 1
        with torch.no_grad():
            self.sampling_offsets.bias = nn.Parameter(grid_init.view(-1))
        constant_(self.attention_weights.weight.data, 0.)
        constant_(self.attention_weights.bias.data, 0.)
        xavier_uniform_(self.value_proj.weight.data)
        constant_(self.value_proj.bias.data, 0.)
        xavier_uniform_(self.output_proj.weight.data)
        constant_(self.output_proj.bias.data, 0.)

    # -- fused prologue -----------------------------------------------------------------------
    # When a caller does not read the sampling_locations / attention_weights the reference module
    # returns (`return_samples = False`; the transformers in vnext_amd/models set it), the softmax and
    # the location arithmetic run inside the sampling kernels (MSDeformAttnFusedFunction) and the two
    # tensors are never materialised; the module then returns None in their place.
    return_samples = True
    fused_prologue = True

    # -- one path from the query to the sampled rows -------------------------------------------
    # Every tensor below may carry the frame axis of a clip behind the batch axis ([N, T, ...]); whatever leads folds into
    # the op's batch axis for the launch and unfolds afterwards.
    def _project_value(self, input_flatten, input_padding_mask, spatial_shapes):
        """input [..., S, C] -> value [..., S, M, D], padded rows zero."""
        check_flattened_length(spatial_shapes, input_flatten.shape[-2])
        # value = self.value_proj(input_flatten); value.masked_fill(input_padding_mask[..., None], 0)  (SeqFormer :94-96):
        # one GEMM + one in-place pass on the GPU (vnext_amd/ops/fused_ffn.py), the expression itself elsewhere
        value = linear_masked(input_flatten, self.value_proj, input_padding_mask)
        return value.view(*value.shape[:-1], self.n_heads, self.d_model // self.n_heads)

    def _offsets_and_logits(self, query):
        """The two Linears, once: raw offsets [..., Lq, M, L, P, 2] and attention logits [..., Lq, M, L*P].  The fused
        kernels read them as they are; the unfused op takes `_weights(logits)` and `_locations(..., offsets, ...)`."""
        lead = query.shape[:-1]
        query = autocast_once(query)      # (feeds two Linears: one cast under autocast instead of two)
        offsets = self.sampling_offsets(query).view(*lead, self.n_heads, self.n_levels, self.n_points, 2)
        logits = self.attention_weights(query).view(*lead, self.n_heads, self.n_levels * self.n_points)
        return offsets, logits

    def _weights(self, logits):
        return F.softmax(logits, -1).view(*logits.shape[:-1], self.n_levels, self.n_points)

    def _locations(self, reference_points, offsets, spatial_shapes):
        """reference_points [..., Lq, L, 2|4] and offsets [..., Lq, M, L, P, 2] broadcast over
        their leading axes (the reference's expressions, IDOL :102-108)."""
        if reference_points.shape[-1] == 2:
            offset_normalizer = torch.stack([spatial_shapes[..., 1], spatial_shapes[..., 0]], -1)
            return reference_points[..., :, None, :, None, :] + offsets / offset_normalizer[None, None, None, :, None, :]
        if reference_points.shape[-1] == 4:
            return reference_points[..., :, None, :, None, :2] \
                + offsets / self.n_points * reference_points[..., :, None, :, None, 2:] * 0.5
        raise ValueError("Last dim of reference_points must be 2 or 4, but get {} instead.".format(
            reference_points.shape[-1]))

    def _sample_fused(self, value, offsets, logits, reference, spatial_shapes, level_start_index, want_samples):
        """value [..., S, M, D], offsets [..., Lq, M, L, P, 2], logits [..., Lq, M, L*P], reference [..., Lq, L, 2|4] (with
        the frame axis, or without it when the frames share the points) -> sampled [..., Lq, C], or None when the caller
        wants the locations / weights back (`want_samples`) or the fused kernels do not take this case."""
        if want_samples or not self.fused_prologue:
            return None
        lead = value.shape[:-3]
        value, offsets, logits = value.flatten(0, -4), offsets.flatten(0, -6), logits.flatten(0, -4)
        reference = reference.flatten(0, -4)
        if reference.dtype != offsets.dtype and not (offsets.dtype == torch.bfloat16 and value.dtype == torch.bfloat16
                                                     and reference.dtype == torch.float32):
            # autocast: the Linears emit 16-bit tensors, the reference points stay fp32 -- rounding positions to 8 mantissa bits
            # would cost more than half a pixel at 720p.  bf16: the kernels read the offsets / logits as they are beside fp32
            # reference points (VNX_MSDA_REF_F32, round 6: until then both were promoted here, two casts forward and two
            # backward per call, 78 MB each on an encoder call); other combinations are promoted.
            offsets, logits, reference = offsets.float(), logits.float(), reference.float()
        reference = reference.contiguous()
        if not msda_ext.fused_supported(value, spatial_shapes, offsets, logits, reference, level_start_index):
            return None
        out = MSDeformAttnFusedFunction.apply(value.contiguous(), spatial_shapes, level_start_index,
                                              offsets.contiguous(), logits.contiguous(), reference)
        return out.view(*lead, *out.shape[1:])

    def _sample(self, value, locations, weights, spatial_shapes, level_start_index):
        """The unfused op: value [..., S, M, D], locations [..., Lq, M, L, P, 2], weights [..., Lq, M, L, P] -> [..., Lq, C]"""
        lead = value.shape[:-3]
        out = MSDeformAttnFunction.apply(value.flatten(0, -4), spatial_shapes, level_start_index,
                                         locations.flatten(0, -6).contiguous(), weights.flatten(0, -5).contiguous(),
                                         self.im2col_step)
        return out.view(*lead, *out.shape[1:])


class MSDeformAttnIDOL(_MSDeformAttnBase):
    """IDOL's module (no frame axis)."""

    def __init__(self, d_model=256, n_levels=4, n_heads=8, n_points=4):
        super().__init__(d_model, n_levels, n_heads, n_points)
        self._reset_parameters()

    def forward(self, query, reference_points, input_flatten, input_spatial_shapes,
                input_level_start_index, input_padding_mask=None):
        value = self._project_value(input_flatten, input_padding_mask, input_spatial_shapes)
        offsets, logits = self._offsets_and_logits(query)
        sampled = self._sample_fused(value, offsets, logits, reference_points, input_spatial_shapes,
                                     input_level_start_index, self.return_samples)
        locations = weights = None
        if sampled is None:
            weights = self._weights(logits)
            locations = self._locations(reference_points, offsets, input_spatial_shapes)
            sampled = self._sample(value, locations, weights, input_spatial_shapes, input_level_start_index)
        return self._project_output(sampled, self.output_proj), locations, weights

    def encode_forward(self, query, reference_points, input_flatten, input_spatial_shapes,
                       input_level_start_index, input_padding_mask=None):
        return self.forward(query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index,
                            input_padding_mask)[0]


class MSDeformAttnSeqFormer(_MSDeformAttnBase):
    """SeqFormer's module: clip tensors [N, T, ...]; T is folded into the op batch."""

    def __init__(self, d_model=256, n_levels=4, n_heads=8, n_points=4, mode='encode'):
        super().__init__(d_model, n_levels, n_heads, n_points)
        self.mode = mode
        # present in the reference whatever the mode, and NOT re-initialised by
        # _reset_parameters (SeqFormer :63,77-80) -- kept so state dicts round-trip
        self.output_proj_box = nn.Linear(d_model, d_model)
        self._reset_parameters()

    def forward(self, query, query_box, reference_points, input_flatten, input_spatial_shapes,
                input_level_start_index, input_padding_mask=None):
        if self.mode == 'encode':
            return self.encode_forward(query, reference_points, input_flatten, input_spatial_shapes,
                                       input_level_start_index, input_padding_mask)
        elif self.mode == 'decode':
            return self.decode_forward(query, query_box, reference_points, input_flatten,
                                       input_spatial_shapes, input_level_start_index, input_padding_mask)

    def encode_forward(self, query, reference_points, input_flatten, input_spatial_shapes,
                       input_level_start_index, input_padding_mask=None):
        value = self._project_value(input_flatten, input_padding_mask, input_spatial_shapes)
        if reference_points.shape[-1] != 2:
            raise ValueError('Last dim of reference_points must be 2 or 4, but get {} instead.'.format(
                reference_points.shape[-1]))
        offsets, logits = self._offsets_and_logits(query)  # [N,nf,Lq,M,L,P,2], [N,nf,Lq,M,L*P]
        # (never returned locations / weights: the fused kernels whatever `return_samples` says)
        sampled = self._sample_fused(value, offsets, logits, reference_points, input_spatial_shapes,
                                     input_level_start_index, want_samples=False)
        if sampled is None:
            weights = self._weights(logits)
            # the encoder's reference points are shared by the frames: [N, Lq, L, 2] (SeqFormer :107-112)
            locations = self._locations(reference_points[:, None], offsets, input_spatial_shapes)
            sampled = self._sample(value, locations, weights, input_spatial_shapes, input_level_start_index)
        return self._project_output(sampled, self.output_proj)

    def decode_forward(self, query, query_box, reference_points, input_flatten, input_spatial_shapes,
                       input_level_start_index, input_padding_mask=None):
        value = self._project_value(input_flatten, input_padding_mask, input_spatial_shapes)
        offsets, logits = self._offsets_and_logits(query_box)
        # first decoder layer, query_box [N, Lq, C]: one set of offsets / weights per query, shared by the frames
        # (SeqFormer :128-171), which the fused kernels do not take; later [N, nf, Lq, C]: per-frame box queries (:172-217).
        # reference_points are per frame either way [N, nf, Lq, L, 2|4]
        shared = query_box.dim() == 3
        assert shared or query_box.dim() == 4
        sampled = None if shared else self._sample_fused(value, offsets, logits, reference_points, input_spatial_shapes,
                                                         input_level_start_index, self.return_samples)
        locations = weights = None
        if sampled is None:
            weights = self._weights(logits)
            locations = self._locations(reference_points, offsets[:, None] if shared else offsets, input_spatial_shapes)
            per_frame = weights[:, None].expand(*value.shape[:2], *weights.shape[1:]) if shared else weights
            sampled = self._sample(value, locations, per_frame, input_spatial_shapes, input_level_start_index)
            locations = locations[:, -1]      # the reference returns the LAST frame's locations (the loop variable, :171,217)
        return (self._project_output(sampled, self.output_proj), self._project_output(sampled, self.output_proj_box),
                locations, weights)
