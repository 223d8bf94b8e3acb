"""What the two deformable transformers (seqformer_transformer.py, idol_transformer.py) share: the encoder layer and the encoder,
the base of the two `DeformableTransformer`s (level embedding, initial reference points, initialisation, the encoder pass),
the flattened multi-level buffers the encoder reads and the reference points a decoder layer samples around.  Each file
keeps its decoder layer, its decoder and the tail of its `forward`.  Behaviour as the reference's
(projects/SeqFormer/seqformer/models/deformable_transformer.py:78-129, 336-385;
projects/IDOL/idol/models/deformable_transformer.py:135-198, 325-375), expressed once and without the per-level lists + `cat`
and the per-layer recomputation of constants."""
from __future__ import annotations

import copy

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.init import constant_, normal_, xavier_uniform_

from ..ops import shadow_weights
from ..ops.decoder_glue import inverse_sigmoid, refined_boxes  # noqa: F401  (re-exported: the models import them from here)
from ..ops.functions import level_tensors
from ..ops.fused_ffn import ffn_block
from ..ops.fused_norm import add_dropout_norm
from ..ops.modules.ms_deform_attn import _MSDeformAttnBase


def flatten_levels(srcs, masks, pos_embeds, level_embed):
    """Per level [..., C, H_l, W_l] features and position embeddings and [..., H_l, W_l] padding masks -> ONE buffer each:
    features [..., S, C], position + level embedding [..., S, C], mask [..., S], the levels back to back in level order (the
    packed layout the op's grad_value kernels rely on), plus the op's (spatial_shapes, level_start_index) pair and the list
    of level sizes.  Every level is written straight into its slice: no list of transposed views, no `cat`."""
    lead, channels = srcs[0].shape[:-3], srcs[0].shape[-3]
    sizes = [tuple(int(v) for v in s.shape[-2:]) for s in srcs]
    total = sum(h * w for h, w in sizes)
    feats = srcs[0].new_empty(*lead, total, channels)
    # (the sum's own dtype: under bf16 autocast the position embeddings may arrive in bf16 while the level embedding is an fp32
    #  parameter -- the promoted sum must not be rounded back into a bf16 buffer; the `cat`-based form kept it: ADVICE r5)
    pos = pos_embeds[0].new_empty(*lead, total, channels, dtype=torch.result_type(pos_embeds[0], level_embed))
    pad = masks[0].new_empty(*lead, total)
    at = 0
    for lvl, (h, w) in enumerate(sizes):
        rows = slice(at, at + h * w)
        feats[..., rows, :] = srcs[lvl].flatten(-2).transpose(-1, -2)
        pos[..., rows, :] = pos_embeds[lvl].flatten(-2).transpose(-1, -2) + level_embed[lvl]
        pad[..., rows] = masks[lvl].flatten(-2)
        at += h * w
    shapes_t, start_t = level_tensors(sizes, feats.device)      # cached device tensors, tagged packed, host-side sizes attached
    return feats, pad, pos, shapes_t, start_t, sizes


class ReferenceScaler:
    """reference points -> what a decoder layer samples around: points (2 components) or boxes (4) times the valid ratios of
    every level.  The two ratio tensors are constants of a forward pass: built once here, not once per layer."""

    def __init__(self, valid_ratios, extra_axes):
        # valid_ratios [N, L, 2]; reference points [N, (T,) Q, 2|4]: `extra_axes` singleton axes sit between N and L
        index = (slice(None),) + (None,) * extra_axes
        self.xy = valid_ratios[index]
        self.xywh = torch.cat([valid_ratios, valid_ratios], -1)[index]

    def __call__(self, reference_points):
        scale = self.xywh if reference_points.shape[-1] == 4 else self.xy
        return reference_points.unsqueeze(-2) * scale


def _get_clones(module, n):
    return nn.ModuleList([copy.deepcopy(module) for _ in range(n)])


def _get_activation_fn(activation):
    if activation == "relu":
        return F.relu
    if activation == "gelu":
        return F.gelu
    if activation == "glu":
        return F.glu
    raise RuntimeError(f"activation should be relu/gelu, not {activation}.")


class DeformableTransformerEncoderLayer(nn.Module):
    """Both stacks' encoder layer.  `attention(d_model, n_levels, n_heads, n_points)` builds the stack's MSDeformAttn module;
    the layer reaches it through `encode_forward`, which both classes spell alike (ops/modules/ms_deform_attn.py)."""

    def __init__(self, attention, d_model=256, d_ffn=1024, dropout=0.1, activation="relu", n_levels=4, n_heads=8,
                 n_points=4):
        super().__init__()
        self.self_attn = attention(d_model, n_levels, n_heads, n_points)
        self.self_attn.defer_output_bias = True      # added in norm1's pass (forward below)
        self.dropout1 = nn.Dropout(dropout)
        self.norm1 = nn.LayerNorm(d_model)
        self.linear1 = nn.Linear(d_model, d_ffn)
        self.activation = _get_activation_fn(activation)
        self.dropout2 = nn.Dropout(dropout)
        self.linear2 = nn.Linear(d_ffn, d_model)
        self.dropout3 = nn.Dropout(dropout)
        self.norm2 = nn.LayerNorm(d_model)
        shadow_weights.install(self)     # under autocast: this layer's GEMM weights cast once, together

    def forward(self, src, pos, reference_points, spatial_shapes, level_start_index, padding_mask=None):
        src2 = self.self_attn.encode_forward(src if pos is None else src + pos, reference_points, src, spatial_shapes,
                                             level_start_index, padding_mask)
        src = add_dropout_norm(src, src2, self.dropout1, self.norm1, r_bias=self.self_attn.output_proj.bias)
        # norm2(src + dropout3(linear2(dropout2(activation(linear1(src)))))) -- vnext_amd/ops/fused_ffn.py
        return ffn_block(src, self.linear1, self.activation, self.dropout2, self.linear2, self.dropout3, self.norm2)


class DeformableTransformerEncoder(nn.Module):
    def __init__(self, encoder_layer, num_layers):
        super().__init__()
        self.layers = _get_clones(encoder_layer, num_layers)
        self.num_layers = num_layers

    @staticmethod
    def get_reference_points(spatial_shapes, valid_ratios, device):
        # pixel centres / (valid ratio * size), then * valid ratio  (SeqFormer :183-196, IDOL :249-261)
        refs = []
        for lvl, (H_, W_) in enumerate(spatial_shapes):
            H_, W_ = int(H_), int(W_)
            ref_y, ref_x = torch.meshgrid(
                torch.linspace(0.5, H_ - 0.5, H_, dtype=torch.float32, device=device),
                torch.linspace(0.5, W_ - 0.5, W_, dtype=torch.float32, device=device), indexing="ij")
            ref_y = ref_y.reshape(-1)[None] / (valid_ratios[:, None, lvl, 1] * H_)
            ref_x = ref_x.reshape(-1)[None] / (valid_ratios[:, None, lvl, 0] * W_)
            refs.append(torch.stack((ref_x, ref_y), -1))
        reference_points = torch.cat(refs, 1)
        return reference_points[:, :, None] * valid_ratios[:, None]

    def forward(self, src, spatial_shapes, level_start_index, valid_ratios, pos=None, padding_mask=None,
                spatial_shapes_list=None):
        shapes_iter = spatial_shapes_list if spatial_shapes_list is not None else spatial_shapes.tolist()
        reference_points = self.get_reference_points(shapes_iter, valid_ratios, device=src.device)
        output = src
        for layer in self.layers:
            output = layer(output, pos, reference_points, spatial_shapes, level_start_index, padding_mask)
        return output


class DeformableTransformerBase(nn.Module):
    """What a `DeformableTransformer` owns around its two stacks: the level embedding, the Linear behind the initial
    reference points, the reference's initialisation, and the encoder pass.  A subclass builds its stacks (encoder first:
    the order of the seeded draws), hands them over and writes `forward` from `encode` on."""

    def __init__(self, encoder, decoder, d_model, nhead, num_feature_levels, decoder_returns_samples=False):
        super().__init__()
        self.d_model, self.nhead, self.num_feature_levels = d_model, nhead, num_feature_levels
        self.encoder = encoder
        self.decoder = decoder
        self.level_embed = nn.Parameter(torch.Tensor(num_feature_levels, d_model))
        self.reference_points = nn.Linear(d_model, 2)
        self._reset_parameters()
        # an encoder never reads the modules' locations / weights, nor does a decoder unless it keeps samples (IDOL's
        # `return_samples=True`): fused prologue
        for m in (self.encoder if decoder_returns_samples else self).modules():
            if isinstance(m, _MSDeformAttnBase):
                m.return_samples = False

    def _reset_parameters(self):
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        for m in self.modules():
            if isinstance(m, _MSDeformAttnBase):
                m._reset_parameters()
        xavier_uniform_(self.reference_points.weight.data, gain=1.0)
        constant_(self.reference_points.bias.data, 0.)
        normal_(self.level_embed)

    @staticmethod
    def get_valid_ratio(mask):
        _, H, W = mask.shape
        valid_H = torch.sum(~mask[:, :, 0], 1)
        valid_W = torch.sum(~mask[:, 0, :], 1)
        return torch.stack([valid_W.float() / W, valid_H.float() / H], -1)

    def encode(self, srcs, masks, pos_embeds, valid_ratios):
        """Per-level features, padding masks and position embeddings -> (memory [..., S, C], padding [..., S], and the op's
        (spatial_shapes, level_start_index) pair): `flatten_levels`, then the encoder."""
        memory_in, padding, pos, shapes_t, start_t, sizes = flatten_levels(srcs, masks, pos_embeds, self.level_embed)
        memory = self.encoder(memory_in, shapes_t, start_t, valid_ratios, pos, padding, spatial_shapes_list=sizes)
        return memory, padding, shapes_t, start_t
