"""Swin Transformer backbone: SwinTransformer and D2SwinTransformer(cfg)
(projects/SeqFormer/seqformer/backbone/swin.py; the same file backs IDOL's Swin-L configs).

Same constructor arguments, cfg keys (MODEL.SWIN.*, projects/SeqFormer/seqformer/config.py:67-83) and parameter / buffer
names as the reference, so the backbone subtree of a reference checkpoint loads with strict=True:
patch_embed.{proj,norm}, layers.i.blocks.j.{norm1, attn.{qkv, proj, relative_position_bias_table,
relative_position_index}, norm2, mlp.{fc1, fc2}}, layers.i.downsample.{norm, reduction}, norm0..norm3.

The shifted-window attention of every block is vnext_amd/ops/window_attention.py (one HIP launch each way on the GPU;
the reference expression by torch on CPU).  LayerNorm, the MLP, PatchMerging and the patch embedding are library ops.
Opt-in (`BasicLayer.fused_glue` / `PatchMerging.fused_glue`, train.enable_fused_swin_glue): the stochastic depth, residual
add and LayerNorm around the two branches of every block, and PatchMerging's pad + gather + LayerNorm, run through
vnext_amd/ops/swin_glue.py (one HIP pass per site each way on the GPU; the same expression by torch elsewhere).

Differences from the reference, all outside the numbers: APE (absolute position embedding) is rejected (no config enables
it), USE_CHECKPOINT is rejected (activation checkpointing is not built), and timm's DropPath / trunc_normal_ are replaced by
`drop_path` below and torch.nn.init.trunc_normal_.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import swin_glue
from ..ops.window_attention import window_attention_block


def drop_path(x, p: float, training: bool):
    """Stochastic depth: with probability p a sample's residual branch is dropped, the kept ones scaled by 1 / (1 - p)."""
    if p == 0.0 or not training:
        return x
    keep = 1.0 - p
    mask = (keep + torch.rand((x.shape[0],) + (1,) * (x.dim() - 1), dtype=x.dtype, device=x.device)).floor_()
    return x.div(keep) * mask


class DropPath(nn.Module):
    def __init__(self, drop_prob=None):
        super().__init__()
        self.drop_prob = float(drop_prob or 0.0)

    def forward(self, x):
        return drop_path(x, self.drop_prob, self.training)


def _pair(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x, x)


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x):
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


def relative_position_index(w):
    """[w*w, w*w]: (dy + w - 1) (2 w - 1) + (dx + w - 1) for query token (y_i, x_i) and key token (y_j, x_j), dy = y_i - y_j."""
    ys, xs = torch.meshgrid(torch.arange(w), torch.arange(w), indexing="ij")
    ys, xs = ys.flatten(), xs.flatten()
    dy = ys[:, None] - ys[None, :] + w - 1
    dx = xs[:, None] - xs[None, :] + w - 1
    return dy * (2 * w - 1) + dx


class WindowAttention(nn.Module):
    """Parameters of the reference's WindowAttention; the computation is window_attention_block (ops/window_attention.py)."""

    def __init__(self, dim, window_size, num_heads, qkv_bias=True, qk_scale=None, attn_drop=0.0, proj_drop=0.0):
        super().__init__()
        self.dim = dim
        self.window_size = _pair(window_size)
        assert self.window_size[0] == self.window_size[1], "square windows only"
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        w = self.window_size[0]
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * w - 1) * (2 * w - 1), num_heads))
        self.register_buffer("relative_position_index", relative_position_index(w))
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        # opt-in (train.enable_bf16_window_attention): under torch.autocast(bfloat16) on CUDA the attention core takes the
        # bf16 qkv rows as the GEMM left them and runs on the matrix cores; off = the fp32 core (custom_fwd casts up)
        self.bf16_core = False
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02, a=-2.0, b=2.0)


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim, num_heads, window_size=7, shift_size=0, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop=0.0,
                 attn_drop=0.0, drop_path=0.0, act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.num_heads = num_heads
        self.window_size = window_size
        self.shift_size = shift_size
        self.mlp_ratio = mlp_ratio
        assert 0 <= self.shift_size < self.window_size, "shift_size must in 0-window_size"
        self.norm1 = norm_layer(dim)
        self.attn = WindowAttention(dim, window_size=window_size, num_heads=num_heads, qkv_bias=qkv_bias,
                                    qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)

    def forward(self, x, H, W):
        """x [B, H*W, C] -> [B, H*W, C]"""
        B, L, C = x.shape
        assert L == H * W, "input feature has wrong size"
        x = x + self.drop_path(window_attention_block(self.norm1(x), H, W, self.attn, self.window_size, self.shift_size))
        return x + self.drop_path(self.mlp(self.norm2(x)))


class PatchMerging(nn.Module):
    def __init__(self, dim, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = norm_layer(4 * dim)
        self.fused_glue = False      # opt-in (train.enable_fused_swin_glue): pad + gather + norm in one pass (ops/swin_glue.py)

    def forward(self, x, H, W):
        B, L, C = x.shape
        assert L == H * W, "input feature has wrong size"
        if self.fused_glue:
            return self.reduction(swin_glue.merge_norm(x, H, W, self.norm))
        x = x.view(B, H, W, C)
        if H % 2 == 1 or W % 2 == 1:
            x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
        x = torch.cat([x[:, 0::2, 0::2, :], x[:, 1::2, 0::2, :], x[:, 0::2, 1::2, :], x[:, 1::2, 1::2, :]], -1)
        return self.reduction(self.norm(x.view(B, -1, 4 * C)))


class BasicLayer(nn.Module):
    """One stage: `depth` blocks, W-MSA and SW-MSA alternating, then PatchMerging (but the last stage)."""

    def __init__(self, dim, depth, num_heads, window_size=7, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop=0.0,
                 attn_drop=0.0, drop_path=0.0, norm_layer=nn.LayerNorm, downsample=None, use_checkpoint=False):
        super().__init__()
        if use_checkpoint:
            raise NotImplementedError("SwinTransformer: activation checkpointing (USE_CHECKPOINT) is not built")
        self.window_size = window_size
        self.shift_size = window_size // 2
        self.depth = depth
        self.use_checkpoint = use_checkpoint
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim=dim, num_heads=num_heads, window_size=window_size,
                                 shift_size=0 if (i % 2 == 0) else window_size // 2, mlp_ratio=mlp_ratio,
                                 qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop, attn_drop=attn_drop,
                                 drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path,
                                 norm_layer=norm_layer)
            for i in range(depth)])
        self.downsample = downsample(dim=dim, norm_layer=norm_layer) if downsample is not None else None
        # opt-in (train.enable_fused_swin_glue): every residual add (with its stochastic depth) is fused with the LayerNorm
        # that follows it -- norm2 inside a block, the NEXT block's norm1 between blocks (ops/swin_glue.py)
        self.fused_glue = False

    def _blocks_fused(self, x, H, W):
        """The blocks with (x, n) threaded through them: x the residual stream, n the LayerNorm of it the next branch reads.
        The same function as the loop over blk(x, H, W); the stochastic-depth masks are drawn at the same points."""
        assert x.shape[1] == H * W, "input feature has wrong size"
        blocks = list(self.blocks)
        _, n = swin_glue.residual_norm(x, None, None, blocks[0].norm1)
        for i, blk in enumerate(blocks):
            p = getattr(blk.drop_path, "drop_prob", 0.0)
            a = window_attention_block(n, H, W, blk.attn, blk.window_size, blk.shift_size)
            x, n = swin_glue.residual_norm(x, a, swin_glue.drop_scale(a, p, blk.drop_path.training), blk.norm2)
            a = blk.mlp(n)
            x, n = swin_glue.residual_norm(x, a, swin_glue.drop_scale(a, p, blk.drop_path.training),
                                           blocks[i + 1].norm1 if i + 1 < len(blocks) else None)
        return x

    def forward(self, x, H, W):
        if self.fused_glue and len(self.blocks) > 0:
            x = self._blocks_fused(x, H, W)
        else:
            for blk in self.blocks:
                x = blk(x, H, W)
        if self.downsample is not None:
            return x, H, W, self.downsample(x, H, W), (H + 1) // 2, (W + 1) // 2
        return x, H, W, x, H, W


class PatchEmbed(nn.Module):
    def __init__(self, patch_size=4, in_chans=3, embed_dim=96, norm_layer=None):
        super().__init__()
        self.patch_size = _pair(patch_size)
        self.in_chans = in_chans
        self.embed_dim = embed_dim
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=self.patch_size)
        self.norm = norm_layer(embed_dim) if norm_layer is not None else None

    def forward(self, x):
        _, _, H, W = x.size()
        if W % self.patch_size[1] != 0:
            x = F.pad(x, (0, self.patch_size[1] - W % self.patch_size[1]))
        if H % self.patch_size[0] != 0:
            x = F.pad(x, (0, 0, 0, self.patch_size[0] - H % self.patch_size[0]))
        x = self.proj(x)
        if self.norm is not None:
            Wh, Ww = x.size(2), x.size(3)
            x = self.norm(x.flatten(2).transpose(1, 2)).transpose(1, 2).view(-1, self.embed_dim, Wh, Ww)
        return x


class SwinTransformer(nn.Module):
    """forward(x [B, 3, H, W]) -> {"res2": .., "res5": ..} NCHW, the stages in `out_indices` (the reference's output)."""

    def __init__(self, pretrain_img_size=224, patch_size=4, in_chans=3, embed_dim=96, depths=(2, 2, 6, 2),
                 num_heads=(3, 6, 12, 24), window_size=7, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop_rate=0.0,
                 attn_drop_rate=0.0, drop_path_rate=0.2, norm_layer=nn.LayerNorm, ape=False, patch_norm=True,
                 out_indices=(0, 1, 2, 3), frozen_stages=-1, use_checkpoint=False):
        super().__init__()
        if ape:
            raise NotImplementedError("SwinTransformer: the absolute position embedding (APE) is not built")
        self.pretrain_img_size = pretrain_img_size
        self.num_layers = len(depths)
        self.embed_dim = embed_dim
        self.ape = ape
        self.patch_norm = patch_norm
        self.out_indices = tuple(out_indices)
        self.frozen_stages = frozen_stages
        self.patch_embed = PatchEmbed(patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim,
                                      norm_layer=norm_layer if patch_norm else None)
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, sum(depths))]     # linear stochastic-depth schedule
        self.layers = nn.ModuleList()
        for i in range(self.num_layers):
            self.layers.append(BasicLayer(
                dim=int(embed_dim * 2 ** i), depth=depths[i], num_heads=num_heads[i], window_size=window_size,
                mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate,
                drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])], norm_layer=norm_layer,
                downsample=PatchMerging if i < self.num_layers - 1 else None, use_checkpoint=use_checkpoint))
        self.num_features = [int(embed_dim * 2 ** i) for i in range(self.num_layers)]
        for i in self.out_indices:
            self.add_module(f"norm{i}", norm_layer(self.num_features[i]))
        self._freeze_stages()

    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            self.patch_embed.eval()
            for p in self.patch_embed.parameters():
                p.requires_grad = False
        if self.frozen_stages >= 2:
            self.pos_drop.eval()
            for i in range(0, self.frozen_stages - 1):
                m = self.layers[i]
                m.eval()
                for p in m.parameters():
                    p.requires_grad = False

    def _stages(self, x, wanted):
        x = self.patch_embed(x)
        Wh, Ww = x.size(2), x.size(3)
        x = self.pos_drop(x.flatten(2).transpose(1, 2))
        outs = {}
        last = max(wanted)
        for i in range(last + 1):
            x_out, H, W, x, Wh, Ww = self.layers[i](x, Wh, Ww)
            if i in wanted:
                x_out = getattr(self, f"norm{i}")(x_out)
                outs[f"res{i + 2}"] = x_out.view(-1, H, W, self.num_features[i]).permute(0, 3, 1, 2).contiguous()
        return outs

    def forward(self, x):
        return self._stages(x, self.out_indices)

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        return self


class D2SwinTransformer(SwinTransformer):
    """The reference's Detectron2 backbone, built from cfg.MODEL.SWIN.*, as this package's DeformableDETR consumes a
    backbone (the interface of seqformer.ResNet50Trunk): forward(x) -> [res3, res4, res5] NCHW, strides (8, 16, 32),
    num_channels (2 C, 4 C, 8 C).  `features(x)` gives the reference's dict, filtered by MODEL.SWIN.OUT_FEATURES.

    res2 (norm0) is computed by the reference and never read by SeqFormer / IDOL.  Here forward() does not compute it and
    norm0's parameters stay (the checkpoint has them) with requires_grad False, so DistributedDataParallel with
    find_unused_parameters=False / static_graph=True finds no parameter that never gets a gradient."""
    strides = (8, 16, 32)

    def __init__(self, cfg, input_shape=None):
        s = cfg.MODEL.SWIN
        super().__init__(s.PRETRAIN_IMG_SIZE, s.PATCH_SIZE, 3, s.EMBED_DIM, list(s.DEPTHS), list(s.NUM_HEADS),
                         s.WINDOW_SIZE, s.MLP_RATIO, s.QKV_BIAS, s.QK_SCALE, s.DROP_RATE, s.ATTN_DROP_RATE,
                         s.DROP_PATH_RATE, nn.LayerNorm, s.APE, s.PATCH_NORM, use_checkpoint=s.USE_CHECKPOINT)
        self._out_features = list(s.OUT_FEATURES)
        self._out_feature_strides = {"res2": 4, "res3": 8, "res4": 16, "res5": 32}
        self._out_feature_channels = {f"res{i + 2}": self.num_features[i] for i in range(4)}
        self.num_channels = tuple(self.num_features[1:4])
        self.norm0.requires_grad_(False)

    def features(self, x):
        assert x.dim() == 4, f"SwinTransformer takes an input of shape (N, C, H, W). Got {x.shape} instead!"
        y = super().forward(x)
        return {k: v for k, v in y.items() if k in self._out_features}

    def forward(self, x):
        y = self._stages(x, (1, 2, 3))
        return [y["res3"], y["res4"], y["res5"]]

    def output_shape(self):
        return {name: (self._out_feature_channels[name], self._out_feature_strides[name]) for name in self._out_features}

    @property
    def size_divisibility(self):
        return 32


def is_swin(cfg) -> bool:
    backbone = getattr(cfg.MODEL, "BACKBONE", None)
    return backbone is not None and getattr(backbone, "NAME", "") == "D2SwinTransformer"
