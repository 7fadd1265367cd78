"""Point Transformer V3 on sparse voxels ("Point Transformer V3: Simpler, Faster, Stronger", https://arxiv.org/abs/2312.10035;
reference `warpconvnet/models/point_transformer_v3.py`): a U-Net of serialized patch-attention blocks between max-pool
downsamples and additive unpoolings.  Constructor arguments and state-dict layouts are the reference's.

The attention sub-layer of a block, ``x + drop_path(attention(norm1(x), order))``, is around the attention itself a LayerNorm,
two row gathers, the stochastic-depth multiply and the residual add: nine row passes over [N, C].  ``PatchAttentionBlock`` runs
it as ``layer_norm_permute`` -> ``PatchAttention.forward_ordered`` -> ``permute_add`` (`nn/functional/row_permute.py`, two row
passes) where that applies, and as the composed expression otherwise; ``WARPCONVNET_AMD_PTV3_FUSED=0`` forces the composed
one.  The serialization of a level is computed once per order and kept in the geometry's spatial cache.

Divergences from the reference: ``use_checkpoint=True`` wraps a block in ``torch.utils.checkpoint`` (the reference's
checkpointing mixins are not ported); attention dropout while training raises ``NotImplementedError`` (``PatchAttention``).
"""
import os
from typing import Literal, Optional, Tuple, Union

import torch
import torch.nn as nn
from torch.utils.checkpoint import checkpoint

from warpconvnet_amd.geometry.base.geometry import Geometry
from warpconvnet_amd.geometry.coords.ops.serialization import POINT_ORDERING, to_point_ordering
from warpconvnet_amd.nn.functional.row_permute import hip_row_permute_supported, layer_norm_permute, permute_add
from warpconvnet_amd.nn.modules.activations import GELU, DropPath
from warpconvnet_amd.nn.modules.attention import LayerNorm, PatchAttention
from warpconvnet_amd.nn.modules.base_module import BaseSpatialModel, BaseSpatialModule
from warpconvnet_amd.nn.modules.mlp import Linear
from warpconvnet_amd.nn.modules.sequential import Sequential, _has_hooks
from warpconvnet_amd.nn.modules.sparse_conv import SparseConv3d
from warpconvnet_amd.nn.modules.sparse_pool import SparseMaxPool, SparseUnpool

__all__ = ["MLP", "PatchAttentionBlock", "SerializedUnpooling", "PointTransformerV3"]

# dtypes whose attention sub-layer takes the fused row passes by default (the measured table decides this)
_FUSED_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _fused_enabled() -> bool:
    return os.environ.get("WARPCONVNET_AMD_PTV3_FUSED", "1") != "0"


class MLP(nn.Module):
    """Linear -> act -> Dropout -> Linear -> Dropout on the features (state-dict keys ``mlp.0.*``, ``mlp.3.*``)."""

    def __init__(self, in_channels, hidden_channels=None, out_channels=None, act_layer=nn.GELU, drop=0.0):
        super().__init__()
        out_channels = out_channels or in_channels
        hidden_channels = hidden_channels or in_channels
        self.mlp = Sequential(
            nn.Linear(in_channels, hidden_channels),
            act_layer(),
            nn.Dropout(drop),
            nn.Linear(hidden_channels, out_channels),
            nn.Dropout(drop),
        )

    def forward(self, x):
        return self.mlp(x)


class PatchAttentionBlock(BaseSpatialModule):
    """``x = conv(x) + shortcut(x); x = x + drop_path(attention(norm1(x), order)); x = x + drop_path(mlp(norm2(x)))``."""

    def __init__(self, in_channels: int, attention_channels: int, patch_size: int, num_heads: int, kernel_size: int = 3,
                 mlp_ratio: float = 4.0, qkv_bias: bool = True, qk_scale: Optional[float] = None, attn_drop: float = 0.0,
                 proj_drop: float = 0.0, drop_path: float = 0.0, norm_layer: type = LayerNorm, act_layer: type = GELU,
                 attn_type: Literal["patch"] = "patch", order: POINT_ORDERING = POINT_ORDERING.MORTON_XYZ,
                 use_checkpoint: bool = False):
        super().__init__()
        self.use_checkpoint = use_checkpoint
        self.order = order
        self.conv = Sequential(
            SparseConv3d(in_channels, in_channels, kernel_size=kernel_size, stride=1, bias=True),
            nn.Linear(in_channels, attention_channels),
            norm_layer(attention_channels),
        )
        self.conv_shortcut = nn.Identity() if in_channels == attention_channels else Linear(in_channels, attention_channels)
        self.norm1 = norm_layer(attention_channels)
        self.attention = PatchAttention(attention_channels, patch_size=patch_size, num_heads=num_heads, qkv_bias=qkv_bias,
                                        qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=proj_drop, order=order)
        self.norm2 = norm_layer(attention_channels)
        self.mlp = MLP(in_channels=attention_channels, hidden_channels=int(attention_channels * mlp_ratio),
                       out_channels=attention_channels, drop=proj_drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()

    # ---- the attention sub-layer -----------------------------------------------------------------------------------------
    def _fused_applies(self, x: Geometry) -> bool:
        """The fused row passes compute what the composed expression computes only for the package ``LayerNorm`` with its
        affine pair; they call neither ``norm1`` nor ``attention`` nor ``drop_path`` as modules, so any hook on those (and
        autocast, which changes what the modules' own calls return) keeps the composed expression."""
        feats = x.feature_tensor
        norm = self.norm1
        if not (_fused_enabled() and feats.dtype in _FUSED_DTYPES and hip_row_permute_supported(feats)):
            return False
        if type(norm) is not LayerNorm or type(norm.norm) is not nn.LayerNorm:
            return False
        ln = norm.norm
        if ln.weight is None or ln.bias is None or tuple(ln.normalized_shape) != (feats.shape[1],):
            return False
        if torch.is_autocast_enabled() or (self.training and self.attention.attn_drop_p > 0.0):
            return False
        return not any(_has_hooks(m) for m in (norm, ln, self.attention, self.drop_path))

    def _drop_path_scale(self, feats: torch.Tensor) -> Optional[torch.Tensor]:
        """The per-row factor of ``drop_path`` (`nn/modules/activations.py`), drawn the way it draws it."""
        dp = self.drop_path
        if not isinstance(dp, DropPath) or dp.drop_prob == 0.0 or not self.training:
            return None
        keep_prob = 1 - dp.drop_prob
        mask = feats.new_empty((feats.shape[0], 1)).bernoulli_(keep_prob)
        if keep_prob > 0.0 and dp.scale_by_keep:
            mask.div_(keep_prob)
        return mask

    def _attention_sublayer(self, x: Geometry, order) -> Geometry:
        if self._fused_applies(x):
            attn = self.attention
            res = attn.serialization(x, to_point_ordering(order or attn.order))
            if res is not None:  # (a geometry already in that order has nothing to permute)
                feats = x.feature_tensor
                ln = self.norm1.norm
                rows = layer_norm_permute(feats, res.perm, res.inverse_perm, ln.weight, ln.bias, ln.eps)
                rows = attn.forward_ordered(rows, x.offsets).to(feats.dtype)
                out = permute_add(rows, res.inverse_perm, res.perm, feats, self._drop_path_scale(feats))
                return x.replace(batched_features=out)
        return self.drop_path(self.attention(self.norm1(x), order)) + x

    def _forward(self, x: Geometry, order: Optional[Union[POINT_ORDERING, str]] = None) -> Geometry:
        x = self.conv(x) + self.conv_shortcut(x)
        x = self._attention_sublayer(x, order)
        x = self.drop_path(self.mlp(self.norm2(x))) + x
        return x

    def forward(self, x: Geometry, order: Optional[Union[POINT_ORDERING, str]] = None) -> Geometry:
        if hasattr(x, "spatial_cache"):
            x.spatial_cache  # created before the first `replace`, so every geometry of this level shares one cache
        if self.use_checkpoint and torch.is_grad_enabled():
            out = checkpoint(lambda f: self._forward(x.replace(batched_features=f), order).feature_tensor, x.feature_tensor,
                             use_reentrant=False)
            return x.replace(batched_features=out)
        return self._forward(x, order)


class SerializedUnpooling(BaseSpatialModule):
    """Project the coarse features, unpool them onto the skip's voxels and ADD the projected skip features (the official
    Point Transformer V3 unpooling; nothing is concatenated)."""

    def __init__(self, in_channels: int, skip_channels: int, out_channels: int, kernel_size: int = 2, stride: int = 2,
                 norm_layer: type = nn.BatchNorm1d, act_layer: type = GELU):
        super().__init__()
        self.proj = Sequential(
            nn.Linear(in_channels, out_channels),
            norm_layer(out_channels) if norm_layer is not None else nn.Identity(),
            act_layer() if act_layer is not None else nn.Identity(),
        )
        self.proj_skip = Sequential(
            nn.Linear(skip_channels, out_channels),
            norm_layer(out_channels) if norm_layer is not None else nn.Identity(),
            act_layer() if act_layer is not None else nn.Identity(),
        )
        self.unpool = SparseUnpool(kernel_size=kernel_size, stride=stride, concat_unpooled_st=False)

    def forward(self, x: Geometry, skip: Geometry) -> Geometry:
        x = self.unpool(self.proj(x), skip)
        skip = self.proj_skip(skip)
        return x.replace(batched_features=x.feature_tensor + skip.feature_tensor)


class PointTransformerV3(BaseSpatialModel):
    """Encoder of ``len(enc_depths)`` levels, decoder of one level fewer.  Every block runs under one of ``orders``: drawn
    from ``torch.randint`` per block when ``shuffle_orders`` (seed with ``torch.manual_seed``), else cycling through
    ``orders`` by block number.  ``out_channels=`` adds a final ``Linear``."""

    def __init__(self, in_channels: int = 6, enc_depths: Tuple[int, ...] = (2, 2, 2, 6, 2),
                 enc_channels: Tuple[int, ...] = (32, 64, 128, 256, 512), enc_num_head: Tuple[int, ...] = (2, 4, 8, 16, 32),
                 enc_patch_size: Tuple[int, ...] = (1024, 1024, 1024, 1024, 1024), dec_depths: Tuple[int, ...] = (2, 2, 2, 2),
                 dec_channels: Tuple[int, ...] = (64, 64, 128, 256), dec_num_head: Tuple[int, ...] = (4, 4, 8, 16),
                 dec_patch_size: Tuple[int, ...] = (1024, 1024, 1024, 1024), mlp_ratio: float = 4, qkv_bias: bool = True,
                 qk_scale: Optional[float] = None, attn_drop: float = 0.0, proj_drop: float = 0.0, drop_path: float = 0.2,
                 orders: Tuple[POINT_ORDERING, ...] = tuple(POINT_ORDERING), shuffle_orders: bool = True,
                 attn_type: Literal["patch"] = "patch", use_checkpoint: bool = False, **kwargs):
        super().__init__()
        num_level = len(enc_depths)
        assert num_level == len(enc_channels)
        assert num_level == len(enc_num_head)
        assert num_level == len(enc_patch_size)
        assert num_level - 1 == len(dec_channels)
        assert num_level - 1 == len(dec_depths)
        assert num_level - 1 == len(dec_num_head)
        assert num_level - 1 == len(dec_patch_size)
        self.num_level = num_level
        self.shuffle_orders = shuffle_orders
        self.orders = orders

        self.conv = Sequential(
            SparseConv3d(in_channels, enc_channels[0], kernel_size=5, bias=False),
            nn.BatchNorm1d(enc_channels[0]),
            nn.GELU(),
        )

        def blocks(channels, patch_size, heads, depth, level):
            return nn.ModuleList([
                PatchAttentionBlock(in_channels=channels, attention_channels=channels, patch_size=patch_size, num_heads=heads,
                                    mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop,
                                    proj_drop=proj_drop, drop_path=drop_path, order=self.orders[level % len(self.orders)],
                                    attn_type=attn_type, use_checkpoint=use_checkpoint)
                for _ in range(depth)
            ])

        encs = nn.ModuleList()
        down_convs = nn.ModuleList()
        for i in range(num_level):
            encs.append(blocks(enc_channels[i], enc_patch_size[i], enc_num_head[i], enc_depths[i], i))
            if i < num_level - 1:
                down_convs.append(
                    Sequential(
                        nn.Linear(enc_channels[i], enc_channels[i + 1]),
                        SparseMaxPool(kernel_size=2, stride=2),
                        nn.BatchNorm1d(enc_channels[i + 1]),
                        nn.GELU(),
                    )
                )

        decs = nn.ModuleList()
        up_convs = nn.ModuleList()
        dec_channels_list = list(dec_channels) + [enc_channels[-1]]
        for i in reversed(range(num_level - 1)):
            up_convs.append(
                SerializedUnpooling(in_channels=dec_channels_list[i + 1], skip_channels=enc_channels[i],
                                    out_channels=dec_channels_list[i], kernel_size=2, stride=2, norm_layer=nn.BatchNorm1d,
                                    act_layer=GELU)
            )
            decs.append(blocks(dec_channels_list[i], dec_patch_size[i], dec_num_head[i], dec_depths[i], i))

        self.encs = encs
        self.down_convs = down_convs
        self.decs = decs
        self.up_convs = up_convs

        out_channels = kwargs.get("out_channels")
        if out_channels is not None:
            self.out_channels = out_channels
            self.final = Linear(dec_channels_list[0], out_channels)
        else:
            self.final = nn.Identity()

    def _select_order(self, blk_idx: int) -> POINT_ORDERING:
        """The ordering of block ``blk_idx``; ``torch.manual_seed`` controls the draw."""
        if self.shuffle_orders:
            idx = torch.randint(0, len(self.orders), (1,)).item()
            return self.orders[idx]
        return self.orders[blk_idx % len(self.orders)]

    def forward(self, x: Geometry) -> Geometry:
        x = self.conv(x)
        skips = []
        blk_idx = 0
        for level in range(self.num_level):
            for block in self.encs[level].children():
                x = block(x, self._select_order(blk_idx))
                blk_idx += 1
            if level < self.num_level - 1:
                skips.append(x)
                x = self.down_convs[level](x)
        for level in range(self.num_level - 1):
            x = self.up_convs[level](x, skips[-(level + 1)])
            for block in self.decs[level].children():
                x = block(x, self._select_order(blk_idx))
                blk_idx += 1
        return self.final(x)
