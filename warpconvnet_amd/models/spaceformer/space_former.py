"""SpaCeFormer: a sparse-voxel U-Net whose attention flavour is chosen per level (https://arxiv.org/abs/2604.20395; reference
`warpconvnet/models/spaceformer/space_former.py`).

Every level runs blocks of ``block_factory(block_type)`` (`nn/modules/space_attention.py`) with one of
  ``curve``  serialized attention along a space-filling curve (``PatchAttention``),
  ``space``  window-grouped 3-D attention (``SpaceAttention``),
  ``all``    attention over whole batch elements (``AllAttention``);
levels are joined by stride-2 max pooling on the way down and by ``SparseUnpool`` with the skip features concatenated on the
way up.  Constructor arguments and state-dict layouts are the reference's.

Two switches surface the blocks' own ``NotImplementedError``: ``use_rope=True`` with a ``"curve"`` level (rotary curve attention:
``PatchAttention(use_rope=True)``), and ``use_checkpoint=True`` (the blocks do not checkpoint).  Logging goes through the
standard ``logging`` module.
"""
import logging
from typing import List, Literal, Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn

from warpconvnet_amd.geometry.base.geometry import Geometry
from warpconvnet_amd.geometry.coords.ops.serialization import POINT_ORDERING
from warpconvnet_amd.nn.functional.voxel_encode import WINDOW_OFFSET_TYPE
from warpconvnet_amd.nn.modules.base_module import BaseSpatialModel
from warpconvnet_amd.nn.modules.mlp import Linear
from warpconvnet_amd.nn.modules.sequential import Sequential, TupleSequential
from warpconvnet_amd.nn.modules.space_attention import block_factory
from warpconvnet_amd.nn.modules.sparse_conv import SparseConv3d
from warpconvnet_amd.nn.modules.sparse_pool import SparseMaxPool, SparseUnpool

__all__ = ["SpaCeFormer", "_parse_attn_type"]

logger = logging.getLogger(__name__)

_ATTN = Literal["curve", "space", "all"]


def _parse_attn_type(attn_type: Union[List[_ATTN], _ATTN, str], num_level: int) -> List[_ATTN]:
    """``attn_type`` as one name per level: a single name (``"curve"`` / ``"space"`` / ``"all"``) stands for every level, a
    compact code of ``num_level`` letters reads ``c`` / ``s`` / ``a`` per level (``"ccssa"``), a sequence of names is taken
    as it is."""
    mapping = {"c": "curve", "s": "space", "a": "all"}
    valid = set(mapping.values())
    if isinstance(attn_type, str):
        if attn_type.lower() in valid:
            return [attn_type] * num_level
        assert len(attn_type) == num_level, f"attn_type compact code {attn_type!r} must have length {num_level}"
        result = []
        for c in attn_type:
            assert c in mapping, f"Invalid attention code {c!r} in {attn_type!r}"
            result.append(mapping[c])
        return result
    if isinstance(attn_type, Sequence):
        assert len(attn_type) == num_level, f"attn_type sequence length {len(attn_type)} != num_level {num_level}"
        for t in attn_type:
            assert t in valid, f"Invalid attention type: {t!r}"
        return list(attn_type)
    raise ValueError(f"Invalid attn_type: {attn_type!r}")


class SpaCeFormer(BaseSpatialModel):
    """Encoder of ``len(enc_depths)`` levels, decoder of one fewer; ``enc_attn_types`` / ``dec_attn_types`` choose the
    attention of every level (``_parse_attn_type``), ``block_type`` where the norms sit (``pre_norm``, ``post_norm``,
    ``stream_norm``).  ``patch_size`` is the patch length of a ``curve`` level and the window edge of a ``space`` level.
    Every block call gets an ordering: one of ``patch_orders`` for a ``curve`` block, a window offset of ``voxel_offsets``
    otherwise - drawn from ``torch.randint`` when ``shuffle_orders``, else cycling by block number.  ``rope_base`` overrides
    both per-level lists.  ``conv_norm_layer`` follows the stem and the pooling / unpooling projections (None: no norm);
    ``out_channels`` adds a final ``Linear``."""

    def __init__(self, in_channels: int = 6, enc_depths: Tuple[int, ...] = (2, 2, 2, 6, 2),
                 enc_channels: Tuple[int, ...] = (32, 64, 128, 256, 512), enc_num_head: Tuple[int, ...] = (2, 4, 8, 16, 32),
                 enc_patch_size: Tuple[int, ...] = (1024, 1024, 1024, 1024, 1024), enc_attn_types: Union[_ATTN, str] = "curve",
                 dec_depths: Tuple[int, ...] = (2, 2, 2, 2), dec_channels: Tuple[int, ...] = (64, 64, 128, 256),
                 dec_num_head: Tuple[int, ...] = (4, 4, 8, 16), dec_patch_size: Tuple[int, ...] = (1024, 1024, 1024, 1024),
                 dec_attn_types: Union[_ATTN, str] = "curve",
                 block_type: Literal["pre_norm", "post_norm", "stream_norm"] = "pre_norm", kernel_size: int = 3,
                 mlp_ratio: float = 2.0, qkv_bias: bool = True, qk_scale: Optional[float] = None, attn_drop: float = 0.0,
                 proj_drop: float = 0.0, drop_path: float = 0.2, shuffle_orders: bool = True, use_rope: bool = False,
                 rope_base: Optional[int] = None, enc_rope_bases: Tuple[int, ...] = (250, 250, 250, 250, 250),
                 dec_rope_bases: Tuple[int, ...] = (250, 250, 250, 250),
                 voxel_offsets: List[Union[WINDOW_OFFSET_TYPE, str]] = ["zero", "xyz"],
                 patch_orders: Tuple[POINT_ORDERING, ...] = tuple(POINT_ORDERING), conv_norm_layer: Optional[type] = nn.BatchNorm1d,
                 out_channels: Optional[int] = None, use_checkpoint: bool = False):
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

        enc_attn_types = _parse_attn_type(enc_attn_types, num_level)
        dec_attn_types = _parse_attn_type(dec_attn_types, num_level - 1)
        self.enc_attn_types = enc_attn_types
        self.dec_attn_types = dec_attn_types
        self.voxel_offsets = voxel_offsets
        self.patch_orders = patch_orders

        self._log_level_configs("Encoder", "enc", block_type, enc_attn_types, enc_depths, range(num_level))
        self._log_level_configs("Decoder", "dec", block_type, dec_attn_types, dec_depths, list(reversed(range(num_level - 1))))

        if conv_norm_layer is None:
            conv_norm_layer = nn.Identity
        if rope_base is not None:
            enc_rope_bases = tuple([rope_base] * num_level)
            dec_rope_bases = tuple([rope_base] * (num_level - 1))
        logger.info("enc_rope_bases: %s", enc_rope_bases)
        logger.info("dec_rope_bases: %s", dec_rope_bases)

        block_cls = block_factory(block_type)

        def blocks(channels, patch_size, heads, depth, level, attn_type, base):
            return nn.ModuleList([
                block_cls(in_channels=channels, attention_channels=channels, patch_size=patch_size, num_heads=heads,
                          kernel_size=kernel_size, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop,
                          proj_drop=proj_drop, drop_path=drop_path, order=self._select_order(level, attn_type),
                          attn_type=attn_type, use_rope=use_rope, rope_base=base, use_checkpoint=use_checkpoint)
                for _ in range(depth)
            ])

        self.conv = Sequential(
            SparseConv3d(in_channels, enc_channels[0], kernel_size=5),
            conv_norm_layer(enc_channels[0]),
            nn.GELU(),
        )

        encs = nn.ModuleList()
        down_convs = nn.ModuleList()
        for i in range(num_level):
            encs.append(blocks(enc_channels[i], enc_patch_size[i], enc_num_head[i], enc_depths[i], i, enc_attn_types[i],
                               enc_rope_bases[i]))
            if i < num_level - 1:
                down_convs.append(
                    Sequential(
                        nn.Linear(enc_channels[i], enc_channels[i + 1]),
                        SparseMaxPool(kernel_size=2, stride=2),
                        conv_norm_layer(enc_channels[i + 1]),
                        nn.GELU(),
                    )
                )

        decs = nn.ModuleList()
        up_convs = nn.ModuleList()
        dec_channels_list = list(dec_channels) + [enc_channels[-1]]
        for i in reversed(range(num_level - 1)):
            up_convs.append(
                TupleSequential(
                    nn.Linear(dec_channels_list[i + 1], dec_channels_list[i]),
                    SparseUnpool(kernel_size=2, stride=2, concat_unpooled_st=True),
                    nn.Linear(dec_channels_list[i] + enc_channels[i], dec_channels_list[i]),
                    conv_norm_layer(dec_channels_list[i]),
                    nn.GELU(),
                    tuple_layer=1,
                )
            )
            decs.append(blocks(dec_channels_list[i], dec_patch_size[i], dec_num_head[i], dec_depths[i], i, dec_attn_types[i],
                               dec_rope_bases[i]))

        self.encs = encs
        self.down_convs = down_convs
        self.decs = decs
        self.up_convs = up_convs

        if out_channels is not None:
            self.out_channels = out_channels
            self.final = Linear(dec_channels_list[0], out_channels)
        else:
            self.final = nn.Identity()

    def _log_level_configs(self, phase_label: str, prefix: str, block_type, attn_types, depths, indices) -> None:
        for i in indices:
            if attn_types[i] in ("space", "all"):
                what, value = "voxel_offset", self.voxel_offsets[i % len(self.voxel_offsets)]
            else:
                what, value = "patch_order", self.patch_orders[i % len(self.patch_orders)]
            logger.info("[%s Level %d] %s_block_type: %s, %s_attn_type: %s, %s: %s, %d blocks", phase_label, i, prefix,
                        block_type, prefix, attn_types[i], what, value, depths[i])

    def _select_order(self, blk_idx: int, order_type: _ATTN) -> Union[POINT_ORDERING, str]:
        """The ordering of block ``blk_idx``: a window offset of ``voxel_offsets`` for ``space`` / ``all`` blocks (``all``
        does not use it), a curve of ``patch_orders`` for ``curve`` blocks; ``torch.manual_seed`` controls the draw."""
        orders = self.voxel_offsets if order_type in ("space", "all") else self.patch_orders
        if self.shuffle_orders:
            idx = torch.randint(0, len(orders), (1,)).item()
            return orders[idx]
        return orders[blk_idx % len(orders)]

    def forward(self, x: Geometry) -> Geometry:
        x = self.conv(x)
        skips = []
        block_idx = 0
        for level in range(self.num_level):
            for block in self.encs[level].children():
                x = block(x, self._select_order(block_idx, self.enc_attn_types[level]))
                block_idx += 1
            if level < self.num_level - 1:
                skips.append(x)
                x = self.down_convs[level](x)
        for level in range(self.num_level - 1):
            x = self.up_convs[level](x, skips[-(level + 1)])
            for block in self.decs[level].children():
                x = block(x, self._select_order(block_idx, self.dec_attn_types[-(level + 1)]))
                block_idx += 1
        return self.final(x)
