"""Window-grouped voxel attention and the SpaCeFormer block family (reference `nn/modules/space_attention.py`).

``SpaceAttention`` groups the voxels into 3-D windows (optionally on a shifted window grid) and runs multi-head softmax
attention inside every window; ``window_size="all"`` attends over whole batch elements.  The forward is

    voxel_encode (cached on the geometry's spatial cache)  ->  rows gathered by ``perm``  ->  ``qkv``  ->  rotary embedding
    ->  ``flash_attn_varlen_qkvpacked(cu_seqlens, max_count)``  ->  ``proj``  ->  rows gathered by ``inverse_perm``

with the grouping from `csrc/window_group.hip`, the rotation from `csrc/qk_prologue.hip` and the attention core from
`csrc/attn_varlen.hip`.  Both row permutations go through one autograd function whose backward is the gather by the other
permutation: no ``index_put`` accumulation, bit-identical gradients from run to run.  CPU tensors take the same path with
``varlen_attention_reference`` as the core (fp32, no fp16 cast).

``PreNormBlock`` / ``PostNormBlock`` / ``StreamNormBlock`` bundle a sparse-conv shortcut, one of ``STR2ATTN`` and a
``FeedForward``.  Constructor arguments and state-dict layouts are the reference's.  Attention dropout while training and
``use_checkpoint=True`` raise ``NotImplementedError``.
"""
from typing import Literal, Optional, Tuple, Union

import torch
import torch.nn as nn
from torch import Tensor
from torch.autograd import Function

from warpconvnet_amd.geometry.base.geometry import Geometry
from warpconvnet_amd.geometry.coords.ops.serialization import POINT_ORDERING
from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_qkvpacked, varlen_attention_reference
from warpconvnet_amd.nn.functional.qk_prologue import qk_prologue, rope_table
from warpconvnet_amd.nn.functional.voxel_encode import WINDOW_OFFSET_TYPE, VoxelEncodeResult, voxel_encode, voxel_encode_cached
from warpconvnet_amd.nn.modules.activations import DropPath
from warpconvnet_amd.nn.modules.attention import BatchedLinear, FeedForward, LayerNorm, PatchAttention
from warpconvnet_amd.nn.modules.base_module import BaseSpatialModule
from warpconvnet_amd.nn.modules.mlp import Linear
from warpconvnet_amd.nn.modules.rope import VoxelRotaryPositionalEmbeddings
from warpconvnet_amd.nn.modules.sequential import Sequential
from warpconvnet_amd.nn.modules.sparse_conv import SparseConv3d

__all__ = ["SpaceAttention", "AllAttention", "STR2ATTN", "SpaCeFormerBlockBase", "PreNormBlock", "PostNormBlock",
           "StreamNormBlock", "BLOCK_REGISTRY", "block_factory", "permute_rows"]


class _PermuteRows(Function):
    """``out[j] = x[index[j]]`` for a permutation ``index`` with inverse ``inverse``: the gradient is the gather
    ``dx[i] = dout[inverse[i]]`` (every row read once, nothing accumulated)."""

    @staticmethod
    def forward(ctx, x: Tensor, index: Tensor, inverse: Tensor) -> Tensor:
        ctx.save_for_backward(inverse)
        return x.index_select(0, index)

    @staticmethod
    def backward(ctx, dout: Tensor):
        (inverse,) = ctx.saved_tensors
        return dout.index_select(0, inverse), None, None


def permute_rows(x: Tensor, index: Tensor, inverse: Tensor) -> Tensor:
    """Rows of ``x`` in the order of the permutation ``index``; ``inverse`` is its inverse permutation."""
    return _PermuteRows.apply(x, index, inverse)


def _combine_consecutive_ones(counts: Tensor) -> Tensor:
    """Sequence boundaries (int32) of the windows with every run of length-1 windows merged into one sequence."""
    if counts.numel() == 0:
        return torch.zeros(1, device=counts.device, dtype=torch.int32)
    is_one = counts == 1
    follows_one = torch.cat([is_one.new_zeros(1), is_one[:-1]])
    starts = ~(is_one & follows_one)  # a window opens a sequence unless it is a 1 right behind a 1
    ends = torch.cumsum(counts, dim=0)
    return torch.cat([(ends - counts)[starts], ends[-1:]]).int().contiguous()


class SpaceAttention(BaseSpatialModule):
    """Multi-head attention inside 3-D windows of ``window_size`` voxels per axis (an int, 3 ints, or ``"all"`` for whole
    batch elements).  ``offset`` shifts the window grid: a key of ``STR2COORD_OFFSET`` or 3 fractions of the window.
    ``combine_consecutive_ones`` merges runs of single-voxel windows into one sequence.  ``use_rope`` turns Q and K by
    ``VoxelRotaryPositionalEmbeddings`` (``rope_base``).  fp32 features run the attention core in fp16 on the GPU.  The
    reference's constructor and state dict (``qkv``, ``proj``)."""

    def __init__(self, dim: int, window_size: Optional[Union[Tuple[int, int, int], int, str]] = None, num_heads: int = 8,
                 qkv_bias: bool = False, qk_scale: Optional[float] = None, attn_drop: float = 0.0, proj_drop: float = 0.0,
                 offset: Union[WINDOW_OFFSET_TYPE, Tuple[float, float, float]] = "zero",
                 combine_consecutive_ones: bool = False, use_rope: bool = True, rope_base: int = 250,
                 use_batched_qkv: bool = True, encoding_method: str = "counting_sort"):
        super().__init__()
        self.encoding_method = encoding_method
        if isinstance(window_size, str):
            assert window_size == "all", f"Invalid window_size: {window_size}"
        if isinstance(window_size, int):
            window_size = (window_size, window_size, window_size)
        self.window_size = window_size
        self.num_heads = num_heads
        assert dim % num_heads == 0, "dim must be divisible by num_heads"
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.use_batched_qkv = use_batched_qkv
        if use_batched_qkv:
            self.qkv = BatchedLinear(dim, dim, num_matrices=3, bias=qkv_bias)
        else:
            self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.offset = offset
        self.attn_drop_p = attn_drop
        self.combine_consecutive_ones = combine_consecutive_ones
        self.use_rope = use_rope
        if use_rope:
            self.rope = VoxelRotaryPositionalEmbeddings(dim=dim, num_heads=num_heads, base=rope_base)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def _attn_offset(self, counts: Tensor) -> Tensor:
        return torch.cat([counts.new_zeros(1), torch.cumsum(counts, dim=0)]).int().contiguous()

    def _attn_offset_combine_consecutive_ones(self, counts: Tensor) -> Tensor:
        return _combine_consecutive_ones(counts)

    # ---- what depends on the coordinates alone: cached on the geometry ---------------------------------------------------
    def _encode(self, x: Geometry, coord_offset) -> Tuple[VoxelEncodeResult, Optional[dict], tuple]:
        """The window grouping of ``x``: from the geometry's spatial cache (shared by every geometry made from it with
        ``replace``, so sibling blocks of one level encode once), else from the module-level cache of ``voxel_encode``."""
        cache = getattr(x, "spatial_cache", None)
        if cache is None:
            return voxel_encode_cached(x.coordinate_tensor, batch_offsets=x.offsets, window_size=self.window_size,
                                       coord_offset=coord_offset, encoding_method=self.encoding_method), None, ()
        kwargs = dict(batch_offsets=x.offsets, window_size=self.window_size, coord_offset=coord_offset, return_perm=True,
                      return_inverse=True, return_counts=True, encoding_method=self.encoding_method)
        if coord_offset == "random":
            return voxel_encode(x.coordinate_tensor, **kwargs), None, ()
        offset_key = coord_offset if isinstance(coord_offset, str) else tuple(float(v) for v in coord_offset)
        key = ("voxel_encode", tuple(self.window_size), offset_key, self.encoding_method)
        res = cache.get(key)
        if res is None:
            res = cache[key] = voxel_encode(x.coordinate_tensor, **kwargs)
        return res, cache, key

    def _sequences(self, res: VoxelEncodeResult, cache: Optional[dict], key: tuple) -> Tuple[Tensor, int]:
        if not self.combine_consecutive_ones:
            return res.cu_seqlens, int(res.max_count)
        ckey = ("combined_ones",) + key
        hit = cache.get(ckey) if cache is not None and key else None
        if hit is None:
            cu = self._attn_offset_combine_consecutive_ones(res.counts)
            # a merged run can be longer than the longest window: the attention grid is sized by the longest SEQUENCE
            hit = (cu, int((cu[1:] - cu[:-1]).max()) if cu.numel() > 1 else 0)
            if cache is not None and key:
                cache[ckey] = hit
        return hit

    def _rotate(self, qkv: Tensor, coords: Tensor, cache: Optional[dict], key: tuple) -> Tensor:
        """[M, 3, C] -> [M, 3, H, D], Q and K turned; the (cos, sin) table of the ordered coordinates is cached next to the
        grouping.  The convention of ``fused_rope_qkv``: positions count from the column minimum, plus one."""
        m, h = qkv.shape[0], self.num_heads
        x = qkv.reshape(m, 3, h, -1)
        rope = self.rope
        if rope.rope_dim == 0 or m == 0:
            return x
        tkey = ("rope_table", rope.base, rope.head_dim) + key
        table = cache.get(tkey) if cache is not None and key else None
        if table is None:
            table = rope_table(coords, rope.theta, origin=coords.min(0).values.to(torch.float32), bias=1.0)
            if cache is not None and key:
                cache[tkey] = table
        # the GPU kernels write fp16 for fp32 rows (the core's dtype); the CPU path stays in the input dtype
        return qk_prologue(x, table, out_dtype=None if x.is_cuda else x.dtype)

    def forward(self, x: Geometry,
                coord_offset: Union[Tuple[float, float, float], WINDOW_OFFSET_TYPE, None] = "zero") -> Geometry:
        if self.training and self.attn_drop_p > 0.0:
            raise NotImplementedError("SpaceAttention: attention dropout (attn_drop > 0 while training) is not implemented")
        if coord_offset is None:
            coord_offset = self.offset
        assert isinstance(coord_offset, str) or (isinstance(coord_offset, tuple) and len(coord_offset) == 3), (
            "coord_offset must be a tuple of 3 floats or a string")
        feats = x.feature_tensor
        coords = x.coordinate_tensor
        m, c = feats.shape[:2]
        res, cache, key = None, getattr(x, "spatial_cache", None), ()
        if self.window_size == "all":
            offsets = x.offsets.to(device="cpu", dtype=torch.int64)
            lens = offsets[1:] - offsets[:-1]
            cu, max_seqlen = offsets.to(torch.int32), (int(lens.max()) if lens.numel() else 0)
            key = ("all",)
        else:
            res, cache, key = self._encode(x, coord_offset)
            cu, max_seqlen = self._sequences(res, cache, key)
            feats = permute_rows(feats, res.perm, res.inverse_perm)
            if self.use_rope:
                coords = coords[res.perm]
        qkv = self.qkv(feats)
        if self.use_rope:
            qkv = self._rotate(qkv.reshape(m, 3, c), coords, cache, key)
        else:
            qkv = qkv.reshape(m, 3, self.num_heads, c // self.num_heads)
        if qkv.is_cuda:
            if qkv.dtype not in (torch.float16, torch.bfloat16):
                qkv = qkv.to(torch.float16)
            out = flash_attn_varlen_qkvpacked(qkv, cu, max_seqlen=max_seqlen, dropout_p=0.0, softmax_scale=self.scale)
        else:
            out, _ = varlen_attention_reference(qkv, cu, self.scale,
                                                dtype=torch.float64 if qkv.dtype == torch.float64 else torch.float32)
        out = out.reshape(m, c).to(feats.dtype)
        out = self.proj(out)
        out = self.proj_drop(out)
        if res is not None:
            out = permute_rows(out, res.inverse_perm, res.perm)
        return x.replace(batched_features=out.to(feats.dtype))


class AllAttention(SpaceAttention):
    """``SpaceAttention`` over whole batch elements (``window_size="all"``); a ``window_size`` argument is accepted and
    ignored."""

    def __init__(self, dim: int, window_size=None, num_heads: int = 8, **kwargs):
        super().__init__(dim=dim, window_size="all", num_heads=num_heads, **kwargs)


STR2ATTN = {
    "curve": PatchAttention,
    "space": SpaceAttention,
    "all": AllAttention,
}


class SpaCeFormerBlockBase(BaseSpatialModule):
    """Sparse-conv shortcut + attention (``attn_type`` of ``STR2ATTN``) + ``FeedForward``; the subclasses choose where the
    norms sit.  ``patch_size`` is the patch length of ``"curve"`` and the window of ``"space"``."""

    def __init__(self, in_channels: int, attention_channels: int, patch_size: int, num_heads: int, kernel_size: int = 3,
                 mlp_ratio: float = 4.0, qkv_bias: bool = True, qk_scale: Optional[float] = None, attn_drop: float = 0.0,
                 proj_drop: float = 0.0, drop_path: float = 0.0, norm_layer: type = LayerNorm,
                 attn_type: Literal["curve", "space", "all"] = "curve", order: POINT_ORDERING = POINT_ORDERING.RANDOM,
                 use_rope: bool = False, rope_base: int = 250, use_checkpoint: bool = False):
        super().__init__()
        if use_checkpoint:
            raise NotImplementedError("SpaCeFormer blocks: use_checkpoint=True (gradient checkpointing) is not implemented")
        self.use_checkpoint = use_checkpoint
        self.order = order
        assert attn_type in STR2ATTN, f"Invalid attention type: {attn_type}"
        attn_block = STR2ATTN[attn_type]
        self.conv = Sequential(
            SparseConv3d(in_channels, in_channels, kernel_size=kernel_size, stride=1, bias=True),
            nn.Linear(in_channels, attention_channels),
            norm_layer(attention_channels),
        )
        self.conv_shortcut = nn.Identity() if in_channels == attention_channels else Linear(in_channels, attention_channels)
        self.norm1 = norm_layer(attention_channels)
        if attn_type == "curve":
            self.attention = attn_block(dim=attention_channels, patch_size=patch_size, num_heads=num_heads, qkv_bias=qkv_bias,
                                        qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=proj_drop, order=order,
                                        use_rope=use_rope, rope_base=rope_base)
        else:
            self.attention = attn_block(dim=attention_channels, window_size=patch_size, num_heads=num_heads,
                                        qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=proj_drop,
                                        offset=order if isinstance(order, str) else "zero", use_rope=use_rope,
                                        rope_base=rope_base)
        self.norm2 = norm_layer(attention_channels)
        self.mlp = FeedForward(dim=attention_channels, hidden_dim=int(attention_channels * mlp_ratio))
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()

    def forward(self, x: Geometry, order: Optional[Union[POINT_ORDERING, str]] = None) -> Geometry:
        if hasattr(x, "spatial_cache"):
            x.spatial_cache  # created before the first `replace`, so every geometry of this level shares one cache
        return self._forward(x, order)


class PreNormBlock(SpaCeFormerBlockBase):
    """``x + sublayer(norm(x))``."""

    def _forward(self, x: Geometry, order=None) -> Geometry:
        x = self.conv(x) + self.conv_shortcut(x)
        x = self.drop_path(self.attention(self.norm1(x), order)) + x
        x = self.drop_path(self.mlp(self.norm2(x))) + x
        return x


class PostNormBlock(SpaCeFormerBlockBase):
    """The norm behind each sublayer's residual sum."""

    def _forward(self, x: Geometry, order=None) -> Geometry:
        x = self.conv(x) + self.conv_shortcut(x)
        x = self.drop_path(self.attention(x, order)) + x
        x = self.norm1(x)
        x = self.drop_path(self.mlp(x)) + x
        x = self.norm2(x)
        return x


class StreamNormBlock(SpaCeFormerBlockBase):
    """``x = norm(x); x = sublayer(x) + x``: the residual stream itself stays normalized."""

    def _forward(self, x: Geometry, order=None) -> Geometry:
        x = self.conv(x) + self.conv_shortcut(x)
        x = self.norm1(x)
        x = self.drop_path(self.attention(x, order)) + x
        x = self.norm2(x)
        x = self.drop_path(self.mlp(x)) + x
        return x


BLOCK_REGISTRY = {
    "pre_norm": PreNormBlock,
    "post_norm": PostNormBlock,
    "stream_norm": StreamNormBlock,
}


def block_factory(block_type: Literal["pre_norm", "post_norm", "stream_norm"]) -> type:
    """The block class of ``BLOCK_REGISTRY`` under ``block_type``."""
    if block_type not in BLOCK_REGISTRY:
        raise ValueError(f"Invalid block type: {block_type!r}. Must be one of {list(BLOCK_REGISTRY)}")
    return BLOCK_REGISTRY[block_type]
