"""Serialized patch attention for point / voxel transformers (reference `nn/modules/attention.py:342-583`,
`nn/modules/mlp.py:62-121`, `nn/modules/normalizations.py:70-99`).

``PatchAttention`` orders every batch element along a space-filling curve, cuts the ordered rows into patches of
``patch_size`` and runs multi-head softmax attention inside each patch through the varlen HIP kernels
(``flash_attn_varlen_qkvpacked``).  ``TransformerBlock`` = pre-norm PatchAttention + SwiGLU ``FeedForward`` with
residuals, the block of Point Transformer V3.  Constructor arguments and state-dict layouts are the reference's.

Whole-scene attention (reference `nn/modules/attention.py:33-340`): ``Attention`` on a padded batch [B, N, C] and
``SpatialFeatureAttention`` on a geometry, every point attending to every point of its own batch element.  With flash enabled
the padded batch is unpadded by the row repack kernel (`csrc/pad.hip`), qkv, ``flash_attn_varlen_qkvpacked`` and the projection
run on the packed rows, and the repack back zero-fills the padding; a geometry's concatenated rows go straight through and no
padded tensor is built.  Flash disabled, or attention dropout while training, takes the reference's masked-softmax composition.
"""
import functools
from typing import Any, Callable, List, Literal, Optional, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from warpconvnet_amd.geometry.base.geometry import Geometry
from warpconvnet_amd.geometry.coords.ops.serialization import (POINT_ORDERING, SerializationResult, encode,
                                                                to_point_ordering)
from warpconvnet_amd.geometry.features.ops.convert import cat_to_pad_tensor, pad_to_cat_tensor
from warpconvnet_amd.nn.encodings import SinusoidalEncoding
from warpconvnet_amd.nn.functional.attention import (flash_attn_varlen_qkvpacked, patch_cu_seqlens,
                                                     varlen_attention_reference)
from warpconvnet_amd.nn.modules.base_module import BaseSpatialModule
from warpconvnet_amd.nn.modules.normalizations import NormalizationBase

__all__ = ["BatchedLinear", "PatchAttention", "FeedForward", "TransformerBlock", "LayerNorm", "zero_out_points", "ZeroOutPoints",
           "offset_to_mask", "GeometryToPaddedBatch", "PaddedBatchToGeometry", "Attention", "SpatialFeatureAttention"]


class BatchedLinear(nn.Module):
    """``num_matrices`` independent linears stacked as ``weight`` [num_matrices, in, out] (Xavier-uniform), flat ``bias``
    [num_matrices * out]: [..., in] -> [..., num_matrices, out] (reference `nn/modules/mlp.py:62-121`)."""

    def __init__(self, in_features: int, out_features: int, num_matrices: int = 3, bias: bool = True):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.num_matrices = num_matrices
        self.weight = nn.Parameter(torch.empty(num_matrices, in_features, out_features))
        nn.init.xavier_uniform_(self.weight)
        if bias:
            self.bias = nn.Parameter(torch.zeros(num_matrices * out_features))
        else:
            self.register_parameter("bias", None)

    def forward(self, input: Tensor) -> Tensor:
        # one GEMM against the [in, num_matrices * out] view of the weight
        w = self.weight.to(input.dtype).permute(1, 0, 2).reshape(self.in_features, self.num_matrices * self.out_features)
        out = input @ w
        if self.bias is not None:
            out = out + self.bias.to(out.dtype)
        return out.reshape(*input.shape[:-1], self.num_matrices, self.out_features).to(input.dtype)

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, num_matrices={self.num_matrices}, "
                f"bias={self.bias is not None}")


class LayerNorm(NormalizationBase):
    """``torch.nn.LayerNorm`` over ``Geometry`` features (reference `nn/modules/normalizations.py:70-99`)."""

    def __init__(self, normalized_shape: Union[int, List[int]], eps: float = 1e-5, elementwise_affine: bool = True,
                 bias: bool = True):
        super().__init__(nn.LayerNorm(normalized_shape, eps=eps, elementwise_affine=elementwise_affine, bias=bias))


class PatchAttention(BaseSpatialModule):
    """Multi-head attention inside patches of ``patch_size`` consecutive rows of the ``order``-serialized batch elements.
    Features in fp32 run the attention core in fp16 (as the reference does); the output has the input's dtype and row
    order.  CPU tensors take ``varlen_attention_reference`` as the core.  ``use_rope`` and attention dropout are not
    implemented."""

    def __init__(self, dim: int, patch_size: int, num_heads: int = 8, qkv_bias: bool = False, qk_scale: Optional[float] = None,
                 attn_drop: float = 0.0, proj_drop: float = 0.0, order: POINT_ORDERING = POINT_ORDERING.MORTON_XYZ,
                 use_batched_qkv: bool = True, use_rope: bool = False, rope_base: int = 10_000):
        super().__init__()
        if use_rope:
            raise NotImplementedError("PatchAttention: use_rope=True (rotary embeddings) is not implemented")
        assert dim % num_heads == 0, "dim must be divisible by num_heads"
        self.patch_size = patch_size
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.use_batched_qkv = use_batched_qkv
        if use_batched_qkv:
            self.qkv = BatchedLinear(dim, dim, num_matrices=3, bias=qkv_bias)
        else:
            self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.order = order
        self.attn_drop_p = attn_drop
        self.use_rope = use_rope
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def serialization(self, x: Geometry, order: POINT_ORDERING) -> Optional[SerializationResult]:
        """The permutation that puts the rows of ``x`` in ``order`` (and its inverse); None where ``x`` is in that order
        already.  It depends on the coordinates alone, so it is kept in the geometry's spatial cache, which every geometry
        made from ``x`` with ``replace`` shares: the blocks of a level encode once per order.  ``RANDOM`` draws a new
        permutation every time and is never cached."""
        if getattr(x, "ordering", None) == order:
            return None
        cache = getattr(x, "spatial_cache", None)
        if cache is None or order == POINT_ORDERING.RANDOM:
            return encode(x.coordinate_tensor, batch_offsets=x.offsets, order=order, return_perm=True, return_inverse=True)
        key = ("serialization", order.value)
        res = cache.get(key)
        if res is None:
            res = cache[key] = encode(x.coordinate_tensor, batch_offsets=x.offsets, order=order, return_perm=True,
                                      return_inverse=True)
        return res

    def forward_ordered(self, feats: Tensor, offsets: Tensor) -> Tensor:
        """qkv, the attention inside patches of consecutive rows, and the projection on rows [M, C] that are in curve order
        already (batch element b = rows ``offsets[b] : offsets[b + 1]``); the result is in the same order."""
        m, c = feats.shape[:2]
        qkv = self.qkv(feats).reshape(m, 3, self.num_heads, c // self.num_heads)
        cu = patch_cu_seqlens(offsets, self.patch_size).to(torch.int32)
        if not qkv.is_cuda:  # CPU tensors: the per-sequence torch reference in the features' precision (no fp16 cast)
            out, _ = varlen_attention_reference(qkv, cu, self.scale,
                                                dtype=torch.float64 if qkv.dtype == torch.float64 else torch.float32)
            return self.proj_drop(self.proj(out.reshape(m, c).to(feats.dtype)))
        if qkv.dtype not in (torch.float16, torch.bfloat16):
            qkv = qkv.to(torch.float16)
        out = flash_attn_varlen_qkvpacked(qkv, cu, max_seqlen=self.patch_size, dropout_p=0.0, softmax_scale=self.scale)
        out = self.proj(out.reshape(m, c).to(feats.dtype))
        return self.proj_drop(out)

    def forward(self, x: Geometry, order: Optional[POINT_ORDERING] = None) -> Geometry:
        if self.training and self.attn_drop_p > 0.0:
            raise NotImplementedError("PatchAttention: attention dropout (attn_drop > 0 while training) is not implemented")
        order = to_point_ordering(order or self.order)
        feats = x.feature_tensor
        res = self.serialization(x, order)
        if res is not None:
            feats = feats[res.perm]
        out = self.forward_ordered(feats, x.offsets)
        if res is not None:
            out = out[res.inverse_perm]
        return x.replace(batched_features=out.to(feats.dtype))


class FeedForward(BaseSpatialModule):
    """SwiGLU: w2(silu(w1 x) * w3 x), no biases."""

    def __init__(self, dim: int, hidden_dim: int):
        super().__init__()
        self.w1 = nn.Linear(dim, hidden_dim, bias=False)
        self.w2 = nn.Linear(hidden_dim, dim, bias=False)
        self.w3 = nn.Linear(dim, hidden_dim, bias=False)

    def forward(self, x: Union[Tensor, Geometry]) -> Union[Tensor, Geometry]:
        feat = x.feature_tensor if isinstance(x, Geometry) else x
        feat = self.w2(F.silu(self.w1(feat)) * self.w3(feat))
        return x.replace(batched_features=feat) if isinstance(x, Geometry) else feat


class TransformerBlock(BaseSpatialModule):
    """h = x + attention(attention_norm(x)); out = h + feed_forward(ffn_norm(h))."""

    def __init__(self, dim: int, num_heads: int = 8, qkv_bias: bool = False, qk_scale: Optional[float] = None,
                 attn_drop: float = 0.0, proj_drop: float = 0.0, ffn_multiplier: float = 4.0, ffn_multiple_of: int = 32,
                 norm_eps: float = 1e-5, attn_fn: Optional[Callable[..., nn.Module]] = None,
                 norm_fn: Optional[Callable[..., nn.Module]] = LayerNorm, use_batched_qkv: bool = True):
        super().__init__()
        if attn_fn is None:
            attn_fn = functools.partial(PatchAttention, patch_size=1024)
        self.dim = dim
        self.attention = attn_fn(dim=dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop,
                                 proj_drop=proj_drop, use_batched_qkv=use_batched_qkv)
        hidden_dim = int((ffn_multiplier * dim + ffn_multiple_of - 1) // ffn_multiple_of * ffn_multiple_of)
        self.feed_forward = FeedForward(dim=dim, hidden_dim=hidden_dim)
        self.attention_norm = norm_fn(dim, eps=norm_eps)
        self.ffn_norm = norm_fn(dim, eps=norm_eps)

    def forward(self, x: Geometry, *args: Any, **kwargs: Any) -> Geometry:
        h = x + self.attention(self.attention_norm(x), *args, **kwargs)
        return h + self.feed_forward(self.ffn_norm(h))


# ---- whole-scene attention on padded batches ----------------------------------------------------------------------------------
def _valid_rows(num_points: Tensor, n: int, device) -> Tensor:
    """[B, N] bool: row j of element b holds a point."""
    return torch.arange(n, device=device)[None, :] < num_points.to(device)[:, None]


def zero_out_points(x: Tensor, num_points: Tensor) -> Tensor:
    """``x`` [B, N, C] with the rows from ``num_points[b]`` on set to zero (a NaN there becomes zero too; no gradient flows
    into them).  One masked fill, no loop over the batch; returns a new tensor."""
    return x.masked_fill(~_valid_rows(num_points, x.shape[1], x.device).unsqueeze(-1), 0)


class ZeroOutPoints(nn.Module):
    def forward(self, x: Tensor, num_points: Tensor) -> Tensor:
        return zero_out_points(x, num_points)


def offset_to_mask(x: Tensor, offsets: Tensor, max_num_points: int, dtype: torch.dtype = torch.bool) -> Tensor:
    """Key-validity mask [B, 1, M, M] of a padded batch: ``mask[b, 0, :, j]`` is True iff ``j`` is a point of element b."""
    b = x.shape[0]
    offsets = torch.as_tensor(offsets)
    assert b == offsets.shape[0] - 1
    if dtype != torch.bool:
        raise ValueError(f"Unsupported dtype: {dtype}")
    keys = _valid_rows(offsets[1:] - offsets[:-1], max_num_points, x.device)
    return keys[:, None, None, :].expand(b, 1, max_num_points, max_num_points)


class GeometryToPaddedBatch(BaseSpatialModule):
    """Geometry -> ``(features [B, M, C], pos_enc [B, M, C / heads] or None, mask [B, 1, M, M], num_points [B])``."""

    def __init__(self, out_channels: int, use_encoding: bool = False, num_encoding_channels: Optional[int] = None,
                 encoding_range: Optional[float] = None, num_heads: int = 1, concat_input: bool = True,
                 num_spatial_features: int = 3, out_type: Literal["nested", "cat"] = "cat"):
        super().__init__()
        self.out_type = out_type
        self.use_encoding = use_encoding
        if use_encoding:
            assert num_encoding_channels is not None, "num_encoding_channels must be provided"
            assert encoding_range is not None, "encoding_range must be provided"
            self.encoding = nn.Sequential(
                SinusoidalEncoding(num_channels=num_encoding_channels, data_range=encoding_range, concat_input=concat_input),
                nn.Linear(num_encoding_channels * num_spatial_features + (num_spatial_features if concat_input else 0),
                          out_channels // num_heads),
            )

    def encode(self, x: Geometry) -> Optional[Tensor]:
        """The positional encoding of the concatenated rows [N, C / heads], None without one."""
        return self.encoding(x.coordinate_tensor) if self.use_encoding else None

    def forward(self, x: Geometry) -> Tuple[Tensor, Optional[Tensor], Tensor, Tensor]:
        if self.out_type == "nested":
            raise NotImplementedError("GeometryToPaddedBatch: out_type='nested' is not implemented")
        offsets = x.offsets
        features = cat_to_pad_tensor(x.feature_tensor, offsets)
        pos_enc = self.encode(x)
        if pos_enc is not None:
            pos_enc = cat_to_pad_tensor(pos_enc, offsets)
        mask = offset_to_mask(features, offsets, features.shape[1])
        return features, pos_enc, mask, offsets[1:] - offsets[:-1]


class PaddedBatchToGeometry(nn.Module):
    def forward(self, x: Tensor, target: Geometry) -> Geometry:
        return target.replace(batched_features=pad_to_cat_tensor(x, target.offsets))


class Attention(nn.Module):
    """Multi-head attention of every row of a padded batch [B, N, C] over the rows of its batch element; with ``num_points``
    the padding neither attends nor is attended to, and comes out zero.  Features in fp32 run the flash core in fp16 (the
    policy of ``PatchAttention``); CPU tensors take ``varlen_attention_reference`` as the core."""

    def __init__(self, dim: int, num_heads: int = 8, qkv_bias: bool = False, qk_scale: Optional[float] = None,
                 attn_drop: float = 0.0, proj_drop: float = 0.0, enable_flash: bool = True, use_batched_qkv: bool = True):
        super().__init__()
        assert dim % num_heads == 0, "dim must be divisible by num_heads"
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.enable_flash = enable_flash
        self.use_batched_qkv = use_batched_qkv
        self.attn_drop_p = attn_drop
        if not enable_flash:
            self.attn_drop = nn.Dropout(attn_drop)
        if use_batched_qkv:
            self.qkv = BatchedLinear(dim, dim, num_matrices=3, bias=qkv_bias)
        else:
            self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def _use_flash(self) -> bool:
        return self.enable_flash and not (self.training and self.attn_drop_p > 0.0)

    def _packed_forward(self, rows: Tensor, pos: Optional[Tensor], cu: Tensor, max_seqlen: int) -> Tensor:
        """qkv, the varlen core and the projection on packed rows [T, C]; sequence s = rows ``cu[s] : cu[s + 1]``."""
        t, c = rows.shape
        if pos is not None:
            rows = rows + pos
        qkv = self.qkv(rows).reshape(t, 3, self.num_heads, c // self.num_heads)
        if not qkv.is_cuda:
            out, _ = varlen_attention_reference(qkv, cu, self.scale,
                                                dtype=torch.float64 if qkv.dtype == torch.float64 else torch.float32)
        else:
            if qkv.dtype not in (torch.float16, torch.bfloat16):
                qkv = qkv.to(torch.float16)
            out = flash_attn_varlen_qkvpacked(qkv, cu.to(torch.int32), max_seqlen=max_seqlen, dropout_p=0.0,
                                              softmax_scale=self.scale)
        return self.proj_drop(self.proj(out.reshape(t, c).to(rows.dtype)))

    def _masked_softmax_forward(self, x: Tensor, pos_enc: Optional[Tensor], mask: Optional[Tensor],
                                num_points: Optional[Tensor]) -> Tensor:
        b, n, c = x.shape
        qkv = self.qkv(x).reshape(b, n, 3, self.num_heads, c // self.num_heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        if pos_enc is not None:
            q = q + pos_enc.unsqueeze(1)
            k = k + pos_enc.unsqueeze(1)
        attn = (q @ k.transpose(-2, -1)) * self.scale
        if mask is None and num_points is not None:
            mask = _valid_rows(num_points, n, x.device)[:, None, None, :]
        if mask is not None:
            # padded keys leave the softmax; an element without points leaves rows of -inf whose softmax is NaN: those are
            # padded query rows, zeroed below, and 0 keeps the gradients finite
            attn = torch.nan_to_num(attn.masked_fill(~mask, float("-inf")).softmax(dim=-1))
        else:
            attn = attn.softmax(dim=-1)
        attn = F.dropout(attn, self.attn_drop_p, self.training)
        x = (attn @ v).transpose(1, 2).reshape(b, n, c)
        x = self.proj_drop(self.proj(x))
        return zero_out_points(x, num_points) if num_points is not None else x

    def forward(self, x: Tensor, pos_enc: Optional[Tensor] = None, mask: Optional[Tensor] = None,
                num_points: Optional[Tensor] = None) -> Tensor:
        if not self._use_flash():
            return self._masked_softmax_forward(x, pos_enc, mask, num_points)
        b, n, c = x.shape
        if num_points is None:  # every row is a point: B sequences of N rows, packed as they lie
            cu = torch.arange(b + 1, dtype=torch.int64) * n
            pos = None if pos_enc is None else pos_enc.reshape(b * n, -1)
            return self._packed_forward(x.reshape(b * n, c), pos, cu, n).reshape(b, n, c)
        # unpad, run on the packed rows, pad back with zeros (= zero_out_points).  Host num_points (what a geometry's offsets
        # give) cost no device read; device ones cost the one read of the row count.
        cu = F.pad(torch.as_tensor(num_points).to(torch.int64).cumsum(0), (1, 0))
        total = int(cu[-1])
        rows = pad_to_cat_tensor(x, cu, num_rows=total)
        pos = None if pos_enc is None else pad_to_cat_tensor(pos_enc, cu, num_rows=total)
        out = self._packed_forward(rows, pos, cu, n)
        return cat_to_pad_tensor(out, cu, max_num_points=n)


class SpatialFeatureAttention(Attention):
    """``Attention`` over the points of every batch element of a geometry, with an optional sinusoidal encoding of the
    coordinates.  On the flash path the concatenated rows are the packed layout already: no padded tensor is built."""

    def __init__(self, dim: int, num_heads: int = 8, qkv_bias: bool = False, qk_scale: Optional[float] = None,
                 attn_drop: float = 0.0, proj_drop: float = 0.0, num_encoding_channels: int = 32, encoding_range: float = 1.0,
                 use_encoding: bool = False, enable_flash: bool = True, use_batched_qkv: bool = True, **kwargs):
        super().__init__(dim, num_heads, qkv_bias, qk_scale, attn_drop, proj_drop, enable_flash, use_batched_qkv)
        self.to_attn = GeometryToPaddedBatch(dim, use_encoding=use_encoding, num_encoding_channels=num_encoding_channels,
                                             encoding_range=encoding_range, num_heads=num_heads, concat_input=True,
                                             num_spatial_features=3)
        self.from_attn = PaddedBatchToGeometry()

    def forward(self, x: Geometry) -> Geometry:
        if not self._use_flash():
            features, pos_enc, mask, num_points = self.to_attn(x)
            return self.from_attn(Attention.forward(self, features, pos_enc, mask, num_points), x)
        offsets = x.offsets.to(torch.int64)
        longest = int((offsets[1:] - offsets[:-1]).max()) if offsets.numel() > 1 else 0
        out = self._packed_forward(x.feature_tensor, self.to_attn.encode(x), offsets, longest)
        return x.replace(batched_features=out)
