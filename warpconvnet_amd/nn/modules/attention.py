"""Serialized patch attention for point / voxel transformers (reference `nn/modules/attention.py:342-583`,
`nn/modules/mlp.py:62-121`, `nn/modules/normalizations.py:70-99`).

``PatchAttention`` orders every batch element along a space-filling curve, cuts the ordered rows into patches of
``patch_size`` and runs multi-head softmax attention inside each patch through the varlen HIP kernels
(``flash_attn_varlen_qkvpacked``).  ``TransformerBlock`` = pre-norm PatchAttention + SwiGLU ``FeedForward`` with
residuals, the block of Point Transformer V3.  Constructor arguments and state-dict layouts are the reference's.
"""
import functools
from typing import Any, Callable, List, Optional, Union

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from warpconvnet_amd.geometry.base.geometry import Geometry
from warpconvnet_amd.geometry.coords.ops.serialization import POINT_ORDERING, encode, to_point_ordering
from warpconvnet_amd.nn.functional.attention import (flash_attn_varlen_qkvpacked, patch_cu_seqlens,
                                                     varlen_attention_reference)
from warpconvnet_amd.nn.modules.base_module import BaseSpatialModule
from warpconvnet_amd.nn.modules.normalizations import NormalizationBase

__all__ = ["BatchedLinear", "PatchAttention", "FeedForward", "TransformerBlock", "LayerNorm"]


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

    def forward(self, x: Geometry, order: Optional[POINT_ORDERING] = None) -> Geometry:
        if self.training and self.attn_drop_p > 0.0:
            raise NotImplementedError("PatchAttention: attention dropout (attn_drop > 0 while training) is not implemented")
        order = to_point_ordering(order or self.order)
        feats = x.feature_tensor
        m, c = feats.shape[:2]
        inverse_perm = None
        if getattr(x, "ordering", None) != order:
            res = encode(x.coordinate_tensor, batch_offsets=x.offsets, order=order, return_perm=True, return_inverse=True)
            feats = feats[res.perm]
            inverse_perm = res.inverse_perm
        qkv = self.qkv(feats).reshape(m, 3, self.num_heads, c // self.num_heads)
        cu = patch_cu_seqlens(x.offsets, self.patch_size).to(torch.int32)
        if not qkv.is_cuda:  # CPU tensors: the per-sequence torch reference in the features' precision (no fp16 cast)
            out, _ = varlen_attention_reference(qkv, cu, self.scale,
                                                dtype=torch.float64 if qkv.dtype == torch.float64 else torch.float32)
            out = self.proj_drop(self.proj(out.reshape(m, c).to(feats.dtype)))
            if inverse_perm is not None:
                out = out[inverse_perm]
            return x.replace(batched_features=out.to(feats.dtype))
        if qkv.dtype not in (torch.float16, torch.bfloat16):
            qkv = qkv.to(torch.float16)
        out = flash_attn_varlen_qkvpacked(qkv, cu, max_seqlen=self.patch_size, dropout_p=0.0, softmax_scale=self.scale)
        out = self.proj(out.reshape(m, c).to(feats.dtype))
        out = self.proj_drop(out)
        if inverse_perm is not None:
            out = out[inverse_perm]
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
