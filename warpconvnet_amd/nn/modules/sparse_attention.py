"""Multi-head attention over the voxels of each batch element (reference `nn/modules/sparse_dit_attention.py`):
self-attention with rotary position embeddings from the voxel coordinates and a per-head RMS norm on Q and K, and
cross-attention of the voxels to a dense context or to a second ``Voxels``.

The self forward is ``to_qkv`` -> ONE ``qk_prologue`` call (norm, rotation, cast: `csrc/qk_prologue.hip`) ->
``flash_attn_varlen_qkvpacked`` (`csrc/attn_varlen.hip`, a batch element is one sequence) -> ``to_out``.  The cross forward
is ``to_q`` / ``to_kv`` -> ``flash_attn_varlen_kvpacked_func`` or ``flash_attn_varlen_func`` (the same kernels with separate
K/V operands and lengths) -> ``to_out``.  Dropout is not implemented; ``attn_mode`` other than ``"full"`` raises here -
attention inside 3-D windows (with an optional shift of the window grid) is ``SpaceAttention`` (`nn/modules/space_attention.py`).
"""
from typing import Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from warpconvnet_amd.geometry.types.voxels import Voxels
from warpconvnet_amd.nn.functional.attention import (cross_attention_reference, flash_attn_varlen_func,
                                                     flash_attn_varlen_kvpacked_func)
from warpconvnet_amd.nn.functional.qk_prologue import (qk_prologue, qk_prologue_reference, rope_table,
                                                       sparse_scaled_dot_product_attention)
from warpconvnet_amd.nn.modules.normalizations import MultiHeadRMSNorm

__all__ = ["SparseMultiHeadAttention", "SparseMultiHeadCrossAttention", "SparseRotaryPositionEmbedder",
           "sparse_scaled_dot_product_attention"]


class SparseRotaryPositionEmbedder(nn.Module):
    """Rotary phases of the voxels' integer (x, y, z): ``freqs[i] = f0 / f1 ** (i / F)``, ``F = head_dim // 6``, positions
    as they stand (no origin, no bias).  The (cos, sin) table is cached on the input ``Voxels`` under the reference's
    key, so a stack of blocks builds it once."""

    def __init__(self, head_dim: int, dim: int = 3, rope_freq: Tuple[float, float] = (1.0, 10000.0)):
        super().__init__()
        assert head_dim % 2 == 0, "head_dim must be even"
        if dim != 3:
            raise NotImplementedError(f"SparseRotaryPositionEmbedder: dim = {dim} (only 3 spatial axes are implemented)")
        self.head_dim = head_dim
        self.dim = dim
        self.rope_freq = rope_freq
        self.freq_dim = head_dim // 2 // dim
        freqs = torch.arange(self.freq_dim, dtype=torch.float32) / max(self.freq_dim, 1)
        self.freqs = rope_freq[0] / (rope_freq[1] ** freqs)

    def cache_key(self) -> str:
        return f"rope_phase_{self.dim}d_freq{self.rope_freq[0]}-{self.rope_freq[1]}_hd{self.head_dim}"

    def table_for(self, voxels: Voxels) -> Tensor:
        """fp32 [T, 3F, 2] (cos, sin) of the voxels' coordinates, from the spatial cache when it is there."""
        cache = voxels.spatial_cache
        table = cache.get(self.cache_key())
        if table is None:
            self.freqs = self.freqs.to(voxels.coordinate_tensor.device)
            table = rope_table(voxels.coordinate_tensor, self.freqs)
            cache[self.cache_key()] = table
        return table

    def forward(self, voxels: Voxels, q_feats: Tensor, k_feats: Optional[Tensor] = None):
        """Rotate ``q_feats`` (and ``k_feats``) [T, H, D] on their own - the attention module fuses this with the norm
        and the cast instead."""
        table = self.table_for(voxels)
        pair = k_feats if k_feats is not None else q_feats
        out = qk_prologue(torch.stack([q_feats, pair, pair], dim=1), table, out_dtype=q_feats.dtype)
        if k_feats is None:
            return out[:, 0]
        return out[:, 0], out[:, 1]


class SparseMultiHeadAttention(nn.Module):
    """Self-attention over a ``Voxels`` token sequence: the reference's constructor arguments and state dict
    (``to_qkv``, ``to_out``, ``q_rms_norm.gamma``, ``k_rms_norm.gamma``)."""

    def __init__(self, channels: int, num_heads: int, ctx_channels: Optional[int] = None, type: str = "self",
                 attn_mode: str = "full", qkv_bias: bool = True, use_rope: bool = False,
                 rope_freq: Tuple[float, float] = (1.0, 10000.0), qk_rms_norm: bool = False):
        super().__init__()
        assert channels % num_heads == 0
        assert type in ("self", "cross")
        if attn_mode != "full":
            raise NotImplementedError("SparseMultiHeadAttention currently supports only attn_mode='full'")
        if type == "cross" and use_rope:
            raise ValueError("Rotary position embeddings only supported for self-attn")
        if type == "cross":
            raise NotImplementedError("SparseMultiHeadAttention: type='cross' (attention with separate K/V sequence lengths) "
                                      "is a class of its own here: use SparseMultiHeadCrossAttention")
        self.channels = channels
        self.head_dim = channels // num_heads
        self.ctx_channels = ctx_channels if ctx_channels is not None else channels
        self.num_heads = num_heads
        self._type = type
        self.attn_mode = attn_mode
        self.use_rope = use_rope
        self.qk_rms_norm = qk_rms_norm
        self.to_qkv = nn.Linear(channels, channels * 3, bias=qkv_bias)
        if qk_rms_norm:
            self.q_rms_norm = MultiHeadRMSNorm(self.head_dim, num_heads)
            self.k_rms_norm = MultiHeadRMSNorm(self.head_dim, num_heads)
        self.to_out = nn.Linear(channels, channels)
        if use_rope:
            self.rope = SparseRotaryPositionEmbedder(self.head_dim, rope_freq=rope_freq)

    def forward(self, x: Voxels, context=None) -> Voxels:
        feats = x.feature_tensor
        t = feats.shape[0]
        qkv = self.to_qkv(feats).reshape(t, 3, self.num_heads, self.head_dim)
        half = qkv.dtype in (torch.float16, torch.bfloat16)
        if self.qk_rms_norm or self.use_rope or not half:
            table = self.rope.table_for(x) if self.use_rope else None
            gq = self.q_rms_norm.gamma if self.qk_rms_norm else None
            gk = self.k_rms_norm.gamma if self.qk_rms_norm else None
            if qkv.is_cuda:
                qkv = qk_prologue(qkv, table, gq, gk)  # fp32 features leave it as fp16
            else:
                qkv = qk_prologue_reference(qkv, table, gq, gk, out_dtype=qkv.dtype)
        h = sparse_scaled_dot_product_attention(qkv, x)  # [T, H, D]
        out = self.to_out(h.reshape(t, -1).to(feats.dtype))
        return x.replace(batched_features=out.to(feats.dtype))


class SparseMultiHeadCrossAttention(nn.Module):
    """Cross-attention of a ``Voxels`` token sequence to a context: the reference's
    ``SparseMultiHeadAttention(type="cross")`` with its attribute names and state dict (``to_q``, ``to_kv``, ``to_out``,
    ``q_rms_norm.gamma``, ``k_rms_norm.gamma``).  It is a class of its own because ``SparseMultiHeadAttention`` keeps
    refusing ``type="cross"`` (its constructor's contract is pinned by the existing tests); a checkpoint of the reference's
    cross module loads into this one unchanged.

    ``context`` is a dense [B, L, ctx_channels] tensor (every batch element attends to its own L tokens) or a ``Voxels``
    (element b attends to the context's element b).  Key boundaries and ``max_seqlen_k`` come from the host offsets.  With
    ``qk_rms_norm`` Q and K pass through ``MultiHeadRMSNorm`` in plain torch.  fp32 features are cast to fp16 in front of
    the attention kernel and back after ``to_out``; CPU tensors take ``cross_attention_reference``."""

    def __init__(self, channels: int, num_heads: int, ctx_channels: Optional[int] = None, qkv_bias: bool = True,
                 qk_rms_norm: bool = False):
        super().__init__()
        assert channels % num_heads == 0
        self.channels = channels
        self.head_dim = channels // num_heads
        self.ctx_channels = ctx_channels if ctx_channels is not None else channels
        self.num_heads = num_heads
        self.qk_rms_norm = qk_rms_norm
        self.to_q = nn.Linear(channels, channels, bias=qkv_bias)
        self.to_kv = nn.Linear(self.ctx_channels, channels * 2, bias=qkv_bias)
        if qk_rms_norm:
            self.q_rms_norm = MultiHeadRMSNorm(self.head_dim, num_heads)
            self.k_rms_norm = MultiHeadRMSNorm(self.head_dim, num_heads)
        self.to_out = nn.Linear(channels, channels)

    def forward(self, x: Voxels, context) -> Voxels:
        feats = x.feature_tensor
        t, nh, hd = feats.shape[0], self.num_heads, self.head_dim
        if isinstance(context, Voxels):
            ctx = context.feature_tensor
            cu_k = context.offsets.to(device="cpu", dtype=torch.int64)
        else:
            if not isinstance(context, Tensor) or context.ndim != 3:
                raise ValueError("context must be a Voxels or a dense [B, L, ctx_channels] tensor")
            b, l = context.shape[0], context.shape[1]
            ctx = context.reshape(b * l, context.shape[2])
            cu_k = torch.arange(b + 1, dtype=torch.int64) * l
        cu_q = x.offsets.to(device="cpu", dtype=torch.int64)
        if cu_k.numel() != cu_q.numel():
            raise ValueError(f"the context has {cu_k.numel() - 1} batch elements, x has {x.batch_size}")
        lens_q, lens_k = cu_q[1:] - cu_q[:-1], cu_k[1:] - cu_k[:-1]
        max_q = int(lens_q.max()) if lens_q.numel() else 0
        max_k = int(lens_k.max()) if lens_k.numel() else 0
        q = self.to_q(feats).reshape(t, nh, hd)
        kv = self.to_kv(ctx).reshape(ctx.shape[0], 2, nh, hd)
        k = None
        if self.qk_rms_norm:
            q = self.q_rms_norm(q)
            k, v = self.k_rms_norm(kv[:, 0]), kv[:, 1]
        if not q.is_cuda:
            if k is None:
                k, v = kv[:, 0], kv[:, 1]
            h, _ = cross_attention_reference(q, k, v, cu_q, cu_k)
        else:
            kdt = q.dtype if q.dtype in (torch.float16, torch.bfloat16) else torch.float16
            cq, ck = cu_q.to(torch.int32), cu_k.to(torch.int32)
            if k is None:
                h = flash_attn_varlen_kvpacked_func(q.to(kdt), kv.to(kdt), cq, ck, max_q, max_k)
            else:
                h = flash_attn_varlen_func(q.to(kdt), k.to(kdt), v.to(kdt), cq, ck, max_q, max_k)
        out = self.to_out(h.reshape(t, -1).to(feats.dtype))
        return x.replace(batched_features=out.to(feats.dtype))
