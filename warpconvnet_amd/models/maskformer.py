"""MaskFormer: instance segmentation by learned queries (reference `warpconvnet/models/maskformer.py`).  A backbone turns the
input into per-point features; ``MaskTransformer`` refines ``num_queries`` learned query vectors per scene with decoder blocks
(self-attention among the queries, cross-attention of the queries over every point of the scene, an FFN); a class head reads the
queries, and ``MaskInnerProduct`` multiplies them with the projected point features into one [Q, N_b] mask tensor per scene.
Constructor arguments and state-dict keys are the reference's, so checkpoints interchange.

Backends (``backend="hip" | "torch" | None``, None = hip for GPU features): the torch side of ``CrossAttention`` is the
reference's padded composition on any device and dtype.  The hip side never builds the padded [B, N, C] tensor: the keys are
the geometry's concatenated rows with ``cu_k = offsets``, the queries [B * Q, H, D] with ``cu_q = arange(B + 1) * Q``, and the
core is the varlen attention (``flash_attn_varlen_kvpacked_func``, the kv-packed form of ``flash_attn_varlen_func``) with
``k_splits=0``: a hundred queries against 10^4 .. 10^5 points is the shape the split-key sweep exists for.  fp32 features run
the core in fp16 (``Attention``'s policy).  Training with ``attn_drop > 0`` and head sizes above 64 take the torch path, whatever backend is named; ``backend="hip"``
with CPU features or with a feature dtype other than fp32 / fp16 / bf16 raises (``None`` takes the torch path for those); a head
size of at most 64 that the kernels do not serve (the reference's own example: 96 / 8 = 12) is zero-padded to the next of
16, 32, 64 - exact: the zero columns add nothing to q.k, the scale stays that of the true size, the padded output columns
are dropped.  ``MaskInnerProduct`` on the hip side is one ``segment_bmm`` call whose [N, Q] result the returned tensors view.

Left out: ``MaskFormer._downsampled_queries`` - it refers to attributes the reference never defines (``query_projection``,
``pos_enc``) and nothing calls it."""
from typing import List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from warpconvnet_amd.geometry.base.geometry import Geometry
from warpconvnet_amd.geometry.features.ops.convert import cat_to_pad_tensor
from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_kvpacked_func
from warpconvnet_amd.nn.functional.bmm import hip_bmm_supported, segment_bmm
from warpconvnet_amd.nn.modules.attention import (BatchedLinear, GeometryToPaddedBatch, PaddedBatchToGeometry, _valid_rows,
                                                  zero_out_points)
from warpconvnet_amd.nn.modules.base_module import BaseSpatialModel
from warpconvnet_amd.nn.modules.mlp import Linear

__all__ = ["MaskInnerProduct", "FFNLayer", "CrossAttention", "GeometryToPaddedBatchNoMask", "SpatialFeatureCrossAttention",
           "TransformerDecoderBlock", "MaskTransformer", "MaskFormer"]

_KERNEL_HEAD_DIMS = (16, 32, 64)
_HIP_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _check_backend(backend: Optional[str]) -> Optional[str]:
    if backend not in (None, "torch", "hip"):
        raise ValueError(f"backend must be 'torch', 'hip' or None, got {backend!r}")
    return backend


class MaskInnerProduct(BaseSpatialModel):
    """``queries`` [B, Q, C] against the point features of every scene -> a list of [Q, N_b]."""

    def __init__(self, backend: Optional[str] = None):
        super().__init__()
        self.backend = _check_backend(backend)

    def forward(self, queries: Tensor, scene_feats: Geometry) -> List[Tensor]:
        feats, offsets = scene_feats.feature_tensor, scene_feats.offsets
        off = [int(o) for o in offsets.tolist()]
        weights = queries.transpose(1, 2).to(feats.dtype)                  # [B, C, Q]
        backend = self.backend
        if backend != "torch" and not (hip_bmm_supported(feats, weights) and feats.shape[0] > 0):
            if backend == "hip" and not feats.is_cuda:
                raise RuntimeError(f"backend='hip' needs GPU features, got {feats.device}; there is no CPU fallback")
            backend = "torch"      # outside bmm's channel limits (or nothing to multiply): the per-scene matmul
        if backend == "torch":
            return [queries[b].to(feats.dtype) @ feats[off[b]:off[b + 1]].T for b in range(len(off) - 1)]
        out = segment_bmm(feats, weights.contiguous(), offsets, backend="hip")   # [N, Q]
        return [out[off[b]:off[b + 1]].T for b in range(len(off) - 1)]


class FFNLayer(nn.Module):
    def __init__(self, d_model: int, dim_feedforward: int, dropout: float):
        super().__init__()
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout = nn.Dropout(dropout)
        self.activation = nn.GELU()
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm = nn.LayerNorm(d_model)

    def forward(self, x: Tensor) -> Tensor:
        x = x + self.linear2(self.dropout(self.activation(self.linear1(x))))
        return self.norm(x)


class CrossAttention(nn.Module):
    """Queries [B, Q, C] attend to the points of their own scene: a padded batch [B, N, C] with ``num_points`` (``forward``,
    the reference's signature) or concatenated rows [N, C] with ``offsets`` (``forward_rows``, what the hip side runs on)."""

    def __init__(self, dim: int, num_heads: int = 8, qkv_bias: bool = False, qk_scale: Optional[float] = None,
                 attn_drop: float = 0.0, proj_drop: float = 0.0, enable_flash: bool = False, use_batched_kv: bool = True,
                 backend: Optional[str] = None):
        super().__init__()
        assert dim % num_heads == 0, "dim must be divisible by num_heads"
        self.dim = dim
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.enable_flash = enable_flash
        self.use_batched_kv = use_batched_kv
        self.backend = _check_backend(backend)
        assert not enable_flash, "Flash attention is not supported for cross attention"   # (the reference's flag and message)
        self.attn_drop = nn.Dropout(attn_drop)
        self.q = nn.Linear(dim, dim, bias=qkv_bias)
        if use_batched_kv:
            self.kv = BatchedLinear(dim, dim, num_matrices=2, bias=qkv_bias)
        else:
            self.kv = nn.Linear(dim, dim * 2, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def _use_hip(self, feats: Tensor) -> bool:
        if self.backend == "torch":
            return False
        if self.backend == "hip" and not feats.is_cuda:
            raise RuntimeError(f"backend='hip' needs GPU features, got {feats.device}; there is no CPU fallback")
        if self.backend == "hip" and feats.dtype not in _HIP_DTYPES:
            raise TypeError(f"backend='hip' serves float32 / float16 / bfloat16 features, got {feats.dtype}")
        if self.training and self.attn_drop.p > 0.0:
            return False                                   # attention dropout: the torch composition
        if self.dim // self.num_heads > max(_KERNEL_HEAD_DIMS):
            return False
        return feats.is_cuda and feats.dtype in _HIP_DTYPES      # backend None: anything else is the torch composition

    def forward(self, q: Tensor, kv: Tensor, num_points: Tensor, pos_enc: Optional[Tensor] = None) -> Tensor:
        """The reference's padded composition."""
        B, Q, _ = q.shape
        N = kv.shape[1]
        h, d = self.num_heads, self.dim // self.num_heads
        q = self.q(q).reshape(B, Q, h, d).transpose(1, 2)                              # [B, H, Q, D]
        kv = self.kv(kv).reshape(B, N, 2, h, d).permute(2, 0, 3, 1, 4)                 # [2, B, H, N, D]
        k, v = kv[0], kv[1]
        if pos_enc is not None:
            k = k + pos_enc.unsqueeze(1)                                               # K only, broadcast over the heads
        num_points = num_points.to(q.device)
        mask = ~_valid_rows(num_points, N, q.device).view(B, 1, 1, N)
        attn = (q @ k.transpose(-2, -1)) * self.scale
        attn = attn.masked_fill(mask, torch.finfo(attn.dtype).min).softmax(dim=-1)
        attn = self.attn_drop(attn)
        x = (attn @ v).transpose(1, 2).reshape(B, Q, self.dim)
        x = self.proj_drop(self.proj(x))
        # the reference zeroes the QUERY rows by the KEY counts: a scene with fewer points than queries loses its trailing rows
        return zero_out_points(x, num_points)

    def forward_rows(self, q: Tensor, feats: Tensor, offsets: Tensor, pos: Optional[Tensor] = None) -> Tensor:
        """The same result from the concatenated rows ``feats`` [N, C] (scene b = rows ``offsets[b] : offsets[b + 1]``, host
        offsets) and their positional encoding ``pos`` [N, C / H], through the varlen HIP attention."""
        B, Q, C = q.shape
        n = feats.shape[0]
        h, d = self.num_heads, C // self.num_heads
        offsets = torch.as_tensor(offsets).to(device="cpu", dtype=torch.int64)
        num_points = offsets[1:] - offsets[:-1]
        qh = self.q(q).reshape(B * Q, h, d)
        kv = self.kv(feats).reshape(n, 2, h, d)
        if pos is not None:
            # The kernels read K and V through ONE row stride, so K cannot become a tensor of its own while V stays a slot
            # of the kv projection: the encoding is added in place into the K slot (one elementwise pass, no copy of V).
            kv[:, 0] += pos.to(kv.dtype).unsqueeze(1)
        core = kv.dtype if kv.dtype in (torch.float16, torch.bfloat16) else torch.float16
        qh, kvh = qh.to(core), kv.to(core)
        dp = next(x for x in _KERNEL_HEAD_DIMS if x >= d)
        if dp != d:                                        # zero columns: exact (module docstring)
            qh, kvh = F.pad(qh, (0, dp - d)), F.pad(kvh, (0, dp - d))
        cu_q = torch.arange(B + 1, dtype=torch.int32) * Q
        max_k = int(num_points.max()) if num_points.numel() else 0
        out = flash_attn_varlen_kvpacked_func(qh, kvh, cu_q, offsets, Q, max_k, softmax_scale=self.scale, k_splits=0)
        x = out[..., :d].reshape(B, Q, C).to(q.dtype)
        x = self.proj_drop(self.proj(x))
        return zero_out_points(x, num_points)


class GeometryToPaddedBatchNoMask(GeometryToPaddedBatch):
    """Geometry -> ``(features [B, M, C], pos_enc [B, M, C / heads] or None, num_points [B])``."""

    def encode(self, x: Geometry) -> Optional[Tensor]:
        """The positional encoding of the concatenated rows, computed in the dtype of the encoding's own parameters (fp32
        coordinates under a module cast to 16 bits)."""
        if not self.use_encoding:
            return None
        return self.encoding(x.coordinate_tensor.to(self.encoding[1].weight.dtype))

    def forward(self, x: Geometry) -> Tuple[Tensor, Optional[Tensor], Tensor]:
        if self.out_type == "nested":
            raise NotImplementedError("GeometryToPaddedBatchNoMask: out_type='nested' is not implemented")
        offsets = x.offsets
        features = cat_to_pad_tensor(x.feature_tensor, offsets)
        pos_enc = self.encode(x)
        if pos_enc is not None:
            pos_enc = cat_to_pad_tensor(pos_enc, offsets)
        return features, pos_enc, offsets[1:] - offsets[:-1]


class SpatialFeatureCrossAttention(CrossAttention):
    def __init__(self, dim: int, num_heads: int = 8, qkv_bias: bool = False, qk_scale: Optional[float] = None,
                 attn_drop: float = 0.0, proj_drop: float = 0.0, num_encoding_channels: int = 32, encoding_range: float = 1.0,
                 use_encoding: bool = True, enable_flash: bool = False, use_batched_kv: bool = True,
                 backend: Optional[str] = None, **kwargs):
        super().__init__(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop,
                         proj_drop=proj_drop, enable_flash=enable_flash, use_batched_kv=use_batched_kv, backend=backend)
        self.to_attn = GeometryToPaddedBatchNoMask(dim, use_encoding=use_encoding, num_encoding_channels=num_encoding_channels,
                                                   encoding_range=encoding_range, num_heads=num_heads, concat_input=True,
                                                   num_spatial_features=3)
        self.from_attn = PaddedBatchToGeometry()

    def forward(self, q: Tensor, kv: Geometry) -> Tensor:
        feats = kv.feature_tensor
        if self._use_hip(feats):
            pos = self.to_attn.encode(kv)
            return self.forward_rows(q, feats, kv.offsets, None if pos is None else pos.to(feats.dtype))
        features, pos_enc, num_points = self.to_attn(kv)
        return super().forward(q, features, num_points.to(features.device), pos_enc)


class TransformerDecoderBlock(nn.Module):
    def __init__(self, d_model: int, nhead: int, dim_feedforward: int, dropout: float = 0.0, backend: Optional[str] = None):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout, batch_first=True)
        self.self_attn_norm = nn.LayerNorm(d_model)
        self.cross_attn = SpatialFeatureCrossAttention(d_model, nhead, backend=backend)
        self.cross_attn_norm = nn.LayerNorm(d_model)
        self.ffn = FFNLayer(d_model, dim_feedforward, dropout)

    def forward(self, queries: Tensor, scene_feats: Geometry) -> Tensor:
        queries = self.self_attn_norm(queries + self.self_attn(queries, queries, queries)[0])
        queries = self.cross_attn_norm(queries + self.cross_attn(queries, scene_feats))
        return self.ffn(queries)


class MaskTransformer(BaseSpatialModel):
    """Decoder blocks over ``num_queries`` learned queries per scene; the query embedding is added before every block."""

    def __init__(self, hidden_dim: int, num_queries: int, num_heads: int, num_layers: int, dim_feedforward: int,
                 dropout: float = 0.0, backend: Optional[str] = None):
        super().__init__()
        self.num_queries = num_queries
        self.hidden_dim = hidden_dim
        self.layers = nn.ModuleList([TransformerDecoderBlock(hidden_dim, num_heads, dim_feedforward, dropout, backend=backend)
                                     for _ in range(num_layers)])
        self.norm = nn.LayerNorm(hidden_dim)
        self.query_embed = nn.Embedding(num_queries, hidden_dim)

    def forward(self, scene_features: Geometry) -> Tensor:
        feats = scene_features.feature_tensor
        queries = torch.zeros((scene_features.batch_size, self.num_queries, self.hidden_dim), dtype=feats.dtype,
                              device=feats.device)
        for layer in self.layers:
            queries = layer(queries + self.query_embed.weight.unsqueeze(0).to(feats.dtype), scene_features)
        return self.norm(queries)


class MaskFormer(BaseSpatialModel):
    def __init__(self, backbone: nn.Module, hidden_dim: int, num_queries: int, num_heads: int, num_decoders: int,
                 dim_feedforward: int, dropout: float, num_classes: int, backend: Optional[str] = None, **kwargs):
        super().__init__()
        self.backbone = backbone
        self.mask_features_head = Linear(hidden_dim, hidden_dim)
        self.mask_transformer = MaskTransformer(hidden_dim=hidden_dim, num_queries=num_queries, num_heads=num_heads,
                                                num_layers=num_decoders, dim_feedforward=dim_feedforward, dropout=dropout,
                                                backend=backend)
        self.class_head = nn.Linear(hidden_dim, num_classes + 1)  # +1 for background
        self.mask_inner_product = MaskInnerProduct(backend=backend)

    def forward(self, x: Geometry) -> Tuple[Tensor, List[Tensor]]:
        scene_features = self.backbone(x)
        queries = self.mask_transformer(scene_features)          # [B, Q, C]
        logits = self.class_head(queries)
        mask_features = self.mask_features_head(scene_features)
        return logits, self.mask_inner_product(queries, mask_features)
