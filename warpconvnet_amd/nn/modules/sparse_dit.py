"""Sparse DiT blocks: the adaLN-modulated transformer blocks over a ``Voxels`` token sequence (reference
`nn/modules/sparse_dit.py`: ``ModulatedSparseTransformerBlock``, ``ModulatedSparseTransformerCrossBlock``,
``SparseFeedForwardNet``).

``x`` is a ``Voxels``; ``mod`` a per-batch-element conditioning tensor [B, C] ([B, 6C] with ``share_mod``).  The block is
``SparseMultiHeadAttention`` and an MLP, each behind ``LN(x) * (1 + scale[b]) + shift[b]`` and added back through
``gate[b]``.  That glue is three fused kernel calls (`nn/functional/adaln.py`) instead of the reference's two dozen
element-wise passes.  The cross block puts ``SparseMultiHeadCrossAttention`` to a ``context`` between the two, behind a plain
affine LayerNorm and added back ungated.
"""
from typing import Tuple

import torch
import torch.nn as nn
from torch import Tensor
from torch.utils.checkpoint import checkpoint

from warpconvnet_amd.geometry.types.voxels import Voxels
from warpconvnet_amd.nn.functional.adaln import adaln_gate_residual, adaln_gate_residual_modulate, adaln_modulate
from warpconvnet_amd.nn.modules.normalizations import LayerNorm32
from warpconvnet_amd.nn.modules.sparse_attention import SparseMultiHeadAttention, SparseMultiHeadCrossAttention

__all__ = ["ModulatedSparseTransformerBlock", "ModulatedSparseTransformerCrossBlock", "SparseFeedForwardNet"]


class SparseFeedForwardNet(nn.Module):
    """Linear -> GELU(tanh) -> Linear per voxel, with the reference's attribute layout (state-dict keys ``mlp.0.*``,
    ``mlp.2.*``).  Takes a ``Voxels`` or a feature tensor."""

    def __init__(self, channels: int, mlp_ratio: float = 4.0):
        super().__init__()
        self.mlp = nn.Sequential(
            nn.Linear(channels, int(channels * mlp_ratio)),
            nn.GELU(approximate="tanh"),
            nn.Linear(int(channels * mlp_ratio), channels),
        )

    def forward(self, x):
        if isinstance(x, Tensor):
            return self.mlp(x)
        return x.replace(batched_features=self.mlp(x.feature_tensor))


class ModulatedSparseTransformerBlock(nn.Module):
    """``x + gate_msa * attn(adaLN(x))``, then ``+ gate_mlp * mlp(adaLN(.))``: the reference's constructor arguments and
    state dict (``attn.*``, ``mlp.mlp.*``, ``adaLN_modulation.1.*`` or ``modulation``).  ``norm1`` / ``norm2`` are
    parameter-free ``LayerNorm32``: the fused kernels compute them (eps from ``norm1.eps`` / ``norm2.eps``)."""

    def __init__(self, channels: int, num_heads: int, mlp_ratio: float = 4.0, attn_mode: str = "full",
                 use_checkpoint: bool = False, use_rope: bool = False, rope_freq: Tuple[float, float] = (1.0, 10000.0),
                 qk_rms_norm: bool = False, qkv_bias: bool = True, share_mod: bool = False):
        super().__init__()
        self.channels = channels
        self.use_checkpoint = use_checkpoint
        self.share_mod = share_mod
        self.norm1 = LayerNorm32(channels, elementwise_affine=False, eps=1e-6)
        self.norm2 = LayerNorm32(channels, elementwise_affine=False, eps=1e-6)
        self.attn = SparseMultiHeadAttention(channels, num_heads=num_heads, attn_mode=attn_mode, qkv_bias=qkv_bias,
                                             use_rope=use_rope, rope_freq=rope_freq, qk_rms_norm=qk_rms_norm)
        self.mlp = SparseFeedForwardNet(channels, mlp_ratio=mlp_ratio)
        if not share_mod:
            self.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(channels, 6 * channels, bias=True))
        else:
            self.modulation = nn.Parameter(torch.randn(6 * channels) / channels ** 0.5)

    def _split_mod(self, mod: Tensor):
        """(shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp) as the reference forms them, cast to fp32 ONCE:
        the six [B, C] chunks stay views of one [B, 6C] tensor, which is how the kernels read them."""
        if self.share_mod:
            mod6 = (self.modulation + mod).type(mod.dtype)
        else:
            mod6 = self.adaLN_modulation(mod)
        return mod6.float().chunk(6, dim=1)

    def _body(self, x: Voxels, feats: Tensor, mod: Tensor) -> Tensor:
        shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = self._split_mod(mod)
        offsets = x.offsets
        y1 = adaln_modulate(feats, offsets, shift_msa, scale_msa, eps=self.norm1.eps)
        h1 = self.attn(x.replace(batched_features=y1)).feature_tensor
        x1, y2 = adaln_gate_residual_modulate(feats, h1, gate_msa, offsets, shift_mlp, scale_mlp, eps=self.norm2.eps)
        h2 = self.mlp(y2)
        return adaln_gate_residual(x1, h2, gate_mlp, offsets)

    def forward(self, x: Voxels, mod: Tensor) -> Voxels:
        want = 6 * self.channels if self.share_mod else self.channels
        if mod.ndim != 2 or mod.shape[0] != x.batch_size or mod.shape[1] != want:
            raise ValueError(f"mod must be [B, {want}] with B = {x.batch_size} batch elements, got {tuple(mod.shape)}")
        feats = x.feature_tensor
        if self.use_checkpoint and torch.is_grad_enabled():
            out = checkpoint(lambda f, m: self._body(x, f, m), feats, mod, use_reentrant=False)
        else:
            out = self._body(x, feats, mod)
        return x.replace(batched_features=out)


class ModulatedSparseTransformerCrossBlock(nn.Module):
    """``x + gate_msa * self_attn(adaLN(x))``, then ``+ cross_attn(norm2(.), context)``, then ``+ gate_mlp * mlp(adaLN(.))``:
    the reference's constructor arguments and state dict (``norm2.*`` - the only affine norm -, ``self_attn.*``,
    ``cross_attn.*``, ``mlp.mlp.*``, ``adaLN_modulation.1.*`` or ``modulation``).  The two modulated sites run the fused adaLN
    kernels (``norm1`` / ``norm3`` are parameter-free, eps from them); ``norm2`` is a plain ``LayerNorm32`` and the cross
    branch has no scale, shift or gate."""

    def __init__(self, channels: int, ctx_channels: int, num_heads: int, mlp_ratio: float = 4.0, attn_mode: str = "full",
                 use_checkpoint: bool = False, use_rope: bool = False, rope_freq: Tuple[float, float] = (1.0, 10000.0),
                 qk_rms_norm: bool = False, qk_rms_norm_cross: bool = False, qkv_bias: bool = True, share_mod: bool = False):
        super().__init__()
        self.channels = channels
        self.use_checkpoint = use_checkpoint
        self.share_mod = share_mod
        self.norm1 = LayerNorm32(channels, elementwise_affine=False, eps=1e-6)
        self.norm2 = LayerNorm32(channels, elementwise_affine=True, eps=1e-6)
        self.norm3 = LayerNorm32(channels, elementwise_affine=False, eps=1e-6)
        self.self_attn = SparseMultiHeadAttention(channels, num_heads=num_heads, type="self", attn_mode=attn_mode,
                                                  qkv_bias=qkv_bias, use_rope=use_rope, rope_freq=rope_freq,
                                                  qk_rms_norm=qk_rms_norm)
        self.cross_attn = SparseMultiHeadCrossAttention(channels, num_heads=num_heads, ctx_channels=ctx_channels,
                                                        qkv_bias=qkv_bias, qk_rms_norm=qk_rms_norm_cross)
        self.mlp = SparseFeedForwardNet(channels, mlp_ratio=mlp_ratio)
        if not share_mod:
            self.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(channels, 6 * channels, bias=True))
        else:
            self.modulation = nn.Parameter(torch.randn(6 * channels) / channels ** 0.5)

    _split_mod = ModulatedSparseTransformerBlock._split_mod

    def _norm2(self, x: Tensor) -> Tensor:
        """``norm2`` in fp32 whatever dtype the module was cast to (``LayerNorm32`` itself wants fp32 parameters)."""
        n = self.norm2
        return nn.functional.layer_norm(x.float(), n.normalized_shape, n.weight.float(), n.bias.float(), n.eps).to(x.dtype)

    def _body(self, x: Voxels, feats: Tensor, mod: Tensor, context) -> Tensor:
        shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = self._split_mod(mod)
        offsets = x.offsets
        y1 = adaln_modulate(feats, offsets, shift_msa, scale_msa, eps=self.norm1.eps)
        h1 = self.self_attn(x.replace(batched_features=y1)).feature_tensor
        x1 = adaln_gate_residual(feats, h1, gate_msa, offsets)
        h2 = self.cross_attn(x.replace(batched_features=self._norm2(x1)), context).feature_tensor
        x2 = x1 + h2
        y3 = adaln_modulate(x2, offsets, shift_mlp, scale_mlp, eps=self.norm3.eps)
        h3 = self.mlp(y3)
        return adaln_gate_residual(x2, h3, gate_mlp, offsets)

    def forward(self, x: Voxels, mod: Tensor, context) -> Voxels:
        want = 6 * self.channels if self.share_mod else self.channels
        if mod.ndim != 2 or mod.shape[0] != x.batch_size or mod.shape[1] != want:
            raise ValueError(f"mod must be [B, {want}] with B = {x.batch_size} batch elements, got {tuple(mod.shape)}")
        feats = x.feature_tensor
        if self.use_checkpoint and torch.is_grad_enabled():
            if isinstance(context, Tensor):
                out = checkpoint(lambda f, m, c: self._body(x, f, m, c), feats, mod, context, use_reentrant=False)
            else:
                out = checkpoint(lambda f, m, cf: self._body(x, f, m, context.replace(batched_features=cf)), feats, mod,
                                 context.feature_tensor, use_reentrant=False)
        else:
            out = self._body(x, feats, mod, context)
        return x.replace(batched_features=out)
