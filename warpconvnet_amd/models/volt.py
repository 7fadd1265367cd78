"""Volt: a volume transformer for sparse-voxel semantic segmentation.

Counterpart of the reference's `warpconvnet/models/volt/volt.py`: voxels are grouped into non-overlapping ``K^3`` patches, every
patch becomes one token, a plain pre-norm transformer with axial rotary embedding and global attention per scene runs over the
tokens, and the tokens are un-embedded back to the voxels.  Constructor arguments, defaults, module tree and therefore the
``state_dict`` keys and shapes are the reference's in every configuration (pinned by `tests/golden/volt_state.json`); a
checkpoint of one loads into the other.  The reference's ``cis_cache_*`` buffers are non-persistent and do not exist here.

What is different is how a forward runs:

* the tokenizer and the detokenizer are sparse convolutions over the patch table (`nn/functional/patch_token.py`): no
  zero-filled ``[T, K^3 C]`` tensor, no ``K^3`` slots computed per token to gather one;
* one patch table, one axial rotary table and one set of HOST sequence boundaries are built per forward and shared by all
  blocks; nothing is read back from the device for them;
* attention is ``qk_prologue`` (rotation of Q and K and, for fp32 activations, the cast to fp16 the reference performs with
  ``.half()``) followed by ``flash_attn_varlen_qkvpacked``.  ``qk_norm=True`` is a per-head ``LayerNorm``: it runs as
  framework ops in front of the prologue;
* token rows follow `stride_coords` (batch-contiguous first occurrence), the reference's the sorted ``unique``: per-voxel
  outputs do not depend on it.  Negative coordinates are served (``angle = coord * freq``); the reference indexes a cache.
"""
from typing import Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor
from torch.nn.init import trunc_normal_

from warpconvnet_amd.geometry.types.voxels import Voxels
from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_qkvpacked, varlen_attention_reference
from warpconvnet_amd.nn.functional.patch_token import PatchTable, patch_embed, patch_table, patch_unembed
from warpconvnet_amd.nn.functional.qk_prologue import qk_prologue, rope_table_axial
from warpconvnet_amd.nn.modules.sparse_conv import SparseConv3d

__all__ = ["Tokenizer", "ConvBlockTokenizer", "SparseResBlock", "TokenConv", "RoPE", "RoPEAttention", "Mlp", "LayerScale",
           "DropPath", "Block", "Detokenizer", "Decoder", "Volt"]


def _bn(channels: int) -> nn.BatchNorm1d:
    return nn.BatchNorm1d(channels, eps=1e-3, momentum=0.01)


class DropPath(nn.Module):
    """Stochastic depth per row: a dropped row contributes nothing to the residual sum, the kept ones are rescaled."""

    def __init__(self, drop_prob: float = 0.0, scale_by_keep: bool = True):
        super().__init__()
        self.drop_prob, self.scale_by_keep = drop_prob, scale_by_keep

    def forward(self, x: Tensor) -> Tensor:
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1.0 - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.ndim - 1)).bernoulli_(keep)
        if keep > 0.0 and self.scale_by_keep:
            mask.div_(keep)
        return x * mask

    def extra_repr(self) -> str:
        return f"drop_prob={self.drop_prob}"


class Mlp(nn.Module):
    """Linear -> activation -> Linear (parameters ``fc1`` / ``fc2``)."""

    def __init__(self, in_features: int, hidden_features: Optional[int] = None, out_features: Optional[int] = None,
                 act_layer=nn.GELU):
        super().__init__()
        # a width that is not given (None or 0) is the input's
        widths = [in_features, hidden_features if hidden_features else in_features, out_features if out_features else in_features]
        self.fc1 = nn.Linear(widths[0], widths[1])
        self.act = act_layer()
        self.fc2 = nn.Linear(widths[1], widths[2])

    def forward(self, x: Tensor) -> Tensor:
        hidden = self.act(self.fc1(x))
        return self.fc2(hidden)


class LayerScale(nn.Module):
    """Learnable scale per channel (parameter ``gamma``)."""

    def __init__(self, dim: int, init_values: float = 1e-5, inplace: bool = False):
        super().__init__()
        self.gamma = nn.Parameter(torch.full((dim,), float(init_values)))
        self.inplace = bool(inplace)

    def forward(self, x: Tensor) -> Tensor:
        if self.inplace:
            x *= self.gamma
            return x
        return self.gamma * x


class Tokenizer(nn.Module):
    """``K^3`` patches -> one token each through ``proj`` (``nn.Linear(K^3 C, E)`` layout, `patch_embed`)."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int):
        super().__init__()
        self.kernel_size, self.out_channels = kernel_size, out_channels
        self.proj = nn.Linear(kernel_size ** 3 * in_channels, out_channels)

    def forward(self, features: Tensor, table: PatchTable) -> Tensor:
        return patch_embed(features, self.proj.weight, self.proj.bias, table)


class SparseResBlock(nn.Module):
    """conv - BN - GELU - conv - BN, plus the input, GELU; stride 1."""

    def __init__(self, dim: int, kernel_size: int = 3):
        super().__init__()
        self.conv1 = SparseConv3d(dim, dim, kernel_size=kernel_size, stride=1)
        self.bn1 = _bn(dim)
        self.conv2 = SparseConv3d(dim, dim, kernel_size=kernel_size, stride=1)
        self.bn2 = _bn(dim)
        self.act = nn.GELU()

    def forward(self, vox: Voxels) -> Voxels:
        skip = vox.feature_tensor
        x = self.conv1(vox)
        x = x.replace(batched_features=self.act(self.bn1(x.feature_tensor)))
        x = self.conv2(x)
        y = self.bn2(x.feature_tensor)
        return x.replace(batched_features=self.act(y + skip.to(y.dtype)))


class ConvBlockTokenizer(nn.Module):
    """A stride-1 sparse-conv stem (conv - BN - GELU, then ``num_blocks`` residual blocks) in front of the per-slot embed."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, stem_dim: int = 64, num_blocks: int = 2):
        super().__init__()
        self.kernel_size, self.out_channels = kernel_size, out_channels
        self.stem = SparseConv3d(in_channels, stem_dim, kernel_size=3, stride=1)
        self.bn = _bn(stem_dim)
        self.act = nn.GELU()
        self.blocks = nn.ModuleList([SparseResBlock(stem_dim) for _ in range(num_blocks)])
        self.proj = nn.Linear(kernel_size ** 3 * stem_dim, out_channels)

    def forward(self, voxels: Voxels, table: PatchTable) -> Tensor:
        x = self.stem(voxels)
        x = x.replace(batched_features=self.act(self.bn(x.feature_tensor)))
        for blk in self.blocks:
            x = blk(x)
        return patch_embed(x.feature_tensor, self.proj.weight, self.proj.bias, table)


class RoPE(nn.Module):
    """Axial rotary embedding with its own number of rotated pairs per axis: ``freqs_a = theta^(-linspace(0, 1, n_a))``.
    ``forward(coords [T, 3])`` -> the (cos, sin) table [T, sum(freq_split), 2] of `rope_table_axial`.  ``max_grid_size`` is
    accepted for the reference's signature; angles are computed, not looked up, so no grid bound applies."""

    def __init__(self, theta: float = 100.0, freq_split: Tuple[int, int, int] = (12, 12, 8),
                 max_grid_size: Tuple[int, int, int] = (1024, 1024, 512)) -> None:
        super().__init__()
        self.theta, self.freq_split, self.max_grid_size = theta, tuple(freq_split), tuple(max_grid_size)
        for name, n in zip("xyz", self.freq_split):
            self.register_buffer(f"freqs_{name}", 1.0 / theta ** torch.linspace(0, 1, n), persistent=False)

    @property
    def freqs(self) -> Tuple[Tensor, Tensor, Tensor]:
        return self.freqs_x, self.freqs_y, self.freqs_z

    def forward(self, coords: Tensor) -> Tensor:
        return rope_table_axial(coords, self.freqs)


class RoPEAttention(nn.Module):
    """Multi-head self-attention over the tokens of each scene, Q and K rotated by the axial table."""

    def __init__(self, dim: int = 768, num_heads: int = 12, qk_norm: bool = False) -> None:
        super().__init__()
        assert dim % num_heads == 0, "dim should be divisible by num_heads"
        self.num_heads, self.h_dim = num_heads, dim // num_heads
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)
        self.q_norm = nn.LayerNorm(self.h_dim) if qk_norm else nn.Identity()
        self.k_norm = nn.LayerNorm(self.h_dim) if qk_norm else nn.Identity()

    def forward(self, x: Tensor, table: Tensor, cu_seqlens: Tensor, max_seqlen: int) -> Tensor:
        n, c = x.shape
        qkv = self.qkv(x).view(n, 3, self.num_heads, self.h_dim)
        if not isinstance(self.q_norm, nn.Identity):
            q, k, v = qkv.unbind(dim=1)
            qkv = torch.stack([self.q_norm(q).to(v.dtype), self.k_norm(k).to(v.dtype), v], dim=1)
        if 2 * table.shape[1] > self.h_dim:
            raise ValueError(f"{table.shape[1]} rotated pairs do not fit head_dim {self.h_dim}")
        rot = qk_prologue(qkv, table)  # (fp32 activations leave it as fp16)
        if rot.is_cuda:
            out = flash_attn_varlen_qkvpacked(rot, cu_seqlens, max_seqlen)
        else:
            out = varlen_attention_reference(rot, cu_seqlens, dtype=torch.float32)[0].to(rot.dtype)
        return self.proj(out.reshape(n, c).to(qkv.dtype))


class TokenConv(nn.Module):
    """Stride-1 sparse convolution over the token grid."""

    def __init__(self, dim: int, kernel_size: int = 3):
        super().__init__()
        self.conv = SparseConv3d(dim, dim, kernel_size=kernel_size, stride=1)

    def forward(self, feats: Tensor, tokens: Voxels) -> Tensor:
        return self.conv(tokens.replace(batched_features=feats)).feature_tensor


class Block(nn.Module):
    def __init__(self, dim: int = 768, num_heads: int = 12, mlp_ratio: float = 4.0, init_values: Optional[float] = None,
                 qk_norm: bool = False, drop_path: float = 0.0, act_layer=nn.GELU, norm_layer=nn.LayerNorm, mlp_layer=Mlp,
                 use_conv: bool = False) -> None:
        super().__init__()
        self.use_conv = use_conv

        def scale():
            return LayerScale(dim, init_values=init_values) if init_values else nn.Identity()

        def drop():
            return DropPath(drop_path) if drop_path > 0.0 else nn.Identity()

        if use_conv:
            self.norm0 = norm_layer(dim)
            self.conv = TokenConv(dim)
            self.ls0 = scale()
            self.drop_path0 = drop()
        self.norm1 = norm_layer(dim)
        self.attn = RoPEAttention(dim=dim, num_heads=num_heads, qk_norm=qk_norm)
        self.ls1 = scale()
        self.drop_path1 = drop()
        self.norm2 = norm_layer(dim)
        self.mlp = mlp_layer(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer)
        self.ls2 = scale()
        self.drop_path2 = drop()

    def forward(self, x: Tensor, table: Tensor, cu_seqlens: Tensor, max_seqlen: int, tokens: Optional[Voxels] = None) -> Tensor:
        if self.use_conv:
            x = x + self.drop_path0(self.ls0(self.conv(self.norm0(x), tokens).to(x.dtype)))
        x = x + self.drop_path1(self.ls1(self.attn(self.norm1(x), table, cu_seqlens, max_seqlen)))
        x = x + self.drop_path2(self.ls2(self.mlp(self.norm2(x))))
        return x


class Detokenizer(nn.Module):
    """Every voxel from its token: ``proj`` is ``nn.Linear(C, K^3 C_out, bias=False)``, only the occupied slots are computed
    (`patch_unembed`); ``bias`` [C_out] is added per voxel."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int):
        super().__init__()
        self.kernel_size, self.out_channels = kernel_size, out_channels
        self.proj = nn.Linear(in_channels, kernel_size ** 3 * out_channels, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_channels))

    def forward(self, coarse_features: Tensor, table: PatchTable) -> Tensor:
        return patch_unembed(coarse_features, self.proj.weight, self.bias, table)


class Decoder(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, kernel_size: int) -> None:
        super().__init__()
        self.pre = nn.Sequential(_bn(in_channels), nn.GELU(), nn.Linear(in_channels, out_channels, bias=False), _bn(out_channels),
                                 nn.GELU())
        self.unembed = Detokenizer(out_channels, out_channels, kernel_size=kernel_size)
        self.post = nn.Sequential(_bn(out_channels), nn.GELU())

    def forward(self, x: Tensor, table: PatchTable) -> Tensor:
        return self.post(self.unembed(self.pre(x), table))


class Volt(nn.Module):
    """``Voxels -> Voxels`` with ``up_mlp_dim`` channels per voxel; `forward_tensors` takes raw ``(feat, grid_coord, batch)``."""

    def __init__(self, in_channels: int = 6, embed_dim: int = 768, depth: int = 12, num_heads: int = 12, mlp_ratio: float = 4,
                 init_values: Optional[float] = None, qk_norm: bool = False, drop_path: float = 0.3, stride: int = 5,
                 kernel_size: int = 5, up_mlp_dim: int = 256, increase_drop_path: bool = True, tokenizer_type: str = "linear",
                 conv_before_attn: bool = False):
        super().__init__()
        # (an AssertionError, as the reference raises for it)
        assert stride == kernel_size, f"Volt tokens are disjoint patches: stride ({stride}) must equal kernel_size ({kernel_size})"
        tokenizers = {"linear": Tokenizer, "convblock": ConvBlockTokenizer}
        if tokenizer_type not in tokenizers:
            raise ValueError(f"tokenizer_type must be one of {sorted(tokenizers)}, got {tokenizer_type!r}")
        self.conv_before_attn, self.tokenizer_type, self.kernel_size = conv_before_attn, tokenizer_type, kernel_size
        self.tokenizer = tokenizers[tokenizer_type](in_channels, embed_dim, kernel_size)
        rates = torch.linspace(0, drop_path, depth).tolist() if increase_drop_path else [drop_path] * depth
        self.blocks = nn.ModuleList([
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, init_values=init_values, qk_norm=qk_norm,
                  drop_path=rates[i], act_layer=nn.GELU, norm_layer=nn.LayerNorm, mlp_layer=Mlp, use_conv=conv_before_attn)
            for i in range(depth)
        ])
        self.pos_enc = RoPE()
        self.decoder = Decoder(in_channels=embed_dim, out_channels=up_mlp_dim, kernel_size=kernel_size)
        # every Linear (the tokenizer's and detokenizer's projections included): truncated normal, std 0.02, zero bias
        for linear in (m for m in self.modules() if isinstance(m, nn.Linear)):
            trunc_normal_(linear.weight, std=0.02)
            if linear.bias is not None:
                linear.bias.data.zero_()

    def _run(self, voxels: Voxels) -> Tensor:
        table = patch_table(voxels, self.kernel_size)
        if self.tokenizer_type == "convblock":
            x = self.tokenizer(voxels, table)
        else:
            x = self.tokenizer(voxels.feature_tensor, table)
        # shared by all blocks: the rotary table, the host boundaries (from the table's host offsets) and their device copy
        rope = self.pos_enc(table.coords[:, 1:])
        cu_host, max_seqlen = table.cu_seqlens()
        cu = cu_host.to(x.device) if x.is_cuda else cu_host
        tokens = None
        if self.conv_before_attn:
            tokens = Voxels(batched_coordinates=table.coords[:, 1:].contiguous(), batched_features=x, offsets=table.offsets.long())
        for blk in self.blocks:
            x = blk(x, rope, cu, max_seqlen, tokens)
        return self.decoder(x, table)

    def forward_tensors(self, feat: Tensor, grid_coord: Tensor, batch: Tensor) -> Tensor:
        """Per-voxel features [N, up_mlp_dim] from raw tensors.  ``batch`` must be non-decreasing (a batch element is a contiguous
        run of rows, as everywhere in this package)."""
        b = batch.long()
        if b.numel() > 1 and bool((b[1:] < b[:-1]).any()):
            raise ValueError("Volt.forward_tensors: batch must be non-decreasing (sort the voxels by batch index first)")
        num = int(b[-1]) + 1 if b.numel() else 0
        counts = torch.bincount(b, minlength=num)
        offsets = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).cpu()
        vox = Voxels(batched_coordinates=grid_coord.int().contiguous(), batched_features=feat, offsets=offsets)
        return self._run(vox)

    def forward(self, voxels: Voxels) -> Voxels:
        return voxels.replace(batched_features=self._run(voxels))
