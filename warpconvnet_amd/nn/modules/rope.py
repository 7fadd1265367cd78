"""Rotary position embeddings from voxel coordinates (reference `nn/modules/rope.py:14-59,140-198`)."""
import math
from typing import Any

import torch
import torch.nn as nn
from torch import Tensor

from warpconvnet_amd.nn.functional.qk_prologue import fused_rope_qkv

__all__ = ["VoxelRotaryPositionalEmbeddings", "suggest_voxel_rope_base"]


def suggest_voxel_rope_base(num_heads: int, channel_size: int, max_coordinate: int, *, strategy: str = "scaled_window",
                            scale: float = 4.0, min_base: int = 8, max_base: int = 4096,
                            prefer_power_of_two: bool = True) -> int:
    """A rotation base for 3-D voxel attention over a window of ``max_coordinate`` cells (same results as the reference).
    ``scaled_window``: ``scale * window``; ``half_wave``: the base whose slowest band spans half a sinusoid over the
    window.  Clamped to ``[min_base, max_base]``, then (by default) snapped to the nearest power of two."""
    window = max(1, int(max_coordinate))
    if strategy == "half_wave":
        head_dim = channel_size // max(1, num_heads)
        bands = (head_dim // 6) * 6 // 3
        alpha = 1.0 - ((2 if bands % 2 == 0 else 1) / float(bands)) if bands > 0 else 0.0
        raw = window / math.pi
        if alpha > 1e-6:
            raw = raw ** (1.0 / alpha)
        proposed = max(2, int(round(raw)))
    else:
        proposed = int(round(scale * window))
    proposed = max(min_base, min(proposed, max_base))
    if prefer_power_of_two:
        log2_val = math.log2(proposed)
        lower, upper = 1 << int(math.floor(log2_val)), 1 << int(math.ceil(log2_val))
        proposed = lower if (proposed - lower) <= (upper - proposed) else upper
    return int(proposed)


class VoxelRotaryPositionalEmbeddings(nn.Module):
    """3-D rotary embedding of a packed qkv tensor: Q and K turn over the largest multiple of 6 channels of every head
    (``rope_dim``), the rest passes; ``dim`` = ``num_heads * head_dim``.  The reference's constructor and (empty) state
    dict: ``theta`` is a non-persistent buffer."""

    def __init__(self, dim: int, num_heads: int, base: int = 10_000) -> None:
        super().__init__()
        assert dim % num_heads == 0, f"Dimension {dim} must be divisible by num_heads {num_heads}"
        self.dim = dim
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.base = base
        self.rope_dim = (self.head_dim // 6) * 6
        self.pass_dim = self.head_dim - self.rope_dim
        if self.rope_dim > 0:
            third = self.rope_dim // 3
            self.register_buffer("theta", 1.0 / (self.base ** (torch.arange(0, third, 2).float() / third)), persistent=False)
        else:
            self.theta = None

    def forward(self, qkv: Tensor, coords: Tensor, **kwargs: Any) -> Tensor:
        """``qkv`` [M, 3, C] or [M, 3C], ``coords`` [M, 3] -> [M, 3, num_heads, head_dim]."""
        m = qkv.shape[0]
        if qkv.dim() == 2:
            qkv = qkv.view(m, 3, self.dim)
        if self.rope_dim == 0:
            return qkv.reshape(m, 3, self.num_heads, self.head_dim)
        return fused_rope_qkv(qkv, coords, self.theta, self.num_heads, self.rope_dim)
