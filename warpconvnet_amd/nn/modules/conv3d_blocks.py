"""Dense 3-D convolution blocks of the TRELLIS.2 sparse-structure VAE (reference `nn/modules/conv3d_blocks.py`): the
reference's arguments, attributes and parameter names - every convolution is a plain ``nn.Conv3d``, so state dicts interchange.

On a GPU the layer-norm blocks run in one layout, channels-last, with no transposes: the norm sites are the
row kernel ``layer_norm_act(act="silu")`` on the tensor's own memory, the convolutions are ``dense_conv3d`` with bias, residual
and pixel shuffle in their store.  ``backend`` (an attribute): ``"hip"`` asks for that path, ``"torch"`` runs the reference's
composition, ``None`` (default) takes the path for a block whose convolution ``hip_dense_conv3d_preferred`` - the measured
rule of `nn/functional/dense_conv3d.py` - has ahead, and the composition for the others.  On a GPU the composition first makes
its input NCDHW-contiguous (a copy after a channels-last block, nothing otherwise): the framework's convolution was measured
2 - 10 x faster in that layout at 16^3 x 512 and 32^3 x 128, and 20 % slower at 64^3 x 32.
"""
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from warpconvnet_amd.nn.functional.dense_conv3d import (dense_conv3d, hip_dense_conv3d_preferred,
                                                         hip_dense_conv3d_supported, unshuffled_rows)
from warpconvnet_amd.nn.functional.pixel_shuffle import pixel_shuffle_3d
from warpconvnet_amd.nn.modules.normalizations import ChannelLayerNorm32, GroupNorm32
from warpconvnet_amd.nn.utils import zero_module

__all__ = ["DownsampleBlock3d", "ResBlock3d", "UpsampleBlock3d", "norm_layer_3d"]


def norm_layer_3d(norm_type: str, channels: int) -> nn.Module:
    """An fp32-internal normalisation for ``(B, C, D, H, W)`` tensors: "group" (32 groups) or "layer" (over the channels)."""
    if norm_type == "group":
        return GroupNorm32(32, channels)
    if norm_type == "layer":
        return ChannelLayerNorm32(channels)
    raise ValueError(f"Invalid norm type {norm_type}")


def _fast(module: nn.Module, x: Tensor, weight: Tensor, pixel_shuffle: int = 1, in_resblock: bool = False) -> bool:
    """Whether the block runs channels-last on the brick kernels (then every convolution in it does)."""
    if module.backend == "torch" or not x.is_cuda or x.ndim != 5 or weight.shape[1] != x.shape[1]:
        return False
    if module.backend == "hip":
        return True  # (dense_conv3d raises on what the kernels do not take)
    return hip_dense_conv3d_supported(x, weight, None, None, pixel_shuffle) and hip_dense_conv3d_preferred(x, weight, in_resblock)


def _composed(x: Tensor) -> Tensor:
    """The input of a composition path: NCDHW-contiguous on a GPU (module docstring)."""
    return x.contiguous() if x.is_cuda else x


class ResBlock3d(nn.Module):
    """Pre-norm residual block: norm -> SiLU -> conv, twice, plus the skip (a 1^3 convolution when the width changes)."""

    def __init__(self, channels: int, out_channels: Optional[int] = None, norm_type: str = "layer",
                 backend: Optional[str] = None):
        super().__init__()
        self.channels = channels
        self.out_channels = out_channels or channels
        self.backend = backend
        self.norm1 = norm_layer_3d(norm_type, channels)
        self.norm2 = norm_layer_3d(norm_type, self.out_channels)
        self.conv1 = nn.Conv3d(channels, self.out_channels, 3, padding=1)
        self.conv2 = zero_module(nn.Conv3d(self.out_channels, self.out_channels, 3, padding=1))
        self.skip_connection = nn.Conv3d(channels, self.out_channels, 1) if channels != self.out_channels else nn.Identity()

    def forward(self, x: Tensor) -> Tensor:
        if not (isinstance(self.norm1, ChannelLayerNorm32) and _fast(self, x, self.conv1.weight, in_resblock=True)):
            x = _composed(x)
            h = self.conv1(F.silu(self.norm1(x)))
            h = self.conv2(F.silu(self.norm2(h)))
            return h + self.skip_connection(x)
        x = x.contiguous(memory_format=torch.channels_last_3d)
        h = dense_conv3d(self.norm1(x, act="silu"), self.conv1.weight, self.conv1.bias, backend="hip")
        h = self.norm2(h.contiguous(memory_format=torch.channels_last_3d), act="silu")
        skip = x
        if isinstance(self.skip_connection, nn.Conv3d):
            skip = dense_conv3d(x, self.skip_connection.weight, self.skip_connection.bias, backend="hip")
        return dense_conv3d(h, self.conv2.weight, self.conv2.bias, residual=skip, backend="hip")


class DownsampleBlock3d(nn.Module):
    """2x down-sampling by a 2^3 stride-2 convolution ("conv") or average pooling ("avgpool")."""

    def __init__(self, in_channels: int, out_channels: int, mode: str = "conv", backend: Optional[str] = None):
        super().__init__()
        assert mode in ("conv", "avgpool")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.backend = backend
        if mode == "conv":
            self.conv = nn.Conv3d(in_channels, out_channels, 2, stride=2)
        else:
            assert in_channels == out_channels

    def forward(self, x: Tensor) -> Tensor:
        if not hasattr(self, "conv"):
            return F.avg_pool3d(x, 2)
        # a 2^3 stride-2 convolution is a 1^3 one on the un-shuffled tensor: channel ci * 8 + (kd * 4 + kh * 2 + kw) there
        # is weight[:, ci, kd, kh, kw], the order of weight.reshape(Cout, Cin * 8)
        w = self.conv.weight.reshape(self.out_channels, self.in_channels * 8, 1, 1, 1)
        # (backend=None: the 1^3 kernel has not been timed against the strided framework call, so it stays with that)
        if self.backend != "hip" or not x.is_cuda or x.shape[1] != self.in_channels or any(s % 2 for s in x.shape[2:]):
            return self.conv(_composed(x))
        return dense_conv3d(unshuffled_rows(x).permute(0, 4, 1, 2, 3), w, self.conv.bias, backend="hip")


class UpsampleBlock3d(nn.Module):
    """2x up-sampling by a convolution to 8x the channels and a pixel shuffle ("conv") or nearest interpolation."""

    def __init__(self, in_channels: int, out_channels: int, mode: str = "conv", backend: Optional[str] = None):
        super().__init__()
        assert mode in ("conv", "nearest")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.backend = backend
        if mode == "conv":
            self.conv = nn.Conv3d(in_channels, out_channels * 8, 3, padding=1)
        else:
            assert in_channels == out_channels

    def forward(self, x: Tensor) -> Tensor:
        if not hasattr(self, "conv"):
            return F.interpolate(x, scale_factor=2, mode="nearest")
        if not _fast(self, x, self.conv.weight, 2):
            return pixel_shuffle_3d(self.conv(_composed(x)), 2)
        return dense_conv3d(x, self.conv.weight, self.conv.bias, pixel_shuffle=2, backend="hip")
