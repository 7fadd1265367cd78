"""ConvNeXt block on ``Voxels`` (reference `nn/modules/sparse_convnext.py`: ``SparseConvNeXtBlock3d``): submanifold
convolution -> LayerNorm32 (affine) -> Linear, SiLU, zero-initialised Linear -> + x.  Constructor arguments, attribute names
and state-dict keys (``norm.*``, ``conv.*``, ``mlp.0.*``, ``mlp.2.*``) are the reference's; the norm runs through the fused
``layer_norm_act`` kernel (`nn/functional/ln_act.py`)."""
from typing import Type

import torch
import torch.nn as nn
from torch import Tensor
from torch.utils.checkpoint import checkpoint

from warpconvnet_amd.geometry.types.voxels import Voxels
from warpconvnet_amd.nn.functional import ln_act
from warpconvnet_amd.nn.modules.normalizations import LayerNorm32
from warpconvnet_amd.nn.modules.sparse_conv import SparseConv3d
from warpconvnet_amd.nn.utils import zero_module

__all__ = ["SparseConvNeXtBlock3d"]


class SparseConvNeXtBlock3d(nn.Module):
    """``x + mlp(norm(conv(x)))``; the last ``Linear`` starts at zero, so the block starts as the identity."""

    def __init__(self, channels: int, mlp_ratio: float = 4.0, kernel_size: int = 3, use_checkpoint: bool = False,
                 conv_cls: Type[nn.Module] = SparseConv3d):
        super().__init__()
        self.channels = channels
        self.use_checkpoint = use_checkpoint
        hidden = int(channels * mlp_ratio)
        self.norm = LayerNorm32(channels, elementwise_affine=True, eps=1e-6)
        self.conv = conv_cls(channels, channels, kernel_size=kernel_size)
        self.mlp = nn.Sequential(nn.Linear(channels, hidden), nn.SiLU(), zero_module(nn.Linear(hidden, channels)))

    def _body(self, x: Voxels, feats: Tensor) -> Tensor:
        h = self.conv(x.replace(batched_features=feats)).feature_tensor
        h = ln_act.layer_norm_act(h, self.norm.weight, self.norm.bias, eps=self.norm.eps, act="none")
        return self.mlp(h) + feats

    def forward(self, x: Voxels) -> Voxels:
        feats = x.feature_tensor
        if self.use_checkpoint and torch.is_grad_enabled():
            out = checkpoint(lambda f: self._body(x, f), feats, use_reentrant=False)
        else:
            out = self._body(x, feats)
        return x.replace(batched_features=out)
