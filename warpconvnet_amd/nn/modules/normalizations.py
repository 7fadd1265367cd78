"""Normalisation modules over ``Geometry`` features (reference `nn/modules/normalizations.py:30-68`)."""
from typing import Union

import torch
import torch.nn as nn
from torch import Tensor

from warpconvnet_amd.geometry.base.geometry import Geometry
from warpconvnet_amd.nn.functional.normalizations import (batch_norm_module_forward, hip_batch_norm_supported,
                                                          segmented_layer_norm)
from warpconvnet_amd.nn.modules.base_module import BaseSpatialModule


def apply_batch_norm(norm: nn.modules.batchnorm._BatchNorm, x: Tensor, relu: bool = False) -> Tensor:
    """BatchNorm (+ ReLU) on a feature tensor: HIP kernels for 2-D GPU tensors, the framework's module otherwise."""
    if hip_batch_norm_supported(x) and type(norm) in (nn.BatchNorm1d,):
        return batch_norm_module_forward(norm, x, relu)
    y = norm(x)
    return nn.functional.relu(y) if relu else y


class NormalizationBase(BaseSpatialModule):
    """Applies a normalisation module to the feature tensor of a geometry."""

    def __init__(self, norm: nn.Module):
        super().__init__()
        self.norm = norm

    def __repr__(self):
        return f"{self.__class__.__name__}({self.norm})"

    def forward(self, input: Union[Geometry, Tensor]):
        feats = input.feature_tensor if isinstance(input, Geometry) else input
        out = apply_batch_norm(self.norm, feats) if isinstance(self.norm, nn.BatchNorm1d) else self.norm(feats)
        return input.replace(batched_features=out) if isinstance(input, Geometry) else out


class BatchNorm(NormalizationBase):
    """``torch.nn.BatchNorm1d`` over ``Geometry`` features (same parameters / state dict as the reference's module)."""

    def __init__(self, num_features: int, eps: float = 1e-5, momentum: float = 0.1):
        super().__init__(nn.BatchNorm1d(num_features, eps=eps, momentum=momentum))


class MultiHeadRMSNorm(nn.Module):
    """RMS norm per attention head (reference `nn/modules/normalizations.py:226-245`): ``x`` [..., heads, dim] ->
    ``x / max(|x|_2, 1e-12) * gamma * sqrt(dim)`` in fp32, returned in the input dtype.  Called on its own this is plain
    torch; ``SparseMultiHeadAttention`` hands ``gamma`` to the fused Q/K prologue kernel instead."""

    def __init__(self, dim: int, heads: int):
        super().__init__()
        self.scale = dim ** 0.5
        self.gamma = nn.Parameter(torch.ones(heads, dim))

    def forward(self, x: Tensor) -> Tensor:
        return (nn.functional.normalize(x.float(), dim=-1) * self.gamma * self.scale).to(x.dtype)


class SegmentedLayerNorm(nn.LayerNorm):
    """Layer normalisation over the rows of every batch element of a geometry, per channel, with ``nn.LayerNorm``'s
    ``weight`` / ``bias`` [channels] (reference `nn/modules/normalizations.py:102-141`).  ``detach_stats=True`` is the
    reference's backward (mean and std are constants), ``False`` the true gradient."""

    def __init__(self, channels: int, eps: float = 1e-5, elementwise_affine: bool = True, bias: bool = True,
                 detach_stats: bool = True):
        super().__init__([channels], eps=eps, elementwise_affine=elementwise_affine, bias=bias)
        self.detach_stats = detach_stats

    def forward(self, x: Geometry):
        assert isinstance(x, Geometry), f"SegmentedLayerNorm only works for Geometry, got {type(x)}"
        out = segmented_layer_norm(x.feature_tensor, x.offsets, gamma=self.weight, beta=self.bias, eps=self.eps,
                                   detach_stats=self.detach_stats)
        return x.replace(batched_features=out)

    def __repr__(self):
        shape = None if self.weight is None else self.weight.shape
        return f"{self.__class__.__name__}({shape}, eps={self.eps}, elementwise_affine={self.elementwise_affine})"


class LayerNorm32(nn.LayerNorm):
    """``torch.nn.LayerNorm`` that always computes in fp32, then casts back (reference
    `nn/modules/normalizations.py:196-201`).  Plain torch; ``ModulatedSparseTransformerBlock`` keeps its two as attributes
    and runs their math inside the fused adaLN kernels."""

    def forward(self, x: Tensor) -> Tensor:
        return super().forward(x.float()).to(x.dtype)
