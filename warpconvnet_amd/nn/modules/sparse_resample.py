"""Resampling modules over ``Voxels`` (reference `warpconvnet/nn/modules/sparse_resample.py:44-287`): same constructor and
``forward`` arguments, no parameters; the work is in `nn/functional/sparse_resample.py`."""
from typing import Literal, Optional

import torch.nn as nn

from warpconvnet_amd.geometry.types.voxels import Voxels
from warpconvnet_amd.nn.functional.sparse_resample import (
    _check_factor,
    sparse_channel_to_spatial,
    sparse_downsample,
    sparse_spatial_to_channel,
    sparse_subdivide,
    sparse_upsample,
)

__all__ = ["SparseChannel2Spatial", "SparseDownsample", "SparseSpatial2Channel", "SparseSubdivide", "SparseUpsample"]


class _Resample(nn.Module):
    def __init__(self, factor: int):
        super().__init__()
        self.factor = _check_factor(factor)

    def extra_repr(self) -> str:
        return f"factor={self.factor}"


class SparseDownsample(_Resample):
    """Mean / max of the ``factor^3`` children of every coarse cell."""

    def __init__(self, factor: int, mode: Literal["mean", "max"] = "mean"):
        super().__init__(factor)
        if mode not in ("mean", "max"):
            raise ValueError(f"mode must be 'mean' or 'max', got {mode!r}")
        self.mode = mode

    def forward(self, x: Voxels) -> Voxels:
        return sparse_downsample(x, self.factor, self.mode)


class SparseUpsample(_Resample):
    """Inverse of `SparseDownsample`: needs the paired down-sample's cache or a ``subdivision`` mask ``[N, factor^3]``."""

    def forward(self, x: Voxels, subdivision: Optional[Voxels] = None) -> Voxels:
        return sparse_upsample(x, self.factor, subdivision)


class SparseSubdivide(_Resample):
    """Repeat every voxel into all of its ``factor^3`` children (z fastest, as the reference)."""

    def forward(self, x: Voxels) -> Voxels:
        return sparse_subdivide(x, self.factor)


class SparseSpatial2Channel(_Resample):
    """Pack the ``factor^3`` children of a coarse cell into the channel axis; absent children are zeros."""

    def __init__(self, factor: int = 2):
        super().__init__(factor)

    def forward(self, x: Voxels) -> Voxels:
        return sparse_spatial_to_channel(x, self.factor)


class SparseChannel2Spatial(_Resample):
    """Inverse of `SparseSpatial2Channel`, driven by the paired cache or by a ``subdivision`` mask."""

    def __init__(self, factor: int = 2):
        super().__init__(factor)

    def forward(self, x: Voxels, subdivision: Optional[Voxels] = None) -> Voxels:
        return sparse_channel_to_spatial(x, self.factor, subdivision)
