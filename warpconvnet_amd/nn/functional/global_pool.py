"""Whole-scene operations on a geometry (reference `nn/functional/global_pool.py`): ``global_pool`` (one feature row per batch
element, `sparse_pool.py`) and ``global_scale`` (every row times its batch element's row of ``scale``)."""
from typing import Optional

from torch import Tensor

from warpconvnet_amd.geometry.base.geometry import Geometry
from warpconvnet_amd.nn.functional.segmented_arithmetics import segmented_multiply
from warpconvnet_amd.nn.functional.sparse_pool import global_pool

__all__ = ["global_pool", "global_scale"]


def global_scale(x: Geometry, scale: Tensor, backend: Optional[str] = None) -> Geometry:
    """``features[i] * scale[b]`` for every row ``i`` of batch element ``b``; ``scale`` [B, C].  Same geometry, new features."""
    if scale.shape[0] != x.batch_size:
        raise ValueError(f"scale must have one row per batch element ({x.batch_size}), got {tuple(scale.shape)}")
    return x.replace(batched_features=segmented_multiply(x.feature_tensor, scale, x.offsets, backend=backend))
