"""``SparsePrune`` (reference `warpconvnet/nn/modules/prune.py:12-29`)."""
from torch import Tensor

from warpconvnet_amd.geometry.base.geometry import Geometry
from warpconvnet_amd.nn.functional.sparse_ops import prune_spatially_sparse_tensor
from warpconvnet_amd.nn.modules.base_module import BaseSpatialModule


class SparsePrune(BaseSpatialModule):
    """Keep the rows of ``spatial_tensor`` where ``mask`` (aligned with its coordinates) is true."""

    def forward(self, spatial_tensor: Geometry, mask: Tensor) -> Geometry:
        return prune_spatially_sparse_tensor(spatial_tensor, mask)
