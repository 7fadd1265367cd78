"""Pooling modules over ``Voxels`` and the points -> voxels -> points wrapper (reference
`warpconvnet/nn/modules/sparse_pool.py:20-203`)."""
from typing import Literal, Union

from warpconvnet_amd.geometry.base.geometry import Geometry
from warpconvnet_amd.geometry.types.points import Points
from warpconvnet_amd.geometry.types.voxels import Voxels
from warpconvnet_amd.nn.functional.point_pool import point_pool
from warpconvnet_amd.nn.functional.point_unpool import point_unpool
from warpconvnet_amd.nn.functional.sparse_pool import global_pool, sparse_reduce, sparse_unpool
from warpconvnet_amd.nn.modules.base_module import BaseSpatialModule
from warpconvnet_amd.ops.reductions import REDUCTIONS


class SparsePool(BaseSpatialModule):
    """Reduce the features of every ``kernel_size`` window placed with ``stride`` (``max`` / ``min`` / ``mean`` / ``sum``)."""

    def __init__(self, kernel_size: int, stride: int, reduce: Literal["max", "min", "mean", "sum"] = "max"):
        super().__init__()
        self.kernel_size, self.stride, self.reduce = kernel_size, stride, reduce

    def __repr__(self):
        return f"{self.__class__.__name__}(kernel_size={self.kernel_size}, stride={self.stride}, reduce={self.reduce})"

    def forward(self, st: Voxels) -> Voxels:
        return sparse_reduce(st, self.kernel_size, self.stride, self.reduce)


class SparseMaxPool(SparsePool):
    def __init__(self, kernel_size: int, stride: int):
        super().__init__(kernel_size, stride, "max")


class SparseMinPool(SparsePool):
    def __init__(self, kernel_size: int, stride: int):
        super().__init__(kernel_size, stride, "min")


class GlobalPool(BaseSpatialModule):
    """One feature row per batch element."""

    def __init__(self, reduce: Literal["min", "max", "mean", "sum"] = "max"):
        super().__init__()
        self.reduce = reduce

    def forward(self, x: Geometry) -> Geometry:
        return global_pool(x, self.reduce)


class SparseUnpool(BaseSpatialModule):
    """Copy pooled features back onto the fine voxels (optionally concatenated with the fine features)."""

    def __init__(self, kernel_size: int, stride: int, concat_unpooled_st: bool = True):
        super().__init__()
        self.kernel_size, self.stride, self.concat_unpooled_st = kernel_size, stride, concat_unpooled_st

    def forward(self, st: Voxels, unpooled_st: Voxels) -> Voxels:
        return sparse_unpool(st, unpooled_st, self.kernel_size, self.stride, self.concat_unpooled_st)


class PointToVoxel(BaseSpatialModule):
    """Pool points onto voxels of edge ``voxel_size``, run ``inner_module`` on the ``Voxels`` and unpool its output back
    onto the points, followed by the points' own features when ``concat_unpooled_pc`` (reference
    `nn/modules/sparse_pool.py:140-189`).  One voxel map serves both directions."""

    def __init__(self, inner_module: BaseSpatialModule, voxel_size: float, reduction: Union[REDUCTIONS, str] = REDUCTIONS.MEAN,
                 unique_method: str = "morton", concat_unpooled_pc: bool = True):
        super().__init__()
        self.inner_module = inner_module
        self.voxel_size = voxel_size
        self.reduction = reduction
        self.concat_unpooled_pc = concat_unpooled_pc
        self.unique_method = unique_method

    def forward(self, pc: Points) -> Points:
        st, to_unique = point_pool(pc, reduction=self.reduction, downsample_voxel_size=self.voxel_size, return_type="voxel",
                                   return_to_unique=True, unique_method=self.unique_method)
        out_st = self.inner_module(st)
        assert isinstance(out_st, Voxels), "Output of inner module must be a Voxels"
        return point_unpool(out_st.to_point(self.voxel_size), pc, concat_unpooled_pc=self.concat_unpooled_pc,
                            to_unique=to_unique)


class PointToSparseWrapper(PointToVoxel):
    """Deprecated alias for ``PointToVoxel``."""

    def __init__(self, *args, **kwargs):
        import warnings

        warnings.warn("PointToSparseWrapper is deprecated; use PointToVoxel instead.", DeprecationWarning, stacklevel=2)
        super().__init__(*args, **kwargs)
