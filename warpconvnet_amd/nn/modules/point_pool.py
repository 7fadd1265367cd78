"""Point pooling / unpooling modules (reference `warpconvnet/nn/modules/point_pool.py:23-201`)."""
from typing import Optional, Union

from warpconvnet_amd.geometry.types.points import Points
from warpconvnet_amd.nn.functional.point_pool import point_pool
from warpconvnet_amd.nn.functional.point_unpool import FEATURE_UNPOOLING_MODE, point_unpool
from warpconvnet_amd.nn.modules.base_module import BaseSpatialModule
from warpconvnet_amd.ops.reductions import REDUCTIONS

__all__ = ["PointPoolBase", "PointMaxPool", "PointAvgPool", "PointSumPool", "PointUnpool"]


class PointPoolBase(BaseSpatialModule):
    """``point_pool`` as a module.  ``return_type`` is ``"point"`` or ``"sparse"`` (``"voxel"``); the misspelt
    ``avereage_pooled_coordinates`` is the reference's argument name.  ``sample_method`` ("random" / "fps") picks the
    survivors of ``downsample_max_num_points``."""

    def __init__(
        self,
        reduction: Union[str, REDUCTIONS] = REDUCTIONS.MAX,
        downsample_max_num_points: Optional[int] = None,
        downsample_voxel_size: Optional[float] = None,
        return_type: str = "point",
        unique_method: str = "torch",
        avereage_pooled_coordinates: bool = False,
        return_neighbor_search_result: bool = False,
        sample_method: str = "random",
    ):
        super().__init__()
        if isinstance(reduction, str):
            reduction = REDUCTIONS(reduction)
        self.reduction = reduction
        self.downsample_max_num_points = downsample_max_num_points
        self.downsample_voxel_size = downsample_voxel_size
        self.return_type = return_type
        self.return_neighbor_search_result = return_neighbor_search_result
        self.unique_method = unique_method
        self.avereage_pooled_coordinates = avereage_pooled_coordinates
        self.sample_method = sample_method

    def forward(self, pc: Points):
        return point_pool(
            pc=pc,
            reduction=self.reduction,
            downsample_max_num_points=self.downsample_max_num_points,
            downsample_voxel_size=self.downsample_voxel_size,
            return_type=self.return_type,
            return_neighbor_search_result=self.return_neighbor_search_result,
            unique_method=self.unique_method,
            average_pooled_coordinates=self.avereage_pooled_coordinates,
            sample_method=self.sample_method,
        )


class _FixedReductionPool(PointPoolBase):
    REDUCTION: REDUCTIONS

    def __init__(
        self,
        downsample_max_num_points: Optional[int] = None,
        downsample_voxel_size: Optional[float] = None,
        return_type: str = "point",
        return_neighbor_search_result: bool = False,
        sample_method: str = "random",
    ):
        super().__init__(
            reduction=self.REDUCTION,
            downsample_max_num_points=downsample_max_num_points,
            downsample_voxel_size=downsample_voxel_size,
            return_type=return_type,
            return_neighbor_search_result=return_neighbor_search_result,
            sample_method=sample_method,
        )


class PointMaxPool(_FixedReductionPool):
    REDUCTION = REDUCTIONS.MAX


class PointAvgPool(_FixedReductionPool):
    REDUCTION = REDUCTIONS.MEAN


class PointSumPool(_FixedReductionPool):
    REDUCTION = REDUCTIONS.SUM


class PointUnpool(BaseSpatialModule):
    """``point_unpool`` without a map: every point of ``unpooled_pc`` takes its nearest pooled point's features."""

    def __init__(self, unpooling_mode: Union[str, FEATURE_UNPOOLING_MODE] = FEATURE_UNPOOLING_MODE.REPEAT,
                 concat_unpooled_pc: bool = False):
        super().__init__()
        if isinstance(unpooling_mode, str):
            unpooling_mode = FEATURE_UNPOOLING_MODE(unpooling_mode)
        self.unpooling_mode = unpooling_mode
        self.concat_unpooled_pc = concat_unpooled_pc

    def forward(self, pooled_pc: Points, unpooled_pc: Points):
        return point_unpool(pooled_pc=pooled_pc, unpooled_pc=unpooled_pc, unpooling_mode=self.unpooling_mode,
                            concat_unpooled_pc=self.concat_unpooled_pc)
