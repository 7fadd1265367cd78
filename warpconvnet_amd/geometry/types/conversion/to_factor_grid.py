"""A point cloud pooled onto every grid of a ``FactorGrid`` (reference
`warpconvnet/geometry/types/conversion/to_factor_grid.py` / `types/factor_grid.py`: ``points_to_factor_grid``)."""
from typing import List, Literal, Optional, Tuple, Union

from torch import Tensor

from warpconvnet_amd.geometry.features.grid import GridMemoryFormat, as_memory_format
from warpconvnet_amd.geometry.types.conversion.to_grid import points_to_grid
from warpconvnet_amd.geometry.types.factor_grid import FactorGrid
from warpconvnet_amd.ops.reductions import REDUCTION_TYPES_STR

__all__ = ["points_to_factor_grid"]


def points_to_factor_grid(
    points: "Points",  # noqa: F821
    grid_shapes: List[Tuple[int, int, int]],
    memory_formats: List[Union[GridMemoryFormat, str]] = (GridMemoryFormat.b_zc_x_y, GridMemoryFormat.b_xc_y_z,
                                                          GridMemoryFormat.b_yc_x_z),
    bounds: Optional[Tuple[Tensor, Tensor]] = None,
    search_radius: Optional[float] = None,
    k: int = 8,
    search_type: Literal["radius", "knn", "voxel"] = "radius",
    reduction: REDUCTION_TYPES_STR = "mean",
) -> FactorGrid:
    """One ``points_to_grid`` per (shape, format) pair; every grid sees the same points, bounds and reduction."""
    assert len(grid_shapes) == len(memory_formats), (
        f"grid_shapes and memory_formats must have the same length: {len(grid_shapes)} != {len(memory_formats)}")
    return FactorGrid([
        points_to_grid(points, shape, memory_format=as_memory_format(fmt), bounds=bounds, search_radius=search_radius, k=k,
                       search_type=search_type, reduction=reduction)
        for shape, fmt in zip(grid_shapes, memory_formats)
    ])
