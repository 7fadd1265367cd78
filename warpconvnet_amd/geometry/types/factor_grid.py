"""A group of grids in different factorized memory formats: the representation of FIGConvNet, where 3-D space is held as
several thin grids (e.g. 2 x 128 x 128, 128 x 2 x 128, 128 x 128 x 2), each folded into a 2-D image (reference
`warpconvnet/geometry/types/factor_grid.py`: ``FactorGrid`` with the same methods; ``points_to_factor_grid`` lives in
`geometry/types/conversion/to_factor_grid.py` and is re-exported here like in the reference)."""
from typing import Any, Dict, List, Optional, Tuple, Union

import torch
from torch import Tensor

from warpconvnet_amd.geometry.features.grid import COMPRESSED_FORMATS, GridMemoryFormat, as_memory_format
from warpconvnet_amd.geometry.types.grid import Grid

__all__ = ["FactorGrid", "points_to_factor_grid"]


class FactorGrid:
    def __init__(self, grids: List[Grid], **kwargs):
        assert len(grids) > 0, "At least one geometry must be provided"
        self.grids = list(grids)
        first = self.grids[0]
        for g in self.grids:
            assert g.batch_size == first.batch_size, "All geometries must have the same batch size"
            assert g.num_channels == first.num_channels, "All geometries must have the same number of channels"
            assert g.memory_format in COMPRESSED_FORMATS, f"Expected factorized format, got {g.memory_format}"
        formats = [g.memory_format for g in self.grids]
        assert len(set(formats)) == len(formats), "Each geometry must have a unique memory format"
        if "_extra_attributes" in kwargs:
            attr = kwargs.pop("_extra_attributes")
            assert isinstance(attr, dict), f"_extra_attributes must be a dictionary, got {attr}"
            kwargs = {**attr, **kwargs}
        self._extra_attributes: Dict[str, Any] = kwargs

    @classmethod
    def create_from_grid_shape(cls, grid_shapes: List[Tuple[int, int, int]], num_channels: int,
                               memory_formats: List[Union[GridMemoryFormat, str]] = ("b_zc_x_y", "b_xc_y_z", "b_yc_x_z"),
                               bounds: Optional[Tuple[Tensor, Tensor]] = None, batch_size: int = 1,
                               device: Optional[torch.device] = None, dtype: Optional[torch.dtype] = None) -> "FactorGrid":
        """Zero grids of the given shapes, one per memory format."""
        assert len(grid_shapes) == len(memory_formats), "grid_shapes and memory_formats must have the same length"
        grids = []
        for shape, fmt in zip(grid_shapes, memory_formats):
            assert isinstance(shape, tuple) and len(shape) == 3, f"grid_shape: {shape} must be a tuple of 3 integers."
            grids.append(Grid.from_shape(shape, num_channels, memory_format=as_memory_format(fmt), bounds=bounds,
                                         batch_size=batch_size, device=device, dtype=dtype))
        return cls(grids)

    @property
    def batch_size(self) -> int:
        return self.grids[0].batch_size

    @property
    def num_channels(self) -> int:
        return self.grids[0].num_channels

    @property
    def device(self) -> torch.device:
        return self.grids[0].device

    @property
    def shapes(self) -> List[Dict[str, Union[int, Tuple[int, ...]]]]:
        return [g.shape for g in self.grids]

    def to(self, device: torch.device) -> "FactorGrid":
        return FactorGrid([g.to(device) for g in self.grids])

    def get_by_format(self, memory_format: GridMemoryFormat) -> Optional[Grid]:
        memory_format = as_memory_format(memory_format)
        return next((g for g in self.grids if g.memory_format == memory_format), None)

    def __getitem__(self, idx: int) -> Grid:
        return self.grids[idx]

    def __len__(self) -> int:
        return len(self.grids)

    def __iter__(self):
        return iter(self.grids)

    def __add__(self, other: "FactorGrid") -> "FactorGrid":
        assert len(self) == len(other), f"FactorGrid lengths must match: {len(self)} != {len(other)}"
        return FactorGrid([a.replace(batched_features=a.grid_features.batched_tensor + b.grid_features.batched_tensor)
                           for a, b in zip(self.grids, other.grids)])

    def __repr__(self) -> str:
        return "FactorGrid(" + "".join(f"\n\t{g}" for g in self.grids) + "\n)"


def points_to_factor_grid(*args, **kwargs) -> FactorGrid:
    from warpconvnet_amd.geometry.types.conversion.to_factor_grid import points_to_factor_grid as impl

    return impl(*args, **kwargs)
