"""Dense grid geometry: lazy vertex coordinates + features in one of six memory formats (reference
`warpconvnet/geometry/types/grid.py`: ``Grid`` with the same constructor, ``from_shape``, properties, ``to_memory_format``,
``replace`` and ``to``)."""
from typing import Dict, Optional, Tuple, Union

import torch
from torch import Tensor

from warpconvnet_amd.geometry.base.geometry import Geometry
from warpconvnet_amd.geometry.coords.grid import GridCoords
from warpconvnet_amd.geometry.features.grid import (COMPRESSED_FORMATS, FORMAT_TO_AXIS, GridFeatures, GridMemoryFormat,
                                                    as_memory_format)

__all__ = ["Grid", "GridMemoryFormat", "GridFeatures", "GridCoords"]


def _channels_of(tensor: Tensor, memory_format: GridMemoryFormat, grid_shape) -> int:
    if memory_format == GridMemoryFormat.b_x_y_z_c:
        return tensor.shape[-1]
    axis = FORMAT_TO_AXIS[memory_format]
    return tensor.shape[1] if axis < 0 else tensor.shape[1] // grid_shape[axis]


class Grid(Geometry):
    def __init__(self, batched_coordinates: GridCoords, batched_features: Union[GridFeatures, Tensor],
                 memory_format: Optional[GridMemoryFormat] = None, grid_shape: Optional[Tuple[int, int, int]] = None,
                 num_channels: Optional[int] = None, **kwargs):
        if isinstance(batched_features, Tensor):
            assert memory_format is not None, "Memory format must be provided if features are a tensor"
            memory_format = as_memory_format(memory_format)
            if grid_shape is None:
                grid_shape = batched_coordinates.grid_shape
            if num_channels is None:
                num_channels = _channels_of(batched_features, memory_format, grid_shape)
            batched_features = GridFeatures(batched_features, batched_coordinates.offsets.clone(), memory_format, grid_shape,
                                            num_channels)
        else:
            assert memory_format is None or as_memory_format(memory_format) == batched_features.memory_format, (
                f"Memory format must be None or match the GridFeatures memory format: {batched_features.memory_format}. "
                f"Provided: {memory_format}")
        self.check(batched_coordinates, batched_features)
        super().__init__(batched_coordinates, batched_features, **kwargs)

    def check(self, coords: GridCoords, features: GridFeatures):
        assert coords.shape[-1] == 3
        assert tuple(coords.grid_shape) == tuple(features.grid_shape), (
            f"Grid shape ({coords.grid_shape}) must match feature grid shape ({features.grid_shape})")
        n_coords, n_feats = coords.numel() // 3, features.numel() // max(features.num_channels, 1)
        assert n_coords == n_feats, f"Number of coordinates ({n_coords}) must match number of features ({n_feats})"

    @classmethod
    def from_shape(cls, grid_shape: Tuple[int, int, int], num_channels: int,
                   memory_format: GridMemoryFormat = GridMemoryFormat.b_x_y_z_c, bounds: Optional[Tuple[Tensor, Tensor]] = None,
                   batch_size: int = 1, device: Optional[torch.device] = None, dtype: Optional[torch.dtype] = None,
                   **kwargs) -> "Grid":
        """Zero features; the coordinates stay a recipe (`GridCoords.from_shape`) until somebody reads them."""
        kwargs.pop("flatten", None)  # the reference's voxels_to_grid passes it; the coordinates are always flattened here
        coords = GridCoords.from_shape(grid_shape, bounds=bounds, batch_size=batch_size, device=device, flatten=True)
        feats = GridFeatures.create_empty(grid_shape, num_channels, batch_size=batch_size, memory_format=memory_format,
                                          device=device, dtype=dtype)
        return cls(coords, feats, memory_format, **kwargs)

    # ---- properties ---------------------------------------------------------------------------------------------------------
    @property
    def grid_features(self) -> GridFeatures:
        return self.batched_features

    @property
    def grid_coords(self) -> GridCoords:
        return self.batched_coordinates

    @property
    def grid_shape(self) -> Tuple[int, int, int]:
        return self.grid_coords.grid_shape

    @property
    def bounds(self) -> Tuple[Tensor, Tensor]:
        return self.grid_coords.bounds

    @property
    def num_channels(self) -> int:
        return self.grid_features.num_channels

    @property
    def memory_format(self) -> GridMemoryFormat:
        return self.grid_features.memory_format

    def channel_size(self, memory_format: Optional[GridMemoryFormat] = None) -> int:
        return self.grid_features.channel_size(memory_format)

    @property
    def shape(self) -> Dict[str, Union[int, Tuple[int, ...]]]:
        h, w, d = self.grid_shape
        return {"grid_shape": self.grid_shape, "batch_size": self.batch_size, "num_channels": self.num_channels,
                "total_elements": h * w * d * self.batch_size}

    def numel(self):
        return self.grid_features.numel()

    # ---- functional updates -------------------------------------------------------------------------------------------------
    def to_memory_format(self, memory_format: GridMemoryFormat) -> "Grid":
        memory_format = as_memory_format(memory_format)
        if memory_format == self.memory_format:
            return self
        return self.replace(batched_features=self.grid_features.to_memory_format(memory_format))

    def to(self, device=None, dtype: Optional[torch.dtype] = None) -> "Grid":
        if isinstance(device, torch.dtype):
            device, dtype = None, device
        if device is None:
            device = self.device
        return Grid(self.grid_coords.to(device), self.grid_features.to(device, dtype), **self._moved_extra(device))

    def _moved_extra(self, device) -> dict:
        if torch.device(device) == torch.device(self.device):
            return dict(self._extra_attributes)
        return {k: v for k, v in self._extra_attributes.items() if k not in ("_cache", "_spatial_cache")}

    def replace(self, batched_coordinates: Optional[GridCoords] = None,
                batched_features: Optional[Union[GridFeatures, Tensor]] = None, **kwargs) -> "Grid":
        """A feature tensor keeps the current memory format and grid shape; only its channel count may differ."""
        kwargs.pop("memory_format", None)
        if isinstance(batched_features, Tensor):
            fmt = self.memory_format
            want_ndim = 4 if fmt in COMPRESSED_FORMATS else 5
            if batched_features.ndim != want_ndim:
                raise ValueError(f"Unsupported feature tensor shape {tuple(batched_features.shape)} for {fmt.name}")
            batched_features = GridFeatures(batched_features, self.grid_features.offsets, fmt, self.grid_shape,
                                            _channels_of(batched_features, fmt, self.grid_shape))
        elif batched_features is not None and not isinstance(batched_features, GridFeatures):
            raise ValueError(f"Unsupported features: {type(batched_features)}")
        if "_extra_attributes" in kwargs:
            kwargs = {**kwargs.pop("_extra_attributes"), **kwargs}
        coords = batched_coordinates if batched_coordinates is not None else self.batched_coordinates
        feats = batched_features if batched_features is not None else self.batched_features
        return self.__class__(coords, feats, **{**self._extra_attributes, **kwargs})

    def _apply_feature_transform(self, fn) -> "Grid":
        return self.replace(batched_features=fn(self.grid_features.batched_tensor))
