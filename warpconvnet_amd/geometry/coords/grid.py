"""Coordinates of a dense grid, built on first use (reference `warpconvnet/geometry/coords/grid.py`: ``GridCoords`` with
``from_shape`` / ``from_tensor``, the same constructor arguments and properties).

A grid's vertex positions follow from its shape and bounds, and most consumers (the samplers of `csrc/grid.hip`, the 2-D
convolutions over the factorized formats) never look at them.  ``from_shape`` therefore stores the recipe only; the
``[B * H * W * D, 3]`` tensor appears when ``batched_tensor`` is first read.  ``to()`` of a lazy object stays lazy.  The bounds
live on the host: they are six numbers that parameterise launches.
"""
from dataclasses import dataclass, replace as _dc_replace
from typing import Optional, Tuple

import torch
from torch import Tensor

from warpconvnet_amd.geometry.base.batched import BatchedTensor
from warpconvnet_amd.geometry.base.coords import Coords
from warpconvnet_amd.geometry.coords.ops.grid import create_grid_coordinates

__all__ = ["GridCoords", "GridCoordsLazyInit"]


@dataclass
class GridCoordsLazyInit:
    batch_size: int = 1
    flatten: bool = True
    device: Optional[torch.device] = torch.device("cpu")
    dtype: torch.dtype = torch.float32

    def replace(self, **kwargs) -> "GridCoordsLazyInit":
        return _dc_replace(self, **kwargs)


class GridCoords(Coords):
    def __init__(self, batched_tensor: Tensor, offsets: Tensor, grid_shape: Tuple[int, int, int],
                 bounds: Optional[Tuple[Tensor, Tensor]] = None, lazy_init: Optional[GridCoordsLazyInit] = None):
        assert len(grid_shape) == 3, "Grid shape must be (H, W, D)"
        self.grid_shape = tuple(int(g) for g in grid_shape)
        if bounds is None:
            bounds = (torch.zeros(3), torch.ones(3))
        assert len(bounds) == 2 and tuple(bounds[0].shape) == (3,) and tuple(bounds[1].shape) == (3,), "bounds = (min [3], max [3])"
        self.bounds = (bounds[0].detach().to("cpu"), bounds[1].detach().to("cpu"))
        self._lazy_params = lazy_init
        if lazy_init is None:
            assert batched_tensor.ndim in (2, 5) and batched_tensor.shape[-1] == 3, (
                f"Tensor must have shape (B,H,W,D,3) or (N,3). Got {tuple(batched_tensor.shape)}")
            if batched_tensor.ndim == 5:
                assert tuple(batched_tensor.shape[1:4]) == self.grid_shape
            BatchedTensor.__init__(self, batched_tensor, offsets)
        else:
            BatchedTensor.__init__(self, torch.zeros((1, 3)), offsets)  # a placeholder until the first read
            del self.__dict__["batched_tensor"]

    # the coordinate tensor is an instance attribute once built; until then the lookup lands here
    def __getattr__(self, name):
        if name == "batched_tensor" and self.__dict__.get("_lazy_params") is not None:
            p = self._lazy_params
            coords, _ = create_grid_coordinates(self.grid_shape, self.bounds, p.batch_size, device=p.device, flatten=p.flatten,
                                                dtype=p.dtype)
            self.__dict__["batched_tensor"] = coords
            return coords
        raise AttributeError(name)

    @classmethod
    def from_tensor(cls, tensor: Tensor, offsets: Tensor, grid_shape: Tuple[int, int, int],
                    bounds: Optional[Tuple[Tensor, Tensor]] = None) -> "GridCoords":
        return cls(tensor, offsets, grid_shape, bounds)

    @classmethod
    def from_shape(cls, grid_shape: Tuple[int, int, int], bounds: Optional[Tuple[Tensor, Tensor]] = None, batch_size: int = 1,
                   device: Optional[torch.device] = None, flatten: bool = True) -> "GridCoords":
        cells = int(grid_shape[0]) * int(grid_shape[1]) * int(grid_shape[2])
        offsets = torch.arange(batch_size + 1, dtype=torch.long) * cells
        return cls(torch.zeros((1, 3)), offsets, grid_shape, bounds,
                   lazy_init=GridCoordsLazyInit(batch_size=batch_size, flatten=flatten, device=device))

    @property
    def is_initialized(self) -> bool:
        return "batched_tensor" in self.__dict__

    def check(self):
        if self.is_initialized:
            super().check()

    def _new(self, tensor: Tensor) -> "GridCoords":
        out = super()._new(tensor)
        out._lazy_params = None
        return out

    def to(self, device=None, dtype: Optional[torch.dtype] = None) -> "GridCoords":
        if isinstance(device, torch.dtype):
            device, dtype = None, device
        if self.is_initialized:
            return super().to(device=device, dtype=dtype)
        p = self._lazy_params
        lazy = p.replace(device=device if device is not None else p.device, dtype=dtype if dtype is not None else p.dtype)
        return self.__class__(torch.zeros((1, 3)), self.offsets, self.grid_shape, self.bounds, lazy_init=lazy)

    def half(self):
        return self.to(dtype=torch.float16)

    def float(self):
        return self.to(dtype=torch.float32)

    def double(self):
        return self.to(dtype=torch.float64)

    # ---- what can be said without the tensor ------------------------------------------------------------------------------
    @property
    def device(self):
        if self.is_initialized:
            return self.batched_tensor.device
        dev = self._lazy_params.device
        return torch.device("cpu") if dev is None else torch.device(dev)

    @property
    def dtype(self):
        return self.batched_tensor.dtype if self.is_initialized else self._lazy_params.dtype

    @property
    def shape(self):
        if self.is_initialized:
            return self.batched_tensor.shape
        h, w, d = self.grid_shape
        p = self._lazy_params
        return (p.batch_size * h * w * d, 3) if p.flatten else (p.batch_size, h, w, d, 3)

    @property
    def num_spatial_dims(self) -> int:
        return 3

    def numel(self):
        h, w, d = self.grid_shape
        return self.batch_size * h * w * d * 3

    def __len__(self) -> int:
        h, w, d = self.grid_shape
        return self.batch_size * h * w * d

    def get_spatial_indices(self, flat_indices: Tensor):
        _, w, d = self.grid_shape
        return flat_indices // (w * d), (flat_indices % (w * d)) // d, flat_indices % d

    def get_flattened_indices(self, h_indices: Tensor, w_indices: Tensor, d_indices: Tensor) -> Tensor:
        _, w, d = self.grid_shape
        return h_indices * (w * d) + w_indices * d + d_indices

    def __repr__(self) -> str:
        if not self.is_initialized:
            return f"{self.__class__.__name__}(grid_shape={self.grid_shape}, lazy=True, device={self.device})"
        return super().__repr__()

    __str__ = __repr__
