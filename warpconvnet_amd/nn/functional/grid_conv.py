"""3-D convolution over a ``Grid`` (reference `warpconvnet/nn/functional/grid_conv.py`: ``grid_conv`` with the same
arguments).  A wrapper on the framework's ``F.conv3d`` over ``b_c_z_x_y``; a grid in another memory format is converted with a
warning.  The grid shape of the result is read off the output tensor, so stride, padding and dilation need no formula here."""
import warnings
from typing import Optional, Tuple, Union

import torch.nn.functional as F
from torch import Tensor

from warpconvnet_amd.geometry.coords.grid import GridCoords
from warpconvnet_amd.geometry.features.grid import GridMemoryFormat
from warpconvnet_amd.geometry.types.grid import Grid

__all__ = ["grid_conv"]


def grid_conv(grid: Grid, weight: Tensor, stride: Union[int, Tuple[int, ...]] = 1, padding: Union[int, Tuple[int, ...]] = 0,
              dilation: Union[int, Tuple[int, ...]] = 1, bias: Optional[Tensor] = None) -> Grid:
    """``weight`` [C_out, C_in, D, H, W] over the tensor axes (z, x, y); ``bias`` a tensor or ``None``."""
    if grid.memory_format != GridMemoryFormat.b_c_z_x_y:
        warnings.warn(f"Input grid memory format is {grid.memory_format}, converting to {GridMemoryFormat.b_c_z_x_y}")
        grid = grid.to_memory_format(GridMemoryFormat.b_c_z_x_y)
    out = F.conv3d(grid.grid_features.batched_tensor, weight, bias, stride, padding, dilation)
    d, h, w = (int(s) for s in out.shape[2:])
    coords = GridCoords.from_shape((h, w, d), bounds=grid.bounds, batch_size=grid.batch_size, device=grid.device)
    return Grid(coords, out, memory_format=GridMemoryFormat.b_c_z_x_y)
