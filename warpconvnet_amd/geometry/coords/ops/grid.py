"""Vertex coordinates of a regular grid (reference `warpconvnet/geometry/coords/ops/grid.py`: same names and arguments).

The vertices of an axis are ``linspace(min, max, res)``: the first and the last vertex sit ON the bounds (align-corners), which
is the convention the trilinear sampler (`csrc/grid.hip`) interpolates in.
"""
from typing import Optional, Tuple

import torch
from torch import Tensor

__all__ = ["create_grid_coordinates", "strided_grid_coords"]


def create_grid_coordinates(
    grid_shape: Tuple[int, int, int],
    bounds: Optional[Tuple[Tensor, Tensor]] = None,
    batch_size: int = 1,
    device: Optional[torch.device] = None,
    flatten: bool = True,
    dtype: torch.dtype = torch.float32,
) -> Tuple[Tensor, Tensor]:
    """``(coords, offsets)``: ``coords`` [B * H * W * D, 3] (``flatten``) or [B, H, W, D, 3], z fastest; ``offsets`` [B + 1] on
    the host.  ``bounds=None`` is the unit cube."""
    if bounds is None:
        lo, hi = torch.zeros(3, device=device), torch.ones(3, device=device)
    else:
        lo, hi = bounds[0].to(device), bounds[1].to(device)
    axes = [lo[a] + torch.linspace(0, 1, int(grid_shape[a]), device=device, dtype=dtype) * (hi[a] - lo[a]) for a in range(3)]
    coords = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1)
    if batch_size > 1:
        coords = coords.unsqueeze(0).expand(batch_size, -1, -1, -1, -1)  # a view until it is flattened
    if flatten:
        coords = coords.reshape(-1, 3)
    cells = int(grid_shape[0]) * int(grid_shape[1]) * int(grid_shape[2])
    offsets = torch.arange(batch_size + 1, dtype=torch.long) * cells
    return coords, offsets


def strided_grid_coords(vertices: Tensor, curr_grid_shape: Tuple[int, int, int], grid_shape: Tuple[int, int, int],
                        batch_size: int) -> Tensor:
    """The vertices [B * H * W * D, 3] of ``curr_grid_shape`` at the coarser ``grid_shape``: every stride-th vertex when the
    shapes divide, otherwise a new grid over the same bounding box."""
    curr_grid_shape, grid_shape = tuple(curr_grid_shape), tuple(grid_shape)
    if curr_grid_shape == grid_shape:
        return vertices
    v5 = vertices.reshape(batch_size, *curr_grid_shape, 3)
    if all(c % g == 0 for c, g in zip(curr_grid_shape, grid_shape)):
        sx, sy, sz = (c // g for c, g in zip(curr_grid_shape, grid_shape))
        return v5[:, ::sx, ::sy, ::sz, :].reshape(-1, 3)
    flat = v5.reshape(-1, 3)
    new_coords, _ = create_grid_coordinates(grid_shape, (flat.min(dim=0)[0], flat.max(dim=0)[0]), batch_size=batch_size,
                                            device=vertices.device)
    return new_coords
