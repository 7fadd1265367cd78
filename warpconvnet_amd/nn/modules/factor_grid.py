"""Modules over ``FactorGrid`` geometries (reference `warpconvnet/nn/modules/factor_grid.py`: the same class names,
constructor arguments and parameter names, so ``state_dict``s interchange).

``FactorGridToPoint`` brings the grids back to the points: every grid is interpolated trilinearly at the point positions
(`grid_sample_points`: on the GPU one strided launch per grid writing side by side into one tensor, ragged batches allowed),
joined with the point features and the position relative to the box centre (raw or sinusoidally embedded) and passed through
``combine_mlp``.  ``PointToFactorGrid`` is ``points_to_factor_grid`` with the box and search settings held by the module.

``FactorGridProjection`` is the first of FIGConvNet's convolution blocks: one ``Conv2d`` - ``norm`` - ``activation`` per grid
over the folded 2-D image, channel dim ``C * compressed_dim`` (the framework's convolution).  Two defects of the reference
are not copied: its ``forward`` hands a ``Grid`` to an ``nn.Sequential`` of tensor ops and raises - here the block runs on the
feature tensor and the grid is rebuilt; and with image sizes that ``stride`` does not divide it would build a ``Grid`` whose
shape disagrees with its features - here that raises a ``ValueError`` naming the shapes.  ``FactorGridGlobalConv`` and the
model are not part of this module.
"""
from typing import List, Literal, Optional, Tuple, Type

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from warpconvnet_amd.geometry.features.grid import COMPRESSED_FORMATS, FORMAT_TO_AXIS, GridMemoryFormat, as_memory_format
from warpconvnet_amd.geometry.types.factor_grid import FactorGrid
from warpconvnet_amd.geometry.types.points import Points
from warpconvnet_amd.nn.functional.encodings import get_freqs, sinusoidal_encoding
from warpconvnet_amd.nn.functional.factor_grid import (factor_grid_cat, factor_grid_intra_communication, factor_grid_pool,
                                                       factor_grid_transform)
from warpconvnet_amd.nn.functional.grid_sample import grid_sample_points
from warpconvnet_amd.nn.modules.base_module import BaseSpatialModule

__all__ = ["FactorGridTransform", "FactorGridCat", "FactorGridPool", "FactorGridIntraCommunication", "FactorGridPadToMatch",
           "FactorGridToPoint", "PointToFactorGrid", "FactorGridProjection"]


class FactorGridTransform(BaseSpatialModule):
    """``transform`` (a module over feature tensors) applied to every grid."""

    def __init__(self, transform: nn.Module, in_place: bool = True) -> None:
        super().__init__()
        self.transform = transform
        self.in_place = in_place

    def forward(self, factor_grid: FactorGrid) -> FactorGrid:
        return factor_grid_transform(factor_grid, self.transform, self.in_place)


class FactorGridCat(BaseSpatialModule):
    def forward(self, factor_grid1: FactorGrid, factor_grid2: FactorGrid) -> FactorGrid:
        return factor_grid_cat(factor_grid1, factor_grid2)


class FactorGridPool(BaseSpatialModule):
    def __init__(self, pooling_type: Literal["max", "mean", "attention"] = "max"):
        super().__init__()
        self.pooling_type = pooling_type
        if pooling_type == "max":
            self.pool_op = nn.AdaptiveMaxPool1d(1)
        elif pooling_type == "mean":
            self.pool_op = nn.AdaptiveAvgPool1d(1)
        elif pooling_type == "attention":
            self.attention = None  # set by the owner once the feature width is known; mean pooling until then
            self.pool_op = None
        else:
            raise ValueError(f"Unsupported pooling type: {pooling_type}")

    def forward(self, factor_grid: FactorGrid) -> Tensor:
        return factor_grid_pool(factor_grid, self.pooling_type, pool_op=self.pool_op,
                                attention_layer=getattr(self, "attention", None))


class FactorGridIntraCommunication(BaseSpatialModule):
    def __init__(self, communication_types: List[Literal["sum", "mul"]] = ["sum"]) -> None:
        super().__init__()
        assert len(communication_types) > 0, "At least one communication type must be provided"
        assert len(communication_types) <= 2, "At most two communication types can be provided"
        self.communication_types = communication_types

    def forward(self, factor_grid: FactorGrid) -> FactorGrid:
        return factor_grid_intra_communication(factor_grid, self.communication_types)


class FactorGridPadToMatch(BaseSpatialModule):
    """The grids of ``up_factor_grid`` padded (replicating the border) to the image sizes of ``down_factor_grid``: the skip
    connection of a U-Net whose transposed convolutions came out a row or column short."""

    def forward(self, up_factor_grid: FactorGrid, down_factor_grid: FactorGrid) -> FactorGrid:
        assert len(up_factor_grid) == len(down_factor_grid), "FactorGrids must have same number of grids"
        from warpconvnet_amd.geometry.coords.grid import GridCoords
        from warpconvnet_amd.geometry.types.grid import Grid

        out = []
        for up, down in zip(up_factor_grid, down_factor_grid):
            t, want = up.grid_features.batched_tensor, down.grid_features.batched_tensor.shape[2:]
            have = t.shape[2:]
            if tuple(have) == tuple(want):
                out.append(up)
                continue
            pad = []
            for h, w in zip(reversed(have), reversed(want)):  # F.pad counts from the last dimension
                pad += [0, max(0, w - h)]
            t = F.pad(t, tuple(pad), mode="replicate")
            shape = list(up.grid_shape)
            axes = [a for a in range(3) if a != FORMAT_TO_AXIS[up.memory_format]] if up.memory_format in COMPRESSED_FORMATS \
                else {GridMemoryFormat.b_c_x_y_z: [0, 1, 2], GridMemoryFormat.b_c_z_x_y: [2, 0, 1]}[up.memory_format]
            for a, size in zip(axes, t.shape[2:]):
                shape[a] = int(size)
            coords = GridCoords.from_shape(tuple(shape), bounds=up.bounds, batch_size=up.batch_size, device=t.device)
            out.append(Grid(coords, t, memory_format=up.memory_format, grid_shape=tuple(shape), num_channels=up.num_channels))
        return FactorGrid(out)


class FactorGridToPoint(BaseSpatialModule):
    """Grid features interpolated at the points (``sample_method="interp"``), joined with the point features and the relative
    position, then ``combine_mlp``.  The gradient reaches the grid features, the point features and the MLP; the point
    coordinates receive none through the interpolation weights."""

    def __init__(self, grid_in_channels: int, point_in_channels: int, num_grids: int, out_channels: int, use_rel_pos: bool = True,
                 use_rel_pos_embed: bool = False, pos_embed_dim: int = 32, sample_method: Literal["graphconv", "interp"] = "interp",
                 neighbor_search_type: Literal["radius", "knn"] = "radius", knn_k: int = 16, reductions: List[str] = ["mean"]):
        super().__init__()
        if sample_method != "interp":
            raise NotImplementedError(f"sample_method={sample_method!r}: only 'interp' is implemented")
        self.grid_in_channels = grid_in_channels
        self.point_in_channels = point_in_channels
        self.out_channels = out_channels
        self.use_rel_pos = use_rel_pos
        self.use_rel_pos_embed = use_rel_pos_embed
        self.pos_embed_dim = pos_embed_dim
        self.sample_method = sample_method
        self.neighbor_search_type = neighbor_search_type
        self.knn_k = knn_k
        self.reductions = reductions
        self.freqs = get_freqs(pos_embed_dim)
        combined = grid_in_channels * num_grids + point_in_channels
        if use_rel_pos_embed:
            combined += pos_embed_dim * 3
        elif use_rel_pos:
            combined += 3
        self.combine_mlp = nn.Sequential(nn.Linear(combined, out_channels), nn.LayerNorm(out_channels), nn.GELU(),
                                         nn.Linear(out_channels, out_channels))

    def forward(self, factor_grid: FactorGrid, point_features: Points, backend: Optional[str] = None) -> Points:
        coords, feats = point_features.coordinate_tensor, point_features.feature_tensor
        parts = [feats, grid_sample_points(factor_grid, point_features, backend=backend).to(feats.dtype)]
        if self.use_rel_pos_embed or self.use_rel_pos:
            lo, hi = (b.to(device=coords.device, dtype=coords.dtype) for b in factor_grid[0].bounds)
            rel = coords - (hi + lo) / 2.0
            if self.use_rel_pos_embed:
                rel = sinusoidal_encoding(rel, self.pos_embed_dim, data_range=2)
            parts.append(rel.to(feats.dtype))
        out = self.combine_mlp(torch.cat(parts, dim=-1))
        return Points(batched_coordinates=point_features.batched_coordinates, batched_features=out)


class PointToFactorGrid(BaseSpatialModule):
    """``points_to_factor_grid`` over the box ``[aabb_min, aabb_max]``.  ``projections`` are created like in the reference
    (one per grid, so the parameter names match) and, like there, not applied in ``forward``."""

    def __init__(self, in_channels: int, out_channels: int, grid_shapes: List[Tuple[int, int, int]],
                 memory_formats: List[GridMemoryFormat], aabb_max: Tuple[float, float, float],
                 aabb_min: Tuple[float, float, float], use_rel_pos: bool = True, use_rel_pos_embed: bool = True,
                 pos_encode_dim: int = 32, search_radius: Optional[float] = None, k: int = 8,
                 search_type: Literal["radius", "knn", "voxel"] = "radius", reduction: str = "mean"):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.grid_shapes = grid_shapes
        self.memory_formats = [as_memory_format(f) for f in memory_formats]
        self.aabb_max = aabb_max
        self.aabb_min = aabb_min
        self.use_rel_pos = use_rel_pos
        self.use_rel_pos_embed = use_rel_pos_embed
        self.pos_encode_dim = pos_encode_dim
        self.search_radius = search_radius
        self.k = k
        self.search_type = search_type
        self.reduction = reduction
        self.compressed_spatial_dims = []
        for shape, fmt in zip(grid_shapes, self.memory_formats):
            if fmt not in COMPRESSED_FORMATS:
                raise ValueError(f"Unsupported memory format: {fmt}")
            # the reference sizes the b_zc_x_y projection by grid_shape[0]; kept, so that the parameter shapes interchange
            self.compressed_spatial_dims.append(shape[1] if fmt == GridMemoryFormat.b_yc_x_z else shape[0])
        self.projections = nn.ModuleList([nn.Linear(in_channels, out_channels * d) for d in self.compressed_spatial_dims])

    def forward(self, points: Points) -> FactorGrid:
        from warpconvnet_amd.geometry.types.conversion.to_factor_grid import points_to_factor_grid

        return points_to_factor_grid(points, self.grid_shapes, self.memory_formats,
                                     bounds=(torch.tensor(self.aabb_min), torch.tensor(self.aabb_max)),
                                     search_radius=self.search_radius, k=self.k, search_type=self.search_type,
                                     reduction=self.reduction)


def _image_axes(memory_format: GridMemoryFormat) -> List[int]:
    return [a for a in range(3) if a != FORMAT_TO_AXIS[memory_format]]


def _rebuilt(grid, features: Tensor, grid_shape: Tuple[int, int, int]):
    """``grid`` with new features over ``grid_shape`` (same box, batch size and memory format)."""
    from warpconvnet_amd.geometry.coords.grid import GridCoords
    from warpconvnet_amd.geometry.types.grid import Grid

    if tuple(grid_shape) == tuple(grid.grid_shape):
        return grid.replace(batched_features=features)
    coords = GridCoords.from_shape(tuple(grid_shape), bounds=grid.bounds, batch_size=grid.batch_size, device=features.device)
    return Grid(coords, features, memory_format=grid.memory_format, grid_shape=tuple(grid_shape))


class FactorGridProjection(BaseSpatialModule):
    """One ``Conv2d - norm - activation`` per grid over the folded channels (``convs``)."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, compressed_spatial_dims: Tuple[int, ...],
                 compressed_memory_formats: Tuple[GridMemoryFormat, ...], stride: int = 1,
                 norm: Type[nn.Module] = nn.BatchNorm2d, activation: Type[nn.Module] = nn.GELU):
        super().__init__()
        self.stride = stride
        self.convs = nn.ModuleList()
        for dim, _ in zip(compressed_spatial_dims, compressed_memory_formats):
            self.convs.append(nn.Sequential(
                nn.Conv2d(in_channels * dim, out_channels * dim, kernel_size, stride, (kernel_size - 1) // 2, bias=True),
                norm(out_channels * dim), activation()))

    def forward(self, grid: FactorGrid) -> FactorGrid:
        assert len(grid) == len(self.convs), f"Expected {len(self.convs)} grids, got {len(grid)}"
        out = []
        for g, conv in zip(grid, self.convs):
            feats = conv(g.grid_features.batched_tensor)
            axes, shape = _image_axes(g.memory_format), list(g.grid_shape)
            shape[axes[0]], shape[axes[1]] = int(feats.shape[2]), int(feats.shape[3])
            if self.stride != 1 and any(g.grid_shape[a] % self.stride for a in axes):
                raise ValueError(f"stride {self.stride} does not divide the image axes of grid shape {tuple(g.grid_shape)} "
                                 f"({g.memory_format.name}); the convolution gives features of shape {tuple(feats.shape)}")
            out.append(_rebuilt(g, feats, tuple(shape)))
        return FactorGrid(out)
