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
shape disagrees with its features - here that raises a ``ValueError`` naming the shapes.

``FactorGridGlobalConv`` is the block of FIGConvNet's U-Net: per grid one ``_FactorGridConvNormAct`` (``Conv2d`` of stride 1 / 2
or ``ConvTranspose2d`` of ``up_stride`` 2, norm, activation), then the intra-communication and, with two communication types,
a 1 x 1 ``FactorGridProjection``.  Every convolution goes through `nn/functional/dense_conv2d.py` on the module's own
``nn.Conv2d`` / ``nn.ConvTranspose2d`` parameters (``backend``: ``"hip"`` the tile kernels of csrc/dense_conv2d.hip, ``"torch"``
the framework, ``None`` by the measured table); where the kernels run the features become channels-last once at the block's
entry and the norm and activation run on that layout.  The same two departures hold for these blocks.
"""
from typing import List, Literal, Optional, Tuple, Type

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from warpconvnet_amd.geometry.features.grid import COMPRESSED_FORMATS, FORMAT_TO_AXIS, GridMemoryFormat, as_memory_format
from warpconvnet_amd.geometry.types.factor_grid import FactorGrid
from warpconvnet_amd.geometry.types.points import Points
from warpconvnet_amd.nn.functional.dense_conv2d import dense_conv2d, dense_conv_transpose2d, takes_hip
from warpconvnet_amd.nn.functional.encodings import get_freqs, sinusoidal_encoding
from warpconvnet_amd.nn.functional.factor_grid import (factor_grid_cat, factor_grid_intra_communication, factor_grid_pool,
                                                       factor_grid_transform)
from warpconvnet_amd.nn.functional.grid_sample import grid_sample_points
from warpconvnet_amd.nn.modules.base_module import BaseSpatialModule

__all__ = ["FactorGridTransform", "FactorGridCat", "FactorGridPool", "FactorGridIntraCommunication", "FactorGridPadToMatch",
           "FactorGridToPoint", "PointToFactorGrid", "FactorGridProjection", "FactorGridGlobalConv"]


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


def _conv_norm_act(layers: nn.Sequential, feats: Tensor, backend: Optional[str]) -> Tensor:
    """``layers`` = (``Conv2d`` | ``ConvTranspose2d``, norm, activation) on ``feats``: the convolution through the dense 2-D
    functional on the layer's own parameters, the rest as framework ops on whatever layout the convolution left."""
    conv = layers[0]
    transposed = isinstance(conv, nn.ConvTranspose2d)
    if takes_hip(feats, conv.weight, conv.bias, conv.stride[0], transposed, backend):
        feats = feats.contiguous(memory_format=torch.channels_last)  # once, at the block's entry
    fn = dense_conv_transpose2d if transposed else dense_conv2d
    feats = fn(feats, conv.weight, conv.bias, stride=conv.stride[0], backend=backend)
    for layer in list(layers)[1:]:
        feats = layer(feats)
    return feats


class FactorGridProjection(BaseSpatialModule):
    """One ``Conv2d - norm - activation`` per grid over the folded channels (``convs``)."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, compressed_spatial_dims: Tuple[int, ...],
                 compressed_memory_formats: Tuple[GridMemoryFormat, ...], stride: int = 1,
                 norm: Type[nn.Module] = nn.BatchNorm2d, activation: Type[nn.Module] = nn.GELU, backend: Optional[str] = None):
        super().__init__()
        self.stride = stride
        self.backend = backend
        self.convs = nn.ModuleList()
        for dim, _ in zip(compressed_spatial_dims, compressed_memory_formats):
            self.convs.append(nn.Sequential(
                nn.Conv2d(in_channels * dim, out_channels * dim, kernel_size, stride, (kernel_size - 1) // 2, bias=True),
                norm(out_channels * dim), activation()))

    def forward(self, grid: FactorGrid) -> FactorGrid:
        assert len(grid) == len(self.convs), f"Expected {len(self.convs)} grids, got {len(grid)}"
        out = []
        for g, conv in zip(grid, self.convs):
            feats = _conv_norm_act(conv, g.grid_features.batched_tensor, self.backend)
            axes, shape = _image_axes(g.memory_format), list(g.grid_shape)
            shape[axes[0]], shape[axes[1]] = int(feats.shape[2]), int(feats.shape[3])
            if self.stride != 1 and any(g.grid_shape[a] % self.stride for a in axes):
                raise ValueError(f"stride {self.stride} does not divide the image axes of grid shape {tuple(g.grid_shape)} "
                                 f"({g.memory_format.name}); the convolution gives features of shape {tuple(feats.shape)}")
            out.append(_rebuilt(g, feats, tuple(shape)))
        return FactorGrid(out)


class _FactorGridConvNormAct(BaseSpatialModule):
    """``Conv2d`` (stride 1 / 2) or ``ConvTranspose2d`` (``up_stride``), norm and activation on one grid's folded image
    (``conv_norm_layers``).  A stride divides the image axes (ValueError otherwise); after the transposed convolution the image
    (``2 H - 1``) is padded, replicating its border, to ``up_stride * H``."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, compressed_spatial_dim: int,
                 compressed_memory_format: GridMemoryFormat, stride: int = 1, up_stride: Optional[int] = None,
                 norm: Type[nn.Module] = nn.BatchNorm2d, activation: Type[nn.Module] = nn.GELU, backend: Optional[str] = None):
        super().__init__()
        compressed_memory_format = as_memory_format(compressed_memory_format)
        assert compressed_memory_format in COMPRESSED_FORMATS, f"not a compressed format: {compressed_memory_format}"
        self.stride, self.up_stride, self.backend = stride, up_stride, backend
        self.compressed_spatial_dim = compressed_spatial_dim
        self.compressed_memory_format = compressed_memory_format
        cin, cout, pad = in_channels * compressed_spatial_dim, out_channels * compressed_spatial_dim, (kernel_size - 1) // 2
        self.conv_norm_layers = nn.Sequential(
            nn.Conv2d(cin, cout, kernel_size, stride, pad, bias=True) if up_stride is None
            else nn.ConvTranspose2d(cin, cout, kernel_size, stride=up_stride, padding=pad, bias=True),
            norm(cout) if norm is not None else nn.Identity(),
            activation() if activation is not None else nn.Identity())

    def forward(self, grid):
        feats = _conv_norm_act(self.conv_norm_layers, grid.grid_features.batched_tensor, self.backend)
        if self.up_stride is None and self.stride == 1:
            return grid.replace(batched_features=feats)
        axes, shape = _image_axes(grid.memory_format), list(grid.grid_shape)
        if self.up_stride is not None:
            for a in axes:
                shape[a] = grid.grid_shape[a] * self.up_stride
            pad_h, pad_w = max(0, shape[axes[0]] - feats.shape[2]), max(0, shape[axes[1]] - feats.shape[3])
            feats = F.pad(feats, (0, pad_w, 0, pad_h), mode="replicate")
        else:
            if any(grid.grid_shape[a] % self.stride for a in axes):
                raise ValueError(f"stride {self.stride} does not divide the image axes of grid shape {tuple(grid.grid_shape)} "
                                 f"({grid.memory_format.name}); the convolution gives features of shape {tuple(feats.shape)}")
            for a in axes:
                shape[a] = grid.grid_shape[a] // self.stride
        return _rebuilt(grid, feats, tuple(shape))


class FactorGridGlobalConv(BaseSpatialModule):
    """Per grid a ``_FactorGridConvNormAct`` (``conv_blocks``), then ``intra_communications`` and, with two communication types,
    the 1 x 1 projection ``proj`` back to ``out_channels``."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, compressed_spatial_dims: Tuple[int, ...],
                 compressed_memory_formats: Tuple[GridMemoryFormat, ...], stride: int = 1, up_stride: Optional[int] = None,
                 communication_types: List[Literal["sum", "mul"]] = ["sum"], norm: Type[nn.Module] = nn.BatchNorm2d,
                 activation: Type[nn.Module] = nn.GELU, backend: Optional[str] = None):
        super().__init__()
        assert len(compressed_spatial_dims) == len(compressed_memory_formats), "one compressed dimension per memory format"
        self.conv_blocks = nn.ModuleList([
            _FactorGridConvNormAct(in_channels, out_channels, kernel_size, dim, fmt, stride=stride, up_stride=up_stride, norm=norm,
                                   activation=activation, backend=backend)
            for dim, fmt in zip(compressed_spatial_dims, compressed_memory_formats)])
        self.intra_communications = FactorGridIntraCommunication(communication_types=communication_types)
        if len(communication_types) > 1:
            self.proj = FactorGridProjection(out_channels * len(communication_types), out_channels, 1, compressed_spatial_dims,
                                             compressed_memory_formats, stride=1, backend=backend)
        else:
            self.proj = nn.Identity()

    def forward(self, factor_grid: FactorGrid) -> FactorGrid:
        assert len(factor_grid) == len(self.conv_blocks), f"Expected {len(self.conv_blocks)} grids, got {len(factor_grid)}"
        convolved = FactorGrid([block(g) for g, block in zip(factor_grid, self.conv_blocks)])
        return self.proj(self.intra_communications(convolved))
