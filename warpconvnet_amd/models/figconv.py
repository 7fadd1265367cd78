"""FIGConvNet: a U-Net of 2-D convolutions over factorised grids (reference `warpconvnet/models/figconv.py`: the same class
names, constructor arguments and ``state_dict`` keys, so checkpoints interchange by key).

Points are scattered onto a few thin grids (``PointToFactorGrid``); every level of the U-Net is a ``FactorGridGlobalConv`` -
per grid a convolution of the folded image (stride 2 on the way down, a transposed convolution of stride 2 on the way up; the
tile kernels of csrc/dense_conv2d.hip) and an exchange between the grids; a pooled copy of the chosen
levels feeds an MLP that predicts one scalar (drag) per cloud; the finest grids are sampled back at the points
(``FactorGridToPoint``) and projected to ``out_channels``.  ``backend`` goes to every convolution.

One departure: ``to_point_sample_method`` defaults to ``"interp"``, the one method ``FactorGridToPoint`` implements here (the
reference's default ``"graphconv"`` raises ``NotImplementedError``).
"""
from typing import List, Literal, Optional, Tuple, Union

import torch
import torch.nn as nn
from torch import Tensor

from warpconvnet_amd.geometry.features.grid import FORMAT_TO_AXIS, GridMemoryFormat, as_memory_format
from warpconvnet_amd.geometry.types.factor_grid import FactorGrid
from warpconvnet_amd.geometry.types.points import Points
from warpconvnet_amd.nn.modules.base_module import BaseSpatialModel
from warpconvnet_amd.nn.modules.factor_grid import FactorGridGlobalConv, FactorGridPool, FactorGridToPoint, PointToFactorGrid
from warpconvnet_amd.nn.modules.mlp import FeatureMLPBlock

__all__ = ["FIGConvNet", "FIGConvNetDrivAer"]


class FIGConvNet(BaseSpatialModel):
    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, hidden_channels: List[int], num_levels: int = 3,
                 num_down_blocks: Union[int, List[int]] = 1, num_up_blocks: Union[int, List[int]] = 1,
                 mlp_channels: List[int] = [2048, 2048], aabb_max: Tuple[float, float, float] = (1.0, 1.0, 1.0),
                 aabb_min: Tuple[float, float, float] = (0.0, 0.0, 0.0), voxel_size: Optional[float] = None,
                 resolution_memory_format_pairs: List[Tuple[GridMemoryFormat, Tuple[int, int, int]]] = [
                     (GridMemoryFormat.b_xc_y_z, (2, 128, 128)), (GridMemoryFormat.b_yc_x_z, (128, 2, 128)),
                     (GridMemoryFormat.b_zc_x_y, (128, 128, 2))],
                 use_rel_pos: bool = True, use_rel_pos_embed: bool = False, pos_encode_dim: int = 32,
                 communication_types: List[Literal["mul", "sum"]] = ["sum"],
                 to_point_sample_method: Literal["graphconv", "interp"] = "interp",
                 neighbor_search_type: Literal["knn", "radius"] = "radius", knn_k: int = 16, reductions: List[str] = ["mean"],
                 pooling_type: Literal["attention", "max", "mean"] = "max", pooling_layers: Optional[List[int]] = None,
                 backend: Optional[str] = None):
        super().__init__()
        self.in_channels, self.out_channels, self.hidden_channels, self.num_levels = in_channels, out_channels, hidden_channels, num_levels
        self.aabb_max, self.aabb_min = aabb_max, aabb_min
        formats = [as_memory_format(f) for f, _ in resolution_memory_format_pairs]
        shapes = [tuple(s) for _, s in resolution_memory_format_pairs]
        self.grid_feature_group_size = len(shapes)
        self.compressed_spatial_dims = dims = [s[FORMAT_TO_AXIS[f]] for f, s in zip(formats, shapes)]
        self.point_to_factor_grids = PointToFactorGrid(
            in_channels, hidden_channels[0], shapes, formats, aabb_max, aabb_min, use_rel_pos=use_rel_pos,
            use_rel_pos_embed=use_rel_pos_embed, pos_encode_dim=pos_encode_dim,
            search_radius=voxel_size * 2 if voxel_size else None, k=knn_k, search_type=neighbor_search_type,
            reduction=reductions[0] if reductions else "mean")

        def level(n_blocks, cin, cout, **first):
            """``n_blocks`` blocks; the first one changes the resolution (``first``: stride or up_stride)."""
            return nn.Sequential(*[
                FactorGridGlobalConv(cin if i == 0 else cout, cout, kernel_size, tuple(dims), tuple(formats),
                                     communication_types=communication_types, backend=backend, **(first if i == 0 else {}))
                for i in range(n_blocks)])

        n_down = [num_down_blocks] * num_levels if isinstance(num_down_blocks, int) else num_down_blocks
        n_up = [num_up_blocks] * num_levels if isinstance(num_up_blocks, int) else num_up_blocks
        self.down_blocks = nn.ModuleList(level(n_down[i], hidden_channels[i], hidden_channels[i + 1], stride=2)
                                         for i in range(num_levels))
        self.up_blocks = nn.ModuleList(level(n_up[i], hidden_channels[i + 1], hidden_channels[i], up_stride=2)
                                       for i in range(num_levels))

        self.pooling_layers = [num_levels] if pooling_layers is None else pooling_layers
        assert all(layer <= num_levels for layer in self.pooling_layers), f"pooling_layers {self.pooling_layers} above {num_levels}"
        self.grid_pools = nn.ModuleList(FactorGridPool(pooling_type=pooling_type) for _ in self.pooling_layers)
        pooled = sum(hidden_channels[layer] * d for layer in self.pooling_layers for d in dims)
        self.mlp = FeatureMLPBlock(pooled, mlp_channels[-1], mlp_channels[:-1])
        self.mlp_projection = nn.Linear(mlp_channels[-1], 1)

        width = hidden_channels[0] * 2
        self.to_point = FactorGridToPoint(hidden_channels[0], in_channels, len(shapes), width, use_rel_pos=use_rel_pos,
                                          use_rel_pos_embed=use_rel_pos_embed, pos_embed_dim=pos_encode_dim,
                                          sample_method=to_point_sample_method, neighbor_search_type=neighbor_search_type,
                                          knn_k=knn_k, reductions=reductions)
        self.projection = nn.Sequential(nn.Linear(width, width), nn.LayerNorm(width), nn.GELU(), nn.Linear(width, out_channels))

    def _grid_forward(self, points: Points) -> Tuple[FactorGrid, Tensor]:
        """The U-Net over the grids: the finest level's grids after the up path and the ``[B, 1]`` drag prediction."""
        levels = [self.point_to_factor_grids(points)]
        for block in self.down_blocks:
            levels.append(block(levels[-1]))
        pooled = [pool(levels[layer]) for pool, layer in zip(self.grid_pools, self.pooling_layers)]
        drag = self.mlp_projection(self.mlp(torch.cat(pooled, dim=-1)))
        for i in reversed(range(self.num_levels)):  # the up block restores level i's grid shape; its output joins the skip
            levels[i] = self.up_blocks[i](levels[i + 1]) + levels[i]
        return levels[0], drag

    def forward(self, points: Points) -> Tuple[Points, Tensor]:
        grids, drag = self._grid_forward(points)
        feats = self.projection(self.to_point(grids, points).feature_tensor)
        return Points(batched_coordinates=points.batched_coordinates, batched_features=feats), drag


class FIGConvNetDrivAer(FIGConvNet):
    """FIGConvNet with the DrivAer box, grids (4 x 120 x 80, 200 x 3 x 80, 200 x 120 x 2) and search defaults."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, hidden_channels: List[int], num_levels: int = 3,
                 num_down_blocks: Union[int, List[int]] = 1, num_up_blocks: Union[int, List[int]] = 1,
                 aabb_max: Tuple[float, float, float] = (2.5, 1.5, 1.0), aabb_min: Tuple[float, float, float] = (-2.5, -1.5, -1.0),
                 voxel_size: Optional[float] = None,
                 resolution_memory_format_pairs: List[Tuple[GridMemoryFormat, Tuple[int, int, int]]] = [
                     (GridMemoryFormat.b_xc_y_z, (4, 120, 80)), (GridMemoryFormat.b_yc_x_z, (200, 3, 80)),
                     (GridMemoryFormat.b_zc_x_y, (200, 120, 2))],
                 use_rel_pos: bool = True, use_rel_pos_embed: bool = True, pos_encode_dim: int = 32,
                 communication_types: List[Literal["mul", "sum"]] = ["sum"],
                 to_point_sample_method: Literal["graphconv", "interp"] = "interp",
                 neighbor_search_type: Literal["knn", "radius"] = "knn", knn_k: int = 16, reductions: List[str] = ["mean"],
                 pooling_type: Literal["attention", "max", "mean"] = "max", pooling_layers: Optional[List[int]] = None,
                 drag_loss_weight: Optional[float] = None, backend: Optional[str] = None):
        super().__init__(in_channels, out_channels, kernel_size, hidden_channels, num_levels=num_levels,
                         num_down_blocks=num_down_blocks, num_up_blocks=num_up_blocks, aabb_max=aabb_max, aabb_min=aabb_min,
                         voxel_size=voxel_size, resolution_memory_format_pairs=resolution_memory_format_pairs,
                         use_rel_pos=use_rel_pos, use_rel_pos_embed=use_rel_pos_embed, pos_encode_dim=pos_encode_dim,
                         communication_types=communication_types, to_point_sample_method=to_point_sample_method,
                         neighbor_search_type=neighbor_search_type, knn_k=knn_k, reductions=reductions,
                         pooling_type=pooling_type, pooling_layers=pooling_layers, backend=backend)
        if drag_loss_weight is not None:
            self.drag_loss_weight = drag_loss_weight
