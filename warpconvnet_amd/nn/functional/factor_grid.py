"""Operations over the grids of a ``FactorGrid`` (reference `warpconvnet/nn/functional/factor_grid.py`: the same four
functions and signatures).

``factor_grid_intra_communication`` lets every grid take in the features of the others: each source grid is interpolated
trilinearly at the vertex positions of the target grid and added to (``sum``) or multiplied into (``mul``) the target.  On the
GPU the interpolation is the strided sampler of `csrc/grid.hip`: the source is read in place in its own memory format and the
map from the target's vertices to the source's cells - a function of the two shapes and the bounds only - is built once and
kept (``_VERTEX_MAPS``).  The ``+=`` / ``*=`` itself is a framework op.  CPU tensors take the framework's ``F.grid_sample``
composition (`grid_sample.py`, ``backend="torch"``).
"""
from typing import Callable, Dict, List, Literal, Optional

import torch
import torch.nn.functional as F
from torch import Tensor

from warpconvnet_amd.geometry.features.grid import COMPRESSED_FORMATS, GridMemoryFormat, convert_from_standard_format
from warpconvnet_amd.geometry.types.factor_grid import FactorGrid
from warpconvnet_amd.geometry.types.grid import Grid
from warpconvnet_amd.nn.functional.grid_sample import GridSampleMap, _GridSampleHip, _sample_torch, default_backend

__all__ = ["factor_grid_transform", "factor_grid_cat", "factor_grid_pool", "factor_grid_intra_communication"]

# (source shape, target shape, bounds of both, batch size, device) -> (GridSampleMap, the target's vertex positions)
_VERTEX_MAPS: Dict[tuple, tuple] = {}
_VERTEX_MAPS_MAX = 64


def factor_grid_transform(factor_grid: FactorGrid, transform_fn: Callable[[Tensor], Tensor], in_place: bool = True) -> FactorGrid:
    """``transform_fn`` applied to the feature tensor of every grid (``in_place`` is accepted for the reference's module, which
    passes it; the grids are always new objects)."""
    return FactorGrid([g.replace(batched_features=transform_fn(g.grid_features.batched_tensor)) for g in factor_grid])


def factor_grid_cat(factor_grid1: FactorGrid, factor_grid2: FactorGrid) -> FactorGrid:
    """Concatenation along the channel dimension, grid by grid (dim 1, the last one for ``b_x_y_z_c``).  Like in the
    reference the folded dim 1 of a factorized format is joined as it stands: the result holds the first grid's ``axis * C1``
    planes followed by the second's, which is what the 2-D convolutions that follow were trained on."""
    assert len(factor_grid1) == len(factor_grid2), f"FactorGrid lengths must match: {len(factor_grid1)} != {len(factor_grid2)}"
    out = []
    for g1, g2 in zip(factor_grid1, factor_grid2):
        dim = -1 if g1.memory_format == GridMemoryFormat.b_x_y_z_c else 1
        out.append(g1.replace(batched_features=torch.cat([g1.grid_features.batched_tensor, g2.grid_features.batched_tensor],
                                                         dim=dim)))
    return FactorGrid(out)


def factor_grid_pool(factor_grid: FactorGrid, pooling_type: Literal["max", "mean", "attention"] = "max",
                     pool_op: Optional[Callable] = None, attention_layer: Optional[Callable] = None) -> Tensor:
    """Every grid reduced over its two image axes and the results joined: [B, sum of folded channels]."""
    pooled = []
    for g in factor_grid:
        if g.memory_format not in COMPRESSED_FORMATS:
            raise ValueError(f"Unsupported memory format for pooling: {g.memory_format}")
        t = g.grid_features.batched_tensor
        flat = t.reshape(t.shape[0], t.shape[1], -1)
        if pooling_type in ("max", "mean"):
            if pool_op is not None:
                p = pool_op(flat).squeeze(-1)
            else:
                p = (F.adaptive_max_pool1d if pooling_type == "max" else F.adaptive_avg_pool1d)(flat, 1).squeeze(-1)
        elif pooling_type == "attention":
            if attention_layer is not None:
                seq = flat.transpose(1, 2)
                p = attention_layer(seq, seq, seq)[0].mean(dim=1)
            else:
                p = F.adaptive_avg_pool1d(flat, 1).squeeze(-1)
        else:
            raise ValueError(f"Unsupported pooling type: {pooling_type}")
        pooled.append(p)
    return torch.cat(pooled, dim=-1)


def _vertex_map(source: Grid, target: Grid):
    """The cached map from the target grid's vertices (as points) to the source grid's cells."""
    dev = source.grid_features.batched_tensor.device
    key = (source.grid_shape, target.grid_shape, tuple(source.bounds[0].tolist()), tuple(source.bounds[1].tolist()),
           tuple(target.bounds[0].tolist()), tuple(target.bounds[1].tolist()), source.batch_size, str(dev))
    hit = _VERTEX_MAPS.get(key)
    if hit is None:
        with torch.no_grad():
            coords = target.grid_coords.to(dev).batched_tensor.reshape(-1, 3).float().contiguous()
            hit = (GridSampleMap(coords, target.grid_coords.offsets, source.grid_shape, source.bounds), coords)
        if len(_VERTEX_MAPS) >= _VERTEX_MAPS_MAX:
            _VERTEX_MAPS.pop(next(iter(_VERTEX_MAPS)))
        _VERTEX_MAPS[key] = hit
    return hit


def _sample_at_vertices(source: Grid, target: Grid, backend: str) -> Tensor:
    """``source`` interpolated at the vertices of ``target``, in the target's memory format."""
    b, (h, w, d), c = target.batch_size, target.grid_shape, source.num_channels
    if backend == "hip":
        m, _ = _vertex_map(source, target)
        rows = _GridSampleHip.apply([m], [(source.memory_format, c)], source.grid_features.batched_tensor)
    else:
        coords = target.grid_coords.to(source.device).batched_tensor.reshape(-1, 3)
        rows = _sample_torch(source, coords.to(source.grid_features.batched_tensor.dtype), target.grid_coords.offsets)
    return convert_from_standard_format(rows.view(b, h, w, d, c), target.memory_format, target.grid_shape)


def _factor_grid_intra_communication(factor_grid: FactorGrid, communication_type: str, backend: Optional[str]) -> FactorGrid:
    if communication_type not in ("sum", "mul"):
        raise ValueError(f"Unknown communication type: {communication_type}")
    if len(factor_grid) == 1:
        return factor_grid
    if backend is None:
        backend = default_backend(factor_grid.device)
    out = []
    for i, target in enumerate(factor_grid):
        feats = target.grid_features.batched_tensor
        for j, source in enumerate(factor_grid):
            if i == j:
                continue
            assert source.num_channels == target.num_channels, (
                f"All grids must have same channels: {source.num_channels} != {target.num_channels}")
            sampled = _sample_at_vertices(source, target, backend).to(feats.dtype)
            feats = feats + sampled if communication_type == "sum" else feats * sampled
        out.append(target.replace(batched_features=feats))
    return FactorGrid(out)


def factor_grid_intra_communication(factor_grid: FactorGrid, communication_types: List[Literal["sum", "mul"]] = ["sum"],
                                    cat_fn: Optional[Callable] = None, backend: Optional[str] = None) -> FactorGrid:
    """One communication type, or two whose results are joined channel-wise (``cat_fn``, default ``factor_grid_cat``).
    ``backend``: ``"hip"`` / ``"torch"``, default by device."""
    if len(communication_types) == 1:
        return _factor_grid_intra_communication(factor_grid, communication_types[0], backend)
    if len(communication_types) == 2:
        r1 = _factor_grid_intra_communication(factor_grid, communication_types[0], backend)
        r2 = _factor_grid_intra_communication(factor_grid, communication_types[1], backend)
        return cat_fn(r1, r2) if cat_fn is not None else factor_grid_cat(r1, r2)
    raise ValueError(f"Unsupported number of communication types: {len(communication_types)}")
