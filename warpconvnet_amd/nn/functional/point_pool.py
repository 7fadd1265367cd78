"""Pooling a point cloud onto voxels or onto fewer points (reference `warpconvnet/nn/functional/point_pool.py:205-370`:
``point_pool`` and ``point_pool_by_code``, every argument and default of the reference).

The voxel route builds the point <-> voxel map once (``voxel_downsample_csr_mapping``: packed keys, one stable sort,
``wcn_voxel_map``) and pools the features with ``csr_pool`` (`ops/csr_rows.py`: ``wcn_csr_gather_reduce`` forward,
``wcn_row_spread`` backward) - the reference materialises ``features[to_csr_indices]`` and calls ``torch_scatter``.  The
returned ``ToUnique`` drives ``point_unpool``.  ``return_type`` also accepts ``"sparse"`` for ``"voxel"``: the reference's own
modules pass it.
"""
import warnings
from typing import Optional, Union

import torch
from torch import Tensor

from warpconvnet_amd.geometry.coords.integer import IntCoords
from warpconvnet_amd.geometry.coords.ops.batch_index import offsets_from_offsets
from warpconvnet_amd.geometry.coords.ops.voxel import voxel_downsample_csr_mapping, voxel_downsample_random_indices
from warpconvnet_amd.geometry.coords.real import RealCoords
from warpconvnet_amd.geometry.coords.sample import farthest_sample_per_batch, random_sample_per_batch
from warpconvnet_amd.geometry.coords.search.knn import batched_knn_search
from warpconvnet_amd.geometry.coords.search.search_results import RealSearchResult
from warpconvnet_amd.ops.csr_rows import csr_pool, csr_unpool
from warpconvnet_amd.ops.reductions import REDUCTION_TYPES_STR, REDUCTIONS, two_pass_var
from warpconvnet_amd.utils.unique import ToUnique, UniqueInfo

__all__ = ["point_pool", "point_pool_by_code", "pool_features"]


def pool_features(features: Tensor, to_unique: ToUnique, reduction: Union[REDUCTIONS, REDUCTION_TYPES_STR], eps: float = 1e-6):
    """``features`` [N, C] reduced over the groups of ``to_unique``; ``var`` / ``std`` are the two passes of
    ``ops.reductions.two_pass_var`` (the mean is spread back to the points with ``wcn_row_spread``)."""
    if isinstance(reduction, str):
        reduction = REDUCTIONS(reduction)
    if reduction in (REDUCTIONS.SUM, REDUCTIONS.MEAN, REDUCTIONS.MAX, REDUCTIONS.MIN):
        return csr_pool(features, to_unique, reduction.value)
    if reduction in (REDUCTIONS.VAR, REDUCTIONS.STD):
        return two_pass_var(features, lambda t: csr_pool(t, to_unique, "mean"), lambda y: csr_unpool(y, to_unique),
                            std=reduction == REDUCTIONS.STD, eps=eps)
    raise ValueError(f"Invalid reduction for pooling: {reduction}")


def _return_class(return_type: str):
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.geometry.types.voxels import Voxels

    return Voxels if return_type in ("voxel", "sparse") else Points


def _pooled_coordinates(pc, return_type: str, to_unique: Optional[ToUnique], unique_indices: Tensor, unique_offsets: Tensor,
                        voxel_size: float, average_pooled_coordinates: bool, unique_coords: Optional[Tensor] = None):
    if return_type == "point":
        if average_pooled_coordinates:
            return RealCoords(csr_pool(pc.coordinate_tensor, to_unique, "mean"), unique_offsets)
        return RealCoords(pc.coordinate_tensor[unique_indices], unique_offsets)
    if unique_coords is None:
        unique_coords = torch.floor(pc.coordinate_tensor[unique_indices] / voxel_size).int()
    return IntCoords(unique_coords, unique_offsets)


def _pool_by_random_sample(pc, voxel_size: float, return_type: str):
    unique_indices, unique_offsets = voxel_downsample_random_indices(pc.coordinate_tensor, pc.offsets, voxel_size)
    coords = _pooled_coordinates(pc, return_type, None, unique_indices, unique_offsets, voxel_size, False)
    return _return_class(return_type)(batched_coordinates=coords, batched_features=pc.features[unique_indices],
                                      voxel_size=voxel_size)


def _pool_by_max_num_points(pc, reduction, max_num_points: int, return_type: str, return_neighbor_search_result: bool,
                            sample_method: str = "random"):
    """At most ``max_num_points`` points per batch element survive, drawn at random (with replacement) or by farthest point
    sampling from the element's first point (``sample_method="fps"``: the same cloud gives the same survivors); every point
    is pooled onto its nearest survivor."""
    dev = pc.coordinate_tensor.device
    if sample_method == "fps":
        assert bool((pc.offsets.diff() > 0).all()), "sample_method='fps' needs at least one point in every batch element"
        sample_idx, sampled_offsets = farthest_sample_per_batch(pc.coordinate_tensor, pc.offsets, max_num_points)
    else:
        sample_idx, sampled_offsets = random_sample_per_batch(pc.offsets, max_num_points)
    sample_idx = sample_idx.to(dev, torch.int64)
    sampled_coords = pc.coordinate_tensor[sample_idx]
    nearest = batched_knn_search(sampled_coords, sampled_offsets, pc.coordinate_tensor, pc.offsets, k=1).reshape(-1)
    nearest_sorted, order = torch.sort(nearest, stable=True)
    survivors, counts = torch.unique_consecutive(nearest_sorted, return_counts=True)
    knn_offsets = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    to_orig = torch.empty_like(nearest)
    to_orig[order] = torch.repeat_interleave(torch.arange(len(survivors), device=dev), counts, output_size=len(nearest))
    groups = ToUnique.from_info(UniqueInfo(to_orig, order, knn_offsets, order[knn_offsets[:-1]]))
    down_features = pool_features(pc.features, groups, reduction)
    if len(survivors) != len(sample_idx):  # samples that are nobody's nearest (or drawn twice) drop out
        sampled_coords = sampled_coords[survivors]
        sampled_offsets = offsets_from_offsets(sampled_offsets, survivors)
        if return_neighbor_search_result:
            warnings.warn(
                "Neighbor search result requires remapping the indices to the unique indices. "
                "This may incur additional overhead.",
                stacklevel=2,
            )
            nearest = to_orig
    out = _return_class(return_type)(batched_coordinates=sampled_coords, batched_features=down_features,
                                     offsets=sampled_offsets, num_points=max_num_points)
    if return_neighbor_search_result:
        return out, RealSearchResult(nearest, knn_offsets)
    return out


def point_pool(
    pc: "Points",  # noqa: F821
    reduction: Union[REDUCTIONS, REDUCTION_TYPES_STR],
    downsample_max_num_points: Optional[int] = None,
    downsample_voxel_size: Optional[float] = None,
    return_type: str = "point",
    average_pooled_coordinates: bool = False,
    return_neighbor_search_result: bool = False,
    return_to_unique: bool = False,
    unique_method: str = "torch",
    sample_method: str = "random",
):
    """Pool ``pc`` onto voxels of edge ``downsample_voxel_size`` or onto at most ``downsample_max_num_points`` points per
    batch element (the latter wins when both are given, like the reference).  ``sample_method`` picks those points:
    ``"random"`` (the reference's draw with replacement) or ``"fps"`` (farthest point sampling, repeatable).
    Returns ``Points`` (``return_type="point"``) or ``Voxels`` (``"voxel"`` / ``"sparse"``), followed by the ``ToUnique``
    (``return_to_unique``) or a ``RealSearchResult`` (``return_neighbor_search_result``) when asked."""
    if isinstance(reduction, str):
        reduction = REDUCTIONS(reduction)
    assert (
        downsample_max_num_points is not None or downsample_voxel_size is not None
    ), "Either downsample_num_points or downsample_voxel_size must be provided."
    assert return_type in ("point", "voxel", "sparse"), "return_type must be either point or voxel."
    assert sample_method in ("random", "fps"), "sample_method must be either random or fps."
    if return_type != "point":
        assert not average_pooled_coordinates, "averaging pooled coordinates is not supported for Voxels return type"

    if downsample_max_num_points is not None:
        assert not return_to_unique, "return_to_unique must be False when downsample_max_num_points is provided."
        return _pool_by_max_num_points(pc, reduction, downsample_max_num_points, return_type, return_neighbor_search_result,
                                       sample_method)

    if reduction == REDUCTIONS.RANDOM:
        assert not return_to_unique, "return_to_unique must be False when reduction is RANDOM."
        assert not return_neighbor_search_result, "return_neighbor_search_result must be False when reduction is RANDOM."
        return _pool_by_random_sample(pc, downsample_voxel_size, return_type)

    unique_coords, unique_offsets, _, _, to_unique = voxel_downsample_csr_mapping(
        pc.coordinate_tensor, pc.offsets, downsample_voxel_size, unique_method=unique_method
    )
    down_features = pool_features(pc.feature_tensor, to_unique, reduction)
    coords = _pooled_coordinates(pc, return_type, to_unique, to_unique.to_unique_indices, unique_offsets,
                                 downsample_voxel_size, average_pooled_coordinates, unique_coords)
    out = _return_class(return_type)(batched_coordinates=coords, batched_features=down_features,
                                     voxel_size=downsample_voxel_size)
    if return_to_unique:
        return out, to_unique
    if return_neighbor_search_result:
        return out, RealSearchResult(to_unique.to_unique_indices, unique_offsets)
    return out


def point_pool_by_code(
    pc: "Points",  # noqa: F821
    code: Tensor,
    reduction: Union[REDUCTIONS, REDUCTION_TYPES_STR],
    average_pooled_coordinates: bool = False,
    return_to_unique: bool = False,
):
    """Pool the points that share a value of ``code`` [N] (a clustering or serialisation code; batch-sorted like the points).
    The pooled cloud keeps the other attributes of ``pc`` and carries the distinct codes as ``code``."""
    to_unique = ToUnique(return_to_unique_indices=True)
    unique_code = to_unique.to_unique(code)
    if average_pooled_coordinates:
        coords = csr_pool(pc.coordinate_tensor, to_unique, "mean")
    else:
        coords = pc.coordinate_tensor[to_unique.to_unique_indices]
    features = pool_features(pc.feature_tensor, to_unique, reduction)
    offsets = offsets_from_offsets(pc.offsets, to_unique.to_unique_indices)
    out = pc.replace(batched_coordinates=RealCoords(coords, offsets), batched_features=features, code=unique_code)
    if return_to_unique:
        return out, to_unique
    return out
