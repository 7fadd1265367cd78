"""Concatenate / prune spatially sparse tensors (reference `warpconvnet/nn/functional/sparse_ops.py:14-65`).

Pruning a ``Voxels`` is one compaction on the device (`wcn_resample_expand` with one slot per row: count, scan, emit - kept
coordinates, the old-row -> new-row table and the new batch offsets with ONE host read, no ``bincount``) and one copy of the
kept feature rows (`wcn_resample_unpack`; its gradient is `wcn_resample_pack`, zeros for the dropped rows).  No CPU fallback.
"""
import torch
from torch import Tensor

from warpconvnet_amd import _lib
from warpconvnet_amd.geometry.base.geometry import Geometry
from warpconvnet_amd.geometry.coords.integer import IntCoords
from warpconvnet_amd.utils.compile_guard import eager_unless_compiling


def cat_spatially_sparse_tensors(*sparse_tensors: Geometry) -> Geometry:
    """Concatenate the features of tensors on the same coordinates along the channel axis."""
    if len(sparse_tensors) == 0:
        raise ValueError("cat_spatially_sparse_tensors needs at least one tensor")
    offsets = sparse_tensors[0].offsets
    for st in sparse_tensors:
        o = st.offsets.to(offsets)
        if o.shape != offsets.shape or not torch.equal(o, offsets):
            raise ValueError("All sparse tensors must have the same offsets")
    feats = torch.cat([st.feature_tensor for st in sparse_tensors], dim=-1)
    return sparse_tensors[0].replace(batched_features=feats)


@eager_unless_compiling
def prune_spatially_sparse_tensor(spatial_tensor: Geometry, mask: Tensor) -> Geometry:
    """Keep the rows where ``mask`` is true (non-bool masks are cast); the number of batch elements is preserved."""
    from warpconvnet_amd.nn.functional.sparse_resample import ChildTable, _UnpackFunction, _expand

    n = spatial_tensor.coordinate_tensor.shape[0]
    if mask.shape[0] != n:
        raise ValueError(f"Mask length {mask.shape[0]} must match number of coordinates {n}")
    coords = spatial_tensor.batched_coordinates
    if not hasattr(coords, "prune"):
        raise TypeError(f"{coords.__class__.__name__} does not implement prune()")
    if not isinstance(coords, IntCoords) or coords.num_spatial_dims != 3:
        raise NotImplementedError("prune_spatially_sparse_tensor: the HIP path covers 3-D integer coordinates (Voxels)")
    _lib.require_gpu_tensor(spatial_tensor.batched_features.batched_tensor, "features")
    mask = mask.to(spatial_tensor.device)
    if mask.dtype != torch.bool:
        mask = mask.bool()
    bc = spatial_tensor.batch_indexed_coordinates
    if bc.dtype != torch.int32:
        bc = bc.to(torch.int32)
    kept, tbl, offsets = _expand(bc, mask.reshape(n, 1), 1, 1, _lib.WCN_SLOT_X_FASTEST, spatial_tensor.batch_size)
    table = ChildTable(tbl, _lib.WCN_SLOT_X_FASTEST, 1, 1, n, kept.shape[0])
    feats = _UnpackFunction.apply(spatial_tensor.feature_tensor, table, kept.shape[0], False)
    pruned = coords._like(kept[:, 1:].to(coords.batched_tensor.dtype), offsets.to(coords.offsets.dtype))
    extra = {k: v for k, v in spatial_tensor._extra_attributes.items() if k not in ("_cache", "_spatial_cache")}
    return spatial_tensor.__class__(pruned, feats, **extra)
