"""Voxel de-duplication of (real or integer) coordinates.

Reference: `warpconvnet/geometry/coords/ops/voxel.py:112` (``voxel_downsample_random_indices``): the
reference keeps an unspecified ("random") representative per voxel; this build keeps the FIRST row
of every voxel (smallest row index) so results are deterministic.
"""
from typing import Optional, Tuple

import torch
from torch import Tensor

from warpconvnet_amd.geometry.coords.ops.batch_index import (
    batch_indexed_coordinates,
    offsets_from_batch_index,
)


@torch.no_grad()
def voxel_downsample_random_indices(
    batched_points: Tensor, offsets: Tensor, voxel_size: Optional[float] = None
) -> Tuple[Tensor, Tensor]:
    """Returns ``(unique_row_indices sorted ascending, new CPU offsets)``."""
    from warpconvnet_amd.utils.unique import unique_first_indices

    if voxel_size is not None:
        coords = torch.floor(batched_points / voxel_size).to(torch.int32)
    else:
        coords = batched_points.to(torch.int32)
    bcoords = batch_indexed_coordinates(coords, offsets)
    idx = unique_first_indices(bcoords)
    new_offsets = offsets_from_batch_index(bcoords[idx, 0], num_batches=len(offsets) - 1)
    return idx, new_offsets


MAX_PACKED_BATCHES = 512


def _csr_mapping_torch(batched_points: Tensor, offsets: Tensor, voxel_size: float, unique_method):
    """Any device, any range: ``torch.unique`` over the (b, x, y, z) rows."""
    from warpconvnet_amd.geometry.coords.ops.batch_index import batch_index_from_offset
    from warpconvnet_amd.utils.unique import ToUnique

    cells = torch.floor(batched_points / voxel_size).to(torch.int32)
    bidx = batch_index_from_offset(offsets, device=cells.device)
    to_unique = ToUnique(unique_method=unique_method, return_to_unique_indices=True)
    rows = to_unique.to_unique(torch.cat([bidx.unsqueeze(1), cells], dim=1), dim=0)
    unique_offsets = offsets_from_batch_index(rows[:, 0], num_batches=len(offsets) - 1)
    return rows[:, 1:].contiguous(), unique_offsets, to_unique.to_csr_indices, to_unique.to_csr_offsets, to_unique


@torch.no_grad()
def voxel_downsample_csr_mapping(
    batched_points: Tensor, offsets: Tensor, voxel_size: float, unique_method: Optional[str] = None
) -> Tuple[Tensor, Tensor, Tensor, Tensor, "ToUnique"]:  # noqa: F821
    """Points -> voxels of edge ``voxel_size`` (reference `coords/ops/voxel.py:51-108`).

    Returns ``(unique_coords int32 [M, 3], unique_offsets CPU int32 [B + 1], to_csr_indices [N], to_csr_offsets [M + 1],
    to_unique)``: the voxels in ascending (b, x, y, z) order - the order of ``torch.unique(dim=0)`` - and inside a voxel
    the points in ascending row.  On the GPU the rows become packed int64 keys (``wcn_voxel_keys``), one stable radix sort
    orders them and ``wcn_voxel_map`` writes every map; the host reads once.  A cloud with a cell outside the packed range
    (|cell| >= 2^17, more than 512 batch elements) takes the torch row-unique path and gives the same result."""
    from warpconvnet_amd.utils.unique import ToUnique

    n, B = len(batched_points), len(offsets) - 1
    assert int(offsets[-1]) == n, f"Offsets {offsets} does not match the number of points {n}"
    packed = (batched_points.is_cuda and n > 0 and 1 <= B <= MAX_PACKED_BATCHES and batched_points.dtype == torch.float32
              and batched_points.ndim == 2 and batched_points.shape[1] == 3)
    if packed:
        info = _csr_mapping_hip(batched_points.contiguous(), offsets, float(voxel_size))
        if info is not None:
            ucoords, unique_offsets, uinfo = info
            return ucoords, unique_offsets, uinfo.to_csr_indices, uinfo.to_csr_offsets, ToUnique.from_info(uinfo, unique_method)
    return _csr_mapping_torch(batched_points, offsets, voxel_size, unique_method)


def _csr_mapping_hip(points: Tensor, offsets: Tensor, voxel_size: float):
    """The kernel route; None when a cell lies outside the packed range.  `wcn_voxel_keys` must quantise the way
    `torch.floor(points / voxel_size).int()` does ON THE DEVICE, bit for bit - `Points.sort`, `voxel_downsample` and the kernel
    maps all quantise that way: the device multiplies by fp32(1.0 / voxel_size), the quotient taken in double (the ctypes
    `c_float` conversion below rounds the Python double once, to nearest) - measured, DESIGN.md 4.19."""
    from warpconvnet_amd import _lib
    from warpconvnet_amd.utils.unique import voxel_map_from_keys, voxel_map_meta

    n, B, dev = points.shape[0], len(offsets) - 1, points.device
    meta = voxel_map_meta(B, dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    off_dev = offsets.to(device=dev, dtype=torch.int32)
    _lib.check(
        _lib.lib().wcn_voxel_keys(_lib.ptr(points), n, _lib.ptr(off_dev), B, 1.0 / voxel_size, _lib.ptr(keys), _lib.ptr(meta),
                                  _lib.stream_handle(dev)),
        "wcn_voxel_keys",
    )
    uinfo, _, ucoords, host = voxel_map_from_keys(keys, num_batches=B, meta=meta, decode=True)
    status = int(host[0])
    if status & 2:
        raise RuntimeError(f"voxel_downsample_csr_mapping: batch_offsets {offsets.tolist()} do not cover the {n} points")
    if status & 1:
        return None
    return ucoords, host[3:].clone(), uinfo
