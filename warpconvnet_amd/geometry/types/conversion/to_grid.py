"""Point clouds and voxels pooled onto a dense grid (reference `warpconvnet/geometry/types/conversion/to_grid.py`:
``points_to_grid``, ``voxels_to_grid``, ``points_to_closest_voxel_mapping`` with the same arguments).

    search_type="voxel"   every point belongs to the cell it falls into: `wcn_grid_point_keys` gives the flat cell id
                          (v_a = (p_a - lo_a) * (dims_a / (hi_a - lo_a)) clamped to [0, dims_a - 1] in float, so huge and
                          non-finite coordinates land in a valid cell), one stable sort groups the points, the offsets of all
                          B * H * W * D cells come from a search over the sorted ids (a known size: nothing is read back) and
                          `wcn_csr_gather_reduce` pools them.  Backward: `wcn_row_spread` (`ops/csr_rows.py`).
    "radius" / "knn"      the grid vertices query the points (`batched_radius_search` / `batched_knn_search`); the lists are
                          reduced by the same kernel.  The gradient reaches the point features through the transposed lists.

The reference loops over the grid cells in Python for radius / kNN and scatters with float atomics for ``voxel``; here the
three modes share one fixed-order kernel, so results are bitwise repeatable.  Divergences: ``max`` / ``min``
of a non-empty cell is the extremum of its points (the reference's voxel mode folds the initial 0 in), an empty cell is 0,
``voxels_to_grid`` applies the requested reduction (the reference overwrites in arbitrary order).  ``reduction="mul"`` is
served for CPU tensors only.  ``bounds=None`` pads the points' bounding box by 1 %.
"""
from typing import Literal, Optional, Tuple

import torch
from torch import Tensor
from torch.autograd import Function

from warpconvnet_amd.geometry.coords.grid import GridCoords
from warpconvnet_amd.geometry.features.grid import GridFeatures, GridMemoryFormat, as_memory_format, convert_from_standard_format
from warpconvnet_amd.ops.csr_rows import _CsrPool, csr_gather_reduce
from warpconvnet_amd.ops.reductions import _OP, REDUCTION_TYPES_STR, REDUCTIONS, _segment_cpu

__all__ = ["points_to_grid", "voxels_to_grid", "points_to_closest_voxel_mapping", "cell_ids"]


def _resolve_bounds(coords: Tensor, bounds: Optional[Tuple[Tensor, Tensor]]) -> Tuple[Tensor, Tensor]:
    if bounds is not None:
        return bounds[0].detach().float().cpu(), bounds[1].detach().float().cpu()
    lo, hi = coords.min(dim=0)[0].float().cpu(), coords.max(dim=0)[0].float().cpu()
    pad = (hi - lo) * 0.01
    return lo - pad, hi + pad


def cell_ids(coords: Tensor, offsets: Tensor, grid_shape: Tuple[int, int, int], bounds: Tuple[Tensor, Tensor]) -> Tensor:
    """int64 [N]: ``b * H * W * D + flat cell`` of every point (module docstring); GPU tensors through the key kernel."""
    from warpconvnet_amd.nn.functional.grid_sample import cell_scale, grid_point_keys

    coords = coords.float()
    if coords.is_cuda:
        return grid_point_keys(coords.contiguous(), offsets, grid_shape, bounds, corner=False)[0]
    dims = torch.tensor([int(g) for g in grid_shape])
    scale = torch.tensor(cell_scale(grid_shape, bounds), dtype=torch.float32)
    v = (coords - bounds[0].float()) * scale
    v = torch.minimum(torch.nan_to_num(v, nan=0.0, posinf=float("inf"), neginf=0.0).clamp_min(0.0), (dims - 1).float())
    v = v.to(torch.int64)
    counts = (offsets[1:] - offsets[:-1]).long()
    batch = torch.repeat_interleave(torch.arange(len(counts)), counts)
    return ((batch * dims[0] + v[:, 0]) * dims[1] + v[:, 1]) * dims[2] + v[:, 2]


def points_to_closest_voxel_mapping(points, grid_shape, bounds, memory_format=None) -> Tensor:
    """The flat cell id of every point (``memory_format`` is unused, kept like in the reference)."""
    return cell_ids(points.coordinate_tensor, points.offsets, grid_shape, _resolve_bounds(points.coordinate_tensor, bounds))


def _check_reduction(reduction, features: Tensor) -> str:
    op = reduction.value if isinstance(reduction, REDUCTIONS) else str(reduction)
    if op == "mul":
        if features.is_cuda:
            raise ValueError("reduction='mul' is served for CPU tensors only; on the GPU use sum, mean, max or min")
        return op
    if op not in _OP:
        raise ValueError(f"Unsupported reduction: {op} (sum, mean, max, min; mul on the CPU)")
    return op


def _segment_prod_cpu(gathered: Tensor, offsets: Tensor) -> Tensor:
    m = offsets.numel() - 1
    counts = (offsets[1:] - offsets[:-1]).long()
    seg = torch.repeat_interleave(torch.arange(m), counts)
    out = torch.ones((m, gathered.shape[1]), dtype=gathered.dtype)
    out = out.scatter_reduce(0, seg[:, None].expand_as(gathered), gathered, "prod", include_self=True)
    return out * (counts > 0).to(out.dtype).unsqueeze(1)


def _pool_cells(features: Tensor, ids: Tensor, num_cells: int, op: str) -> Tensor:
    """``features`` [N, C] reduced over the points of every cell: [num_cells, C], 0 for an empty cell."""
    sorted_ids, perm = torch.sort(ids, stable=True)
    offsets = torch.searchsorted(sorted_ids, torch.arange(num_cells + 1, device=ids.device))
    if op == "mul":
        return _segment_prod_cpu(features[perm], offsets)
    return _CsrPool.apply(features, perm, offsets, ids, op, -1)


def _row_major(t: Tensor) -> Tensor:
    """``t`` [N, C] with strides (C, 1): a one-column tensor counts as contiguous whatever its strides say."""
    t = t.contiguous()
    return t if t.stride() == (t.shape[1], 1) else t.reshape(-1).view(t.shape)


class _ListPool(Function):
    """``out[m] = op over j in [offsets[m], offsets[m + 1]) of features[indices[j]]`` where a row may sit in many lists
    (radius / kNN); backward = the same kernel over the transposed lists, fixed order, no atomics."""

    @staticmethod
    def forward(ctx, features: Tensor, indices: Tensor, offsets: Tensor, op: str):
        if features.is_cuda:
            res = csr_gather_reduce(_row_major(features), indices, offsets, op, return_arg=op in ("max", "min"))
            out, arg = res if isinstance(res, tuple) else (res, None)
        else:
            out, pos = _segment_cpu(features[indices], offsets, op)
            arg = None if pos is None else torch.where(pos >= 0, indices[pos.clamp_min(0)], pos)
        ctx.op, ctx.n = op, features.shape[0]
        ctx.save_for_backward(indices, offsets, arg if arg is not None else torch.empty(0))
        return out

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        indices, offsets, arg = ctx.saved_tensors
        dev = grad_out.device
        counts = offsets[1:] - offsets[:-1]
        entry_list = torch.repeat_interleave(torch.arange(counts.numel(), device=dev), counts, output_size=indices.numel())
        g = grad_out
        if ctx.op == "mean":
            g = g / counts.clamp_min(1).to(g.dtype).unsqueeze(1)
        sorted_rows, order = torch.sort(indices, stable=True)
        row_offsets = torch.searchsorted(sorted_rows, torch.arange(ctx.n + 1, device=dev))
        if ctx.op in ("max", "min"):  # an entry carries its list's gradient where it was the extremum
            src = g[entry_list] * (arg[entry_list] == indices.unsqueeze(1)).to(g.dtype)
            take = order
        else:
            src, take = g, entry_list[order]
        if g.is_cuda:
            return csr_gather_reduce(_row_major(src), take, row_offsets, "sum"), None, None, None
        return _segment_cpu(src[take], row_offsets, "sum")[0], None, None, None


def _pool_lists(features: Tensor, indices: Tensor, offsets: Tensor, op: str) -> Tensor:
    if op == "mul":
        return _segment_prod_cpu(features[indices], offsets)
    return _ListPool.apply(features, indices, offsets, op)


def _vertex_lists(points, grid_coords: GridCoords, search_type: str, search_radius: Optional[float], k: int):
    """CSR ``(indices, offsets)`` int64 of the points every grid vertex takes."""
    from warpconvnet_amd.geometry.coords.search.knn import knn_search
    from warpconvnet_amd.geometry.coords.search.radius import batched_radius_search

    ref = points.coordinate_tensor.float().contiguous()
    query = grid_coords.batched_tensor.to(ref.device).float().contiguous()
    if search_type == "radius":
        assert search_radius is not None, "Search radius must be provided for radius search"
        idx, _, splits = batched_radius_search(ref, points.offsets, query, grid_coords.offsets, search_radius)
        return idx.long(), splits.long()
    idx, counts = [], []
    for b in range(points.batch_size):  # per batch element: it may hold fewer than k points
        r0, r1 = int(points.offsets[b]), int(points.offsets[b + 1])
        q0, q1 = int(grid_coords.offsets[b]), int(grid_coords.offsets[b + 1])
        kb = min(k, r1 - r0)
        counts.append(torch.full((q1 - q0,), kb, dtype=torch.int64, device=ref.device))
        if kb > 0:
            idx.append((knn_search(ref[r0:r1], query[q0:q1], kb) + r0).reshape(-1))
    idx = torch.cat(idx) if idx else torch.zeros(0, dtype=torch.int64, device=ref.device)
    counts = torch.cat(counts)
    valid = idx >= 0
    if not bool(valid.all()):  # entries of -1 (no such neighbour) are dropped first
        entry_list = torch.repeat_interleave(torch.arange(counts.numel(), device=ref.device), counts)
        counts = torch.bincount(entry_list[valid], minlength=counts.numel())
        idx = idx[valid]
    return idx, torch.cat([counts.new_zeros(1), counts.cumsum(0)])


def _to_grid(standard: Tensor, grid_coords: GridCoords, memory_format: GridMemoryFormat):
    from warpconvnet_amd.geometry.types.grid import Grid

    shape, channels = grid_coords.grid_shape, standard.shape[-1]
    tensor = convert_from_standard_format(standard, memory_format, shape)
    return Grid(grid_coords, GridFeatures(tensor, grid_coords.offsets, memory_format, shape, channels))


def points_to_grid(
    points: "Points",  # noqa: F821
    grid_shape: Tuple[int, int, int],
    memory_format: Optional[GridMemoryFormat] = None,
    bounds: Optional[Tuple[Tensor, Tensor]] = None,
    search_radius: Optional[float] = None,
    k: int = 8,
    search_type: Literal["radius", "knn", "voxel"] = "radius",
    reduction: REDUCTION_TYPES_STR = "mean",
) -> "Grid":  # noqa: F821
    """The features of ``points`` reduced onto a grid of ``grid_shape`` vertices over ``bounds`` (module docstring)."""
    memory_format = GridMemoryFormat.b_x_y_z_c if memory_format is None else as_memory_format(memory_format)
    feats = points.feature_tensor
    op = _check_reduction(reduction, feats)
    h, w, d = (int(g) for g in grid_shape)
    batch = points.batch_size
    if search_type == "voxel":
        lo_hi = _resolve_bounds(points.coordinate_tensor, bounds)
        ids = cell_ids(points.coordinate_tensor, points.offsets, (h, w, d), lo_hi)
        pooled = _pool_cells(feats, ids, batch * h * w * d, op)
        grid_coords = GridCoords.from_shape((h, w, d), bounds=lo_hi, batch_size=batch, device=feats.device, flatten=True)
    elif search_type in ("radius", "knn"):
        grid_coords = GridCoords.from_shape((h, w, d), bounds=bounds, batch_size=batch, device=feats.device, flatten=True)
        indices, offsets = _vertex_lists(points, grid_coords, search_type, search_radius, k)
        pooled = _pool_lists(feats, indices, offsets, op)
    else:
        raise ValueError(f"Unsupported search type: {search_type}")
    return _to_grid(pooled.view(batch, h, w, d, feats.shape[1]), grid_coords, memory_format)


def voxels_to_grid(
    voxels: "Voxels",  # noqa: F821
    grid_shape: Tuple[int, int, int],
    grid_bounds: Optional[Tuple[Tensor, Tensor]] = None,
    memory_format: Optional[GridMemoryFormat] = None,
    search_type: Literal["voxel"] = "voxel",
    reduction: REDUCTION_TYPES_STR = "mean",
) -> "Grid":  # noqa: F821
    """Voxel features reduced onto the grid cell their integer coordinate falls into."""
    if search_type != "voxel":
        raise ValueError(f"Unsupported search type: {search_type}")
    memory_format = GridMemoryFormat.b_x_y_z_c if memory_format is None else as_memory_format(memory_format)
    feats = voxels.feature_tensor
    op = _check_reduction(reduction, feats)
    h, w, d = (int(g) for g in grid_shape)
    coords = voxels.coordinate_tensor.float()
    lo_hi = _resolve_bounds(coords, grid_bounds)
    ids = cell_ids(coords, voxels.offsets, (h, w, d), lo_hi)
    pooled = _pool_cells(feats, ids, voxels.batch_size * h * w * d, op)
    grid_coords = GridCoords.from_shape((h, w, d), bounds=lo_hi, batch_size=voxels.batch_size, device=feats.device, flatten=True)
    return _to_grid(pooled.view(voxels.batch_size, h, w, d, feats.shape[1]), grid_coords, memory_format)
