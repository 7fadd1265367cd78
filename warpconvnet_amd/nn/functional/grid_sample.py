"""Trilinear sampling of dense grids at point positions: ``grid_sample_points`` and the point <-> cell map it runs on.

    grid_sample_points(grid_or_factor_grid, points, backend="hip" | "torch")  ->  [N, sum C]

``backend="hip"`` (`csrc/grid.hip`): one launch per grid reads the grid in place through its five element strides, whatever
its memory format, and writes its columns of the ``[N, sum C]`` result directly; batches may be ragged.  The backward writes
every element of ``d_grid`` exactly once without float atomics, so two runs give the same bits.  ``backend="torch"`` is the
reference's composition (`nn/modules/factor_grid.py:250-279`): conversion to ``b_c_x_y_z``, ``F.grid_sample`` with
``align_corners=True, padding_mode="border"``, transposes and a ``cat`` - per batch element, so ragged batches work too.  It
is the path of CPU tensors and the yardstick the kernels are compared with.

The gradient goes to the grid features only; the point coordinates receive none (neither backend is asked for it by the
modules built on this, and the hip map treats the positions as geometry).

``GridSampleMap`` depends only on the point coordinates, the grid shape and the bounds: the corner keys and fractions
(`wcn_grid_point_keys`), one stable sort of the keys and the rows of every base cell.  It is built once per geometry and kept
in the points' ``_cache``; every call, every grid of that shape and both directions reuse it.
"""
from typing import List, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.autograd import Function

from warpconvnet_amd import _lib
from warpconvnet_amd.geometry.features.grid import GridMemoryFormat, grid_strides

__all__ = ["grid_sample_points", "GridSampleMap", "grid_point_keys", "grid_sample_raw", "grid_sample_backward_raw",
           "sample_scale", "cell_scale"]

_5L = _lib.c_int64 * 5
_3F = _lib.ctypes.c_float * 3


def _f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float64).to(torch.float32))


def sample_scale(dims: Sequence[int], bounds: Tuple[Tensor, Tensor]) -> List[float]:
    """``float32((dims - 1) / (hi - lo))`` per axis: the quotient in fp64, rounded once."""
    lo, hi = bounds[0].detach().double().cpu(), bounds[1].detach().double().cpu()
    return [_f32((int(dims[a]) - 1) / float(hi[a] - lo[a])) for a in range(3)]


def cell_scale(dims: Sequence[int], bounds: Tuple[Tensor, Tensor]) -> List[float]:
    """``float32(dims / (hi - lo))`` per axis (points -> grid pooling)."""
    lo, hi = bounds[0].detach().double().cpu(), bounds[1].detach().double().cpu()
    return [_f32(int(dims[a]) / float(hi[a] - lo[a])) for a in range(3)]


def grid_point_keys(coords: Tensor, offsets: Tensor, dims: Sequence[int], bounds: Tuple[Tensor, Tensor], corner: bool):
    """GPU: ``(keys int64 [N], fractions fp32 [N, 3] or None)`` of `wcn_grid_point_keys`."""
    _lib.require_gpu_tensor(coords, "coords")
    assert coords.dtype == torch.float32 and coords.ndim == 2 and coords.shape[1] == 3, "coords must be fp32 [N, 3]"
    assert all(float(bounds[1][a]) > float(bounds[0][a]) for a in range(3)), "bounds: max must exceed min on every axis"
    n, nb = coords.shape[0], len(offsets) - 1
    keys = torch.empty(n, dtype=torch.int64, device=coords.device)
    frac = torch.empty((n, 3), dtype=torch.float32, device=coords.device) if corner else None
    off = offsets.to(device=coords.device, dtype=torch.int64)
    lo = [_f32(float(v)) for v in bounds[0]]
    scale = sample_scale(dims, bounds) if corner else cell_scale(dims, bounds)
    _lib.check(
        _lib.lib().wcn_grid_point_keys(_lib.ptr(coords), n, _lib.ptr(off), nb, _lib.i3(dims), _3F(*lo), _3F(*scale),
                                       _lib.WCN_GRID_KEY_CORNER if corner else _lib.WCN_GRID_KEY_CELL, _lib.ptr(keys),
                                       _lib.ptr(frac), _lib.stream_handle(coords.device)),
        "wcn_grid_point_keys",
    )
    return keys, frac


class GridSampleMap:
    """The map between N points and the base cells of a grid of ``dims`` vertices over ``bounds`` (module docstring)."""

    def __init__(self, coords: Tensor, offsets: Tensor, dims: Sequence[int], bounds: Tuple[Tensor, Tensor]):
        self.dims = tuple(int(d) for d in dims)
        self.num_batches = len(offsets) - 1
        self.n = coords.shape[0]
        keys, self.fractions = grid_point_keys(coords.contiguous(), offsets, self.dims, bounds, corner=True)
        self.sorted_keys, self.perm = torch.sort(keys, stable=True)
        cells = self.num_batches
        for d in self.dims:
            cells *= max(d - 1, 1)
        # the rows of every cell: the array has a known size, nothing is read back for it
        self.cell_offsets = torch.searchsorted(self.sorted_keys, torch.arange(cells + 1, device=coords.device))
        chunk = _lib.lib().wcn_grid_chunk_points()
        # one host read per geometry: a map without crowded cells skips the chunk pass of every backward
        self.max_cell_points = self.n if self.n <= chunk else int((self.cell_offsets[1:] - self.cell_offsets[:-1]).max())


def _map_key(coords: Tensor, offsets: Tensor, dims, bounds):
    return ("grid_sample_map", coords.data_ptr(), coords.shape[0], coords._version, tuple(offsets.tolist()),
            tuple(int(d) for d in dims), tuple(bounds[0].tolist()), tuple(bounds[1].tolist()))


def sample_map_of(points, dims, bounds) -> GridSampleMap:
    """The cached ``GridSampleMap`` of a ``Points`` geometry (or of ``(coords, offsets)``)."""
    if isinstance(points, tuple):
        return GridSampleMap(points[0].float(), points[1], dims, bounds)
    coords = points.coordinate_tensor
    cache = points._extra_attributes.setdefault("_cache", {})
    key = _map_key(coords, points.offsets, dims, bounds)
    if key not in cache:
        cache[key] = GridSampleMap(coords.float(), points.offsets, dims, bounds)
    return cache[key]


def grid_sample_raw(grid: Tensor, strides: Sequence[int], dims: Sequence[int], channels: int, m: GridSampleMap, out: Tensor,
                    col0: int) -> None:
    """`wcn_grid_sample` into columns ``[col0, col0 + channels)`` of ``out`` [N, pitch]."""
    assert out.stride(1) == 1 and out.dtype == grid.dtype and out.shape[0] == m.n
    _lib.check(
        _lib.lib().wcn_grid_sample(_lib.ptr(grid), _5L(*[int(s) for s in strides]), _lib.i3(dims), channels,
                                   _lib.dtype_code(grid.dtype), m.num_batches, _lib.ptr(m.sorted_keys), _lib.ptr(m.perm),
                                   _lib.ptr(m.fractions), m.n, _lib.ptr(out), out.stride(0), col0,
                                   _lib.stream_handle(grid.device)),
        "wcn_grid_sample",
    )


def grid_sample_backward_raw(dy: Tensor, col0: int, d_grid: Tensor, strides: Sequence[int], dims: Sequence[int], channels: int,
                             m: GridSampleMap) -> None:
    """`wcn_grid_sample_backward`: every element of ``d_grid`` is written, the caller does not zero it."""
    assert dy.stride(1) == 1 and dy.dtype == d_grid.dtype
    L = _lib.lib()
    ws, ws_bytes = None, 0
    if m.max_cell_points > L.wcn_grid_chunk_points():
        ws_bytes = L.wcn_grid_sample_backward_workspace_bytes(m.n, channels)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dy.device)
    _lib.check(
        L.wcn_grid_sample_backward(_lib.ptr(dy), dy.stride(0), col0, _5L(*[int(s) for s in strides]), _lib.i3(dims), channels,
                                   _lib.dtype_code(dy.dtype), m.num_batches, _lib.ptr(m.sorted_keys), _lib.ptr(m.perm),
                                   _lib.ptr(m.cell_offsets), _lib.ptr(m.fractions), m.n, m.max_cell_points, _lib.ptr(d_grid),
                                   _lib.ptr(ws), ws_bytes, _lib.stream_handle(dy.device)),
        "wcn_grid_sample_backward",
    )


class _GridSampleHip(Function):
    """All grids of one call in one node: forward writes side by side into [N, sum C], backward one d_grid per grid, laid out
    like the grid it belongs to."""

    @staticmethod
    def forward(ctx, maps, metas, *tensors: Tensor):
        n = maps[0].n
        total = sum(c for _, c in metas)
        out = torch.empty((n, total), dtype=tensors[0].dtype, device=tensors[0].device)
        col = 0
        for t, m, (fmt, c) in zip(tensors, maps, metas):
            grid_sample_raw(t, grid_strides(t, fmt, c), m.dims, c, m, out, col)
            col += c
        ctx.maps, ctx.metas = maps, metas
        ctx.like = [(t.shape, t.stride(), t.dtype) for t in tensors]
        return out

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        g = grad_out if grad_out.stride(1) == 1 else grad_out.contiguous()
        grads, col = [], 0
        for i, (m, (fmt, c), (shape, stride, dtype)) in enumerate(zip(ctx.maps, ctx.metas, ctx.like)):
            if ctx.needs_input_grad[2 + i]:
                dg = torch.empty_strided(shape, stride, dtype=dtype, device=g.device) if _dense(shape, stride) else \
                    torch.empty(shape, dtype=dtype, device=g.device)
                gi = g if g.dtype == dtype else g.to(dtype)
                grid_sample_backward_raw(gi, col, dg, grid_strides(dg, fmt, c), m.dims, c, m)
                grads.append(dg)
            else:
                grads.append(None)
            col += c
        return (None, None, *grads)


def _dense(shape, stride) -> bool:
    """True when (shape, stride) covers its memory exactly once (a permuted contiguous tensor)."""
    expect = 1
    for size, st in sorted(((s, t) for s, t in zip(shape, stride) if s != 1), key=lambda p: p[1]):
        if st != expect:
            return False
        expect *= size
    return True


def _grids_of(grid_or_factor_grid) -> list:
    from warpconvnet_amd.geometry.types.grid import Grid

    if isinstance(grid_or_factor_grid, Grid):
        return [grid_or_factor_grid]
    return list(grid_or_factor_grid)


def _sample_torch(grid, coords: Tensor, offsets: Tensor) -> Tensor:
    """The reference's composition for one grid, per batch element: [N, C]."""
    feats = grid.grid_features.to_memory_format(GridMemoryFormat.b_c_x_y_z).batched_tensor
    lo, hi = (b.to(device=coords.device, dtype=coords.dtype) for b in grid.bounds)
    normalized = (coords - lo) / (hi - lo) * 2.0 - 1.0
    outs = []
    for b in range(len(offsets) - 1):
        xyz = normalized[int(offsets[b]):int(offsets[b + 1])]
        # grid_sample indexes its input (D_in, H_in, W_in) by (z, y, x) of the sampling position: b_c_x_y_z makes x the depth
        pos = xyz.flip(-1).view(1, -1, 1, 1, 3).to(feats.dtype)
        s = F.grid_sample(feats[b:b + 1], pos, mode="bilinear", padding_mode="border", align_corners=True)
        outs.append(s.view(feats.shape[1], -1).transpose(0, 1))
    return torch.cat(outs, dim=0) if outs else feats.new_zeros((0, feats.shape[1]))


def default_backend(device) -> str:
    return "hip" if torch.device(device).type == "cuda" else "torch"


def grid_sample_points(grid_or_factor_grid, points, backend: Optional[str] = None) -> Tensor:
    """Features of one ``Grid`` or of every grid of a ``FactorGrid``, interpolated trilinearly at the positions of ``points``
    (a ``Points`` geometry or ``(coords [N, 3], offsets [B + 1])``): ``[N, sum C]``, the grids side by side in their order.
    Positions outside the bounds take the border value.  The gradient goes to the grid features only."""
    grids = _grids_of(grid_or_factor_grid)
    coords, offsets = points if isinstance(points, tuple) else (points.coordinate_tensor, points.offsets)
    assert len(offsets) - 1 == grids[0].batch_size, "points and grid differ in batch size"
    if backend is None:
        backend = default_backend(grids[0].device)
    if backend == "torch":
        return torch.cat([_sample_torch(g, coords, offsets) for g in grids], dim=-1)
    if backend != "hip":
        raise ValueError(f"unknown backend {backend!r} (hip, torch)")
    tensors = [g.grid_features.batched_tensor for g in grids]
    if torch.is_autocast_enabled():
        amp = torch.get_autocast_dtype("cuda")
        tensors = [t if t.dtype == amp else t.to(amp) for t in tensors]
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"backend='hip' needs GPU tensors (got {t.device}); there is no CPU fallback")
        _lib.dtype_code(t.dtype)
        assert t.dtype == tensors[0].dtype, "the grids of one call share a dtype"
    maps = [sample_map_of(points, g.grid_shape, g.bounds) for g in grids]
    metas = [(g.memory_format, g.num_channels) for g in grids]
    return _GridSampleHip.apply(maps, metas, *tensors)
