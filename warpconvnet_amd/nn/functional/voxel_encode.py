"""Voxels grouped into 3-D windows: the step that turns coordinates into the attention sequences of ``SpaceAttention``
(reference `nn/functional/voxel_encode.py`; names and signatures are the reference's).

``voxel_encode`` gives every voxel the integer code of its window and, on request, the permutation that sorts the rows by
(batch element, window), its inverse and the window lengths.  Three methods are implemented:

- ``"counting_sort"``: GPU tensors go through ``wcn_window_group`` (`csrc/window_group.hip`): codes + dense histogram,
  a three-launch prefix sum that also compacts the non-empty windows, a scatter and an in-LDS sort of every window's
  segment.  The host reads the device twice: the bounding box (to size the histogram) and ``(S, max_count)``.  CPU tensors,
  histograms above ``MAX_BINS`` and windows longer than ``wcn_window_group_max_segment()`` rows take the torch path with
  the same codes, and return the same integers.
- ``"ravel_fast"`` / ``"ravel"``: the torch path with the reference's code formulas (they differ from the counting-sort
  codes, not in the order they induce).
- ``"morton"`` raises ``NotImplementedError``.

The torch path is one ``torch.sort(batch * max_code + code, stable=True)`` and a ``unique_consecutive``.  Every path returns
``perm`` as the STABLE sort: inside a window rows appear in ascending original index, so two runs give the same bits (the
reference's counting sort takes its slots with a racy atomic and does not).
"""
import random
from dataclasses import dataclass
from typing import Literal, Optional, Tuple, Union

import torch
from torch import Tensor

from warpconvnet_amd import _lib

__all__ = ["STR2COORD_OFFSET", "WINDOW_OFFSET_TYPE", "VoxelEncodeResult", "voxel_encode", "voxel_encode_cached",
           "clear_encode_cache", "MAX_BINS"]

STR2COORD_OFFSET = {
    "random": (None, None, None),
    "zero": (0, 0, 0),
    "x": (0.5, 0, 0),
    "y": (0, 0.5, 0),
    "z": (0, 0, 0.5),
    "xy": (0.5, 0.5, 0),
    "xz": (0.5, 0, 0.5),
    "yz": (0, 0.5, 0.5),
    "xyz": (0.5, 0.5, 0.5),
}

WINDOW_OFFSET_TYPE = Literal["random", "zero", "x", "y", "z", "xy", "xz", "yz", "xyz"]

MAX_BINS = 4 * 1024 * 1024  # dense histogram bins (B * W) the counting sort takes; above: the torch path

_METHODS = ("morton", "ravel", "ravel_fast", "counting_sort")


@dataclass
class VoxelEncodeResult:
    """``codes`` [N] int64; ``perm`` [N] int64 sorts the rows by window (sorted = data[perm]); ``inverse_perm`` restores
    them; ``counts`` [S] int64 lengths of the non-empty windows in sorted order; ``cu_seqlens`` [S + 1] int32 their
    boundaries (ready for ``flash_attn_varlen_qkvpacked``); ``max_count`` the longest window (a host int).  Fields that were
    not asked for are None."""

    codes: Tensor
    perm: Optional[Tensor] = None
    inverse_perm: Optional[Tensor] = None
    counts: Optional[Tensor] = None
    cu_seqlens: Optional[Tensor] = None
    max_count: Optional[int] = None


# key -> (coords tensor, result).  The key is the reference's (data_ptr, rows, window, offset, method); the entry keeps the
# coords tensor alive, so its storage cannot be handed to another tensor while the key is live.
_ENCODE_CACHE: dict = {}


def clear_encode_cache():
    """Clear the voxel encode cache. Call at the start of each forward pass."""
    _ENCODE_CACHE.clear()


def _window3(window_size) -> Tuple[int, int, int]:
    assert window_size is not None, "window_size must be provided"
    if isinstance(window_size, int):
        window_size = (window_size, window_size, window_size)
    assert isinstance(window_size, (tuple, list)) and len(window_size) == 3, (
        "window_size must be an integer or a tuple of 3 integers")
    return tuple(int(w) for w in window_size)


def voxel_encode_cached(grid_coord: Tensor, batch_offsets: Optional[Tensor] = None,
                        window_size: Optional[Union[int, Tuple[int, int, int]]] = None,
                        coord_offset: Union[str, Tuple[float, float, float]] = (0.0, 0.0, 0.0),
                        encoding_method: str = "counting_sort") -> VoxelEncodeResult:
    """Cached ``voxel_encode`` with ``perm``, ``inverse_perm`` and ``counts``: one encode per (coords, window, offset,
    method).  ``coord_offset == "random"`` is never cached.  Call ``clear_encode_cache`` before each forward pass."""
    kwargs = dict(window_size=window_size, coord_offset=coord_offset, return_perm=True, return_inverse=True, return_counts=True,
                  encoding_method=encoding_method)
    if isinstance(coord_offset, str) and coord_offset == "random":
        return voxel_encode(grid_coord, batch_offsets, **kwargs)
    offset_key = coord_offset if isinstance(coord_offset, str) else tuple(float(x) for x in coord_offset)
    key = (grid_coord.data_ptr(), grid_coord.shape[0], _window3(window_size), offset_key, encoding_method)
    entry = _ENCODE_CACHE.get(key)
    if entry is None:
        entry = (grid_coord, voxel_encode(grid_coord, batch_offsets, **kwargs))
        _ENCODE_CACHE[key] = entry
    return entry[1]


def _batch_index(batch_offsets: Optional[Tensor], n: int, device) -> Optional[Tensor]:
    if batch_offsets is None:
        return None
    return torch.searchsorted(batch_offsets[1:].to(device=device, dtype=torch.int64), torch.arange(n, device=device),
                              side="right")


def _finish_torch(codes: Tensor, key: Tensor, return_perm: bool, return_inverse: bool, return_counts: bool) -> VoxelEncodeResult:
    """perm / inverse / counts of the torch path: a stable sort of ``key`` (batch element major, window code minor)."""
    n, dev = key.shape[0], key.device
    sorted_key, perm = torch.sort(key, stable=True)
    res = VoxelEncodeResult(codes=codes, perm=perm if return_perm else None)
    if return_inverse:
        inverse = torch.empty(n, dtype=torch.int64, device=dev)
        inverse[perm] = torch.arange(n, device=dev)  # perm is a permutation: every slot written once
        res.inverse_perm = inverse
    if return_counts:
        counts = torch.unique_consecutive(sorted_key, return_counts=True)[1]
        res.counts = counts
        res.cu_seqlens = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).to(torch.int32)
        res.max_count = int(counts.max())
    return res


def _counting_sort_codes_torch(grid_coord: Tensor, batch_offsets: Optional[Tensor], window: Tuple[int, int, int],
                               shift: Tensor) -> Tensor:
    """The counting sort's codes in torch: ``b * W + (wx * gs1 + wy) * gs2 + wz`` over the grid of the shifted bounding box."""
    dev, n = grid_coord.device, grid_coord.shape[0]
    ws = torch.tensor(window, dtype=torch.int64, device=dev)
    c = grid_coord.to(torch.int64)
    lo, hi = c.min(0).values, c.max(0).values
    gs = (hi - lo + shift.to(dev) + 1 + ws - 1) // ws
    w = (c + shift.to(dev) - lo) // ws
    code = (w[:, 0] * gs[1] + w[:, 1]) * gs[2] + w[:, 2]
    b = _batch_index(batch_offsets, n, dev)
    return code if b is None else b * (gs[0] * gs[1] * gs[2]) + code


def _counting_sort_hip(grid_coord: Tensor, batch_offsets: Optional[Tensor], window: Tuple[int, int, int],
                       shift: Tuple[int, int, int]) -> Optional[VoxelEncodeResult]:
    """The whole encode through ``wcn_window_group``, or None where the torch path has to take over: a histogram above
    ``MAX_BINS`` (known after the first host read) or a window longer than the in-LDS sort holds (known after the second)."""
    dev, n = grid_coord.device, grid_coord.shape[0]
    coords = grid_coord.to(torch.int32).contiguous()
    if batch_offsets is None:
        batch_offsets = torch.tensor([0, n], dtype=torch.int32)
    offs = batch_offsets.to(device=dev, dtype=torch.int32).contiguous()
    nb = offs.numel() - 1
    box = torch.stack(torch.aminmax(coords, dim=0)).cpu().tolist()  # host read 1 of 2: the bounding box
    lo, hi = box
    gs = [(hi[a] - lo[a] + shift[a] + 1 + window[a] - 1) // window[a] for a in range(3)]
    num_bins = nb * gs[0] * gs[1] * gs[2]
    if num_bins > MAX_BINS:
        return None
    L = _lib.lib()
    cap = min(n, num_bins)
    codes = torch.empty(n, dtype=torch.int64, device=dev)
    perm = torch.empty(n, dtype=torch.int64, device=dev)
    inverse = torch.empty(n, dtype=torch.int64, device=dev)
    cu = torch.empty(cap + 1, dtype=torch.int32, device=dev)
    counts = torch.empty(cap, dtype=torch.int64, device=dev)
    summary = torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(L.wcn_window_group_workspace_bytes(n, num_bins), dtype=torch.uint8, device=dev)
    _lib.check(
        L.wcn_window_group(_lib.ptr(coords), n, _lib.ptr(offs), nb, _lib.i3(window), _lib.i3(shift), _lib.i3(lo), _lib.i3(gs),
                           _lib.ptr(codes), _lib.ptr(perm), _lib.ptr(inverse), _lib.ptr(cu), _lib.ptr(counts),
                           _lib.ptr(summary), _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev)),
        "wcn_window_group",
    )
    s, max_count = summary.cpu().tolist()  # host read 2 of 2
    if s < 0:
        raise RuntimeError("voxel_encode: batch_offsets does not cover the rows of grid_coord")
    if max_count > L.wcn_window_group_max_segment():
        return None
    return VoxelEncodeResult(codes=codes, perm=perm, inverse_perm=inverse, counts=counts[:s], cu_seqlens=cu[:s + 1],
                             max_count=int(max_count))


@torch.no_grad()
def voxel_encode(grid_coord: Tensor, batch_offsets: Optional[Tensor] = None,
                 window_size: Optional[Union[int, Tuple[int, int, int]]] = None,
                 coord_offset: Union[str, Tuple[float, float, float]] = (0.0, 0.0, 0.0), return_perm: bool = False,
                 return_inverse: bool = False, return_counts: bool = False,
                 encoding_method: str = "ravel") -> Union[Tensor, VoxelEncodeResult]:
    """Integer codes shared by the voxels of one window.  ``grid_coord`` [N, 3] integers, ``batch_offsets`` [B + 1],
    ``window_size`` an int or 3 ints, ``coord_offset`` a shift of the window grid as 3 fractions of the window or a key of
    ``STR2COORD_OFFSET``.  Without a ``return_*`` flag the result is the ``codes`` tensor, otherwise a ``VoxelEncodeResult``."""
    dev = grid_coord.device
    wanted = return_perm or return_inverse or return_counts
    if grid_coord.shape[0] == 0:
        codes = torch.empty(0, dtype=torch.int64, device=dev)
        if not return_perm and not return_inverse:
            return codes
        empty = lambda on: torch.empty(0, dtype=torch.int64, device=dev) if on else None  # noqa: E731
        return VoxelEncodeResult(codes=codes, perm=empty(return_perm), inverse_perm=empty(return_inverse),
                                 counts=empty(return_counts),
                                 cu_seqlens=torch.zeros(1, dtype=torch.int32, device=dev) if return_counts else None,
                                 max_count=0 if return_counts else None)
    assert grid_coord.shape[1] == 3, "grid_coord must be a 3D tensor"
    assert encoding_method in _METHODS, (
        f"encoding_method must be 'morton', 'ravel', 'ravel_fast', or 'counting_sort', got {encoding_method}")
    if encoding_method == "morton":
        raise NotImplementedError("voxel_encode: encoding_method='morton' is not implemented (use 'counting_sort', "
                                  "'ravel_fast' or 'ravel')")
    if isinstance(coord_offset, str):
        if coord_offset == "random":
            coord_offset = (random.random(), random.random(), random.random())
        else:
            coord_offset = STR2COORD_OFFSET[coord_offset]
    assert isinstance(coord_offset, tuple) and len(coord_offset) == 3, "coord_offset must be a tuple of 3 floats"
    window = _window3(window_size)
    ws_cpu = torch.tensor(window, dtype=torch.int32)
    shift_cpu = torch.round(torch.tensor(coord_offset, dtype=torch.float32) * ws_cpu.float()).int()  # host arithmetic
    n = grid_coord.shape[0]

    if encoding_method == "counting_sort":
        if grid_coord.is_cuda:
            res = _counting_sort_hip(grid_coord, batch_offsets, window, tuple(shift_cpu.tolist()))
            if res is not None:
                if not wanted:
                    return res.codes
                if not return_perm:
                    res.perm = None
                if not return_inverse:
                    res.inverse_perm = None
                if not return_counts:
                    res.counts = res.cu_seqlens = res.max_count = None
                return res
        codes = _counting_sort_codes_torch(grid_coord, batch_offsets, window, shift_cpu.long())
        if not wanted:
            return codes
        return _finish_torch(codes, codes, return_perm, return_inverse, return_counts)

    shift, ws = shift_cpu.to(dev), ws_cpu.to(dev)
    min_coord = grid_coord.min(dim=0).values.int()
    voxel_coord = ((grid_coord + shift - min_coord) // ws).long()
    if encoding_method == "ravel":  # the ravel over the box of the WINDOW coordinates, their minimum taken off again
        voxel_coord = voxel_coord - voxel_coord.min(dim=0).values
    shape = voxel_coord.max(dim=0).values + 1
    codes = (voxel_coord[:, 0] * shape[1] + voxel_coord[:, 1]) * shape[2] + voxel_coord[:, 2]
    if not wanted:
        return codes
    b = _batch_index(batch_offsets, n, dev)
    key = codes if b is None else b * (codes.max() + 1) + codes
    return _finish_torch(codes, key, return_perm, return_inverse, return_counts)
