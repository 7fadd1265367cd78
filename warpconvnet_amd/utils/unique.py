"""Coordinate de-duplication.

Reference: `warpconvnet/utils/unique.py:124-143` (``unique_hashmap``: hash-insert then
``torch.unique`` of the winner indices).  On the GPU this build uses its own HIP hash table
(insert keeps the smallest row index per key, so the result is deterministic); on the CPU it
uses a lexicographic sort.  Both return the ascending row indices of first occurrences.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch import Tensor


@torch.no_grad()
def unique_first_indices(bcoords: Tensor) -> Tensor:
    """bcoords [N, 4|3] int -> int64 ascending indices of the first occurrence of every distinct row."""
    if bcoords.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int64, device=bcoords.device)
    if bcoords.is_cuda:
        return unique_hashmap(bcoords)[0]
    _, inverse = torch.unique(bcoords, dim=0, return_inverse=True)
    n = bcoords.shape[0]
    first = torch.full((int(inverse.max()) + 1,), n, dtype=torch.int64)
    first.scatter_reduce_(0, inverse, torch.arange(n, dtype=torch.int64), reduce="amin")
    return torch.sort(first).values


@torch.no_grad()
def unique_hashmap(bcoords: Tensor, **kwargs) -> Tuple[Tensor, "PackedHashTable"]:  # noqa: F821
    """GPU path: returns ``(unique_indices int64 ascending, table)`` (reference signature)."""
    from warpconvnet_amd.geometry.coords.search.packed_hashmap import PackedHashTable

    assert bcoords.is_cuda, f"Batched coordinates must be on a GPU device, got {bcoords.device}"
    if bcoords.shape[1] == 3:
        bcoords = torch.nn.functional.pad(bcoords, (0, 1), value=0)
    table = PackedHashTable.from_coords(bcoords, device=bcoords.device)
    return table.unique_index, table


_ARANGE = {}


def arange_i32(n: int, dev) -> Tensor:
    """``torch.arange(n, int32)`` on ``dev``, kept per size (read-only by contract): identity pair lists and first-occurrence
    tests ask for the same few sizes every iteration."""
    key = (int(n), str(dev))
    t = _ARANGE.get(key)
    if t is None:
        if len(_ARANGE) >= 32:
            _ARANGE.clear()
        t = _ARANGE[key] = torch.arange(n, dtype=torch.int32, device=dev)
    return t


@torch.no_grad()
def unique_first_indices_with_offsets(bcoords: Tensor) -> Tuple[Tensor, Tensor]:
    """GPU: ``(ascending int64 rows of the first occurrence of every distinct [b, x, y, z] row, CPU int32 offsets [B+1] of
    the surviving rows per batch index)`` with ONE host read.

    The generic route (`unique_hashmap` -> `PackedHashTable.insert` -> `unique_index` -> `offsets_from_batch_index`) reads
    the status word, the number of survivors and the per-batch counts back separately - three queue-draining waits per
    strided convolution; here the status word and a 512-bin per-batch histogram of the survivors travel together and the
    index list is compacted with a known size (`nonzero_static`)."""
    from warpconvnet_amd.geometry.coords.search.packed_hashmap import PackedHashTable

    assert bcoords.is_cuda and bcoords.ndim == 2 and bcoords.shape[1] == 4
    coords = bcoords.contiguous().to(torch.int32)
    n, dev = coords.shape[0], coords.device
    table = PackedHashTable(max(16, 2 * n), device=dev)
    meta = torch.zeros(1 + PackedHashTable.BATCH_MAX + 1, dtype=torch.int32, device=dev)  # [status, counts[512]]
    table._launch_insert(coords, meta[:1])
    first = table.search(coords) == arange_i32(n, dev)
    b = coords[:, 0].long().clamp_(0, PackedHashTable.BATCH_MAX)  # out-of-range batch ids are reported through the status
    meta[1:].index_add_(0, b, first.to(torch.int32))
    host = meta.cpu()  # the one host read
    PackedHashTable.raise_for_flags(int(host[0]), n, table.capacity)
    counts = host[1:]
    nz = torch.nonzero(counts)
    num_batches = int(nz[-1]) + 1 if len(nz) else 0
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), counts[:num_batches].to(torch.int64).cumsum(0)]).to(torch.int32)
    idx = torch.nonzero_static(first, size=int(offsets[-1])).squeeze(1)
    return idx, offsets


# ---- point <-> voxel maps ------------------------------------------------------------------------------------------------------
@dataclass
class UniqueInfo:
    """The map between N rows and their M distinct values (reference `utils/unique.py:146-151`).  ``max_segment`` is this
    build's addition: the longest CSR segment when the builder knows it (the pooling kernel skips its chunk passes for short
    segments), -1 when it does not."""

    to_orig_indices: Tensor          # [N] int64: unique[to_orig_indices] == x
    to_csr_indices: Tensor           # [N] int64: rows grouped by value, ascending row inside a group
    to_csr_offsets: Tensor           # [M + 1] int64
    to_unique_indices: Optional[Tensor]  # [M] int64: x[to_unique_indices] == unique, the FIRST (smallest) row of every value
    max_segment: int = -1


def _csr_from_inverse(inverse: Tensor, counts: Tensor) -> UniqueInfo:
    """Plain torch: the CSR of an inverse map (any device); the first row of a group is its smallest, because the argsort is
    stable."""
    csr_indices = torch.argsort(inverse, stable=True)
    csr_offsets = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    first = csr_indices[csr_offsets[:-1]]
    return UniqueInfo(inverse, csr_indices, csr_offsets, first)


def voxel_map_meta(num_batches: int, device) -> Tensor:
    """The words one map build sends to the host: [status of the key kernel, M, longest segment, voxel offsets [B + 1]]."""
    return torch.zeros(3 + num_batches + 1, dtype=torch.int32, device=device)


def voxel_map_from_keys(keys: Tensor, num_batches: int = 0, meta: Optional[Tensor] = None, decode: bool = False):
    """GPU: int64 ``keys`` [N] -> ``(UniqueInfo, unique_keys [M], unique_coords [M, 3] or None, host words)`` through a stable
    radix sort of the keys and ``wcn_voxel_map`` (`csrc/voxelize.hip`).  The host words - the status word of the key kernel,
    M, the longest segment and the voxel offsets of the ``num_batches`` batch elements (`voxel_map_meta`; pass the tensor the key
    kernel wrote its status into) - come back in ONE read."""
    from warpconvnet_amd import _lib

    assert keys.is_cuda and keys.ndim == 1 and keys.dtype == torch.int64
    n, dev = keys.numel(), keys.device
    if meta is None:
        meta = voxel_map_meta(num_batches, dev)
    skeys, perm = torch.sort(keys, stable=True)
    ukeys = torch.empty(n, dtype=torch.int64, device=dev)
    ucoords = torch.empty((n, 3), dtype=torch.int32, device=dev) if decode else None
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    to_orig = torch.empty(n, dtype=torch.int64, device=dev)
    first = torch.empty(n, dtype=torch.int64, device=dev)
    L = _lib.lib()
    ws_bytes = L.wcn_voxel_map_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(
        L.wcn_voxel_map(_lib.ptr(skeys), _lib.ptr(perm), n, num_batches, _lib.ptr(ukeys), _lib.ptr(ucoords), _lib.ptr(offsets),
                        _lib.ptr(to_orig), _lib.ptr(first), _lib.ptr(meta[3:]) if num_batches else None, _lib.ptr(meta[1:]),
                        _lib.ptr(ws), ws_bytes, _lib.stream_handle(dev)),
        "wcn_voxel_map",
    )
    host = meta.cpu()  # the one host read
    m = int(host[1])
    info = UniqueInfo(to_orig, perm, offsets[: m + 1], first[:m], max_segment=int(host[2]))
    return info, ukeys[:m], (ucoords[:m] if decode else None), host


class ToUnique:
    """Distinct values of a tensor and the maps between the rows and them (reference `utils/unique.py:154-240`, same
    methods and properties).

    A 1-D integer tensor on the GPU (codes, packed voxel keys) is de-duplicated by a stable sort and ``wcn_voxel_map``;
    everything else - CPU tensors, rows of several columns - by ``torch.unique``.  Either way the values come out ascending
    (rows: lexicographic), ``to_csr_indices`` lists the rows of every value in ascending order and ``to_unique_indices`` is
    the FIRST row of every value (`coords/ops/voxel.py`; the reference leaves the choice to a scatter and so to the device).

    ``unique_method`` is accepted for compatibility: ``"torch"``, ``"ravel"`` and ``"morton"`` all give this one order.  The
    reference's ``morton`` order exists only on its CUDA path and nothing consumes it - every caller uses the maps, not the
    order.  ``to_unique_indices`` is always filled in (it costs nothing here), whatever ``return_to_unique_indices`` says.
    """

    unique_info: UniqueInfo

    def __init__(self, unique_method: Optional[str] = "torch", return_to_unique_indices: bool = False):
        self.unique_method = unique_method or "torch"
        assert self.unique_method in ("torch", "ravel") or self.unique_method.startswith("morton"), (
            f"Given unique method '{self.unique_method}' - must be one of torch, ravel, morton"
        )
        self.return_to_unique_indices = return_to_unique_indices

    @classmethod
    def from_info(cls, info: UniqueInfo, unique_method: Optional[str] = "torch") -> "ToUnique":
        out = cls(unique_method=unique_method, return_to_unique_indices=True)
        out.unique_info = info
        return out

    @torch.no_grad()
    def to_unique(self, x: Tensor, dim: int = 0) -> Tensor:
        if x.is_cuda and x.ndim == 1 and x.numel() > 0 and not x.dtype.is_floating_point and x.dtype != torch.bool:
            self.unique_info, unique, _, _ = voxel_map_from_keys(x.to(torch.int64).contiguous())
            return unique.to(x.dtype)
        unique, inverse, counts = torch.unique(x, dim=dim, sorted=True, return_inverse=True, return_counts=True)
        self.unique_info = _csr_from_inverse(inverse, counts)
        return unique

    def to_unique_csr(self, x: Tensor, dim: int = 0) -> Tuple[Tensor, Tensor, Tensor]:
        """``(unique, to_csr_indices, to_csr_offsets)``: ``x[to_csr_indices]`` is ``unique`` with every value repeated
        ``to_csr_offsets.diff()`` times."""
        unique = self.to_unique(x, dim=dim)
        return unique, self.unique_info.to_csr_indices, self.unique_info.to_csr_offsets

    def to_original(self, unique: Tensor) -> Tensor:
        return unique[self.unique_info.to_orig_indices]

    @property
    def to_unique_indices(self) -> Tensor:
        return self.unique_info.to_unique_indices

    @property
    def to_csr_indices(self) -> Tensor:
        return self.unique_info.to_csr_indices

    @property
    def to_csr_offsets(self) -> Tensor:
        return self.unique_info.to_csr_offsets

    @property
    def to_orig_indices(self) -> Tensor:
        return self.unique_info.to_orig_indices
