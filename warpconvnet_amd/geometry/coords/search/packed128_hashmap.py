"""Packed 128-bit coordinate hash table on the GPU: keys of up to 7 axes of 17 bits.

Public surface of the reference's ``PackedHashTable128`` (`warpconvnet/geometry/coords/search/packed128_hashmap.py`):
``DIM``, ``COORD_BITS``, ``COORD_MIN`` / ``COORD_MAX``, ``MAX_BATCHED_K``, ``from_keys``, ``insert``, ``search``,
``batched_search``, ``key_dim``, ``capacity`` (a power of two), ``num_entries``.  Keys narrower than 7 axes behave as if
zero-padded.  The caller guarantees DISTINCT keys (run ``torch.unique`` upstream): insertion does not deduplicate.

Differences by design, in the style of ``PackedHashTable``:

* the range check always runs, on the device, and a coordinate outside [-65536, 65535] raises ``ValueError`` (the reference
  hides the check behind an environment variable and otherwise truncates the key);
* a table without room for the keys raises ``RuntimeError``;
* both are reported through one device status word and one host read.

AMD GPUs have no 128-bit compare-and-swap.  A slot is claimed by a 32-bit CAS on its *value* word (-1 -> row index) under
linear probing and the two key words are then written with a plain 16-byte store; an inserting thread never compares keys, a
claimed slot is simply skipped.  That is correct because keys are distinct by contract and searches run in a later launch.
"""
from typing import Optional, Union

import torch
from torch import Tensor

from warpconvnet_amd import _lib


def _next_power_of_2(n: int) -> int:
    return 1 if n <= 1 else 1 << (int(n) - 1).bit_length()


class PackedHashTable128:
    DIM = 7
    COORD_BITS = 17
    COORD_MIN = -(1 << (COORD_BITS - 1))  # -65536
    COORD_MAX = (1 << (COORD_BITS - 1)) - 1  # 65535
    MAX_BATCHED_K = 32

    def __init__(self, capacity: int, device: Union[str, torch.device] = "cuda", key_dim: int = DIM):
        if not (1 <= key_dim <= self.DIM):
            raise ValueError(f"key_dim must be in [1, {self.DIM}]; got {key_dim}")
        self._capacity = _next_power_of_2(max(int(capacity), 1))
        self._device = torch.device(device)
        self._key_dim = int(key_dim)
        self._keys: Optional[Tensor] = None  # int64 [capacity, 2]
        self._values: Optional[Tensor] = None  # int32 [capacity], -1 = empty
        self._num_entries = 0

    @property
    def capacity(self) -> int:
        return self._capacity

    @property
    def key_dim(self) -> int:
        """Logical key width; narrower keys behave as if zero-padded to ``DIM`` axes."""
        return self._key_dim

    @property
    def num_entries(self) -> int:
        return self._num_entries

    @property
    def device(self) -> torch.device:
        return self._keys.device if self._keys is not None else self._device

    @classmethod
    def from_keys(cls, coords: Tensor, device: Union[str, torch.device, None] = None, capacity: Optional[int] = None,
                  key_dim: Optional[int] = None) -> "PackedHashTable128":
        target = torch.device(device) if device is not None else coords.device
        if key_dim is None:
            key_dim = int(coords.shape[1])
        if not (1 <= key_dim <= cls.DIM):
            raise ValueError(f"key_dim must be in [1, {cls.DIM}]; got {key_dim}")
        if coords.shape[1] != key_dim:
            raise ValueError(f"coords width {coords.shape[1]} != key_dim {key_dim}")
        cap = capacity if capacity is not None else max(16, coords.shape[0] * 2)
        obj = cls(capacity=cap, device=target, key_dim=key_dim)
        obj.insert(coords.to(device=target))
        return obj

    def _check(self, t: Tensor, what: str) -> Tensor:
        if t.ndim != 2 or t.shape[1] != self._key_dim:
            raise ValueError(f"{what} must be (N, {self._key_dim}); got {tuple(t.shape)}")
        if not t.is_cuda:
            raise RuntimeError("PackedHashTable128 lives on the GPU (HIP path, no CPU fallback); got a CPU tensor")
        return t.to(dtype=torch.int32).contiguous()

    def _launch_insert(self, coords: Tensor, status: Tensor) -> None:
        """Clear + insert, asynchronous; flags are OR-ed into ``status[0]`` (int32, cleared by the caller)."""
        dev = coords.device
        self._keys = torch.empty((self._capacity, 2), dtype=torch.int64, device=dev)
        self._values = torch.empty(self._capacity, dtype=torch.int32, device=dev)
        _lib.check(
            _lib.lib().wcn_hash128_insert(_lib.ptr(self._keys), _lib.ptr(self._values), self._capacity, _lib.ptr(coords),
                                          coords.shape[0], self._key_dim, _lib.ptr(status), _lib.stream_handle(dev)),
            "wcn_hash128_insert",
        )
        self._num_entries = coords.shape[0]

    def insert(self, coords: Tensor) -> None:
        coords = self._check(coords, "coords")
        n = coords.shape[0]
        # no launch: every thread left over once the table is full would probe all of its slots before giving up.  So the
        # kernel's WCN_FLAG_TABLE_FULL (checked below all the same) is only ever raised for direct callers of the C ABI
        if n > self._capacity:
            raise RuntimeError(f"PackedHashTable128.insert failed: hash table is full (num_keys={n}, "
                               f"capacity={self._capacity}). Increase capacity.")
        status = torch.zeros(1, dtype=torch.int32, device=coords.device)
        self._launch_insert(coords, status)
        flags = int(status.item())  # the single host read
        if flags & _lib.WCN_FLAG_COORD_RANGE:
            self._keys = self._values = None
            self._num_entries = 0
            raise ValueError(f"Coord out of range [{self.COORD_MIN}, {self.COORD_MAX}]")
        if flags & _lib.WCN_FLAG_TABLE_FULL:
            raise RuntimeError(f"PackedHashTable128.insert failed: hash table is full (num_keys={n}, "
                               f"capacity={self._capacity}). Increase capacity.")

    def _search(self, queries: Tensor, offsets: Optional[Tensor], k: int) -> Tensor:
        if self._keys is None:
            raise RuntimeError("Call insert() first")
        m = queries.shape[0]
        out = torch.empty((k, m), dtype=torch.int32, device=queries.device)
        _lib.check(
            _lib.lib().wcn_hash128_search(_lib.ptr(self._keys), _lib.ptr(self._values), self._capacity, _lib.ptr(queries),
                                          _lib.ptr(offsets), m, k, self._key_dim, _lib.ptr(out),
                                          _lib.stream_handle(queries.device)),
            "wcn_hash128_search",
        )
        return out

    def search(self, queries: Tensor) -> Tensor:
        """int32 [M]: row index of each query key in the inserted tensor, -1 on a miss (or a key outside the range)."""
        return self._search(self._check(queries, "queries"), None, 1)[0]

    def batched_search(self, queries: Tensor, offsets: Tensor) -> Tensor:
        """int32 [K, M]: ``result[k, i]`` = row of ``queries[i] + offsets[k]`` or -1; one launch, K in [1, 32]."""
        queries, offsets = self._check(queries, "queries"), self._check(offsets, "offsets")
        k = offsets.shape[0]
        if not (1 <= k <= self.MAX_BATCHED_K):
            raise ValueError(f"K={k} out of range [1, {self.MAX_BATCHED_K}]")
        return self._search(queries, offsets, k)
