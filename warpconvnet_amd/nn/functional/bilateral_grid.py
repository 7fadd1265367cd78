"""Sparse d-dimensional bilateral grid (Barron & Poole, "The Fast Bilateral Solver", arXiv:1511.03296): every point spreads
its feature over the 2^d corners of its grid cell with d-linear weights, a three-tap blur runs along each axis over the
populated cells, and the result is gathered back with the same weights.

Public surface of ``BilateralGrid`` / ``bilateral_filter_grid`` of the reference's ``nn/functional/bilateral_grid.py`` (the
solver built on the grid is not part of this package).  ``build`` takes ``backend="auto" | "torch" | "hip"`` (see
``_lattice.py``).  d <= 6: a point has at most 64 corners.

The blur along one axis is the reference's in-place chain, in which each step reads the previous step's result: with taps
(a, b, c) the centre is scaled by b, then c times the already scaled forward neighbour is added, then a times the backward
neighbour of that sum.  Here that is two passes over ping-pong buffers: ``y = b x + (c b) x[fwd]``, then ``y + a y[bwd]``.
"""
from itertools import product
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from warpconvnet_amd import _lib
from warpconvnet_amd.geometry.coords.search.packed128_hashmap import PackedHashTable128
from warpconvnet_amd.nn.functional import _lattice as lt
from warpconvnet_amd.nn.functional.permutohedral import bilateral_positions


def _corner_offsets(d: int, device) -> Tensor:
    """(2^d, d) int64: the corners of the unit d-cube, the last axis fastest."""
    return torch.tensor(list(product([0, 1], repeat=d)), dtype=torch.int64, device=device).reshape(2 ** d, d)


def _corner_geometry(positions: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """(floors int64 [N, d], keys int64 [N * 2^d, d], weights [N, 2^d]) with framework ops."""
    d = positions.shape[1]
    cells = torch.floor(positions)
    floors = cells.to(torch.int64)
    frac = (positions - cells).unsqueeze(1)  # [N, 1, d], in [0, 1)
    corners = _corner_offsets(d, positions.device)
    on = corners.unsqueeze(0).to(positions.dtype)  # [1, 2^d, d]
    weights = (on * frac + (1 - on) * (1 - frac)).prod(dim=-1)
    keys = (floors.unsqueeze(1) + corners.unsqueeze(0)).reshape(-1, d)
    return floors, keys, weights


class BilateralGrid(lt.SparseLattice):
    """Build once from positions (already divided by the bandwidth per axis), then ``filter`` any feature tensor of matching N,
    or use ``splat`` / ``blur`` / ``slice`` on their own.

    Attributes as the reference's: ``floors`` int64 (N, d), ``weights`` (N, 2^d), ``unique_keys`` int32 (V, d) in the row order
    of ``torch.unique(dim=0)``, ``inverse`` int64 (N 2^d,), ``d``, ``n_input``, ``hash_table`` (``None`` on the CPU),
    ``num_vertices``."""

    def __init__(self, floors: Tensor, weights: Tensor, unique_keys: Tensor, inverse: Tensor, d: int, n_input: int, hash_table,
                 backend: str = "torch", rows: Optional[lt.RowLists] = None):
        self.floors, self.weights, self.unique_keys, self.inverse = floors, weights, unique_keys, inverse
        self.d, self.n_input, self.hash_table, self.backend = d, n_input, hash_table, backend
        self._entry_weights, self._rows = weights, rows

    @classmethod
    @torch.no_grad()
    def build(cls, positions: Tensor, backend: str = "auto") -> "BilateralGrid":
        lt.check_positions(positions)
        backend = lt.pick_backend(backend, positions)
        n, d = positions.shape
        if backend == "hip":
            return cls._build_hip(positions.detach().float().contiguous())
        floors, keys, weights = _corner_geometry(positions.detach())
        if n and (int(keys.min()) < lt.COORD_MIN or int(keys.max()) > lt.COORD_MAX or not bool(torch.isfinite(weights).all())):
            raise lt.range_error("BilateralGrid.build")
        unique_keys, inverse = torch.unique(keys.to(torch.int32), dim=0, return_inverse=True)
        table = None
        if positions.is_cuda:
            table = PackedHashTable128.from_keys(unique_keys, capacity=max(16, 2 * unique_keys.shape[0]))
        return cls(floors, weights, unique_keys, inverse, d, n, table, "torch")

    @staticmethod
    def _geometry_hip(positions: Tensor, for_build: bool, status: Tensor):
        n, d = positions.shape
        dev = positions.device
        k = 1 << d
        floors = hi = lo = keys = None
        if for_build:
            floors = torch.empty((n, d), dtype=torch.int64, device=dev)
            lo = torch.empty(n * k, dtype=torch.int64, device=dev)
            hi = torch.empty_like(lo) if d * lt.COORD_BITS > 64 else None
        else:
            keys = torch.empty((n * k, d), dtype=torch.int32, device=dev)
        weights = torch.empty((n, k), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().wcn_grid_corners(_lib.ptr(positions), n, d, _lib.ptr(floors), _lib.ptr(hi), _lib.ptr(lo),
                                               _lib.ptr(keys), _lib.ptr(weights), _lib.ptr(status), _lib.stream_handle(dev)),
                   "wcn_grid_corners")
        return floors, hi, lo, keys, weights

    @classmethod
    def _build_hip(cls, positions: Tensor) -> "BilateralGrid":
        n, d = positions.shape
        status = torch.zeros(4, dtype=torch.int32, device=positions.device)
        floors, hi, lo, _, weights = cls._geometry_hip(positions, True, status)
        built = lt.hip_vertex_map(hi, lo, d, status)
        if built is None:
            raise lt.range_error("BilateralGrid.build")
        unique_keys, inverse, rows = built
        table = PackedHashTable128(max(16, 2 * unique_keys.shape[0]), positions.device, d)
        table._launch_insert(unique_keys, status)  # keys decoded from in-range, distinct fields: no flag can be raised
        return cls(floors, weights, unique_keys, inverse, d, n, table, "hip", rows)

    # -- what SparseLattice asks for -------------------------------------------------------------------------------------------
    def _neighbour_offsets(self) -> Tensor:
        step = torch.eye(self.d, dtype=torch.int32, device=self.unique_keys.device)
        return torch.stack([step, -step], dim=1).reshape(2 * self.d, self.d)

    def _passes(self, taps) -> List[lt.Pass]:
        a, b, c = (float(t) for t in taps)
        passes: List[lt.Pass] = []
        for axis in range(self.d):
            passes += [(2 * axis, -1, b, c * b, 0.0), (2 * axis + 1, -1, 1.0, a, 0.0)]
        return passes

    def _default_passes(self) -> List[lt.Pass]:
        return self._passes((0.5, 1.0, 0.5))

    def _query_geometry(self, query_positions: Tensor) -> Tuple[Tensor, Tensor]:
        if self.backend == "hip" and query_positions.is_cuda and query_positions.dtype in lt.HIP_DTYPES:
            status = torch.zeros(1, dtype=torch.int32, device=query_positions.device)  # a query outside the range is a miss
            _, _, _, keys, weights = self._geometry_hip(query_positions.detach().float().contiguous(), False, status)
            return keys, weights
        _, keys, weights = _corner_geometry(query_positions.detach())
        weights = torch.where(torch.isfinite(weights), weights, torch.zeros_like(weights))
        return keys.clamp(lt.COORD_MIN - 1, lt.COORD_MAX + 1).to(torch.int32), weights

    # -- the reference's operations --------------------------------------------------------------------------------------------
    def splat(self, features: Tensor) -> Tensor:
        """(N, F) -> (V, F): every feature over the 2^d corners of its cell."""
        return self._splat(features)

    def blur(self, lattice: Tensor, *, taps: Tuple[float, float, float] = (0.5, 1.0, 0.5)) -> Tensor:
        """(V, F) -> (V, F): the three-tap blur along every axis, unnormalised; absent neighbours read as zero."""
        return self._blur(lattice, self._passes(taps))

    def slice(self, lattice: Tensor) -> Tensor:
        """(V, F) -> (N, F): the d-linear gather at the build positions."""
        return self._slice(lattice)

    def _slice_at_query(self, lattice: Tensor, query_positions: Tensor) -> Tensor:
        q = self._query_entries(query_positions)
        return self._slice(lattice, q.index, q.weights)

    def filter(self, features: Tensor, *, query_positions: Optional[Tensor] = None, normalize: bool = True) -> Tensor:
        """splat -> blur -> slice with the default taps; ``normalize`` divides by a channel of ones carried along.  Corners of
        query cells that hold no vertex contribute zero.  A lattice built by the HIP back end runs the HIP kernels for
        float32 / float16 / bfloat16 features on its GPU; any other feature tensor (float64 in particular) silently takes the
        framework-op path over the same lattice arrays - correct, differentiable, and not the hot path."""
        return self._filter(features, query_positions, normalize)


def bilateral_filter_grid(src_xyz: Tensor, src_feat: Tensor, src_value: Tensor, *, sigma_xyz: float = 0.05,
                          sigma_feat: float = 20.0, backend: str = "auto") -> Tensor:
    """One-shot bilateral filter of ``src_value`` (N, V) on the grid over ``[xyz / sigma_xyz, feat / sigma_feat]``."""
    grid = BilateralGrid.build(bilateral_positions(src_xyz, src_feat, sigma_xyz, sigma_feat), backend=backend)
    return grid.filter(src_value, normalize=True)
