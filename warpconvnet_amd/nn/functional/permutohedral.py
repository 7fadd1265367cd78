"""Permutohedral lattice filter (Adams, Baek, Davis 2010, "Fast High-Dimensional Filtering Using the Permutohedral Lattice").

splat: every point spreads its feature over the d + 1 vertices of the lattice simplex that encloses it, by barycentric
weight.  blur: a (1/2, 1, 1/2) pass along each of the d + 1 lattice axes; the neighbours of a vertex along axis a differ by
-d on that axis and +1 on every other one.  slice: the barycentric gather at the output positions, times 1 / (1 + 2^-(d+1)).

Public surface of the reference's ``nn/functional/permutohedral.py``.  Keys hold d + 1 <= 7 axes, so d <= 6.  ``build`` takes
``backend="auto" | "torch" | "hip"`` (see ``_lattice.py``); the HIP path computes the geometry in one kernel, the unique
vertices by a radix sort of packed keys, and keeps the neighbour table on the lattice, so ``filter`` never searches.  Unlike
the reference the result is bitwise reproducible in both directions (no float atomics), the lattice width is not padded to
dodge a slow framework gather, and positions that leave the 17-bit key range raise ``ValueError``.
"""
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from warpconvnet_amd import _lib
from warpconvnet_amd.geometry.coords.search.packed128_hashmap import PackedHashTable128
from warpconvnet_amd.nn.functional import _lattice as lt


def _embed_scale(d: int, dtype: torch.dtype, device) -> Tensor:
    """Per-axis factors of the embedding: (d + 1) sqrt(2/3) / sqrt((i + 1)(i + 2)), one lattice cell per unit of input.

    The reference writes ``scalar / torch.sqrt(...)``, which the framework evaluates as ``sqrt(...).reciprocal() * scalar``:
    three roundings in the tensor's dtype.  The float32 result of that expression was seen to differ in its last bit between two
    hosts (d = 6, last axis), and one ulp of a factor moves most barycentric weights by several ulps.  So the table is formed
    on the host, for both back ends, by the same three steps carried out in float64 and rounded to float32 after each - every
    one of them then is the correctly rounded float32 operation, on any host.  float64 positions take the float64 steps."""
    steps = torch.arange(1, d + 1, dtype=torch.float64)
    numerator = torch.tensor((d + 1) * (2.0 / 3.0) ** 0.5, dtype=torch.float64)
    if dtype == torch.float64:
        return ((1.0 / torch.sqrt(steps * (steps + 1))) * numerator).to(device)
    root = torch.sqrt(steps * (steps + 1)).float()
    reciprocal = (1.0 / root.double()).float()
    return (reciprocal.double() * numerator.float().double()).float().to(device=device, dtype=dtype)


def _embed_lattice(features: Tensor) -> Tensor:
    """(N, d) -> (N, d + 1) coordinates on the hyperplane of coordinate sum 0 (the `elevated` step of Adams' code)."""
    n, d = features.shape
    scaled = features * _embed_scale(d, features.dtype, features.device)
    out = torch.empty((n, d + 1), dtype=features.dtype, device=features.device)
    running = torch.zeros(n, dtype=features.dtype, device=features.device)
    for i in range(d, 0, -1):
        column = scaled[:, i - 1]
        out[:, i] = running - i * column
        running = running + column
    out[:, 0] = running
    return out


def _find_enclosing_simplex(elevated: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """(greedy int64 (N, d + 1): the nearest lattice vertex of coordinate sum 0; rank int64 (N, d + 1): a permutation of
    0..d, the position of each axis when the residuals are ordered descending, ties to the lower axis; barycentric weights
    (N, d + 1), summing to 1)."""
    n, dp1 = elevated.shape
    d = dp1 - 1
    inv = 1.0 / dp1
    cells = elevated * inv
    above, below = torch.ceil(cells) * dp1, torch.floor(cells) * dp1
    nearest = torch.where((above - elevated) < (elevated - below), above, below)
    greedy = nearest.to(torch.int64)
    excess = greedy.sum(dim=-1) // dp1  # how many steps of d + 1 the vertex is off the hyperplane

    residual = elevated - nearest
    bigger = residual.unsqueeze(1) > residual.unsqueeze(2)  # [n, j, q]: residual[q] > residual[j]
    equal_lower = (residual.unsqueeze(1) == residual.unsqueeze(2)) & torch.ones(dp1, dp1, dtype=torch.bool,
                                                                                device=elevated.device).tril(-1)
    rank = (bigger | equal_lower).sum(dim=-1)

    too_high = rank >= (dp1 - excess.clamp(min=0)).unsqueeze(-1)
    too_low = rank < (-excess).clamp(min=0).unsqueeze(-1)
    shift = (too_low.to(torch.int64) - too_high.to(torch.int64)) * dp1
    greedy = greedy + shift
    rank = rank + excess.unsqueeze(-1) + shift

    delta = (elevated - greedy.to(elevated.dtype)) * inv
    by_rank = delta.gather(1, torch.argsort(rank, dim=-1))  # by_rank[:, r] = delta of the axis with rank r
    bary = torch.empty_like(delta)
    if d >= 1:
        bary[:, 1:] = by_rank[:, :d].flip(-1) - by_rank[:, 1:].flip(-1)  # weight t = delta(rank d - t) - delta(rank d + 1 - t)
    bary[:, 0] = (by_rank[:, d] + 1.0) - by_rank[:, 0]
    return greedy, rank, bary


def _canonical_simplex_offsets(d: int, device) -> Tensor:
    """(d + 1, d + 1) int64: what vertex k adds to an axis of rank r: k while r <= d - k, k - (d + 1) after."""
    k = torch.arange(d + 1, device=device).unsqueeze(1)
    r = torch.arange(d + 1, device=device).unsqueeze(0)
    return torch.where(r <= d - k, k, k - (d + 1)).to(torch.int64)


def _simplex_keys(positions: Tensor) -> Tuple[Tensor, Tensor]:
    """(keys int64 [N * (d + 1), d + 1], bary [N, d + 1]) with framework ops."""
    d = positions.shape[1]
    greedy, rank, bary = _find_enclosing_simplex(_embed_lattice(positions))
    steps = _canonical_simplex_offsets(d, positions.device)[:, rank].permute(1, 0, 2)  # [N, vertex, axis]
    return (greedy.unsqueeze(1) + steps).reshape(-1, d + 1), bary


class PermutohedralLattice(lt.SparseLattice):
    """Build once, filter many times::

        lat = PermutohedralLattice.build(positions / sigma)   # (N, d), one lattice cell per sigma
        out = lat.filter(features)                            # (N, F)
        out = lat.filter(features, query_positions=q / sigma)

    Attributes as the reference's: ``unique_keys`` int32 (V, d + 1) in the row order of ``torch.unique(dim=0)``, ``inverse``
    int64 (N (d + 1),), ``bary`` (N, d + 1), ``d``, ``n_input``, ``hash_table`` (``None`` on the CPU, where lookups are a
    sorted search over the packed keys)."""

    def __init__(self, unique_keys: Tensor, inverse: Tensor, bary: Tensor, d: int, n_input: int, hash_table,
                 backend: str = "torch", rows: Optional[lt.RowLists] = None):
        self.unique_keys, self.inverse, self.bary = unique_keys, inverse, bary
        self.d, self.n_input, self.hash_table, self.backend = d, n_input, hash_table, backend
        self._entry_weights, self._rows = bary, rows
        self._alpha = 1.0 / (1.0 + 2.0 ** (-(d + 1)))

    @classmethod
    @torch.no_grad()
    def build(cls, positions: Tensor, backend: str = "auto") -> "PermutohedralLattice":
        """``positions`` (N, d), d <= 6, already divided by the bandwidth(s)."""
        lt.check_positions(positions)
        backend = lt.pick_backend(backend, positions)
        n, d = positions.shape
        if backend == "hip":
            return cls._build_hip(positions.detach().float().contiguous())
        keys, bary = _simplex_keys(positions.detach())
        if n and (int(keys.min()) < lt.COORD_MIN or int(keys.max()) > lt.COORD_MAX or not bool(torch.isfinite(bary).all())):
            raise lt.range_error("PermutohedralLattice.build")
        unique_keys, inverse = torch.unique(keys.to(torch.int32), dim=0, return_inverse=True)
        table = None
        if positions.is_cuda:
            table = PackedHashTable128.from_keys(unique_keys, capacity=max(16, 2 * unique_keys.shape[0]))
        return cls(unique_keys, inverse, bary, d, n, table, "torch")

    @staticmethod
    def _geometry_hip(positions: Tensor, key_words: bool, status: Tensor):
        n, d = positions.shape
        dev = positions.device
        hi = lo = keys = None
        if key_words:
            hi = torch.empty(n * (d + 1), dtype=torch.int64, device=dev)
            lo = torch.empty_like(hi)
        else:
            keys = torch.empty((n * (d + 1), d + 1), dtype=torch.int32, device=dev)
        bary = torch.empty((n, d + 1), dtype=torch.float32, device=dev)
        scale = (_lib.ctypes.c_float * 6)(*_embed_scale(d, torch.float32, "cpu").tolist())
        _lib.check(_lib.lib().wcn_permuto_simplex(_lib.ptr(positions), n, d, scale, _lib.ptr(hi), _lib.ptr(lo), _lib.ptr(keys),
                                                  _lib.ptr(bary), _lib.ptr(status), _lib.stream_handle(dev)),
                   "wcn_permuto_simplex")
        return hi, lo, keys, bary

    @classmethod
    def _build_hip(cls, positions: Tensor) -> "PermutohedralLattice":
        n, d = positions.shape
        status = torch.zeros(4, dtype=torch.int32, device=positions.device)
        hi, lo, _, bary = cls._geometry_hip(positions, True, status)
        built = lt.hip_vertex_map(hi, lo, d + 1, status)
        if built is None:
            raise lt.range_error("PermutohedralLattice.build")
        unique_keys, inverse, rows = built
        table = PackedHashTable128(max(16, 2 * unique_keys.shape[0]), positions.device, d + 1)
        table._launch_insert(unique_keys, status)  # keys decoded from in-range, distinct fields: no flag can be raised
        return cls(unique_keys, inverse, bary, d, n, table, "hip", rows)

    # -- what SparseLattice asks for -------------------------------------------------------------------------------------------
    def _neighbour_offsets(self) -> Tensor:
        d = self.d
        forward = torch.ones((d + 1, d + 1), dtype=torch.int32, device=self.unique_keys.device)
        forward.fill_diagonal_(-d)
        return torch.stack([forward, -forward], dim=1).reshape(2 * (d + 1), d + 1)

    def _default_passes(self) -> List[lt.Pass]:
        return [(2 * a, 2 * a + 1, 1.0, 0.5, 0.5) for a in range(self.d + 1)]

    def _query_geometry(self, query_positions: Tensor) -> Tuple[Tensor, Tensor]:
        if self.backend == "hip" and query_positions.is_cuda and query_positions.dtype in lt.HIP_DTYPES:
            status = torch.zeros(1, dtype=torch.int32, device=query_positions.device)  # a query outside the range is a miss
            _, _, keys, bary = self._geometry_hip(query_positions.detach().float().contiguous(), False, status)
            return keys, bary
        keys, bary = _simplex_keys(query_positions.detach())
        bary = torch.where(torch.isfinite(bary), bary, torch.zeros_like(bary))
        return keys.clamp(lt.COORD_MIN - 1, lt.COORD_MAX + 1).to(torch.int32), bary

    # -- the reference's pipeline ----------------------------------------------------------------------------------------------
    def filter(self, features: Tensor, query_positions: Optional[Tensor] = None, *, normalize: bool = True) -> Tensor:
        """splat -> blur -> slice; (N, F) -> (N, F), or (M, F) at ``query_positions`` (pre-scaled like the build positions).
        ``normalize`` carries a channel of ones along and divides by it (homogeneous coordinates, Adams section 4.4), which
        turns the accumulation into a Gaussian-weighted average.  Query simplices with no populated vertex give zeros.  A lattice built by the HIP back end runs the HIP kernels for
        float32 / float16 / bfloat16 features on its GPU; any other feature tensor (float64 in particular) silently takes the
        framework-op path over the same lattice arrays - correct, differentiable, and not the hot path."""
        return self._filter(features, query_positions, normalize)

    def _slice_at_query_positions(self, lattice: Tensor, query_positions: Tensor) -> Tensor:
        q = self._query_entries(query_positions)
        return self._slice(lattice, q.index, q.weights)


def _scaled(positions: Tensor, sigmas, sigma) -> Tensor:
    if sigmas is not None:
        return positions / torch.as_tensor(sigmas, dtype=positions.dtype, device=positions.device)
    return positions / sigma


def permutohedral_filter(positions: Tensor, features: Tensor, *, sigmas=None, sigma: Optional[float] = None,
                         query_positions: Optional[Tensor] = None, backend: str = "auto") -> Tensor:
    """One-shot Gaussian filter over ``positions`` (N, d) with per-axis ``sigmas`` or a scalar ``sigma``."""
    if sigmas is None and sigma is None:
        raise ValueError("Pass either sigmas (per-axis) or sigma (scalar).")
    lattice = PermutohedralLattice.build(_scaled(positions, sigmas, sigma), backend=backend)
    queries = None if query_positions is None else _scaled(query_positions, sigmas, sigma)
    return lattice.filter(features, query_positions=queries)


def bilateral_positions(xyz: Tensor, feat: Tensor, sigma_xyz: float, sigma_feat: float) -> Tensor:
    """Lattice positions of a bilateral filter: space and range features, each divided by its bandwidth."""
    if xyz.shape[1] + feat.shape[1] > lt.MAX_AXES:
        raise ValueError(f"D_xyz + D_feat = {xyz.shape[1] + feat.shape[1]} > {lt.MAX_AXES}; the keys of PackedHashTable128 hold "
                         f"at most {lt.MAX_AXES + 1} axes.")
    if xyz.shape[0] != feat.shape[0]:
        raise ValueError(f"xyz has {xyz.shape[0]} rows, feat {feat.shape[0]}")
    return torch.cat([xyz / sigma_xyz, feat / sigma_feat], dim=-1)


def bilateral_query_positions(query_xyz, query_feat, sigma_xyz: float, sigma_feat: float) -> Optional[Tensor]:
    if query_xyz is None and query_feat is None:
        return None
    if query_xyz is None or query_feat is None:
        raise ValueError("Pass both query_xyz and query_feat, or neither.")
    return bilateral_positions(query_xyz, query_feat, sigma_xyz, sigma_feat)


def bilateral_permutohedral_filter(src_xyz: Tensor, src_feat: Tensor, src_value: Tensor, *, sigma_xyz: float = 0.05,
                                   sigma_feat: float = 20.0, query_xyz: Optional[Tensor] = None,
                                   query_feat: Optional[Tensor] = None, normalize: bool = True,
                                   backend: str = "auto") -> Tensor:
    """Bilateral filter of ``src_value`` (N, V): the lattice positions are ``[xyz / sigma_xyz, feat / sigma_feat]``, so the
    range features (for instance RGB) keep edges.  D_xyz + D_feat <= 6."""
    if src_value.shape[0] != src_xyz.shape[0]:
        raise ValueError(f"src_value has {src_value.shape[0]} rows, src_xyz {src_xyz.shape[0]}")
    lattice = PermutohedralLattice.build(bilateral_positions(src_xyz, src_feat, sigma_xyz, sigma_feat), backend=backend)
    queries = bilateral_query_positions(query_xyz, query_feat, sigma_xyz, sigma_feat)
    return lattice.filter(src_value, query_positions=queries, normalize=normalize)
