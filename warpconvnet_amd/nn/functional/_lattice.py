"""What the permutohedral lattice and the bilateral grid share: a sparse set of integer vertices, ``K`` weighted entries per
point, and splat -> blur -> slice over them.

Two back ends.  ``"torch"`` is the reference's algorithm as framework ops on any device and dtype (the CPU path, the float64
path and the tests' operator oracle).  ``"hip"`` runs the kernels of ``csrc/lattice.hip``: fp32 rows padded to a multiple of
four floats, a fixed-order CSR splat without float atomics, a neighbour table built once per lattice, and one
``autograd.Function`` over the three steps whose backward reuses the same kernels (transposed slice = splat over the slicing
entries, transposed splat = slice, transposed blur = the passes in reverse with the neighbour directions swapped).

The gradient goes to the features only: the lattice is built without grad.  The reference, all framework ops, would also
differentiate the barycentric weights with respect to the positions; that is not offered here.
"""
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from warpconvnet_amd import _lib
from warpconvnet_amd.geometry.coords.search.packed128_hashmap import PackedHashTable128

HIP_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
COORD_BITS = PackedHashTable128.COORD_BITS
COORD_MIN, COORD_MAX = PackedHashTable128.COORD_MIN, PackedHashTable128.COORD_MAX
MAX_AXES = PackedHashTable128.DIM - 1  # position dimensions either lattice takes
_INT64_MIN = torch.iinfo(torch.int64).min

# one blur pass: y = s0 * x + s1 * x[table[t1]] + s2 * x[table[t2]] (t2 = -1: no third term); tables are rows of `neighbours`
Pass = Tuple[int, int, float, float, float]


def pick_backend(backend: str, positions: Tensor) -> str:
    if backend not in ("auto", "torch", "hip"):
        raise ValueError(f"backend must be 'auto', 'torch' or 'hip'; got {backend!r}")
    if backend == "auto":
        return "hip" if positions.is_cuda and positions.dtype in HIP_DTYPES else "torch"
    if backend == "hip" and not positions.is_cuda:
        raise RuntimeError("backend='hip' needs positions on a GPU; there is no CPU fallback for the HIP path")
    return backend


def check_positions(positions: Tensor) -> None:
    if positions.dim() != 2:
        raise ValueError(f"positions must be (N, d); got {tuple(positions.shape)}")
    if not (1 <= positions.shape[1] <= MAX_AXES):
        raise ValueError(f"d = {positions.shape[1]} is outside [1, {MAX_AXES}] (keys hold at most {MAX_AXES + 1} axes)")


def range_error(what: str) -> ValueError:
    return ValueError(f"{what}: a lattice coordinate is outside [{COORD_MIN}, {COORD_MAX}] (or a position is not finite); "
                      "positions must already be divided by the bandwidth")


# ---- packed keys: the order and the search of the torch back end -----------------------------------------------------------------
def pack_keys(keys: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """int rows [M, key_dim] -> (hi, lo, in_range): 17-bit fields biased by 2^16, axis 0 most significant, the top bit of lo
    flipped, so the signed order of (hi, lo) is the lexicographic order of the rows."""
    b = keys.to(torch.int64) - COORD_MIN
    ok = ((b >= 0) & (b <= COORD_MAX - COORD_MIN)).all(dim=1)
    b = b.clamp(0, COORD_MAX - COORD_MIN)
    hi = torch.zeros(keys.shape[0], dtype=torch.int64, device=keys.device)
    lo = torch.zeros_like(hi)
    field = (1 << COORD_BITS) - 1
    for j in range(keys.shape[1]):
        hi = (hi << COORD_BITS) | ((lo >> (64 - COORD_BITS)) & field)
        lo = (lo << COORD_BITS) | b[:, j]
    return hi, lo ^ _INT64_MIN, ok


def sorted_search(table_keys: Tensor, queries: Tensor) -> Tensor:
    """Row of every query in ``table_keys`` (distinct rows in lexicographic order, as ``torch.unique(dim=0)`` leaves them) or
    -1: a bisection over the packed keys, int64 [M]."""
    V, M = table_keys.shape[0], queries.shape[0]
    if V == 0 or M == 0:
        return torch.full((M,), -1, dtype=torch.int64, device=queries.device)
    th, tl, _ = pack_keys(table_keys)
    qh, ql, ok = pack_keys(queries)
    left = torch.zeros(M, dtype=torch.int64, device=queries.device)
    right = torch.full_like(left, V)
    for _ in range(V.bit_length() + 1):
        mid = ((left + right) >> 1).clamp_max(V - 1)
        below = (th[mid] < qh) | ((th[mid] == qh) & (tl[mid] < ql))
        active = left < right
        left = torch.where(active & below, mid + 1, left)
        right = torch.where(active & ~below, mid, right)
    at = left.clamp_max(V - 1)
    hit = ok & (left < V) & (th[at] == qh) & (tl[at] == ql)
    return torch.where(hit, at, torch.full_like(at, -1))


# ---- framework ops: the torch back end and the operator oracle -------------------------------------------------------------------
def rows_or_zero(x: Tensor, index: Tensor) -> Tensor:
    """``x[index]`` with -1 reading as a zero row."""
    return x[index.clamp_min(0)] * (index >= 0).to(x.dtype).unsqueeze(-1)


def torch_splat(features: Tensor, weights: Tensor, inverse: Tensor, num_vertices: int) -> Tensor:
    n, k = weights.shape
    contrib = (weights.to(features.dtype).unsqueeze(-1) * features.unsqueeze(1)).reshape(n * k, features.shape[1])
    out = torch.zeros((num_vertices, features.shape[1]), dtype=features.dtype, device=features.device)
    return out.index_add_(0, inverse, contrib)


def torch_blur(x: Tensor, neighbours: Tensor, passes: Sequence[Pass]) -> Tensor:
    for t1, t2, s0, s1, s2 in passes:
        y = s0 * x + s1 * rows_or_zero(x, neighbours[t1].long())
        x = y + s2 * rows_or_zero(x, neighbours[t2].long()) if t2 >= 0 else y
    return x


def torch_slice(x: Tensor, index: Tensor, weights: Tensor, alpha: float) -> Tensor:
    m, k = weights.shape
    picked = rows_or_zero(x, index).reshape(m, k, x.shape[1])
    return (weights.to(x.dtype).unsqueeze(-1) * picked).sum(dim=1) * alpha


def transposed(passes: Sequence[Pass]) -> List[Pass]:
    """The passes of the transposed blur: reverse order, every table replaced by the one of the opposite direction (rows 2a and
    2a + 1 of the neighbour table: u is the forward neighbour of v exactly when v is the backward neighbour of u)."""
    flip = lambda t: t ^ 1 if t >= 0 else t  # noqa: E731
    return [(flip(t1), flip(t2), s0, s1, s2) for t1, t2, s0, s1, s2 in reversed(list(passes))]


# ---- HIP wrappers ------------------------------------------------------------------------------------------------------------------
def pitch_of(channels: int) -> int:
    """Row pitch in floats: the channel count rounded up to four, so every row access is made of 16-byte pieces."""
    return max(4, (channels + 3) // 4 * 4)


def pad_rows(x: Tensor, pitch: int) -> Tensor:
    """fp32 [rows, pitch] copy of ``x`` with zero padding columns."""
    out = torch.zeros((x.shape[0], pitch), dtype=torch.float32, device=x.device)
    out[:, : x.shape[1]] = x
    return out


class RowLists:
    """A CSR by vertex over weighted entries, with the chunk plan of its long rows (``None``: no row is longer than a chunk)."""

    def __init__(self, row_offsets: Tensor, row_entries: Tensor, num_rows: int, longest: int):
        self.row_offsets, self.row_entries, self.num_rows = row_offsets, row_entries, num_rows
        self.nnz = row_entries.shape[0]
        self.plan = None
        L = _lib.lib()
        if self.nnz > 0 and num_rows > 0 and (longest < 0 or longest > L.wcn_lattice_chunk_rows()):  # < 0: not known
            self.plan = torch.empty(L.wcn_lattice_plan_ints(self.nnz), dtype=torch.int32, device=row_entries.device)
            _lib.check(L.wcn_lattice_plan(_lib.ptr(row_offsets), num_rows, self.nnz, _lib.ptr(self.plan),
                                          _lib.stream_handle(row_entries.device)), "wcn_lattice_plan")


def hip_splat(f: Tensor, weights: Tensor, rows: RowLists, k: int, alpha: float) -> Tensor:
    """[V, pitch] = alpha * sum over the entries e of each row of weights[e] * f[e // k]; ``f`` fp32 [*, pitch]."""
    L = _lib.lib()
    pitch = f.shape[1]
    out = torch.empty((rows.num_rows, pitch), dtype=torch.float32, device=f.device)
    partials = None
    if rows.plan is not None:
        partials = torch.empty((L.wcn_lattice_plan_items(rows.nnz), pitch), dtype=torch.float32, device=f.device)
    _lib.check(L.wcn_lattice_splat(_lib.ptr(f), _lib.ptr(weights), _lib.ptr(rows.row_offsets), _lib.ptr(rows.row_entries),
                                   rows.num_rows, rows.nnz, k, pitch, alpha, _lib.ptr(rows.plan), _lib.ptr(partials),
                                   _lib.ptr(out), _lib.stream_handle(f.device)), "wcn_lattice_splat")
    return out


def hip_blur(x: Tensor, neighbours: Tensor, passes: Sequence[Pass]) -> Tensor:
    """The passes over two ping-pong buffers; ``x`` itself is never written."""
    if x.shape[0] == 0 or not passes:
        return x
    L = _lib.lib()
    stream = _lib.stream_handle(x.device)
    spare = [torch.empty_like(x), torch.empty_like(x) if len(passes) > 1 else None]
    for i, (t1, t2, s0, s1, s2) in enumerate(passes):
        y = spare[i & 1]
        _lib.check(L.wcn_lattice_blur(_lib.ptr(x), _lib.ptr(neighbours[t1]), _lib.ptr(neighbours[t2]) if t2 >= 0 else None,
                                      s0, s1, s2, x.shape[0], x.shape[1], _lib.ptr(y), stream), "wcn_lattice_blur")
        x = y
    return x


def hip_slice(x: Tensor, index: Tensor, weights: Tensor, alpha: float) -> Tensor:
    L = _lib.lib()
    n, k = weights.shape
    out = torch.empty((n, x.shape[1]), dtype=torch.float32, device=x.device)
    _lib.check(L.wcn_lattice_slice(_lib.ptr(x), _lib.ptr(index), _lib.ptr(weights), n, k, x.shape[0], x.shape[1], alpha,
                                   _lib.ptr(out), _lib.stream_handle(x.device)), "wcn_lattice_slice")
    return out


def hip_vertex_map(key_hi: Tensor, key_lo: Tensor, key_dim: int, status: Tensor):
    """Entry keys -> (unique_keys, inverse, RowLists): stable sort of lo then hi (framework radix sort; the hi pass is needless
    when the key fits 64 bits), then the run-head / scan / apply kernels.  ``status`` int32 [4]: word 0 carries the flags of the
    geometry kernel, words 2..3 receive (V, longest row); reading it is the build's single host read."""
    L = _lib.lib()
    dev = key_lo.device
    nnz = key_lo.shape[0]
    lo_sorted, perm = torch.sort(key_lo, stable=True)
    hi_sorted = None
    if key_dim * COORD_BITS > 64:
        hi_sorted, second = torch.sort(key_hi[perm], stable=True)
        perm, lo_sorted = perm[second], lo_sorted[second]
    unique_keys = torch.empty((nnz, key_dim), dtype=torch.int32, device=dev)
    inverse = torch.empty(nnz, dtype=torch.int64, device=dev)
    row_offsets = torch.empty(nnz + 1, dtype=torch.int64, device=dev)
    ws_bytes = L.wcn_lattice_map_workspace_bytes(nnz)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(L.wcn_lattice_map(_lib.ptr(hi_sorted), _lib.ptr(lo_sorted), _lib.ptr(perm), nnz, key_dim, _lib.ptr(unique_keys),
                                 _lib.ptr(inverse), _lib.ptr(row_offsets), _lib.ptr(status[2:]), _lib.ptr(ws), ws_bytes,
                                 _lib.stream_handle(dev)), "wcn_lattice_map")
    flags, _, num_vertices, longest = status.tolist()  # the single host read
    if flags & _lib.WCN_FLAG_COORD_RANGE:
        return None
    rows = RowLists(row_offsets[: num_vertices + 1].clone(), perm, num_vertices, longest)
    return unique_keys[:num_vertices].clone(), inverse, rows


class QueryEntries:
    """The slicing entries of a set of query points: vertex per entry (-1 = absent) and weights.  The CSR by vertex that the
    backward's splat needs is built by one stable sort the first time a backward asks for it."""

    def __init__(self, index: Tensor, weights: Tensor, num_vertices: int):
        self.index, self.weights, self.num_vertices = index, weights, num_vertices
        self._rows: Optional[RowLists] = None

    def rows(self) -> RowLists:
        if self._rows is None:
            ordered, perm = torch.sort(self.index, stable=True)
            bounds = torch.arange(self.num_vertices + 1, dtype=torch.int64, device=self.index.device)
            self._rows = RowLists(torch.searchsorted(ordered, bounds), perm, self.num_vertices, -1)
        return self._rows


class _LatticeFilterFunction(torch.autograd.Function):
    """splat -> blur -> slice on fp32 rows of one pitch; the gradient goes to the features."""

    @staticmethod
    def forward(ctx, f: Tensor, lattice: "SparseLattice", passes: Sequence[Pass], query: Optional[QueryEntries]) -> Tensor:
        x = hip_splat(f, lattice._entry_weights, lattice._rows, lattice._k, 1.0)
        x = hip_blur(x, lattice.neighbours, passes)
        ctx.lattice, ctx.passes, ctx.query = lattice, passes, query
        if query is None:
            return hip_slice(x, lattice.inverse, lattice._entry_weights, lattice._alpha)
        return hip_slice(x, query.index, query.weights, lattice._alpha)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g: Tensor):
        lattice, query = ctx.lattice, ctx.query
        g = g.contiguous()
        if query is None:
            x = hip_splat(g, lattice._entry_weights, lattice._rows, lattice._k, lattice._alpha)
        else:
            x = hip_splat(g, query.weights, query.rows(), lattice._k, lattice._alpha)
        x = hip_blur(x, lattice.neighbours, transposed(ctx.passes))
        return hip_slice(x, lattice.inverse, lattice._entry_weights, 1.0), None, None, None


class SparseLattice:
    """Base of ``PermutohedralLattice`` and ``BilateralGrid``.  A subclass sets ``unique_keys`` int32 [V, key_dim], ``inverse``
    int64 [N * K], ``_entry_weights`` [N, K], ``d``, ``n_input``, ``hash_table``, ``backend`` (and ``_rows`` on the HIP back
    end) and provides ``_neighbour_offsets``, ``_default_passes``, ``_query_geometry`` and ``_alpha``."""

    _alpha = 1.0
    _neighbours: Optional[Tensor] = None
    _rows: Optional[RowLists] = None

    # -- what a subclass provides ----------------------------------------------------------------------------------------------
    def _neighbour_offsets(self) -> Tensor:
        raise NotImplementedError

    def _default_passes(self) -> List[Pass]:
        raise NotImplementedError

    def _query_geometry(self, query_positions: Tensor) -> Tuple[Tensor, Tensor]:
        """(keys int32 [M * K, key_dim], weights [M, K]) of the query points."""
        raise NotImplementedError

    # -- shared ----------------------------------------------------------------------------------------------------------------
    @property
    def _k(self) -> int:
        return self._entry_weights.shape[1]

    @property
    def num_vertices(self) -> int:
        return int(self.unique_keys.shape[0])

    def _lookup(self, keys: Tensor) -> Tensor:
        """int64 [M]: vertex of every key row, -1 when absent."""
        if self.hash_table is not None:
            return self.hash_table.search(keys).long()
        return sorted_search(self.unique_keys, keys)

    @property
    def neighbours(self) -> Tensor:
        """int32 [2 * axes, V]: rows 2a / 2a + 1 = the vertex one step forward / backward along axis a, -1 when absent.  Built
        once per lattice; ``filter`` never searches again."""
        if self._neighbours is None:
            offsets = self._neighbour_offsets()
            if self.hash_table is not None:
                self._neighbours = self.hash_table.batched_search(self.unique_keys, offsets)
            else:
                keys = self.unique_keys.unsqueeze(0) + offsets.unsqueeze(1)  # [2 axes, V, key_dim]
                found = sorted_search(self.unique_keys, keys.reshape(-1, keys.shape[-1]))
                self._neighbours = found.reshape(offsets.shape[0], -1).to(torch.int32)
        return self._neighbours

    def _use_hip(self, t: Tensor) -> bool:
        return self.backend == "hip" and t.is_cuda and t.dtype in HIP_DTYPES

    def _forward_only(self, t: Tensor, what: str) -> None:
        if t.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError(f"{what} on the HIP back end is forward-only; differentiate filter(), which has one "
                                      "autograd.Function over splat -> blur -> slice, or build with backend='torch'")

    def _splat(self, features: Tensor) -> Tensor:
        """(N, F) -> (V, F)."""
        if features.dim() != 2 or features.shape[0] != self.n_input:
            raise ValueError(f"features must be ({self.n_input}, F); got {tuple(features.shape)}")
        if not self._use_hip(features):
            return torch_splat(features, self._entry_weights, self.inverse, self.num_vertices)
        self._forward_only(features, "splat")
        c = features.shape[1]
        out = hip_splat(pad_rows(features, pitch_of(c)), self._entry_weights, self._rows, self._k, 1.0)
        return out[:, :c].to(features.dtype)

    def _blur(self, lattice: Tensor, passes: Optional[Sequence[Pass]] = None) -> Tensor:
        """(V, F) -> (V, F): the separable three-tap blur, one axis after the other."""
        passes = self._default_passes() if passes is None else passes
        if not self._use_hip(lattice):
            return torch_blur(lattice, self.neighbours, passes)
        self._forward_only(lattice, "blur")
        c = lattice.shape[1]
        return hip_blur(pad_rows(lattice, pitch_of(c)), self.neighbours, passes)[:, :c].to(lattice.dtype)

    def _slice(self, lattice: Tensor, index: Optional[Tensor] = None, weights: Optional[Tensor] = None) -> Tensor:
        """(V, F) -> (M, F) at the build positions, or at the given entries."""
        index = self.inverse if index is None else index
        weights = self._entry_weights if weights is None else weights
        if not self._use_hip(lattice):
            return torch_slice(lattice, index, weights, self._alpha)
        self._forward_only(lattice, "slice")
        c = lattice.shape[1]
        out = hip_slice(pad_rows(lattice, pitch_of(c)), index.contiguous(), weights.float().contiguous(), self._alpha)
        return out[:, :c].to(lattice.dtype)

    def _query_entries(self, query_positions: Tensor) -> QueryEntries:
        if query_positions.dim() != 2 or query_positions.shape[1] != self.d:
            raise ValueError(f"query_positions must be (M, {self.d}); got {tuple(query_positions.shape)}")
        with torch.no_grad():
            keys, weights = self._query_geometry(query_positions)
            return QueryEntries(self._lookup(keys), weights, self.num_vertices)

    def _filter(self, features: Tensor, query_positions: Optional[Tensor], normalize: bool,
                passes: Optional[Sequence[Pass]] = None) -> Tensor:
        if features.dim() != 2 or features.shape[0] != self.n_input:
            raise ValueError(f"features must be ({self.n_input}, F); got {tuple(features.shape)}")
        passes = self._default_passes() if passes is None else passes
        query = None if query_positions is None else self._query_entries(query_positions)
        n, c = features.shape[0], features.shape[1] + (1 if normalize else 0)
        if self._use_hip(features):
            f = torch.zeros((n, pitch_of(c)), dtype=torch.float32, device=features.device)
            f[:, : features.shape[1]] = features
            if normalize:
                f[:, c - 1] = 1.0
            out = _LatticeFilterFunction.apply(f, self, passes, query)[:, :c]
        else:
            f = features
            if normalize:
                f = torch.cat([features, torch.ones((n, 1), dtype=features.dtype, device=features.device)], dim=-1)
            x = torch_blur(torch_splat(f, self._entry_weights, self.inverse, self.num_vertices), self.neighbours, passes)
            if query is None:
                out = torch_slice(x, self.inverse, self._entry_weights, self._alpha)
            else:
                out = torch_slice(x, query.index, query.weights, self._alpha)
        if normalize:  # the homogeneous-channel division stays in the framework
            out = out[:, :-1] / out[:, -1:].clamp_min(1e-20)
        return out.to(features.dtype)
